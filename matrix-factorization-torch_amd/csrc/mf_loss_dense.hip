// mf_loss_dense.hip -- the dense (unmined) path of the losses: the forward sweep over score tiles with per-row statistics,
// the dU and dV sweeps of the backward (recompute-free contractions of the stashed logits) and their split sums, and the
// launches and the switch of the distinct-column plan (mf_loss_cols.h).  mf_loss_ws.h lists the units and what they share.
#include <cfloat>
#include <mutex>
#include <type_traits>
#include <unordered_map>

#include "mf_loss_ws.h"

// ---------------------------------------------------------- dense forward ------
struct FwdParams {
    const float *u, *v, *nu, *nv, *lii, *sgn, *logq;
    const uint32_t* maskW;
    float* part;
    float* stash;          // [Bp/32][NT] blocks of 32 x 32 logits (see BwdParams)
    int64_t B, N, Bp;
    int NT, tps, need;
    float sigma, margin;
    // side inputs of a tile as ONE buffer: byte offsets of maskW / nv / logq from aux_base, and the span covered
    const char* aux_base;
    uint32_t aux_mask, aux_nv, aux_lq, aux_bytes;
    // distinct-column sweep (CP): v, nv, logq, maskW are the packed arrays, N their padded height; the tile range comes from
    // the device words, the column weights ride in lanes 24..31 of the side-input DMA
    const int32_t* geo;
    uint32_t aux_w;
    // split scores (SPLIT): the bf16 piece image of the streamed item tiles (fsi_index, mf_bf_split.h), NT tiles
    const unsigned short* img;
};

// The side inputs -- fp's mask words, norms and -logQ, and the column weights `cw` of a distinct-column sweep -- live in
// the workspace: ONE descriptor over their span (lowest to highest address), the four byte offsets into it.  false: the
// span, or a split's share of the streamed operand, is more than a buffer descriptor covers (4 GiB).
static bool fwd_aux_span(FwdParams& fp, const LossWs& w, const float* cw) {
    const char *pm = (const char*)fp.maskW, *pn = (const char*)fp.nv, *pl = (const char*)fp.logq;
    const char* lo = pm < pn ? (pm < pl ? pm : pl) : (pn < pl ? pn : pl);
    const char *em = pm + (size_t)w.NT * w.Bp * 4, *en = pn + (size_t)w.NT * 128, *el = pl + (size_t)w.NT * 128;
    const char* hi = em > en ? (em > el ? em : el) : (en > el ? en : el);
    if (cw) {
        const char* pw = (const char*)cw;
        if (pw < lo) lo = pw;
        if (pw + (size_t)w.NT * 128 > hi) hi = pw + (size_t)w.NT * 128;
        fp.aux_w = (uint32_t)(pw - lo);
    }
    if ((size_t)(hi - lo) > MF_SRD_MAX_BYTES || (size_t)w.tps_f * 32 * w.d * 4 > MF_SRD_MAX_BYTES) return false;
    fp.aux_base = lo; fp.aux_mask = (uint32_t)(pm - lo); fp.aux_nv = (uint32_t)(pn - lo); fp.aux_lq = (uint32_t)(pl - lo);
    fp.aux_bytes = (uint32_t)(hi - lo);
    return true;
}

// Workgroup = 4 waves x 32 users; item tiles arrive through a 2-slot LDS ring filled by LDS-DMA, together with
// their mask words, norms and -logQ (a separate 4-deep ring of side-input slots).  The loop is software-pipelined
// inside each wave: the 64 MFMAs of tile t+1 are issued in the same basic block as the (branch-free) statistics of
// tile t, and the DMA pieces of tile t+2 -- into the slot tile t just left -- go out one per MFMA group, so the
// matrix pipe, the VALU and the memory instructions overlap without relying on a second wave.  The tile loop is
// unrolled by the two slots: every LDS address is lane base + immediate, and the two accumulator sets swap roles
// by name (no register copies at the loop edge).
// SPLIT (d = 128): the score tile on the bf16 matrix cores, fp32-grade (mf_bf_split.h).  The item tile arrives as its image of
// three bf16 pieces (fwd_split_image_kernel: 24 KiB per tile, six 1-KiB DMA pieces per wave), the user fragment is split in
// registers once per workgroup, and a tile's scores are 8 k-steps x 6 piece products into the same fp32 accumulators: 48 MFMAs
// of 8 passes instead of 64 of 16.  An MFMA group is then a k-step; the statistics go four slices to a group and the stage's
// seven memory instructions DPG = 3 to a group, so that the last of them is issued in group 2 of 8 and has most of a tile's
// matrix time to land.
template <int D, bool SPLIT = false>
struct FwdLds {
    using G = TileGeom<D>;
    static_assert(!SPLIT || D == 128, "the split forward is written for d = 128");
    // side inputs: one 1-KiB DMA per wave and tile -- lanes 0..7 the wave's 32 mask words, 8..15 the tile's item
    // norms, 16..23 its -logq (every wave keeps its own copy: no cross-wave dependency), the other lanes zeros
    static constexpr int AUX_NV = 128, AUX_LQ = 256, AUX_CW = 384, AUXW = 1024, AUXB = G::NW * AUXW;
    static constexpr int SLOTB = SPLIT ? FSI_TILEB : G::TILEB;   // bytes of a tile slot
    static constexpr int AUX0 = 2 * SLOTB;              // 4 side-input slots after the 2 tile slots
    static constexpr int BYTES = AUX0 + 4 * AUXB;
    static constexpr int NG = SPLIT ? 8 : D / 8;        // MFMA groups per tile (SPLIT: the k-steps, six MFMAs each)
    static constexpr int PPW = SPLIT ? FSI_TILEB / G::NW / 1024 : G::PPW;   // 1-KiB DMA pieces of a tile per wave
    static constexpr int NDMA = PPW + 1;                // memory instructions of a stage: the tile pieces, then the side inputs
    static constexpr int DPG = SPLIT ? 3 : 1;           // of them per MFMA group
    static constexpr int LASTG = (NDMA - 1) / DPG;      // group of a stage's last DMA
    // stash stores of a tile (issued behind logit slices 3, 7, 11, 15 of 32) that are YOUNGER than the stage's last
    // DMA: `s_waitcnt vmcnt(KEEP)` at the next tile's top then proves every DMA of the stage has landed
    // (a group issues its DMA before its slices, so a store of group LASTG itself is already younger; SPLIT counts only
    // the stores of LATER groups -- it waits for one store more than it must and needs no order inside a group)
    static constexpr int store_group(int s) { return s * NG / 32; }
    static constexpr bool younger(int s) { return SPLIT ? store_group(s) > LASTG : store_group(s) >= LASTG; }
    static constexpr int KEEP = younger(3) + younger(7) + younger(11) + younger(15);
    static_assert(LASTG < NG, "a stage's DMAs must fit the tile's MFMA groups");
    static_assert(SPLIT || (LASTG == G::PPW && NDMA == LASTG + 1), "fp32 scores: one DMA per group, the side inputs last");
    static_assert(!SPLIT || (PPW == 6 && LASTG == 2 && KEEP == 1 && BYTES == 64 * 1024), "split scores: 7 DMAs in groups 0..2, the store of group 3 is younger");
};

template <int NEED>
__device__ __forceinline__ void stats_add_masked(RowStats& s, float Lm, float sm, float lii, float margin) {
    // Lm is -inf for masked elements: every term below is then exactly 0 (the count is kept separately)
    if (NEED & NEED_CONTR) s.A += fmaxf(Lm + sm, 0.f);
    if (NEED & (NEED_HINGE | NEED_LOGI)) {
        const float x = (Lm - lii) + margin;
        if (NEED & NEED_HINGE) {
            s.H += fmaxf(x, 0.f);
            s.Hc += x > 0.f ? 1.f : 0.f;
        }
        if (NEED & NEED_LOGI) {
            float sp, sg;
            softplus_sigmoid(x, sp, sg);
            s.Lg += sp;
            s.Ls += sg;
        }
    }
}
// the same with a column weight (the copies of a distinct column): every summed term times cw (a masked term is 0 x cw = 0)
template <int NEED>
__device__ __forceinline__ void stats_add_masked_w(RowStats& s, float Lm, float sm, float lii, float margin, float cw) {
    if (NEED & NEED_CONTR) s.A = __builtin_fmaf(cw, fmaxf(Lm + sm, 0.f), s.A);
    if (NEED & (NEED_HINGE | NEED_LOGI)) {
        const float x = (Lm - lii) + margin;
        if (NEED & NEED_HINGE) {
            s.H = __builtin_fmaf(cw, fmaxf(x, 0.f), s.H);
            s.Hc += x > 0.f ? cw : 0.f;
        }
        if (NEED & NEED_LOGI) {
            float sp, sg;
            softplus_sigmoid(x, sp, sg);
            s.Lg = __builtin_fmaf(cw, sp, s.Lg);
            s.Ls = __builtin_fmaf(cw, sg, s.Ls);
        }
    }
}

// The user row of lane (c, h) as the B fragments of the split score tile: x[s][q] is piece q of features 16 s + 8 h .. + 7
// (the order the image keeps the item rows in, fsi_index); rows past the end are zeros, as in mf_load_frag.
struct RowFragSplit {
    mbf16x8 x[8][3];
};
__device__ __forceinline__ void mf_load_frag_split(RowFragSplit& f, const float* __restrict__ base, int64_t row, bool valid) {
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
    const int h = mf_lane() >> 5;
    const f32x4* p = reinterpret_cast<const f32x4*>(base + (valid ? row : 0) * 128 + 8 * h);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const f32x4 lo = p[4 * s], hi = p[4 * s + 1];
        u16x8 g3[3];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            unsigned short o[3];
            mbf_split3(valid ? (j < 4 ? lo[j] : hi[j - 4]) : 0.f, o);
            g3[0][j] = o[0]; g3[1][j] = o[1]; g3[2][j] = o[2];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) f.x[s][q] = __builtin_bit_cast(mbf16x8, g3[q]);
    }
}

#ifndef FWD_SPLIT_DROP
#define FWD_SPLIT_DROP -1     // A/B knob (wrong results): leave out piece product 0..5 -- the build the precision test must fail on
#endif
// The split score tile of the staged image with the previous tile's VALU work between the MFMAs, as
// mf_tile_scores_interleaved (mf_stream.h) does for the fp32 tile: a group is one k-step -- its three A fragments are read
// one k-step ahead, `hook(g)` issues the group's memory instructions, then the six piece products a_i x_j, i + j <= 2, the
// smallest first, and the group's share of the slices; VPM VALU / SALU instructions are placed behind each MFMA.
template <int NSLICE, int VPM, class Slice, class Hook>
__device__ __forceinline__ f32x16 mf_tile_scores_split_interleaved(const char* lds_tile, const RowFragSplit& x, Slice&& slice, Hook&& hook) {
    constexpr int NG = 8;
    static_assert(NSLICE % NG == 0, "slices and k-steps must nest");
    const mbf16x8* img = reinterpret_cast<const mbf16x8*>(lds_tile) + mf_lane();
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    mbf16x8 a_next[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) a_next[q] = img[(q * 8) * 64];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        mbf16x8 a[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) a[q] = a_next[q];
        if (g + 1 < NG) {
#pragma unroll
            for (int q = 0; q < 3; ++q) a_next[q] = img[(q * 8 + g + 1) * 64];
        }
        hook(g);
#pragma unroll
        for (int pr = 0; pr < 6; ++pr) {
            // (a piece, x piece): (2,0) (1,1) (0,2) | (1,0) (0,1) | (0,0)
            const int ai = pr == 0 ? 2 : (pr == 1 || pr == 3) ? 1 : 0;
            const int xi = pr == 2 ? 2 : (pr == 1 || pr == 4) ? 1 : 0;
            if (pr == FWD_SPLIT_DROP) continue;
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ai], x.x[g][xi], acc, 0, 0, 0);
        }
#pragma unroll
        for (int sidx = g * NSLICE / NG; sidx < (g + 1) * NSLICE / NG; ++sidx) slice(sidx);
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x006, VPM, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    return acc;
}

#ifndef FWD_SPLIT_VPM
#define FWD_SPLIT_VPM 14      // A/B knob: VALU / SALU instructions of the previous tile's statistics behind each MFMA of the split score tile
#endif
template <int D, int NEED, bool CP, bool SPLIT>
__global__ __launch_bounds__(64 * mf_nw(D), mf_wg_per_cu(D)) void loss_fwd_dense_kernel(FwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using G = TileGeom<D>;
    using L = FwdLds<D, SPLIT>;
    const int lane = mf_lane(), c = lane & 31, h = lane >> 5;
    const int wave = mf_wave_id();
    // grid = (item-range split, user block): consecutive workgroup ids -- dealt round-robin to the 8 XCDs --
    // differ in the SPLIT, so the workgroups of one XCD stream the same 1/nsplit of V through its L2
    const int64_t i0 = (int64_t)blockIdx.y * G::XB;
    const int64_t i = i0 + wave * 32 + c;
    // CP: the tile range of N' distinct columns (device words); a workgroup beyond it writes the empty statistics
    const int nt_e = CP ? p.geo[CG_NT] : p.NT, tps_e = CP ? p.geo[CG_TPSF] : p.tps;
    const int t0 = blockIdx.x * tps_e, t1 = min(nt_e, t0 + tps_e);
    RowFrag<D> xf;
    RowFragSplit xs;
    if constexpr (SPLIT) mf_load_frag_split(xs, p.u, i, i < p.B);
    else mf_load_frag<D>(xf, p.u, i, i < p.B);
    const float nu_i = p.nu[i], s_i = p.sgn[i], lii = p.lii[i];
    const float sm = s_i * p.margin;
    RowStats st;
    stats_init(st);

    TileSrc<D> tsrc;
    if constexpr (!SPLIT) mf_tile_src_init<D>(tsrc, p.v, p.N, (int64_t)t0 * 32);
    // SPLIT: the image is copied linearly -- one descriptor over its tiles [t0, nt_e) (the image kernel wrote exactly those of
    // the streamed range), piece j of this wave's share at lane offset + scalar ((t - t0) tiles + j KiB)
    mf_rsrc_t irsrc;
    const unsigned ioff = (unsigned)(wave * L::PPW * 1024 + lane * 16);
    if constexpr (SPLIT) {
        int64_t bytes = (int64_t)(nt_e - t0) * FSI_TILEB;
        bytes = bytes < 0 ? 0 : (bytes > (int64_t)MF_SRD_MAX_BYTES ? (int64_t)MF_SRD_MAX_BYTES : bytes);
#if defined(__HIP_DEVICE_COMPILE__)
        irsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(p.img + (int64_t)t0 * FSI_TILE_ELEMS), 0, (int)(unsigned)bytes, 0x00020000);
#else
        (void)irsrc; (void)ioff;
#endif
    }
    // side inputs: per-lane byte offset into the aux buffer, advanced by a per-lane stride from stage to stage
    // (stages are issued in tile order t0, t0 + 1, ...); lanes 24.. stay out of range and bring zeros
    mf_rsrc_t arsrc;
    uint32_t aoff, astep;
    {
        const int part = lane >> 3, l8 = lane & 7;
        aoff = part == 0 ? p.aux_mask + (uint32_t)(((int64_t)t0 * p.Bp + i0 + wave * 32) * 4) + l8 * 16
             : part == 1 ? p.aux_nv + (uint32_t)t0 * 128u + l8 * 16
             : part == 2 ? p.aux_lq + (uint32_t)t0 * 128u + l8 * 16
             : (CP && part == 3) ? p.aux_w + (uint32_t)t0 * 128u + l8 * 16 : MF_SRD_DEAD;
        astep = part == 0 ? (uint32_t)p.Bp * 4u : part <= (CP ? 3 : 2) ? 128u : 0u;
#if defined(__HIP_DEVICE_COMPILE__)
        arsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.aux_base), 0, (int)p.aux_bytes, 0x00020000);
#else
        (void)arsrc; (void)aoff;
#endif
    }
    // one memory instruction of the stage of tile t (into tile slot `slot`): j < PPW a tile piece, j = PPW the side inputs
    auto stage_piece = [&](int t, int slot, int j, bool live) {
        if (SPLIT && j < L::PPW) {
#if defined(__HIP_DEVICE_COMPILE__)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(irsrc, (mf_lds_ptr)(smem + slot * L::SLOTB + (wave * L::PPW + j) * 1024), 16, (int)ioff,
                                                     live ? (int)((unsigned)(t - t0) * FSI_TILEB + j * 1024) : (int)MF_SRD_DEAD, 0, 0);
#endif
        } else if (j < L::PPW) {
            mf_stage_tile_piece<D>(smem + slot * G::TILEB, t * 32, j, tsrc, live);
        } else {
#if defined(__HIP_DEVICE_COMPILE__)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(arsrc, (mf_lds_ptr)(smem + L::AUX0 + ((t - t0) & 3) * L::AUXB + wave * L::AUXW), 16,
                                                     (int)aoff, live ? 0 : (int)MF_SRD_DEAD, 0, 0);
#endif
            aoff += astep;
        }
    };
    auto stage = [&](int t, int slot) {
#pragma unroll
        for (int j = 0; j < L::NDMA; ++j) stage_piece(t, slot, j, true);
    };
    // The statistics of one tile, cut in 32 slices so they can be threaded between the MFMAs of
    // the next tile: slices 0..15 turn score e into logit e (and stash it), slices 16..31 fold
    // logit e into the running statistics.
    float Lg[16];
    float tmax = -FLT_MAX, nmx = -FLT_MAX, nmx2 = 0.f;
    uint32_t mw = 0u;
    f32x4 nv4 = {0.f, 0.f, 0.f, 0.f}, lq4 = {0.f, 0.f, 0.f, 0.f}, cw4 = {0.f, 0.f, 0.f, 0.f};
    auto slice = [&](int sidx, int te, const f32x16& acc) {
        const char* aux = smem + L::AUX0 + ((te - t0) & 3) * L::AUXB + wave * L::AUXW;
        if (sidx < 16) {
            const int e = sidx, q = e >> 2, r = e & 3;
            if (e == 0) {
                mw = reinterpret_cast<const uint32_t*>(aux)[c];
                tmax = -FLT_MAX;
                // valid negatives among this lane's 16 rows of the tile (rows (e&3) + 8 (e>>2) + 4 h)
                if (!CP) st.cnt += (float)(16 - __builtin_popcount(mw & (h ? 0xF0F0F0F0u : 0x0F0F0F0Fu)));
                mw >>= 4 * h;           // this lane's rows now sit at the compile-time bit (e&3) + 8 (e>>2)
            }
            if (r == 0) {
                nv4 = *reinterpret_cast<const f32x4*>(aux + L::AUX_NV + (8 * q + 4 * h) * 4);
                lq4 = *reinterpret_cast<const f32x4*>(aux + L::AUX_LQ + (8 * q + 4 * h) * 4);
                if (CP) cw4 = *reinterpret_cast<const f32x4*>(aux + L::AUX_CW + (8 * q + 4 * h) * 4);
            }
            // masked logit: -inf where the column is not a valid negative -> every statistic below and
            // every dloss/dL of the backward is exactly 0 there, with no further mask test
            const float Lraw = mf_logit(nu_i, nv4[r], acc[e], s_i, p.sigma, -lq4[r]);      // lq4 holds -logq
            Lg[e] = (mw & (1u << mf_acc_row(e, 0))) ? -INFINITY : Lraw;
            if (CP) st.cnt += (mw & (1u << mf_acc_row(e, 0))) ? 0.f : cw4[r];      // valid negatives: the copies count
            tmax = fmaxf(tmax, Lg[e]);
            if (r == 3) {   // stash 4 masked logits of the block for the backward sweeps
                float* blk = p.stash + ((int64_t)(i0 / 32 + wave) * p.NT + te) * 1024 + lane * 4;
                *reinterpret_cast<f32x4*>(blk + q * 256) = f32x4{Lg[e - 3], Lg[e - 2], Lg[e - 1], Lg[e]};
            }
        } else {
            const int e = sidx - 16;
            if (e == 0) {
                nmx = fmaxf(st.mx, tmax);
                if (NEED & NEED_LSE) st.se *= __expf(st.mx - nmx);
                st.mx = nmx;
                // exp(L - nmx) = exp2(fma(L, log2 e, -nmx log2 e)): one fma + one exp2 per element; the clamp
                // keeps the constant finite while nothing valid has been seen (nmx = -FLT_MAX, every L = -inf)
                nmx2 = -fmaxf(nmx, -1e30f) * 1.44269504088896341f;
            }
            if (CP) {
                if ((e & 3) == 0) cw4 = *reinterpret_cast<const f32x4*>(aux + L::AUX_CW + (8 * (e >> 2) + 4 * h) * 4);
                stats_add_masked_w<NEED>(st, Lg[e], sm, lii, p.margin, cw4[e & 3]);
                if (NEED & NEED_LSE) st.se = __builtin_fmaf(cw4[e & 3], __builtin_amdgcn_exp2f(__builtin_fmaf(Lg[e], 1.44269504088896341f, nmx2)), st.se);
            } else {
                stats_add_masked<NEED>(st, Lg[e], sm, lii, p.margin);
                if (NEED & NEED_LSE) st.se += __builtin_amdgcn_exp2f(__builtin_fmaf(Lg[e], 1.44269504088896341f, nmx2));
            }
        }
    };
    // one iteration: wait for tile tj + 1 (slot NS), then its 64 MFMAs into `nxt`, interleaved with the slices of tile
    // tj on `cur` and -- MODE 1: always, 2: if it exists, 0: never -- the stage of tile tj + 2 into the slot tile tj has left
    auto iterate = [&](int tj, auto cs_tag, auto mode_tag, const f32x16& cur, f32x16& nxt) {
        constexpr int CS = decltype(cs_tag)::value, NS = CS ^ 1, MODE = decltype(mode_tag)::value;
        // every DMA of the stage of tile tj + 1 is older than the KEEP youngest stores
        if (tj == t0) mf_wait_vmcnt<0>(); else mf_wait_vmcnt<L::KEEP>();
        mf_block_barrier();
        const bool live = MODE == 1 || tj + 2 < t1;
        if constexpr (SPLIT) {
            nxt = mf_tile_scores_split_interleaved<32, FWD_SPLIT_VPM>(
                smem + NS * L::SLOTB, xs, [&](int sidx) { slice(sidx, tj, cur); },
                [&](int g) {
                    if (MODE != 0 && g <= L::LASTG) {
#pragma unroll
                        for (int j = g * L::DPG; j < (g + 1) * L::DPG && j < L::NDMA; ++j) stage_piece(tj + 2, CS, j, live);
                    }
                });
        } else {
        nxt = mf_tile_scores_interleaved<D, 32, (40 * 32 / D)>(
            smem + NS * G::TILEB, xf, [&](int sidx) { slice(sidx, tj, cur); },
            [&](int g) { if (MODE != 0 && g <= L::LASTG) stage_piece(tj + 2, CS, g, live); });
        }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;

    if (t0 < t1) {
        stage(t0, 0);
        if (t0 + 1 < t1) stage(t0 + 1, 1);
        // tile t0: its stage's DMAs are the older ones
        if (t0 + 1 < t1) mf_wait_vmcnt<L::NDMA>(); else mf_wait_vmcnt<0>();
        mf_block_barrier();
        f32x16 accA, accB;
        if constexpr (SPLIT) accA = mf_tile_scores_split_interleaved<32, FWD_SPLIT_VPM>(smem, xs, [](int) {}, [](int) {});
        else accA = mf_tile_scores_interleaved<D, 32, (40 * 32 / D)>(smem, xf, [](int) {});
        int tj = t0;
        for (; tj + 2 < t1; tj += 2) {      // two tiles per trip: slots and accumulators swap roles by name
            iterate(tj, I0{}, I1{}, accA, accB);
            iterate(tj + 1, I1{}, I2{}, accB, accA);
        }
        if (tj + 1 < t1) {                  // tiles tj (scores in accA) and tj + 1 remain
            iterate(tj, I0{}, I0{}, accA, accB);
#pragma unroll
            for (int sidx = 0; sidx < 32; ++sidx) slice(sidx, tj + 1, accB);
        } else {                            // tile tj remains
#pragma unroll
            for (int sidx = 0; sidx < 32; ++sidx) slice(sidx, tj, accA);
        }
        mf_wait_vmcnt<0>();                 // nothing of this workgroup may still be on its way into LDS when it ends
    }
    // the row's other half of the columns lives in lane ^ 32
    {
        const float mx2 = mf_shfl_xor32(st.mx), se2 = mf_shfl_xor32(st.se);
        lse_merge(st.mx, st.se, mx2, se2);
        st.cnt += mf_shfl_xor32(st.cnt); st.A += mf_shfl_xor32(st.A);
        st.H += mf_shfl_xor32(st.H); st.Hc += mf_shfl_xor32(st.Hc);
        st.Lg += mf_shfl_xor32(st.Lg); st.Ls += mf_shfl_xor32(st.Ls);
    }
    if (h == 0) {
        float* o = p.part + (int64_t)blockIdx.x * NSTAT * p.Bp + i;
        o[ST_CNT * p.Bp] = st.cnt; o[ST_A * p.Bp] = st.A; o[ST_MX * p.Bp] = st.mx; o[ST_SE * p.Bp] = st.se;
        o[ST_H * p.Bp] = st.H; o[ST_HC * p.Bp] = st.Hc; o[ST_LG * p.Bp] = st.Lg; o[ST_LS * p.Bp] = st.Ls;
    }
}

template <int D, int NEED, bool CP, bool SPLIT>
static void launch_fwd_n(dim3 grid, const FwdParams& fp, hipStream_t s) {
    auto fn = loss_fwd_dense_kernel<D, NEED, CP, SPLIT>;
    using L = FwdLds<D, SPLIT>;
    if (L::BYTES > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, L::BYTES);
    fn<<<grid, 64 * mf_nw(D), L::BYTES, s>>>(fp);
}
template <int D, bool CP = false, bool SPLIT = false>
static void launch_fwd(int need, dim3 grid, const FwdParams& fp, hipStream_t s) {
    switch (need) {   // single-loss calls get a specialised epilogue; anything else computes every statistic
        case NEED_CONTR: launch_fwd_n<D, NEED_CONTR, CP, SPLIT>(grid, fp, s); break;
        case NEED_LSE: launch_fwd_n<D, NEED_LSE, CP, SPLIT>(grid, fp, s); break;
        case NEED_HINGE: launch_fwd_n<D, NEED_HINGE, CP, SPLIT>(grid, fp, s); break;
        case NEED_LOGI: launch_fwd_n<D, NEED_LOGI, CP, SPLIT>(grid, fp, s); break;
        default: launch_fwd_n<D, 15, CP, SPLIT>(grid, fp, s); break;
    }
}

// The image of the streamed item tiles for the split forward (fsi_index, mf_bf_split.h): a workgroup is one tile, thread
// (k-step s, lane (c, h)) reads features 16 s + 8 h .. + 7 of tile row c and writes the 16-byte fragments of its three pieces
// -- whole KiB per wave and piece.  Rows from `rows` on (geo: from the N' distinct columns on) are written as zeros; of a
// packed v' only the tiles the sweep streams are written.
__global__ __launch_bounds__(512) void fwd_split_image_kernel(const float* __restrict__ src, int64_t rows, unsigned short* __restrict__ img,
                                                              const int32_t* __restrict__ geo) {
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
    const int tile = (int)blockIdx.x;
    if (geo) {
        if (tile >= geo[CG_NT]) return;
        rows = geo[CG_NCOLS];
    }
    const int s = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int64_t y = (int64_t)tile * 32 + c;
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
    if (y < rows) {
        const f32x4* p = reinterpret_cast<const f32x4*>(src + y * 128 + 16 * s + 8 * h);
        lo = p[0]; hi = p[1];
    }
    u16x8 out[3];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        unsigned short o[3];
        mbf_split3(j < 4 ? lo[j] : hi[j - 4], o);
        out[0][j] = o[0]; out[1][j] = o[1]; out[2][j] = o[2];
    }
    u16x8* dst = reinterpret_cast<u16x8*>(img + (int64_t)tile * FSI_TILE_ELEMS);
#pragma unroll
    for (int q = 0; q < 3; ++q) dst[fsi_index(c, 16 * s + 8 * h, q) >> 3] = out[q];
}
// tests only: slot of (row of the tile, feature, piece) in a tile's forward image
extern "C" int mf_fwd_split_image_index(int row, int feature, int piece) {
    if (row < 0 || row >= 32 || feature < 0 || feature >= 128 || piece < 0 || piece >= 3) return -1;
    return fsi_index(row, feature, piece);
}

__global__ __launch_bounds__(256) void mask_export_dense_kernel(const uint32_t* __restrict__ maskW, int64_t B,
                                                                int64_t N, int64_t Bp, int NT,
                                                                uint32_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= B * NT) return;
    const int64_t i = t / NT;
    const int w = (int)(t % NT);
    uint32_t bits = ~maskW[(int64_t)w * Bp + i];
    const int64_t rem = N - (int64_t)w * 32;
    if (rem < 32) bits &= (1u << rem) - 1u;
    out[i * NT + w] = bits;
}

// The forward stashes the MASKED logits (-inf where the column is not a valid negative) of every
// 32 x 32 (user tile, item tile) block in HBM (B x N fp32: 0.5 GB at B = 8192 -- MI355X has
// 288 GB) so that the two backward sweeps only contract: they never recompute the score tile.
// Block (ti, tj) is 4 KiB: [q = e / 4][lane][e % 4] in the forward's accumulator layout
// (lane = user), i.e. four whole-KiB coalesced stores per tile and a linear LDS-DMA on the way
// back.  The dU sweep turns each block into G' = dloss/dL (one exp / step / sigmoid per element,
// diagonal patched).  What happens to G' next depends on which pipe contracts it:
//  * fp32 sweeps (v_mfma_f32_32x32x2f32; d = 32, 256, and d = 128 with the split switched off): dU writes G' to a second
//    stash and dV, which runs after it, reads it and has no per-element arithmetic at all.  The fp32 MFMA and the VALU share
//    the SIMD's FP32 lanes there (a VALU op costs ~2 cycles of MFMA throughput, a transcendental ~17 -- measured), so every
//    VALU instruction removed from those loops is MFMA time won back.
//  * split sweeps (v_mfma_f32_32x32x16_bf16, d = 128; SPLIT below) and d = 64: the matrix time of a tile is short, VALU work
//    beside a bf16 MFMA costs it nothing while it fits the gaps, and the sweeps are bound by the 4 KiB stash block each
//    tile brings.  dV derives G' from the logit stash itself and dU writes no second stash (RECOMP in BwdLds): one pass
//    over the stash per sweep instead of three for the pair.
// (Folding the split sum into these kernels -- the workgroup that reaches an X block's ticket last adds the
// partials -- was measured and dropped: 64..128 last workgroups reading 8 x 64 KiB each is far less parallel than
// the separate sum_parts launch; dU 0.287 -> 0.489 ms.)
struct BwdParams {
    const float *u, *v, *rowc;
    const float* grad_out;   // device scalar: the row coefficients are scaled by it here
    const float* stash;      // masked logits (forward); stays intact so that a backward can be repeated
    float* gstash;           // G' = dloss/dL blocks: written by the dU sweep, read by the dV sweep
    float* dpart;
    float* rpart;            // [split][Xp] partial row sums of G'
    int64_t B, N, Bp, Np;
    int NT, YT, tps;
    // distinct-column sweeps (CP): v is the packed v', the streamed / kept extent of the item axis comes from the device words
    const int32_t* geo;
    const float* cw;         // column weights (dU: the MFMA operand and the row sum take G' x w; the stash keeps G' itself)
    const unsigned short* img;   // split sweeps: the bf16 piece image of the streamed operand, YT tiles (mf_bf_split.h)
};

#ifndef BWD_SPLIT_VPM
#define BWD_SPLIT_VPM 7       // A/B knob: VALU / SALU instructions of the next tile's G' placed behind each MFMA of the split contraction
#endif
#ifndef BWD_SPLIT_DPG
#define BWD_SPLIT_DPG 4       // A/B knob: memory instructions of the next stage per step (12 MFMAs) of the split contraction (12: all in the first)
#endif
template <int D, bool XU, int SPLIT = 0>
struct BwdLds {
    using G = TileGeom<D>;
    static_assert(SPLIT == 0 || D == 128, "the split sweeps are written for d = 128");
    // Two schedules (see the kernel): SPREAD for long tiles (d >= 64) -- 2-slot tile ring, the wave's own
    // 4 KiB stash / G' block comes straight into registers (it is wave-private: routing it through LDS
    // only added 16 KiB of DMA writes and 16 KiB of reads per tile to an LDS port that the MFMA operand
    // reads need); otherwise whole stages two tiles ahead, stash blocks behind the tile in each slot.
    static constexpr bool SPREAD = D >= 64;
    static constexpr int LT = G::TILEB;                  // (not SPREAD) NW x 4 KiB stash blocks behind the tile
    static constexpr int SLOT = SPLIT ? BSI_TILEB : G::TILEB + (SPREAD ? 0 : G::NW * 4096);
    static constexpr int EXTRA = XU ? 0 : G::NW * 32 * 32 * 4;   // dV: per-wave 32 x 32 transpose scratch (XOR-swizzled)
    // the deepest ring that still puts two waves on every SIMD (two 4-wave workgroups per CU, or one of
    // eight waves); 2 slots cost a second barrier per tile, measured free
    static constexpr int NSLOT = SPREAD ? 2 : (((G::NW == 8 ? 1 : 2) * (3 * SLOT + EXTRA) <= 160 * 1024) ? 3 : 2);
    static constexpr int TR = NSLOT * SLOT;
    static constexpr int BYTES = TR + EXTRA;
    // d = 64 (config C2): the sweeps are HBM-bound on the 4 KiB stash blocks, not MFMA-bound (a block costs 4 KiB at every width, a tile's
    // MFMAs shrink with d).  There the dV sweep derives G' from the LOGIT stash itself -- the per-element map dU applies, with
    // the users' coefficients loaded per tile (lanes are users BEFORE the block is transposed) -- and dU no longer writes a
    // G' stash: dU moves 0.57 GB instead of 1.07 at C2's shape (round 4; same bits: the same map on the same logits).
    // (The split sweeps at d = 128 are stash-bound in the same way and do the same.)
    static constexpr bool RECOMP = D == 64 || SPLIT != 0;   // (d = 32 stages two tiles ahead: the coefficients would need a ring of their own)
    static constexpr int NCOEF = (RECOMP && !XU) ? 4 : 0;   // a, b, coefG, gdiag of the tile's users
    static constexpr int PPW = SPLIT ? BSI_TILEB / G::NW / 1024 : G::PPW;   // 1-KiB DMA pieces of the streamed tile per wave
    static constexpr int NDMA = PPW + 4 + NCOEF;         // memory instructions per wave per stage (4 = the stash block)
    static constexpr int NSTORE = (XU && !RECOMP) ? 4 : 0;  // G' stores per tile
};

// XU = true : lanes hold users, item tiles stream, result d loss / d u   (reads L, writes G' back)
// XU = false: lanes hold items, user tiles stream, result d loss / d v   (reads G')
// CP (distinct-column sweeps, mf_loss_cols.h): the item axis holds the N' packed columns.  dU streams the tiles [0, NT')
// of v' in the splits the device words name, weights G' by the copy count for the contraction and the row sum, and
// patches no diagonal (a user's own column is masked by id in every copy: G' = 0 there; the epilogue adds the term).
// dV is launched as a LINEAR grid for the worst case: workgroup id -> (X block, split) by the device geometry.
// SPLIT (d = 128): the contraction on the bf16 matrix cores, fp32-grade (mf_bf_split.h).  The streamed operand arrives as its
// image of three bf16 pieces (bwd_split_image_kernel), G' is split in registers -- in accumulator layout it IS the B operand
// of v_mfma_f32_32x32x16_bf16, two k-steps of 16 rows -- and the six leading piece products go into the same fp32
// accumulators: 48 MFMAs of 8 passes per tile instead of 64 of 16.  Everything around the contraction -- the G' map, the
// stash, the transpose, the row sum, the epilogue -- is the fp32 sweep's; dV derives G' itself (RECOMP, see BwdLds).
template <int D, bool XU, int GMODE, bool CP, int SPLIT>
__global__ __launch_bounds__(64 * mf_nw(D), (D == 128 || D == 64) ? BWD_MIN_WG : 1) void loss_bwd_dense_kernel(BwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using L = BwdLds<D, XU, SPLIT>;
    static_assert(!CP || (L::SPREAD && (!L::RECOMP || SPLIT)), "the distinct-column sweeps are written for the d = 128 schedule");
    const int lane = mf_lane(), c = lane & 31, h = lane >> 5;
    const int wave = mf_wave_id();
    int split = blockIdx.x, tps = p.tps, YT = p.YT;
    int64_t xblk = blockIdx.y, nX = XU ? p.B : p.N, Xp = XU ? p.Bp : p.Np;
    if (CP) {
        if (XU) {
            YT = p.geo[CG_NT]; tps = p.geo[CG_TPSU];
            if (split * tps >= YT) return;                  // beyond the splits of N' (the epilogue adds geo's count of them)
        } else {
            const int nsv = p.geo[CG_NSV], xbv = p.geo[CG_XBV];
            tps = p.geo[CG_TPSV];
            xblk = blockIdx.x / nsv; split = blockIdx.x % nsv;
            if (xblk >= xbv) return;
            nX = p.geo[CG_NCOLS]; Xp = (int64_t)xbv * TileGeom<D>::XB;
        }
    }
    const int64_t x0 = xblk * TileGeom<D>::XB + wave * 32;     // this wave's X tile (grid = (Y split, X block))
    const int64_t x = x0 + c;
    const int xt = (int)(x0 >> 5);
    const int64_t nY = XU ? p.N : p.B;
    const float* Y = XU ? p.v : p.u;
    const int t0 = split * tps, t1 = min(YT, t0 + tps);
    constexpr int NDMA = L::NDMA + ((CP && XU) ? 4 : 0);       // memory instructions per wave and stage (CP dU: + the weights)
    constexpr bool RECOMP = L::RECOMP;
    float xa = 0.f, xb = 0.f, xc = 0.f, xd = 0.f;
    const float gout = p.grad_out[0];
    if (XU) {
        xa = p.rowc[x]; xb = p.rowc[p.Bp + x]; xc = gout * p.rowc[2 * p.Bp + x]; xd = gout * p.rowc[3 * p.Bp + x];
    }
    float xb2 = xb * 1.44269504088896341f;             // exp((L - a) + b) = exp2((L - a) log2e + b log2e): a is the row's largest logit
                                                       // (L - a: exact where it matters), b = -log(sum) is small -- rowc_row
    float cn[4] = {0.f, 0.f, 0.f, 0.f};                // dV, RECOMP: the coefficients of the NEXT tile's user (lane = user c of the tile)
    f32x16 dacc[D / 32];
#pragma unroll
    for (int mb = 0; mb < D / 32; ++mb)
#pragma unroll
        for (int e = 0; e < 16; ++e) dacc[mb][e] = 0.f;
    float rsum = 0.f;

    TileSrc<D> tsrc;
    if (!SPLIT) mf_tile_src_init<D>(tsrc, Y, nY, (int64_t)t0 * 32);
    // SPLIT: the image is copied linearly -- one descriptor over its tiles from t0 (p.YT of them exist), piece q of this
    // wave's share at lane offset + scalar ((t - t0) tiles + q KiB); a tile past the descriptor's end would arrive as zeros
    mf_rsrc_t irsrc;
    const unsigned ioff = (unsigned)(wave * L::PPW * 1024 + lane * 16);
    if (SPLIT) {
        int64_t bytes = (int64_t)(p.YT - t0) * BSI_TILEB;
        bytes = bytes < 0 ? 0 : (bytes > (int64_t)MF_SRD_MAX_BYTES ? (int64_t)MF_SRD_MAX_BYTES : bytes);
#if defined(__HIP_DEVICE_COMPILE__)
        irsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(p.img + (int64_t)t0 * BSI_TILE_ELEMS), 0, (int)(unsigned)bytes, 0x00020000);
#else
        (void)irsrc; (void)ioff;
#endif
    }
    auto block_of = [&](int t) { return XU ? ((int64_t)xt * p.NT + t) : ((int64_t)t * p.NT + xt); };
    // piece j of the staging of tile t: 0..3 the wave's 4 KiB stash / G' block (into LDS, or -- SPREAD --
    // straight into the registers Gn), 4.. its share of the Y tile
    constexpr bool SPREAD = L::SPREAD;
    f32x4 Gn[4], Wn[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { Gn[q] = f32x4{0.f, 0.f, 0.f, 0.f}; Wn[q] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    auto stage_piece = [&](int t, int slot_idx, int j) {
        char* slot = smem + slot_idx * L::SLOT;
        if (CP && XU && j >= L::NDMA) {      // the weights of the tile's columns, rows 8 q + 4 h .. + 3 (this lane's registers)
            Wn[j - L::NDMA] = *reinterpret_cast<const f32x4*>(p.cw + (int64_t)t * 32 + 8 * (j - L::NDMA) + 4 * h);
        } else if (L::NCOEF && j >= L::NDMA - L::NCOEF) {
            cn[j - (L::NDMA - L::NCOEF)] = p.rowc[(int64_t)(j - (L::NDMA - L::NCOEF)) * p.Bp + (int64_t)t * 32 + c];
        } else if (j < 4) {
            const char* lsrc = reinterpret_cast<const char*>(((XU || RECOMP) ? p.stash : p.gstash) + block_of(t) * 1024) + lane * 16;
            if (SPREAD) Gn[j] = *reinterpret_cast<const f32x4*>(lsrc + j * 1024);
            else __builtin_amdgcn_global_load_lds((mf_glb_ptr)(lsrc + j * 1024), (mf_lds_ptr)(slot + L::LT + wave * 4096 + j * 1024), 16, 0, 0);
        } else if (SPLIT) {
#if defined(__HIP_DEVICE_COMPILE__)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(irsrc, (mf_lds_ptr)(slot + (wave * L::PPW + (j - 4)) * 1024), 16, (int)ioff,
                                                     (int)((unsigned)(t - t0) * BSI_TILEB + (j - 4) * 1024), 0, 0);
#endif
        } else {
            mf_stage_tile_piece<D>(slot, t * 32, j - 4, tsrc);
        }
    };
    auto stage = [&](int t, int slot_idx) {
#pragma unroll
        for (int j = 0; j < NDMA; ++j) stage_piece(t, slot_idx, j);
    };
    // A tile's stash block as it arrived (SPREAD: in Gn) with its weights, and -- dV, RECOMP -- its users' coefficients
    auto take = [&](float (&Gv)[16], float (&Wv)[16], const char* lt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 t4 = SPREAD ? Gn[q] : *reinterpret_cast<const f32x4*>(lt + q * 1024 + lane * 16);
#pragma unroll
            for (int t = 0; t < 4; ++t) { Gv[4 * q + t] = t4[t]; Wv[4 * q + t] = Wn[q][t]; }
        }
        if (!XU && RECOMP) {            // this tile's users' coefficients (asked for with the block)
            xa = cn[0]; xb = cn[1]; xc = gout * cn[2]; xd = gout * cn[3];
            xb2 = xb * 1.44269504088896341f;
        }
    };
    // a masked logit -> G' (masked entries are -inf: exp / step / sigmoid give exactly 0)
    auto gmap = [&](float Lm) {
        if (GMODE == G_EXP) return xc * __builtin_amdgcn_exp2f(__builtin_fmaf(Lm - xa, 1.44269504088896341f, xb2));
        return xc * g_of(GMODE, (Lm - xa) + xb);
    };
    // The block of tile `tile` -> the B operand of its contraction: G' (unless the stash holds it already), handed to dV,
    // weighted, transposed for dV; its elements are added to the lane's row sum `rs`
    auto gprime = [&](float (&Gv)[16], const float (&Wv)[16], int tile, float& rs) {
        if (XU || RECOMP) {
#pragma unroll
            for (int e = 0; e < 16; ++e) Gv[e] = gmap(Gv[e]);
            if (!CP && tile == xt) {    // only the diagonal tile holds the user's own positive
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (mf_acc_row(e, h) == c) Gv[e] = xd;
            }
        }
        if (XU && !RECOMP) {
            float* blk = p.gstash + block_of(tile) * 1024 + lane * 4;   // hand G' to the dV sweep
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<f32x4*>(blk + q * 256) = f32x4{Gv[4 * q], Gv[4 * q + 1], Gv[4 * q + 2], Gv[4 * q + 3]};
        }
        if (XU && CP) {                 // (the stash keeps the per-copy gradient: dV needs it unweighted)
#pragma unroll
            for (int e = 0; e < 16; ++e) Gv[e] *= Wv[e];
        }
        if (!XU) {
            // block layout is (lane = user, register = item row): transpose to (lane = item, register = user row)
            float* tr = reinterpret_cast<float*>(smem + L::TR) + wave * (32 * 32);
#pragma unroll
            for (int e = 0; e < 16; ++e) tr[mf_acc_row(e, h) * 32 + (c ^ mf_acc_row(e, h))] = Gv[e];
#pragma unroll
            for (int e = 0; e < 16; ++e) Gv[e] = tr[c * 32 + (mf_acc_row(e, h) ^ c)];
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) rs += Gv[e];
    };
    if constexpr (SPLIT != 0) {
        // The split schedule.  The contraction of a tile is 48 short MFMAs, too few to hide what precedes them, so the G' of
        // tile ty + 1 -- map, transpose, the split into pieces: VALU and LDS work -- is computed beside the MFMAs of tile ty,
        // and the register loads (stash block, weights, coefficients) run TWO tiles ahead; the image of tile ty + 1 goes into
        // the slot tile ty - 1 left, as in SPREAD.  One barrier per tile.
        static_assert(L::RECOMP && SPREAD, "the split sweeps keep no G' stash");
        typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
        // G' in three bf16 pieces: g[s][q] is piece q of registers 8 s .. 8 s + 7, the B fragment of k-step s
        auto split_g = [&](const float (&Gv)[16], mbf16x8 (&g)[2][3], int s) {
            u16x8 g3[3];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                unsigned short o[3];
                mbf_split3(Gv[8 * s + j], o);
                g3[0][j] = o[0]; g3[1][j] = o[1]; g3[2][j] = o[2];
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) g[s][q] = __builtin_bit_cast(mbf16x8, g3[q]);
        };
        // The memory instructions of a stage, in issue order: the four register loads of tile `tr`'s stash block (they come
        // from HBM: the longest way), the four per-lane loads of its side inputs (dU under the column plan: the lane's 16 column
        // weights; dV: its user's four coefficients), then the PPW image pieces of tile `ti` (not live: a dead scalar offset,
        // the piece fetches nothing).
        constexpr int NSIDE = XU ? (CP ? 4 : 0) : L::NCOEF;
        constexpr int NMEM = 4 + NSIDE + L::PPW;
        constexpr int DPG = BWD_SPLIT_DPG;
        static_assert(NMEM == NDMA, "the stage of the split loops is the stage BwdLds counts");
        static_assert(DPG >= 1 && DPG <= 12, "one to twelve memory instructions to a step");
        static_assert(4 * DPG >= NMEM, "a stage's memory instructions must fit the four steps of the contraction");
        // where a stage reads: the lane's 16 bytes of tile tr's stash block, its per-lane side inputs, the scalar offset of
        // tile ti's image (dead: past the descriptor's end, + 5 KiB and a lane offset do not wrap) -- computed ahead of the
        // contraction, so that no memory instruction inside it waits for address arithmetic
        struct StageSrc {
            const char* g;
            const float* side;
            unsigned img;
        };
        auto stage_src = [&](int ti, bool live, int tr) {
            StageSrc a;
            a.g = reinterpret_cast<const char*>(p.stash + block_of(tr) * 1024) + lane * 16;
            a.side = XU ? p.cw + (int64_t)tr * 32 + 4 * h : p.rowc + (int64_t)tr * 32 + c;
            a.img = live ? (unsigned)(ti - t0) * BSI_TILEB : MF_SRD_DEAD;
            return a;
        };
        auto mem_piece = [&](int i, int slot_idx, const StageSrc& a) {
            if (i < 4) {
                Gn[i] = *reinterpret_cast<const f32x4*>(a.g + i * 1024);
            } else if (i < 4 + NSIDE) {
                const int j = i - 4;
                if (XU) Wn[j] = *reinterpret_cast<const f32x4*>(a.side + 8 * j);     // rows 8 j + 4 h .. + 3 of the tile
                else cn[j] = a.side[(int64_t)j * p.Bp];
            } else {
#if defined(__HIP_DEVICE_COMPILE__)
                const int j = i - 4 - NSIDE;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(irsrc, (mf_lds_ptr)(smem + slot_idx * L::SLOT + (wave * L::PPW + j) * 1024), 16, (int)ioff,
                                                         (int)(a.img + j * 1024), 0, 0);
#endif
            }
        };
        auto stage_regs = [&](int t) {
            const StageSrc a = stage_src(t0, false, t);
#pragma unroll
            for (int i = 0; i < 4 + NSIDE; ++i) mem_piece(i, 0, a);
        };
        auto stage_image = [&](int t, int slot_idx) {
            const StageSrc a = stage_src(t, true, t);
#pragma unroll
            for (int i = 4 + NSIDE; i < NMEM; ++i) mem_piece(i, slot_idx, a);
        };
        // The G' of a tile in four slices, one beside each step of the previous tile's contraction; the arithmetic and its
        // order are gprime's.  0, 1: the map of registers 8 sl .. 8 sl + 7, the diagonal, the weights and (dV) their way into the
        // transpose scratch; 2: (dV) the transposed block back, the row sum, the pieces of k-step 0; 3: the pieces of k-step 1.
        // (dV: the image pieces in flight would make hipcc drain them before a store it sees: mf_lds_store_b32, mf_stream.h.)
        auto gslice = [&](int sl, float (&Gv)[16], const float (&Wv)[16], int tile, float& rs, mbf16x8 (&g)[2][3]) {
            float* tr = reinterpret_cast<float*>(smem + L::TR) + wave * (32 * 32);
            if (sl < 2) {
#pragma unroll
                for (int e = 8 * sl; e < 8 * sl + 8; ++e) {
                    Gv[e] = gmap(Gv[e]);
                    if (!CP && tile == xt && mf_acc_row(e, h) == c) Gv[e] = xd;
                    if (XU && CP) Gv[e] *= Wv[e];
                    if (!XU) mf_lds_store_b32(&tr[mf_acc_row(e, h) * 32 + (c ^ mf_acc_row(e, h))], Gv[e]);
                }
            } else if (sl == 2) {
                if (!XU) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) Gv[e] = tr[c * 32 + (mf_acc_row(e, h) ^ c)];
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) rs += Gv[e];
            }
            if (sl >= 2) split_g(Gv, g, sl - 2);
        };
        mbf16x8 gb[2][3];
        float Gv[16], Wv[16];
        if (t0 < t1) {
            stage_image(t0, 0);
            stage_regs(t0);
            mf_wait_vmcnt<0>();
            take(Gv, Wv, nullptr);
            if (t0 + 1 < t1) stage_regs(t0 + 1);
#pragma unroll
            for (int sl = 0; sl < 4; ++sl) gslice(sl, Gv, Wv, t0, rsum, gb);
        }
        // In the loop, tile ty's contraction carries the stage behind it: BWD_SPLIT_DPG memory instructions to each of its four
        // steps (fenced: a step's instructions stay in it), the register loads of tile ty + 2 first (they come from HBM),
        // then the image pieces of tile ty + 1.  What keeps this right:
        //  * slot reuse -- the image of tile ty + 1 lands in the slot tile ty - 1 left; every piece is issued behind the barrier
        //    at the top of tile ty, which proves that every wave has finished tile ty - 1 (and the fences between the steps keep
        //    the compiler from moving one above it);
        //  * registers -- take() at the top has copied Gn / Wn / cn (tile ty + 1) out before any load of tile ty + 2
        //    is issued into them, and nothing reads them again before the next top;
        //  * the wait -- everything outstanding at a top was issued during the previous tile, the image of tile ty among it:
        //    vmcnt(0), no count to derive;
        //  * no branch around a load: stage and MFMAs share one basic block.  A piece of a tile that does not exist carries
        //    the dead offset, and the register loads name the split's last tile again (in bounds, copied out, never used).
        int cur = 0;
        for (int ty = t0; ty < t1; ++ty) {
            mf_wait_vmcnt<0>();           // the image of tile ty and the registers of tile ty + 1: issued one tile ago
            mf_block_barrier();
            const bool more = ty + 1 < t1;
            take(Gv, Wv, nullptr);        // tile ty + 1 as it arrived (none: the last tile's block again, unused)
            const int tr = min(ty + 2, t1 - 1);
            const StageSrc src = stage_src(ty + 1, more, tr);
            __builtin_amdgcn_sched_barrier(0);   // what the top of a tile does stays ahead of its first step
            float rs = 0.f;
            mbf16x8 gn[2][3];
            // dX[m][x] += sum_y Y[y][m] * G[y][x], piece products a_i g_j with i + j <= 2, the smallest first.  A step is one
            // k-step of two accumulator blocks (12 MFMAs, alternating between the two); its six A fragments are read one
            // step ahead.
            const mbf16x8* img = reinterpret_cast<const mbf16x8*>(smem + cur * L::SLOT) + lane;
            auto frags = [&](mbf16x8 (&a)[2][3], int step) {
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int q = 0; q < 3; ++q) a[b][q] = img[((q * 4 + 2 * (step & 1) + b) * 2 + (step >> 1)) * 64];
            };
            mbf16x8 av[2][3];
            frags(av, 0);
#pragma unroll
            for (int step = 0; step < 4; ++step) {
                mbf16x8 an[2][3];
                if (step + 1 < 4) frags(an, step + 1);
#pragma unroll
                for (int i = step * DPG; i < (step + 1) * DPG && i < NMEM; ++i) mem_piece(i, cur ^ 1, src);
                gslice(step, Gv, Wv, ty + 1, rs, gn);
                const int s = step >> 1, b0 = 2 * (step & 1);
#pragma unroll
                for (int pr = 0; pr < 6; ++pr) {
                    // (a piece, g piece): (2,0) (1,1) (0,2) | (1,0) (0,1) | (0,0)
                    const int ai = pr == 0 ? 2 : (pr == 1 || pr == 3) ? 1 : 0;
                    const int gi = pr == 2 ? 2 : (pr == 1 || pr == 4) ? 1 : 0;
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        dacc[b0 + b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[b][ai], gb[s][gi], dacc[b0 + b], 0, 0, 0);
                }
                // one MFMA, then a share of the slice's VALU work, twelve times (hipcc otherwise keeps the streams apart); the
                // fence pins the step's memory instructions and its slice to the step
#pragma unroll
                for (int m = 0; m < 12; ++m) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x006, BWD_SPLIT_VPM, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (step + 1 < 4) {
#pragma unroll
                    for (int b = 0; b < 2; ++b)
#pragma unroll
                        for (int q = 0; q < 3; ++q) av[b][q] = an[b][q];
                }
            }
            rsum += more ? rs : 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int q = 0; q < 3; ++q) gb[s][q] = gn[s][q];
            cur ^= 1;
        }
    } else {
    // Two schedules.  SPREAD (2-slot ring, d >= 64): the loads of tile ty+1 are issued ONE PER MFMA STEP
    // inside the contraction of tile ty, the tile pieces into the slot tile ty-1 left; no second barrier.
    // Otherwise (3 slots, short tiles): whole stages, two tiles ahead.
    if (t0 < t1) stage(t0, 0);
    if (!SPREAD && t0 + 1 < t1) stage(t0 + 1, 1);
    int cur = 0;
    for (int ty = t0; ty < t1; ++ty) {
        if (SPREAD) {
            mf_wait_vmcnt<0>();           // tile ty: issued one tile ago, spread over the previous contraction
        } else {
            // queue, oldest first: [DMA(ty)] [G stores(ty-2)] [DMA(ty+1)] [G stores(ty-1)]   (stores: dU only)
            if (ty + 1 >= t1) mf_wait_vmcnt<0>();
            else if (L::NSTORE == 0 || ty == t0) mf_wait_vmcnt<L::NDMA>();
            else mf_wait_vmcnt<L::NDMA + L::NSTORE>();
        }
        mf_block_barrier();
        if (!SPREAD && L::NSLOT == 3 && ty + 2 < t1) stage(ty + 2, cur >= 1 ? cur - 1 : 2);
        const char* slot = smem + cur * L::SLOT;
        float Gv[16], Wv[16];
        take(Gv, Wv, slot + L::LT + wave * 4096);
        gprime(Gv, Wv, ty, rsum);
        // dX[m][x] += sum_y Y[y][m] * G[y][x]   (the G tile is already a B operand)
        // (the Y fragment of step t + 1 is read before the MFMAs of step t are issued)
        const bool more = ty + 1 < t1;
        float yv[D / 32];
        mf_lds_cols<D>(yv, slot, mf_acc_row(0, h), c);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            float yn[D / 32];
            if (t + 1 < 16) mf_lds_cols<D>(yn, slot, mf_acc_row(t + 1, h), c);
            if (SPREAD && t < NDMA && more) stage_piece(ty + 1, cur ^ 1, t);
#pragma unroll
            for (int j = 0; j < D / 32; ++j)
                dacc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(yv[j], Gv[t], dacc[j], 0, 0, 0);
            if (t + 1 < 16) {
#pragma unroll
                for (int j = 0; j < D / 32; ++j) yv[j] = yn[j];
            }
        }
        if (!SPREAD && L::NSLOT == 2) {            // the slot just read is the one tile ty+2 lands in
            mf_block_barrier();
            if (ty + 2 < t1) stage(ty + 2, cur);
        }
        cur = cur + 1 == L::NSLOT ? 0 : cur + 1;
    }
    }
    mf_wait_vmcnt<0>();                 // nothing of this workgroup may still be on its way into LDS when it ends
    rsum += mf_shfl_xor32(rsum);
    // dX[x][m] = sum over splits of (dacc - rsum * X[x][m]): this sweep writes its partial dacc (register e of
    // block j is feature m = NB * row(e, h) + j: NB consecutive floats per register index) and its partial row sum;
    // sum_parts_kernel adds the splits in order and applies the X term once.
    if (x < nX) {
        constexpr int NB = D / 32;
        float* o = p.dpart + ((int64_t)split * Xp + x) * D;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m0 = NB * mf_acc_row(e, h);
            if constexpr (NB == 4) {
                *reinterpret_cast<f32x4*>(o + m0) = f32x4{dacc[0][e], dacc[1][e], dacc[2][e], dacc[3][e]};
            } else if constexpr (NB == 8) {
                *reinterpret_cast<f32x4*>(o + m0) = f32x4{dacc[0][e], dacc[1][e], dacc[2][e], dacc[3][e]};
                *reinterpret_cast<f32x4*>(o + m0 + 4) = f32x4{dacc[4][e], dacc[5][e], dacc[6][e], dacc[7][e]};
            } else {
#pragma unroll
                for (int j = 0; j < NB; ++j) o[m0 + j] = dacc[j][e];
            }
        }
        if (h == 0) p.rpart[(int64_t)split * Xp + x] = rsum;
    }
}

// out[r] = sum over splits (in split order) of dpart[s][r]  -  (sum over splits of rpart[s][r]) * X[r],
// for the rows of dU (workgroups [0, nb_a)) and of dV (the rest) in one launch
struct SumJob {
    const float *dpart, *rpart, *X;
    int nsplit;
    int64_t rows, rows_p;
    float* out;
};
__global__ __launch_bounds__(256) void sum_parts_kernel(SumJob ja, SumJob jb, int d, int nb_a) {
    const bool first = (int)blockIdx.x < nb_a;
    const SumJob& j = first ? ja : jb;
    const int64_t t = (int64_t)(blockIdx.x - (first ? 0 : nb_a)) * 256 + threadIdx.x;   // one float4 each
    const int64_t per_row = d / 4;
    if (t >= j.rows * per_row) return;
    const int64_t r = t / per_row, cidx = t % per_row;
    f32x4 acc = reinterpret_cast<const f32x4*>(j.dpart + r * d)[cidx];
    float rs = j.rpart[r];
    for (int s = 1; s < j.nsplit; ++s) {
        acc += reinterpret_cast<const f32x4*>(j.dpart + ((int64_t)s * j.rows_p + r) * d)[cidx];
        rs += j.rpart[(int64_t)s * j.rows_p + r];
    }
    const f32x4 xr = reinterpret_cast<const f32x4*>(j.X + r * d)[cidx];
    reinterpret_cast<f32x4*>(j.out + r * d)[cidx] = acc - rs * xr;
}

// The same for the distinct-column sweeps (mf_loss_cols.h): the split counts and dV's row stride come from the device words,
// the diagonal term -- no longer patched inside the sweeps -- is added here, and dV is written for ALL N original columns,
// each taking the partials of its representative's slot k = rank[j] (a copy holds ~first: rank[first] is its slot):
//   dU row i: acc = sum_s dpart[s][i] + xd_i v[i],    rs = sum_s rpart[s][i] + xd_i,    out = acc - rs u[i]
//   dV row j: acc = sum_s dpart_v[s][k] (+ xd_j u[j]), rs = sum_s rpart_v[s][k] (+ xd_j), out = acc - rs v[j]     (j < B)
// with xd = grad_out * rowc[3 Bp + .].  Fixed split order, no float atomics.
struct SumColsParams {
    const float *dpart, *rpart, *dpart_v, *rpart_v, *u, *v, *rowc, *grad_out;
    const int32_t *geo, *rank;
    int64_t B, N, Bp;
    float *du, *dv;
    int nb_a, xb;
};
__global__ __launch_bounds__(256) void sum_parts_cols_kernel(SumColsParams p, int d) {
    const bool first = (int)blockIdx.x < p.nb_a;
    const int64_t t = (int64_t)(blockIdx.x - (first ? 0 : p.nb_a)) * 256 + threadIdx.x;   // one float4 each
    const int64_t per_row = d / 4;
    if (t >= (first ? p.B : p.N) * per_row) return;
    const int64_t r = t / per_row, cidx = t % per_row;
    int64_t row = r, stride = p.Bp;
    int nsplit = p.geo[CG_NSU];
    if (!first) {
        int32_t k = p.rank[r];
        if (k < 0) k = p.rank[~k];
        row = k; stride = (int64_t)p.geo[CG_XBV] * p.xb; nsplit = p.geo[CG_NSV];
    }
    const float* dpart = first ? p.dpart : p.dpart_v;
    const float* rpart = first ? p.rpart : p.rpart_v;
    f32x4 acc = reinterpret_cast<const f32x4*>(dpart + row * d)[cidx];
    float rs = rpart[row];
    for (int s = 1; s < nsplit; ++s) {
        acc += reinterpret_cast<const f32x4*>(dpart + ((int64_t)s * stride + row) * d)[cidx];
        rs += rpart[(int64_t)s * stride + row];
    }
    const f32x4 xr = reinterpret_cast<const f32x4*>((first ? p.u : p.v) + r * d)[cidx];
    if (r < p.B) {
        const float xd = p.grad_out[0] * p.rowc[3 * p.Bp + r];
        acc += xd * reinterpret_cast<const f32x4*>((first ? p.v : p.u) + r * d)[cidx];
        rs += xd;
    }
    reinterpret_cast<f32x4*>((first ? p.du : p.dv) + r * d)[cidx] = acc - rs * xr;
}

template <int D, bool XU, int GMODE, bool CP, int SPLIT>
static void launch_bwd_g(dim3 grid, const BwdParams& bp, hipStream_t s) {
    auto fn = loss_bwd_dense_kernel<D, XU, GMODE, CP, SPLIT>;
    using L = BwdLds<D, XU, SPLIT>;
    if (L::BYTES > 64 * 1024) (void)hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, L::BYTES);
    fn<<<grid, 64 * mf_nw(D), L::BYTES, s>>>(bp);
}
template <int D, bool XU, bool CP = false, int SPLIT = 0>
static void launch_bwd(int gmode, dim3 grid, const BwdParams& bp, hipStream_t s) {
    if (gmode == G_EXP) launch_bwd_g<D, XU, G_EXP, CP, SPLIT>(grid, bp, s);
    else if (gmode == G_STEP) launch_bwd_g<D, XU, G_STEP, CP, SPLIT>(grid, bp, s);
    else launch_bwd_g<D, XU, G_SIGM, CP, SPLIT>(grid, bp, s);
}

// ---- the split sweeps' operand images and switch (mf_bf_split.h) ----
// One launch, inside the backward: the images of u (dV streams it) and of v, or of the packed v' (dU).  A workgroup is one
// tile; thread (k-step s, lane (r, h)) reads features 4 r .. 4 r + 3 of the 8 rows its fragment holds -- whole 512-byte rows
// across r -- and writes the 16-byte fragments of 3 pieces x 4 blocks.  Rows from `rows` on are zeros.
struct SplitImage {
    const float* src;
    int64_t rows;
    int tiles;
    unsigned short* img;
};
__global__ __launch_bounds__(128) void bwd_split_image_kernel(SplitImage ja, SplitImage jb, const int32_t* __restrict__ geo) {
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
    const bool first = (int)blockIdx.x < ja.tiles;
    const SplitImage& job = first ? ja : jb;
    const int tile = (int)blockIdx.x - (first ? 0 : ja.tiles);
    if (!first && geo && tile >= geo[CG_NT]) return;          // (packed v': the sweeps stream the tiles of N' only)
    const int s = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    u16x8 out[3][4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t y = (int64_t)tile * 32 + (j & 3) + 8 * (2 * s + (j >> 2)) + 4 * h;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (y < job.rows) x = reinterpret_cast<const f32x4*>(job.src + y * 128)[r];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            unsigned short o[3];
            mbf_split3(x[b], o);
            out[0][b][j] = o[0]; out[1][b][j] = o[1]; out[2][b][j] = o[2];
        }
    }
    u16x8* dst = reinterpret_cast<u16x8*>(job.img + (int64_t)tile * BSI_TILE_ELEMS);
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int b = 0; b < 4; ++b) dst[bsi_index(16 * s + 4 * h, 4 * r + b, q) >> 3] = out[q][b];
}
// tests only: slot of (row of the tile, feature, piece) in a tile's image
extern "C" int mf_bwd_split_image_index(int row, int feature, int piece) {
    if (row < 0 || row >= 32 || feature < 0 || feature >= 128 || piece < 0 || piece >= 3) return -1;
    return bsi_index(row, feature, piece);
}

// 0 never, 1 where it pays (default: from SPLIT_MIN_N columns upward), 2 wherever it can serve (tests).  Served: the dense
// (unmined) backward at d = 128, with or without the column plan.  Below the threshold a sweep's workgroup streams a few tiles
// and the image launch is not paid back: forward + backward in us, fp32 / split -- (B, N) = (1024, 4096): 123.1 / 124.7,
// (2048, 4096): 121.9 / 121.5, (4096, 8192): 192.8 / 174.5 (profiles/bwd_split_threshold.json).
static int g_dense_bwd_split = 1;
static constexpr int64_t SPLIT_MIN_N = 8192;
extern "C" void mf_set_dense_bwd_split(int mode) { g_dense_bwd_split = mode <= 0 ? 0 : (mode >= 2 ? 2 : 1); }
static bool split_serve(const LossWs& w) {
    if (!w.split_ok || g_dense_bwd_split == 0) return false;
    return g_dense_bwd_split == 2 || w.N >= SPLIT_MIN_N;
}
// which path the last backward on a workspace took (tests and tools): bit 0 distinct columns, 1 split contraction, 2 dV recomputed G'
static std::mutex g_path_mu;
static std::unordered_map<const void*, int> g_bwd_path;
extern "C" int mf_loss_bwd_path(const void* ws) {
    std::lock_guard<std::mutex> lk(g_path_mu);
    const auto it = g_bwd_path.find(ws);
    return it == g_bwd_path.end() ? 0 : it->second;
}
static void bwd_path_note(const void* ws, int path) {
    std::lock_guard<std::mutex> lk(g_path_mu);
    g_bwd_path[ws] = path;
}
void dense_bwd_none(const void* ws) { bwd_path_note(ws, 0); }

// The forward's own switch: 0 never, 1 where it pays (default: from FWD_SPLIT_MIN_BN scores upward), 2 wherever d = 128 and
// the loss is dense (tests).  Separate from the backward's: a backward reads the logit stash whichever way the forward filled
// it.  The image launch is paid back once the sweep has enough tiles: forward + backward in us, fp32 forward / split forward
// -- (B, N) = (1024, 4096): 139.9 / 139.4 (inside the spread), (2048, 4096): 154.8 / 150.6, (4096, 8192): 279.7 / 251.5,
// (8192, 16384): 844.1 / 726.2 (profiles/fwd_split_threshold.json).
static int g_dense_fwd_split = 1;
static constexpr int64_t FWD_SPLIT_MIN_BN = (int64_t)2048 * 4096;
extern "C" void mf_set_dense_fwd_split(int mode) { g_dense_fwd_split = mode <= 0 ? 0 : (mode >= 2 ? 2 : 1); }
static bool fwd_split_serve(const LossWs& w) {
    if (!w.split_ok || g_dense_fwd_split == 0) return false;
    return g_dense_fwd_split == 2 || w.B * w.N >= FWD_SPLIT_MIN_BN;
}
// which path the last forward on a workspace took (tests and tools): bit 0 distinct columns, bit 1 split scores; 0 for a
// forward that ran no dense sweep
static std::unordered_map<const void*, int> g_fwd_path;
extern "C" int mf_loss_fwd_path(const void* ws) {
    std::lock_guard<std::mutex> lk(g_path_mu);
    const auto it = g_fwd_path.find(ws);
    return it == g_fwd_path.end() ? 0 : it->second;
}
static void fwd_path_note(const void* ws, int path) {
    std::lock_guard<std::mutex> lk(g_path_mu);
    g_fwd_path[ws] = path;
}

// ---- the distinct-column sweeps' switch (mf_loss_cols.h) ----
// 0 never, 1 where it pays (default), 2 wherever it can serve (tests).  Served: the dense (unmined) path at d = 128, all
// seven kinds, masks built inside the forward, no mask export; mode 1 from COLS_MIN_N columns upward.
static int g_dense_dedup = 1;
static constexpr int64_t COLS_MIN_N = 4096;
extern "C" void mf_set_dense_dedup(int mode) { g_dense_dedup = mode <= 0 ? 0 : (mode >= 2 ? 2 : 1); }
static bool cols_serve(const LossWs& w, bool masks_ready, bool export_masks) {
    if (!w.cols_ok || masks_ready || export_masks || g_dense_dedup == 0) return false;
    return g_dense_dedup == 2 || w.N >= COLS_MIN_N;
}
// Which path the LAST forward on a workspace took: its backward must contract the stashes that forward wrote, whatever the
// switch says by then (and the backward's arguments do not tell, e.g., that the masks had been prepared ahead).
static std::mutex g_cols_mu;
static std::unordered_map<const void*, bool> g_cols_served;
static void cols_note(const void* ws, bool served) {
    std::lock_guard<std::mutex> lk(g_cols_mu);
    g_cols_served[ws] = served;
}
static bool cols_served(const void* ws) {
    std::lock_guard<std::mutex> lk(g_cols_mu);
    const auto it = g_cols_served.find(ws);
    return it != g_cols_served.end() && it->second;
}

// tests and tools only (a device -> host copy: never inside a step): out[9] = {served, N', NT', forward (nsplit, tps),
// dU (nsplit, tps), dV (nsplit, tps)} of the last forward on this workspace; not served: the rest is 0
extern "C" int mf_loss_cols_info(const void* ws, int64_t* out9) {
    if (!ws || !out9) return mf_set_error(MF_EINVAL, "mf_loss_cols_info: bad argument");
    for (int i = 0; i < 9; ++i) out9[i] = 0;
    if (!cols_served(ws)) return MF_OK;
    int32_t g[CG_WORDS];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(g, ws, sizeof(g), hipMemcpyDeviceToHost) != hipSuccess)
        return mf_set_error(MF_ELAUNCH, "mf_loss_cols_info: copy failed");
    out9[0] = 1;
    for (int i = 0; i < 8; ++i) out9[1 + i] = g[i];
    return MF_OK;
}
// host-only: the geometry the device derives for `ncols` distinct columns of this shape, and what is launched and allocated
// around it: out[16] = {can serve, NT', forward (nsplit, tps), dU (nsplit, tps), dV (nsplit, tps), dV X blocks,
// launched: forward splits, dU splits, dV workgroups, capacity: forward partial splits, dU partial splits, dV partial X blocks, 0}
extern "C" int mf_loss_cols_plan(int64_t B, int64_t N, int d, int64_t ncols, int64_t* out16) {
    if (!out16) return mf_set_error(MF_EINVAL, "mf_loss_cols_plan: out is NULL");
    if (B <= 0 || N < B || ncols < 1 || ncols > N || !mf_width_ok(d))
        return mf_set_error(MF_EINVAL, "mf_loss_cols_plan: need 0 < B <= N, 1 <= ncols <= N and a supported width");
    const LossWs w = loss_ws(nullptr, B, N, d, 0);
    const ColsGeom g = cols_geometry(w.BT, w.NT, w.NW, ncols, w.wgs_f, w.wgs_b);
    const size_t xb = (size_t)32 * w.NW;
    size_t rows_v = (size_t)w.nsplit_v * w.Np;
    if ((size_t)w.cl.grid_v * xb > rows_v) rows_v = (size_t)w.cl.grid_v * xb;
    const int64_t o[16] = {w.cols_ok ? 1 : 0, g.nt, g.nsf, g.tpsf, g.nsu, g.tpsu, g.nsv, g.tpsv, g.xbv,
                           w.cl.grid_f, w.cl.grid_u, w.cl.grid_v, w.cl.grid_f, w.cl.grid_u, (int64_t)(rows_v / xb), 0};
    for (int i = 0; i < 16; ++i) out16[i] = o[i];
    return MF_OK;
}

// the plan behind build_masks' table and first-column kernels: kept columns, their slots, the packed side arrays, the
// geometry words; then the mask words of the PACKED columns (mask_sweep_kernel fed first')
template <int D>
static void cols_plan_launch(const LossWs& w, const float* v, int planes, hipStream_t s) {
    const int64_t N = w.N;
    cols_mark_kernel<D><<<dim3((unsigned)w.NT), 1024, 0, s>>>(v, w.logq, w.colfirst, N, w.ckept, w.ctcnt);
    const ColsPack cp{v, w.nv, w.logq, w.colfirst, w.ckept, w.ctcnt, N, w.Np, w.NT, w.BT, w.NW, w.wgs_f, w.wgs_b,
                      w.crank, w.cfirst, w.geo, w.ccnt, w.cnv, w.clq};
    cols_pack_kernel<D><<<dim3((unsigned)((w.Np + 1023) / 1024)), 1024, 0, s>>>(cp);
    cols_rows_kernel<D><<<dim3((unsigned)w.NT), 1024, 0, s>>>(v, w.crank, w.ccnt, w.geo, N, w.cv, w.cw);
    loss_sweep_masks(w, w.cfirst, planes, s);
}

bool dense_fwd_cols(const LossWs& w, const void* ws, bool scores_needed, bool masks_ready, bool export_masks) {
    const bool cols = scores_needed && cols_serve(w, masks_ready, export_masks);
    cols_note(ws, cols);
    fwd_path_note(ws, 0);               // (dense_fwd, if this forward reaches it, records what it launched)
    return cols;
}

int dense_fwd(const LossWs& w, const void* ws, bool cols, int planes, const float* u, const float* v, int need, float sigma, float margin,
              uint32_t* out_mask_bits, hipStream_t s, int* merge_splits) {
    const int64_t B = w.B, N = w.N;
    const int d = w.d;
    if (cols) cols_plan_launch<128>(w, v, planes, s);
    // logq is read by whole float4s up to the padded width: prep_kernel keeps a zero-padded copy in ws
    // (all zeros when there is no logQ correction: L - 0 is exact, and the kernels stay branch-free)
    FwdParams fp{u, v, w.nu, w.nv, w.lii, w.sgn, w.logq, w.maskW, w.part, w.stash, B, N, w.Bp, w.NT, w.tps_f, need, sigma, margin};
    if (cols) { fp.v = w.cv; fp.nv = w.cnv; fp.logq = w.clq; fp.N = w.Np; fp.geo = w.geo; }
    if (!fwd_aux_span(fp, w, cols ? w.cw : nullptr))
        return mf_set_error(MF_EINVAL, "mf_loss_fwd: batch x catalog too large for one sweep (mask words beyond 4 GiB)");
    const bool split = fwd_split_serve(w);
    fwd_path_note(ws, (cols ? 1 : 0) | (split ? 2 : 0));
    if (split) {
        // The image of the streamed tiles, once per forward, where the backward's image of the same operand will go (inside the
        // G' stash wherever that fits: nothing uses those bytes until the backward, whose own image launch may overwrite it).
        fp.img = w.bimg_v;
        fwd_split_image_kernel<<<dim3((unsigned)w.NT), 512, 0, s>>>(fp.v, cols ? w.Np : N, w.bimg_v, cols ? w.geo : nullptr);
    }
    if (cols) {
        // launched for the most splits any N' can ask for; a split beyond N''s writes the empty statistics, which merge as nothing
        dim3 grid((unsigned)w.cl.grid_f, (unsigned)(w.BT / w.NW));
        if (split) MF_TIMED("loss_fwd_dense", s, (launch_fwd<128, true, true>(need, grid, fp, s)));
        else MF_TIMED("loss_fwd_dense", s, (launch_fwd<128, true>(need, grid, fp, s)));
        *merge_splits = w.cl.grid_f;
    } else if (split) {
        dim3 grid((unsigned)w.nsplit_f, (unsigned)(w.BT / w.NW));
        MF_TIMED("loss_fwd_dense", s, (launch_fwd<128, false, true>(need, grid, fp, s)));
        *merge_splits = w.nsplit_f;
    } else {
        MF_DISPATCH_D(d, {
            dim3 grid((unsigned)w.nsplit_f, (unsigned)(w.BT / w.NW));
            MF_TIMED("loss_fwd_dense", s, (launch_fwd<D>(need, grid, fp, s)));
        });
        *merge_splits = w.nsplit_f;
    }
    if (out_mask_bits)
        mask_export_dense_kernel<<<dim3((unsigned)((B * ((N + 31) / 32) + 255) / 256)), 256, 0, s>>>(w.maskW, B, N, w.Bp, (int)((N + 31) / 32), out_mask_bits);
    return MF_OK;
}

int dense_bwd(const LossWs& w, const void* ws, int gmode, const float* u, const float* v, const float* grad_out, float* du,
              float* dv, hipStream_t s) {
    const int64_t B = w.B, N = w.N;
    const int d = w.d;
    const bool cols = cols_served(ws), split = split_serve(w);
    bwd_path_note(ws, (cols ? 1 : 0) | (split ? 2 | 4 : 0));
    if (split) {
        // (tile shares of a split sweep are checked against the descriptor by split_ok: the whole image fits one)
        const SplitImage ju{u, B, w.BT, w.bimg_u}, jv{cols ? w.cv : v, cols ? w.Np : N, w.NT, w.bimg_v};
        bwd_split_image_kernel<<<dim3((unsigned)(w.BT + w.NT)), 128, 0, s>>>(ju, jv, cols ? w.geo : nullptr);
    }
    if (cols) {
        // the forward on this workspace swept the distinct columns: so do dU and dV (the stashes hold packed columns)
        BwdParams bp{u, w.cv, w.rowc, grad_out, w.stash, w.gstash, w.dpart, w.rpart, B, w.Np, w.Bp, w.Np, w.NT, 0, 0, w.geo, w.cw};
        const dim3 grid_u((unsigned)w.cl.grid_u, (unsigned)(w.BT / w.NW)), grid_v((unsigned)w.cl.grid_v);
        bp.YT = w.NT; bp.img = w.bimg_v;
        if (split) MF_TIMED("loss_bwd_du", s, (launch_bwd<128, true, true, 1>(gmode, grid_u, bp, s)));
        else MF_TIMED("loss_bwd_du", s, (launch_bwd<128, true, true>(gmode, grid_u, bp, s)));
        bp.YT = w.BT; bp.dpart = w.dpart_v; bp.rpart = w.rpart_v; bp.img = w.bimg_u;
        if (split) MF_TIMED("loss_bwd_dv", s, (launch_bwd<128, false, true, 1>(gmode, grid_v, bp, s)));
        else MF_TIMED("loss_bwd_dv", s, (launch_bwd<128, false, true>(G_EXP, grid_v, bp, s)));
        const int nb_a = (int)((B * (d / 4) + 255) / 256), nb_b = (int)((N * (d / 4) + 255) / 256);
        const SumColsParams sp{w.dpart, w.rpart, w.dpart_v, w.rpart_v, u, v, w.rowc, grad_out, w.geo, w.crank, B, N, w.Bp, du, dv, nb_a, 32 * w.NW};
        sum_parts_cols_kernel<<<dim3((unsigned)(nb_a + nb_b)), 256, 0, s>>>(sp, d);
        return MF_OK;
    }
    if ((size_t)w.tps_u * 32 * d * 4 > MF_SRD_MAX_BYTES || (size_t)w.tps_v * 32 * d * 4 > MF_SRD_MAX_BYTES)
        return mf_set_error(MF_ENOTSUP, "mf_loss_bwd: a sweep's share of the batch exceeds 4 GiB (buffer descriptor)");
    BwdParams bp{u, v, w.rowc, grad_out, w.stash, w.gstash, w.dpart, w.rpart, B, N, w.Bp, w.Np, w.NT, 0, 0, nullptr, nullptr};
    if (split) {
        bp.YT = w.NT; bp.tps = w.tps_u; bp.img = w.bimg_v;
        MF_TIMED("loss_bwd_du", s, (launch_bwd<128, true, false, 1>(gmode, dim3((unsigned)w.nsplit_u, (unsigned)(w.BT / w.NW)), bp, s)));
        bp.YT = w.BT; bp.tps = w.tps_v; bp.dpart = w.dpart_v; bp.rpart = w.rpart_v; bp.img = w.bimg_u;
        MF_TIMED("loss_bwd_dv", s, (launch_bwd<128, false, false, 1>(gmode, dim3((unsigned)w.nsplit_v, (unsigned)(w.NT / w.NW)), bp, s)));
        const SumJob ja{w.dpart, w.rpart, u, w.nsplit_u, B, w.Bp, du}, jb{w.dpart_v, w.rpart_v, v, w.nsplit_v, N, w.Np, dv};
        const int nb_a = (int)((B * (128 / 4) + 255) / 256), nb_b = (int)((N * (128 / 4) + 255) / 256);
        sum_parts_kernel<<<dim3((unsigned)(nb_a + nb_b)), 256, 0, s>>>(ja, jb, 128, nb_a);
        return MF_OK;
    }
    MF_DISPATCH_D(d, {
        bp.YT = w.NT; bp.tps = w.tps_u;
        MF_TIMED("loss_bwd_du", s, (launch_bwd<D, true>(gmode, dim3((unsigned)w.nsplit_u, (unsigned)(w.BT / w.NW)), bp, s)));
        bp.YT = w.BT; bp.tps = w.tps_v; bp.dpart = w.dpart_v; bp.rpart = w.rpart_v;
        MF_TIMED("loss_bwd_dv", s, (launch_bwd<D, false>(D == 64 ? gmode : G_EXP, dim3((unsigned)w.nsplit_v, (unsigned)(w.NT / w.NW)), bp, s)));
        const SumJob ja{w.dpart, w.rpart, u, w.nsplit_u, B, w.Bp, du}, jb{w.dpart_v, w.rpart_v, v, w.nsplit_v, N, w.Np, dv};
        const int nb_a = (int)((B * (D / 4) + 255) / 256), nb_b = (int)((N * (D / 4) + 255) / 256);
        sum_parts_kernel<<<dim3((unsigned)(nb_a + nb_b)), 256, 0, s>>>(ja, jb, D, nb_a);
    });
    return MF_OK;
}
