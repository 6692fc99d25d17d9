// mf_loss.hip -- the in-batch score matrix and the seven xfmr_rec/losses.py losses,
// forward and backward, without ever materialising the B x N logits or the
// B x N x P positive-mask temp of the reference (xfmr_rec/losses.py:108).
//
// Pipeline (all on the caller's stream, no allocation, no sync):
//   fwd : chain norms -> diagonal (L_ii) -> sort item ids -> hit bitmask
//         (B x N BITS, both orientations) ->
//           dense : score tiles + per-row statistics (split over item ranges)
//           mined : streaming per-row top-k of mining keys -> merge -> statistics
//         -> per-row losses -> fixed-order reduction to the 7 scalars
//   bwd : per-row coefficients of dloss/dL -> dense: dU pass + dV pass (each a
//         recompute-and-contract sweep over score tiles), or mined: sparse rows.
//
// This unit holds the set-up (prep_kernel), the tail (finish / rowc / diag_bwd), the argument checks and the two
// orchestration functions; the stages between are mf_loss_masks.hip, mf_loss_dense.hip and mf_loss_mined.hip, called
// through the host functions of mf_loss_ws.h (which also lays out the workspace).
//
// Reference restated: negative_masks :92-110, semi_hard_mining :134-162,
// alignment/contrastive/infonce/mine :164-246, pairwise :324-359, reduction
// `(loss * target.abs()).sum()`.  Formulas: SURVEY.md Appendix A.
#include "mf_loss_ws.h"

extern "C" size_t mf_loss_ws_bytes(int64_t B, int64_t N, int d, int P, int num_negatives) {
    if (B <= 0 || N < B) return 0;
    (void)P;                               // (the positives are looked up, not copied: their width does not size anything)
    return loss_ws(nullptr, B, N, d, num_negatives).total;
}

// host-only: the split geometry of the three dense sweeps for a shape, as the launches would use it (nothing is launched)
extern "C" int mf_loss_plan(int64_t B, int64_t N, int d, int num_negatives, int64_t* out8) {
    if (!out8) return mf_set_error(MF_EINVAL, "mf_loss_plan: out is NULL");
    if (B <= 0 || N < B) return mf_set_error(MF_EINVAL, "mf_loss_plan: need 0 < B <= N (B=%lld N=%lld)", (long long)B, (long long)N);
    if (!mf_width_ok(d)) return mf_set_error(MF_EINVAL, "mf_loss_plan: embedding width %d not in {32,64,128,256}", d);
    const LossWs w = loss_ws(nullptr, B, N, d, num_negatives);
    const int64_t last_f = w.NT - (int64_t)(w.nsplit_f - 1) * w.tps_f, last_u = w.NT - (int64_t)(w.nsplit_u - 1) * w.tps_u,
                  last_v = w.BT - (int64_t)(w.nsplit_v - 1) * w.tps_v;
    const int64_t o[8] = {w.mined ? 1 : 0, w.nsplit_f, w.tps_f, w.nsplit_u, w.tps_u, w.nsplit_v, w.tps_v,
                          last_f | (last_u << 20) | (last_v << 40)};     // (a split holds < 2^19 tiles: N < 2^24)
    for (int i = 0; i < 8; ++i) out8[i] = o[i];
    return MF_OK;
}

// ------------------------------------------------------------- per-call setup ---
// ONE launch for everything the sweeps need that is O(B + N): chain norms of both operands, the
// diagonal (L_ii, D_ii, sign), the zero-padded logQ copy, and the clearing of the hash table, the
// per-user bit rows and the reduction ticket.  (Each of these used to be its own ~5 us launch.)
struct PrepParams {
    const float *u, *v;
    const void* target;
    const float* logq;
    const int64_t* item_idx;      // logq_rows > 0: logq is a table looked up by these ids
    int64_t logq_rows;
    int target_i64;
    int64_t B, N, Bp, Np;
    int d;
    float sigma;
    float *nu, *nv, *lii, *dii, *sgn, *wlogq, *wtgt;
    // fills, in 16-byte units (0 = skip): the hash table (0x80..), the first-column table (0x7f..), and to zero a range
    // the caller names (the column plan's copy counts, or the mined path's counters) and the membership bitmap
    uint4* table; int64_t table16;
    uint4* first; int64_t first16;
    uint4* zero; int64_t zero16;
    uint4* bitmap; int64_t bitmap16;
    unsigned* ticket;
};

__device__ __forceinline__ void fill16(uint4* dst, int64_t n16, unsigned pat, int64_t tid, int64_t nthreads) {
    const uint4 v = {pat, pat, pat, pat};
    for (int64_t q = tid; q < n16; q += nthreads) dst[q] = v;
}

// 64-thread workgroups: the per-row chains are serial, so the rows are spread over as many CUs as possible.
// D = 0: no rows (clears only).  The rows come in batches of 32 floats per operand (16 loads in flight per thread).
template <int D>
__global__ __launch_bounds__(64) void prep_kernel(PrepParams p) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (D > 0 && i < p.Np) {
        const bool hv = i < p.N, hu = i < p.B;                  // B <= N: a user row always has its item row
        float nvv = 0.f, nuu = 0.f, dot = 0.f;
        if (hv) {
            const f32x4* pv = reinterpret_cast<const f32x4*>(p.v + i * D);
            const f32x4* pu = reinterpret_cast<const f32x4*>(p.u + (hu ? i : 0) * D);     // (no user: row 0 is read and dropped)
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            // batches of 16 loads; at most 4 batches (64 registers x 4) are in flight at once: fully unrolled, d = 256
            // asked for 8 batches' worth of registers and spilled 396 of them
            constexpr int PREP_UNROLL = D / 32 <= 4 ? (D / 32 > 0 ? D / 32 : 1) : 2;
#pragma unroll PREP_UNROLL
            for (int g0 = 0; g0 < D / 8; g0 += 4) {
                f32x4 va[8], ua[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) { va[j] = pv[2 * g0 + j]; ua[j] = pu[2 * g0 + j]; }
#pragma unroll
                for (int g = 0; g < 4; ++g) {                   // k order of mf_dot_chain
                    const f32x4 a = va[2 * g], b = va[2 * g + 1];
                    const f32x4 xa = hu ? ua[2 * g] : zero4, xb = hu ? ua[2 * g + 1] : zero4;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        nvv = __builtin_fmaf(a[t], a[t], nvv);  nvv = __builtin_fmaf(b[t], b[t], nvv);
                        nuu = __builtin_fmaf(xa[t], xa[t], nuu); nuu = __builtin_fmaf(xb[t], xb[t], nuu);
                        dot = __builtin_fmaf(xa[t], a[t], dot);  dot = __builtin_fmaf(xb[t], b[t], dot);
                    }
                }
            }
        }
        p.nv[i] = nvv;
        float lq = 0.f;
        if (p.logq && hv) {
            if (p.logq_rows > 0) {
                const int64_t id = p.item_idx[i];
                lq = (id >= 0 && id < p.logq_rows) ? p.logq[id] : 0.f;
            } else {
                lq = p.logq[i];
            }
        }
        p.wlogq[i] = -lq;                 // the sweeps read -logq (one fma operand, no negation in the loop)
        if (i < p.Bp) {
            float l = 0.f, dd = 0.f, sg = 0.f;
            float tg = 0.f;
            if (hu) {
                tg = p.target_i64 ? (float)static_cast<const int64_t*>(p.target)[i] : static_cast<const float*>(p.target)[i];
                sg = mf_sign(tg);
                dd = mf_half_sqdist(nuu, nvv, dot);
                l = mf_logit(nuu, nvv, dot, sg, p.sigma, lq);
            }
            p.nu[i] = nuu; p.lii[i] = l; p.dii[i] = dd; p.sgn[i] = sg; p.wtgt[i] = tg;
        }
    }
    if (i == 0) *p.ticket = 0u;
    const int64_t nthreads = (int64_t)gridDim.x * 64;
    fill16(p.table, p.table16, 0x80808080u, i, nthreads);
    fill16(p.first, p.first16, 0x7f7f7f7fu, i, nthreads);
    fill16(p.zero, p.zero16, 0u, i, nthreads);
    fill16(p.bitmap, p.bitmap16, 0u, i, nthreads);
}

// The tail of the forward in ONE launch: merge the item-range splits of the row statistics in split
// order (nsplit = 0: `stats` is already final), evaluate the seven per-row losses, and sum them over
// the batch in a fixed order: in-block tree, then the last workgroup to finish (ticket) adds the
// block sums in block order -- deterministic, no second launch.
__global__ __launch_bounds__(64) void finish_kernel(const float* __restrict__ part, int nsplit, int64_t B, int64_t Bp,
                                                     const float* __restrict__ target, const float* __restrict__ lii,
                                                     const float* __restrict__ dii, float sigma, int kind_mask,
                                                     float* __restrict__ stats, float* __restrict__ rowloss,
                                                     float* __restrict__ blockpart, unsigned* __restrict__ ticket,
                                                     float* __restrict__ out, int rowc_kind, float margin,
                                                     const float* __restrict__ sgn, float* __restrict__ rowc) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    float acc[NSTAT];
    if (i < Bp) {
        if (nsplit > 0) {
            for (int s = 0; s < NSTAT; ++s) acc[s] = part[(int64_t)s * Bp + i];
            for (int sp0 = 1; sp0 < nsplit; sp0 += 7) {             // seven splits' loads in flight, merged in order
                float q[7][NSTAT];
#pragma unroll
                for (int j = 0; j < 7; ++j)
#pragma unroll
                    for (int s = 0; s < NSTAT; ++s)
                        q[j][s] = sp0 + j < nsplit ? part[((int64_t)(sp0 + j) * NSTAT + s) * Bp + i] : 0.f;
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    if (sp0 + j >= nsplit) break;
                    lse_merge(acc[ST_MX], acc[ST_SE], q[j][ST_MX], q[j][ST_SE]);
                    acc[ST_CNT] += q[j][ST_CNT]; acc[ST_A] += q[j][ST_A]; acc[ST_H] += q[j][ST_H];
                    acc[ST_HC] += q[j][ST_HC]; acc[ST_LG] += q[j][ST_LG]; acc[ST_LS] += q[j][ST_LS];
                }
            }
            for (int s = 0; s < NSTAT; ++s) stats[(int64_t)s * Bp + i] = acc[s];
        } else {
            for (int s = 0; s < NSTAT; ++s) acc[s] = stats[(int64_t)s * Bp + i];
        }
    }
    float o[MF_NUM_KINDS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < B) row_losses(acc, target[i], lii[i], dii[i], sigma, o);
    if (rowc_kind >= 0 && i < Bp) {       // the backward's row coefficients of the one trained loss (MF_LOSS_ROWC)
        float a = 0.f, b = 0.f, cg = 0.f, gd = 0.f;
        if (i < B) rowc_row(rowc_kind, target[i], sgn[i], lii[i], acc[ST_CNT], acc[ST_MX], acc[ST_SE], acc[ST_HC], acc[ST_LS],
                            sigma, margin, a, b, cg, gd);
        rowc[i] = a; rowc[Bp + i] = b; rowc[2 * Bp + i] = cg; rowc[3 * Bp + i] = gd;
    }
    // one wave per workgroup: the block sum is a fixed xor tree over the lanes (no LDS, no barrier)
    const int lane = mf_lane();
    for (int k = 0; k < MF_NUM_KINDS; ++k) {
        if (i < Bp) rowloss[(int64_t)k * Bp + i] = o[k];
        float v = o[k];
        v = mf_wave_sum(v);
        if (lane == 0) blockpart[(int64_t)k * gridDim.x + blockIdx.x] = v;
    }
    // release only (the block sums are in L2 before the ticket moves): a full fence also invalidates the L1, ~1.7 us each;
    // the last workgroup reads the sums with L1-bypassing loads instead of an acquire fence
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    int last = 0;
    if (lane == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    last = __shfl(last, 0, 64);
    if (last) {
        // the last workgroup adds the block sums of every loss kind: lane-strided partial sums, then a fixed
        // xor tree -- the same order on every run
        float tot[MF_NUM_KINDS];
#pragma unroll
        for (int k = 0; k < MF_NUM_KINDS; ++k) tot[k] = 0.f;
        for (unsigned b = lane; b < gridDim.x; b += 64) {       // the seven kinds' loads of a round are in flight together
            float v[MF_NUM_KINDS];
#pragma unroll
            for (int k = 0; k < MF_NUM_KINDS; ++k)
                v[k] = __hip_atomic_load(blockpart + (int64_t)k * gridDim.x + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < MF_NUM_KINDS; ++k) tot[k] += v[k];
        }
#pragma unroll
        for (int k = 0; k < MF_NUM_KINDS; ++k) {
            float t = tot[k];
            t = mf_wave_sum(t);
            if (lane == 0) out[k] = ((kind_mask >> k) & 1) ? t : 0.f;   // every entry is written
        }
    }
}

// ------------------------------------------------------------------ backward ---
__global__ __launch_bounds__(256) void rowc_kernel(const float* __restrict__ stats, const float* __restrict__ target,
                                                   const float* __restrict__ lii, const float* __restrict__ sgn,
                                                   int64_t B, int64_t Bp, int kind, float sigma, float margin,
                                                   float* __restrict__ rowc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Bp) return;
    float a = 0.f, b = 0.f, cg = 0.f, gd = 0.f;
    if (i < B)
        rowc_row(kind, target[i], sgn[i], lii[i], stats[ST_CNT * Bp + i], stats[ST_MX * Bp + i], stats[ST_SE * Bp + i],
                 stats[ST_HC * Bp + i], stats[ST_LS * Bp + i], sigma, margin, a, b, cg, gd);
    rowc[0 * Bp + i] = a; rowc[1 * Bp + i] = b; rowc[2 * Bp + i] = cg; rowc[3 * Bp + i] = gd;
}

// alignment-only backward: only the diagonal carries gradient
template <int D>
__global__ __launch_bounds__(256) void diag_bwd_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                       const float* __restrict__ rowc, const float* __restrict__ grad_out,
                                                       int64_t B, int64_t N, int64_t Bp,
                                                       float* __restrict__ du, float* __restrict__ dv) {
    constexpr int LPR = D / 4;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = t / LPR;
    const int c = (int)(t % LPR);
    if (r >= N) return;
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (r < B) {
        const float gd = grad_out[0] * rowc[3 * Bp + r];
        const f32x4 ui = reinterpret_cast<const f32x4*>(u + r * D)[c];
        const f32x4 vi = reinterpret_cast<const f32x4*>(v + r * D)[c];
        reinterpret_cast<f32x4*>(du + r * D)[c] = gd * (vi - ui);
        reinterpret_cast<f32x4*>(dv + r * D)[c] = gd * (ui - vi);
    } else {
        reinterpret_cast<f32x4*>(dv + r * D)[c] = z;
    }
}

// -------------------------------------------------------------- orchestration ---
// the fills that empty the mask build's tables (the hit rows are written whole: nothing to clear there)
static void prep_clears(PrepParams& pp, const LossWs& w) {
    pp.table = reinterpret_cast<uint4*>(w.gtab); pp.table16 = (int64_t)w.M * 8 / 16;
    pp.first = reinterpret_cast<uint4*>(w.gfirst); pp.first16 = (int64_t)w.M * 4 / 16;
    pp.bitmap = reinterpret_cast<uint4*>(w.bmap); pp.bitmap16 = ((int64_t)4 << (w.bmbits - 5)) / 16;
}
// workgroups of a prep launch: its rows (`nb`), or more where the fills ask for it (~8 stores per thread)
static unsigned prep_blocks(const PrepParams& pp, int64_t nb) {
    const int64_t want = (pp.table16 + pp.first16 + pp.zero16 + pp.bitmap16 + 64 * 8 - 1) / (64 * 8);
    if (want > nb) nb = want < 8192 ? want : 8192;
    return (unsigned)nb;
}

void loss_clear_tables(const LossWs& w, hipStream_t s) {
    PrepParams pp{};
    prep_clears(pp, w);
    pp.ticket = w.ticket;
    prep_kernel<0><<<dim3(prep_blocks(pp, 1)), 64, 0, s>>>(pp);
}

static int check_loss_args(const char* what, int64_t B, int64_t N, int d, int P, int num_negatives,
                           const void* u, const void* v, const void* target, void* ws, size_t ws_bytes) {
    if (int rc = loss_check_shape(what, B, N, d, P >= 0 && u && v && target && ws, true)) return rc;
    if (mining_on(num_negatives, N) && (num_negatives > KSEL_MAX || !mf_select_plan(B, N, d, num_negatives).ok))
        return mf_set_error(MF_ENOTSUP, "%s: mining with num_negatives = %d unsupported (max %d; 32 at d = 256)", what,
                            num_negatives, KSEL_MAX);
    if (ws_bytes < mf_loss_ws_bytes(B, N, d, P, num_negatives))
        return mf_set_error(MF_ENOSPC, "%s: workspace too small (%zu < %zu)", what, ws_bytes,
                            mf_loss_ws_bytes(B, N, d, P, num_negatives));
    return MF_OK;
}

static int loss_fwd_impl(const char* what, int64_t B, int64_t N, int d, const PosSrc& src, int num_negatives, float sigma, float margin,
                         int kind_mask, const float* u, const float* v, const void* target,
                         const int64_t* item_idx, const float* logq, int64_t logq_rows,
                         int flags, void* ws, size_t ws_bytes, float* out_losses, uint32_t* out_mask_bits,
                         mf_stream_t stream) {
    int rc = check_loss_args(what, B, N, d, 0, num_negatives, u, v, target, ws, ws_bytes);
    if (rc) return rc;
    const bool masks_ready = item_idx == nullptr || (flags & MF_LOSS_MASKS_READY);       // mf_loss_masks ran on this workspace
    if (!out_losses || !(kind_mask & 0x7F)) return mf_set_error(MF_EINVAL, "%s: bad argument", what);
    if (!masks_ready && (rc = pos_src_check(what, src))) return rc;
    if (logq && logq_rows > 0 && !item_idx) return mf_set_error(MF_EINVAL, "%s: a logQ table needs item_idx", what);
    int rowc_kind = -1;
    if (flags & MF_LOSS_ROWC) {
        if (__builtin_popcount(kind_mask & 0x7F) != 1) return mf_set_error(MF_EINVAL, "%s: MF_LOSS_ROWC needs exactly one loss kind", what);
        rowc_kind = __builtin_ctz(kind_mask & 0x7F);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const LossWs w = loss_ws(ws, B, N, d, num_negatives);
    const int need = need_flags(kind_mask);
    const bool scores_needed = (kind_mask & ~(1 << MF_ALIGNMENT)) != 0 || out_mask_bits;
    const bool build = scores_needed && !masks_ready;
    const bool cols = dense_fwd_cols(w, ws, scores_needed, masks_ready, out_mask_bits != nullptr);   // the distinct-column sweeps

    // 1. set-up: norms, diagonal, -logQ copy, and every clear the later stages want
    {
        PrepParams pp{u, v, target, logq, item_idx, logq_rows, (flags & MF_LOSS_TARGET_I64) ? 1 : 0,
                      B, N, w.Bp, w.Np, d, sigma, w.nu, w.nv, w.lii, w.dii, w.sgn, w.logq, w.tgt,
                      nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, w.ticket};
        if (build) prep_clears(pp, w);
        if (cols) { pp.zero = reinterpret_cast<uint4*>(w.ccnt); pp.zero16 = w.Np * 4 / 16; }      // the copy counts start at 0
        if (scores_needed && w.mined) {
            // the mined path's counters and bounds (gtau .. cand_cnt, and behind them the prefilter's maxima, copy bitmaps, spill
            // cursors and gate: one contiguous range of the workspace) are cleared here too -- it used to be a launch of its own
            pp.zero = reinterpret_cast<uint4*>(w.gtau);
            pp.zero16 = (int64_t)(((char*)(w.mbf.ok ? (void*)(w.mbf_gate + 4) : (void*)(w.mbf_max + MBF_MAXSLOTS * MBF_MAXSTRIDE)) - (char*)w.gtau) / 16);
        }
        const unsigned nb = prep_blocks(pp, (w.Np + 63) / 64);
        MF_DISPATCH_D(d, { prep_kernel<D><<<dim3(nb), 64, 0, s>>>(pp); });
    }
    // 2. hit masks (unless they were built ahead); 3. the scores of every valid negative, dense or mined; 4. the tail
    int planes = 0, merge_splits = 0;
    if (build) planes = loss_build_masks(w, item_idx, src, s, !cols);
    if (scores_needed && !w.mined) rc = dense_fwd(w, ws, cols, planes, u, v, need, sigma, margin, out_mask_bits, s, &merge_splits);
    else if (scores_needed) rc = mined_fwd(w, u, v, num_negatives, need, sigma, margin, out_mask_bits, s);
    else mf_zero_async(w.stats, (size_t)NSTAT * w.Bp * 4, s);
    if (rc) return rc;
    finish_kernel<<<dim3((unsigned)((w.Bp + 63) / 64)), 64, 0, s>>>(w.part, merge_splits, B, w.Bp, w.tgt, w.lii, w.dii,
                                                                                       sigma, kind_mask, w.stats, w.rowloss,
                                                                                       w.blockpart, w.ticket, out_losses,
                                                                                       rowc_kind, margin, w.sgn, w.rowc);
    return mf_check_launch(what);
}

extern "C" int mf_loss_fwd(int64_t B, int64_t N, int d, int P, int num_negatives, float sigma, float margin,
                           int kind_mask, const float* u, const float* v, const void* target,
                           const int64_t* item_idx, const int64_t* pos_idx, const float* logq, int64_t logq_rows,
                           int flags, void* ws, size_t ws_bytes, float* out_losses, uint32_t* out_mask_bits,
                           mf_stream_t stream) {
    const PosSrc src{pos_idx, P, nullptr, nullptr, nullptr, 0};
    return loss_fwd_impl("mf_loss_fwd", B, N, d, src, num_negatives, sigma, margin, kind_mask, u, v, target, item_idx, logq, logq_rows,
                         flags, ws, ws_bytes, out_losses, out_mask_bits, stream);
}

extern "C" int mf_loss_fwd_csr(int64_t B, int64_t N, int d, int num_negatives, float sigma, float margin,
                               int kind_mask, const float* u, const float* v, const void* target,
                               const int64_t* item_idx, const int64_t* user_ids, const int64_t* pos_off, const int64_t* pos_items,
                               int64_t num_users, const float* logq, int64_t logq_rows,
                               int flags, void* ws, size_t ws_bytes, float* out_losses, uint32_t* out_mask_bits,
                               mf_stream_t stream) {
    if (!pos_off && !(item_idx == nullptr || (flags & MF_LOSS_MASKS_READY))) return mf_set_error(MF_EINVAL, "mf_loss_fwd_csr: pos_off is NULL");
    const PosSrc src{nullptr, 0, user_ids, pos_off, pos_items, num_users};
    return loss_fwd_impl("mf_loss_fwd_csr", B, N, d, src, num_negatives, sigma, margin, kind_mask, u, v, target, item_idx, logq, logq_rows,
                         flags, ws, ws_bytes, out_losses, out_mask_bits, stream);
}

extern "C" int mf_loss_bwd(int64_t B, int64_t N, int d, int P, int num_negatives, float sigma, float margin,
                           int kind, const float* u, const float* v, int flags, void* ws, size_t ws_bytes,
                           const float* grad_out, float* du, float* dv, mf_stream_t stream) {
    int rc = check_loss_args("mf_loss_bwd", B, N, d, P, num_negatives, u, v, ws, ws, ws_bytes);
    if (rc) return rc;
    if (kind < 0 || kind >= MF_NUM_KINDS || !grad_out || !du || !dv)
        return mf_set_error(MF_EINVAL, "mf_loss_bwd: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const LossWs w = loss_ws(ws, B, N, d, num_negatives);
    if (!(flags & MF_LOSS_ROWC))      // else finish_kernel of the forward already wrote them
        rowc_kernel<<<dim3((unsigned)((w.Bp + 255) / 256)), 256, 0, s>>>(w.stats, w.tgt, w.lii, w.sgn, B, w.Bp, kind, sigma, margin, w.rowc);
    const int gmode = gmode_of(kind);
    if (kind == MF_ALIGNMENT || w.mined) dense_bwd_none(ws);
    if (kind == MF_ALIGNMENT) {
        MF_DISPATCH_D(d, {
            const int64_t nthreads = N * (D / 4);
            diag_bwd_kernel<D><<<dim3((unsigned)((nthreads + 255) / 256)), 256, 0, s>>>(u, v, w.rowc, grad_out, B, N, w.Bp, du, dv);
        });
    } else {
        rc = w.mined ? mined_bwd(w, gmode, u, v, grad_out, du, dv, s) : dense_bwd(w, ws, gmode, u, v, grad_out, du, dv, s);
        if (rc) return rc;
    }
    return mf_check_launch("mf_loss_bwd");
}
