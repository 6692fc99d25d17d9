// mf_loss_mined.hip -- the mined path of the losses (semi_hard_mining, xfmr_rec/losses.py:134-162): the candidate search
// (the fp32 select of mf_select.h, or through the split-bf16 prefilter of mf_mine_bf.h), the exact row top-k with the
// selected negatives' logits and statistics, and the sparse backward with its fixed-point dV.  Also mf_mine_logits, the
// reference's mining methods on a materialised logits matrix.  mf_loss_ws.h lists the units and what they share.
#include <cfloat>

#include "mf_loss_ws.h"

// ------------------------------------------------------------- mined forward ---
struct MiningPolicy {
    struct Params {
        const float *nu, *nv, *lii, *sgn, *logq;
        const uint32_t* maskW;
        int64_t Bp, N;
        float sigma;
    };
    struct Row {
        float nu, sgn, lii;
    };
    struct Tile {
        uint32_t mw;
        f32x4 nv4[4], lq4[4];
    };
    static constexpr int AUX_DMA = 2;
    // The mining rank orders Dm = L_ij - L_ii: semi-hard (Dm < 0, larger first) above hard (Dm >= 0, smaller
    // first), so `rank >= bound` is an INTERVAL of Dm: [v, 0) for a semi-hard bound, (-inf, v'] for a hard one.
    // Dm is computed exactly as key() does; the interval is widened to the bound's 30 kept rank bits
    // (conservative), everything exact happens in key().
    struct Thr {
        float lo, hi;
    };
    static __device__ __forceinline__ Thr thr_all() { return Thr{-__builtin_inff(), __builtin_inff()}; }
    static __device__ __forceinline__ Thr thr_none() { return Thr{__builtin_inff(), -__builtin_inff()}; }
    static __device__ __forceinline__ Thr make_thr(unsigned bound) {
        const unsigned cls = bound >> 30;
        const float v = mf_unorderable((bound & 0x3FFFFFFFu) << 2);   // smallest value whose rank has these 30 bits
        if (cls == 2u) return Thr{v, 0.f};              // semi-hard bound: Dm in [v, 0]  (Dm = 0 itself fails key())
        if (cls == 1u) return Thr{-__builtin_inff(), 0.f - v};   // hard bound at -Dm >= v: every Dm <= -v
        return cls == 0u ? thr_all() : thr_none();
    }
    static __device__ __forceinline__ bool maybe(const Params& p, const Row& r, const Tile& t, float score, int e, int,
                                                 const Thr& th) {
        const float L = mf_logit(r.nu, t.nv4[e >> 2][e & 3], score, r.sgn, p.sigma, -t.lq4[e >> 2][e & 3]);   // lq4 holds -logq
        const float dm = L - r.lii;
        return dm >= th.lo && dm <= th.hi;
    }
    static __device__ __forceinline__ void stage_aux(const Params& p, char* aux, int wave, int t, int64_t x0, int W0) {
        mf_stage_small(aux + wave * 128, p.maskW + (int64_t)t * p.Bp + x0, 128);
        const float* src = (wave == 1 && p.logq) ? p.logq : p.nv;
        mf_stage_small(aux + W0 + wave * 128, src + (int64_t)t * 32, 128);    // W0: nv, W0 + 128: logq, rest: copies
    }
    static __device__ __forceinline__ Row row_init(const Params& p, int64_t x, bool) {
        return Row{p.nu[x], p.sgn[x], p.lii[x]};
    }
    static __device__ __forceinline__ Tile tile_init(const Params& p, const Row&, const char* aux, int wave, int c, int h, int W0) {
        Tile t;
        t.mw = reinterpret_cast<const uint32_t*>(aux + wave * 128)[c];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            t.nv4[q] = *reinterpret_cast<const f32x4*>(aux + W0 + (8 * q + 4 * h) * 4);
            t.lq4[q] = p.logq ? *reinterpret_cast<const f32x4*>(aux + W0 + 128 + (8 * q + 4 * h) * 4)
                              : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        return t;
    }
    static __device__ __forceinline__ bool key(const Params& p, const Row& r, const Tile& t, float score, int e, int h,
                                               unsigned y, unsigned& hi, unsigned& lo) {
        const float L = mf_logit(r.nu, t.nv4[e >> 2][e & 3], score, r.sgn, p.sigma, -t.lq4[e >> 2][e & 3]);
        const float dm = L - r.lii;
        hi = mf_key_mining_hi(dm);
        lo = mf_key_mining_lo(dm, y);
        return !((t.mw >> mf_acc_row(e, h)) & 1u);          // hit, diagonal or padding column
    }
};

// One wave per user: exact ordered top-k of the row's candidate list -> sel[i][0..cnt), then -- same wave, the
// user's row still in its registers -- the logits of the selected negatives (every item row is read by the whole
// wave: coalesced 16-byte lanes; the dot is a wave reduction here, not the chain: these logits feed the loss value
// and its gradient, tolerance 1e-4, not the bit-exact selection) and the row's statistics in selection order.
struct MinedRowParams {
    const unsigned long long* cand;
    const int32_t* cand_cnt;
    int rowcap, k;
    const float *u, *v, *nu, *nv, *lii, *sgn, *nlogq;    // nlogq: the workspace's -logq copy
    int64_t B, Bp;
    int d;
    float sigma, margin;
    int need;
    int32_t *sel, *sel_cnt;
    float *sel_L, *stats;
    const int32_t* gate;         // not NULL: the launch does nothing unless *gate is set (behind the prefilter, whose rescoring waves
                                 // finish their users themselves: MinedRowFinish)
};
// sorted[0 .. m) (LDS): user i's selected negatives in order -> sel, their logits, the row's statistics.  i >= B: only the
// (empty) statistics are written.
struct MinedRowFinish {
    using Params = MinedRowParams;
    static __device__ __forceinline__ void run(const MinedRowParams& p, int64_t i, int m, const unsigned long long* sorted) {
        const int lane = mf_lane();
        RowStats st;
        stats_init(st);
        if (i < p.B) {
            if (lane < m) p.sel[i * KSEL_MAX + lane] = (int32_t)mf_key_mining_col(sorted[lane]);
            if (lane == 0) p.sel_cnt[i] = m;
            const float s_i = p.sgn[i], l = p.lii[i], sm = s_i * p.margin, nu_i = p.nu[i];
            const int d4 = p.d / 4;                  // <= 64 chunks of 16 bytes (d <= 256): one per lane
            f32x4 ur = {0.f, 0.f, 0.f, 0.f};
            if (lane < d4) ur = reinterpret_cast<const f32x4*>(p.u + i * p.d)[lane];
            // (four rows, their norms and logQ in flight at a time: one at a time was a memory round trip per selected negative)
            for (int t0 = 0; t0 < m; t0 += 4) {
                f32x4 vr[4];
                float nvj[4], lqj[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t j = t0 + q < m ? (int64_t)mf_key_mining_col(sorted[t0 + q]) : 0;
                    vr[q] = (lane < d4 && t0 + q < m) ? reinterpret_cast<const f32x4*>(p.v + j * p.d)[lane] : f32x4{0.f, 0.f, 0.f, 0.f};
                    nvj[q] = p.nv[j];
                    lqj[q] = p.nlogq[j];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (t0 + q < m) {                            // (wave-uniform)
                        float part = ur[0] * vr[q][0] + ur[1] * vr[q][1] + ur[2] * vr[q][2] + ur[3] * vr[q][3];
                        part = mf_wave_sum(part);
                        const float L = mf_logit(nu_i, nvj[q], part, s_i, p.sigma, -lqj[q]);
                        if (lane == 0) p.sel_L[i * KSEL_MAX + t0 + q] = L;
                        stats_add(st, p.need, L, sm, l, p.margin);
                        if (p.need & NEED_LSE) lse_merge(st.mx, st.se, L, 1.f);
                    }
                }
            }
        }
        if (lane == 0) {
            float* o = p.stats + i;
            o[ST_CNT * p.Bp] = st.cnt; o[ST_A * p.Bp] = st.A; o[ST_MX * p.Bp] = st.mx; o[ST_SE * p.Bp] = st.se;
            o[ST_H * p.Bp] = st.H; o[ST_HC * p.Bp] = st.Hc; o[ST_LG * p.Bp] = st.Lg; o[ST_LS * p.Bp] = st.Ls;
        }
    }
};
__global__ __launch_bounds__(64) void mined_rows_kernel(MinedRowParams p) {
    __shared__ unsigned long long win[64], sorted[64];
    const int64_t i = blockIdx.x;
    if (p.gate && __hip_atomic_load(p.gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    int m = 0;
    if (i < p.B) m = mf_row_topk<8>(p.cand + i * (int64_t)p.rowcap, p.cand_cnt[i], p.k, win, sorted);
    MinedRowFinish::run(p, i, m, sorted);
}

__global__ __launch_bounds__(256) void mask_export_mined_kernel(const int32_t* __restrict__ sel,
                                                                const int32_t* __restrict__ sel_cnt, int64_t B,
                                                                int NT, uint32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const int n = sel_cnt[i];
    for (int t = 0; t < n; ++t) {
        const int j = sel[i * KSEL_MAX + t];
        out[i * NT + (j >> 5)] |= 1u << (j & 31);   // one thread owns the whole row
    }
}

// Mined backward.  du_i accumulates in registers, in selection order.  dv_j sums contributions of many users:
// they are added as 64-bit FIXED-POINT integers with integer atomics -- integer addition is associative, so the sum is
// the same bits whatever order the atomics land in (run-to-run deterministic, unlike the fp32 atomics this replaces),
// and it is rounded to fp32 once, by dv_fix_to_f32_kernel.  The unit 2^-E is chosen per batch by dv_scale_kernel so
// that the sum cannot wrap (dv_fix_of, mf_loss_math.h): 2^-40 for ordinary batches -- a contribution is then exact on the
// grid down to |x| = 2^-17 and off by <= 2^-41 below.  Lane c of a 32-lane row group owns the features c, c + 32, ..:
// one atomic instruction covers 256 contiguous bytes of a row.
__global__ __launch_bounds__(1024) void dv_scale_kernel(const float* __restrict__ rowc, const float* __restrict__ grad_out,
                                                        const float* __restrict__ nu, const float* __restrict__ nv, int64_t B, int64_t N,
                                                        int64_t Bp, float* __restrict__ dvsc, uint4* __restrict__ zero16, int64_t n16) {
    // (blocks 1 .. clear the fixed-point accumulator: one launch instead of two)
    if (blockIdx.x > 0) {
        const int64_t stride = (int64_t)(gridDim.x - 1) * 1024;
        for (int64_t q = (int64_t)(blockIdx.x - 1) * 1024 + threadIdx.x; q < n16; q += stride) zero16[q] = uint4{0u, 0u, 0u, 0u};
        return;
    }
    // (maxima of magnitudes as unsigned bit patterns: exact, order-free, and the same rule as the one-launch step's)
    __shared__ unsigned red[3][16];
    const int tid = threadIdx.x, lane = mf_lane(), wave = mf_wave_id();
    const float go = grad_out[0];
    unsigned g = 0u, a = 0u, b = 0u;
    for (int64_t i = tid; i < B; i += 1024) {
        g = max(g, max(dv_mag(go * rowc[2 * Bp + i]), dv_mag(go * rowc[3 * Bp + i])));
        a = max(a, dv_mag(nu[i]));
    }
    for (int64_t j = tid; j < N; j += 1024) b = max(b, dv_mag(nv[j]));
    g = mf_wave_max_u32(g); a = mf_wave_max_u32(a); b = mf_wave_max_u32(b);
    if (lane == 0) { red[0][wave] = g; red[1][wave] = a; red[2][wave] = b; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) { g = max(g, red[0][w]); a = max(a, red[1][w]); b = max(b, red[2][w]); }
        const DvFix f = dv_fix_of(__builtin_bit_cast(float, g), __builtin_bit_cast(float, a), __builtin_bit_cast(float, b), (long long)B);
        dvsc[0] = f.scale; dvsc[1] = f.clamp; dvsc[2] = f.inv;
    }
}

// Round 4: a workgroup is 32 users (1024 threads), and its contributions to dV meet in LDS first -- 64-bit fixed point is
// associative, so ANY grouping gives the same bits.  The mined columns of a Zipf batch are few and hot (the first copies of
// the popular items are picked by thousands of users): 5.2 M global 64-bit atomics, thousands of them on the same words, were
// this kernel's 60 us.  Now a column is claimed in a small LDS table (key by LDS compare-and-swap; a column that loses its
// slot to another goes to global memory as before), the users add with LDS atomics, and the workgroup flushes every
// occupied slot with one global atomic per feature.
template <int D>
struct MinedBwdLds {
    static constexpr int SLOTS = D <= 128 ? 48 : 24;        // 48 KB of accumulators at d = 128 (d x 8 bytes per slot)
    static constexpr int BYTES = SLOTS * D * 8 + SLOTS * 4;
};
template <int D>
__global__ __launch_bounds__(1024) void mined_bwd_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                         const float* __restrict__ rowc, const int32_t* __restrict__ sel,
                                                         const int32_t* __restrict__ sel_cnt,
                                                         const float* __restrict__ sel_L, const float* __restrict__ grad_out,
                                                         int64_t B, int64_t Bp,
                                                         int gmode, float* __restrict__ du, long long* __restrict__ dvfix,
                                                         const float* __restrict__ dvsc) {
    extern __shared__ __attribute__((aligned(16))) char bsm[];
    using L = MinedBwdLds<D>;
    unsigned long long* lacc = reinterpret_cast<unsigned long long*>(bsm);                  // [SLOTS][D]
    int* lkey = reinterpret_cast<int*>(bsm + L::SLOTS * D * 8);                             // [SLOTS]: the column, -1 = free
    constexpr int LPR = 32, NE = D / LPR;            // lanes per row, features per lane (c, c + 32, ...)
    for (int q = threadIdx.x; q < L::SLOTS * D; q += 1024) lacc[q] = 0ull;
    if (threadIdx.x < L::SLOTS) lkey[threadIdx.x] = -1;
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const int64_t i = t / LPR;
    const int c = (int)(t % LPR);
    if (i < B) {
        const float go = grad_out[0];
        const float fix_scale = dvsc[0], fix_clamp = dvsc[1];
        const float a = rowc[i], b = rowc[Bp + i], cg = go * rowc[2 * Bp + i], gd = go * rowc[3 * Bp + i];
        float ui[NE], acc[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) { ui[e] = u[i * D + c + LPR * e]; acc[e] = 0.f; }
        const int n = sel_cnt[i];
        for (int s = -1; s < n; ++s) {
            int64_t j;
            float g;
            if (s < 0) { j = i; g = gd; }
            else { j = sel[i * KSEL_MAX + s]; g = cg * g_of(gmode, (sel_L[i * KSEL_MAX + s] - a) + b); }
            // the user's own column is its alone (one diagonal per column): straight to memory; a mined column through LDS
            int slot = -1;
            if (s >= 0) {
                const int want = (int)(((unsigned)j * 2654435761u) >> 16) % L::SLOTS;
                int got = 0;
                if (c == 0) {
                    const int old = atomicCAS(&lkey[want], -1, (int)j);
                    got = (old == -1 || old == (int)j) ? 1 : 0;
                }
                got = __shfl(got, threadIdx.x & 32, 64);     // (the group's lane 0: lane 0 or 32 of the wave)
                slot = got ? want : -1;
            }
            unsigned long long* o = reinterpret_cast<unsigned long long*>(dvfix) + j * D + c;
            unsigned long long* lo = lacc + (slot < 0 ? 0 : slot) * D + c;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const float vj = v[j * D + c + LPR * e];
                acc[e] += g * (vj - ui[e]);
                const float dvj = g * (ui[e] - vj);
                const long long q = dv_fix_term(dvj, fix_scale, fix_clamp);
                if (slot >= 0) atomicAdd(lo + LPR * e, (unsigned long long)q);      // two's complement: the unsigned add IS the signed add
                else if (s >= 0) atomicAdd(o + LPR * e, (unsigned long long)q);
                // (s < 0, the user's own column: ONE such term per column -- dv_fix_to_f32_kernel adds it, no atomic at all)
            }
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) du[i * D + c + LPR * e] = acc[e];
    }
    __syncthreads();
    // flush: one global atomic per occupied slot and feature (zeros are skipped)
    for (int q = threadIdx.x; q < L::SLOTS * D; q += 1024) {
        const int slot = q / D, f = q % D;
        const int j = lkey[slot];
        const unsigned long long val = lacc[q];
        if (j >= 0 && val != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(dvfix) + (int64_t)j * D + f, val);
    }
}

// fixed point -> fp32, and the diagonal terms on the way: column j < B also receives gd_j (u_j - v_j) -- one term per column,
// the same integer the backward kernel used to add atomically
__global__ __launch_bounds__(256) void dv_fix_to_f32_kernel(const long long* __restrict__ dvfix, int64_t n, float* __restrict__ dv,
                                                            const float* __restrict__ dvsc, const float* __restrict__ u,
                                                            const float* __restrict__ v, const float* __restrict__ rowc,
                                                            const float* __restrict__ grad_out, int64_t B, int64_t Bp, int d) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    long long acc = dvfix[t];
    const int64_t j = t / d;
    if (j < B) {
        const float gd = grad_out[0] * rowc[3 * Bp + j];
        acc += dv_fix_term(gd * (u[t] - v[t]), dvsc[0], dvsc[1]);
    }
    dv[t] = (float)((double)acc * (double)dvsc[2]);
}

// The candidate search of the mined losses through the split-bf16 prefilter: the fp32 seeding pass and its bound as before,
// then item plane / user fragments + intervals / ONE scan on the bf16 cores / exact rescoring into the row lists.
// Run-time switch: 1 = the prefilter where it pays (default), 2 = wherever it can serve (tests and the stress compare the two
// searches on small shapes), 0 = the fp32 search everywhere; MF_MINE_BF in the environment sets the initial value.
// (One variable for the process: here, beside mf_set_mining_prefilter, not in a header that several units include.)
static int g_mine_bf_mode = -1;
static int mine_bf_mode() {
    if (g_mine_bf_mode < 0) {
        const char* e = getenv("MF_MINE_BF");
        g_mine_bf_mode = (e && e[0] == '0') ? 0 : (e && e[0] == '2') ? 2 : 1;
    }
    return g_mine_bf_mode;
}
static bool mine_bf_use(const MineBfPlan& p) { return p.ok && (mine_bf_mode() == 2 || (mine_bf_mode() == 1 && p.pays)); }

static unsigned long long* g_mine_dbg = nullptr;
#ifdef MF_BF3_LAB         // per-kernel spans in lab builds; the product records ONE span over the whole search (spans do not nest)
#define MBF_TIMED(name, s, ...) MF_TIMED(name, s, __VA_ARGS__)
#else
#define MBF_TIMED(name, s, ...) do { __VA_ARGS__; } while (0)
#endif
template <int D>
static void mine_bf_prepare(const LossWs& w, const float* u, const float* v, int64_t B, int64_t N, float sigma, hipStream_t s) {
    const MineBfPlan& m = w.mbf;
    int lab_abl = 0;
#ifdef MF_BF3_LAB
    if (const char* e = getenv("MF_MBF_ABL")) lab_abl = atoi(e);
#endif
    const int item_blocks = (int)((m.Nq * (D / 8) + 255) / 256), user_blocks = (int)((m.Xq * (D / 8) + 255) / 256);
    MineUserFrags uf{u, w.sgn, B, m.Xq, sigma, static_cast<mbf16x8*>(w.mbf_ufrag)};
    MBF_TIMED("mining_items", s, (mine_items_kernel<D><<<dim3((unsigned)(item_blocks + user_blocks)), 256, 0, s>>>(
        v, w.nv, w.logq, w.colfirst, N, m.Nq, sigma, w.mbf_plane, w.mbf_max, w.mbf_rep, w.mbf_copybits, w.mbf_lastcopy,
        __builtin_ctz((unsigned)m.blk), lab_abl, item_blocks, uf)));
}
template <int D>
static void mine_bf_launch(const LossWs& w, const MinedRowParams& fin, const float* u, const float* v, int64_t B, int64_t N, int k, float sigma, hipStream_t s) {
    const MineBfPlan& m = w.mbf;
    {
        MineBound mb{w.seeds, w.plan.seeds_per_row, k, w.nu, w.lii, w.sgn, w.mbf_max, B, m.Xq, sigma, w.gtau, static_cast<f32x4*>(w.mbf_rowk),
                     w.mbf_flag, w.mbf_gate, g_mine_dbg};
        MBF_TIMED("mining_bound", s, (mine_bound_kernel<D, MiningPolicy><<<dim3((unsigned)(m.Xq / 4)), 256, 0, s>>>(mb)));
    }
    {
        MineScan ms{w.mbf_plane, m.Nq, m.NT, m.tpc, static_cast<const mbf16x8*>(w.mbf_ufrag), static_cast<const f32x4*>(w.mbf_rowk), m.Xq,
                    w.mbf_plist, m.lpc * MBF_CAPL, w.mbf_pcnt, w.mbf_spill, w.mbf_spill_cnt, w.mbf_gate, g_mine_dbg, 0};
#ifdef MF_BF3_LAB
        if (const char* e = getenv("MF_MBF_ABL")) ms.abl = atoi(e);
#endif
        auto fn = mine_scan_kernel<D>;
        const int bytes = MineLds<D>::BYTES;
        static bool attr = false;                            // (per instantiation)
        if (!attr) { (void)hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); attr = true; }
        MBF_TIMED("mining_scan", s, (fn<<<dim3((unsigned)m.nchunk, (unsigned)m.gy), 64 * MBF_WAVES, bytes, s>>>(ms)));
    }
    {
        MineRescore mr{u, v, w.nu, w.nv, w.lii, w.sgn, w.logq, w.maskW, B, w.Bp, N, m.Xq, sigma, m.nlists, k,
                       m.lpc, MineRescoreGeom<D>::keys_cap(m.nlists, k), w.mbf_plist, w.mbf_pcnt, w.mbf_flag, w.mbf_spill, w.mbf_spill_cnt, w.mbf_gate, w.mbf_rep, w.mbf_copybits, w.mbf_lastcopy, m.blk, w.cand, w.cand_cnt, w.plan.rowcap,
                       g_mine_dbg};
        auto fn = mine_rescore_kernel<D, MinedRowFinish>;
        const int bytes = MineRescoreGeom<D>::bytes(m.nlists, k);      // (at most 4 KB rows + 9.3 KB keys + 1.5 KB: below the 64 KB that need no attribute)
        MBF_TIMED("mining_rescore", s, (fn<<<dim3((unsigned)w.Bp), 64, bytes, s>>>(mr, fin)));
    }
}
static int mine_bf_run(const LossWs& w, const MiningPolicy::Params& mp, const SelectCommon& sc, const MinedRowParams& fin, const float* u, const float* v, int64_t B,
                       int64_t N, int d, int k, float sigma, hipStream_t s) {
#ifdef MF_BF3_LAB
    const bool whole = false;
#else
    const bool whole = mf_timing_on();
#endif
    if (whole) mf_timing_begin("mining_prefilter", s);
    // item plane + user fragments (one launch) -> fp32 seeding pass -> bound + intervals (one launch) -> scan -> rescoring
    if (d == 64) mine_bf_prepare<64>(w, u, v, B, N, sigma, s);
    else mine_bf_prepare<128>(w, u, v, B, N, sigma, s);
    MF_DISPATCH_D(d, { MBF_TIMED("mining_select", s, (mf_select_run<D, MiningPolicy>(w.plan, mp, sc, w.seeds, B, s, true, false, true))); });
    if (d == 64) mine_bf_launch<64>(w, fin, u, v, B, N, k, sigma, s);
    else mine_bf_launch<128>(w, fin, u, v, B, N, k, sigma, s);
    // behind it, gated on the device: a batch the prefilter gave up on (a spill list overflowed -- thousands of exact ties --,
    // a user without a bound, non-finite norms) is answered by the fp32 search; otherwise its workgroups leave at once
    SelectCommon scg = sc;
    scg.gate = w.mbf_gate;
    MF_DISPATCH_D(d, { mf_select_run<D, MiningPolicy>(w.plan, mp, scg, w.seeds, B, s, false, true); });
    if (whole) mf_timing_end("mining_prefilter", s);
    return MF_OK;
}
// tools/lab/mined_timeline.py, tests/test_gpu_mining_prefilter.py: sixteen counters since the last call -- [0] candidates
// rescored, [1] users, [2] users walked exactly, [3] .. [7] (mf_mine_bf.h), [8] the largest copy-expansion pool (keys)
extern "C" int mf_probe_mining_prefilter(unsigned long long* out16, int enable) {
    static unsigned long long* buf = nullptr;
    if (!buf) {
        if (hipMalloc(reinterpret_cast<void**>(&buf), 128) != hipSuccess) return -1;
        (void)hipMemset(buf, 0, 128);
    }
    (void)hipDeviceSynchronize();
    if (out16) (void)hipMemcpy(out16, buf, 128, hipMemcpyDeviceToHost);
    (void)hipMemset(buf, 0, 128);
    g_mine_dbg = enable ? buf : nullptr;
    return 0;
}
// 1 = the prefilter where it pays (default), 2 = wherever it can serve (tests), 0 = select_kernel only
extern "C" void mf_set_mining_prefilter(int mode) { g_mine_bf_mode = mode <= 0 ? 0 : (mode >= 2 ? 2 : 1); }
// host-only: the prefilter's plan for a shape, as mine_bf_launch would use it (nothing is launched)
extern "C" int mf_mining_prefilter_plan(int64_t B, int64_t N, int d, int k, int64_t* out8) {
    if (!out8) return mf_set_error(MF_EINVAL, "mf_mining_prefilter_plan: out is NULL");
    const MineBfPlan m = mine_bf_plan(B, N, d, k);
    int64_t kc = 0, lds = 0;
    if (d == 64) { kc = MineRescoreGeom<64>::keys_cap(m.nlists, k); lds = MineRescoreGeom<64>::bytes(m.nlists, k); }
    else if (d == 128) { kc = MineRescoreGeom<128>::keys_cap(m.nlists, k); lds = MineRescoreGeom<128>::bytes(m.nlists, k); }
    const int64_t o[8] = {m.ok ? 1 : 0, m.pays ? 1 : 0, m.nchunk, m.tpc, m.lpc, m.nlists, kc, lds};
    for (int i = 0; i < 8; ++i) out8[i] = o[i];
    return MF_OK;
}

// ---- the two stages the orchestration calls (mf_loss_ws.h) ----
int mined_fwd(const LossWs& w, const float* u, const float* v, int num_negatives, int need, float sigma, float margin,
              uint32_t* out_mask_bits, hipStream_t s) {
    const int64_t B = w.B, N = w.N;
    const int d = w.d;
    MiningPolicy::Params mp{w.nu, w.nv, w.lii, w.sgn, w.logq, w.maskW, w.Bp, N, sigma};
    SelectCommon sc{u, B, v, N, 0, (int)((N + 31) / 32), w.plan.tpc, w.Bp, num_negatives, w.plan.xw, w.gtau, w.priv, w.cand, w.cand_cnt, w.plan.rowcap};
    // (gtau, cand_cnt and the prefilter's cleared range: prep_kernel did it)
    MinedRowParams mr{w.cand, w.cand_cnt, w.plan.rowcap, num_negatives, u, v, w.nu, w.nv, w.lii, w.sgn, w.logq, B, w.Bp, d,
                      sigma, margin, need, w.sel, w.sel_cnt, w.sel_L, w.stats, nullptr};
    if (mine_bf_use(w.mbf) && w.plan.YTa > 0 && w.plan.rowcap >= num_negatives) {
        // (the rescoring waves finish their users themselves; mined_rows_kernel behind them only runs for a batch handed
        // to the fp32 search)
        if (int rc = mine_bf_run(w, mp, sc, mr, u, v, B, N, d, num_negatives, sigma, s)) return rc;
        mr.gate = w.mbf_gate;
    } else {
        MF_DISPATCH_D(d, { MF_TIMED("mining_select", s, (mf_select_run<D, MiningPolicy>(w.plan, mp, sc, w.seeds, B, s))); });
    }
    mined_rows_kernel<<<dim3((unsigned)w.Bp), 64, 0, s>>>(mr);
    if (out_mask_bits) {
        (void)hipMemsetAsync(out_mask_bits, 0, (size_t)B * ((N + 31) / 32) * 4, s);
        mask_export_mined_kernel<<<dim3((unsigned)((B + 255) / 256)), 256, 0, s>>>(w.sel, w.sel_cnt, B, (int)((N + 31) / 32), out_mask_bits);
    }
    return MF_OK;
}

int mined_bwd(const LossWs& w, int gmode, const float* u, const float* v, const float* grad_out, float* du, float* dv,
              hipStream_t s) {
    const int64_t B = w.B, N = w.N;
    const int d = w.d;
    {
        const int64_t n16 = N * d * 8 / 16;              // (d is a multiple of 32: whole 16-byte units)
        int64_t zb = (n16 + 1023) / 1024;
        if (zb > 1024) zb = 1024;
        dv_scale_kernel<<<dim3((unsigned)(1 + zb)), 1024, 0, s>>>(w.rowc, grad_out, w.nu, w.nv, B, N, w.Bp, w.dvsc, reinterpret_cast<uint4*>(w.dvfix), n16);
    }
    MF_DISPATCH_D(d, {
        const int64_t nthreads = B * 32;
        mined_bwd_kernel<D><<<dim3((unsigned)((nthreads + 1023) / 1024)), 1024, MinedBwdLds<D>::BYTES, s>>>(u, v, w.rowc, w.sel, w.sel_cnt, w.sel_L,
                                                                                                          grad_out, B, w.Bp, gmode, du, w.dvfix, w.dvsc);
    });
    dv_fix_to_f32_kernel<<<dim3((unsigned)((N * d + 255) / 256)), 256, 0, s>>>(w.dvfix, N * d, dv, w.dvsc, u, v, w.rowc, grad_out, B, w.Bp, d);
    return MF_OK;
}

#ifdef MF_PROBE
extern "C" void mf_probe_mining_counters(unsigned long long* out16, int reset) {   // tools/mined_probe.py
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out16, HIP_SYMBOL(mf_sel_dbg), 16 * 8);
    if (reset) {
        unsigned long long z[16] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(mf_sel_dbg), z, 16 * 8);
    }
}
#endif

// ------------------------------------------------------ public mining helper ----
// API parity with the reference's EmbeddingLoss.hard_mining (losses.py:112-132, never called upstream) and
// semi_hard_mining (:134-162) on a MATERIALISED logits matrix.  Not the hot path.
// one wave per row: k rounds, each extracting the best remaining valid key (exact, any k)
__global__ __launch_bounds__(64) void mine_logits_kernel(const float* __restrict__ logits, int64_t N, int k, int semi_hard,
                                                         uint8_t* __restrict__ mask) {
    const int64_t i = blockIdx.x;
    const int lane = mf_lane();
    const float* row = logits + i * N;
    uint8_t* mrow = mask + i * N;
    const float lii = row[i];
    unsigned long long prev = ~0ull;
    int taken = 0;
    for (int r = 0; r < k; ++r) {
        unsigned long long best = 0ull;
        for (int64_t j = lane; j < N; j += 64) {
            if (!(mrow[j] & 1)) continue;
            const unsigned long long key = semi_hard ? mf_key_mining(row[j] - lii, (unsigned)j)
                                                     : (((unsigned long long)mf_orderable(row[j]) << 30) | (0x3FFFFFFFu - (unsigned)j));
            if (key < prev && key > best) best = key;
        }
        best = mf_wave_max_u64(best);
        if (best == 0ull) break;
        prev = best;
        ++taken;
        const unsigned col = 0x3FFFFFFFu - (unsigned)(best & 0x3FFFFFFFull);
        if (lane == 0) mrow[col] |= 2;
    }
    __syncthreads();
    (void)taken;
    for (int64_t j = lane; j < N; j += 64) mrow[j] = (mrow[j] & 2) ? 1 : 0;
}

extern "C" int mf_mine_logits(const float* logits, int64_t B, int64_t N, int k, int semi_hard, uint8_t* mask,
                              mf_stream_t stream) {
    if (!logits || !mask || B <= 0 || N < B) return mf_set_error(MF_EINVAL, "mf_mine_logits: bad argument");
    if (N >= (1ll << 30)) return mf_set_error(MF_ENOTSUP, "mf_mine_logits: N >= 2^30");
    if (k <= 0 || k >= N) return MF_OK;       // losses.py:115-119 / :137-141: mining disabled, mask unchanged
    mine_logits_kernel<<<dim3((unsigned)B), 64, 0, static_cast<hipStream_t>(stream)>>>(logits, N, k, semi_hard, mask);
    return mf_check_launch("mf_mine_logits");
}
