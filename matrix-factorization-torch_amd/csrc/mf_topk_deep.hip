// mf_topk_deep.hip -- exact top-k for deep candidate lists (64 < k <= 1024; serves any k in 1..1024), gfx950.
//
// The three engines for k <= 64 keep a row's result in ONE wavefront (lane t = the t-th best); a candidate list for a
// ranker (Recall@100 .. @1000) does not fit there.  This engine scores once and selects from the scores, in blocks of
// queries whose score slab stays in cache:
//
//   1. slab    topk_deep_slab_kernel: slab[Qb][Np] of 32-bit ranks mf_orderable(score) (0 = no candidate; columns >= N
//              are 0), scores from the fp32 MFMA engine of mf_common.h -- the chain of oracle/chain.c bit for bit.  Four
//              query tiles per workgroup (queries in registers), catalog tiles streamed through the mf_stream.h ring.
//              Here the QUERIES are the MFMA's A operand (accumulator rows) and the catalog tile its B operand (lanes):
//              fmaf(a, b, c) == fmaf(b, a, c), so the bits are those of select_kernel / scores_kernel, and a store
//              instruction writes 32 consecutive columns of a query's row -- whole 128-byte lines.
//   2. excl    topk_deep_excl_kernel: one workgroup per query stores rank 0 over its excluded columns.
//   3. select  topk_deep_select_kernel, one workgroup of 256 threads per query, reading its slab row through L2:
//              MSB-first radix select over the rank (4 passes x 8 bits, 256-bin LDS histograms of integer atomics: exact
//              counts) -> tau = rank of the k-th best, c = candidates above tau; every rank > tau is collected into LDS
//              (arrival order free), ranks == tau in ascending column order (block prefix counts over 1024-column
//              chunks; when ALL of them are needed no order has to be decided and they are collected with the rest);
//              bitonic sort of the <= 1024 unique 64-bit keys, best first, -inf / -1 behind them.
//
// No float atomics, no host read, nothing depends on atomic arrival order.
#include <cmath>

#include "mf_common.h"
#include "mf_stream.h"
#include "mf_lists.h"
#include "mf_topk_io.h"

// a query block's slab is at most this large (the host's preferred block).  Measured at Q = 1024 x N = 62,423 (tools/
// topk_deep_probe.py, profiles/topk_deep_probe.json): slabs of 16 / 64 / 256 MiB -- 16 / 4 / 1 query blocks -- take the call
// 1.87 / 0.72 / 0.38 ms at k = 100: a block's selection runs one workgroup per query, and 64 or 256 of them leave most of the
// chip idle.  Hence the largest.  A/B builds: EXTRA=-DMF_DEEP_SLAB_CAP_MIB=...
#ifndef MF_DEEP_SLAB_CAP_MIB
#define MF_DEEP_SLAB_CAP_MIB 256
#endif
static constexpr int64_t DEEP_SLAB_CAP = (int64_t)MF_DEEP_SLAB_CAP_MIB << 20;
static constexpr int DEEP_MAX_TPC = 4096;      // catalog tiles per workgroup at most: 4096 x 32 rows x 1 KiB (d = 256) = 128 MiB per descriptor

// ------------------------------------------------------------------------------------------------ 1. score slab ----
// grid = (catalog chunk, group of NW query tiles); wave w owns query tile blockIdx.y * NW + w of the block (rows
// q0 + 32 tile ..), every wave stages its share of each catalog tile (2-deep ring, one barrier per tile)
template <int D>
__global__ __launch_bounds__(64 * mf_nw(D)) void topk_deep_slab_kernel(const float* __restrict__ q, int64_t q0, int64_t Q, int qtiles,
                                                                        const float* __restrict__ items, int64_t N, int NT, int tpc,
                                                                        int64_t Np, unsigned* __restrict__ slab) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using G = TileGeom<D>;
    const int lane = mf_lane(), c = lane & 31, h = lane >> 5;
    const int wave = mf_wave_id();
    const int xt = (int)blockIdx.y * G::NW + wave;
    const bool active = xt < qtiles;                         // (wave-uniform) a wave without a query tile only stages
    const int t0 = (int)blockIdx.x * tpc;
    const int t1 = min(NT, t0 + tpc);

    RowFrag<D> qf;
    const int64_t qrow = q0 + (int64_t)xt * 32 + c;
    mf_load_frag<D>(qf, q, qrow, active && qrow < Q);
    TileSrc<D> tsrc;
    mf_tile_src_init<D>(tsrc, items, N, (int64_t)t0 * 32);
    // lane (c, h) holds, in accumulator e, query row mf_acc_row(e, h) x catalog column y0 + c
    unsigned* out = slab + ((int64_t)xt * 32 + 4 * h) * Np + c;
    const int sw = G::swz(c);

    if (t0 < t1) mf_stage_tile<D>(smem, t0 * 32, tsrc);
    for (int t = t0; t < t1; ++t) {
        mf_wait_vmcnt<0>();                                  // tile t has landed (this wave's share)
        mf_block_barrier();                                  // ... everybody's; and every wave is done with tile t - 1
        if (t + 1 < t1) mf_stage_tile<D>(smem + ((t + 1 - t0) & 1) * G::TILEB, (t + 1) * 32, tsrc);
        if (!active) continue;
        const char* rowp = smem + ((t - t0) & 1) * G::TILEB + c * G::ROWB;
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int g = 0; g < D / 8; ++g) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(rowp + (((2 * g + h) ^ sw) << 4));
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qf.v[g][k4], b[k4], acc, 0, 0, 0);
        }
        const int64_t y = (int64_t)t * 32 + c;
        const bool col_ok = y < N;
#pragma unroll
        for (int e = 0; e < 16; ++e)
            out[(int64_t)((e & 3) + 8 * (e >> 2)) * Np + (int64_t)t * 32] = col_ok ? mf_orderable(acc[e]) : 0u;
    }
}

// ------------------------------------------------------------------------------------------------ 2. exclusions ----
__global__ __launch_bounds__(256) void topk_deep_excl_kernel(const int64_t* __restrict__ excl_off, const int64_t* __restrict__ excl_idx,
                                                             int64_t idx_base, int64_t N, int64_t Np, int64_t q0,
                                                             unsigned* __restrict__ slab) {
    const int64_t r = blockIdx.x;
    for (int64_t e = excl_off[q0 + r] + threadIdx.x; e < excl_off[q0 + r + 1]; e += 256) {
        const int64_t y = excl_idx[e] - idx_base;
        if (y >= 0 && y < N) slab[r * Np + y] = 0u;
    }
}

// ------------------------------------------------------------------------------------- 3.-5. select, collect, sort ----
static constexpr int DEEP_THREADS = 256;

__global__ __launch_bounds__(DEEP_THREADS) void topk_deep_select_kernel(const unsigned* __restrict__ slab, int64_t Np, int k,
                                                                        int64_t idx_base, float* __restrict__ out_scores,
                                                                        int64_t* __restrict__ out_idx) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long keys[MF_TOPK_DEEP_MAX_K];
    __shared__ unsigned s_sel[4];
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const uint4* row4 = reinterpret_cast<const uint4*>(slab + r * Np);     // Np is a multiple of 32, the slab 256-byte aligned
    const int n4 = (int)(Np >> 2);
    auto sweep = [&](auto&& f) {                             // f(four ranks, first column) over the row
        for (int i = tid; i < n4; i += DEEP_THREADS) f(row4[i], 4 * i);
    };

    // MSB-first radix select: after pass p the k-th best rank is known down to bit 24 - 8 p
    unsigned prefix = 0u, mask = 0u, eq = 0u;
    int need = k, above = 0;
    bool all = false;                                        // fewer than k candidates: every one is taken
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        hist[tid] = 0u;
        __syncthreads();
        auto count = [&](unsigned v) {
            if (v != 0u && (v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
        };
        sweep([&](const uint4& v, int) { count(v.x); count(v.y); count(v.z); count(v.w); });
        __syncthreads();
        // thread t owns bin 255 - t: the exclusive scan gives the number of candidates in the bins above it
        const int64_t mine = hist[255 - tid];
        int64_t sc[1] = {mine}, tot[1];
        block_excl_scan<DEEP_THREADS, 1>(sc, tot);
        if (pass == 0 && tot[0] < need) {                    // (uniform)
            all = true;
            above = (int)tot[0];
            break;
        }
        if (sc[0] < need && need <= sc[0] + mine) {           // exactly one thread: the bin that holds the k-th best
            s_sel[0] = 255u - (unsigned)tid;
            s_sel[1] = (unsigned)(need - sc[0]);
            s_sel[2] = (unsigned)sc[0];
            s_sel[3] = (unsigned)mine;
        }
        __syncthreads();
        prefix |= s_sel[0] << shift;
        mask |= 0xFFu << shift;
        need = (int)s_sel[1];
        above += (int)s_sel[2];
        eq = s_sel[3];
    }
    const unsigned tau = all ? 0u : prefix;                  // rank of the k-th best; `above` candidates rank strictly higher
    // eq candidates rank == tau and `need` of them are wanted: when that is all of them, no order has to be decided
    const bool with_ties = !all && eq == (unsigned)need;

    for (int i = tid; i < MF_TOPK_DEEP_MAX_K; i += DEEP_THREADS) keys[i] = 0ull;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    auto collect = [&](unsigned v, int col) {
        if (v > tau || (with_ties && v == tau)) {
            const int slot = atomicAdd(&s_cnt, 1);           // (integer: which slot a key gets is free, the sort decides the order)
            if (slot < k) keys[slot] = ((unsigned long long)v << 32) | (unsigned long long)mf_key_retrieval_lo((unsigned)col);
        }
    };
    sweep([&](const uint4& v, int col) { collect(v.x, col); collect(v.y, col + 1); collect(v.z, col + 2); collect(v.w, col + 3); });
    __syncthreads();
    if (!all && !with_ties) {
        // the cut falls inside a run of equal ranks: the lowest columns win -- ascending chunks of 1024 columns, a block
        // prefix count per chunk, until `need` are in (slots above .. above + need - 1 = .. k - 1)
        int taken = 0;
        for (int i0 = 0; i0 < n4 && taken < need; i0 += DEEP_THREADS) {
            const int i = i0 + tid;
            const uint4 v = i < n4 ? row4[i] : uint4{0u, 0u, 0u, 0u};     // (tau != 0: a counted candidate's rank)
            const unsigned vv[4] = {v.x, v.y, v.z, v.w};
            int64_t p[1] = {(int64_t)((vv[0] == tau) + (vv[1] == tau) + (vv[2] == tau) + (vv[3] == tau))}, tot[1];
            block_excl_scan<DEEP_THREADS, 1>(p, tot);
            int pos = taken + (int)p[0];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (vv[j] == tau) {
                    if (pos < need) keys[above + pos] = ((unsigned long long)tau << 32) | (unsigned long long)mf_key_retrieval_lo((unsigned)(4 * i + j));
                    ++pos;
                }
            taken += (int)tot[0];
        }
        __syncthreads();
    }

    // bitonic sort, descending, of the first P = 2^ceil(log2 k) slots (unused ones hold 0 and sink to the end)
    int P = 1;
    while (P < k) P <<= 1;
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (P >> 1); i += DEEP_THREADS) {
                const int a = ((i / stride) * 2 * stride) + (i % stride), b = a + stride;
                const unsigned long long ka = keys[a], kb = keys[b];
                const bool desc = (a & size) == 0;
                if (desc ? ka < kb : ka > kb) {
                    keys[a] = kb;
                    keys[b] = ka;
                }
            }
            __syncthreads();
        }
    }
    // (written out, not mf_store_topk of mf_topk_io.h: through the helper this kernel's registers were allocated differently)
    for (int t = tid; t < k; t += DEEP_THREADS) {
        const unsigned long long key = keys[t];
        if (key != 0ull) {
            out_scores[r * k + t] = mf_key_retrieval_score(key);
            out_idx[r * k + t] = idx_base + (int64_t)mf_key_retrieval_col(key);
        } else {
            out_scores[r * k + t] = -INFINITY;
            out_idx[r * k + t] = -1;
        }
    }
}

// ------------------------------------------------------------------------------------------------------- host ----
struct DeepPlan {
    bool ok;
    int64_t Np, row_bytes;
    int64_t qb_pref;          // preferred queries per block
};
static DeepPlan deep_plan(int64_t Q, int64_t N, int d, int k) {
    DeepPlan p{};
    if (Q <= 0 || N <= 0 || !mf_width_ok(d) || k <= 0 || k > MF_TOPK_DEEP_MAX_K || N >= (1ll << 31)) return p;
    p.Np = mf_pad32(N);
    p.row_bytes = p.Np * 4;
    if (32 * p.row_bytes > (int64_t)MF_SRD_MAX_BYTES) return p;        // one 32-query slab must stay below the descriptor limit
    int64_t qb = DEEP_SLAB_CAP / p.row_bytes / 32 * 32;
    if (qb < 32) qb = 32;
    if (qb > mf_pad32(Q)) qb = mf_pad32(Q);
    p.qb_pref = qb;
    p.ok = true;
    return p;
}
// queries per block for a workspace of ws_bytes (0: not even 32)
static int64_t deep_qb(const DeepPlan& p, size_t ws_bytes) {
    int64_t qb = (int64_t)(ws_bytes / (size_t)p.row_bytes) / 32 * 32;
    return qb > p.qb_pref ? p.qb_pref : qb;
}

extern "C" size_t mf_topk_deep_ws_bytes(int64_t Q, int64_t N, int d, int k) {
    const DeepPlan p = deep_plan(Q, N, d, k);
    return p.ok ? mf_align_up((size_t)(p.qb_pref * p.row_bytes), 256) : 0;
}
extern "C" size_t mf_topk_deep_min_ws_bytes(int64_t Q, int64_t N, int d, int k) {
    const DeepPlan p = deep_plan(Q, N, d, k);
    return p.ok ? mf_align_up((size_t)(32 * p.row_bytes), 256) : 0;
}
extern "C" int mf_topk_deep_plan(int64_t Q, int64_t N, int d, int k, size_t ws_bytes, int64_t* out) {
    const DeepPlan p = deep_plan(Q, N, d, k);
    if (!p.ok || !out) return mf_set_error(MF_EINVAL, "mf_topk_deep_plan: bad argument");
    const int64_t qb = deep_qb(p, ws_bytes);
    if (qb < 32) return mf_set_error(MF_ENOSPC, "mf_topk_deep_plan: workspace too small");
    out[0] = qb;
    out[1] = (Q + qb - 1) / qb;
    out[2] = qb * p.row_bytes;
    return MF_OK;
}

extern "C" int mf_topk_deep(const float* q, int64_t Q, const float* items, int64_t N, int d, int k,
                            const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, void* ws, size_t ws_bytes,
                            float* out_scores, int64_t* out_idx, mf_stream_t stream) {
    if (const int rc = mf_topk_check_args("mf_topk_deep", {MF_TOPK_DEEP_MAX_K, 32, 31, 0}, q, Q, items, N, d, k, excl_off, excl_idx, idx_base, ws,
                                          out_scores, out_idx))
        return rc;
    const DeepPlan p = deep_plan(Q, N, d, k);
    if (!p.ok) return mf_set_error(MF_ENOTSUP, "mf_topk_deep: a 32-query score slab of %lld columns exceeds the descriptor limit", (long long)N);
    const int64_t qb = deep_qb(p, ws_bytes);
    if (qb < 32) return mf_set_error(MF_ENOSPC, "mf_topk_deep: workspace too small");
    // launch geometry of the scoring pass: ~2048 workgroups, at least 4 catalog tiles each; a workgroup's tiles go through
    // one buffer descriptor based at its first row (mf_stream.h)
    const int nw = mf_nw(d);
    const int NT = (int)(p.Np / 32);
    if ((int64_t)DEEP_MAX_TPC * 32 * d * 4 > (int64_t)MF_SRD_MAX_BYTES || qb * p.row_bytes > (int64_t)MF_SRD_MAX_BYTES)
        return mf_set_error(MF_ENOTSUP, "mf_topk_deep: extent beyond the descriptor limit");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned* slab = static_cast<unsigned*>(ws);
    for (int64_t q0 = 0; q0 < Q; q0 += qb) {
        const int64_t nq = Q - q0 < qb ? Q - q0 : qb;
        const int qtiles = (int)((nq + 31) / 32);
        const int gy = (qtiles + nw - 1) / nw;
        const int want = (2048 + gy - 1) / gy;
        int tpc = (NT + want - 1) / want;
        if (tpc < 4) tpc = 4;
        if (tpc > DEEP_MAX_TPC) tpc = DEEP_MAX_TPC;
        const int nchunk = (NT + tpc - 1) / tpc;
        MF_DISPATCH_D(d, {
            auto fn = topk_deep_slab_kernel<D>;
            const int bytes = 2 * TileGeom<D>::TILEB;
            (void)hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
            MF_TIMED("topk_deep_scores", s, (fn<<<dim3((unsigned)nchunk, (unsigned)gy), 64 * mf_nw(D), bytes, s>>>(
                q, q0, Q, qtiles, items, N, NT, tpc, p.Np, slab)));
        });
        if (excl_off) topk_deep_excl_kernel<<<dim3((unsigned)nq), 256, 0, s>>>(excl_off, excl_idx, idx_base, N, p.Np, q0, slab);
        MF_TIMED("topk_deep_select", s, (topk_deep_select_kernel<<<dim3((unsigned)nq), DEEP_THREADS, 0, s>>>(
            slab, p.Np, k, idx_base, out_scores + q0 * k, out_idx + q0 * k)));
    }
    return mf_check_launch("mf_topk_deep");
}
