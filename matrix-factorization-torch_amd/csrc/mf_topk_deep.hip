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
// The slab is also all it takes to say where GIVEN rows stand in a query's order of the whole catalog (mf_target_positions:
// stages 1 and 2, then target_positions_kernel, section 4 below) -- evaluation without a list, at any depth.  Over a catalog
// that is row-sharded the same count runs per shard on keys given from outside (mf_target_words + mf_key_positions, section 5).
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

// bitonic sort of keys[0 .. P - 1] in LDS, descending (P a power of two; every thread of the workgroup calls it; ends on a barrier)
__device__ __forceinline__ void deep_sort_desc(unsigned long long* keys, int P) {
    const int tid = threadIdx.x;
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
}

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
    deep_sort_desc(keys, P);
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

// ----------------------------------------------------------------------------------- 4. positions of given rows ----
// Instead of the k best rows of a query, the place of GIVEN rows (its targets) in the order of all admissible ones: the
// number of slab words whose key (word << 32 | ~column) is larger than the target's.  One workgroup per query, the target
// list in passes of POS_PASS entries; a pass sweeps the slab row once.  Up to POS_FEW entries are counted by plain compares
// in registers and reduced once (one or two targets would send nearly every element of the row to the same LDS word); more
// are sorted, an element finds by binary search how many of the pass's keys are >= its own and adds 1 to that bin (integer
// LDS atomics: exact, order-free), and a scan over the bins gives every key the number of elements above it.  Elements
// below the pass's lowest key are above nobody and are not binned.
static constexpr int POS_PASS = 1024;
static constexpr int POS_FEW = 16;
static constexpr int POS_LOADS = 4;        // 16-byte loads a thread has in flight during the sweep

// f(four words, first column) over the slab row, zero words included; POS_LOADS independent loads are issued before the first is used
template <class F>
__device__ __forceinline__ void pos_sweep(const uint4* __restrict__ row4, int n4, F&& f) {
    for (int i0 = 0; i0 < n4; i0 += POS_LOADS * DEEP_THREADS) {
        uint4 v[POS_LOADS];
#pragma unroll
        for (int u = 0; u < POS_LOADS; ++u) {
            const int i = i0 + u * DEEP_THREADS + (int)threadIdx.x;
            v[u] = i < n4 ? row4[i] : uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < POS_LOADS; ++u) {
            const unsigned w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            f(w, 4u * (unsigned)(i0 + u * DEEP_THREADS + (int)threadIdx.x));
        }
    }
}

__device__ __forceinline__ unsigned long long pos_key(unsigned word, unsigned col) {
    return ((unsigned long long)word << 32) | (unsigned long long)mf_key_retrieval_lo(col);
}

// a pass of at most M <= POS_FEW entries, keys[0 .. M - 1] in LDS (unused slots hold all ones: nothing is above them);
// leaves the counts in red[0][0 .. M - 1] and the row's non-zero words in red[0][M].  (A zero word makes a key below every
// admissible entry's, so it needs no test here.)
template <int M>
__device__ __forceinline__ void pos_count_few(const uint4* __restrict__ row4, int n4, const unsigned long long* keys,
                                              int (*red)[POS_FEW + 1]) {
    unsigned long long kk[M];
    int cnt[M], nz = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        kk[j] = keys[j];
        cnt[j] = 0;
    }
    pos_sweep(row4, n4, [&](const unsigned (&w)[4], unsigned col) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned long long ek = pos_key(w[c], col + c);
            nz += w[c] != 0u ? 1 : 0;
#pragma unroll
            for (int j = 0; j < M; ++j) cnt[j] += ek > kk[j] ? 1 : 0;
        }
    });
    const int lane = mf_lane(), wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int c = mf_wave_sum_int(cnt[j]);
        if (lane == 0) red[wave][j] = c;
    }
    nz = mf_wave_sum_int(nz);
    if (lane == 0) red[wave][M] = nz;
    __syncthreads();
    if ((int)threadIdx.x <= M) {
        int t = 0;
        for (int w = 0; w < DEEP_THREADS / 64; ++w) t += red[w][threadIdx.x];
        red[0][threadIdx.x] = t;                              // (thread j reads and writes column j only)
    }
    __syncthreads();
}

// Where an entry's key comes from -- src(row, e, key) sets the key of target entry e against this query's slab row, and leaves
// the 0 it finds there when the entry is not admissible.
// PosOwnRow: the catalog is whole, the entry names one of its rows and the key is read off that row's slab word.
struct PosOwnRow {
    int64_t N, idx_base;
    const int64_t* __restrict__ tgt_idx;
    __device__ __forceinline__ void operator()(const unsigned* row, int64_t e, unsigned long long& key) const {
        const int64_t y = tgt_idx[e] - idx_base;
        if (y >= 0 && y < N) {
            const unsigned w = row[y];
            if (w != 0u) key = pos_key(w, (unsigned)y);
        }
    }
};
// PosGivenKey: the catalog is ONE SHARD of N rows, local row l = global row l * stride + offset, and the entry's word was
// computed by the shard that holds its global row g (mf_target_words, the maximum over the shards; 0: nobody holds it).  Global
// order = word descending, then global row ascending; g(l) grows with l, so this shard's rows above (word, g) are those with a
// larger word, or the same word and l < L = clamp(ceil((g - offset) / stride), 0, N) -- the comparison against (word << 32 | ~L),
// and on the shard that holds g, L is the row itself: there a slab word of 0 (excluded) makes the entry inadmissible.
struct PosGivenKey {
    int64_t N, stride, offset;
    const int64_t* __restrict__ tgt_idx;
    const int64_t* __restrict__ tgt_word;
    __device__ __forceinline__ void operator()(const unsigned* row, int64_t e, unsigned long long& key) const {
        const unsigned w = (unsigned)tgt_word[e];
        if (w == 0u) return;
        const int64_t g = tgt_idx[e];
        int64_t L = 0;
        if (g >= offset) {                                   // (g - offset cannot overflow: both are >= 0 here)
            const int64_t dist = g - offset, quo = dist / stride;
            if (quo >= N) L = N;                             // beyond the last row: every equal word is above
            else if (quo * stride != dist) L = quo + 1;      // between two rows
            else if (row[quo] == 0u) return;                 // this shard's row, and it is excluded
            else L = quo;
        }
        key = pos_key(w, (unsigned)L);
    }
};

// one query's targets against its slab row (every thread of the workgroup; r = the query's row of the slab, q0 + r its number)
template <class Src>
__device__ __forceinline__ void pos_count_row(const unsigned* slab, int64_t Np, int64_t q0, const int64_t* tgt_off, const Src src, int64_t* out_pos,
                                              float* out_score, int64_t* out_ncand) {
    __shared__ unsigned long long keys[POS_PASS];
    __shared__ unsigned bins[POS_PASS];
    __shared__ int red[DEEP_THREADS / 64][POS_FEW + 1];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const unsigned* row = slab + r * Np;
    const uint4* row4 = reinterpret_cast<const uint4*>(row);             // Np is a multiple of 32, the slab 256-byte aligned
    const int n4 = (int)(Np >> 2);
    const int64_t e0 = tgt_off[q0 + r], e1 = tgt_off[q0 + r + 1];

    for (int64_t p0 = e0; p0 == e0 || p0 < e1; p0 += POS_PASS) {        // (a query without targets: one pass, for its count)
        const int m = (int)(e1 - p0 < POS_PASS ? (e1 > p0 ? e1 - p0 : 0) : POS_PASS);
        // entry tid + 256 j of the pass: its key (0: excluded, out of range -- not admissible)
        unsigned long long mine[POS_PASS / DEEP_THREADS];
#pragma unroll
        for (int j = 0; j < POS_PASS / DEEP_THREADS; ++j) {
            const int t = tid + DEEP_THREADS * j;
            mine[j] = 0ull;
            if (t < m) src(row, p0 + t, mine[j]);
        }
        if (m <= POS_FEW) {
            if (tid < POS_FEW) keys[tid] = tid < m && mine[0] != 0ull ? mine[0] : ~0ull;
            __syncthreads();
            if (m <= 1) pos_count_few<1>(row4, n4, keys, red);
            else if (m <= 4) pos_count_few<4>(row4, n4, keys, red);
            else pos_count_few<POS_FEW>(row4, n4, keys, red);
            if (tid < m) {
                out_pos[p0 + tid] = mine[0] != 0ull ? (int64_t)red[0][tid] : -1;
                out_score[p0 + tid] = mine[0] != 0ull ? mf_key_retrieval_score(mine[0]) : -INFINITY;
            }
            if (p0 == e0 && tid == 0) out_ncand[q0 + r] = red[0][m <= 1 ? 1 : (m <= 4 ? 4 : POS_FEW)];
            __syncthreads();                                 // (keys and red are written again by the next pass)
            continue;
        }
        // sort the pass's keys, best first; the inadmissible entries' zeros sink behind the nvalid admissible ones
        int P = 32;
        while (P < m) P <<= 1;
        int64_t nv[1] = {0}, nvt[1];
#pragma unroll
        for (int j = 0; j < POS_PASS / DEEP_THREADS; ++j) {
            const int t = tid + DEEP_THREADS * j;
            if (t < P) keys[t] = mine[j];
            bins[t] = 0u;
            nv[0] += mine[j] != 0ull ? 1 : 0;
        }
        block_excl_scan<DEEP_THREADS, 1>(nv, nvt);           // (its barriers also publish keys and bins)
        const int nvalid = (int)nvt[0];
        deep_sort_desc(keys, P);
        const unsigned long long kmin = nvalid > 0 ? keys[nvalid - 1] : ~0ull;
        int nz = 0;
        pos_sweep(row4, n4, [&](const unsigned (&w)[4], unsigned col) {
            unsigned long long ek[4];
            bool any = false;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                nz += w[c] != 0u ? 1 : 0;
                ek[c] = pos_key(w[c], col + c);
                any |= ek[c] > kmin;
            }
            if (!any) return;                                // below the pass's lowest key: above nobody
            // bin = the number of sorted keys >= the element's = the first key below it (0 .. nvalid - 1 for an element above
            // kmin); a fixed log2 P halvings, the four words' searches side by side: four LDS reads in flight
            int at[4] = {0, 0, 0, 0};
            for (int s = P >> 1; s > 0; s >>= 1) {
#pragma unroll
                for (int c = 0; c < 4; ++c) at[c] += keys[at[c] + s - 1] >= ek[c] ? s : 0;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (ek[c] > kmin) atomicAdd(&bins[at[c]], 1u);
        });
        if (p0 == e0) {                                      // (uniform)
            nz = mf_wave_sum_int(nz);
            if (mf_lane() == 0) red[tid >> 6][0] = nz;
        }
        __syncthreads();
        // bins -> elements above sorted key i = bins[0] + .. + bins[i]; thread t owns bins 4 t .. 4 t + 3
        unsigned b4[4];
        int64_t sc[1] = {0}, tot[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            b4[j] = bins[4 * tid + j];
            sc[0] += b4[j];
        }
        block_excl_scan<DEEP_THREADS, 1>(sc, tot);
        unsigned run = (unsigned)sc[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            run += b4[j];
            bins[4 * tid + j] = run;
        }
        __syncthreads();
        // every entry looks its own key up: equal keys (duplicates in the list) meet the same answer
#pragma unroll
        for (int j = 0; j < POS_PASS / DEEP_THREADS; ++j) {
            const int t = tid + DEEP_THREADS * j;
            if (t >= m) continue;
            if (mine[j] == 0ull) {
                out_pos[p0 + t] = -1;
                out_score[p0 + t] = -INFINITY;
                continue;
            }
            int lo = 0, hi = nvalid - 1;                     // the first sorted key <= mine: one of its copies
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (keys[mid] <= mine[j]) hi = mid;
                else lo = mid + 1;
            }
            out_pos[p0 + t] = (int64_t)bins[lo];
            out_score[p0 + t] = mf_key_retrieval_score(mine[j]);
        }
        if (p0 == e0 && tid == 0) {
            int t = 0;
            for (int w = 0; w < DEEP_THREADS / 64; ++w) t += red[w][0];
            out_ncand[q0 + r] = t;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(DEEP_THREADS) void target_positions_kernel(const unsigned* __restrict__ slab, int64_t Np, int64_t N, int64_t q0,
                                                                        int64_t idx_base, const int64_t* __restrict__ tgt_off,
                                                                        const int64_t* __restrict__ tgt_idx, int64_t* __restrict__ out_pos,
                                                                        float* __restrict__ out_score, int64_t* __restrict__ out_ncand) {
    pos_count_row(slab, Np, q0, tgt_off, PosOwnRow{N, idx_base, tgt_idx}, out_pos, out_score, out_ncand);
}

// ------------------------------------------------------------------- 5. positions over a row-sharded catalog ----
// One shard's share of a position: the same count, the entries' keys given from outside (PosGivenKey above).
__global__ __launch_bounds__(DEEP_THREADS) void shard_key_count_kernel(const unsigned* __restrict__ slab, int64_t Np, int64_t N, int64_t q0,
                                                                       int64_t stride, int64_t offset, const int64_t* __restrict__ tgt_off,
                                                                       const int64_t* __restrict__ tgt_idx, const int64_t* __restrict__ tgt_word,
                                                                       int64_t* __restrict__ out_above, float* __restrict__ out_score,
                                                                       int64_t* __restrict__ out_ncand) {
    pos_count_row(slab, Np, q0, tgt_off, PosGivenKey{N, stride, offset, tgt_idx, tgt_word}, out_above, out_score, out_ncand);
}

// The words themselves: entry e of query r names global row g; the shard that holds it (local row l = (g - offset) / stride)
// writes mf_orderable of the canonical chain q_r . items_l -- the bits its MFMA slab holds at [r][l] -- and every other shard 0.
// One lane per entry (the chain is one accumulator), workgroup (r, c) takes entries c * 256 + tid, + WORDS_SPLIT * 256, .. of
// query r's list with the query row in LDS (every lane reads the same word: a broadcast) and the item row from memory in
// 16-byte loads, up to 128 floats in flight.
static constexpr int WORDS_THREADS = 256;
static constexpr int WORDS_SPLIT = 4;

template <int D>
__global__ __launch_bounds__(WORDS_THREADS) void shard_words_kernel(const float* __restrict__ q, const float* __restrict__ items, int64_t N,
                                                                     const int64_t* __restrict__ tgt_off, const int64_t* __restrict__ tgt_idx,
                                                                     int64_t stride, int64_t offset, int64_t* __restrict__ out_word) {
    __shared__ __attribute__((aligned(16))) float xq[D];
    const int64_t r = blockIdx.x;
    const int64_t e0 = tgt_off[r] + (int64_t)blockIdx.y * WORDS_THREADS, e1 = tgt_off[r + 1];
    if (e0 >= e1) return;                                    // (uniform)
    for (int i = threadIdx.x; i < D; i += WORDS_THREADS) xq[i] = q[r * D + i];
    __syncthreads();
    constexpr int B = D < 128 ? D : 128;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += (int64_t)WORDS_SPLIT * WORDS_THREADS) {
        const int64_t g = tgt_idx[e];
        unsigned word = 0u;
        if (g >= offset) {                                   // (g - offset cannot overflow: both are >= 0 here)
            const int64_t dist = g - offset, l = dist / stride;
            if (l * stride == dist && l < N) {
                const float* __restrict__ row = items + l * D;
                float acc = 0.f;
#pragma unroll
                for (int g0 = 0; g0 < D; g0 += B) {
                    f32x4 y[B / 4];
#pragma unroll
                    for (int j = 0; j < B / 4; ++j) y[j] = *reinterpret_cast<const f32x4*>(row + g0 + 4 * j);
#pragma unroll
                    for (int k = 0; k < B; k += 8)           // k order of mf_dot_chain
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            acc = __builtin_fmaf(xq[g0 + k + t], y[k / 4][t], acc);
                            acc = __builtin_fmaf(xq[g0 + k + 4 + t], y[k / 4 + 1][t], acc);
                        }
                }
                word = mf_orderable(acc);
            }
        }
        out_word[e] = (int64_t)word;
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

// one query block's slab: scores of queries q0 .. q0 + nq - 1 against the whole catalog, exclusions stored over them.
// Launch geometry of the scoring pass: ~2048 workgroups, at least 4 catalog tiles each; a workgroup's tiles go through one
// buffer descriptor based at its first row (mf_stream.h)
static int deep_fill_slab(const float* q, int64_t q0, int64_t nq, int64_t Q, const float* items, int64_t N, int d, const DeepPlan& p,
                          const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, unsigned* slab, hipStream_t s) {
    const int nw = mf_nw(d);
    const int NT = (int)(p.Np / 32);
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
    return MF_OK;
}
static bool deep_extent_ok(const DeepPlan& p, int64_t qb, int d) {
    return (int64_t)DEEP_MAX_TPC * 32 * d * 4 <= (int64_t)MF_SRD_MAX_BYTES && qb * p.row_bytes <= (int64_t)MF_SRD_MAX_BYTES;
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
    if (!deep_extent_ok(p, qb, d)) return mf_set_error(MF_ENOTSUP, "mf_topk_deep: extent beyond the descriptor limit");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned* slab = static_cast<unsigned*>(ws);
    for (int64_t q0 = 0; q0 < Q; q0 += qb) {
        const int64_t nq = Q - q0 < qb ? Q - q0 : qb;
        if (const int rc = deep_fill_slab(q, q0, nq, Q, items, N, d, p, excl_off, excl_idx, idx_base, slab, s)) return rc;
        MF_TIMED("topk_deep_select", s, (topk_deep_select_kernel<<<dim3((unsigned)nq), DEEP_THREADS, 0, s>>>(
            slab, p.Np, k, idx_base, out_scores + q0 * k, out_idx + q0 * k)));
    }
    return mf_check_launch("mf_topk_deep");
}

// ---- positions: the same blocks and slabs, k out of the picture
extern "C" size_t mf_target_positions_ws_bytes(int64_t Q, int64_t N, int d) { return mf_topk_deep_ws_bytes(Q, N, d, 1); }
extern "C" size_t mf_target_positions_min_ws_bytes(int64_t Q, int64_t N, int d) { return mf_topk_deep_min_ws_bytes(Q, N, d, 1); }

extern "C" int mf_target_positions(const float* q, int64_t Q, const float* items, int64_t N, int d, const int64_t* tgt_off,
                                   const int64_t* tgt_idx, int64_t n_targets, const int64_t* excl_off, const int64_t* excl_idx,
                                   int64_t idx_base, void* ws, size_t ws_bytes, int64_t* out_pos, float* out_score, int64_t* out_ncand,
                                   mf_stream_t stream) {
    if (!tgt_off || !tgt_idx || !out_ncand || n_targets < 0) return mf_set_error(MF_EINVAL, "mf_target_positions: bad argument");
    if (const int rc = mf_topk_check_args("mf_target_positions", {1, 32, 31, 0}, q, Q, items, N, d, 1, excl_off, excl_idx, idx_base, ws,
                                          out_score, out_pos))
        return rc;
    const DeepPlan p = deep_plan(Q, N, d, 1);
    if (!p.ok)
        return mf_set_error(MF_ENOTSUP, "mf_target_positions: a 32-query score slab of %lld columns exceeds the descriptor limit", (long long)N);
    const int64_t qb = deep_qb(p, ws_bytes);
    if (qb < 32) return mf_set_error(MF_ENOSPC, "mf_target_positions: workspace too small");
    if (!deep_extent_ok(p, qb, d)) return mf_set_error(MF_ENOTSUP, "mf_target_positions: extent beyond the descriptor limit");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned* slab = static_cast<unsigned*>(ws);
    for (int64_t q0 = 0; q0 < Q; q0 += qb) {
        const int64_t nq = Q - q0 < qb ? Q - q0 : qb;
        if (const int rc = deep_fill_slab(q, q0, nq, Q, items, N, d, p, excl_off, excl_idx, idx_base, slab, s)) return rc;
        MF_TIMED("target_positions", s, (target_positions_kernel<<<dim3((unsigned)nq), DEEP_THREADS, 0, s>>>(
            slab, p.Np, N, q0, idx_base, tgt_off, tgt_idx, out_pos, out_score, out_ncand)));
    }
    return mf_check_launch("mf_target_positions");
}

// ---- positions over a row-sharded catalog: every shard runs the two calls below, the caller combines (mf_hip.h)
extern "C" int mf_target_words(const float* q, int64_t Q, const float* items, int64_t N, int d, const int64_t* tgt_off,
                               const int64_t* tgt_idx, int64_t n_targets, int64_t stride, int64_t offset, int64_t* out_word,
                               mf_stream_t stream) {
    if (!q || !items || !tgt_off || !tgt_idx || !out_word || Q <= 0 || N <= 0 || n_targets < 0 || stride < 1 || offset < 0)
        return mf_set_error(MF_EINVAL, "mf_target_words: bad argument");
    if (!mf_width_ok(d)) return mf_set_error(MF_EINVAL, "mf_target_words: embedding width %d not in {32,64,128,256}", d);
    if (N >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "mf_target_words: item indices must fit 32 bits");
    if (Q >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "mf_target_words: Q = %lld queries exceed one launch", (long long)Q);
    hipStream_t s = static_cast<hipStream_t>(stream);
    MF_DISPATCH_D(d, {
        MF_TIMED("target_words", s, (shard_words_kernel<D><<<dim3((unsigned)Q, WORDS_SPLIT), WORDS_THREADS, 0, s>>>(
            q, items, N, tgt_off, tgt_idx, stride, offset, out_word)));
    });
    return mf_check_launch("mf_target_words");
}

extern "C" size_t mf_key_positions_ws_bytes(int64_t Q, int64_t N, int d) { return mf_target_positions_ws_bytes(Q, N, d); }
extern "C" size_t mf_key_positions_min_ws_bytes(int64_t Q, int64_t N, int d) { return mf_target_positions_min_ws_bytes(Q, N, d); }

extern "C" int mf_key_positions(const float* q, int64_t Q, const float* items, int64_t N, int d, const int64_t* tgt_off,
                                const int64_t* tgt_idx, const int64_t* tgt_word, int64_t n_targets, int64_t stride, int64_t offset,
                                const int64_t* excl_off, const int64_t* excl_local, void* ws, size_t ws_bytes, int64_t* out_above,
                                float* out_score, int64_t* out_ncand, mf_stream_t stream) {
    if (!tgt_off || !tgt_idx || !tgt_word || !out_ncand || n_targets < 0 || stride < 1 || offset < 0)
        return mf_set_error(MF_EINVAL, "mf_key_positions: bad argument");
    if (const int rc = mf_topk_check_args("mf_key_positions", {1, 32, 31, 0}, q, Q, items, N, d, 1, excl_off, excl_local, 0, ws, out_score,
                                          out_above))
        return rc;
    const DeepPlan p = deep_plan(Q, N, d, 1);
    if (!p.ok)
        return mf_set_error(MF_ENOTSUP, "mf_key_positions: a 32-query score slab of %lld columns exceeds the descriptor limit", (long long)N);
    const int64_t qb = deep_qb(p, ws_bytes);
    if (qb < 32) return mf_set_error(MF_ENOSPC, "mf_key_positions: workspace too small");
    if (!deep_extent_ok(p, qb, d)) return mf_set_error(MF_ENOTSUP, "mf_key_positions: extent beyond the descriptor limit");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned* slab = static_cast<unsigned*>(ws);
    for (int64_t q0 = 0; q0 < Q; q0 += qb) {
        const int64_t nq = Q - q0 < qb ? Q - q0 : qb;
        if (const int rc = deep_fill_slab(q, q0, nq, Q, items, N, d, p, excl_off, excl_local, 0, slab, s)) return rc;
        MF_TIMED("key_positions", s, (shard_key_count_kernel<<<dim3((unsigned)nq), DEEP_THREADS, 0, s>>>(
            slab, p.Np, N, q0, stride, offset, tgt_off, tgt_idx, tgt_word, out_above, out_score, out_ncand)));
    }
    return mf_check_launch("mf_key_positions");
}
