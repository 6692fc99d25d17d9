// mf_pq.hip -- product-quantised cells with an exact refine: the other half of the reference's IVF_PQ index (gfx950).
//
// The reference builds its index with num_sub_vectors = embedding_dim // 8 and searches it with
// nprobes(num_probes).refine_factor(refine_factor) (xfmr_rec/data/lightning.py:162-165, 203-204, 222-229, 250-259): the rows of
// the probed partitions are ranked by a score read from per-query tables over one-byte codes, and the refine_factor * top_k
// best of them are scored again on the stored vectors.  mf_ivf.hip keeps the cells and scores every probed row exactly from a
// cell-ordered fp32 copy; here that copy is replaced by the codes (one byte per dsub channels), and only R = refine_factor *
// top_k rows per query are read from the original matrix.  Which rows are returned is approximate; their scores are the
// canonical chain's (mf_numerics.h), keyed by the catalog row.
//
// Arithmetic (D = M * dsub channels, codebooks B[M][256][dsub], chain = mf_dot_chain over a sub-vector; at dsub = 4 the four
// products in ascending channel order -- the chain of the sub-vector zero-padded to 8):
//   residual   r = x - centroid[cell]                                      one fp32 subtraction per channel
//   encode     code[m] = argmax_j (chain(r[m], B[m][j]) - 0.5f * chain(B[m][j], B[m][j])), lowest j on ties
//   table      lut[m][j] = chain(q[m], B[m][j])
//   approx     ((base + lut[0][code_0]) + lut[1][code_1]) + ..,  base = chain(q, centroid[cell]) (the coarse search's score)
//
// Code layout ("cell-ordered", what pq_encode_kernel writes and pq_scan_kernel reads): positions are those of row_of[Npad]
// (partition_layout: every cell padded to whole 64-row blocks).  With U = min(M, 4) bytes per unit and M / U units per row,
//   byte ((blk * (M / U) + u) * 64 + lane) * U + b  =  code u * U + b of position blk * 64 + lane:
// [64-row block][M / 4][64] 32-bit words, lane = row, so a wave loads a unit of a block as one coalesced 256 B (M = 2: 128 B)
// and a row costs M bytes -- Npad * M in all.  Padding positions hold code 0 and are masked by row_of < 0.
//
//   * pq_encode_kernel: a workgroup per 64 positions, lane = position, a wave per sub-space in turn: the residual sub-vector
//     in registers, the 256 codewords through scalar loads, their half norms in LDS.
//   * pq_scan_kernel: a workgroup per (query, probe, slice).  It builds the query's M x 256 table in LDS from the codebooks
//     (thread = codeword), then walks the slice's blocks, a block per wave and pass, lane = row.  Keys that beat the bound (and
//     only those are looked up in the exclusion list) are appended behind the R kept ones in a workgroup-wide LDS buffer of
//     1,024 keys -- the waves' counts are exchanged through LDS, no atomics --, which a bitonic sort orders when another pass
//     might not fit.  Every workgroup writes all R entries of its ordered list: [nprobe * S][Q][R] packed, the form
//     mf_topk_merge_packed_deep takes.  The exclusion look-up, the packed entry, the slice plan and the export's checks
//     are mf_cells.h's, shared with mf_ivf.hip; the tables and the buffer are this kernel's own.
//   * pq_scan_allow_kernel: the same kernel text (mf_pq_scan.inc) reading an allow bitmap, one 64-bit word per 64-row block
//     (mf_filter_cell_bits): a row whose bit is clear has key 0 before it meets the bound -- mf_pq_scan_allow.
//   * pq_refine_kernel: a workgroup per query, a thread per merged candidate: the chain on the original row, then the
//     top_k <= 64 by mf_row_topk (as the join of ivf_scan_kernel), stored with the standard tail.
//   * pq_refine_deep_kernel: the refine of the deep lists (mf_ivf_deep.hip: pq_deep_scan_kernel, up to 1,024 candidates): a
//     thread scores up to four candidates with the same chain, the keys are sorted in LDS (pq_sort_desc), the first k leave.
// The geometry's dispatch, the sub-vector chain and the scans' parameters are mf_pq_tables.h's, shared with the deep scan.
#include "mf_cells.h"
#include "mf_pq_tables.h"
#include "mf_select.h"

static constexpr int PQ_THREADS = 64 * MF_CELLS_NW;
static constexpr int PQ_MAX_K = 64;            // one wavefront holds the result
static constexpr int PQ_MAX_R = PQ_THREADS;    // candidates per query: a thread each in the refine
static constexpr int PQ_BUF = 1024;            // keys of the workgroup's buffer: PQ_MAX_R kept, then the waiting ones
// lists of R <= 256 entries, G * R of a query within the keys mf_topk_merge_packed_deep holds in LDS
static constexpr MfCellsLimits PQ_LISTS{PQ_MAX_R, MF_TOPK_MERGE_DEEP_MAX_KEYS, 'R'};

// ---------------------------------------------------------------------- encode ----
struct PqEncodeParams {
    const float* rows;          // [N][d]: the stored rows, or residuals when centroids is null
    const float* centroids;     // [C][d], nullable
    const int64_t* assign;      // [N], with centroids
    const float* codebooks;     // [M][256][dsub]
    const int64_t* row_of;      // [npos]: the row at a position, -1 for padding; null: position = row, codes [N][M]
    int64_t N, npos;
    int d, M;
    unsigned char* codes;
};

template <int DSUB>
__global__ __launch_bounds__(PQ_THREADS) void pq_encode_kernel(PqEncodeParams p) {
    __shared__ float half_norm[PQ_THREADS / 64][256];
    const int lane = mf_lane(), wave = mf_wave_id();
    const int64_t pos = (int64_t)blockIdx.x * 64 + lane;
    int64_t row = -1;
    if (pos < p.npos) row = p.row_of ? p.row_of[pos] : pos;
    if (row >= p.N) row = -1;
    const int64_t safe = row < 0 ? 0 : row;
    const float* x = p.rows + safe * p.d;
    const float* cen = p.centroids ? p.centroids + p.assign[safe] * p.d : nullptr;
    const int U = p.M < 4 ? p.M : 4;
    for (int m = wave; m < p.M; m += PQ_THREADS / 64) {                // (wave-uniform)
        const float* book = p.codebooks + (size_t)m * 256 * DSUB;
        mf_row_topk_sync<true>();                                  // the wave has read the last sub-space's norms
#pragma unroll
        for (int j = lane; j < 256; j += 64) {
            float b[DSUB];
            pq_load_sub<DSUB>(b, book + j * DSUB);
            half_norm[wave][j] = 0.5f * pq_chain<DSUB>(b, b);
        }
        mf_row_topk_sync<true>();
        float r[DSUB], c[DSUB];
        pq_load_sub<DSUB>(r, x + m * DSUB);
        if (cen) {
            pq_load_sub<DSUB>(c, cen + m * DSUB);
#pragma unroll
            for (int t = 0; t < DSUB; ++t) r[t] = r[t] - c[t];
        }
        mf_const_f32 bc = (mf_const_f32)book;                        // wave-uniform addresses: scalar loads
        float best = -INFINITY;
        int code = 0;
        for (int j = 0; j < 256; ++j) {
            const float s = pq_chain<DSUB>(r, bc + j * DSUB) - half_norm[wave][j];
            if (s > best) {                                        // strictly: the lowest j of equal scores stays
                best = s;
                code = j;
            }
        }
        if (pos < p.npos) {
            const unsigned char byte = row >= 0 ? (unsigned char)code : (unsigned char)0;
            if (p.row_of) p.codes[(((int64_t)blockIdx.x * (p.M / U) + m / U) * 64 + lane) * U + m % U] = byte;
            else if (row >= 0) p.codes[pos * p.M + m] = byte;
        }
    }
}

extern "C" int mf_pq_encode(const float* rows, int64_t N, int d, const float* centroids, const int64_t* assign, const float* codebooks,
                            int dsub, const int64_t* row_of, int64_t Npad, void* codes, mf_stream_t stream) {
    if (!rows || !codebooks || !codes || N <= 0 || (row_of ? (Npad < N || (Npad & 63) != 0) : Npad != N))
        return mf_set_error(MF_EINVAL, "mf_pq_encode: bad argument");
    if ((centroids == nullptr) != (assign == nullptr)) return mf_set_error(MF_EINVAL, "mf_pq_encode: centroids/assign mismatch");
    if (!mf_width_ok(d)) return mf_set_error(MF_EINVAL, "mf_pq_encode: embedding width %d not in {32,64,128,256}", d);
    if (!pq_dsub_ok(dsub) || d / dsub > PQ_MAX_M)
        return mf_set_error(MF_ENOTSUP, "mf_pq_encode: sub-vector length %d not in {4,8,16} or more than %d sub-vectors", dsub, PQ_MAX_M);
    if (Npad >= (1ll << 31) * 64) return mf_set_error(MF_ENOTSUP, "mf_pq_encode: too many rows");
    PqEncodeParams p{rows, centroids, assign, codebooks, row_of, N, Npad, d, d / dsub, static_cast<unsigned char*>(codes)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((Npad + 63) / 64));
    MF_TIMED("pq_encode", s, {
        if (dsub == 4) pq_encode_kernel<4><<<grid, PQ_THREADS, 0, s>>>(p);
        else if (dsub == 8) pq_encode_kernel<8><<<grid, PQ_THREADS, 0, s>>>(p);
        else pq_encode_kernel<16><<<grid, PQ_THREADS, 0, s>>>(p);
    });
    return mf_check_launch("mf_pq_encode");
}

// ------------------------------------------------------------------------ scan ----
// buf[0, n) in descending order, n a power of two <= PQ_BUF; every thread of the workgroup calls it
__device__ __forceinline__ void pq_sort_desc(unsigned long long* buf, int n) {
    const int tid = threadIdx.x;
    for (int k2 = 2; k2 <= n; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < n / 2; t += PQ_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                const unsigned long long a = buf[i], b = buf[l];
                const bool rising = (i & k2) != 0;                 // (never in the last round: the whole is descending)
                if (rising ? a > b : a < b) {
                    buf[i] = b;
                    buf[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

// The scan kernel in its two forms (mf_pq_scan.inc): as it was, and reading the allow bitmap of mf_pq_scan_allow.
#define MF_SCAN_KERNEL pq_scan_kernel
#define MF_SCAN_ALLOW false
#include "mf_pq_scan.inc"
#undef MF_SCAN_KERNEL
#undef MF_SCAN_ALLOW
#define MF_SCAN_KERNEL pq_scan_allow_kernel
#define MF_SCAN_ALLOW true
#include "mf_pq_scan.inc"
#undef MF_SCAN_KERNEL
#undef MF_SCAN_ALLOW

// ------------------------------------------------------------------ the plan ----
// (the rule: mf_cells_slices, with the candidate depth R and the key budget of the deep merge)
extern "C" int mf_pq_plan(int64_t Q, int nprobe, int R, int64_t max_cell_blocks, int64_t* out4) {
    return mf_cells_plan("mf_pq_plan", PQ_LISTS, Q, nprobe, R, max_cell_blocks, out4);
}

extern "C" size_t mf_pq_ws_bytes(int64_t Q, int nprobe, int R, int64_t max_cell_blocks) {
    return mf_cells_ws_bytes(PQ_LISTS, Q, nprobe, R, max_cell_blocks);
}

// Both exports: the scan's checks in the order their callers rely on, then -- with a bitmap -- the bitmap's (mf_cells_check_allow).
static int pq_scan_run(const char* who, const float* q, int64_t Q, const void* codes, const float* codebooks, int dsub, const int64_t* cell_blk,
                       const int64_t* row_of, int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes,
                       const float* probe_scores, int nprobe, int R, int S, const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base,
                       bool with_allow, const uint64_t* allow, int64_t n_masks, const int64_t* allow_of, void* ws, size_t ws_bytes,
                       mf_stream_t stream) {
    const bool pointers = q && codes && codebooks && cell_blk && row_of && probes && probe_scores && ws;
    if (const int rc = mf_cells_check_shape(who, PQ_LISTS, pointers, Q, Npad, N, C, d, max_cell_blocks, nprobe, R, S)) return rc;
    if (!pq_dsub_ok(dsub) || d / dsub > PQ_MAX_M)
        return mf_set_error(MF_ENOTSUP, "%s: sub-vector length %d not in {4,8,16} or more than %d sub-vectors", who, dsub, PQ_MAX_M);
    if (const int rc = mf_cells_check_lists(who, PQ_LISTS, Q, Npad, N, max_cell_blocks, nprobe, R, S, excl_off, excl_idx, idx_base, ws_bytes))
        return rc;
    if (with_allow)
        if (const int rc = mf_cells_check_allow(who, allow, n_masks, allow_of, Npad)) return rc;
    const int64_t G = (int64_t)nprobe * S;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PqScanParams p{q, codebooks, static_cast<const unsigned char*>(codes), cell_blk, row_of, probes, probe_scores, Q, C, nprobe, S, R,
                   excl_off, excl_idx, idx_base, static_cast<long long*>(ws),
                   {reinterpret_cast<const unsigned long long*>(allow), allow_of, n_masks, Npad / 64}};
    const dim3 grid((unsigned)(Q * G));
    if (with_allow) {
        PQ_DISPATCH(d, dsub, { MF_TIMED("pq_scan_allow", s, { pq_scan_allow_kernel<M, DSUB><<<grid, PQ_THREADS, 0, s>>>(p); }); });
    } else {
        PQ_DISPATCH(d, dsub, { MF_TIMED("pq_scan", s, { pq_scan_kernel<M, DSUB><<<grid, PQ_THREADS, 0, s>>>(p); }); });
    }
    return mf_check_launch(who);
}

extern "C" int mf_pq_scan(const float* q, int64_t Q, const void* codes, const float* codebooks, int dsub, const int64_t* cell_blk,
                          const int64_t* row_of, int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes,
                          const float* probe_scores, int nprobe, int R, int S, const int64_t* excl_off, const int64_t* excl_idx,
                          int64_t idx_base, void* ws, size_t ws_bytes, mf_stream_t stream) {
    return pq_scan_run("mf_pq_scan", q, Q, codes, codebooks, dsub, cell_blk, row_of, Npad, N, C, d, max_cell_blocks, probes, probe_scores, nprobe,
                       R, S, excl_off, excl_idx, idx_base, false, nullptr, 0, nullptr, ws, ws_bytes, stream);
}

extern "C" int mf_pq_scan_allow(const float* q, int64_t Q, const void* codes, const float* codebooks, int dsub, const int64_t* cell_blk,
                                const int64_t* row_of, int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks,
                                const int64_t* probes, const float* probe_scores, int nprobe, int R, int S, const int64_t* excl_off,
                                const int64_t* excl_idx, int64_t idx_base, const uint64_t* allow, int64_t n_masks, const int64_t* allow_of,
                                void* ws, size_t ws_bytes, mf_stream_t stream) {
    return pq_scan_run("mf_pq_scan_allow", q, Q, codes, codebooks, dsub, cell_blk, row_of, Npad, N, C, d, max_cell_blocks, probes, probe_scores,
                       nprobe, R, S, excl_off, excl_idx, idx_base, true, allow, n_masks, allow_of, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------- refine ----
template <int D>
__global__ __launch_bounds__(PQ_THREADS) void pq_refine_kernel(const float* __restrict__ q, const float* __restrict__ items,
                                                               const int64_t* __restrict__ cand, int R, int k, int64_t N, int64_t idx_base,
                                                               float* __restrict__ out_scores, int64_t* __restrict__ out_idx) {
    __shared__ unsigned long long all[PQ_THREADS], win[64], sorted[64];
    const int tid = threadIdx.x, lane = mf_lane();
    const int64_t qi = blockIdx.x;
    unsigned long long key = 0ull;
    if (tid < R) {
        const int64_t grow = cand[qi * R + tid], local = grow - idx_base;
        if (grow >= 0 && local >= 0 && local < N) {
            const f32x4* x = reinterpret_cast<const f32x4*>(items + local * D);
            mf_const_f32 qc = (mf_const_f32)q + (size_t)qi * D;
            float acc = 0.f;
#pragma unroll 4
            for (int g = 0; g < D / 8; ++g) {
                const f32x4 a = x[2 * g], b = x[2 * g + 1];
#pragma unroll
                for (int t = 0; t < 4; ++t) {                      // k order of mf_dot_chain
                    acc = __builtin_fmaf(a[t], qc[8 * g + t], acc);
                    acc = __builtin_fmaf(b[t], qc[8 * g + 4 + t], acc);
                }
            }
            key = mf_key_retrieval(acc, (unsigned)grow);
        }
    }
    all[tid] = key;
    __syncthreads();
    if (mf_wave_id() != 0) return;
    const int m = mf_row_topk<PQ_THREADS / 64, true>(all, PQ_THREADS, k, win, sorted);
    if (lane < k) mf_store_topk(out_scores, out_idx, qi, k, lane, lane < m ? sorted[lane] : 0ull, 0);
}

extern "C" int mf_pq_refine(const float* q, int64_t Q, const float* items, int64_t N, int d, const int64_t* cand, int R, int k,
                            int64_t idx_base, float* out_scores, int64_t* out_idx, mf_stream_t stream) {
    if (!q || !items || !cand || !out_scores || !out_idx || Q <= 0 || N <= 0 || Q >= (1ll << 31))
        return mf_set_error(MF_EINVAL, "mf_pq_refine: bad argument");
    if (k <= 0 || k > PQ_MAX_K) return mf_set_error(MF_ENOTSUP, "mf_pq_refine: k = %d outside 1..%d", k, PQ_MAX_K);
    if (R < k || R > PQ_MAX_R) return mf_set_error(MF_ENOTSUP, "mf_pq_refine: R = %d outside k..%d", R, PQ_MAX_R);
    if (!mf_width_ok(d)) return mf_set_error(MF_EINVAL, "mf_pq_refine: embedding width %d not in {32,64,128,256}", d);
    if (N >= (1ll << 31) || idx_base < 0 || idx_base + N > (1ll << 32))
        return mf_set_error(MF_ENOTSUP, "mf_pq_refine: item indices must fit 32 bits");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MF_DISPATCH_D(d, { MF_TIMED("pq_refine", s, { pq_refine_kernel<D><<<dim3((unsigned)Q), PQ_THREADS, 0, s>>>(q, items, cand, R, k, N, idx_base, out_scores, out_idx); }); });
    return mf_check_launch("mf_pq_refine");
}

// ----------------------------------------------------------------- deep refine ----
// The same refine for the lists of mf_pq_scan_deep: k and R up to PQ_BUF = MF_TOPK_DEEP_MAX_K.  A workgroup per query; thread t
// scores candidates t, t + 256, .. (four at most) with pq_refine_kernel's arithmetic -- the canonical chain on the original row,
// the key by the global row, key 0 for a -1 or out-of-range candidate --, the keys go to an LDS buffer of the power of two >= R
// (64 at least), pq_sort_desc orders it, and the first k entries leave with the standard tail.  The candidates of a query are
// distinct rows by contract (the merge's output): equal keys would be written twice.
template <int D>
__global__ __launch_bounds__(PQ_THREADS) void pq_refine_deep_kernel(const float* __restrict__ q, const float* __restrict__ items,
                                                                    const int64_t* __restrict__ cand, int R, int k, int64_t N,
                                                                    int64_t idx_base, float* __restrict__ out_scores,
                                                                    int64_t* __restrict__ out_idx) {
    __shared__ unsigned long long keys[PQ_BUF];
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    int n = 64;
    while (n < R) n <<= 1;                                         // (R <= PQ_BUF was checked)
    mf_const_f32 qc = (mf_const_f32)q + (size_t)qi * D;
    for (int c = tid; c < n; c += PQ_THREADS) {
        unsigned long long key = 0ull;
        if (c < R) {
            const int64_t grow = cand[qi * R + c], local = grow - idx_base;
            if (grow >= 0 && local >= 0 && local < N) {
                const f32x4* x = reinterpret_cast<const f32x4*>(items + local * D);
                float acc = 0.f;
#pragma unroll 4
                for (int g = 0; g < D / 8; ++g) {
                    const f32x4 a = x[2 * g], b = x[2 * g + 1];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {                  // k order of mf_dot_chain
                        acc = __builtin_fmaf(a[t], qc[8 * g + t], acc);
                        acc = __builtin_fmaf(b[t], qc[8 * g + 4 + t], acc);
                    }
                }
                key = mf_key_retrieval(acc, (unsigned)grow);
            }
        }
        keys[c] = key;
    }
    __syncthreads();
    pq_sort_desc(keys, n);                                         // (a barrier behind its last stage)
    for (int i = tid; i < k; i += PQ_THREADS) mf_store_topk(out_scores, out_idx, qi, k, i, keys[i], 0);
}

extern "C" int mf_pq_refine_deep(const float* q, int64_t Q, const float* items, int64_t N, int d, const int64_t* cand, int R, int k,
                                 int64_t idx_base, float* out_scores, int64_t* out_idx, mf_stream_t stream) {
    if (!q || !items || !cand || !out_scores || !out_idx || Q <= 0 || N <= 0 || Q >= (1ll << 31))
        return mf_set_error(MF_EINVAL, "mf_pq_refine_deep: bad argument");
    if (k <= 0 || k > PQ_BUF) return mf_set_error(MF_ENOTSUP, "mf_pq_refine_deep: k = %d outside 1..%d", k, PQ_BUF);
    if (R < k || R > PQ_BUF) return mf_set_error(MF_ENOTSUP, "mf_pq_refine_deep: R = %d outside k..%d", R, PQ_BUF);
    if (!mf_width_ok(d)) return mf_set_error(MF_EINVAL, "mf_pq_refine_deep: embedding width %d not in {32,64,128,256}", d);
    if (N >= (1ll << 31) || idx_base < 0 || idx_base + N > (1ll << 32))
        return mf_set_error(MF_ENOTSUP, "mf_pq_refine_deep: item indices must fit 32 bits");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MF_DISPATCH_D(d, { MF_TIMED("pq_refine_deep", s, { pq_refine_deep_kernel<D><<<dim3((unsigned)Q), PQ_THREADS, 0, s>>>(q, items, cand, R, k, N, idx_base, out_scores, out_idx); }); });
    return mf_check_launch("mf_pq_refine_deep");
}
