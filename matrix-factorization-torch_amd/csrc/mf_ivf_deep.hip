// mf_ivf_deep.hip -- deep lists (k up to MF_TOPK_DEEP_MAX_K = 1024) from the cell scan of mf_ivf.hip (gfx950).
//
// ivf_scan_kernel keeps a list per wave, so it stops at k = 64.  Here the same scan -- blockIdx.x = (q * nprobe + probe) * S +
// slice, a 64-row block per wave and pass, lane = row, the query in scalar registers, the canonical fmaf chain, the key by the
// ORIGINAL global row -- keeps its keys per WORKGROUP, as pq_scan_kernel does: one LDS buffer holds the best keys in
// descending order at the front, [0, kp), and the waiting ones behind them; `tau`, the k-th best key once k are held, is the
// bound a key has to beat before anything else is done with it.  The waves append through the per-pass count exchange of
// mf_pq_scan.inc (no atomics), and a settle -- a bitonic sort of the used part of the buffer -- runs when the next pass's 256
// keys might not fit.  Keys are unique (a key contains the row, a row lies in one cell), so what is kept does not depend on the
// order in which the waves append.  Every workgroup writes all k entries of its list [g = probe * S + slice][q][k], "none"
// for a probe outside [0, C), an empty cell, an empty slice or fewer rows than k: nothing to clear between calls.  The
// lists go to mf_topk_merge_packed_deep as they are.
//
//   * kp, the kept part, is a power of two >= k in classes (128 / 256 / 512 / 1024): a shallow request neither waits for
//     4,096 keys before its first bound nor sorts them.
//   * the sort: n keys, n a power of two, wave w owns the quarter [w n / 4, (w + 1) n / 4).  A compare-exchange distance of
//     n / 8 or less stays inside a quarter, and the LDS executes one wave's operations in order -- so of the log2(n) (log2(n) +
//     1) / 2 stages only the three with distance n / 4 or n / 2 need workgroup barriers (66 stages at n = 2,048, 78 at 4,096).
//   * ivf_scan_deep_allow_kernel: the same text reading an allow bitmap (mf_ivf_scan_allow's, a scalar load a block ahead).
//   * pq_deep_scan_kernel / pq_deep_scan_allow_kernel (mf_pq_deep_scan.inc, at the end): the same keeping over the quantised
//     cells of mf_pq.hip -- its tables and scoring, lists of up to 1,024 candidates for mf_pq_refine_deep.
#include "mf_cells.h"
#include "mf_pq_tables.h"
#include "mf_select.h"

// ---- the buffer's constants (tests/test_ivf_deep_cpu.py reads them from here)
static constexpr int IVFD_PASS = 64 * MF_CELLS_NW;     // threads of a workgroup = rows, so keys at most, of a pass
static constexpr int IVFD_KP_MIN = 128;                // the kept part: the power of two >= k, IVFD_KP_MIN at least
static constexpr int IVFD_KP_MAX = 1024;               // == MF_TOPK_DEEP_MAX_K
static constexpr int IVFD_BUF_MIN = 2048;              // keys of the buffer a scan uses: 4 kp, IVFD_BUF_MIN at least
static constexpr int IVFD_BUF = 4096;                  // keys of the buffer (32 KiB of LDS) = 4 * IVFD_KP_MAX
static constexpr int IVFD_SORT_MIN = 512;              // the shortest sort: 64 pairs per wave
static_assert(IVFD_KP_MAX == MF_TOPK_DEEP_MAX_K && IVFD_BUF == 4 * IVFD_KP_MAX && IVFD_PASS == 256, "mf_ivf_deep: buffer constants");
// lists of k <= 1,024 entries, G * k of a query within the 16,384 keys mf_topk_merge_packed_deep holds in LDS
static constexpr MfCellsLimits IVFD_LISTS{MF_TOPK_DEEP_MAX_K, MF_TOPK_MERGE_DEEP_MAX_KEYS, 'k'};

static inline int ivfd_kept(int k) {
    int kp = IVFD_KP_MIN;
    while (kp < k) kp <<= 1;
    return kp;
}
// Keys of the buffer a scan with kept part kp uses; it settles when more than ivfd_capacity(kp) - kp - IVFD_PASS keys wait.
__host__ __device__ static inline int ivfd_capacity(int kp) { return 4 * kp > IVFD_BUF_MIN ? 4 * kp : IVFD_BUF_MIN; }

struct IvfDeepParams {
    const float* blocked;       // [Npad / 64][D / 4][64][4]
    const float* q;             // [Q][D]
    const int64_t* cell_blk;    // [C + 1]: first 64-row block of every cell
    const int64_t* row_of;      // [Npad]: original row at a padded position, -1 for padding
    const int64_t* probes;      // [Q][nprobe]
    int64_t Q, C;
    int nprobe, S, k, kp;
    const int64_t *excl_off, *excl_idx;     // nullable
    int64_t idx_base;
    long long* out;             // [nprobe * S][Q][k] packed entries (mf_topk_io.h)
    MfCellsAllow allow;         // the ALLOW kernels' bitmap (mf_cells.h); the others never look at it
};

// buf[0, n) in descending order, n a power of two in [IVFD_SORT_MIN, IVFD_BUF]; every thread of the workgroup calls it.  What
// the other waves wrote before the call is seen (a barrier at the start), and the order by everyone after it (one at the end).
__device__ __forceinline__ void ivfd_sort_desc(unsigned long long* buf, int n) {
    const int lane = mf_lane(), wave = mf_wave_id();
    const int per = n / (2 * MF_CELLS_NW);                             // pairs of a wave: those of its quarter at j <= per
    __syncthreads();
    for (int k2 = 2; k2 <= n; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const bool cross = j > per;                                // (workgroup-uniform) partners in another wave's quarter
            if (cross) __syncthreads();
            for (int t = wave * per + lane; t < (wave + 1) * per; t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                const unsigned long long a = buf[i], b = buf[l];
                const bool rising = (i & k2) != 0;                     // (never in the last round: the whole is descending)
                if (rising ? a > b : a < b) {
                    buf[i] = b;
                    buf[l] = a;
                }
            }
            if (cross) __syncthreads();
            else mf_row_topk_sync<true>();
        }
    }
    __syncthreads();
}

// The scan kernel in its two forms (mf_ivf_deep_scan.inc): plain, and reading the allow bitmap of mf_ivf_scan_deep_allow.
#define MF_SCAN_KERNEL ivf_scan_deep_kernel
#define MF_SCAN_ALLOW false
#include "mf_ivf_deep_scan.inc"
#undef MF_SCAN_KERNEL
#undef MF_SCAN_ALLOW
#define MF_SCAN_KERNEL ivf_scan_deep_allow_kernel
#define MF_SCAN_ALLOW true
#include "mf_ivf_deep_scan.inc"
#undef MF_SCAN_KERNEL
#undef MF_SCAN_ALLOW

// ------------------------------------------------------------------ the plan ----
// (the rule: mf_cells_slices, with the key budget of the deep merge)
extern "C" int mf_ivf_deep_plan(int64_t Q, int nprobe, int k, int64_t max_cell_blocks, int64_t* out4) {
    return mf_cells_plan("mf_ivf_deep_plan", IVFD_LISTS, Q, nprobe, k, max_cell_blocks, out4);
}

extern "C" size_t mf_ivf_deep_ws_bytes(int64_t Q, int nprobe, int k, int64_t max_cell_blocks) {
    return mf_cells_ws_bytes(IVFD_LISTS, Q, nprobe, k, max_cell_blocks);
}

// Both exports: the scan's checks in the order their callers rely on, then -- with a bitmap -- the bitmap's (mf_cells_check_allow).
static int ivf_scan_deep_run(const char* who, const float* q, int64_t Q, const float* blocked, const int64_t* cell_blk, const int64_t* row_of,
                             int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes, int nprobe, int k, int S,
                             const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, bool with_allow, const uint64_t* allow,
                             int64_t n_masks, const int64_t* allow_of, void* ws, size_t ws_bytes, mf_stream_t stream) {
    if (const int rc = mf_cells_check_shape(who, IVFD_LISTS, q && blocked && cell_blk && row_of && probes && ws, Q, Npad, N, C, d, max_cell_blocks,
                                            nprobe, k, S))
        return rc;
    if (const int rc = mf_cells_check_lists(who, IVFD_LISTS, Q, Npad, N, max_cell_blocks, nprobe, k, S, excl_off, excl_idx, idx_base, ws_bytes))
        return rc;
    if (with_allow)
        if (const int rc = mf_cells_check_allow(who, allow, n_masks, allow_of, Npad)) return rc;
    const int64_t G = (int64_t)nprobe * S;
    hipStream_t s = static_cast<hipStream_t>(stream);
    IvfDeepParams p{blocked, q, cell_blk, row_of, probes, Q, C, nprobe, S, k, ivfd_kept(k), excl_off, excl_idx, idx_base, static_cast<long long*>(ws),
                    {reinterpret_cast<const unsigned long long*>(allow), allow_of, n_masks, Npad / 64}};
    const dim3 grid((unsigned)(Q * G));
    if (with_allow) {
        MF_DISPATCH_D(d, { MF_TIMED("ivf_scan_deep_allow", s, { ivf_scan_deep_allow_kernel<D><<<grid, IVFD_PASS, 0, s>>>(p); }); });
    } else {
        MF_DISPATCH_D(d, { MF_TIMED("ivf_scan_deep", s, { ivf_scan_deep_kernel<D><<<grid, IVFD_PASS, 0, s>>>(p); }); });
    }
    return mf_check_launch(who);
}

extern "C" int mf_ivf_scan_deep(const float* q, int64_t Q, const float* blocked, const int64_t* cell_blk, const int64_t* row_of, int64_t Npad,
                                int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes, int nprobe, int k, int S,
                                const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, void* ws, size_t ws_bytes,
                                mf_stream_t stream) {
    return ivf_scan_deep_run("mf_ivf_scan_deep", q, Q, blocked, cell_blk, row_of, Npad, N, C, d, max_cell_blocks, probes, nprobe, k, S, excl_off,
                             excl_idx, idx_base, false, nullptr, 0, nullptr, ws, ws_bytes, stream);
}

extern "C" int mf_ivf_scan_deep_allow(const float* q, int64_t Q, const float* blocked, const int64_t* cell_blk, const int64_t* row_of,
                                      int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes, int nprobe, int k,
                                      int S, const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, const uint64_t* allow,
                                      int64_t n_masks, const int64_t* allow_of, void* ws, size_t ws_bytes, mf_stream_t stream) {
    return ivf_scan_deep_run("mf_ivf_scan_deep_allow", q, Q, blocked, cell_blk, row_of, Npad, N, C, d, max_cell_blocks, probes, nprobe, k, S,
                             excl_off, excl_idx, idx_base, true, allow, n_masks, allow_of, ws, ws_bytes, stream);
}

// ---------------------------------------------------- deep lists from the quantised cells ----
// The scan of mf_pq.hip with the keeping above: lists of R <= 1,024 candidates, G * R of a query within the deep merge's keys.
// Static LDS: the query's tables, M KiB, beside the buffer -- M * 1024 + IVFD_BUF * 8 + 16 bytes, 34 KiB at M = 2, 96 KiB + 16
// at M = 64 (a CU's 160 KiB hold two workgroups at M = 32, one at M = 64).
static constexpr MfCellsLimits PQD_LISTS{MF_TOPK_DEEP_MAX_K, MF_TOPK_MERGE_DEEP_MAX_KEYS, 'R'};

#define MF_SCAN_KERNEL pq_deep_scan_kernel
#define MF_SCAN_ALLOW false
#include "mf_pq_deep_scan.inc"
#undef MF_SCAN_KERNEL
#undef MF_SCAN_ALLOW
#define MF_SCAN_KERNEL pq_deep_scan_allow_kernel
#define MF_SCAN_ALLOW true
#include "mf_pq_deep_scan.inc"
#undef MF_SCAN_KERNEL
#undef MF_SCAN_ALLOW

extern "C" int mf_pq_deep_plan(int64_t Q, int nprobe, int R, int64_t max_cell_blocks, int64_t* out4) {
    return mf_cells_plan("mf_pq_deep_plan", PQD_LISTS, Q, nprobe, R, max_cell_blocks, out4);
}

extern "C" size_t mf_pq_deep_ws_bytes(int64_t Q, int nprobe, int R, int64_t max_cell_blocks) {
    return mf_cells_ws_bytes(PQD_LISTS, Q, nprobe, R, max_cell_blocks);
}

// Both exports: mf_pq_scan's checks in its order and words, with the deep limits.
static int pq_scan_deep_run(const char* who, const float* q, int64_t Q, const void* codes, const float* codebooks, int dsub,
                            const int64_t* cell_blk, const int64_t* row_of, int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks,
                            const int64_t* probes, const float* probe_scores, int nprobe, int R, int S, const int64_t* excl_off,
                            const int64_t* excl_idx, int64_t idx_base, bool with_allow, const uint64_t* allow, int64_t n_masks,
                            const int64_t* allow_of, void* ws, size_t ws_bytes, mf_stream_t stream) {
    const bool pointers = q && codes && codebooks && cell_blk && row_of && probes && probe_scores && ws;
    if (const int rc = mf_cells_check_shape(who, PQD_LISTS, pointers, Q, Npad, N, C, d, max_cell_blocks, nprobe, R, S)) return rc;
    if (!pq_dsub_ok(dsub) || d / dsub > PQ_MAX_M)
        return mf_set_error(MF_ENOTSUP, "%s: sub-vector length %d not in {4,8,16} or more than %d sub-vectors", who, dsub, PQ_MAX_M);
    if (const int rc = mf_cells_check_lists(who, PQD_LISTS, Q, Npad, N, max_cell_blocks, nprobe, R, S, excl_off, excl_idx, idx_base, ws_bytes))
        return rc;
    if (with_allow)
        if (const int rc = mf_cells_check_allow(who, allow, n_masks, allow_of, Npad)) return rc;
    const int64_t G = (int64_t)nprobe * S;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PqScanParams p{q, codebooks, static_cast<const unsigned char*>(codes), cell_blk, row_of, probes, probe_scores, Q, C, nprobe, S, R,
                   excl_off, excl_idx, idx_base, static_cast<long long*>(ws),
                   {reinterpret_cast<const unsigned long long*>(allow), allow_of, n_masks, Npad / 64}};
    const int kp = ivfd_kept(R);
    const dim3 grid((unsigned)(Q * G));
    if (with_allow) {
        PQ_DISPATCH(d, dsub, { MF_TIMED("pq_scan_deep_allow", s, { pq_deep_scan_allow_kernel<M, DSUB><<<grid, IVFD_PASS, 0, s>>>(p, kp); }); });
    } else {
        PQ_DISPATCH(d, dsub, { MF_TIMED("pq_scan_deep", s, { pq_deep_scan_kernel<M, DSUB><<<grid, IVFD_PASS, 0, s>>>(p, kp); }); });
    }
    return mf_check_launch(who);
}

extern "C" int mf_pq_scan_deep(const float* q, int64_t Q, const void* codes, const float* codebooks, int dsub, const int64_t* cell_blk,
                               const int64_t* row_of, int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks,
                               const int64_t* probes, const float* probe_scores, int nprobe, int R, int S, const int64_t* excl_off,
                               const int64_t* excl_idx, int64_t idx_base, void* ws, size_t ws_bytes, mf_stream_t stream) {
    return pq_scan_deep_run("mf_pq_scan_deep", q, Q, codes, codebooks, dsub, cell_blk, row_of, Npad, N, C, d, max_cell_blocks, probes,
                            probe_scores, nprobe, R, S, excl_off, excl_idx, idx_base, false, nullptr, 0, nullptr, ws, ws_bytes, stream);
}

extern "C" int mf_pq_scan_deep_allow(const float* q, int64_t Q, const void* codes, const float* codebooks, int dsub, const int64_t* cell_blk,
                                     const int64_t* row_of, int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks,
                                     const int64_t* probes, const float* probe_scores, int nprobe, int R, int S, const int64_t* excl_off,
                                     const int64_t* excl_idx, int64_t idx_base, const uint64_t* allow, int64_t n_masks,
                                     const int64_t* allow_of, void* ws, size_t ws_bytes, mf_stream_t stream) {
    return pq_scan_deep_run("mf_pq_scan_deep_allow", q, Q, codes, codebooks, dsub, cell_blk, row_of, Npad, N, C, d, max_cell_blocks, probes,
                            probe_scores, nprobe, R, S, excl_off, excl_idx, idx_base, true, allow, n_masks, allow_of, ws, ws_bytes, stream);
}
