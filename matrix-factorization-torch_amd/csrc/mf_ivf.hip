// mf_ivf.hip -- partitioned (inverted-file) retrieval: a query scans the cells it probes, exactly (gfx950).
//
// The reference does not search its whole catalog per query: ItemProcessor.get_index builds an inverted-file index
// (num_partitions, xfmr_rec/data/lightning.py:203, 222-229) and search visits num_probes = 8 partitions (:250-259),
// scoring their rows through a product quantiser.  Here the only approximate step is WHICH rows are looked at: the
// catalog is kept a second time ordered by cell, every cell padded to whole 64-row blocks, in the blocked layout of the
// few-query scan (mf_topk_small.hip: [64-row block][16-byte chunk][row], one coalesced 1 KiB load per chunk and wave);
// every row of a probed cell is scored with the canonical fmaf chain (mf_numerics.h) and keyed by its ORIGINAL row, so
// the result is bit for bit the exact engines' answer over the union of the probed cells -- and with every cell probed
// their answer over the catalog.
//
//   * ivf_scan_kernel: a 256-thread workgroup takes one (query, probe, slice) and walks the 64-row blocks of that slice
//     of cell probes[q][p], a block per wave and pass, lane = row, the query in scalar registers.  A wave keeps its k best
//     keys in LDS and their k-th as a bound; a key has to beat the bound before anything else is done with it (the
//     exclusion list is only asked about such keys), and the selection (mf_row_topk of mf_select.h) runs only when 64
//     such keys are waiting.  The four waves' lists are joined by one more selection and leave as one partial list of the
//     packed form [G = nprobe * S][Q][k] that mf_topk_merge_packed takes.  No atomics, nothing to clear between calls: every
//     workgroup writes all k entries of its list, "none" for a probe outside [0, C), an empty cell or an empty slice.
//     The exclusion look-up, the packed entry, the slice plan and the export's checks are mf_cells.h's, shared with
//     mf_pq.hip; the scoring and the selection are this kernel's own.
//   * ivf_scan_allow_kernel: the same kernel text (mf_ivf_scan.inc) reading an allow bitmap, one 64-bit word per 64-row block
//     (mf_filter_cell_bits): a row whose bit is clear has key 0, a block whose word is 0 is skipped -- mf_ivf_scan_allow.
//   * ivf_cell_mean_kernel: the k-means update of the build -- a cell's rows added in a given order by one thread per
//     dimension (no float atomics: the same bits every run), then the mean and its L2 normalisation.
#include "mf_cells.h"
#include "mf_select.h"

static constexpr int IVF_MAX_K = 64;           // one wavefront holds a list
static constexpr int IVF_PEND = 128;           // keys a wave collects between selections (a block adds at most 64)
// lists of k <= 64 entries, G * k of a query within the 8,192 keys mf_topk_merge / mf_topk_merge_packed hold in LDS
static constexpr MfCellsLimits IVF_LISTS{IVF_MAX_K, 8192, 'k'};

struct IvfParams {
    const float* blocked;       // [Npad / 64][D / 4][64][4]
    const float* q;             // [Q][D]
    const int64_t* cell_blk;    // [C + 1]: first 64-row block of every cell
    const int64_t* row_of;      // [Npad]: original row at a padded position, -1 for padding
    const int64_t* probes;      // [Q][nprobe]
    int64_t Q, C;
    int nprobe, S, k;
    const int64_t *excl_off, *excl_idx;     // nullable
    int64_t idx_base;
    long long* out;             // [nprobe * S][Q][k] packed entries (mf_topk_io.h)
    MfCellsAllow allow;         // the ALLOW kernels' bitmap (mf_cells.h); the others never look at it
};

// The scan kernel in its two forms (mf_ivf_scan.inc): as it was, and reading the allow bitmap of mf_ivf_scan_allow.
#define MF_SCAN_KERNEL ivf_scan_kernel
#define MF_SCAN_ALLOW false
#include "mf_ivf_scan.inc"
#undef MF_SCAN_KERNEL
#undef MF_SCAN_ALLOW
#define MF_SCAN_KERNEL ivf_scan_allow_kernel
#define MF_SCAN_ALLOW true
#include "mf_ivf_scan.inc"
#undef MF_SCAN_KERNEL
#undef MF_SCAN_ALLOW

// ------------------------------------------------------------------ the plan ----
// (the rule: mf_cells_slices)
extern "C" int mf_ivf_plan(int64_t Q, int nprobe, int k, int64_t max_cell_blocks, int64_t* out4) {
    return mf_cells_plan("mf_ivf_plan", IVF_LISTS, Q, nprobe, k, max_cell_blocks, out4);
}

extern "C" size_t mf_ivf_ws_bytes(int64_t Q, int nprobe, int k, int64_t max_cell_blocks) {
    return mf_cells_ws_bytes(IVF_LISTS, Q, nprobe, k, max_cell_blocks);
}

// Both exports: the scan's checks in the order their callers rely on, then -- with a bitmap -- the bitmap's (mf_cells_check_allow).
static int ivf_scan_run(const char* who, const float* q, int64_t Q, const float* blocked, const int64_t* cell_blk, const int64_t* row_of,
                        int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes, int nprobe, int k, int S,
                        const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, bool with_allow, const uint64_t* allow,
                        int64_t n_masks, const int64_t* allow_of, void* ws, size_t ws_bytes, mf_stream_t stream) {
    if (const int rc = mf_cells_check_shape(who, IVF_LISTS, q && blocked && cell_blk && row_of && probes && ws, Q, Npad, N, C, d, max_cell_blocks,
                                            nprobe, k, S))
        return rc;
    if (const int rc = mf_cells_check_lists(who, IVF_LISTS, Q, Npad, N, max_cell_blocks, nprobe, k, S, excl_off, excl_idx, idx_base, ws_bytes))
        return rc;
    if (with_allow)
        if (const int rc = mf_cells_check_allow(who, allow, n_masks, allow_of, Npad)) return rc;
    const int64_t G = (int64_t)nprobe * S;
    hipStream_t s = static_cast<hipStream_t>(stream);
    IvfParams p{blocked, q, cell_blk, row_of, probes, Q, C, nprobe, S, k, excl_off, excl_idx, idx_base, static_cast<long long*>(ws),
                {reinterpret_cast<const unsigned long long*>(allow), allow_of, n_masks, Npad / 64}};
    const dim3 grid((unsigned)(Q * G));
    if (with_allow) {
        MF_DISPATCH_D(d, { MF_TIMED("ivf_scan_allow", s, { ivf_scan_allow_kernel<D><<<grid, 64 * MF_CELLS_NW, 0, s>>>(p); }); });
    } else {
        MF_DISPATCH_D(d, { MF_TIMED("ivf_scan", s, { ivf_scan_kernel<D><<<grid, 64 * MF_CELLS_NW, 0, s>>>(p); }); });
    }
    return mf_check_launch(who);
}

extern "C" int mf_ivf_scan(const float* q, int64_t Q, const float* blocked, const int64_t* cell_blk, const int64_t* row_of, int64_t Npad,
                           int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes, int nprobe, int k, int S,
                           const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, void* ws, size_t ws_bytes,
                           mf_stream_t stream) {
    return ivf_scan_run("mf_ivf_scan", q, Q, blocked, cell_blk, row_of, Npad, N, C, d, max_cell_blocks, probes, nprobe, k, S, excl_off, excl_idx,
                        idx_base, false, nullptr, 0, nullptr, ws, ws_bytes, stream);
}

extern "C" int mf_ivf_scan_allow(const float* q, int64_t Q, const float* blocked, const int64_t* cell_blk, const int64_t* row_of, int64_t Npad,
                                 int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes, int nprobe, int k, int S,
                                 const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, const uint64_t* allow, int64_t n_masks,
                                 const int64_t* allow_of, void* ws, size_t ws_bytes, mf_stream_t stream) {
    return ivf_scan_run("mf_ivf_scan_allow", q, Q, blocked, cell_blk, row_of, Npad, N, C, d, max_cell_blocks, probes, nprobe, k, S, excl_off,
                        excl_idx, idx_base, true, allow, n_masks, allow_of, ws, ws_bytes, stream);
}

// ------------------------------------------------------------- k-means update ----
// One workgroup per cell, thread t = dimension t: the cell's rows order[cell_off[c] .. cell_off[c + 1]) are added one after
// the other (eight loads in flight, the additions in list order), so the sum does not depend on scheduling.  out[c] = the
// mean, or (normalize) the mean scaled to unit L2 length -- its square norm added in dimension order by every thread alike.
// An empty cell leaves out[c] as it is; a mean of norm zero is written as it is.
__global__ __launch_bounds__(256) void ivf_cell_mean_kernel(const float* __restrict__ items, int d, const int64_t* __restrict__ order,
                                                            const int64_t* __restrict__ cell_off, int normalize, float* __restrict__ out) {
    __shared__ float sq[256];
    const int64_t c = blockIdx.x;
    const int t = threadIdx.x;
    const int64_t i0 = cell_off[c], i1 = cell_off[c + 1];
    if (i0 >= i1) return;                                          // (workgroup-uniform)
    float sum = 0.f;
    if (t < d) {
        for (int64_t i = i0; i < i1; i += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = i + u < i1 ? items[order[i + u] * d + t] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (i + u < i1) sum = sum + v[u];
        }
    }
    float mean = sum / (float)(i1 - i0);
    if (normalize) {
        sq[t] = t < d ? mean * mean : 0.f;
        __syncthreads();
        float n2 = 0.f;
        for (int j = 0; j < d; ++j) n2 = n2 + sq[j];
        if (n2 > 0.f) mean = mean / __builtin_sqrtf(n2);
    }
    if (t < d) out[c * d + t] = mean;
}

extern "C" int mf_ivf_cell_mean(const float* items, int64_t N, int d, const int64_t* order, const int64_t* cell_off, int64_t C,
                                int normalize, float* out, mf_stream_t stream) {
    if (!items || !order || !cell_off || !out || N <= 0 || C <= 0 || C >= (1ll << 31)) return mf_set_error(MF_EINVAL, "mf_ivf_cell_mean: bad argument");
    if (!mf_width_ok(d)) return mf_set_error(MF_EINVAL, "mf_ivf_cell_mean: embedding width %d not in {32,64,128,256}", d);
    ivf_cell_mean_kernel<<<dim3((unsigned)C), 256, 0, static_cast<hipStream_t>(stream)>>>(items, d, order, cell_off, normalize, out);
    return mf_check_launch("mf_ivf_cell_mean");
}
