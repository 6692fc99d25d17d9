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
};

template <int D>
__global__ __launch_bounds__(64 * MF_CELLS_NW) void ivf_scan_kernel(IvfParams p) {
    constexpr int CPR = D / 4;
    constexpr int HALF = CPR > 32 ? 32 : CPR;                  // chunks held in registers at once
    __shared__ unsigned long long buf[MF_CELLS_NW][64 + IVF_PEND];  // per wave: its best keys so far [0, 64), then the waiting ones
    __shared__ unsigned long long win[MF_CELLS_NW][64], sorted[MF_CELLS_NW][64];
    __shared__ unsigned long long all[MF_CELLS_NW * 64];
    const int lane = mf_lane(), wave = mf_wave_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    // blockIdx.x = (q * nprobe + probe) * S + slice: everything here is workgroup-uniform (mf_pq.hip has the same lines: mf_cells.h)
    const int64_t wg = blockIdx.x;
    const int slice = (int)(wg % p.S);
    const int probe = (int)((wg / p.S) % p.nprobe);
    const int64_t q = wg / ((int64_t)p.S * p.nprobe);
    const int64_t cell = p.probes[q * p.nprobe + probe];
    int64_t b0 = 0, b1 = 0;
    if (cell >= 0 && cell < p.C) {
        const int64_t c0 = p.cell_blk[cell], nb = p.cell_blk[cell + 1] - c0;
        b0 = c0 + nb * slice / p.S;
        b1 = c0 + nb * (slice + 1) / p.S;
    }
    mf_const_f32 qc = (mf_const_f32)p.q + (size_t)q * D;
    int64_t e0 = 0, e1 = 0;
    if (p.excl_off) {
        e0 = p.excl_off[q];
        e1 = p.excl_off[q + 1];
    }
    unsigned long long* mine = buf[wave];
#pragma unroll
    for (int j = 0; j < (64 + IVF_PEND) / 64; ++j) mine[lane + 64 * j] = 0ull;
    unsigned long long tau = 0ull;             // the wave's k-th best key once it holds k: only a larger key matters
    int pend = 0;
    // the k best of the wave's list and what waits behind it, in descending order at the front; the rest cleared
    auto settle = [&]() {
        mf_row_topk_sync<true>();
        const int m = mf_row_topk<(64 + IVF_PEND) / 64, true>(mine, 64 + IVF_PEND, p.k, win[wave], sorted[wave]);
        const unsigned long long keep = lane < m ? sorted[wave][lane] : 0ull;
        tau = m >= p.k ? sorted[wave][p.k - 1] : 0ull;
        mf_row_topk_sync<true>();
#pragma unroll
        for (int j = 0; j < (64 + IVF_PEND) / 64; ++j) mine[lane + 64 * j] = j == 0 ? keep : 0ull;
        pend = 0;
        mf_row_topk_sync<true>();
    };

    for (int64_t blk = b0 + wave; blk < b1; blk += MF_CELLS_NW) {
        const f32x4* src = reinterpret_cast<const f32x4*>(p.blocked) + blk * (int64_t)CPR * 64 + lane;
        const int64_t orig = p.row_of[blk * 64 + lane];
        f32x4 rc[HALF];
        float acc = 0.f;
#pragma unroll
        for (int h0 = 0; h0 < CPR; h0 += HALF) {
#pragma unroll
            for (int j = 0; j < HALF; ++j) rc[j] = src[(int64_t)(h0 + j) * 64];
#pragma unroll
            for (int g = 0; g < HALF / 2; ++g) {
                const f32x4 a = rc[2 * g], b = rc[2 * g + 1];
                mf_const_f32 qv = qc + 4 * (h0 + 2 * g);         // wave-uniform address: scalar loads
#pragma unroll
                for (int t = 0; t < 4; ++t) {                      // k order of mf_dot_chain
                    acc = __builtin_fmaf(a[t], qv[t], acc);
                    acc = __builtin_fmaf(b[t], qv[4 + t], acc);
                }
            }
        }
        const unsigned grow = (unsigned)(p.idx_base + orig);       // the GLOBAL row: ties break by it whatever the permutation
        const unsigned long long key = orig >= 0 ? mf_key_retrieval(acc, grow) : 0ull;
        bool pass = key > tau;
        if (p.excl_off) pass = mf_cells_admit(pass, grow, p.excl_idx, e0, e1, lane);
        const unsigned long long bal = __ballot(pass);
        if (bal) {
            if (pass) mine[64 + pend + __popcll(bal & below)] = key;
            pend += __popcll(bal);
            if (pend > IVF_PEND - 64) settle();                    // no room for another block's 64
        }
    }
    if (pend > 0) settle();                                        // (else the front is in order already: zeros, or the last settle)
    mf_row_topk_sync<true>();
    all[wave * 64 + lane] = mine[lane];
    __syncthreads();
    if (wave != 0) return;
    const int m = mf_row_topk<MF_CELLS_NW, true>(all, MF_CELLS_NW * 64, p.k, win[0], sorted[0]);
    if (lane < p.k) {
        const long long v = lane < m ? mf_cells_entry(sorted[0][lane]) : MF_PACKED_NONE;
        const int64_t g = (int64_t)probe * p.S + slice;
        p.out[(g * p.Q + q) * p.k + lane] = v;
    }
}

// ------------------------------------------------------------------ the plan ----
// (the rule: mf_cells_slices)
extern "C" int mf_ivf_plan(int64_t Q, int nprobe, int k, int64_t max_cell_blocks, int64_t* out4) {
    return mf_cells_plan("mf_ivf_plan", IVF_LISTS, Q, nprobe, k, max_cell_blocks, out4);
}

extern "C" size_t mf_ivf_ws_bytes(int64_t Q, int nprobe, int k, int64_t max_cell_blocks) {
    return mf_cells_ws_bytes(IVF_LISTS, Q, nprobe, k, max_cell_blocks);
}

extern "C" int mf_ivf_scan(const float* q, int64_t Q, const float* blocked, const int64_t* cell_blk, const int64_t* row_of, int64_t Npad,
                           int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes, int nprobe, int k, int S,
                           const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, void* ws, size_t ws_bytes,
                           mf_stream_t stream) {
    if (const int rc = mf_cells_check_shape("mf_ivf_scan", IVF_LISTS, q && blocked && cell_blk && row_of && probes && ws, Q, Npad, N, C, d,
                                            max_cell_blocks, nprobe, k, S))
        return rc;
    if (const int rc = mf_cells_check_lists("mf_ivf_scan", IVF_LISTS, Q, Npad, N, max_cell_blocks, nprobe, k, S, excl_off, excl_idx, idx_base, ws_bytes))
        return rc;
    const int64_t G = (int64_t)nprobe * S;
    hipStream_t s = static_cast<hipStream_t>(stream);
    IvfParams p{blocked, q, cell_blk, row_of, probes, Q, C, nprobe, S, k, excl_off, excl_idx, idx_base, static_cast<long long*>(ws)};
    MF_DISPATCH_D(d, { MF_TIMED("ivf_scan", s, { ivf_scan_kernel<D><<<dim3((unsigned)(Q * G)), 64 * MF_CELLS_NW, 0, s>>>(p); }); });
    return mf_check_launch("mf_ivf_scan");
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
