// mf_coalesce.h -- the list towers' backward (mf_pool.hip: history tower, mf_bag.hip: feature-bag towers, mf_xfmr.hip:
// transformer tower): every (entry, gradient row) a step parks on one table, coalesced into ONE list of (id, summed row)
// for the sparse updates.  What the towers share beyond this engine -- id validity, the list clamp and cut, the owner
// search, the block scan, stride_grid -- is in mf_lists.h, included here.
//
// Entries are numbered q = 0 .. n: the explicit (ids, grad) rows first (valid ids [0, n_rows)), then pooled entry h = q -
// n_extra, whose owner b is the last with ent_off[b] <= h and whose list position is lo[b] + h - ent_off[b].  The entry
// count n = n_extra + min(ent_off[B], n_entries) stays on the device (the keys kernel leaves it there); the host bound
// n_extra + n_entries sizes every buffer and grid, and the kernels exit early past n.  Hence no host read: a step can be
// captured as a graph.
//
// Keys (id, or n_rows for an entry that carries nothing) are sorted with a stable LSD radix sort: 8-bit digits, ballot
// multi-split inside a wave, linear, no atomics but the integer LDS digit counts.  The runs of equal ids are summed in
// sorted order (= entry order) by a fixed tree of fan-out RUN_CHUNK over sorted positions.  The result is exactly
// `capacity` = min(n_rows, n_extra + n_entries) slots: the unique ids ascending with their summed rows, then id -1 (skipped
// by every update kernel).  Entries with key n_rows sort last, and the tree depends only on where the valid entries sit,
// so the result is bit-identical whatever the host bound.
//
// A tower supplies the entries as a struct E with
//     __device__ uint32_t key(int64_t b, int64_t pos) const         the id of owner b's entry at list position pos, or
//                                                                    n_rows when it carries no gradient;
//     template <int D> __device__ f32x4 grad(int64_t b, int64_t h, int c) const
//                                                                    lane c's four floats of entry h's gradient row (only
//                                                                    called for entries with a valid key).
#pragma once
#include "mf_lists.h"
#include "mf_update.h"

static constexpr int COALESCE_MAX_ROWS = 1 << 20;   // table rows the sort covers (keys <= 2^20: three 8-bit digits)

struct CoalesceSrc {                 // what one call coalesces
    int64_t n_rows;                  // (first: see coalesce_segsum_kernel)
    const int64_t* extra_ids;        // [n_extra] explicit rows, first
    const float* extra_grad;         // [n_extra, d]
    int64_t n_extra;
    const int64_t* lo;               // [B] first list position of owner b's entries
    const int64_t* ent_off;          // [B + 1] number of owner b's first entry; ent_off[B] = the entry count
    int64_t B;
    int64_t n_entries;               // host bound of ent_off[B]
};

struct CoalesceWs {
    uint32_t *k0, *v0, *k1, *v1;
    int32_t *n_dev, *euser, *hist, *tcount, *head_pos;
    float* partial;
    int ntiles;
};
// carves the workspace of a call with n_extra + n_entries entries of width d from `a`
CoalesceWs coalesce_ws(MfArena& a, int64_t n_extra, int64_t n_entries, int d);
// its size: what stands behind the towers' *_backward_ws_bytes / *_coalesce_ws_bytes exports
size_t coalesce_ws_bytes(int64_t n_extra, int64_t n_entries, int d);
// The entry checks every backward shares, with the codes and texts they always had: the explicit rows, the table's size
// (`rows`: how `who` calls the table's rows), the entry count, capacity = min(n_rows, n_extra + n_entries), the workspace.
int coalesce_check(const char* who, const char* rows, int64_t n_rows, int64_t n_extra, const int64_t* extra_ids, const float* extra_grad,
                   int64_t n_entries, int64_t capacity, const void* ws, size_t ws_bytes, size_t need_bytes);
// the radix sort of the keys left by coalesce_keys_kernel, the run heads and the -1 fill of out_ids; returns the sorted
// keys and values
void coalesce_sort(const CoalesceWs& w, int64_t n_rows, int64_t capacity, int64_t* out_ids, hipStream_t s,
                   const uint32_t*& sk, const uint32_t*& sv);

// keys (and values = entry numbers, and the owner of every pooled entry); leaves n on the device
template <class E>
__global__ __launch_bounds__(256) void coalesce_keys_kernel(CoalesceSrc src, E ent, CoalesceWs w) {
    const int64_t n = src.n_extra + min(src.ent_off[src.B], src.n_entries);
    if (blockIdx.x == 0 && threadIdx.x == 0) *w.n_dev = (int32_t)n;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += stride) {
        uint32_t key = (uint32_t)src.n_rows;
        if (q < src.n_extra) {
            const long long id = src.extra_ids[q];
            if (id >= 0 && id < src.n_rows) key = (uint32_t)id;
        } else {
            const int64_t h = q - src.n_extra;
            const int64_t b = list_owner(src.ent_off, src.B, h);
            key = ent.key(b, src.lo[b] + (h - src.ent_off[b]));
            w.euser[h] = (int32_t)b;
        }
        w.k0[q] = key;
        w.v0[q] = (uint32_t)q;
    }
}

// gradient row (lane c's 4 floats) of entry v: an explicit row, or the tower's row of a pooled entry
template <int D, class E>
__device__ __forceinline__ f32x4 coalesce_leaf(const CoalesceSrc& src, const int32_t* __restrict__ euser, const E& ent, uint32_t v, int c) {
    if ((int64_t)v < src.n_extra) return reinterpret_cast<const f32x4*>(src.extra_grad + (int64_t)v * D)[c];
    const int64_t h = (int64_t)v - src.n_extra;
    return ent.template grad<D>(euser[h], h, c);
}

// The runs' sums in sorted order, as a fixed tree of fan-out RUN_CHUNK over sorted positions, one launch per level, so that
// an id in a hundred thousand lists is summed by thousands of lane groups, not by one (update_rows_kernel's two levels
// would leave ~n / 32 partials to one group).  Level 1: the owner of every RUN_CHUNK-aligned unit of a run (its first
// position: the run's head or the unit's start) sums the unit's gradient rows in order.  Level L >= 2 (unit = 32^(L-1)
// positions, block = 32^L): the owner of the run's part of a block adds the level-(L-1) partials of its units, in order.
// A run that ends inside an owner's unit is written to its slot at that level; otherwise the sum is parked at the owner's
// position.  The tree depends on sorted positions only: deterministic.  Most work items of the upper levels exit at once:
// what they read (n_dev .. unit, src.n_rows) leads the kernel arguments, so that it arrives in as few scalar loads.
template <int D, class E>
__global__ __launch_bounds__(256) void coalesce_segsum_kernel(const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv,
                                                              const int32_t* __restrict__ n_dev, const int32_t* __restrict__ head_pos,
                                                              const int32_t* __restrict__ n_unique, int64_t capacity, int64_t unit,
                                                              CoalesceSrc src, const int32_t* __restrict__ euser,
                                                              float* __restrict__ partial, int64_t* __restrict__ out_ids,
                                                              float* __restrict__ out_grad, E ent) {
    constexpr int LPR = D / 4, RPW = 64 / LPR;
    const int lane = mf_lane(), c = lane % LPR;
    const int64_t n = *n_dev;
    const uint32_t n_rows = (uint32_t)src.n_rows;
    // work items: the runs (by output slot), then the blocks of this level (a block start inside a run owns the run's part)
    const int64_t i = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + lane / LPR;
    const int64_t block = unit * RUN_CHUNK;
    int64_t p, sl = -1;
    bool head;
    if (i < capacity) {
        if (i >= *n_unique) return;                      // (no cross-lane operation below)
        sl = i;
        p = head_pos[i];
        head = true;
    } else {
        p = (i - capacity) * block;
        if (p >= n || sk[p] >= n_rows || p == 0 || sk[p - 1] != sk[p]) return;   // past the end, padding, or a run's head
        head = false;
    }
    const uint32_t key = sk[p];
    const int64_t sub = unit / RUN_CHUNK;                // the level below (0: entries)
    const int64_t sub_end = sub ? (p / unit + 1) * unit : p + 1;
    if (sub && head && (sub_end >= n || sk[sub_end] != key)) return;   // finished at a lower level
    const int64_t block_end = min((p / block + 1) * block, n);
    // four positions at a time: their keys, then their rows (or partials), each batch of loads in flight together
    constexpr int NB = 4;
    const int64_t step = sub ? unit : 1;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int64_t e = p;
    if (sub) {
        acc = reinterpret_cast<const f32x4*>(partial + p * D)[c];
        e = sub_end;
    }
    for (;;) {
        uint32_t k8[NB];
#pragma unroll
        for (int t = 0; t < NB; ++t) k8[t] = e + t * step < block_end ? sk[e + t * step] : 0xFFFFFFFFu;
        int m = 0;
#pragma unroll
        for (int t = 0; t < NB; ++t) m += (m == t && k8[t] == key) ? 1 : 0;      // leading positions of the run
        f32x4 g[NB];
        if (!sub) {
            uint32_t v8[NB];
#pragma unroll
            for (int t = 0; t < NB; ++t) v8[t] = t < m ? sv[e + t] : 0u;
#pragma unroll
            for (int t = 0; t < NB; ++t)
                if (t < m) g[t] = coalesce_leaf<D>(src, euser, ent, v8[t], c);
        } else {
#pragma unroll
            for (int t = 0; t < NB; ++t)
                if (t < m) g[t] = reinterpret_cast<const f32x4*>(partial + (e + t * step) * D)[c];
        }
#pragma unroll
        for (int t = 0; t < NB; ++t)
            if (t < m) acc += g[t];
        e += m * step;
        if (m < NB || e >= block_end) break;
    }
    e = min(e, block_end);
    if (head && (e >= n || sk[e] != key)) {              // the whole run
        reinterpret_cast<f32x4*>(out_grad + sl * D)[c] = acc;
        if (c == 0) out_ids[sl] = key;
    } else {
        reinterpret_cast<f32x4*>(partial + p * D)[c] = acc;
    }
}

// The whole coalesce on stream s; segsum_span (nullable) names the mf_timing span around the run sums.  d is checked by
// the caller.
template <class E>
int coalesce(const CoalesceSrc& src, const E& ent, const CoalesceWs& w, int d, int64_t capacity, int64_t* out_ids, float* out_grad,
             const char* segsum_span, hipStream_t s) {
    const int64_t n_cap = src.n_extra + src.n_entries;
    coalesce_keys_kernel<E><<<stride_grid((n_cap + 63) / 64), 256, 0, s>>>(src, ent, w);
    const uint32_t *sk, *sv;
    coalesce_sort(w, src.n_rows, capacity, out_ids, s, sk, sv);
    MF_DISPATCH_D(d, {
        constexpr int RPB = (64 / (D / 4)) * 4;
        auto levels = [&] {
            for (int64_t unit = 1;; unit *= RUN_CHUNK) {          // levels until one block covers every possible position
                const int64_t items = capacity + (n_cap + unit * RUN_CHUNK - 1) / (unit * RUN_CHUNK);
                coalesce_segsum_kernel<D, E><<<dim3((unsigned)((items + RPB - 1) / RPB)), 256, 0, s>>>(
                    sk, sv, w.n_dev, w.head_pos, w.tcount + w.ntiles, capacity, unit, src, w.euser, w.partial, out_ids, out_grad, ent);
                if (unit * RUN_CHUNK >= n_cap) break;
            }
        };
        if (segsum_span) MF_TIMED(segsum_span, s, levels());
        else levels();
    });
    return MF_OK;
}
