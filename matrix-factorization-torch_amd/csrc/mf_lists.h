// mf_lists.h -- what the list towers (mf_pool.hip: history, mf_bag.hip: feature bags, mf_xfmr.hip: transformer) and their
// coalesce (mf_coalesce.h) share: which ids count, where owner b's list lies, the cut to its last L valid entries and the walk
// that packs them, the owner of a numbered work item, a block-wide exclusive scan, the lane groups' butterfly sum and the final row normalisation.
// Everything here is integer arithmetic or one float expression in one fixed order: a caller's results do not depend on
// which tower it is.
#pragma once
#include "mf_common.h"

// grid-stride kernels: enough waves to fill the chip, no more than the work
static inline int stride_grid(int64_t work_waves) {
    const int64_t blocks = (work_waves + 3) / 4;
    return (int)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
}

// ids outside [1, n_rows) are padding
__device__ __forceinline__ bool list_valid(long long id, long long n_rows) { return id >= 1 && id < n_rows; }

// owner b's list is items[lo, hi): start and end clamped to [0, n_items], never negative in length
__device__ __forceinline__ void list_clamp(int64_t start, int64_t end, int64_t n_items, int64_t& lo, int64_t& hi) {
    lo = min(max(start, (int64_t)0), n_items);
    hi = min(max(end, lo), n_items);
}

// last b in [0, B] with off[b] <= k  (off non-decreasing, off[0] = 0 <= k)
__device__ __forceinline__ int64_t list_owner(const int64_t* __restrict__ off, int64_t B, int64_t k) {
    int64_t l = 0, r = B;
    while (r - l > 1) {
        const int64_t m = (l + r) >> 1;
        if (off[m] <= k) l = m;
        else r = m;
    }
    return l;
}

// One wave, the list items[lo, hi): walk back from hi, 64 entries at a time, until the L-th valid entry; returns its position
// (lo when the list has fewer) and leaves need = L - min(valid entries, L).  Every lane gets both.
__device__ __forceinline__ int64_t list_cut_walk(const int64_t* __restrict__ items, int64_t lo, int64_t hi, int64_t n_rows, int L,
                                                 int& need) {
    const int lane = mf_lane();
    int64_t cut = lo;
    need = L;
    for (int64_t top = hi; top > lo; top -= 64) {
        const int64_t pos = top - 1 - lane;                  // lane 0 = the most recent entry of this block
        const bool ok = pos >= lo && list_valid(items[pos >= lo ? pos : lo], n_rows);
        unsigned long long m = __ballot(ok);
        const int c = __popcll(m);
        if (c >= need) {
            for (int i = 1; i < need; ++i) m &= m - 1;       // the need-th valid entry from the end
            cut = top - 1 - __builtin_ctzll(m);
            need = 0;
            break;
        }
        need -= c;
    }
    return cut;
}

// One wave, the list items[lo, hi): its valid entries in list order, the first `count` of them; entry number slot (0 ..) goes
// to emit(slot, id) on the lane that read it.  After list_cut_walk: lo = the cut, count = L - need.
template <class F>
__device__ __forceinline__ void list_pack_walk(const int64_t* __restrict__ items, int64_t lo, int64_t hi, int64_t n_rows, int count,
                                               F emit) {
    const int lane = mf_lane();
    int done = 0;
    for (int64_t base = lo; base < hi && done < count; base += 64) {
        const int64_t pos = base + lane;
        const long long id = pos < hi ? items[pos] : 0;
        const bool ok = list_valid(id, n_rows);
        const unsigned long long m = __ballot(ok);
        const int slot = done + __popcll(m & ((1ull << lane) - 1ull));
        if (ok && slot < count) emit(slot, id);
        done += __popcll(m);
    }
}

// One wave per owner: cut_out[b] = list_cut_walk's position, and with COUNT also nb_out[b] = min(valid entries, L).
template <bool COUNT>
__global__ __launch_bounds__(256) void list_cut_kernel(const int64_t* __restrict__ seg_start, const int64_t* __restrict__ seg_end,
                                                       const int64_t* __restrict__ items, int64_t n_items, int64_t B, int64_t n_rows,
                                                       int L, int64_t* __restrict__ cut_out, int32_t* __restrict__ nb_out) {
    const int lane = mf_lane();
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    int64_t lo, hi;
    list_clamp(seg_start[b], seg_end[b], n_items, lo, hi);
    int need;
    const int64_t cut = list_cut_walk(items, lo, hi, n_rows, L, need);
    if (lane == 0) {
        cut_out[b] = cut;
        if (COUNT) nb_out[b] = L - need;
    }
}

template <class T>
__device__ __forceinline__ T wave_incl_scan(T x) {
    const int lane = mf_lane();
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const T y = __shfl_up(x, s, 64);
        if (lane >= s) x += y;
    }
    return x;
}

// Exclusive scan of Q values per thread over the THREADS threads of a workgroup (every thread calls it): v[q] becomes the
// sum of the earlier threads' v[q], tot[q] the workgroup's.  Two barriers, so it may be called in a loop.
template <int THREADS, int Q>
__device__ __forceinline__ void block_excl_scan(int64_t (&v)[Q], int64_t (&tot)[Q]) {
    __shared__ int64_t wsum[THREADS / 64][Q];
    const int lane = mf_lane(), wave = threadIdx.x >> 6;
    int64_t inc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        inc[q] = wave_incl_scan(v[q]);
        if (lane == 63) wsum[wave][q] = inc[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        int64_t before = 0, all = 0;
        for (int w = 0; w < THREADS / 64; ++w) {
            if (w < wave) before += wsum[w][q];
            all += wsum[w][q];
        }
        v[q] = before + inc[q] - v[q];
        tot[q] = all;
    }
    __syncthreads();
}

// Sum over the lane groups (D / 4 lanes each) of a wave by a fixed butterfly, the lower group's value first: every lane
// ends with the same sum.  A scalar (a count, a weight sum), or lane c's four floats of a row.
template <int D, class T>
__device__ __forceinline__ T group_butterfly_sum(T x) {
#pragma unroll
    for (int s = D / 4; s < 64; s <<= 1) {
        const T o = __shfl_xor(x, s, 64);
        x = (mf_lane() & s) == 0 ? x + o : o + x;
    }
    return x;
}
template <int D>
__device__ __forceinline__ f32x4 group_butterfly_sum(f32x4 x) {
#pragma unroll
    for (int s = D / 4; s < 64; s <<= 1) {
        f32x4 o;
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = __shfl_xor(x[t], s, 64);
        x = (mf_lane() & s) == 0 ? x + o : o + x;
    }
    return x;
}

// a tower's last step on a row held by a lane group (lane c: four floats): inv = 1 / max(|p|, 1e-12) (1 unless do_norm);
// returns p * inv.  Every lane of the group calls it.
template <int D>
__device__ __forceinline__ f32x4 row_normalize(f32x4 p, int do_norm, float& inv) {
    inv = 1.f;
    if (do_norm) {
        const float ss = mf_group_sum(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3], D / 4);
        inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
        p = p * inv;
    }
    return p;
}
