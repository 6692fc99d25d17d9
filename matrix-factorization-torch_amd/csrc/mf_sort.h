// mf_sort.h -- device helpers shared by the pooled towers' backwards (mf_pool.hip: history tower, mf_bag.hip: feature-bag
// towers): the owner search over a CSR, a wave scan, the ballot multi-split of the LSD radix sort and the one-workgroup scan.
#pragma once
#include "mf_update.h"

static constexpr int RADIX_TILE = 4096;          // sorted positions per workgroup (16 rounds of 256)
static constexpr int SCAN_THREADS = 1024;

// last b in [0, B] with off[b] <= k  (off non-decreasing, off[0] = 0 <= k)
__device__ __forceinline__ int64_t pool_owner(const int64_t* __restrict__ off, int64_t B, int64_t k) {
    int64_t l = 0, r = B;
    while (r - l > 1) {
        const int64_t m = (l + r) >> 1;
        if (off[m] <= k) l = m;
        else r = m;
    }
    return l;
}

__device__ __forceinline__ int64_t wave_incl_scan(int64_t x) {
    const int lane = mf_lane();
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int64_t y = __shfl_up(x, s, 64);
        if (lane >= s) x += y;
    }
    return x;
}

// the lanes of this wave with my digit (8 ballots), among the `valid` lanes
__device__ __forceinline__ unsigned long long radix_peers(bool valid, unsigned dg) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const unsigned long long on = __ballot(valid && ((dg >> bit) & 1u));
        m &= ((dg >> bit) & 1u) ? on : ~on;
    }
    return m;
}

// exclusive scan of x[0, n) in place, x[n] = the total (one workgroup of scan_i32_kernel, mf_pool.hip)
void mf_scan_i32(int32_t* x, int64_t n, hipStream_t s);
