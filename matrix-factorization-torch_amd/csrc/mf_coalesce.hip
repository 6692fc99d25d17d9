// mf_coalesce.hip -- the parts of the list towers' coalesce (mf_coalesce.h) that do not depend on the tower: the entry
// checks, the LSD radix sort over the device-side entry count, the run heads and their output slots, and the -1 fill.
#include "mf_coalesce.h"

static constexpr int RADIX_TILE = 4096;          // sorted positions per workgroup (16 rounds of 256)
static constexpr int SCAN_THREADS = 1024;

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

// one 8-bit digit of the LSD radix sort over the first *n_dev keys: per-tile counts (zero past the end) ...
__global__ __launch_bounds__(256) void coalesce_radix_hist_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ n_dev,
                                                                  int shift, int ntiles, int32_t* __restrict__ hist) {
    __shared__ int cnt[256];
    const int64_t n = *n_dev;
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * RADIX_TILE;
    if (t0 < n) {
        for (int i = threadIdx.x; i < RADIX_TILE; i += 256) {
            const int64_t q = t0 + i;
            if (q < n) atomicAdd(&cnt[(keys[q] >> shift) & 255], 1);       // integer counts: order-free
        }
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];  // digit-major: the scan gives each (digit, tile) its base
}

// ... an exclusive scan (one workgroup; x[n] = total) ...
__global__ __launch_bounds__(SCAN_THREADS) void coalesce_scan_kernel(int32_t* __restrict__ x, int64_t n) {
    __shared__ int wsum[SCAN_THREADS / 64];
    constexpr int PER = 16;
    const int lane = mf_lane(), wave = threadIdx.x >> 6;
    int run = 0;
    for (int64_t base = 0; base < n; base += (int64_t)SCAN_THREADS * PER) {
        const int64_t q0 = base + (int64_t)threadIdx.x * PER;
        int v[PER];
        int sum = 0;
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            v[t] = q0 + t < n ? x[q0 + t] : 0;
            sum += v[t];
        }
        const int inc = wave_incl_scan(sum);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < SCAN_THREADS / 64; ++w) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        int at = run + before + inc - sum;
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            if (q0 + t < n) x[q0 + t] = at;
            at += v[t];
        }
        run += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) x[n] = run;
}

// ... and a stable scatter: 16 rounds of 256 positions; inside a wave the rank among equal digits comes from the ballots,
// across waves from a 4 x 256 count table
__global__ __launch_bounds__(256) void coalesce_radix_scatter_kernel(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                                     const int32_t* __restrict__ n_dev, int shift, int ntiles,
                                                                     const int32_t* __restrict__ hist, uint32_t* __restrict__ kout,
                                                                     uint32_t* __restrict__ vout) {
    __shared__ int base[256];
    __shared__ int wcnt[4][256];
    const int64_t n = *n_dev;
    const int64_t t0 = (int64_t)blockIdx.x * RADIX_TILE;
    if (t0 >= n) return;                                               // (block-uniform)
    const int tid = threadIdx.x, lane = mf_lane(), wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    base[tid] = hist[(int64_t)tid * ntiles + blockIdx.x];
    for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    for (int r = 0; r < RADIX_TILE / 256; ++r) {
        const int64_t q = t0 + r * 256 + tid;
        const bool valid = q < n;
        const uint32_t k = valid ? kin[q] : 0u;
        const unsigned dg = (k >> shift) & 255u;
        const unsigned long long peers = radix_peers(valid, dg);
        if (valid && (peers & below) == 0) wcnt[wave][dg] = __popcll(peers);
        __syncthreads();
        if (valid) {
            int pos = base[dg] + __popcll(peers & below);
            for (int w = 0; w < wave; ++w) pos += wcnt[w][dg];
            kout[pos] = k;
            vout[pos] = vin[q];
        }
        __syncthreads();
        base[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
        for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
        __syncthreads();
    }
}

// heads of the runs of valid keys: per-tile counts, then (after the scan) the head position of every output slot
template <bool SLOTS>
__global__ __launch_bounds__(256) void coalesce_heads_kernel(const uint32_t* __restrict__ sk, const int32_t* __restrict__ n_dev, uint32_t n_rows,
                                                             int32_t* __restrict__ tcount, int32_t* __restrict__ head_pos) {
    __shared__ int wcnt[4];
    const int64_t n = *n_dev;
    const int64_t t0 = (int64_t)blockIdx.x * RADIX_TILE;
    if (t0 >= n) {                                                     // (block-uniform) past the end: an empty tile
        if (!SLOTS && threadIdx.x == 0) tcount[blockIdx.x] = 0;
        return;
    }
    const int tid = threadIdx.x, lane = mf_lane(), wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int at = SLOTS ? tcount[blockIdx.x] : 0;
    for (int r = 0; r < RADIX_TILE / 256; ++r) {
        const int64_t q = t0 + r * 256 + tid;
        const bool head = q < n && sk[q] < n_rows && (q == 0 || sk[q - 1] != sk[q]);
        const unsigned long long m = __ballot(head);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; ++w) before += wcnt[w];
        if (SLOTS && head) head_pos[at + before + __popcll(m & below)] = (int32_t)q;
        at += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (!SLOTS && tid == 0) tcount[blockIdx.x] = at;
}

__global__ __launch_bounds__(256) void coalesce_fill_kernel(const int32_t* __restrict__ n_unique, int64_t capacity, int64_t* __restrict__ out_ids) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < capacity && s >= *n_unique) out_ids[s] = -1;
}

CoalesceWs coalesce_ws(MfArena& a, int64_t n_extra, int64_t n_entries, int d) {
    const int64_t n_cap = n_extra + n_entries > 0 ? n_extra + n_entries : 1;
    CoalesceWs w;
    w.ntiles = (int)((n_cap + RADIX_TILE - 1) / RADIX_TILE);
    w.n_dev = a.take<int32_t>(1);
    w.k0 = a.take<uint32_t>((size_t)n_cap);
    w.v0 = a.take<uint32_t>((size_t)n_cap);
    w.k1 = a.take<uint32_t>((size_t)n_cap);
    w.v1 = a.take<uint32_t>((size_t)n_cap);
    w.euser = a.take<int32_t>((size_t)n_entries);
    w.hist = a.take<int32_t>((size_t)256 * w.ntiles + 1);
    w.tcount = a.take<int32_t>((size_t)w.ntiles + 1);
    w.head_pos = a.take<int32_t>((size_t)n_cap);
    w.partial = a.take<float>((size_t)n_cap * d);
    return w;
}

size_t coalesce_ws_bytes(int64_t n_extra, int64_t n_entries, int d) {
    MfArena a(nullptr);
    coalesce_ws(a, n_extra > 0 ? n_extra : 0, n_entries > 0 ? n_entries : 0, d);
    return a.used();
}

int coalesce_check(const char* who, const char* rows, int64_t n_rows, int64_t n_extra, const int64_t* extra_ids, const float* extra_grad,
                   int64_t n_entries, int64_t capacity, const void* ws, size_t ws_bytes, size_t need_bytes) {
    if (!ws || n_rows <= 0 || n_entries < 0 || n_extra < 0 || (n_extra > 0 && (!extra_ids || !extra_grad)))
        return mf_set_error(MF_EINVAL, "%s: bad argument", who);
    if (n_rows > COALESCE_MAX_ROWS) return mf_set_error(MF_ENOTSUP, "%s: %lld %s rows > %d", who, (long long)n_rows, rows, COALESCE_MAX_ROWS);
    const int64_t n = n_extra + n_entries;
    if (n >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "%s: %lld entries >= 2^31", who, (long long)n);
    if (capacity != (n < n_rows ? n : n_rows)) return mf_set_error(MF_EINVAL, "%s: capacity must be min(n_rows, entries)", who);
    if (ws_bytes < need_bytes) return mf_set_error(MF_ENOSPC, "%s: workspace too small", who);
    return MF_OK;
}

void coalesce_sort(const CoalesceWs& w, int64_t n_rows, int64_t capacity, int64_t* out_ids, hipStream_t s,
                   const uint32_t*& sk, const uint32_t*& sv) {
    int bits = 1;
    while ((1ll << bits) <= n_rows) ++bits;                  // keys 0 .. n_rows
    const int passes = (bits + 7) / 8;
    const unsigned tiles = (unsigned)w.ntiles;
    uint32_t *ki = w.k0, *vi = w.v0, *ko = w.k1, *vo = w.v1;
    for (int ps = 0; ps < passes; ++ps) {
        coalesce_radix_hist_kernel<<<tiles, 256, 0, s>>>(ki, w.n_dev, 8 * ps, w.ntiles, w.hist);
        coalesce_scan_kernel<<<1, SCAN_THREADS, 0, s>>>(w.hist, (int64_t)256 * w.ntiles);
        coalesce_radix_scatter_kernel<<<tiles, 256, 0, s>>>(ki, vi, w.n_dev, 8 * ps, w.ntiles, w.hist, ko, vo);
        uint32_t* t = ki; ki = ko; ko = t;
        t = vi; vi = vo; vo = t;
    }
    coalesce_heads_kernel<false><<<tiles, 256, 0, s>>>(ki, w.n_dev, (uint32_t)n_rows, w.tcount, nullptr);
    coalesce_scan_kernel<<<1, SCAN_THREADS, 0, s>>>(w.tcount, w.ntiles);
    coalesce_heads_kernel<true><<<tiles, 256, 0, s>>>(ki, w.n_dev, (uint32_t)n_rows, w.tcount, w.head_pos);
    coalesce_fill_kernel<<<dim3((unsigned)((capacity + 255) / 256)), 256, 0, s>>>(w.tcount + w.ntiles, capacity, out_ids);
    sk = ki;
    sv = vi;
}
