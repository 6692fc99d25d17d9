// mf_pool.hip -- the history-pooled user tower: u_b = normalize(pool_e r_e), r_e = the (normalised) item-table rows of user
// b's history, pool = mean or max, and its backward as ONE coalesced (id, gradient row) list for the sparse updates.
//
// Reference interface replaced: PoolingTransformer.forward(inputs_embeds) (xfmr_rec/models.py:81-84: pooling_mode "mean" /
// "max" over the non-zero rows, models.py:24, then Normalize, models.py:59) with the transformer taken out: the sequence is
// the item rows of the user's history (xfmr_rec/data/prepare.py:229-243, 285-299).  Spec: tests/test_history_tower_cpu.py.
//
// Lists.  User b's list is items[lo_b, hi_b), lo_b = clamp(start[b]), hi_b = clamp(end[b]) (a CSR, the rolling windows
// of InteractionTable or a padded [B, L] matrix all have this form).  Ids outside [1, n_rows) are padding.  max_history = L
// moves lo_b up to the first of the last L valid entries (pool_cut_kernel).
//
// Forward, deterministic and without atomics: the lists are cut into chunks of POOL_CHUNK entries (a 30,000-entry list is
// 469 chunks on as many waves); each wave sums (or maxes) its chunk in a fixed order; chunks are combined in chunk order,
// first 32 at a time (pool_super_kernel), then per user (pool_finish_kernel) -- the two levels of mf_update.h's RUN_CHUNK
// sum.  Max keeps the FIRST entry of a tie (strict comparisons in list order; the entry's offset breaks ties across chunks).
//
// Backward: every (entry, gradient row) of the batch -- the history entries, whose rows are w_b * g_p[b] (mean) or g_p[b]
// routed by the max's winners, plus any explicit rows parked on the same table in the same step (the item tower's) -- is
// sorted by item id with a stable LSD radix sort (8-bit digits, ballot multi-split inside a wave: linear, no atomics, no
// host round trip), and the runs of equal ids are summed in sorted order (= entry order) by a fixed tree of RUN_CHUNK.  The
// result is a list of exactly `capacity` = min(n_rows, entries) slots: the unique ids in ascending order with their summed
// rows, then id -1 (skipped by every update kernel).  The run sums form a fixed tree of fan-out 32 (pool_segsum_kernel).
#include "mf_sort.h"

static constexpr int POOL_CHUNK = 64;            // entries per chunk (one wave)
static constexpr int POOL_SUPER = 32;            // chunks per first-level combine
static constexpr int POOL_MAX_ROWS = 1 << 20;    // item-table rows the radix sort covers (keys <= 2^20: three 8-bit digits)

__device__ __forceinline__ bool pool_valid(long long id, long long n_rows) { return id >= 1 && id < n_rows; }

// ------------------------------------------------------------------------------------------- max_history ----
// One wave per user: walk back from hi 64 entries at a time until the L-th valid entry.
__global__ __launch_bounds__(256) void pool_cut_kernel(const int64_t* __restrict__ seg_start, const int64_t* __restrict__ seg_end,
                                                       const int64_t* __restrict__ items, int64_t n_items, int64_t B, int64_t n_rows,
                                                       int max_history, int64_t* __restrict__ lo_out) {
    const int lane = mf_lane();
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int64_t lo = min(max(seg_start[b], (int64_t)0), n_items);
    const int64_t hi = min(max(seg_end[b], lo), n_items);
    int64_t cut = lo;
    int need = max_history;
    for (int64_t top = hi; top > lo; top -= 64) {
        const int64_t pos = top - 1 - lane;                  // lane 0 = the most recent entry of this block
        const bool ok = pos >= lo && pool_valid(items[pos >= lo ? pos : lo], n_rows);
        unsigned long long m = __ballot(ok);
        const int c = __popcll(m);
        if (c >= need) {
            for (int i = 1; i < need; ++i) m &= m - 1;       // the need-th valid entry from the end
            cut = top - 1 - __builtin_ctzll(m);
            break;
        }
        need -= c;
    }
    if (lane == 0) lo_out[b] = cut;
}

// --------------------------------------------------------------------------------------------------- plan ----
// One workgroup: lo / hi of every user, and the exclusive prefixes of its chunks, first-level groups and entries.
static constexpr int PLAN_THREADS = 256;
// block-wide exclusive scan of three int64 per thread (PLAN_THREADS threads); returns the block totals in tot[3]
__device__ __forceinline__ void block_scan3(int64_t v[3], int64_t tot[3]) {
    __shared__ int64_t wsum[PLAN_THREADS / 64][3];
    const int lane = mf_lane(), wave = threadIdx.x >> 6;
    int64_t inc[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        inc[q] = wave_incl_scan(v[q]);
        if (lane == 63) wsum[wave][q] = inc[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        int64_t before = 0, all = 0;
        for (int w = 0; w < PLAN_THREADS / 64; ++w) {
            if (w < wave) before += wsum[w][q];
            all += wsum[w][q];
        }
        v[q] = before + inc[q] - v[q];
        tot[q] = all;
    }
    __syncthreads();
}

__global__ __launch_bounds__(PLAN_THREADS) void pool_plan_kernel(const int64_t* __restrict__ seg_start, const int64_t* __restrict__ seg_end,
                                                         const int64_t* __restrict__ cut, int64_t n_items, int64_t B,
                                                         int64_t* __restrict__ lo_out, int64_t* __restrict__ ent_off,
                                                         int64_t* __restrict__ chunk_off, int64_t* __restrict__ super_off) {
    int64_t run[3] = {0, 0, 0};
    for (int64_t b0 = 0; b0 < B; b0 += PLAN_THREADS) {
        const int64_t b = b0 + threadIdx.x;
        int64_t v[3] = {0, 0, 0};
        if (b < B) {
            const int64_t lo0 = min(max(seg_start[b], (int64_t)0), n_items);
            const int64_t hi = min(max(seg_end[b], lo0), n_items);
            const int64_t lo = cut ? min(max(cut[b], lo0), hi) : lo0;
            lo_out[b] = lo;
            const int64_t len = hi - lo, nch = (len + POOL_CHUNK - 1) / POOL_CHUNK;
            v[0] = len;
            v[1] = nch;
            v[2] = (nch + POOL_SUPER - 1) / POOL_SUPER;
        }
        int64_t tot[3];
        block_scan3(v, tot);
        if (b < B) {
            ent_off[b] = run[0] + v[0];
            chunk_off[b] = run[1] + v[1];
            super_off[b] = run[2] + v[2];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) run[q] += tot[q];
    }
    if (threadIdx.x == 0) {
        ent_off[B] = run[0];
        chunk_off[B] = run[1];
        super_off[B] = run[2];
    }
}

// ------------------------------------------------------------------------------------------------ chunks ----
// partial of one chunk / group: sum (mean) or per-channel max with the winning entry's offset in the user's list
template <int D, bool MAX>
struct PoolAcc {
    f32x4 v;
    int a[4];
    int n;
    __device__ __forceinline__ void init() {
        const float z = MAX ? -__builtin_huge_valf() : 0.f;
        v = f32x4{z, z, z, z};
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] = 0x7fffffff;
        n = 0;
    }
    // fold in a LATER partial (or entry): ties keep this one
    __device__ __forceinline__ void add(const f32x4& x, const int* xa, int xn) {
        if (MAX) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (x[t] > v[t] || (x[t] == v[t] && xa[t] < a[t])) { v[t] = x[t]; a[t] = xa[t]; }
        } else {
            v += x;
        }
        n += xn;
    }
};

// one wave per chunk (grid-stride over the device-side chunk count): lane group g (D/4 lanes) takes entries g, g + RPW, ...
// of the chunk in order; the groups are combined by a fixed butterfly
template <int D, bool MAX>
__global__ __launch_bounds__(256) void pool_chunk_kernel(const float* __restrict__ table, int64_t n_rows, const int64_t* __restrict__ items,
                                                         const int64_t* __restrict__ lo, const int64_t* __restrict__ ent_off,
                                                         const int64_t* __restrict__ chunk_off, int64_t B, int64_t cap_chunks, int norm_item,
                                                         float* __restrict__ psum, int32_t* __restrict__ parg, int32_t* __restrict__ pcnt) {
    constexpr int LPR = D / 4, RPW = 64 / LPR, PER = POOL_CHUNK / RPW, U = PER < 8 ? PER : 8;
    const int lane = mf_lane(), g = lane / LPR, c = lane % LPR;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int64_t total = min(chunk_off[B], cap_chunks);
    for (int64_t k = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); k < total; k += nwaves) {
        const int64_t b = pool_owner(chunk_off, B, k);
        const int64_t j0 = (k - chunk_off[b]) * POOL_CHUNK;            // offset of the chunk in the user's list
        const int64_t len = ent_off[b + 1] - ent_off[b];
        const int64_t base = lo[b];
        PoolAcc<D, MAX> acc;
        acc.init();
        for (int u0 = 0; u0 < PER; u0 += U) {
            long long id[U];
            bool ok[U];
#pragma unroll
            for (int t = 0; t < U; ++t) {
                const int64_t j = j0 + (int64_t)(u0 + t) * RPW + g;
                id[t] = j < len ? items[base + j] : 0;
                ok[t] = pool_valid(id[t], n_rows);
            }
            f32x4 x[U];
#pragma unroll
            for (int t = 0; t < U; ++t) x[t] = reinterpret_cast<const f32x4*>(table + (ok[t] ? id[t] : 0) * D)[c];
#pragma unroll
            for (int t = 0; t < U; ++t) {
                if (norm_item) {
                    const float ss = mf_group_sum(x[t][0] * x[t][0] + x[t][1] * x[t][1] + x[t][2] * x[t][2] + x[t][3] * x[t][3], LPR);
                    x[t] = x[t] * (1.f / fmaxf(sqrtf(ss), 1e-12f));
                }
                if (ok[t]) {
                    const int jj = (int)(j0 + (u0 + t) * RPW + g);
                    const int ja[4] = {jj, jj, jj, jj};
                    acc.add(x[t], ja, 1);
                }
            }
        }
        // groups in a fixed butterfly: group 0 ends up with all of them (a later group's ties lose: its offsets are larger)
#pragma unroll
        for (int s = LPR; s < 64; s <<= 1) {
            f32x4 o;
            int oa[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                o[t] = __shfl_xor(acc.v[t], s, 64);
                oa[t] = __shfl_xor(acc.a[t], s, 64);
            }
            const int on = __shfl_xor(acc.n, s, 64);
            if (MAX) {
                acc.add(o, oa, on);
            } else {                                                    // the lower group's value first: the same sum in both
                const bool low = (lane & s) == 0;
                f32x4 lo4 = low ? acc.v : o, hi4 = low ? o : acc.v;
                acc.v = lo4 + hi4;
                acc.n += on;
            }
        }
        if (g == 0) {
            reinterpret_cast<f32x4*>(psum + k * D)[c] = acc.v;
            if (MAX) reinterpret_cast<int4*>(parg + k * D)[c] = int4{acc.a[0], acc.a[1], acc.a[2], acc.a[3]};
            if (c == 0) pcnt[k] = acc.n;
        }
    }
}

// first level: chunks POOL_SUPER at a time, in chunk order (one row group per group of chunks)
template <int D, bool MAX>
__global__ __launch_bounds__(256) void pool_super_kernel(const int64_t* __restrict__ chunk_off, const int64_t* __restrict__ super_off,
                                                         int64_t B, int64_t cap_chunks, int64_t cap_supers, const float* __restrict__ psum,
                                                         const int32_t* __restrict__ parg, const int32_t* __restrict__ pcnt,
                                                         float* __restrict__ ssum, int32_t* __restrict__ sarg, int32_t* __restrict__ scnt) {
    constexpr int LPR = D / 4, RPW = 64 / LPR;
    const int lane = mf_lane(), c = lane % LPR;
    const int64_t ngroups = (int64_t)gridDim.x * (blockDim.x >> 6) * RPW;
    const int64_t total = min(super_off[B], cap_supers);
    for (int64_t s = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + lane / LPR; s < total; s += ngroups) {
        const int64_t b = pool_owner(super_off, B, s);
        const int64_t k0 = chunk_off[b] + (s - super_off[b]) * POOL_SUPER;
        const int64_t k1 = min(min(k0 + POOL_SUPER, chunk_off[b + 1]), cap_chunks);
        PoolAcc<D, MAX> acc;
        acc.init();
        for (int64_t k = k0; k < k1; ++k) {
            const f32x4 x = reinterpret_cast<const f32x4*>(psum + k * D)[c];
            int xa[4] = {0, 0, 0, 0};
            if (MAX) {
                const int4 q = reinterpret_cast<const int4*>(parg + k * D)[c];
                xa[0] = q.x; xa[1] = q.y; xa[2] = q.z; xa[3] = q.w;
            }
            acc.add(x, xa, pcnt[k]);
        }
        reinterpret_cast<f32x4*>(ssum + s * D)[c] = acc.v;
        if (MAX) reinterpret_cast<int4*>(sarg + s * D)[c] = int4{acc.a[0], acc.a[1], acc.a[2], acc.a[3]};
        if (c == 0) scnt[s] = acc.n;
    }
}

// second level, per user: p = mean / max, then u = p / max(|p|, 1e-12) (or p); an empty list gives p = u = 0
template <int D, bool MAX>
__global__ __launch_bounds__(256) void pool_finish_kernel(const int64_t* __restrict__ super_off, int64_t B, int64_t cap_supers,
                                                          const float* __restrict__ ssum, const int32_t* __restrict__ sarg,
                                                          const int32_t* __restrict__ scnt, int norm_user, float* __restrict__ out_u,
                                                          float* __restrict__ out_inv, int32_t* __restrict__ out_count,
                                                          int32_t* __restrict__ out_arg) {
    constexpr int LPR = D / 4, RPW = 64 / LPR;
    const int lane = mf_lane(), c = lane % LPR;
    const int64_t b = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + lane / LPR;
    const bool valid = b < B;
    PoolAcc<D, MAX> acc;
    acc.init();
    if (valid) {
        const int64_t s1 = min(super_off[b + 1], cap_supers);
        for (int64_t s = super_off[b]; s < s1; ++s) {
            const f32x4 x = reinterpret_cast<const f32x4*>(ssum + s * D)[c];
            int xa[4] = {0, 0, 0, 0};
            if (MAX) {
                const int4 q = reinterpret_cast<const int4*>(sarg + s * D)[c];
                xa[0] = q.x; xa[1] = q.y; xa[2] = q.z; xa[3] = q.w;
            }
            acc.add(x, xa, scnt[s]);
        }
    }
    f32x4 p = {0.f, 0.f, 0.f, 0.f};
    if (acc.n > 0) p = MAX ? acc.v : acc.v * (1.f / (float)acc.n);
    float inv = 1.f;
    if (norm_user) {
        const float ss = mf_group_sum(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3], LPR);
        inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
        p = p * inv;
    }
    if (valid) {
        reinterpret_cast<f32x4*>(out_u + b * D)[c] = p;
        if (MAX) reinterpret_cast<int4*>(out_arg + b * D)[c] = acc.n > 0 ? int4{acc.a[0], acc.a[1], acc.a[2], acc.a[3]} : int4{-1, -1, -1, -1};
        if (c == 0) {
            out_inv[b] = inv;
            out_count[b] = acc.n;
        }
    }
}

struct PoolWs {
    int64_t *cut, *chunk_off, *super_off;
    float *psum, *ssum;
    int32_t *parg, *pcnt, *sarg, *scnt;
    int64_t cap_chunks, cap_supers;
    size_t total;
};
static PoolWs pool_ws(void* ws, int64_t B, int64_t n_entries, int d, int mode) {
    MfArena a(ws);
    PoolWs w;
    w.cap_chunks = n_entries / POOL_CHUNK + B + 1;          // >= sum_b ceil(len_b / POOL_CHUNK)
    w.cap_supers = w.cap_chunks / POOL_SUPER + B + 1;
    const bool mx = mode == 1;
    w.cut = a.take<int64_t>((size_t)B);
    w.chunk_off = a.take<int64_t>((size_t)B + 1);
    w.super_off = a.take<int64_t>((size_t)B + 1);
    w.psum = a.take<float>((size_t)w.cap_chunks * d);
    w.parg = a.take<int32_t>(mx ? (size_t)w.cap_chunks * d : 0);
    w.pcnt = a.take<int32_t>((size_t)w.cap_chunks);
    w.ssum = a.take<float>((size_t)w.cap_supers * d);
    w.sarg = a.take<int32_t>(mx ? (size_t)w.cap_supers * d : 0);
    w.scnt = a.take<int32_t>((size_t)w.cap_supers);
    w.total = a.used();
    return w;
}

extern "C" size_t mf_pool_ws_bytes(int64_t B, int64_t n_entries, int d, int mode) {
    return pool_ws(nullptr, B > 0 ? B : 1, n_entries > 0 ? n_entries : 0, d, mode).total;
}

static int pool_grid(int64_t work_waves) {        // grid-stride kernels: enough waves to fill the chip, no more than the work
    const int64_t blocks = (work_waves + 3) / 4;
    return (int)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
}

extern "C" int mf_pool_forward(const float* table, int64_t n_rows, int d, const int64_t* seg_start, const int64_t* seg_end,
                               const int64_t* items, int64_t n_items, int64_t B, int64_t n_entries, int max_history, int mode,
                               int norm_item, int norm_user, float* out_u, float* out_inv, int32_t* out_count, int64_t* out_lo,
                               int64_t* out_off, int32_t* out_arg, void* ws, size_t ws_bytes, mf_stream_t stream) {
    if (!table || !seg_start || !seg_end || !items || !out_u || !out_inv || !out_count || !out_lo || !out_off || !ws || B <= 0 ||
        n_rows <= 0 || n_items <= 0 || n_entries < 0 || max_history < 0 || (mode != 0 && mode != 1) || (mode == 1 && !out_arg))
        return mf_set_error(MF_EINVAL, "mf_pool_forward: bad argument");
    if (n_rows > POOL_MAX_ROWS) return mf_set_error(MF_ENOTSUP, "mf_pool_forward: %lld table rows > %d", (long long)n_rows, POOL_MAX_ROWS);
    if (n_entries >= (1ll << 31) || B >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "mf_pool_forward: more than 2^31 entries or users");
    if (ws_bytes < mf_pool_ws_bytes(B, n_entries, d, mode)) return mf_set_error(MF_ENOSPC, "mf_pool_forward: workspace too small");
    PoolWs w = pool_ws(ws, B, n_entries, d, mode);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (max_history > 0)
        pool_cut_kernel<<<dim3((unsigned)((B + 3) / 4)), 256, 0, s>>>(seg_start, seg_end, items, n_items, B, n_rows, max_history, w.cut);
    pool_plan_kernel<<<dim3(1), PLAN_THREADS, 0, s>>>(seg_start, seg_end, max_history > 0 ? w.cut : nullptr, n_items, B, out_lo, out_off,
                                              w.chunk_off, w.super_off);
    const int gc = pool_grid(w.cap_chunks);
    MF_DISPATCH_D(d, {
        constexpr int RPB = (64 / (D / 4)) * 4;
        const int gs = pool_grid((w.cap_supers + RPB / 4 - 1) / (RPB / 4));
        const unsigned gf = (unsigned)((B + RPB - 1) / RPB);
        MF_TIMED("pool_forward", s, {
            if (mode == 1) {
                pool_chunk_kernel<D, true><<<gc, 256, 0, s>>>(table, n_rows, items, out_lo, out_off, w.chunk_off, B, w.cap_chunks, norm_item,
                                                              w.psum, w.parg, w.pcnt);
                pool_super_kernel<D, true><<<gs, 256, 0, s>>>(w.chunk_off, w.super_off, B, w.cap_chunks, w.cap_supers, w.psum, w.parg, w.pcnt, w.ssum,
                                                              w.sarg, w.scnt);
                pool_finish_kernel<D, true><<<gf, 256, 0, s>>>(w.super_off, B, w.cap_supers, w.ssum, w.sarg, w.scnt, norm_user, out_u,
                                                               out_inv, out_count, out_arg);
            } else {
                pool_chunk_kernel<D, false><<<gc, 256, 0, s>>>(table, n_rows, items, out_lo, out_off, w.chunk_off, B, w.cap_chunks,
                                                               norm_item, w.psum, nullptr, w.pcnt);
                pool_super_kernel<D, false><<<gs, 256, 0, s>>>(w.chunk_off, w.super_off, B, w.cap_chunks, w.cap_supers, w.psum, nullptr, w.pcnt, w.ssum,
                                                               nullptr, w.scnt);
                pool_finish_kernel<D, false><<<gf, 256, 0, s>>>(w.super_off, B, w.cap_supers, w.ssum, nullptr, w.scnt, norm_user, out_u,
                                                                out_inv, out_count, nullptr);
            }
        });
    });
    return mf_check_launch("mf_pool_forward");
}

// =========================================================================================== backward ====
// keys: entry q < n_extra is explicit row q (valid ids [0, n_rows)), entry n_extra + h is history entry h (valid ids
// [1, n_rows), h < ent_off[B]); invalid entries get key n_rows and sort last
__global__ __launch_bounds__(256) void pool_keys_kernel(const int64_t* __restrict__ extra_ids, int64_t n_extra, const int64_t* __restrict__ items,
                                                        const int64_t* __restrict__ lo, const int64_t* __restrict__ ent_off, int64_t B,
                                                        int64_t n_entries, int64_t n_rows, uint32_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals, int32_t* __restrict__ euser) {
    const int64_t n = n_extra + n_entries;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t total_h = min(ent_off[B], n_entries);
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += stride) {
        uint32_t key = (uint32_t)n_rows;
        if (q < n_extra) {
            const long long id = extra_ids[q];
            if (id >= 0 && id < n_rows) key = (uint32_t)id;
        } else {
            const int64_t h = q - n_extra;
            if (h < total_h) {
                const int64_t b = pool_owner(ent_off, B, h);
                const long long id = items[lo[b] + (h - ent_off[b])];
                if (pool_valid(id, n_rows)) key = (uint32_t)id;
                euser[h] = (int32_t)b;
            }
        }
        keys[q] = key;
        vals[q] = (uint32_t)q;
    }
}

// one 8-bit digit of the LSD radix sort: per-tile counts ...
__global__ __launch_bounds__(256) void radix_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int shift, int ntiles,
                                                         int32_t* __restrict__ hist) {
    __shared__ int cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * RADIX_TILE;
    for (int i = threadIdx.x; i < RADIX_TILE; i += 256) {
        const int64_t q = t0 + i;
        if (q < n) atomicAdd(&cnt[(keys[q] >> shift) & 255], 1);        // integer counts: order-free
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];  // digit-major: the scan gives each (digit, tile) its base
}

// ... an exclusive scan (one workgroup; x[n] = total) ...
__global__ __launch_bounds__(SCAN_THREADS) void scan_i32_kernel(int32_t* __restrict__ x, int64_t n) {
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
        int inc = sum;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int y = __shfl_up(inc, s, 64);
            if (lane >= s) inc += y;
        }
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

void mf_scan_i32(int32_t* x, int64_t n, hipStream_t s) { scan_i32_kernel<<<1, SCAN_THREADS, 0, s>>>(x, n); }

// ... and a stable scatter: 16 rounds of 256 positions; inside a wave the rank among equal digits comes from the ballots,
// across waves from a 4 x 256 count table
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin, int64_t n,
                                                            int shift, int ntiles, const int32_t* __restrict__ hist,
                                                            uint32_t* __restrict__ kout, uint32_t* __restrict__ vout) {
    __shared__ int base[256];
    __shared__ int wcnt[4][256];
    const int tid = threadIdx.x, lane = mf_lane(), wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    base[tid] = hist[(int64_t)tid * ntiles + blockIdx.x];
    for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * RADIX_TILE;
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
__global__ __launch_bounds__(256) void pool_heads_kernel(const uint32_t* __restrict__ sk, int64_t n, uint32_t n_rows,
                                                         int32_t* __restrict__ tcount, int32_t* __restrict__ head_pos) {
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = mf_lane(), wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int at = SLOTS ? tcount[blockIdx.x] : 0;
    const int64_t t0 = (int64_t)blockIdx.x * RADIX_TILE;
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

__global__ __launch_bounds__(256) void pool_fill_kernel(const int32_t* __restrict__ n_unique, int64_t capacity, int64_t* __restrict__ out_ids) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < capacity && s >= *n_unique) out_ids[s] = -1;
}

struct PoolGradSrc {
    const float* extra_grad;
    int64_t n_extra;
    const int32_t* euser;
    const int64_t* ent_off;
    const int32_t* count;
    const int32_t* arg;
    const float* grad_p;
    int mode;
};

// gradient row (lane c's 4 floats) of entry v
template <int D>
__device__ __forceinline__ f32x4 pool_entry_grad(const PoolGradSrc& src, uint32_t v, int c) {
    if ((int64_t)v < src.n_extra) return reinterpret_cast<const f32x4*>(src.extra_grad + (int64_t)v * D)[c];
    const int64_t h = (int64_t)v - src.n_extra;
    const int64_t b = src.euser[h];
    const f32x4 g = reinterpret_cast<const f32x4*>(src.grad_p + b * D)[c];
    if (src.mode == 0) return g * (1.f / (float)src.count[b]);
    const int j = (int)(h - src.ent_off[b]);
    const int4 a = reinterpret_cast<const int4*>(src.arg + b * D)[c];
    return f32x4{a.x == j ? g[0] : 0.f, a.y == j ? g[1] : 0.f, a.z == j ? g[2] : 0.f, a.w == j ? g[3] : 0.f};
}

// The runs' sums in sorted order, as a fixed tree of fan-out RUN_CHUNK over sorted positions, one launch per level, so that
// an item in a hundred thousand histories is summed by thousands of lane groups, not by one (update_rows_kernel's two
// levels would leave ~n / 32 partials to one group).  Level 1: the owner of every RUN_CHUNK-aligned unit of a run (its first
// position: the run's head or the unit's start) sums the unit's gradient rows in order.  Level L >= 2 (unit = 32^(L-1)
// positions, block = 32^L): the owner of the run's part of a block adds the level-(L-1) partials of its units, in order.
// A run that ends inside an owner's unit is written to its slot at that level; otherwise the sum is parked at the owner's
// position.  The tree depends on sorted positions only: deterministic.
template <int D>
__global__ __launch_bounds__(256) void pool_segsum_kernel(const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv, int64_t n,
                                                          uint32_t n_rows, const int32_t* __restrict__ head_pos,
                                                          const int32_t* __restrict__ n_unique, int64_t capacity, PoolGradSrc src,
                                                          int64_t unit, float* __restrict__ partial, int64_t* __restrict__ out_ids,
                                                          float* __restrict__ out_grad) {
    constexpr int LPR = D / 4, RPW = 64 / LPR;
    const int lane = mf_lane(), c = lane % LPR;
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
                if (t < m) g[t] = pool_entry_grad<D>(src, v8[t], c);
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

struct PoolBwdWs {
    uint32_t *k0, *v0, *k1, *v1;
    int32_t *euser, *hist, *tcount, *head_pos;
    float* partial;
    int ntiles;
    size_t total;
};
static PoolBwdWs pool_bwd_ws(void* ws, int64_t n, int64_t n_entries, int d) {
    MfArena a(ws);
    PoolBwdWs w;
    w.ntiles = (int)((n + RADIX_TILE - 1) / RADIX_TILE);
    w.k0 = a.take<uint32_t>((size_t)n);
    w.v0 = a.take<uint32_t>((size_t)n);
    w.k1 = a.take<uint32_t>((size_t)n);
    w.v1 = a.take<uint32_t>((size_t)n);
    w.euser = a.take<int32_t>((size_t)n_entries);
    w.hist = a.take<int32_t>((size_t)256 * w.ntiles + 1);
    w.tcount = a.take<int32_t>((size_t)w.ntiles + 1);
    w.head_pos = a.take<int32_t>((size_t)n);
    w.partial = a.take<float>((size_t)n * d);
    w.total = a.used();
    return w;
}

extern "C" size_t mf_pool_backward_ws_bytes(int64_t n_extra, int64_t n_entries, int d) {
    const int64_t n = (n_extra > 0 ? n_extra : 0) + (n_entries > 0 ? n_entries : 0);
    return pool_bwd_ws(nullptr, n > 0 ? n : 1, n_entries > 0 ? n_entries : 0, d).total;
}

extern "C" int mf_pool_backward(int64_t n_rows, int d, int mode, const int64_t* items, int64_t B, const int64_t* lo, const int64_t* ent_off,
                                const int32_t* count, const int32_t* arg, const float* grad_p, int64_t n_entries, const int64_t* extra_ids,
                                const float* extra_grad, int64_t n_extra, int64_t capacity, int64_t* out_ids, float* out_grad, void* ws,
                                size_t ws_bytes, mf_stream_t stream) {
    if (!items || !lo || !ent_off || !count || !grad_p || !out_ids || !out_grad || !ws || B <= 0 || n_rows <= 0 || n_entries < 0 ||
        n_extra < 0 || (n_extra > 0 && (!extra_ids || !extra_grad)) || (mode != 0 && mode != 1) || (mode == 1 && !arg))
        return mf_set_error(MF_EINVAL, "mf_pool_backward: bad argument");
    if (n_rows > POOL_MAX_ROWS) return mf_set_error(MF_ENOTSUP, "mf_pool_backward: %lld table rows > %d", (long long)n_rows, POOL_MAX_ROWS);
    const int64_t n = n_extra + n_entries;
    if (n >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "mf_pool_backward: %lld entries >= 2^31", (long long)n);
    if (capacity != (n < n_rows ? n : n_rows)) return mf_set_error(MF_EINVAL, "mf_pool_backward: capacity must be min(n_rows, entries)");
    if (!mf_width_ok(d)) return mf_set_error(MF_EINVAL, "mf_pool_backward: embedding width %d not in {32,64,128,256}", d);
    if (ws_bytes < mf_pool_backward_ws_bytes(n_extra, n_entries, d)) return mf_set_error(MF_ENOSPC, "mf_pool_backward: workspace too small");
    if (n == 0) return MF_OK;
    PoolBwdWs w = pool_bwd_ws(ws, n, n_entries, d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int bits = 1;
    while ((1ll << bits) <= n_rows) ++bits;                  // keys 0 .. n_rows
    const int passes = (bits + 7) / 8;
    const unsigned tiles = (unsigned)w.ntiles;
    MF_TIMED("pool_backward", s, {
        pool_keys_kernel<<<pool_grid((n + 63) / 64), 256, 0, s>>>(extra_ids, n_extra, items, lo, ent_off, B, n_entries, n_rows, w.k0, w.v0,
                                                                  w.euser);
        uint32_t *ki = w.k0, *vi = w.v0, *ko = w.k1, *vo = w.v1;
        for (int ps = 0; ps < passes; ++ps) {
            radix_hist_kernel<<<tiles, 256, 0, s>>>(ki, n, 8 * ps, w.ntiles, w.hist);
            scan_i32_kernel<<<1, SCAN_THREADS, 0, s>>>(w.hist, (int64_t)256 * w.ntiles);
            radix_scatter_kernel<<<tiles, 256, 0, s>>>(ki, vi, n, 8 * ps, w.ntiles, w.hist, ko, vo);
            uint32_t* t = ki; ki = ko; ko = t;
            t = vi; vi = vo; vo = t;
        }
        pool_heads_kernel<false><<<tiles, 256, 0, s>>>(ki, n, (uint32_t)n_rows, w.tcount, nullptr);
        scan_i32_kernel<<<1, SCAN_THREADS, 0, s>>>(w.tcount, w.ntiles);
        pool_heads_kernel<true><<<tiles, 256, 0, s>>>(ki, n, (uint32_t)n_rows, w.tcount, w.head_pos);
        pool_fill_kernel<<<dim3((unsigned)((capacity + 255) / 256)), 256, 0, s>>>(w.tcount + w.ntiles, capacity, out_ids);
        PoolGradSrc src{extra_grad, n_extra, w.euser, ent_off, count, arg, grad_p, mode};
        MF_DISPATCH_D(d, {
            constexpr int RPB = (64 / (D / 4)) * 4;
            MF_TIMED("pool_segsum", s, {
                for (int64_t unit = 1;; unit *= RUN_CHUNK) {          // levels until one block covers every position
                    const int64_t items = capacity + (n + unit * RUN_CHUNK - 1) / (unit * RUN_CHUNK);
                    pool_segsum_kernel<D><<<dim3((unsigned)((items + RPB - 1) / RPB)), 256, 0, s>>>(
                        ki, vi, n, (uint32_t)n_rows, w.head_pos, w.tcount + w.ntiles, capacity, src, unit, w.partial, out_ids, out_grad);
                    if (unit * RUN_CHUNK >= n) break;
                }
            });
        });
    });
    return mf_check_launch("mf_pool_backward");
}
