// mf_pool.hip -- the history-pooled user tower: u_b = normalize(pool_e r_e), r_e = the (normalised) item-table rows of user
// b's history, pool = mean or max, and its backward as ONE coalesced (id, gradient row) list for the sparse updates.
//
// Reference interface replaced: PoolingTransformer.forward(inputs_embeds) (xfmr_rec/models.py:81-84: pooling_mode "mean" /
// "max" over the non-zero rows, models.py:24, then Normalize, models.py:59) with the transformer taken out: the sequence is
// the item rows of the user's history (xfmr_rec/data/prepare.py:229-243, 285-299).  Spec: tests/test_history_tower_cpu.py.
//
// Lists.  User b's list is items[lo_b, hi_b), lo_b = clamp(start[b]), hi_b = clamp(end[b]) (a CSR, the rolling windows
// of InteractionTable or a padded [B, L] matrix all have this form).  Ids outside [1, n_rows) are padding.  max_history = L
// moves lo_b up to the first of the last L valid entries (list_cut_kernel, mf_lists.h).
//
// Forward, deterministic and without atomics: the lists are cut into chunks of POOL_CHUNK entries (a 30,000-entry list is
// 469 chunks on as many waves); each wave sums (or maxes) its chunk in a fixed order; chunks are combined in chunk order,
// first 32 at a time (pool_super_kernel), then per user (pool_finish_kernel) -- the two levels of mf_update.h's RUN_CHUNK
// sum.  Max keeps the FIRST entry of a tie (strict comparisons in list order; the entry's offset breaks ties across chunks).
//
// Backward: every (entry, gradient row) of the batch -- the history entries, whose rows are w_b * g_p[b] (mean) or g_p[b]
// routed by the max's winners, plus any explicit rows parked on the same table in the same step (the item tower's) -- is
// coalesced into one list of exactly `capacity` = min(n_rows, entries) slots by the engine of mf_coalesce.h: the unique
// ids in ascending order with their summed rows, then id -1 (skipped by every update kernel).
#include "mf_coalesce.h"

static constexpr int POOL_CHUNK = 64;            // entries per chunk (one wave)
static constexpr int POOL_SUPER = 32;            // chunks per first-level combine

// --------------------------------------------------------------------------------------------------- plan ----
// One workgroup: lo / hi of every user, and the exclusive prefixes of its chunks, first-level groups and entries.
static constexpr int PLAN_THREADS = 256;
__global__ __launch_bounds__(PLAN_THREADS) void pool_plan_kernel(const int64_t* __restrict__ seg_start, const int64_t* __restrict__ seg_end,
                                                         const int64_t* __restrict__ cut, int64_t n_items, int64_t B,
                                                         int64_t* __restrict__ lo_out, int64_t* __restrict__ ent_off,
                                                         int64_t* __restrict__ chunk_off, int64_t* __restrict__ super_off) {
    int64_t run[3] = {0, 0, 0};
    for (int64_t b0 = 0; b0 < B; b0 += PLAN_THREADS) {
        const int64_t b = b0 + threadIdx.x;
        int64_t v[3] = {0, 0, 0};
        if (b < B) {
            int64_t lo0, hi;
            list_clamp(seg_start[b], seg_end[b], n_items, lo0, hi);
            const int64_t lo = cut ? min(max(cut[b], lo0), hi) : lo0;
            lo_out[b] = lo;
            const int64_t len = hi - lo, nch = (len + POOL_CHUNK - 1) / POOL_CHUNK;
            v[0] = len;
            v[1] = nch;
            v[2] = (nch + POOL_SUPER - 1) / POOL_SUPER;
        }
        int64_t tot[3];
        block_excl_scan<PLAN_THREADS>(v, tot);
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
        const int64_t b = list_owner(chunk_off, B, k);
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
                ok[t] = list_valid(id[t], n_rows);
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
        if (MAX) {
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
                acc.add(o, oa, on);
            }
        } else {
            acc.v = group_butterfly_sum<D>(acc.v);
            acc.n = group_butterfly_sum<D>(acc.n);
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
        const int64_t b = list_owner(super_off, B, s);
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
    float inv;
    p = row_normalize<D>(p, norm_user, inv);
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

extern "C" int mf_pool_forward(const float* table, int64_t n_rows, int d, const int64_t* seg_start, const int64_t* seg_end,
                               const int64_t* items, int64_t n_items, int64_t B, int64_t n_entries, int max_history, int mode,
                               int norm_item, int norm_user, float* out_u, float* out_inv, int32_t* out_count, int64_t* out_lo,
                               int64_t* out_off, int32_t* out_arg, void* ws, size_t ws_bytes, mf_stream_t stream) {
    if (!table || !seg_start || !seg_end || !items || !out_u || !out_inv || !out_count || !out_lo || !out_off || !ws || B <= 0 ||
        n_rows <= 0 || n_items <= 0 || n_entries < 0 || max_history < 0 || (mode != 0 && mode != 1) || (mode == 1 && !out_arg))
        return mf_set_error(MF_EINVAL, "mf_pool_forward: bad argument");
    if (n_rows > COALESCE_MAX_ROWS) return mf_set_error(MF_ENOTSUP, "mf_pool_forward: %lld table rows > %d", (long long)n_rows, COALESCE_MAX_ROWS);
    if (n_entries >= (1ll << 31) || B >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "mf_pool_forward: more than 2^31 entries or users");
    if (ws_bytes < mf_pool_ws_bytes(B, n_entries, d, mode)) return mf_set_error(MF_ENOSPC, "mf_pool_forward: workspace too small");
    PoolWs w = pool_ws(ws, B, n_entries, d, mode);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (max_history > 0)
        list_cut_kernel<false><<<dim3((unsigned)((B + 3) / 4)), 256, 0, s>>>(seg_start, seg_end, items, n_items, B, n_rows, max_history, w.cut, nullptr);
    pool_plan_kernel<<<dim3(1), PLAN_THREADS, 0, s>>>(seg_start, seg_end, max_history > 0 ? w.cut : nullptr, n_items, B, out_lo, out_off,
                                              w.chunk_off, w.super_off);
    const int gc = stride_grid(w.cap_chunks);
    MF_DISPATCH_D(d, {
        constexpr int RPB = (64 / (D / 4)) * 4;
        const int gs = stride_grid((w.cap_supers + RPB / 4 - 1) / (RPB / 4));
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
// history entries: valid ids [1, n_rows); entry h of user b carries g_p[b] / count[b] (mean) or, on the channels it won,
// g_p[b] (max)
struct PoolEntries {
    const int64_t* items;
    int64_t n_rows;
    const int64_t* ent_off;
    const int32_t* count;
    const int32_t* arg;
    const float* grad_p;
    int mode;
    __device__ __forceinline__ uint32_t key(int64_t, int64_t pos) const {
        const long long id = items[pos];
        return list_valid(id, n_rows) ? (uint32_t)id : (uint32_t)n_rows;
    }
    template <int D>
    __device__ __forceinline__ f32x4 grad(int64_t b, int64_t h, int c) const {
        const f32x4 g = reinterpret_cast<const f32x4*>(grad_p + b * D)[c];
        if (mode == 0) return g * (1.f / (float)count[b]);
        const int j = (int)(h - ent_off[b]);
        const int4 a = reinterpret_cast<const int4*>(arg + b * D)[c];
        return f32x4{a.x == j ? g[0] : 0.f, a.y == j ? g[1] : 0.f, a.z == j ? g[2] : 0.f, a.w == j ? g[3] : 0.f};
    }
};

extern "C" size_t mf_pool_backward_ws_bytes(int64_t n_extra, int64_t n_entries, int d) {
    return coalesce_ws_bytes(n_extra, n_entries, d);
}

extern "C" int mf_pool_backward(int64_t n_rows, int d, int mode, const int64_t* items, int64_t B, const int64_t* lo, const int64_t* ent_off,
                                const int32_t* count, const int32_t* arg, const float* grad_p, int64_t n_entries, const int64_t* extra_ids,
                                const float* extra_grad, int64_t n_extra, int64_t capacity, int64_t* out_ids, float* out_grad, void* ws,
                                size_t ws_bytes, mf_stream_t stream) {
    if (!items || !lo || !ent_off || !count || !grad_p || !out_ids || !out_grad || B <= 0 || (mode != 0 && mode != 1) || (mode == 1 && !arg))
        return mf_set_error(MF_EINVAL, "mf_pool_backward: bad argument");
    if (!mf_width_ok(d)) return mf_set_error(MF_EINVAL, "mf_pool_backward: embedding width %d not in {32,64,128,256}", d);
    if (int rc = coalesce_check("mf_pool_backward", "table", n_rows, n_extra, extra_ids, extra_grad, n_entries, capacity, ws, ws_bytes,
                                coalesce_ws_bytes(n_extra, n_entries, d)))
        return rc;
    if (n_extra + n_entries == 0) return MF_OK;
    MfArena a(ws);
    const CoalesceWs w = coalesce_ws(a, n_extra, n_entries, d);
    const CoalesceSrc src{n_rows, extra_ids, extra_grad, n_extra, lo, ent_off, B, n_entries};
    const PoolEntries ent{items, n_rows, ent_off, count, arg, grad_p, mode};
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    MF_TIMED("pool_backward", s, rc = coalesce(src, ent, w, d, capacity, out_ids, out_grad, "pool_segsum", s));
    return rc ? rc : mf_check_launch("mf_pool_backward");
}
