// mf_bag.hip -- hashed feature-bag towers: u_b = normalize(c_b * sum_e w_e F[t_e]) over the (token, weight) bag of entity
// idx[b], and the backward as ONE coalesced (id, gradient row) list for the sparse updates.
//
// Reference interface replaced: the shared text encoder of xfmr_rec/lightning.py:60-74 over the JSON of an item's
// {"title", "genres"} / a user's {"gender", "age", "occupation", "zipcode"} (xfmr_rec/data/prepare.py:69-127).  Here the
// attributes are hashed into tokens on the host (data.FeatureHasher) and each token is a row of one bucket table F [R, d]:
// the classic EmbeddingBag tower.  Spec: tests/test_feature_tower_cpu.py.
//
// Bags.  Entity e's bag is tokens[start[e], end[e]) (clamped to [0, n_tokens), cut to max_len) with weights[...] (or 1); a
// registered CSR passes start = off, end = off + 1.  Bag b of a call is entity idx[b] (idx null: b itself); an entity id
// outside [0, n_seg) is an empty bag.  Tokens outside [1, R) are padding: dropped from the sum, the weight sums and the counts.
// s_b = sum w_e F[t_e]; c_b = 1 (sum), 1 / sum w_e (mean), 1 / sqrt(sum w_e^2) (sqrtn), 0 when sum w_e = 0; p_b = c_b s_b;
// u_b = normalize ? p_b / max(|p_b|, 1e-12) : p_b.
//
// Nothing is read back on the host: max_len (fixed when the bags are registered) sizes every buffer and grid, the kernels
// exit early past the real work, and the backward's entry count stays on the device.
//
// Forward.  max_len <= BAG_SHORT: one lane group (d/4 lanes, 16-byte loads in the gather_rows layout) per bag sums the bag
// in entry order -- no plan, no partials.  Longer bags: one wave per BAG_CHUNK entries of a bag (bag b's chunk j is work
// item b * C + j, C = ceil(max_len / BAG_CHUNK)), lane groups in a fixed butterfly, then one group per bag adds its chunks
// in order.  Either way the summation order depends on the bag lengths only.
//
// Backward.  Entry e of bag b carries w_e * c_b * g_p[b]; entries with w_e = 0 or c_b = 0 carry nothing and are dropped like
// padding.  A plan kernel numbers the bags' entries; the engine of mf_coalesce.h coalesces them after the extras, applying
// the weight at the leaf.  The result is exactly `capacity` = min(R, n_extra + B * max_len) slots: unique ids ascending,
// then -1.  The only atomics are the integer LDS histogram counts.
#include "mf_coalesce.h"

static constexpr int BAG_SHORT = 64;             // longest bag of the one-group-per-bag path
static constexpr int BAG_CHUNK = 64;             // entries per wave on the chunked path
static constexpr int BAG_PLAN_THREADS = 1024;

struct BagSrc {                                  // the bags of one call
    const int64_t* idx;                          // [B] entity ids, or null (bag b = entity b)
    const int64_t* start;                        // [n_seg]
    const int64_t* end;                          // [n_seg]
    int64_t n_seg;
    const int64_t* tokens;
    int64_t n_tokens;
    const float* weights;                        // [n_tokens] or null (1)
    int64_t max_len;
    int64_t R;
};

// first position and length of bag b
__device__ __forceinline__ void bag_span(const BagSrc& s, int64_t b, int64_t& lo, int64_t& len) {
    const int64_t e = s.idx ? s.idx[b] : b;
    lo = 0;
    len = 0;
    if (e < 0 || e >= s.n_seg) return;
    int64_t hi;
    list_clamp(s.start[e], s.end[e], s.n_tokens, lo, hi);
    len = min(hi - lo, s.max_len);
}

// weight of the entry at position pos (0 for padding tokens)
__device__ __forceinline__ float bag_weight(const BagSrc& s, int64_t pos, long long tok) {
    if (!list_valid(tok, s.R)) return 0.f;
    return s.weights ? s.weights[pos] : 1.f;
}

__device__ __forceinline__ float bag_scale(int combiner, float wsum, float w2sum) {
    if (!(wsum > 0.f)) return 0.f;
    return combiner == 0 ? 1.f : (combiner == 1 ? 1.f / wsum : 1.f / sqrtf(w2sum));
}

// p = scale * s, then the tower's normalisation; every lane of the wave calls this
template <int D>
__device__ __forceinline__ void bag_finish(f32x4 acc, float wsum, float w2sum, int combiner, int normalize, bool valid, int64_t b,
                                           int c, float* __restrict__ out_u, float* __restrict__ out_inv, float* __restrict__ out_scale) {
    const float scale = bag_scale(combiner, wsum, w2sum);
    f32x4 p = acc * scale;
    if (scale == 0.f) p = f32x4{0.f, 0.f, 0.f, 0.f};
    float inv;
    p = row_normalize<D>(p, normalize, inv);
    if (valid) {
        reinterpret_cast<f32x4*>(out_u + b * D)[c] = p;
        if (c == 0) {
            out_inv[b] = inv;
            out_scale[b] = scale;
        }
    }
}

// ---------------------------------------------------------------------------------------------- forward ----
// short bags: lane group (D/4 lanes) = one bag, entries in order, four row loads in flight
template <int D>
__global__ __launch_bounds__(256) void bag_short_kernel(const float* __restrict__ table, BagSrc src, int64_t B, int combiner, int normalize,
                                                        float* __restrict__ out_u, float* __restrict__ out_inv, float* __restrict__ out_scale) {
    constexpr int LPR = D / 4, RPW = 64 / LPR, U = 4;
    const int lane = mf_lane(), c = lane % LPR;
    const int64_t b = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + lane / LPR;
    const bool valid = b < B;
    int64_t lo = 0, len = 0;
    if (valid) bag_span(src, b, lo, len);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float wsum = 0.f, w2sum = 0.f;
    for (int64_t j0 = 0; j0 < len; j0 += U) {
        long long tok[U];
        float w[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int64_t j = j0 + t;
            tok[t] = j < len ? src.tokens[lo + j] : 0;
            w[t] = j < len ? bag_weight(src, lo + j, tok[t]) : 0.f;
        }
        f32x4 x[U];
#pragma unroll
        for (int t = 0; t < U; ++t) x[t] = reinterpret_cast<const f32x4*>(table + (w[t] != 0.f ? tok[t] : 0) * D)[c];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            if (w[t] != 0.f) {
                acc += x[t] * w[t];
                wsum += w[t];
                w2sum += w[t] * w[t];
            }
        }
    }
    bag_finish<D>(acc, wsum, w2sum, combiner, normalize, valid, b, c, out_u, out_inv, out_scale);
}

// long bags, first level: one wave per chunk of BAG_CHUNK entries (grid-stride over B * C work items)
template <int D>
__global__ __launch_bounds__(256) void bag_chunk_kernel(const float* __restrict__ table, BagSrc src, int64_t B, int64_t C,
                                                        float* __restrict__ psum, float* __restrict__ pw) {
    constexpr int LPR = D / 4, RPW = 64 / LPR, PER = BAG_CHUNK / RPW, U = PER < 4 ? PER : 4;
    const int lane = mf_lane(), g = lane / LPR, c = lane % LPR;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t k = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); k < B * C; k += nwaves) {
        const int64_t b = k / C, j0 = (k % C) * BAG_CHUNK;
        int64_t lo, len;
        bag_span(src, b, lo, len);
        if (j0 >= len) continue;                                       // (wave-uniform)
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float wsum = 0.f, w2sum = 0.f;
        for (int u0 = 0; u0 < PER; u0 += U) {
            long long tok[U];
            float w[U];
#pragma unroll
            for (int t = 0; t < U; ++t) {
                const int64_t j = j0 + (int64_t)(u0 + t) * RPW + g;
                tok[t] = j < len ? src.tokens[lo + j] : 0;
                w[t] = j < len ? bag_weight(src, lo + j, tok[t]) : 0.f;
            }
            f32x4 x[U];
#pragma unroll
            for (int t = 0; t < U; ++t) x[t] = reinterpret_cast<const f32x4*>(table + (w[t] != 0.f ? tok[t] : 0) * D)[c];
#pragma unroll
            for (int t = 0; t < U; ++t) {
                if (w[t] != 0.f) {
                    acc += x[t] * w[t];
                    wsum += w[t];
                    w2sum += w[t] * w[t];
                }
            }
        }
        // groups in a fixed butterfly, the lower group's value first: every lane ends with the same sums
        acc = group_butterfly_sum<D>(acc);
        wsum = group_butterfly_sum<D>(wsum);
        w2sum = group_butterfly_sum<D>(w2sum);
        if (g == 0) {
            reinterpret_cast<f32x4*>(psum + k * D)[c] = acc;
            if (c == 0) {
                pw[2 * k] = wsum;
                pw[2 * k + 1] = w2sum;
            }
        }
    }
}

// long bags, second level: one lane group per bag adds its chunks in chunk order
template <int D>
__global__ __launch_bounds__(256) void bag_combine_kernel(BagSrc src, int64_t B, int64_t C, const float* __restrict__ psum,
                                                          const float* __restrict__ pw, int combiner, int normalize,
                                                          float* __restrict__ out_u, float* __restrict__ out_inv, float* __restrict__ out_scale) {
    constexpr int LPR = D / 4, RPW = 64 / LPR;
    const int lane = mf_lane(), c = lane % LPR;
    const int64_t b = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + lane / LPR;
    const bool valid = b < B;
    int64_t lo = 0, len = 0;
    if (valid) bag_span(src, b, lo, len);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float wsum = 0.f, w2sum = 0.f;
    const int64_t nch = (len + BAG_CHUNK - 1) / BAG_CHUNK;
    for (int64_t j = 0; j < nch; ++j) {
        const int64_t k = b * C + j;
        acc += reinterpret_cast<const f32x4*>(psum + k * D)[c];
        wsum += pw[2 * k];
        w2sum += pw[2 * k + 1];
    }
    bag_finish<D>(acc, wsum, w2sum, combiner, normalize, valid, b, c, out_u, out_inv, out_scale);
}

static int64_t bag_chunks(int64_t max_len) { return max_len <= BAG_SHORT ? 0 : (max_len + BAG_CHUNK - 1) / BAG_CHUNK; }

extern "C" size_t mf_bag_ws_bytes(int64_t B, int64_t max_len, int d) {
    MfArena a(nullptr);
    const int64_t C = bag_chunks(max_len);
    a.take<float>((size_t)(B > 0 ? B : 0) * C * d);
    a.take<float>((size_t)(B > 0 ? B : 0) * C * 2);
    return a.used();
}

static int bag_check(const char* who, int64_t n_rows, int d, int64_t B, const int64_t* start, const int64_t* end, int64_t n_seg,
                     const int64_t* tokens, int64_t n_tokens, int64_t max_len) {
    if (!start || !end || !tokens || B <= 0 || n_rows <= 0 || n_seg < 0 || n_tokens <= 0 || max_len < 0)
        return mf_set_error(MF_EINVAL, "%s: bad argument", who);
    if (!mf_width_ok(d)) return mf_set_error(MF_EINVAL, "%s: embedding width %d not in {32,64,128,256}", who, d);
    if (n_rows > COALESCE_MAX_ROWS) return mf_set_error(MF_ENOTSUP, "%s: %lld feature-table rows > %d", who, (long long)n_rows, COALESCE_MAX_ROWS);
    if (max_len > 0 && B >= ((1ll << 31) - 1) / max_len) return mf_set_error(MF_ENOTSUP, "%s: B * max_len >= 2^31", who);
    return MF_OK;
}

extern "C" int mf_bag_forward(const float* table, int64_t n_rows, int d, const int64_t* idx, int64_t B, const int64_t* seg_start,
                              const int64_t* seg_end, int64_t n_seg, const int64_t* tokens, int64_t n_tokens, const float* weights,
                              int64_t max_len, int combiner, int normalize, float* out_u, float* out_inv, float* out_scale, void* ws,
                              size_t ws_bytes, mf_stream_t stream) {
    if (!table || !out_u || !out_inv || !out_scale || combiner < 0 || combiner > 2)
        return mf_set_error(MF_EINVAL, "mf_bag_forward: bad argument");
    if (int rc = bag_check("mf_bag_forward", n_rows, d, B, seg_start, seg_end, n_seg, tokens, n_tokens, max_len)) return rc;
    const int64_t C = bag_chunks(max_len);
    if (C > 0 && (!ws || ws_bytes < mf_bag_ws_bytes(B, max_len, d))) return mf_set_error(MF_ENOSPC, "mf_bag_forward: workspace too small");
    const BagSrc src{idx, seg_start, seg_end, n_seg, tokens, n_tokens, weights, max_len, n_rows};
    hipStream_t s = static_cast<hipStream_t>(stream);
    MF_DISPATCH_D(d, {
        constexpr int RPB = (64 / (D / 4)) * 4;                     // bags per 256-thread block
        const unsigned gb = (unsigned)((B + RPB - 1) / RPB);
        MF_TIMED("bag_forward", s, {
            if (C == 0) {
                bag_short_kernel<D><<<gb, 256, 0, s>>>(table, src, B, combiner, normalize, out_u, out_inv, out_scale);
            } else {
                MfArena a(ws);
                float* psum = a.take<float>((size_t)B * C * D);
                float* pw = a.take<float>((size_t)B * C * 2);
                bag_chunk_kernel<D><<<stride_grid(B * C), 256, 0, s>>>(table, src, B, C, psum, pw);
                bag_combine_kernel<D><<<gb, 256, 0, s>>>(src, B, C, psum, pw, combiner, normalize, out_u, out_inv, out_scale);
            }
        });
    });
    return mf_check_launch("mf_bag_forward");
}

// =========================================================================================== backward ====
// One workgroup: lo of every bag and the exclusive prefix of the lengths (the entry numbering); ent_off[B] = the entry count.
__global__ __launch_bounds__(BAG_PLAN_THREADS) void bag_plan_kernel(BagSrc src, int64_t B, int64_t* __restrict__ lo_out,
                                                                   int64_t* __restrict__ ent_off) {
    int64_t run = 0;
    for (int64_t b0 = 0; b0 < B; b0 += BAG_PLAN_THREADS) {
        const int64_t b = b0 + threadIdx.x;
        int64_t lo = 0, v[1] = {0}, tot[1];
        if (b < B) bag_span(src, b, lo, v[0]);
        block_excl_scan<BAG_PLAN_THREADS>(v, tot);
        if (b < B) {
            lo_out[b] = lo;
            ent_off[b] = run + v[0];
        }
        run += tot[0];
    }
    if (threadIdx.x == 0) ent_off[B] = run;
}

// bag entries: padding tokens, zero weights and bags with c_b = 0 carry nothing; entry h of bag b carries w_e * c_b * g_p[b]
struct BagEntries {
    BagSrc bags;
    const int64_t* lo;
    const int64_t* ent_off;
    const float* scale;
    const float* grad_p;
    __device__ __forceinline__ uint32_t key(int64_t b, int64_t pos) const {
        const long long tok = bags.tokens[pos];
        return bag_weight(bags, pos, tok) != 0.f && scale[b] != 0.f ? (uint32_t)tok : (uint32_t)bags.R;
    }
    template <int D>
    __device__ __forceinline__ f32x4 grad(int64_t b, int64_t h, int c) const {
        const float w = bags.weights ? bags.weights[lo[b] + (h - ent_off[b])] : 1.f;
        return reinterpret_cast<const f32x4*>(grad_p + b * D)[c] * (w * scale[b]);
    }
};

struct BagBwdWs {
    int64_t *lo, *ent_off;
    CoalesceWs co;
    size_t total;
};
static BagBwdWs bag_bwd_ws(void* ws, int64_t n_extra, int64_t B, int64_t max_len, int d) {
    MfArena a(ws);
    BagBwdWs w;
    w.lo = a.take<int64_t>((size_t)B);
    w.ent_off = a.take<int64_t>((size_t)B + 1);
    w.co = coalesce_ws(a, n_extra, B * max_len, d);
    w.total = a.used();
    return w;
}

extern "C" size_t mf_bag_backward_ws_bytes(int64_t n_extra, int64_t B, int64_t max_len, int d) {
    return bag_bwd_ws(nullptr, n_extra > 0 ? n_extra : 0, B > 0 ? B : 1, max_len > 0 ? max_len : 0, d).total;
}

extern "C" int mf_bag_backward(int64_t n_rows, int d, const int64_t* idx, int64_t B, const int64_t* seg_start, const int64_t* seg_end,
                               int64_t n_seg, const int64_t* tokens, int64_t n_tokens, const float* weights, int64_t max_len,
                               const float* scale, const float* grad_p, const int64_t* extra_ids, const float* extra_grad, int64_t n_extra,
                               int64_t capacity, int64_t* out_ids, float* out_grad, void* ws, size_t ws_bytes, mf_stream_t stream) {
    if (!scale || !grad_p || !out_ids || !out_grad) return mf_set_error(MF_EINVAL, "mf_bag_backward: bad argument");
    if (int rc = bag_check("mf_bag_backward", n_rows, d, B, seg_start, seg_end, n_seg, tokens, n_tokens, max_len)) return rc;
    const int64_t n_entries = B * max_len;
    if (int rc = coalesce_check("mf_bag_backward", "feature-table", n_rows, n_extra, extra_ids, extra_grad, n_entries, capacity, ws, ws_bytes,
                                mf_bag_backward_ws_bytes(n_extra, B, max_len, d)))
        return rc;
    if (n_extra + n_entries == 0) return MF_OK;
    const BagBwdWs w = bag_bwd_ws(ws, n_extra, B, max_len, d);
    const BagSrc bags{idx, seg_start, seg_end, n_seg, tokens, n_tokens, weights, max_len, n_rows};
    const CoalesceSrc src{n_rows, extra_ids, extra_grad, n_extra, w.lo, w.ent_off, B, n_entries};
    const BagEntries ent{bags, w.lo, w.ent_off, scale, grad_p};
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    MF_TIMED("bag_backward", s, {
        bag_plan_kernel<<<1, BAG_PLAN_THREADS, 0, s>>>(bags, B, w.lo, w.ent_off);
        rc = coalesce(src, ent, w.co, d, capacity, out_ids, out_grad, nullptr, s);
    });
    return rc ? rc : mf_check_launch("mf_bag_backward");
}
