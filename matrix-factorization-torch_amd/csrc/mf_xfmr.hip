// mf_xfmr.hip -- the transformer user tower: u_b = normalize(pool(BertEncoder(rows of user b's last L history items))),
// forward and backward, fp32 throughout (bf16-mixed dense layers on request), no float atomics, bit-reproducible.
//
// Reference interface replaced: PoolingTransformer.forward(inputs_embeds) (xfmr_rec/models.py:66-84): a BERT encoder over
// a [B, L, h] stack of embedding rows whose all-zero rows are padding, pooling_mode mean / max / cls, then Normalize.
// Here the rows are the item tower's rows of the user's history; validity comes from the id (ids outside [1, n_rows) are
// padding) and work is proportional to the valid tokens T = sum_b n_b: tokens are PACKED, user b owns tokens
// tok_off[b] .. tok_off[b + 1], oldest kept entry first (position 0).  Spec: tests/test_xfmr_tower_cpu.py (the eval-mode
// function) and tests/test_xfmr_dropout_cpu.py (training dropout).
//
//   plan      list_cut (last L valid entries, n_b), xfmr_scan (tok_off, T on the device), xfmr_pack (token -> item id, user)
//   embed     z0 = (x + tok[0]) + pos[t], x0 = LN(z0)                                   (gather + LayerNorm, one launch)
//   layer     q, k, v = X W^T + b (three GEMMs); ctx = attention per (user, head), one wave each, softmax over the n_b valid
//             keys only; z1 = ctx Wo^T + bo + X; y1 = LN(z1); a = y1 Wi^T + bi, f = act(a) (one GEMM, two outputs);
//             z2 = f Wo2^T + bo2 + y1; y2 = LN(z2)
//   pool      mean / max (first position wins ties) / cls over the n_b rows of the last layer, then u = p / max(|p|, 1e-12)
//
// GEMM engine: xfmr_gemm_kernel, v_mfma_f32_32x32x2_f32 (exact fp32 products, one k-ordered chain per element) on 64 x 64
// tiles staged through LDS, in three forms: Y = X W^T (+ bias, + residual, activation), dX = dY W (+ residual, * act'),
// and dW = dY^T X as split-K over the tokens with a FIXED number of slices (XFMR_SLICES; the slice length is a function of
// T alone) whose partials a second launch adds in slice order -- so the weight gradients do not depend on scheduling.  The
// bias gradient (column sums of dY) rides with the dW tiles of the first column block.
//
// Stash (what the forward keeps for the backward, per token): z0, x0, and per layer q, k, v, ctx, z1, y1, z2, y2 (h floats
// each), a, f (I floats each) and the two LayerNorm row statistics; the attention probabilities are recomputed.
//
// The gradient into the item table, dL/dx_t = dz0[t], leaves through the coalesce engine of mf_coalesce.h (XfmrEntries).
//
// Training dropout (mf_xfmr_forward_dropout / mf_xfmr_backward_dropout): BertModel's four sites -- the embeddings after
// their LayerNorm, the attention probabilities, the attention-output dense and the FFN-output dense before their residual
// adds.  The masks are counter-based (include/mf_numerics.h): a function of (seed, call, site, user, position, column),
// generated where they are applied; nothing is stored and the backward regenerates the same bits.  Every kernel that can
// drop is a template on that (DROP = false is the code the plain exports always ran), chosen per site on the host.
//
// Serving encode (mf_xfmr_encode, xfmr_encode_kernel): out_u of the eval-mode fp32 forward and nothing else, ONE launch, one
// workgroup per user with the user's <= 64 tokens in LDS from the cut of the list to the pooled vector -- no packing, no
// stash, no host read.  It calls the forward's own __device__ arithmetic in the forward's order: bit-identical to it.
//
// Mixed precision (mf_xfmr_forward_mixed / mf_xfmr_backward_mixed, precision MF_XFMR_BF16_MIXED): the GEMMs of the six dense
// layers per encoder layer, in all three forms, run on xfmr_gemm_bf16_kernel -- both operands rounded to bf16 (nearest even)
// where they are staged, exact products, fp32 accumulation (v_mfma_f32_32x32x16_bf16), the same fp32 epilogue; db, outputs,
// stash, parameters, gradients and every other kernel stay fp32.  MF_XFMR_FP32 launches what it always launched.
#include "mf_coalesce.h"

static constexpr int XFMR_MAX_L = 64;
static constexpr int XFMR_MAX_LAYERS = 4;
static constexpr int XFMR_SLICES = 256;          // split-K slices of a weight gradient
static constexpr int XFMR_LN_SLICES = 1024;      // token slices of the LayerNorm parameter gradients
static constexpr int XFMR_POS_SLICES = 64;       // user slices of the position-embedding gradient
static constexpr int XFMR_GLOBALS = 4;           // pos, tok, emb LN gamma, emb LN beta
static constexpr int XFMR_PER_LAYER = 16;        // Wq bq Wk bk Wv bv Wo bo g1 b1 Wi bi Wo2 bo2 g2 b2
static constexpr float XFMR_LN_EPS = 1e-12f;
static_assert(XFMR_SLICES % 64 == 0 && XFMR_LN_SLICES % 64 == 0 && XFMR_POS_SLICES % 64 == 0, "xfmr_reduce_kernel adds 64 slices at a time");

// ============================================================================================= dropout ====
// One site of one call: the host-made key, the threshold (an element is kept iff its 16-bit field >= thr) and the scale of
// the kept elements.  Hidden-state sites: element (user b, position t, column c) is field c & 3 of word ((b 64 + t) 32 + c / 4);
// attention probabilities: (b, query i, head, key j) is field j & 3 of word (((b 64 + i) 16 + head) 16 + j / 4).
struct XDrop {
    unsigned long long key;
    unsigned thr;
    float scale;
};
__device__ __forceinline__ unsigned long long xdrop_hidden_word(const XDrop& d, int64_t b, int t, int col) {
    return mf_dropout_word(d.key, (unsigned long long)((b * 64 + t) * 32 + (col >> 2)));
}
__device__ __forceinline__ unsigned long long xdrop_attn_word(const XDrop& d, int64_t b, int i, int head, int j) {
    return mf_dropout_word(d.key, (unsigned long long)(((b * 64 + i) * 16 + head) * 16 + (j >> 2)));
}

// ================================================================================================ plan ====
// One workgroup: tok_off = exclusive prefix of n_b (clamped to the host bound t_cap), tok_off[B] = T, also left in *T_dev.
__global__ __launch_bounds__(256) void xfmr_scan_kernel(const int32_t* __restrict__ nb, int64_t B, int64_t t_cap,
                                                        int64_t* __restrict__ tok_off, int32_t* __restrict__ T_dev) {
    int64_t run = 0;
    for (int64_t b0 = 0; b0 < B; b0 += 256) {
        const int64_t b = b0 + threadIdx.x;
        int64_t v[1] = {b < B ? nb[b] : 0}, tot[1];
        block_excl_scan<256>(v, tot);
        if (b < B) tok_off[b] = min(run + v[0], t_cap);
        run += tot[0];
    }
    if (threadIdx.x == 0) {
        tok_off[B] = min(run, t_cap);
        *T_dev = (int32_t)min(run, t_cap);
    }
}

// One wave per user: the valid entries of [cut, hi) in list order -> tokens tok_off[b] ..
__global__ __launch_bounds__(256) void xfmr_pack_kernel(const int64_t* __restrict__ seg_end, const int64_t* __restrict__ cut,
                                                        const int64_t* __restrict__ items, int64_t n_items, int64_t B, int64_t n_rows,
                                                        const int64_t* __restrict__ tok_off, int64_t* __restrict__ tok_item,
                                                        int32_t* __restrict__ tok_user) {
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    int64_t lo, hi;
    list_clamp(cut[b], seg_end[b], n_items, lo, hi);            // (cut[b] lies in the list: lo = cut[b])
    const int64_t t0 = tok_off[b];
    list_pack_walk(items, lo, hi, n_rows, (int)(tok_off[b + 1] - t0), [&](int slot, long long id) {   // (at most n_b <= 64 tokens)
        tok_item[t0 + slot] = id;
        tok_user[t0 + slot] = (int32_t)b;
    });
}

// ================================================================================== rows of 32 lanes ====
// H floats of a row on 32 lanes: lane c holds columns c * E .. c * E + E - 1, E = H / 32.
template <int E>
struct XRow {
    float v[E];
};
template <int E>
__device__ __forceinline__ XRow<E> xrow_load(const float* __restrict__ p, int c) {
    XRow<E> r;
    if constexpr (E == 4) {
        const f32x4 x = reinterpret_cast<const f32x4*>(p)[c];
        r.v[0] = x[0]; r.v[1] = x[1]; r.v[2] = x[2]; r.v[3] = x[3];
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) r.v[e] = p[c * E + e];
    }
    return r;
}
template <int E>
__device__ __forceinline__ void xrow_store(float* __restrict__ p, int c, const XRow<E>& r) {
    if constexpr (E == 4) {
        reinterpret_cast<f32x4*>(p)[c] = f32x4{r.v[0], r.v[1], r.v[2], r.v[3]};
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) p[c * E + e] = r.v[e];
    }
}
template <int E>
__device__ __forceinline__ float xrow_dot(const XRow<E>& a, const XRow<E>& b) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s += a.v[e] * b.v[e];
    return mf_butterfly_sum<32>(s);
}
// LayerNorm of one row (biased variance, two passes): returns y, leaves mean and 1 / sqrt(var + eps)
template <int E>
__device__ __forceinline__ XRow<E> xrow_layernorm(const XRow<E>& z, const XRow<E>& gamma, const XRow<E>& beta, float& mean, float& rstd) {
    constexpr float invh = 1.f / (float)(32 * E);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s += z.v[e];
    mean = mf_butterfly_sum<32>(s) * invh;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) q += (z.v[e] - mean) * (z.v[e] - mean);
    rstd = 1.f / sqrtf(mf_butterfly_sum<32>(q) * invh + XFMR_LN_EPS);
    XRow<E> y;
#pragma unroll
    for (int e = 0; e < E; ++e) y.v[e] = (z.v[e] - mean) * rstd * gamma.v[e] + beta.v[e];
    return y;
}
// r = r / max(|r|, 1e-12) iff do_norm (gather_rows_kernel's arithmetic); returns the factor, 1 when there is none
template <int E>
__device__ __forceinline__ float xrow_normalize(XRow<E>& r, int do_norm) {
    float inv = 1.f;
    if (do_norm) {
        inv = 1.f / fmaxf(sqrtf(xrow_dot<E>(r, r)), 1e-12f);
#pragma unroll
        for (int e = 0; e < E; ++e) r.v[e] = r.v[e] * inv;
    }
    return inv;
}
// the embeddings of one token: z = (x + te) + pe over its item row x (normalised iff norm_item), the token-type row te and its
// position's row pe; returns LN(z), leaves z and the LayerNorm's row statistics
template <int E>
__device__ __forceinline__ XRow<E> xrow_embed(XRow<E> x, int norm_item, const XRow<E>& te, const XRow<E>& pe, const XRow<E>& gamma,
                                              const XRow<E>& beta, XRow<E>& z, float& mean, float& rstd) {
    xrow_normalize<E>(x, norm_item);
#pragma unroll
    for (int e = 0; e < E; ++e) z.v[e] = (x.v[e] + te.v[e]) + pe.v[e];
    return xrow_layernorm<E>(z, gamma, beta, mean, rstd);
}
enum { XPOOL_MEAN = 0, XPOOL_MAX = 1, XPOOL_CLS = 2 };
// the pool of the n > 0 rows at y (row stride ld): their mean, their max (the first position wins ties; ARG: arg[e] = where it
// is) or row 0
template <int E, bool ARG>
__device__ __forceinline__ XRow<E> xrow_pool(const float* y, int ld, int c, int n, int mode, int* arg) {
    XRow<E> p = xrow_load<E>(y, c);
    if constexpr (ARG) {
#pragma unroll
        for (int e = 0; e < E; ++e) arg[e] = 0;
    }
    if (mode != XPOOL_CLS) {
        for (int j = 1; j < n; ++j) {
            const XRow<E> r = xrow_load<E>(y + j * ld, c);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (mode == XPOOL_MEAN) p.v[e] += r.v[e];
                else if (r.v[e] > p.v[e]) {
                    p.v[e] = r.v[e];
                    if constexpr (ARG) arg[e] = j;
                }
            }
        }
        if (mode == XPOOL_MEAN) {
#pragma unroll
            for (int e = 0; e < E; ++e) p.v[e] = p.v[e] / (float)n;
        }
    }
    return p;
}

// ============================================================================================== embed ====
// token t of user b: x = the item row (normalised iff norm_item, gather_rows_kernel's arithmetic), z0 = (x + tok[0]) + pos[t],
// x0 = LN(z0) [DROP: times the embeddings mask].  Eight tokens per workgroup.
template <int H, bool DROP>
__global__ __launch_bounds__(256) void xfmr_embed_kernel(const float* __restrict__ table, const int64_t* __restrict__ tok_item,
                                                         const int32_t* __restrict__ tok_user, const int64_t* __restrict__ tok_off,
                                                         const int32_t* __restrict__ T_dev, int norm_item, const float* __restrict__ pos,
                                                         const float* __restrict__ tok, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ z0, float* __restrict__ st0,
                                                         float* __restrict__ x0, XDrop dr) {
    constexpr int E = H / 32;
    const int c = threadIdx.x & 31;
    const int64_t t = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int64_t T = *T_dev;
    const bool valid = t < T;
    const int64_t tt = valid ? t : 0;
    const bool any = T > 0;
    const int64_t id = any ? tok_item[tt] : 0;
    const int64_t b = any ? tok_user[tt] : 0;
    const int p = any ? (int)(tt - tok_off[b]) : 0;
    XRow<E> z;
    float mean, rstd;
    XRow<E> y = xrow_embed<E>(xrow_load<E>(table + id * H, c), norm_item, xrow_load<E>(tok, c), xrow_load<E>(pos + (int64_t)p * H, c),
                              xrow_load<E>(gamma, c), xrow_load<E>(beta, c), z, mean, rstd);
    if constexpr (DROP) {                                      // (the lane's E <= 4 columns share one word)
        const unsigned long long wd = xdrop_hidden_word(dr, b, p, c * E);
#pragma unroll
        for (int e = 0; e < E; ++e) y.v[e] = y.v[e] * mf_dropout_mul(wd, (c * E + e) & 3, dr.thr, dr.scale);
    }
    if (valid) {
        xrow_store<E>(z0 + t * H, c, z);
        xrow_store<E>(x0 + t * H, c, y);
        if (c == 0) {
            st0[2 * t] = mean;
            st0[2 * t + 1] = rstd;
        }
    }
}

// ========================================================================================== LayerNorm ====
template <int H>
__global__ __launch_bounds__(256) void xfmr_ln_kernel(const float* __restrict__ z, const int32_t* __restrict__ T_dev,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float* __restrict__ y, float* __restrict__ st) {
    constexpr int E = H / 32;
    const int c = threadIdx.x & 31;
    const int64_t t = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int64_t T = *T_dev;
    if ((int64_t)blockIdx.x * 8 >= T) return;                 // (whole workgroup)
    const bool valid = t < T;
    const XRow<E> zr = xrow_load<E>(z + (valid ? t : 0) * H, c);
    float mean, rstd;
    const XRow<E> yr = xrow_layernorm<E>(zr, xrow_load<E>(gamma, c), xrow_load<E>(beta, c), mean, rstd);
    if (valid) {
        xrow_store<E>(y + t * H, c, yr);
        if (c == 0) {
            st[2 * t] = mean;
            st[2 * t + 1] = rstd;
        }
    }
}

// length of one of S token slices: a function of T alone
__device__ __forceinline__ int64_t xfmr_slice_len(int64_t T, int S, int round) {
    const int64_t per = (T + S - 1) / S;
    return (per + round - 1) / round * round;
}

// dz = rstd * (dy gamma - mean(dy gamma) - xhat mean(dy gamma xhat)); slice s of the tokens also leaves its partial of
// dgamma = sum dy xhat and dbeta = sum dy in part[s][2H] (eight row groups, added in group order).
// DROP = XLN_DROP_IN: this LayerNorm's output was dropped (the embeddings): dy is read as mask * dy.  DROP = XLN_DROP_OUT: its
// input is dropped(dense) + residual: dz goes to the residual path as it is and dzm = mask * dz to the dense's backward.
enum { XLN_DROP_NONE = 0, XLN_DROP_IN = 1, XLN_DROP_OUT = 2 };
template <int H, int DROP>
__global__ __launch_bounds__(256) void xfmr_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                          const float* __restrict__ st, const int32_t* __restrict__ T_dev,
                                                          const float* __restrict__ gamma, float* __restrict__ dz,
                                                          float* __restrict__ part, const int32_t* __restrict__ tok_user,
                                                          const int64_t* __restrict__ tok_off, XDrop dr, float* __restrict__ dzm) {
    constexpr int E = H / 32;
    constexpr float invh = 1.f / (float)H;
    __shared__ float sh[8][2 * H];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int64_t T = *T_dev;
    const int64_t len = xfmr_slice_len(T, XFMR_LN_SLICES, 8);
    const int64_t beg = (int64_t)blockIdx.x * len, end = min(beg + len, T);
    const XRow<E> gm = xrow_load<E>(gamma, c);
    XRow<E> ag, ab;
#pragma unroll
    for (int e = 0; e < E; ++e) ag.v[e] = ab.v[e] = 0.f;
    for (int64_t t0 = beg; t0 < end; t0 += 8) {              // (uniform trip count: the row sums need whole waves)
        const int64_t t = t0 + g;
        const bool valid = t < end;
        const int64_t tt = valid ? t : beg;
        XRow<E> d = xrow_load<E>(dy + tt * H, c);
        const XRow<E> zr = xrow_load<E>(z + tt * H, c);
        const float mean = st[2 * tt], rstd = st[2 * tt + 1];
        float mul[E];
        if constexpr (DROP != XLN_DROP_NONE) {
            const int64_t b = tok_user[tt];
            const unsigned long long wd = xdrop_hidden_word(dr, b, (int)(tt - tok_off[b]), c * E);
#pragma unroll
            for (int e = 0; e < E; ++e) mul[e] = mf_dropout_mul(wd, (c * E + e) & 3, dr.thr, dr.scale);
        }
        if constexpr (DROP == XLN_DROP_IN) {
#pragma unroll
            for (int e = 0; e < E; ++e) d.v[e] = d.v[e] * mul[e];
        }
        XRow<E> xh, gd;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            xh.v[e] = (zr.v[e] - mean) * rstd;
            gd.v[e] = d.v[e] * gm.v[e];
            s1 += gd.v[e];
            s2 += gd.v[e] * xh.v[e];
        }
        const float m1 = mf_butterfly_sum<32>(s1) * invh, m2 = mf_butterfly_sum<32>(s2) * invh;
        if (valid) {
            XRow<E> o;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                o.v[e] = rstd * (gd.v[e] - m1 - xh.v[e] * m2);
                ag.v[e] += d.v[e] * xh.v[e];
                ab.v[e] += d.v[e];
            }
            xrow_store<E>(dz + t * H, c, o);
            if constexpr (DROP == XLN_DROP_OUT) {
#pragma unroll
                for (int e = 0; e < E; ++e) o.v[e] = o.v[e] * mul[e];
                xrow_store<E>(dzm + t * H, c, o);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        sh[g][c * E + e] = ag.v[e];
        sh[g][H + c * E + e] = ab.v[e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * H; i += 256) {
        float s = sh[0][i];
#pragma unroll
        for (int q = 1; q < 8; ++q) s += sh[q][i];
        part[(int64_t)blockIdx.x * 2 * H + i] = s;
    }
}

// out[i] = sum_s part[s][i] in a fixed order: eight consecutive slices, eight of those sums, then the sums of 64 -- chains of
// 8 + 8 + S / 64 additions, not one of S (a 1,024-term chain loses ~ sqrt(S) ulp: 8x the fp32 reference's error on a
// LayerNorm weight gradient at T = 4096).  S is a multiple of 64.  Element i goes to out_a (i < n_a) or out_b.
__global__ __launch_bounds__(256) void xfmr_reduce_kernel(const float* __restrict__ part, int S, int64_t size, int64_t n_a,
                                                          float* __restrict__ out_a, float* __restrict__ out_b) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= size) return;
    float s = 0.f;
    for (int q2 = 0; q2 < S; q2 += 64) {
        float s1 = 0.f;
#pragma unroll
        for (int q1 = 0; q1 < 64; q1 += 8) {
            float s0 = part[(int64_t)(q2 + q1) * size + i];
#pragma unroll
            for (int q = 1; q < 8; ++q) s0 += part[(int64_t)(q2 + q1 + q) * size + i];
            s1 = q1 ? s1 + s0 : s0;
        }
        s = q2 ? s + s1 : s1;
    }
    if (i < n_a) out_a[i] = s;
    else out_b[i - n_a] = s;
}

// ========================================================================================= activations ====
enum { XACT_GELU = 0, XACT_RELU = 1, XACT_SILU = 2, XACT_GELU_NEW = 3 };
__device__ __forceinline__ float xfmr_act(float x, int kind) {
    switch (kind) {
        case XACT_RELU: return x > 0.f ? x : 0.f;
        case XACT_SILU: return x / (1.f + expf(-x));
        case XACT_GELU_NEW: {
            const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
            return 0.5f * x * (1.f + tanhf(u));
        }
        default: return 0.5f * x * (1.f + erff(x * 0.7071067811865476f));
    }
}
__device__ __forceinline__ float xfmr_dact(float x, int kind) {
    switch (kind) {
        case XACT_RELU: return x > 0.f ? 1.f : 0.f;
        case XACT_SILU: {
            const float s = 1.f / (1.f + expf(-x));
            return s * (1.f + x * (1.f - s));
        }
        case XACT_GELU_NEW: {
            const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
            const float th = tanhf(u);
            const float du = 0.7978845608028654f * (1.f + 3.f * 0.044715f * x * x);
            return 0.5f * (1.f + th) + 0.5f * x * (1.f - th * th) * du;
        }
        default: return 0.5f * (1.f + erff(x * 0.7071067811865476f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);
    }
}

// ================================================================================================ GEMM ====
// C[m][n] = sum_k A(m, k) B(n, k).  An operand is k-contiguous (elem(r, k) = p[r * ld + k]; ld a multiple of 4, 16-byte
// aligned) or row-contiguous (elem(r, k) = p[k * ld + r]).  dyn = 0: M = *T_dev tokens (tiles past T exit), K static (a
// multiple of 16); dyn = 1: K = *T_dev, cut into XFMR_SLICES slices (blockIdx.z), slice s writes its partial tile to
// C + s * slice_stride and, for the first column block, the column sums of A to C + s * slice_stride + M * N.
enum { XEPI_NONE = 0, XEPI_ACT = 1, XEPI_DACT = 2 };
struct XGemm {
    const float* A; int64_t lda; int a_kc;
    const float* B; int64_t ldb; int b_kc;
    float* C; int64_t ldc;
    int M, N, K;                 // static extents (the dynamic one is ignored)
    const int32_t* T_dev; int dyn;
    const float* bias;           // [N] or null
    const float* R;              // [*, ldc] added to the result, or null (may alias C)
    int epi, act;
    float* C2;                   // XEPI_ACT: act(result)
    const float* P;              // XEPI_DACT: pre-activations, result *= act'(P)
    int64_t slice_stride;
};
static constexpr int XG_LD = 68;        // LDS row stride of a 16 x 64 operand tile

// stage: the thread's share of a 64 (rows) x 16 (k) operand tile, global -> registers -> LDS[k][row]
__device__ __forceinline__ f32x4 xg_fetch(const float* __restrict__ p, int64_t ld, int kc, int64_t r0, int64_t r_lim, int64_t k0,
                                          int64_t k_lim) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (kc) {                                               // row = t / 4, k = (t % 4) * 4 .. + 3 (K is a multiple of 16: no k tail)
        const int64_t r = r0 + (threadIdx.x >> 2), k = k0 + (threadIdx.x & 3) * 4;
        if (r < r_lim && k < k_lim) v = *reinterpret_cast<const f32x4*>(p + r * ld + k);
    } else {                                                // row = t % 64, k = t / 64 + 4 i
        const int64_t r = r0 + (threadIdx.x & 63);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t k = k0 + (threadIdx.x >> 6) + 4 * i;
            if (r < r_lim && k < k_lim) v[i] = p[k * ld + r];
        }
    }
    return v;
}
__device__ __forceinline__ void xg_stage(float (*tile)[XG_LD], int kc, const f32x4& v) {
    if (kc) {
        const int r = threadIdx.x >> 2, k = (threadIdx.x & 3) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[k + i][r] = v[i];
    } else {
        const int r = threadIdx.x & 63, k = threadIdx.x >> 6;
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[k + 4 * i][r] = v[i];
    }
}

// DROP (a linear with a residual, dyn = 0): C = (acc + bias) * mask + R, the mask of row m = token (b, t) at column n
struct XDropRows {
    XDrop d;
    const int32_t* tok_user;
    const int64_t* tok_off;
};
// What both forms of the engine begin with: the workgroup's 64 x 64 tile (rows m0 .. of M, columns n0 ..), its k range and output
// (dyn = 1: slice blockIdx.z of the T tokens and that slice's partials), the wave's 32 x 32 block (wm, wn) and the lane's place
// in an MFMA operand (row l31, k half hh).  empty: the tile lies past the M rows, the whole workgroup leaves.
struct XgTile {
    int64_t T, M, m0, n0, kbeg, kend;
    float* C;
    int wm, wn, l31, hh;
    bool empty;
};
__device__ __forceinline__ XgTile xg_tile(const XGemm& g) {
    XgTile t;
    t.T = *g.T_dev;
    t.M = g.dyn == 0 ? t.T : g.M;
    t.m0 = (int64_t)blockIdx.x * 64, t.n0 = (int64_t)blockIdx.y * 64;
    t.empty = t.m0 >= t.M;
    t.kbeg = 0, t.kend = g.K, t.C = g.C;
    if (g.dyn == 1) {
        const int64_t len = xfmr_slice_len(t.T, XFMR_SLICES, 16);
        t.kbeg = min((int64_t)blockIdx.z * len, t.T);
        t.kend = min(t.kbeg + len, t.T);
        t.C += (int64_t)blockIdx.z * g.slice_stride;
    }
    const int lane = mf_lane(), wave = threadIdx.x >> 6;
    t.wm = wave >> 1, t.wn = wave & 1, t.l31 = lane & 31, t.hh = lane >> 5;
    return t;
}
// the wave's 32 x 32 block of the tile (rows m0 + wm 32 .., columns n0 + wn 32 ..) -> memory, fp32 in both precisions
template <bool DROP>
__device__ __forceinline__ void xg_epilogue(const XGemm& g, const XDropRows& dr, const XgTile& t, const f32x16& acc) {
    float* __restrict__ C = t.C;
    const int64_t n = t.n0 + t.wn * 32 + t.l31;
    if (n < g.N) {
        const float bias = g.bias ? g.bias[n] : 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t m = t.m0 + t.wm * 32 + mf_acc_row(e, t.hh);
            if (m < t.M) {
                const int64_t o = m * g.ldc + n;
                float v = acc[e] + bias;
                if constexpr (DROP) {
                    const int64_t b = dr.tok_user[m];
                    v = v * mf_dropout_mul(xdrop_hidden_word(dr.d, b, (int)(m - dr.tok_off[b]), (int)n), (int)n & 3, dr.d.thr, dr.d.scale);
                }
                if (g.R) v += g.R[o];
                if (g.epi == XEPI_ACT) g.C2[o] = xfmr_act(v, g.act);
                else if (g.epi == XEPI_DACT) v *= xfmr_dact(g.P[o], g.act);
                C[o] = v;
            }
        }
    }
}

template <bool DROP>
__global__ __launch_bounds__(256) void xfmr_gemm_kernel(XGemm g, XDropRows dr) {
    __shared__ float As[16][XG_LD], Bs[16][XG_LD];
    const XgTile t = xg_tile(g);
    if (t.empty) return;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float colsum = 0.f;
    const bool want_colsum = g.dyn == 1 && blockIdx.y == 0 && threadIdx.x < 64;
    f32x4 ra = xg_fetch(g.A, g.lda, g.a_kc, t.m0, t.M, t.kbeg, t.kend);
    f32x4 rb = xg_fetch(g.B, g.ldb, g.b_kc, t.n0, g.N, t.kbeg, t.kend);
    for (int64_t k0 = t.kbeg; k0 < t.kend; k0 += 16) {
        __syncthreads();
        xg_stage(As, g.a_kc, ra);
        xg_stage(Bs, g.b_kc, rb);
        __syncthreads();
        if (k0 + 16 < t.kend) {                              // the next tile's loads fly under this tile's MFMAs
            ra = xg_fetch(g.A, g.lda, g.a_kc, t.m0, t.M, k0 + 16, t.kend);
            rb = xg_fetch(g.B, g.ldb, g.b_kc, t.n0, g.N, k0 + 16, t.kend);
        }
#pragma unroll
        for (int kk = 0; kk < 16; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + t.hh][t.wm * 32 + t.l31], Bs[kk + t.hh][t.wn * 32 + t.l31], acc, 0, 0, 0);
        if (want_colsum) {
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) colsum += As[kk][threadIdx.x];
        }
    }
    xg_epilogue<DROP>(g, dr, t, acc);
    if (want_colsum && t.m0 + threadIdx.x < t.M) t.C[(int64_t)g.M * g.N + t.m0 + threadIdx.x] = colsum;
}

// ---- the bf16-mixed form of the engine (precision MF_XFMR_BF16_MIXED) ----
// The same tiles, operand forms, slices and epilogue; both operands are rounded to bf16 (round-to-nearest-even, the
// conversion of (__bf16)) on their way from the fetch registers to LDS, the products are exact and the accumulation is fp32:
// v_mfma_f32_32x32x16_bf16, whose operand of lane l is row l & 31, k = 8 (l >> 5) .. + 7 of a 16-deep step.  A stage is 64 rows
// x 32 k, LDS[row][k] in bf16 (half the bytes of the fp32 tile for twice the k); what a fetch finds past the end of k (a token
// tail, the second half of a 16-token slice) is zero.  The bias gradient stays the fp32 sum of the UNROUNDED dY: every thread
// adds what it fetched (dyn = 1: A is row-contiguous, thread t holds row t & 63 at k = t / 64 mod 4), four partials per row
// meet in LDS in a fixed order.
typedef __bf16 xbf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 xbf16x8 __attribute__((ext_vector_type(8)));
static constexpr int XGB_K = 32;        // k of a stage: two halves of 16, each one xg_fetch
static constexpr int XGB_LD = 40;       // LDS row stride in bf16: 80 bytes, 16-byte rows, conflict-free 16-byte reads

__device__ __forceinline__ void xgb_stage(__bf16 (*tile)[XGB_LD], int kc, int half, const f32x4& v) {
    if (kc) {
        const int r = threadIdx.x >> 2, k = 16 * half + (threadIdx.x & 3) * 4;
        *reinterpret_cast<xbf16x4*>(&tile[r][k]) = xbf16x4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    } else {
        const int r = threadIdx.x & 63, k = 16 * half + (threadIdx.x >> 6);
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[r][k + 4 * i] = (__bf16)v[i];
    }
}

template <bool DROP>
__global__ __launch_bounds__(256) void xfmr_gemm_bf16_kernel(XGemm g, XDropRows dr) {
    __shared__ __attribute__((aligned(16))) __bf16 As[64][XGB_LD], Bs[64][XGB_LD];
    __shared__ float cs[4][64];
    const XgTile t = xg_tile(g);
    if (t.empty) return;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float colsum = 0.f;
    const bool want_colsum = g.dyn == 1 && blockIdx.y == 0;     // (whole workgroup)
    f32x4 ra[2], rb[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        ra[half] = xg_fetch(g.A, g.lda, g.a_kc, t.m0, t.M, t.kbeg + 16 * half, t.kend);
        rb[half] = xg_fetch(g.B, g.ldb, g.b_kc, t.n0, g.N, t.kbeg + 16 * half, t.kend);
    }
    for (int64_t k0 = t.kbeg; k0 < t.kend; k0 += XGB_K) {
        __syncthreads();
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            xgb_stage(As, g.a_kc, half, ra[half]);
            xgb_stage(Bs, g.b_kc, half, rb[half]);
        }
        if (want_colsum) colsum += ((ra[0][0] + ra[0][1]) + (ra[0][2] + ra[0][3])) + ((ra[1][0] + ra[1][1]) + (ra[1][2] + ra[1][3]));
        __syncthreads();
        if (k0 + XGB_K < t.kend) {                           // the next stage's loads fly under this stage's MFMAs
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                ra[half] = xg_fetch(g.A, g.lda, g.a_kc, t.m0, t.M, k0 + XGB_K + 16 * half, t.kend);
                rb[half] = xg_fetch(g.B, g.ldb, g.b_kc, t.n0, g.N, k0 + XGB_K + 16 * half, t.kend);
            }
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const xbf16x8 a = *reinterpret_cast<const xbf16x8*>(&As[t.wm * 32 + t.l31][16 * half + 8 * t.hh]);
            const xbf16x8 b = *reinterpret_cast<const xbf16x8*>(&Bs[t.wn * 32 + t.l31][16 * half + 8 * t.hh]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
        }
    }
    xg_epilogue<DROP>(g, dr, t, acc);
    if (want_colsum) {
        cs[threadIdx.x >> 6][mf_lane()] = colsum;
        __syncthreads();
        if (threadIdx.x < 64 && t.m0 + threadIdx.x < t.M)
            t.C[(int64_t)g.M * g.N + t.m0 + threadIdx.x] = (cs[0][threadIdx.x] + cs[1][threadIdx.x]) + (cs[2][threadIdx.x] + cs[3][threadIdx.x]);
    }
}

// =========================================================================================== attention ====
// One wave per (user, head): keys across lanes.  K and V of the head sit in LDS; per query the scores, the softmax over
// the n valid keys and the context stay in registers / LDS: nothing [L, L] goes to memory.
template <int DH>
__device__ __forceinline__ void xattn_load(float (*dst)[DH + 1], const float* __restrict__ src, int64_t t0, int n, int h, int col0) {
    for (int i = mf_lane(); i < n * DH; i += 64) {
        const int j = i / DH, c = i % DH;
        dst[j][c] = src[(t0 + j) * h + col0 + c];
    }
}
__device__ __forceinline__ float xattn_bcast(float x, int src_lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src_lane));
}
__device__ __forceinline__ float xattn_wave_max(float x) {
    x = fmaxf(x, mf_xor_lane<32>(x)); x = fmaxf(x, mf_xor_lane<16>(x)); x = fmaxf(x, mf_xor_lane<8>(x));
    x = fmaxf(x, mf_xor_lane<4>(x)); x = fmaxf(x, mf_xor_lane<2>(x)); x = fmaxf(x, mf_xor_lane<1>(x));
    return x;
}
// softmax probability of this lane's key (its DH floats at krow) for the query row qv (lane c holds q[c]); inactive lanes give 0
template <int DH>
__device__ __forceinline__ float xattn_prob(float qv, const float* krow, bool active) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < DH; ++c) s += xattn_bcast(qv, c) * krow[c];
    s = active ? s / sqrtf((float)DH) : -__builtin_huge_valf();
    const float mx = xattn_wave_max(s);
    const float e = active ? expf(s - mx) : 0.f;
    return e / mf_wave_sum(e);
}
template <int DH>
__device__ __forceinline__ float xattn_prob(float qv, const float (*Ks)[DH + 1], int row, bool active) {
    return xattn_prob<DH>(qv, &Ks[row][0], active);
}
// out[c] = sum_j w[j] M[j][c] for c < DH (row j of M at m + j ld): 64 / DH lane groups take every (64 / DH)-th key, then a fixed
// butterfly
template <int DH>
__device__ __forceinline__ float xattn_mix(const float* w, const float* m, int ld, int lane, int n) {
    constexpr int G = 64 / DH;
    const int c = lane % DH, jg = lane / DH;
    float acc = 0.f;
    for (int j = jg; j < n; j += G) acc += w[j] * m[j * ld + c];
    if constexpr (DH <= 32) acc += mf_xor_lane<32>(acc);
    if constexpr (DH <= 16) acc += mf_xor_lane<16>(acc);
    if constexpr (DH <= 8) acc += mf_xor_lane<8>(acc);
    return acc;
}
template <int DH>
__device__ __forceinline__ float xattn_mix(const float* w, const float (*Ms)[DH + 1], int lane, int n) {
    return xattn_mix<DH>(w, &Ms[0][0], DH + 1, lane, n);
}

template <int DH, bool DROP>
__global__ __launch_bounds__(64) void xfmr_attn_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                       const int64_t* __restrict__ tok_off, int h, int heads, float* __restrict__ ctx,
                                                       XDrop dr) {
    __shared__ float Ks[XFMR_MAX_L][DH + 1], Vs[XFMR_MAX_L][DH + 1], Ps[XFMR_MAX_L];
    const int64_t b = blockIdx.x / heads;
    const int col0 = (int)(blockIdx.x % heads) * DH;
    const int64_t t0 = tok_off[b];
    const int n = (int)min(tok_off[b + 1] - t0, (int64_t)XFMR_MAX_L);
    if (n <= 0) return;
    const int lane = mf_lane();
    xattn_load<DH>(Ks, k, t0, n, h, col0);
    xattn_load<DH>(Vs, v, t0, n, h, col0);
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        const float qv = lane < DH ? q[(t0 + i) * h + col0 + lane] : 0.f;
        float p = xattn_prob<DH>(qv, Ks, lane < n ? lane : 0, lane < n);
        if constexpr (DROP) {                                    // lane j's probability of query i: one word per lane per query
            const unsigned long long wd = xdrop_attn_word(dr, b, i, (int)(blockIdx.x % heads), lane);
            p = p * mf_dropout_mul(wd, lane & 3, dr.thr, dr.scale);
        }
        __syncthreads();
        Ps[lane] = p;
        __syncthreads();
        const float o = xattn_mix<DH>(Ps, Vs, lane, n);
        if (lane < DH) ctx[(t0 + i) * h + col0 + lane] = o;
    }
}

// backward: the probabilities are recomputed; lane j accumulates dK[j], dV[j] over the queries, dQ[i] is a mix over keys.
// DROP: the mask is recomputed too (one word per lane per query): dV[j] += (p mask) dc, dp = mask (dc . V[j]).
template <int DH, bool DROP>
__global__ __launch_bounds__(64) void xfmr_attn_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, const float* __restrict__ dctx,
                                                           const int64_t* __restrict__ tok_off, int h, int heads, float* __restrict__ dq,
                                                           float* __restrict__ dk, float* __restrict__ dv, XDrop dr) {
    __shared__ float Ks[XFMR_MAX_L][DH + 1], Vs[XFMR_MAX_L][DH + 1], Ps[XFMR_MAX_L], Qs[64], Ds[64];
    const int64_t b = blockIdx.x / heads;
    const int col0 = (int)(blockIdx.x % heads) * DH;
    const int64_t t0 = tok_off[b];
    const int n = (int)min(tok_off[b + 1] - t0, (int64_t)XFMR_MAX_L);
    if (n <= 0) return;
    const int lane = mf_lane(), row = lane < n ? lane : 0;
    xattn_load<DH>(Ks, k, t0, n, h, col0);
    xattn_load<DH>(Vs, v, t0, n, h, col0);
    __syncthreads();
    float dK[DH], dV[DH];
#pragma unroll
    for (int c = 0; c < DH; ++c) dK[c] = dV[c] = 0.f;
    const float inv_scale = 1.f / sqrtf((float)DH);
    for (int i = 0; i < n; ++i) {
        const float qv = lane < DH ? q[(t0 + i) * h + col0 + lane] : 0.f;
        const float dc = lane < DH ? dctx[(t0 + i) * h + col0 + lane] : 0.f;
        const float p = xattn_prob<DH>(qv, Ks, row, lane < n);
        float dp = 0.f;
#pragma unroll
        for (int c = 0; c < DH; ++c) dp += xattn_bcast(dc, c) * Vs[row][c];
        float pm = p;                                        // the probability that met V in the forward
        if constexpr (DROP) {
            const float mul = mf_dropout_mul(xdrop_attn_word(dr, b, i, (int)(blockIdx.x % heads), lane), lane & 3, dr.thr, dr.scale);
            pm = p * mul;
            dp = dp * mul;
        }
        const float pd = lane < n ? p * dp : 0.f;
        const float pdsum = mf_wave_sum(pd);                 // (whole wave: not inside the select below)
        const float ds = lane < n ? (p * (dp - pdsum)) * inv_scale : 0.f;
        __syncthreads();
        Ps[lane] = ds;
        Qs[lane] = qv;                                       // (from LDS below: 2 DH more lane reads would not fit the SGPRs)
        Ds[lane] = dc;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < DH; ++c) {
            dK[c] += ds * Qs[c];
            dV[c] += pm * Ds[c];
        }
        const float o = xattn_mix<DH>(Ps, Ks, lane, n);
        if (lane < DH) dq[(t0 + i) * h + col0 + lane] = o;
    }
    __syncthreads();
    if (lane < n) {
#pragma unroll
        for (int c = 0; c < DH; ++c) {
            Ks[lane][c] = dK[c];
            Vs[lane][c] = dV[c];
        }
    }
    __syncthreads();
    for (int i = lane; i < n * DH; i += 64) {
        const int j = i / DH, c = i % DH;
        dk[(t0 + j) * h + col0 + c] = Ks[j][c];
        dv[(t0 + j) * h + col0 + c] = Vs[j][c];
    }
}

// ================================================================================================ pool ====
// 32 lanes per user: p = xrow_pool of the n_b rows (0 when there is none), u = p / max(|p|, 1e-12)
template <int H>
__global__ __launch_bounds__(256) void xfmr_pool_kernel(const float* __restrict__ y, const int64_t* __restrict__ tok_off, int64_t B, int mode,
                                                        int norm_user, float* __restrict__ out_u, float* __restrict__ out_inv,
                                                        int32_t* __restrict__ out_arg) {
    constexpr int E = H / 32;
    const int c = threadIdx.x & 31;
    const int64_t b = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool valid = b < B;
    const int64_t t0 = valid ? tok_off[b] : 0;
    const int n = valid ? (int)(tok_off[b + 1] - t0) : 0;
    XRow<E> p;
    int arg[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        p.v[e] = 0.f;
        arg[e] = -1;
    }
    if (n > 0) p = xrow_pool<E, true>(y + t0 * H, H, c, n, mode, arg);
    const float inv = xrow_normalize<E>(p, norm_user);
    if (valid) {
        xrow_store<E>(out_u + b * H, c, p);
        if (c == 0) out_inv[b] = inv;
        if (mode == XPOOL_MAX) {
#pragma unroll
            for (int e = 0; e < E; ++e) out_arg[b * H + c * E + e] = arg[e];
        }
    }
}

// 32 lanes per token: dL/dy of the last layer's row from dL/du (through the normalisation and the pool)
template <int H>
__global__ __launch_bounds__(256) void xfmr_pool_bwd_kernel(const float* __restrict__ grad_u, const float* __restrict__ u,
                                                            const float* __restrict__ inv, const int32_t* __restrict__ arg,
                                                            const int64_t* __restrict__ tok_off, const int32_t* __restrict__ tok_user,
                                                            const int32_t* __restrict__ T_dev, int mode, int norm_user,
                                                            float* __restrict__ dy) {
    constexpr int E = H / 32;
    const int c = threadIdx.x & 31;
    const int64_t t = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int64_t T = *T_dev;
    if ((int64_t)blockIdx.x * 8 >= T) return;
    const bool valid = t < T;
    const int64_t b = tok_user[valid ? t : 0];
    const int64_t t0 = tok_off[b];
    const int j = (int)((valid ? t : 0) - t0), n = (int)(tok_off[b + 1] - t0);
    XRow<E> g = xrow_load<E>(grad_u + b * H, c);
    if (norm_user) {
        const XRow<E> ur = xrow_load<E>(u + b * H, c);
        const float pr = xrow_dot<E>(g, ur), iv = inv[b];
#pragma unroll
        for (int e = 0; e < E; ++e) g.v[e] = (g.v[e] - ur.v[e] * pr) * iv;
    }
    XRow<E> o;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (mode == XPOOL_MEAN) o.v[e] = g.v[e] / (float)n;
        else if (mode == XPOOL_CLS) o.v[e] = j == 0 ? g.v[e] : 0.f;
        else o.v[e] = arg[b * H + c * E + e] == j ? g.v[e] : 0.f;
    }
    if (valid) xrow_store<E>(dy + t * H, c, o);
}

// position-embedding gradient: slice s of the users, position t: part[s][t][c] = sum_b dz0[tok_off[b] + t][c] (b in order)
__global__ __launch_bounds__(128) void xfmr_pos_bwd_kernel(const float* __restrict__ dz0, const int64_t* __restrict__ tok_off, int64_t B,
                                                           int H, int L, float* __restrict__ part) {
    const int t = blockIdx.x, s = blockIdx.y, c = threadIdx.x;
    if (c >= H) return;
    const int64_t per = (B + XFMR_POS_SLICES - 1) / XFMR_POS_SLICES;
    const int64_t b1 = min((int64_t)(s + 1) * per, B);
    float acc = 0.f;
    for (int64_t b = (int64_t)s * per; b < b1; ++b) {
        const int64_t t0 = tok_off[b];
        if (t0 + t < tok_off[b + 1]) acc += dz0[(t0 + t) * H + c];
    }
    part[((int64_t)s * L + t) * H + c] = acc;
}
// token-type row 0 receives every token's gradient = the column sums of dpos (rows >= L are zero); row 1 none
__global__ __launch_bounds__(128) void xfmr_tok_bwd_kernel(const float* __restrict__ dpos, int H, int L, float* __restrict__ dtok) {
    const int c = threadIdx.x;
    if (c >= H) return;
    float acc = 0.f;
    for (int t = 0; t < L; ++t) acc += dpos[(int64_t)t * H + c];
    dtok[c] = acc;
    dtok[H + c] = 0.f;
}

// ====================================================================================== serving encode ====
// mf_xfmr_encode: the eval-mode forward of ONE user per workgroup (256 threads), cut to pooled vector in one launch, every
// activation in LDS, nothing per token in global memory.  Four [64][H + 4] buffers (x, q, k, v by their first use) carry a layer:
//   q, k, v = x W^T + b                      (one pass over the 3 H / 32 column blocks, one wave per block)
//   ctx     = attention, one wave per head, K and V read in place; ctx overwrites q (a query row is read before it is written)
//   z1      = ctx Wo^T + bo + x  -> k;  y1 = LN(z1) in place
//   FFN in chunks of <= H intermediate columns: f = act(y1 Wi^T + bi) -> q;  acc += f Wo2^T with the [64, H] accumulators in
//             registers across the chunks (each output element stays one ascending-k chain)
//   z2      = acc + bo2 + y1 -> v;  y2 = LN(z2) in place; v is the next layer's x
// A GEMM column block is v_mfma_f32_32x32x2_f32 over k ascending from 0 into zeroed accumulators, the A operand from LDS, the
// weight rows from global memory (L2), lanes 0..31 feeding k and 32..63 k + 1: xfmr_gemm_kernel's chain, and xenc_store spells
// xg_epilogue<false>'s (acc + bias) + r and act(.) again, on LDS -- the one piece of the forward's arithmetic written twice.
// Every other float expression is a __device__ function that the forward's kernels call too: xrow_embed (xrow_normalize, then
// xrow_layernorm) as in xfmr_embed_kernel, xrow_layernorm as in xfmr_ln_kernel, xattn_prob and xattn_mix as in xfmr_attn_kernel,
// xfmr_act, xrow_pool and xrow_normalize as in xfmr_pool_kernel; the token ids come from list_cut_walk and list_pack_walk
// (mf_lists.h), the walks of list_cut_kernel and xfmr_pack_kernel.  The library is built with -ffp-contract=off, so at fp32 u is
// bit-identical to mf_xfmr_forward's out_u.  Rows >= n_b of a buffer hold whatever was there: no output depends on them (a
// GEMM row, a LayerNorm row and a softmax over the n_b valid keys read their own rows only), and with n_b <= 32 the second 32-row
// block is skipped.
static constexpr int XENC_PAD = 4;          // row stride H + 4 floats: rows stay 16-byte aligned
struct XEnc {
    const float* table; int64_t n_rows;
    const int64_t *seg_start, *seg_end, *items; int64_t n_items;
    int L, layers, heads, I, act, mode, norm_item, norm_user;
    const float* prm[XFMR_GLOBALS + XFMR_PER_LAYER * XFMR_MAX_LAYERS];
    float* out_u;
};
static size_t xenc_lds_bytes(int h) {
    return ((size_t)4 * XFMR_MAX_L * (h + XENC_PAD) + 4 * 64) * sizeof(float) + XFMR_MAX_L * sizeof(int64_t) + 16;
}
// LDS writes of this wave -> LDS reads of this wave's other lanes (the waves of a workgroup walk different heads: no barrier)
__device__ __forceinline__ void xenc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// One wave, one 32-column block: acc[rb][.] += sum_k A[rb 32 + row][k] w[col][k], k ascending over [0, K) (K a multiple of 16);
// a = the A rows in LDS (row stride lda), wrow = this lane's weight row at its first k.  The next 16 k of the weights are
// fetched under the MFMAs of the current ones.
__device__ __forceinline__ void xenc_mma(const float* a, int lda, const float* __restrict__ wrow, int K, int nrb, int l31, int hh,
                                         f32x16 (&acc)[2]) {
    f32x4 w[4], wn[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = reinterpret_cast<const f32x4*>(wrow)[q];
#pragma unroll 1
    for (int k0 = 0; k0 < K; k0 += 16) {
        if (k0 + 16 < K) {
#pragma unroll
            for (int q = 0; q < 4; ++q) wn[q] = reinterpret_cast<const f32x4*>(wrow + k0 + 16)[q];
        }
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            if (rb < nrb) {
                const f32x4* ar = reinterpret_cast<const f32x4*>(a + (rb * 32 + l31) * lda + k0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 x = ar[q];
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(hh ? x[1] : x[0], hh ? w[q][1] : w[q][0], acc[rb], 0, 0, 0);
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(hh ? x[3] : x[2], hh ? w[q][3] : w[q][2], acc[rb], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = wn[q];
    }
}
__device__ __forceinline__ void xenc_zero(f32x16 (&acc)[2]) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[rb][e] = 0.f;
}
// xg_epilogue<false> on LDS: out[m][n] = act((acc + bias[n]) + r[m][n]) for the wave's column block n0 (r null: no residual;
// act < 0: none); out and r have row stride ld
__device__ __forceinline__ void xenc_store(const f32x16 (&acc)[2], int nrb, int n0, const float* __restrict__ bias, const float* r,
                                           int act, float* out, int ld, int l31, int hh) {
    const int n = n0 + l31;
    const float bv = bias[n];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        if (rb < nrb) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int o = (rb * 32 + mf_acc_row(e, hh)) * ld + n;
                float v = acc[rb][e] + bv;
                if (r) v += r[o];
                out[o] = v;
            }
        }
    }
    if (act >= 0) {                // each lane over its own elements again, as a loop: one copy of xfmr_act's code, not 32
#pragma unroll 1
        for (int i = 0; i < 16 * nrb; ++i) {
            const int o = ((i >> 4) * 32 + mf_acc_row(i & 15, hh)) * ld + n;
            out[o] = xfmr_act(out[o], act);
        }
    }
}
// out = a w^T + bias (+ r) (act), w [N, K]: the N / 32 column blocks over the four waves
__device__ __forceinline__ void xenc_linear(const float* a, int ld, int K, const float* __restrict__ w, const float* __restrict__ bias,
                                            int N, const float* r, int act, float* out, int nrb) {
    const int lane = mf_lane(), l31 = lane & 31, hh = lane >> 5;
    for (int cb = threadIdx.x >> 6; cb < N / 32; cb += 4) {
        f32x16 acc[2];
        xenc_zero(acc);
        xenc_mma(a, ld, w + (int64_t)(cb * 32 + l31) * K, K, nrb, l31, hh, acc);
        xenc_store(acc, nrb, cb * 32, bias, r, act, out, ld, l31, hh);
    }
}
// attention of the heads hd = wave, wave + 4, ..: xfmr_attn_kernel<DH, false>'s loop with K and V read in place; ctx -> q
template <int DH>
__device__ __forceinline__ void xenc_attention(float* q, const float* k, const float* v, int ld, int heads, int n, float* ps) {
    const int lane = mf_lane();
    for (int hd = threadIdx.x >> 6; hd < heads; hd += 4) {
        const int col0 = hd * DH;
        for (int i = 0; i < n; ++i) {
            const float qv = q[i * ld + col0 + (lane & (DH - 1))];              // (lanes >= DH: never read by xattn_prob)
            const float p = xattn_prob<DH>(qv, k + (lane < n ? lane : 0) * ld + col0, lane < n);
            xenc_wave_sync();
            ps[lane] = p;
            xenc_wave_sync();
            const float o = xattn_mix<DH>(ps, v + col0, ld, lane, n);
            if (lane < DH) q[i * ld + col0 + lane] = o;
        }
    }
}
// 32 lanes per row: rows [0, n) of z (row stride ld) -> LayerNorm in place, eight rows at a time (whole waves in the row sums)
template <int E>
__device__ __forceinline__ void xenc_layernorm(float* z, int ld, int n, const float* __restrict__ gamma, const float* __restrict__ beta) {
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const XRow<E> gm = xrow_load<E>(gamma, c), bt = xrow_load<E>(beta, c);
    for (int t0 = 0; t0 < n; t0 += 8) {
        const int t = t0 + g;
        float* row = z + t * ld;                                 // (t <= 63: a row past n is read for nothing)
        float mean, rstd;
        const XRow<E> y = xrow_layernorm<E>(xrow_load<E>(row, c), gm, bt, mean, rstd);
        if (t < n) xrow_store<E>(row, c, y);
    }
}

template <int H>
__global__ __launch_bounds__(256) void xfmr_encode_kernel(XEnc p) {
    constexpr int E = H / 32, S = H + XENC_PAD, BUF = XFMR_MAX_L * S;
    extern __shared__ __attribute__((aligned(16))) float xenc_lds[];
    float* const ps = xenc_lds + 4 * BUF + 64 * (threadIdx.x >> 6);          // the wave's 64 probabilities
    int64_t* const ids = reinterpret_cast<int64_t*>(xenc_lds + 4 * BUF + 4 * 64);
    int* const n_sh = reinterpret_cast<int*>(ids + XFMR_MAX_L);
    const int64_t b = blockIdx.x;
    const int lane = mf_lane(), wave = threadIdx.x >> 6;
    // ---- cut: list_cut_kernel<true>'s and xfmr_pack_kernel's walks for this user, on wave 0
    if (wave == 0) {
        int64_t lo, hi;
        list_clamp(p.seg_start[b], p.seg_end[b], p.n_items, lo, hi);
        int need;
        const int64_t cut = list_cut_walk(p.items, lo, hi, p.n_rows, p.L, need);
        list_pack_walk(p.items, cut, hi, p.n_rows, p.L - need, [&](int slot, long long id) { ids[slot] = id; });
        if (lane == 0) *n_sh = p.L - need;
    }
    __syncthreads();
    const int n = *n_sh;
    if (n <= 0) {                                                // (whole workgroup) an empty list: u = 0
        if (threadIdx.x < H) p.out_u[b * H + threadIdx.x] = 0.f;
        return;
    }
    const int nrb = n > 32 ? 2 : 1;
    float *bx = xenc_lds, *bq = xenc_lds + BUF, *bk = xenc_lds + 2 * BUF, *bv = xenc_lds + 3 * BUF;
    // ---- embed: xrow_embed, as xfmr_embed_kernel<H, false> calls it, eight tokens at a time
    {
        const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
        const XRow<E> te = xrow_load<E>(p.prm[1], c), gm = xrow_load<E>(p.prm[2], c), bt = xrow_load<E>(p.prm[3], c);
        for (int t0 = 0; t0 < n; t0 += 8) {
            const int t = t0 + g;
            const bool valid = t < n;
            const int tt = valid ? t : 0;
            XRow<E> z;
            float mean, rstd;
            const XRow<E> y = xrow_embed<E>(xrow_load<E>(p.table + ids[tt] * H, c), p.norm_item, te,
                                            xrow_load<E>(p.prm[0] + (int64_t)tt * H, c), gm, bt, z, mean, rstd);
            if (valid) xrow_store<E>(bx + t * S, c, y);
        }
    }
    __syncthreads();
    const int l31 = lane & 31, hh = lane >> 5, dh = H / p.heads;
    for (int l = 0; l < p.layers; ++l) {
        const float* const* w = p.prm + XFMR_GLOBALS + XFMR_PER_LAYER * l;
        // q, k, v: 3 H / 32 column blocks
        for (int j = wave; j < 3 * (H / 32); j += 4) {
            const int which = j / (H / 32), cb = j % (H / 32);
            f32x16 acc[2];
            xenc_zero(acc);
            xenc_mma(bx, S, w[2 * which] + (int64_t)(cb * 32 + l31) * H, H, nrb, l31, hh, acc);
            xenc_store(acc, nrb, cb * 32, w[2 * which + 1], nullptr, -1, which == 0 ? bq : which == 1 ? bk : bv, S, l31, hh);
        }
        __syncthreads();
        switch (dh) {
            case 8: xenc_attention<8>(bq, bk, bv, S, p.heads, n, ps); break;
            case 16: xenc_attention<16>(bq, bk, bv, S, p.heads, n, ps); break;
            case 32: xenc_attention<32>(bq, bk, bv, S, p.heads, n, ps); break;
            default:
                if constexpr (H >= 64) xenc_attention<64>(bq, bk, bv, S, p.heads, n, ps);
                break;
        }
        __syncthreads();
        xenc_linear(bq, S, H, w[6], w[7], H, bx, -1, bk, nrb);                 // z1 = ctx Wo^T + bo + x
        __syncthreads();
        xenc_layernorm<E>(bk, S, n, w[8], w[9]);                               // y1
        __syncthreads();
        f32x16 acc[2];                                                         // z2's column block `wave` (H / 32 <= 4 blocks)
        xenc_zero(acc);
        for (int c0 = 0; c0 < p.I; c0 += H) {
            const int ic = min(H, p.I - c0);
            xenc_linear(bk, S, H, w[10] + (int64_t)c0 * H, w[11] + c0, ic, nullptr, p.act, bq, nrb);   // f = act(y1 Wi^T + bi)
            __syncthreads();
            if (wave < H / 32) xenc_mma(bq, S, w[12] + (int64_t)(wave * 32 + l31) * p.I + c0, ic, nrb, l31, hh, acc);
            __syncthreads();
        }
        if (wave < H / 32) xenc_store(acc, nrb, wave * 32, w[13], bk, -1, bv, S, l31, hh);   // z2 = acc + bo2 + y1
        __syncthreads();
        xenc_layernorm<E>(bv, S, n, w[14], w[15]);                             // y2
        __syncthreads();
        float* const t = bx; bx = bv; bv = t;
    }
    // ---- pool: xrow_pool and xrow_normalize over the n rows, as xfmr_pool_kernel calls them, on one wave (both halves compute,
    // the lower one stores) -- the last one: wave 0's mask, made for the cut, would stay in two SGPRs across the whole kernel
    if (wave == 3) {
        XRow<E> pr = xrow_pool<E, false>(bx, S, lane & 31, n, p.mode, nullptr);
        xrow_normalize<E>(pr, p.norm_user);
        if (lane < 32) xrow_store<E>(p.out_u + b * H, lane & 31, pr);
    }
}

// ======================================================================================== host: layout ====
struct XfmrLayerStash {
    float *q, *k, *v, *ctx, *z1, *st1, *y1, *a, *f, *z2, *st2, *y2;
};
struct XfmrStash {
    int64_t *cut, *tok_off, *tok_item;
    int32_t *nb, *T_dev, *tok_user;
    float *z0, *st0, *x0;
    XfmrLayerStash layer[XFMR_MAX_LAYERS];
    size_t total;
};
static XfmrStash xfmr_stash(void* p, int64_t B, int64_t t_cap, int h, int layers, int I) {
    MfArena a(p);
    XfmrStash s;
    const size_t T = (size_t)(t_cap > 0 ? t_cap : 1);
    s.cut = a.take<int64_t>((size_t)B);
    s.nb = a.take<int32_t>((size_t)B);
    s.tok_off = a.take<int64_t>((size_t)B + 1);
    s.T_dev = a.take<int32_t>(1);
    s.tok_item = a.take<int64_t>(T);
    s.tok_user = a.take<int32_t>(T);
    s.z0 = a.take<float>(T * h);
    s.st0 = a.take<float>(T * 2);
    s.x0 = a.take<float>(T * h);
    for (int l = 0; l < layers; ++l) {
        XfmrLayerStash& y = s.layer[l];
        y.q = a.take<float>(T * h); y.k = a.take<float>(T * h); y.v = a.take<float>(T * h); y.ctx = a.take<float>(T * h);
        y.z1 = a.take<float>(T * h); y.st1 = a.take<float>(T * 2); y.y1 = a.take<float>(T * h);
        y.a = a.take<float>(T * I); y.f = a.take<float>(T * I);
        y.z2 = a.take<float>(T * h); y.st2 = a.take<float>(T * 2); y.y2 = a.take<float>(T * h);
    }
    s.total = a.used();
    return s;
}

static const char* xfmr_check_shape(int h, int layers, int heads, int I, int L) {
    if (h != 32 && h != 64 && h != 128) return "hidden size not in {32, 64, 128}";
    if (layers < 1 || layers > XFMR_MAX_LAYERS) return "num_hidden_layers not in 1..4";
    if (heads < 1 || h % heads) return "hidden size not a multiple of the heads";
    const int dh = h / heads;
    if (dh != 8 && dh != 16 && dh != 32 && dh != 64) return "head width not in {8, 16, 32, 64}";
    if (I < 32 || I % 32 || I > 4 * h) return "intermediate size not a multiple of 32 in [32, 4 h]";
    if (L < 1 || L > XFMR_MAX_L) return "max_history not in 1..64";
    return nullptr;
}
// What mf_xfmr_forward* and mf_xfmr_encode check alike, in this order, under the caller's name: the pointers and ranges, the
// shape, the table rows the coalesce covers and the users (and packed tokens; t_cap < 0: none are packed) an index can hold.
static int xfmr_check_inputs(const char* what, const float* table, int64_t n_rows, const int64_t* seg_start, const int64_t* seg_end,
                             const int64_t* items, int64_t n_items, int64_t B, int64_t t_cap, int h, int layers, int heads, int I, int L,
                             int act, int mode, const float* const* params, const float* out_u) {
    if (!table || !seg_start || !seg_end || !items || !params || !out_u || B <= 0 || n_rows <= 0 || n_items <= 0 || act < 0 || act > 3 ||
        mode < 0 || mode > 2)
        return mf_set_error(MF_EINVAL, "%s: bad argument", what);
    if (const char* why = xfmr_check_shape(h, layers, heads, I, L)) return mf_set_error(MF_ENOTSUP, "%s: %s", what, why);
    if (n_rows > COALESCE_MAX_ROWS) return mf_set_error(MF_ENOTSUP, "%s: %lld table rows > %d", what, (long long)n_rows, COALESCE_MAX_ROWS);
    if (t_cap >= (1ll << 31) || B >= (1ll << 31) / 64)
        return mf_set_error(MF_ENOTSUP, t_cap < 0 ? "%s: too many users" : "%s: too many tokens or users", what);
    return MF_OK;
}
// every entry point's last check, after its own space check: no parameter (grads: and no gradient) of the `layers` layers is null
static int xfmr_check_params(const char* what, const float* const* params, float* const* grads, int layers) {
    for (int i = 0; i < XFMR_GLOBALS + XFMR_PER_LAYER * layers; ++i)
        if (!params[i] || (grads && !grads[i]))
            return mf_set_error(MF_EINVAL, grads ? "%s: parameter or gradient %d is null" : "%s: parameter %d is null", what, i);
    return MF_OK;
}

extern "C" size_t mf_xfmr_ws_bytes(int64_t B, int64_t t_cap, int h, int layers, int I) {
    if (layers < 1 || layers > XFMR_MAX_LAYERS) return 0;
    return xfmr_stash(nullptr, B > 0 ? B : 1, t_cap, h, layers, I).total;
}

#define XFMR_DISPATCH_H(h, ...)                                  \
    switch (h) {                                                 \
        case 32: { constexpr int H = 32; __VA_ARGS__; } break;   \
        case 64: { constexpr int H = 64; __VA_ARGS__; } break;   \
        default: { constexpr int H = 128; __VA_ARGS__; } break;  \
    }
#define XFMR_DISPATCH_DH(dh, ...)                                \
    switch (dh) {                                                \
        case 8: { constexpr int DH = 8; __VA_ARGS__; } break;    \
        case 16: { constexpr int DH = 16; __VA_ARGS__; } break;  \
        case 32: { constexpr int DH = 32; __VA_ARGS__; } break;  \
        default: { constexpr int DH = 64; __VA_ARGS__; } break;  \
    }
// one dropout site: DROP = false launches the code the plain exports always ran, and the call hands it an XDrop{}
#define XFMR_DISPATCH_DROP(on, ...)                              \
    if (on) { constexpr bool DROP = true; __VA_ARGS__; }         \
    else { constexpr bool DROP = false; __VA_ARGS__; }

// prec: MF_XFMR_FP32 launches xfmr_gemm_kernel, as every call did before there was a choice; MF_XFMR_BF16_MIXED its bf16 sibling.
// dr: a linear (dyn = 0) whose result is dropped before its residual add names its site (dr.d.thr = 0: the plain kernel).
static void xfmr_gemm(hipStream_t s, int64_t t_cap, XGemm g, int prec, const XDropRows& dr = XDropRows{}) {
    const dim3 grid = g.dyn == 0 ? dim3((unsigned)((t_cap + 63) / 64), (unsigned)((g.N + 63) / 64))
                                 : dim3((unsigned)((g.M + 63) / 64), (unsigned)((g.N + 63) / 64), XFMR_SLICES);
    XFMR_DISPATCH_DROP(dr.d.thr != 0, {
        if (prec == MF_XFMR_BF16_MIXED) xfmr_gemm_bf16_kernel<DROP><<<grid, 256, 0, s>>>(g, DROP ? dr : XDropRows{});
        else xfmr_gemm_kernel<DROP><<<grid, 256, 0, s>>>(g, DROP ? dr : XDropRows{});
    });
}

// The dropout of one call: thresholds of the two probabilities (0 = off) and what the keys are made of.
struct XfmrDropout {
    unsigned thr_hidden, thr_attn;
    unsigned long long seed, call;
    XDrop site(unsigned thr, int stream) const { return XDrop{mf_dropout_key(seed, call, (unsigned long long)stream), thr, mf_dropout_scale(thr)}; }
    XDrop attn(int layer) const { return site(thr_attn, 4 * layer + 0); }
    XDrop attn_out(int layer) const { return site(thr_hidden, 4 * layer + 1); }
    XDrop ffn_out(int layer) const { return site(thr_hidden, 4 * layer + 2); }
    XDrop embeddings() const { return site(thr_hidden, 4 * XFMR_MAX_LAYERS); }
};
// thr = round(p * 65536) (halves up; at most 65535, so that the scale stays finite); false: p outside [0, 1)
static bool xfmr_drop_thr(double p, unsigned* thr) {
    if (!(p >= 0.0 && p < 1.0)) return false;
    const double t = floor(p * 65536.0 + 0.5);
    *thr = t > 65535.0 ? 65535u : (unsigned)t;
    return true;
}
static bool xfmr_dropout(double p_hidden, double p_attn, uint64_t seed, uint64_t call, XfmrDropout* d) {
    d->seed = seed;
    d->call = call;
    return xfmr_drop_thr(p_hidden, &d->thr_hidden) && xfmr_drop_thr(p_attn, &d->thr_attn);
}

extern "C" int mf_dropout_words(uint64_t seed, uint64_t call, uint64_t stream, uint64_t idx0, int64_t n, uint64_t* out) {
    if (!out || n < 0) return mf_set_error(MF_EINVAL, "mf_dropout_words: bad argument");
    const unsigned long long key = mf_dropout_key(seed, call, stream);
    for (int64_t i = 0; i < n; ++i) out[i] = mf_dropout_word(key, idx0 + (uint64_t)i);
    return MF_OK;
}
// Y [T, N] = X [T, K] W[N, K]^T + bias (+ R)
static XGemm xg_linear(const float* X, int K, const float* W, const float* bias, int N, float* Y, const float* R, const int32_t* T_dev) {
    XGemm g{};
    g.A = X; g.lda = K; g.a_kc = 1;
    g.B = W; g.ldb = K; g.b_kc = 1;
    g.C = Y; g.ldc = N; g.N = N; g.K = K; g.T_dev = T_dev; g.dyn = 0; g.bias = bias; g.R = R;
    return g;
}
// dX [T, K] = dY [T, N] W[N, K] (+ R)
static XGemm xg_dinput(const float* dY, int N, const float* W, int K, float* dX, const float* R, const int32_t* T_dev) {
    XGemm g{};
    g.A = dY; g.lda = N; g.a_kc = 1;
    g.B = W; g.ldb = K; g.b_kc = 0;
    g.C = dX; g.ldc = K; g.N = K; g.K = N; g.T_dev = T_dev; g.dyn = 0; g.R = R;
    return g;
}
// dW [N, K] = dY [T, N]^T X [T, K], db [N] = column sums of dY: XFMR_SLICES partials in `part`, then the ordered sum
static void xfmr_dweight(hipStream_t s, const float* dY, int N, const float* X, int K, float* dW, float* db, float* part,
                         const int32_t* T_dev, int prec) {
    XGemm g{};
    g.A = dY; g.lda = N; g.a_kc = 0;
    g.B = X; g.ldb = K; g.b_kc = 0;
    g.C = part; g.ldc = K; g.M = N; g.N = K; g.T_dev = T_dev; g.dyn = 1;
    g.slice_stride = (int64_t)N * K + N;
    xfmr_gemm(s, 0, g, prec);
    const int64_t size = g.slice_stride;
    xfmr_reduce_kernel<<<dim3((unsigned)((size + 255) / 256)), 256, 0, s>>>(part, XFMR_SLICES, size, (int64_t)N * K, dW, db);
}

// ============================================================================================= forward ====
static int xfmr_forward(const float* table, int64_t n_rows, int h, const int64_t* seg_start, const int64_t* seg_end,
                        const int64_t* items, int64_t n_items, int64_t B, int64_t t_cap, int max_history, int layers, int heads,
                        int intermediate, int act, int mode, int norm_item, int norm_user, const float* const* params,
                        float* out_u, float* out_inv, int32_t* out_arg, void* stash, size_t stash_bytes, const XfmrDropout& drop,
                        int prec, mf_stream_t stream) {
    if (prec != MF_XFMR_FP32 && prec != MF_XFMR_BF16_MIXED)
        return mf_set_error(MF_EINVAL, "mf_xfmr_forward: precision %d is neither MF_XFMR_FP32 nor MF_XFMR_BF16_MIXED", prec);
    if (!out_inv || !stash || t_cap < 0 || (mode == XPOOL_MAX && !out_arg)) return mf_set_error(MF_EINVAL, "mf_xfmr_forward: bad argument");
    if (int rc = xfmr_check_inputs("mf_xfmr_forward", table, n_rows, seg_start, seg_end, items, n_items, B, t_cap, h, layers, heads,
                                   intermediate, max_history, act, mode, params, out_u))
        return rc;
    if (stash_bytes < mf_xfmr_ws_bytes(B, t_cap, h, layers, intermediate)) return mf_set_error(MF_ENOSPC, "mf_xfmr_forward: stash too small");
    if (int rc = xfmr_check_params("mf_xfmr_forward", params, nullptr, layers)) return rc;
    const XfmrStash st = xfmr_stash(stash, B, t_cap, h, layers, intermediate);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int I = intermediate, dh = h / heads;
    const unsigned gu = (unsigned)((B + 3) / 4), gt = (unsigned)((t_cap + 7) / 8), ga = (unsigned)(B * heads);
    MF_TIMED("xfmr_forward", s, {
        list_cut_kernel<true><<<gu, 256, 0, s>>>(seg_start, seg_end, items, n_items, B, n_rows, max_history, st.cut, st.nb);
        xfmr_scan_kernel<<<1, 256, 0, s>>>(st.nb, B, t_cap, st.tok_off, st.T_dev);
        xfmr_pack_kernel<<<gu, 256, 0, s>>>(seg_end, st.cut, items, n_items, B, n_rows, st.tok_off, st.tok_item, st.tok_user);
        if (t_cap > 0) {
            XFMR_DISPATCH_DROP(drop.thr_hidden, XFMR_DISPATCH_H(h, xfmr_embed_kernel<H, DROP><<<gt, 256, 0, s>>>(
                                                       table, st.tok_item, st.tok_user, st.tok_off, st.T_dev, norm_item, params[0], params[1],
                                                       params[2], params[3], st.z0, st.st0, st.x0, DROP ? drop.embeddings() : XDrop{})));
            const float* x = st.x0;
            for (int l = 0; l < layers; ++l) {
                const float* const* w = params + XFMR_GLOBALS + XFMR_PER_LAYER * l;
                const XfmrLayerStash& y = st.layer[l];
                MF_TIMED("xfmr_gemm_fwd", s, {
                    xfmr_gemm(s, t_cap, xg_linear(x, h, w[0], w[1], h, y.q, nullptr, st.T_dev), prec);
                    xfmr_gemm(s, t_cap, xg_linear(x, h, w[2], w[3], h, y.k, nullptr, st.T_dev), prec);
                    xfmr_gemm(s, t_cap, xg_linear(x, h, w[4], w[5], h, y.v, nullptr, st.T_dev), prec);
                });
                MF_TIMED("xfmr_attn_fwd", s, XFMR_DISPATCH_DROP(drop.thr_attn, XFMR_DISPATCH_DH(dh, xfmr_attn_kernel<DH, DROP><<<ga, 64, 0, s>>>(
                                                 y.q, y.k, y.v, st.tok_off, h, heads, y.ctx, DROP ? drop.attn(l) : XDrop{}))));
                MF_TIMED("xfmr_gemm_fwd", s, xfmr_gemm(s, t_cap, xg_linear(y.ctx, h, w[6], w[7], h, y.z1, x, st.T_dev), prec,
                                                       XDropRows{drop.attn_out(l), st.tok_user, st.tok_off}));
                XFMR_DISPATCH_H(h, xfmr_ln_kernel<H><<<gt, 256, 0, s>>>(y.z1, st.T_dev, w[8], w[9], y.y1, y.st1));
                MF_TIMED("xfmr_gemm_fwd", s, {
                    XGemm g = xg_linear(y.y1, h, w[10], w[11], I, y.a, nullptr, st.T_dev);
                    g.epi = XEPI_ACT; g.act = act; g.C2 = y.f;
                    xfmr_gemm(s, t_cap, g, prec);
                    xfmr_gemm(s, t_cap, xg_linear(y.f, I, w[12], w[13], h, y.z2, y.y1, st.T_dev), prec,
                              XDropRows{drop.ffn_out(l), st.tok_user, st.tok_off});
                });
                XFMR_DISPATCH_H(h, xfmr_ln_kernel<H><<<gt, 256, 0, s>>>(y.z2, st.T_dev, w[14], w[15], y.y2, y.st2));
                x = y.y2;
            }
        }
        const float* last = t_cap > 0 ? st.layer[layers - 1].y2 : st.x0;
        XFMR_DISPATCH_H(h, xfmr_pool_kernel<H><<<dim3((unsigned)((B + 7) / 8)), 256, 0, s>>>(last, st.tok_off, B, mode, norm_user, out_u,
                                                                                            out_inv, out_arg));
    });
    return mf_check_launch("mf_xfmr_forward");
}

extern "C" int mf_xfmr_forward(const float* table, int64_t n_rows, int h, const int64_t* seg_start, const int64_t* seg_end,
                               const int64_t* items, int64_t n_items, int64_t B, int64_t t_cap, int max_history, int layers, int heads,
                               int intermediate, int act, int mode, int norm_item, int norm_user, const float* const* params,
                               float* out_u, float* out_inv, int32_t* out_arg, void* stash, size_t stash_bytes, mf_stream_t stream) {
    return xfmr_forward(table, n_rows, h, seg_start, seg_end, items, n_items, B, t_cap, max_history, layers, heads, intermediate, act, mode,
                        norm_item, norm_user, params, out_u, out_inv, out_arg, stash, stash_bytes, XfmrDropout{}, MF_XFMR_FP32, stream);
}
extern "C" int mf_xfmr_forward_dropout(const float* table, int64_t n_rows, int h, const int64_t* seg_start, const int64_t* seg_end,
                                       const int64_t* items, int64_t n_items, int64_t B, int64_t t_cap, int max_history, int layers,
                                       int heads, int intermediate, int act, int mode, int norm_item, int norm_user,
                                       const float* const* params, float* out_u, float* out_inv, int32_t* out_arg, void* stash,
                                       size_t stash_bytes, double p_hidden, double p_attn, uint64_t seed, uint64_t call,
                                       mf_stream_t stream) {
    return mf_xfmr_forward_mixed(table, n_rows, h, seg_start, seg_end, items, n_items, B, t_cap, max_history, layers, heads, intermediate, act,
                                 mode, norm_item, norm_user, params, out_u, out_inv, out_arg, stash, stash_bytes, p_hidden, p_attn, seed, call,
                                 MF_XFMR_FP32, stream);
}
extern "C" int mf_xfmr_forward_mixed(const float* table, int64_t n_rows, int h, const int64_t* seg_start, const int64_t* seg_end,
                                     const int64_t* items, int64_t n_items, int64_t B, int64_t t_cap, int max_history, int layers,
                                     int heads, int intermediate, int act, int mode, int norm_item, int norm_user,
                                     const float* const* params, float* out_u, float* out_inv, int32_t* out_arg, void* stash,
                                     size_t stash_bytes, double p_hidden, double p_attn, uint64_t seed, uint64_t call, int precision,
                                     mf_stream_t stream) {
    XfmrDropout drop;
    if (!xfmr_dropout(p_hidden, p_attn, seed, call, &drop))
        return mf_set_error(MF_EINVAL, "mf_xfmr_forward_dropout: dropout probabilities must be in [0, 1): %g, %g", p_hidden, p_attn);
    return xfmr_forward(table, n_rows, h, seg_start, seg_end, items, n_items, B, t_cap, max_history, layers, heads, intermediate, act, mode,
                        norm_item, norm_user, params, out_u, out_inv, out_arg, stash, stash_bytes, drop, precision, stream);
}

// one launch, one workgroup per user: no t_cap, no stash, no host read; everything below is decided before any GPU call
extern "C" int mf_xfmr_encode(const float* table, int64_t n_rows, int h, const int64_t* seg_start, const int64_t* seg_end,
                              const int64_t* items, int64_t n_items, int64_t B, int max_history, int layers, int heads,
                              int intermediate, int act, int mode, int norm_item, int norm_user, const float* const* params,
                              float* out_u, mf_stream_t stream) {
    if (int rc = xfmr_check_inputs("mf_xfmr_encode", table, n_rows, seg_start, seg_end, items, n_items, B, -1, h, layers, heads,
                                   intermediate, max_history, act, mode, params, out_u))
        return rc;
    if (int rc = xfmr_check_params("mf_xfmr_encode", params, nullptr, layers)) return rc;
    XEnc p{};
    for (int i = 0; i < XFMR_GLOBALS + XFMR_PER_LAYER * layers; ++i) p.prm[i] = params[i];
    p.table = table; p.n_rows = n_rows; p.seg_start = seg_start; p.seg_end = seg_end; p.items = items; p.n_items = n_items;
    p.L = max_history; p.layers = layers; p.heads = heads; p.I = intermediate; p.act = act; p.mode = mode;
    p.norm_item = norm_item; p.norm_user = norm_user; p.out_u = out_u;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = xenc_lds_bytes(h);
    MF_TIMED("xfmr_encode", s, {
        XFMR_DISPATCH_H(h, {
            auto fn = xfmr_encode_kernel<H>;
            if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            fn<<<dim3((unsigned)B), 256, lds, s>>>(p);
        });
    });
    return mf_check_launch("mf_xfmr_encode");
}

// ============================================================================================ backward ====
struct XfmrBwdWs {
    float *dy, *dz, *dt, *dctx, *dq, *dk, *dv, *di, *part;
    float* dzm;                 // hidden dropout only: mask * dz, the operand of a dropped dense's backward
    size_t total;
};
// the largest set of partials: XFMR_SLICES slices of a weight gradient with its bias gradient -- [I, h] + I, [h, I] + h, and the
// attention's [h, h] + h, which is the largest one when I < h
static size_t xfmr_part_floats(int h, int I) {
    const size_t widest = (size_t)(I > h ? I : h);
    size_t m = (size_t)XFMR_SLICES * (widest * h + widest);
    const size_t ln = (size_t)XFMR_LN_SLICES * 2 * h, ps = (size_t)XFMR_POS_SLICES * XFMR_MAX_L * h;
    if (ln > m) m = ln;
    if (ps > m) m = ps;
    return m;
}
static XfmrBwdWs xfmr_bwd_ws(void* p, int64_t t_cap, int h, int I, bool dropout = false) {
    MfArena a(p);
    XfmrBwdWs w;
    const size_t T = (size_t)(t_cap > 0 ? t_cap : 1);
    w.dy = a.take<float>(T * h); w.dz = a.take<float>(T * h); w.dt = a.take<float>(T * h); w.dctx = a.take<float>(T * h);
    w.dq = a.take<float>(T * h); w.dk = a.take<float>(T * h); w.dv = a.take<float>(T * h);
    w.di = a.take<float>(T * I);
    w.part = a.take<float>(xfmr_part_floats(h, I));
    w.dzm = dropout ? a.take<float>(T * h) : w.dz;
    w.total = a.used();
    return w;
}
extern "C" size_t mf_xfmr_backward_ws_bytes(int64_t t_cap, int h, int I) { return xfmr_bwd_ws(nullptr, t_cap, h, I).total; }
extern "C" size_t mf_xfmr_backward_dropout_ws_bytes(int64_t t_cap, int h, int I) { return xfmr_bwd_ws(nullptr, t_cap, h, I, true).total; }

// kind: XLN_DROP_*; d.thr = 0 runs the plain kernel whatever the kind (then the caller's dzm is dz)
template <int H>
static void xfmr_ln_bwd(hipStream_t s, const float* dy, const float* z, const float* st, const int32_t* T_dev, const float* gamma,
                        float* dz, float* part, float* dgamma, float* dbeta, int kind = XLN_DROP_NONE, const XDrop& d = XDrop{},
                        const int32_t* tok_user = nullptr, const int64_t* tok_off = nullptr, float* dzm = nullptr) {
    if (d.thr == 0 || kind == XLN_DROP_NONE)
        xfmr_ln_bwd_kernel<H, XLN_DROP_NONE><<<XFMR_LN_SLICES, 256, 0, s>>>(dy, z, st, T_dev, gamma, dz, part, nullptr, nullptr, XDrop{}, nullptr);
    else if (kind == XLN_DROP_IN)
        xfmr_ln_bwd_kernel<H, XLN_DROP_IN><<<XFMR_LN_SLICES, 256, 0, s>>>(dy, z, st, T_dev, gamma, dz, part, tok_user, tok_off, d, nullptr);
    else
        xfmr_ln_bwd_kernel<H, XLN_DROP_OUT><<<XFMR_LN_SLICES, 256, 0, s>>>(dy, z, st, T_dev, gamma, dz, part, tok_user, tok_off, d, dzm);
    xfmr_reduce_kernel<<<dim3((2 * H + 255) / 256), 256, 0, s>>>(part, XFMR_LN_SLICES, 2 * H, H, dgamma, dbeta);
}

// grads: one buffer per parameter, in the parameters' order and shapes; every element is written (no accumulation).
// grad_x [t_cap, h] receives dL/dx_t of the packed tokens (the rows mf_xfmr_coalesce lands on the item table).
static int xfmr_backward(int h, int64_t B, int64_t t_cap, int max_history, int max_pos, int layers, int heads, int intermediate,
                         int act, int mode, int norm_user, const float* const* params, float* const* grads, const void* stash,
                         const float* grad_u, const float* out_u, const float* out_inv, const int32_t* out_arg, float* grad_x,
                         void* ws, size_t ws_bytes, const XfmrDropout& drop, bool dropout_ws, int prec, mf_stream_t stream) {
    if (prec != MF_XFMR_FP32 && prec != MF_XFMR_BF16_MIXED)
        return mf_set_error(MF_EINVAL, "mf_xfmr_backward: precision %d is neither MF_XFMR_FP32 nor MF_XFMR_BF16_MIXED", prec);
    if (!params || !grads || !stash || !grad_u || !out_u || !out_inv || !grad_x || !ws || B <= 0 || t_cap <= 0 || act < 0 || act > 3 ||
        mode < 0 || mode > 2 || (mode == XPOOL_MAX && !out_arg) || max_pos < max_history)
        return mf_set_error(MF_EINVAL, "mf_xfmr_backward: bad argument");
    if (const char* why = xfmr_check_shape(h, layers, heads, intermediate, max_history))
        return mf_set_error(MF_ENOTSUP, "mf_xfmr_backward: %s", why);
    if (ws_bytes < xfmr_bwd_ws(nullptr, t_cap, h, intermediate, dropout_ws).total)
        return mf_set_error(MF_ENOSPC, "mf_xfmr_backward: workspace too small");
    if (int rc = xfmr_check_params("mf_xfmr_backward", params, grads, layers)) return rc;
    const XfmrStash st = xfmr_stash(const_cast<void*>(stash), B, t_cap, h, layers, intermediate);
    const XfmrBwdWs w = xfmr_bwd_ws(ws, t_cap, h, intermediate, dropout_ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int I = intermediate, dh = h / heads, L = max_history;
    float* const dzm = drop.thr_hidden ? w.dzm : w.dz;      // what a dropped dense's backward reads (the residual path reads dz)
    const unsigned gt = (unsigned)((t_cap + 7) / 8), ga = (unsigned)(B * heads);
    const int32_t* Td = st.T_dev;
    MF_TIMED("xfmr_backward", s, {
        XFMR_DISPATCH_H(h, xfmr_pool_bwd_kernel<H><<<gt, 256, 0, s>>>(grad_u, out_u, out_inv, out_arg, st.tok_off, st.tok_user, Td, mode,
                                                                     norm_user, w.dy));
        for (int l = layers - 1; l >= 0; --l) {
            const float* const* p = params + XFMR_GLOBALS + XFMR_PER_LAYER * l;
            float* const* g = grads + XFMR_GLOBALS + XFMR_PER_LAYER * l;
            const XfmrLayerStash& y = st.layer[l];
            const float* x = l == 0 ? st.x0 : st.layer[l - 1].y2;
            // output block: y2 = LN(z2), z2 = drop(f Wo2^T + bo2) + y1
            XFMR_DISPATCH_H(h, xfmr_ln_bwd<H>(s, w.dy, y.z2, y.st2, Td, p[14], w.dz, w.part, g[14], g[15], XLN_DROP_OUT, drop.ffn_out(l),
                                              st.tok_user, st.tok_off, dzm));
            MF_TIMED("xfmr_gemm_bwd", s, {
                xfmr_dweight(s, dzm, h, y.f, I, g[12], g[13], w.part, Td, prec);
                XGemm d = xg_dinput(dzm, h, p[12], I, w.di, nullptr, Td);         // da = (mask dz2 Wo2) * act'(a)
                d.epi = XEPI_DACT; d.act = act; d.P = y.a;
                xfmr_gemm(s, t_cap, d, prec);
                xfmr_dweight(s, w.di, I, y.y1, h, g[10], g[11], w.part, Td, prec);
                xfmr_gemm(s, t_cap, xg_dinput(w.di, I, p[10], h, w.dt, w.dz, Td), prec);  // dy1 = da Wi + dz2
            });
            // attention block: y1 = LN(z1), z1 = drop(ctx Wo^T + bo) + x
            XFMR_DISPATCH_H(h, xfmr_ln_bwd<H>(s, w.dt, y.z1, y.st1, Td, p[8], w.dz, w.part, g[8], g[9], XLN_DROP_OUT, drop.attn_out(l),
                                              st.tok_user, st.tok_off, dzm));
            MF_TIMED("xfmr_gemm_bwd", s, {
                xfmr_dweight(s, dzm, h, y.ctx, h, g[6], g[7], w.part, Td, prec);
                xfmr_gemm(s, t_cap, xg_dinput(dzm, h, p[6], h, w.dctx, nullptr, Td), prec);
            });
            MF_TIMED("xfmr_attn_bwd", s, XFMR_DISPATCH_DROP(drop.thr_attn, XFMR_DISPATCH_DH(dh, xfmr_attn_bwd_kernel<DH, DROP><<<ga, 64, 0, s>>>(
                                             y.q, y.k, y.v, w.dctx, st.tok_off, h, heads, w.dq, w.dk, w.dv, DROP ? drop.attn(l) : XDrop{}))));
            MF_TIMED("xfmr_gemm_bwd", s, {
                xfmr_dweight(s, w.dq, h, x, h, g[0], g[1], w.part, Td, prec);
                xfmr_dweight(s, w.dk, h, x, h, g[2], g[3], w.part, Td, prec);
                xfmr_dweight(s, w.dv, h, x, h, g[4], g[5], w.part, Td, prec);
                xfmr_gemm(s, t_cap, xg_dinput(w.dq, h, p[0], h, w.dy, w.dz, Td), prec);   // dx = dz1 + dq Wq + dk Wk + dv Wv
                xfmr_gemm(s, t_cap, xg_dinput(w.dk, h, p[2], h, w.dy, w.dy, Td), prec);
                xfmr_gemm(s, t_cap, xg_dinput(w.dv, h, p[4], h, w.dy, w.dy, Td), prec);
            });
        }
        // embeddings: x0 = drop(LN(z0)), z0 = (x + tok[0]) + pos[t]
        XFMR_DISPATCH_H(h, xfmr_ln_bwd<H>(s, w.dy, st.z0, st.st0, Td, params[2], grad_x, w.part, grads[2], grads[3], XLN_DROP_IN,
                                          drop.embeddings(), st.tok_user, st.tok_off));
        mf_zero_async(grads[0], (size_t)max_pos * h * sizeof(float), s);
        xfmr_pos_bwd_kernel<<<dim3((unsigned)L, XFMR_POS_SLICES), 128, 0, s>>>(grad_x, st.tok_off, B, h, L, w.part);
        xfmr_reduce_kernel<<<dim3((unsigned)(((int64_t)L * h + 255) / 256)), 256, 0, s>>>(w.part, XFMR_POS_SLICES, (int64_t)L * h,
                                                                                         (int64_t)L * h, grads[0], grads[0]);
        xfmr_tok_bwd_kernel<<<1, 128, 0, s>>>(grads[0], h, L, grads[1]);
    });
    return mf_check_launch("mf_xfmr_backward");
}

extern "C" int mf_xfmr_backward(int h, int64_t B, int64_t t_cap, int max_history, int max_pos, int layers, int heads, int intermediate,
                                int act, int mode, int norm_user, const float* const* params, float* const* grads, const void* stash,
                                const float* grad_u, const float* out_u, const float* out_inv, const int32_t* out_arg, float* grad_x,
                                void* ws, size_t ws_bytes, mf_stream_t stream) {
    return xfmr_backward(h, B, t_cap, max_history, max_pos, layers, heads, intermediate, act, mode, norm_user, params, grads, stash, grad_u,
                         out_u, out_inv, out_arg, grad_x, ws, ws_bytes, XfmrDropout{}, false, MF_XFMR_FP32, stream);
}
extern "C" int mf_xfmr_backward_dropout(int h, int64_t B, int64_t t_cap, int max_history, int max_pos, int layers, int heads,
                                        int intermediate, int act, int mode, int norm_user, const float* const* params,
                                        float* const* grads, const void* stash, const float* grad_u, const float* out_u,
                                        const float* out_inv, const int32_t* out_arg, float* grad_x, void* ws, size_t ws_bytes,
                                        double p_hidden, double p_attn, uint64_t seed, uint64_t call, mf_stream_t stream) {
    return mf_xfmr_backward_mixed(h, B, t_cap, max_history, max_pos, layers, heads, intermediate, act, mode, norm_user, params, grads, stash,
                                  grad_u, out_u, out_inv, out_arg, grad_x, ws, ws_bytes, p_hidden, p_attn, seed, call, MF_XFMR_FP32, stream);
}
extern "C" int mf_xfmr_backward_mixed(int h, int64_t B, int64_t t_cap, int max_history, int max_pos, int layers, int heads,
                                      int intermediate, int act, int mode, int norm_user, const float* const* params,
                                      float* const* grads, const void* stash, const float* grad_u, const float* out_u,
                                      const float* out_inv, const int32_t* out_arg, float* grad_x, void* ws, size_t ws_bytes,
                                      double p_hidden, double p_attn, uint64_t seed, uint64_t call, int precision, mf_stream_t stream) {
    XfmrDropout drop;
    if (!xfmr_dropout(p_hidden, p_attn, seed, call, &drop))
        return mf_set_error(MF_EINVAL, "mf_xfmr_backward_dropout: dropout probabilities must be in [0, 1): %g, %g", p_hidden, p_attn);
    return xfmr_backward(h, B, t_cap, max_history, max_pos, layers, heads, intermediate, act, mode, norm_user, params, grads, stash, grad_u,
                         out_u, out_inv, out_arg, grad_x, ws, ws_bytes, drop, true, precision, stream);
}

// =============================================================================================== dense ====
// ONE dense operation of the engine on the caller's buffers, through the tower's launch helpers: what holds the engine to its
// arithmetic contract without an encoder around it.  Workspace: the token count the kernels read, then (form 2) the partials.
struct XfmrDenseWs {
    int32_t* T_dev;
    float* part;
    size_t total;
};
static XfmrDenseWs xfmr_dense_ws(void* p, int form, int N, int K) {
    MfArena a(p);
    XfmrDenseWs w;
    w.T_dev = a.take<int32_t>(1);
    w.part = form == 2 ? a.take<float>((size_t)XFMR_SLICES * ((size_t)N * K + N)) : nullptr;
    w.total = a.used();
    return w;
}
static bool xfmr_dense_shape(int form, int N, int K) {
    return form >= 0 && form <= 2 && N >= 32 && N <= 512 && N % 32 == 0 && K >= 32 && K <= 512 && K % 32 == 0;
}
extern "C" size_t mf_xfmr_dense_ws_bytes(int form, int N, int K) {
    return xfmr_dense_shape(form, N, K) ? xfmr_dense_ws(nullptr, form, N, K).total : 0;
}
extern "C" int mf_xfmr_dense(int form, int precision, int64_t M, int N, int K, const float* a, const float* b, const float* bias,
                             float* out, float* out_bias, void* ws, size_t ws_bytes, mf_stream_t stream) {
    if (form < 0 || form > 2) return mf_set_error(MF_EINVAL, "mf_xfmr_dense: form %d not in 0..2", form);
    if (precision != MF_XFMR_FP32 && precision != MF_XFMR_BF16_MIXED)
        return mf_set_error(MF_EINVAL, "mf_xfmr_dense: precision %d is neither MF_XFMR_FP32 nor MF_XFMR_BF16_MIXED", precision);
    if (!a || !b || !out || !ws || (form == 2 && !out_bias) || M < 1 || M >= (1ll << 31))
        return mf_set_error(MF_EINVAL, "mf_xfmr_dense: bad argument");
    if (!xfmr_dense_shape(form, N, K)) return mf_set_error(MF_ENOTSUP, "mf_xfmr_dense: N = %d, K = %d not multiples of 32 in [32, 512]", N, K);
    if (ws_bytes < xfmr_dense_ws(nullptr, form, N, K).total) return mf_set_error(MF_ENOSPC, "mf_xfmr_dense: workspace too small");
    const XfmrDenseWs w = xfmr_dense_ws(ws, form, N, K);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w.T_dev), (int)M, 1, s) != hipSuccess) return mf_check_launch("mf_xfmr_dense");
    if (form == 0) xfmr_gemm(s, M, xg_linear(a, K, b, bias, N, out, nullptr, w.T_dev), precision);
    else if (form == 1) xfmr_gemm(s, M, xg_dinput(a, N, b, K, out, nullptr, w.T_dev), precision);
    else xfmr_dweight(s, a, N, b, K, out, out_bias, w.part, w.T_dev, precision);
    return mf_check_launch("mf_xfmr_dense");
}

// ============================================================================================ coalesce ====
// every packed token is an entry: its key is its item id, its row dL/dx_t
struct XfmrEntries {
    const int64_t* tok_item;
    int64_t n_rows;
    const float* grad_x;
    __device__ __forceinline__ uint32_t key(int64_t, int64_t pos) const {
        const long long id = tok_item[pos];
        return list_valid(id, n_rows) ? (uint32_t)id : (uint32_t)n_rows;
    }
    template <int D>
    __device__ __forceinline__ f32x4 grad(int64_t, int64_t t, int c) const {
        return reinterpret_cast<const f32x4*>(grad_x + t * D)[c];
    }
};

extern "C" size_t mf_xfmr_coalesce_ws_bytes(int64_t n_extra, int64_t t_cap, int d) {
    return coalesce_ws_bytes(n_extra, t_cap, d);
}

extern "C" int mf_xfmr_coalesce(int64_t n_rows, int d, int64_t B, int64_t t_cap, int layers, int intermediate, const void* stash,
                                const float* grad_x, const int64_t* extra_ids, const float* extra_grad, int64_t n_extra,
                                int64_t capacity, int64_t* out_ids, float* out_grad, void* ws, size_t ws_bytes, mf_stream_t stream) {
    if (!stash || !grad_x || !out_ids || !out_grad || B <= 0 || layers < 1 || layers > XFMR_MAX_LAYERS)
        return mf_set_error(MF_EINVAL, "mf_xfmr_coalesce: bad argument");
    if (d != 32 && d != 64 && d != 128) return mf_set_error(MF_EINVAL, "mf_xfmr_coalesce: width %d not in {32,64,128}", d);
    if (int rc = coalesce_check("mf_xfmr_coalesce", "table", n_rows, n_extra, extra_ids, extra_grad, t_cap, capacity, ws, ws_bytes,
                                coalesce_ws_bytes(n_extra, t_cap, d)))
        return rc;
    if (n_extra + t_cap == 0) return MF_OK;
    const XfmrStash st = xfmr_stash(const_cast<void*>(stash), B, t_cap, d, layers, intermediate);
    MfArena a(ws);
    const CoalesceWs w = coalesce_ws(a, n_extra, t_cap, d);
    const CoalesceSrc src{n_rows, extra_ids, extra_grad, n_extra, st.tok_off, st.tok_off, B, t_cap};
    const XfmrEntries ent{st.tok_item, n_rows, grad_x};
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    MF_TIMED("xfmr_coalesce", s, rc = coalesce(src, ent, w, d, capacity, out_ids, out_grad, nullptr, s));
    return rc ? rc : mf_check_launch("mf_xfmr_coalesce");
}
