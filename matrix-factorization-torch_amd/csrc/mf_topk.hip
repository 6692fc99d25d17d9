// mf_topk.hip -- exact brute-force full-catalog top-k (retrieval), gfx950.
//
// Replaces ItemProcessor.search (xfmr_rec/data/lightning.py:237-259, LanceDB cosine
// ANN + prefilter) by an exact scan: score tiles from the fp32 MFMA engine, streaming
// per-query selection (mf_select.h), exclusion lists scattered once into a
// bitmask (one coalesced word per query and tile), then an exact ordered merge per query.
// One merge kernel joins the partial top-k of a row-sharded catalog, from (scores, rows) or from
// the packed exchange form (mf_topk_merge, mf_topk_merge_packed: k <= 64); a second one ranks every entry by binary searches over
// the other lists instead of selecting k times, for lists up to k = 1024 (mf_topk_merge_deep, mf_topk_merge_packed_deep); one
// metrics kernel serves every k.
// Argument checks and the result store are shared with the other engines: mf_topk_io.h.
#include <cmath>

#include "mf_common.h"
#include <vector>

#include "mf_select.h"
#include "mf_topk_io.h"

// Exclusion prefilter as a bitmask: exclW[tile][query] holds the 32 "excluded" bits of
// that query for that item tile (the lists are sparse -- ~10^2 of 10^4..10^8 rows --
// so the words are scattered once per call and read with one coalesced load per tile).
struct RetrievalPolicy {
    struct Params {
        const uint32_t* exclW;     // [NT][Qp], all zero when nothing is excluded
        int64_t Qp, nY;
    };
    struct Row {};
    struct Tile {
        uint32_t ew;
    };
    static constexpr int AUX_DMA = 1;
    // the rank is mf_orderable(score): monotone in the raw score, so the bound is one float (NaN and signed
    // zeros pass: conservative)
    struct Thr {
        float f;
    };
    static __device__ __forceinline__ Thr thr_all() { return Thr{__builtin_bit_cast(float, 0xFFFFFFFFu)}; }   // NaN: nothing is below it
    static __device__ __forceinline__ Thr thr_none() { return Thr{__builtin_inff()}; }
    static __device__ __forceinline__ Thr make_thr(unsigned bound) { return Thr{mf_unorderable(bound)}; }
    static __device__ __forceinline__ bool maybe(const Params&, const Row&, const Tile&, float score, int, int, const Thr& t) {
        return !(score < t.f);
    }
    static __device__ __forceinline__ void stage_aux(const Params& p, char* aux, int wave, int t, int64_t x0, int) {
        mf_stage_small(aux + wave * 128, p.exclW + (int64_t)t * p.Qp + x0, 128);
    }
    static __device__ __forceinline__ Row row_init(const Params&, int64_t, bool) { return Row{}; }
    static __device__ __forceinline__ Tile tile_init(const Params&, const Row&, const char* aux, int wave, int c, int, int) {
        return Tile{reinterpret_cast<const uint32_t*>(aux + wave * 128)[c]};
    }
    static __device__ __forceinline__ bool key(const Params& p, const Row&, const Tile& t, float score, int e, int h,
                                               unsigned y, unsigned& hi, unsigned& lo) {
        hi = mf_key_retrieval_hi(score);
        lo = mf_key_retrieval_lo(y);
        return !((t.ew >> mf_acc_row(e, h)) & 1u) && y < (unsigned)p.nY;
    }
};

__global__ __launch_bounds__(256) void excl_scatter_kernel(const int64_t* __restrict__ excl_off,
                                                           const int64_t* __restrict__ excl_idx, int64_t idx_base,
                                                           int64_t N, int64_t Qp, uint32_t* __restrict__ exclW) {
    const int64_t r = blockIdx.x;
    for (int64_t e = excl_off[r] + threadIdx.x; e < excl_off[r + 1]; e += 256) {
        const int64_t y = excl_idx[e] - idx_base;
        if (y >= 0 && y < N) atomicOr(&exclW[(y >> 5) * Qp + r], 1u << (y & 31));
    }
}

struct TopkWs {
    SelectPlan plan;
    int NT;
    unsigned long long* cand;
    unsigned long long* priv;
    unsigned long long* seeds;
    int32_t* cand_cnt;
    uint32_t* exclW;
    unsigned* gtau;      // gtau and cand_cnt sit right behind exclW: one memset clears all three
    size_t total;
};

static TopkWs topk_ws(void* base, int64_t Q, int64_t N, int d, int k) {
    TopkWs w{};
    w.plan = mf_select_plan(Q, N, d, k);
    w.NT = (int)((N + 31) / 32);
    MfArena a(base);
    w.cand = a.take<unsigned long long>((size_t)w.plan.Xp * w.plan.rowcap);
    w.priv = a.take<unsigned long long>((size_t)w.plan.nsets * w.plan.Xp * w.plan.CAP);
    w.seeds = a.take<unsigned long long>((size_t)w.plan.Xp * (w.plan.seeds_per_row > 0 ? w.plan.seeds_per_row : 1));
    w.exclW = a.take<uint32_t>((size_t)w.NT * w.plan.Xp);
    w.gtau = a.take<unsigned>((size_t)w.plan.Xp);
    w.cand_cnt = a.take<int32_t>((size_t)w.plan.Xp);
    w.total = a.used();
    return w;
}

extern "C" size_t mf_topk_ws_bytes(int64_t Q, int64_t N, int d, int k) {
    if (Q <= 0 || N <= 0 || k <= 0 || !mf_width_ok(d)) return 0;
    return topk_ws(nullptr, Q, N, d, k).total;
}

// host-only geometry query (tests, sizing): how mf_topk would cut a catalog for Q queries
extern "C" int mf_topk_chunks(int64_t Q, int64_t N, int d, int k, int64_t* rows_per_chunk) {
    if (Q <= 0 || N <= 0 || k <= 0 || !mf_width_ok(d)) return 0;
    const SelectPlan pl = mf_select_plan(Q, N, d, k);
    if (!pl.ok) return 0;
    if (rows_per_chunk) *rows_per_chunk = (int64_t)pl.tpc * 32;
    return pl.nchunk;
}

// one wave per query: the row's candidate list -> ordered top-k
__global__ __launch_bounds__(64) void topk_merge_cand_kernel(const unsigned long long* __restrict__ cand,
                                                             const int32_t* __restrict__ cand_cnt, int rowcap, int k,
                                                             int64_t idx_base, float* __restrict__ out_scores,
                                                             int64_t* __restrict__ out_idx) {
    __shared__ unsigned long long win[64], sorted[64];
    const int64_t r = blockIdx.x;
    const int m = mf_row_topk<8>(cand + r * (int64_t)rowcap, cand_cnt[r], k, win, sorted);
    const int t = mf_lane();
    if (t < k) {
        if (t < m) mf_store_topk_entry(out_scores, out_idx, r, k, t, sorted[t], idx_base);
        else mf_store_topk_none(out_scores, out_idx, r, k, t);
    }
}

// merge of G already-ordered partial results with GLOBAL indices (< 2^32); load(entry) gives the entry's key, 0 for none
struct MergeParts {                     // (scores, rows), -1 for none
    const float* ps;
    const int64_t* pi;
    __device__ unsigned long long operator()(int64_t at) const { return pi[at] >= 0 ? mf_key_retrieval(ps[at], (unsigned)pi[at]) : 0ull; }
    // the same in two steps, for a kernel that keeps several entries' loads in flight before it looks at any (the deep merge:
    // both words are loaded whatever the row says; operator() stays as topk_merge_kernel was compiled with it)
    struct Raw {
        float s;
        int64_t i;
    };
    __device__ Raw raw(int64_t at) const { return Raw{ps[at], pi[at]}; }
    static __device__ unsigned long long key(const Raw& v) { return v.i >= 0 ? mf_key_retrieval(v.s, (unsigned)v.i) : 0ull; }
};
struct MergePacked {                    // the packed form of mf_topk_io.h: what topk_pack_kernel below and the cell scans write
    const int64_t* packed;
    __device__ unsigned long long operator()(int64_t at) const { return mf_packed_key(packed[at]); }
    using Raw = int64_t;
    __device__ Raw raw(int64_t at) const { return packed[at]; }
    static __device__ unsigned long long key(Raw v) { return mf_packed_key(v); }
};
template <class Load>
__global__ __launch_bounds__(64) void topk_merge_kernel(Load load, int G, int64_t Q, int k, float* __restrict__ out_scores,
                                                        int64_t* __restrict__ out_idx) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_keys[];
    const int64_t r = blockIdx.x;
    const int lane = mf_lane();
    const int total = G * k;
    for (int t = lane; t < total; t += 64) {
        const int g = t / k, e = t % k;
        s_keys[t] = load(((int64_t)g * Q + r) * k + e);
    }
    __syncthreads();
    mf_wave_select(s_keys, total, k, [&](int t, unsigned long long key) { mf_store_topk(out_scores, out_idx, r, k, t, key, 0); });
}
template <class Load>
static int topk_merge_launch(const char* who, Load load, int G, int64_t Q, int k, float* out_scores, int64_t* out_idx, mf_stream_t stream) {
    if ((size_t)G * k * 8 > 64 * 1024) return mf_set_error(MF_ENOTSUP, "%s: G * k too large", who);       // the keys of a query sit in LDS
    topk_merge_kernel<<<dim3((unsigned)Q), 64, (size_t)G * k * 8, static_cast<hipStream_t>(stream)>>>(load, G, Q, k, out_scores, out_idx);
    return mf_check_launch(who);
}

// Deep lists (k up to MF_TOPK_DEEP_MAX_K): the merge above runs k selection rounds over all G k keys; this one uses that every
// partial list arrives ORDERED by the same 64-bit key.  The place of entry e of list g in the merged list is e plus, for every
// other list, the number of its keys that stand before x = key(g, e): one binary search per other list over a descending run
// in LDS.  A key of an earlier list stands before an equal key of a later one (>= x against > x), so the ranks are a
// permutation of 0 .. m - 1 for ANY ordered lists -- equal keys across lists never meet on contract inputs, whose global rows
// are distinct -- and every output column is written exactly once: ranks below k by their entries, [min(m, k), k) as the tail.
// One 256-thread workgroup per query; the keys sit in LDS as [g][e], every list one contiguous run, no padding: a binary
// search has every lane on an address of its own, which no layout turns into a conflict-free pattern, but the lanes of a wave
// hold entries of like rank, so their searches of one list share their first probes (one address: a broadcast) and part only
// near the end.  Integer compares alone: no atomics, no float arithmetic, no selection rounds.  Every probe is clamped to its run, so an
// input that is not ordered gives unspecified results but no access outside the arrays (a rank is >= 0 by construction and
// checked against k before the store).
static constexpr int MERGE_DEEP_THREADS = 256;
static constexpr int MERGE_DEEP_STAGE = 8;             // keys a thread loads before it stores the first
static constexpr int MERGE_DEEP_ILP = 4;             // lists searched side by side by one thread: independent LDS read chains

template <class Load>
__global__ __launch_bounds__(MERGE_DEEP_THREADS) void topk_merge_deep_kernel(Load load, int G, int64_t Q, int k, float* __restrict__ out_scores,
                                                                              int64_t* __restrict__ out_idx) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_keys[];      // [g][e]: list g is the run s_keys + g k
    __shared__ unsigned long long s_floor[MERGE_DEEP_THREADS / 64];
    __shared__ int s_valid[MERGE_DEEP_THREADS / 64];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const int total = G * k;
    // stage the keys (a list is one contiguous piece of the input: coalesced) and count the entries that are there.  m is
    // the sum of the lists' valid lengths: counted here, where every key passes anyway, instead of searched for per list
    // (G lengths would want G more words of LDS: 16,384 lists at k = 1)
    // MERGE_DEEP_STAGE loads per thread are in flight before the first is looked at: a load that is turned into its key under
    // the bounds check is waited for on the spot, and one load per trip was all latency (62 trips in a row at G k = 16,000).
    // So the loads carry no branch -- past the end they read the last entry again, inside the arrays -- and the keys are
    // formed behind them
    int valid = 0;
    for (int t0 = 0; t0 < total; t0 += MERGE_DEEP_STAGE * MERGE_DEEP_THREADS) {      // (uniform trip count: the ballot sees the whole wave)
        typename Load::Raw raw[MERGE_DEEP_STAGE];
#pragma unroll
        for (int j = 0; j < MERGE_DEEP_STAGE; ++j) {
            const int t = min(t0 + j * MERGE_DEEP_THREADS + tid, total - 1);
            const int g = t / k, e = t - g * k;
            raw[j] = load.raw(((int64_t)g * Q + r) * k + e);
        }
#pragma unroll
        for (int j = 0; j < MERGE_DEEP_STAGE; ++j) {
            const int t = t0 + j * MERGE_DEEP_THREADS + tid;
            const unsigned long long key = t < total ? Load::key(raw[j]) : 0ull;
            if (t < total) s_keys[t] = key;
            valid += __popcll(__ballot(key != 0ull));
        }
    }
    if ((tid & 63) == 0) s_valid[tid >> 6] = valid;
    __syncthreads();
    int m = 0;
#pragma unroll
    for (int w = 0; w < MERGE_DEEP_THREADS / 64; ++w) m += s_valid[w];
    const int filled = min(m, k);

    // Most entries are out of the first k (all but k of G k), and most of them can be told without a search: with
    // p = ceil(k / G) - 1, every list holds p + 1 keys >= its own key at p, so G (p + 1) >= k keys are >= the smallest of those
    // G keys -- whatever is below that floor has k keys before it.  (A list shorter than p + 1 makes the floor 0: nothing is
    // dropped, nothing is wrong.)  Rows dealt evenly leave a little more than k entries to rank.
    const int p = (k + G - 1) / G - 1;
    unsigned long long inv = 0ull;                       // ~key: the smallest key is the largest ~key
    for (int gg = tid; gg < G; gg += MERGE_DEEP_THREADS) inv = max(inv, ~s_keys[gg * k + p]);
    inv = mf_wave_max_u64(inv);
    if ((tid & 63) == 0) s_floor[tid >> 6] = inv;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < MERGE_DEEP_THREADS / 64; ++w) inv = max(inv, s_floor[w]);
    const unsigned long long floor_key = ~inv;

    int top = 1;
    while (top * 2 <= k) top *= 2;
    // entries are dealt position-major (t = e G + g): what is left to rank are the heads of the lists, and a wave whose 64
    // entries are all dropped moves on after one LDS read -- dealt list-major, every wave would meet a few survivors in many
    // of its turns and run the searches for them with most lanes idle
    for (int t = tid; t < total; t += MERGE_DEEP_THREADS) {
        const int e = t / G, g = t - e * G;
        const unsigned long long x = s_keys[g * k + e];
        if (x == 0ull || x < floor_key) continue;
        int rank = e;
        // lists before g: keys >= x, i.e. > x - 1 (x != 0); lists behind g: keys > x.  The count c of a run's keys above y grows
        // by powers of two from `top`, the largest one <= k: floor(log2 k) + 1 probes (11 at k = 1024), each at
        // min(c + s, k) - 1, inside the run.  MERGE_DEEP_ILP lists per round, and no further round once the entry is out
        // of the first k
        for (int g0 = 0; g0 < G && rank < k; g0 += MERGE_DEEP_ILP) {
            int c[MERGE_DEEP_ILP], run[MERGE_DEEP_ILP];
            unsigned long long y[MERGE_DEEP_ILP];
#pragma unroll
            for (int j = 0; j < MERGE_DEEP_ILP; ++j) {
                const int gg = min(g0 + j, G - 1);                           // (past the last list: a second search of it, not added)
                c[j] = 0;
                run[j] = gg * k;
                y[j] = gg < g ? x - 1ull : x;
            }
            for (int s = top; s > 0; s >>= 1) {
                unsigned long long v[MERGE_DEEP_ILP];
#pragma unroll
                for (int j = 0; j < MERGE_DEEP_ILP; ++j) v[j] = s_keys[run[j] + min(c[j] + s, k) - 1];
                // all reads of a step are issued before any is looked at (the empty statement pins each value: left alone,
                // the compiler moves every read behind the test of its own `c + s <= k` and waits for them one by one)
#pragma unroll
                for (int j = 0; j < MERGE_DEEP_ILP; ++j) asm volatile("" : "+v"(v[j]));
#pragma unroll
                for (int j = 0; j < MERGE_DEEP_ILP; ++j) c[j] = (c[j] + s <= k && v[j] > y[j]) ? c[j] + s : c[j];
            }
#pragma unroll
            for (int j = 0; j < MERGE_DEEP_ILP; ++j) rank += (g0 + j < G && g0 + j != g) ? c[j] : 0;
        }
        if (rank < k) mf_store_topk_entry(out_scores, out_idx, r, k, rank, x, 0);
    }
    for (int t = filled + tid; t < k; t += MERGE_DEEP_THREADS) mf_store_topk_none(out_scores, out_idx, r, k, t);
}

// the keys of a query sit in LDS: G k <= MF_TOPK_MERGE_DEEP_MAX_KEYS of 8 bytes = 128 KiB of the CU's 160
template <class Load>
static int topk_merge_deep_launch(const char* who, Load load, int G, int64_t Q, int k, float* out_scores, int64_t* out_idx, mf_stream_t stream) {
    if (k > MF_TOPK_DEEP_MAX_K) return mf_set_error(MF_ENOTSUP, "%s: k = %d outside 1..%d", who, k, MF_TOPK_DEEP_MAX_K);
    if ((int64_t)G * k > MF_TOPK_MERGE_DEEP_MAX_KEYS) return mf_set_error(MF_ENOTSUP, "%s: G * k too large", who);
    auto fn = topk_merge_deep_kernel<Load>;
    static const hipError_t lds_set =                  // once per instantiation: the largest dynamic LDS any launch asks for
        hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, MF_TOPK_MERGE_DEEP_MAX_KEYS * 8);
    (void)lds_set;
    fn<<<dim3((unsigned)Q), MERGE_DEEP_THREADS, (size_t)G * k * 8, static_cast<hipStream_t>(stream)>>>(load, G, Q, k, out_scores, out_idx);
    return mf_check_launch(who);
}

// Sharded retrieval, one exchange instead of two: a rank's partial result (scores, LOCAL rows) becomes one int64 per entry
// -- the packed form of mf_topk_io.h, its global row = local * stride + offset (< 2^32) -- in a single launch (the row
// mapping alone took four elementwise launches), travels as ONE all-to-all, and is merged straight from that form.
__global__ __launch_bounds__(256) void topk_pack_kernel(const float* __restrict__ s, const int64_t* __restrict__ rows, int64_t n,
                                                        int64_t stride, int64_t offset, int64_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int64_t r = rows[t];
    out[t] = r >= 0 ? mf_packed_entry(s[t], (unsigned)(r * stride + offset)) : MF_PACKED_NONE;
}

extern "C" int mf_topk_pack(const float* scores, const int64_t* rows, int64_t n, int64_t stride, int64_t offset, int64_t* out_packed,
                            mf_stream_t stream) {
    if (!scores || !rows || !out_packed || n < 0 || stride <= 0 || offset < 0) return mf_set_error(MF_EINVAL, "mf_topk_pack: bad argument");
    if (n == 0) return MF_OK;
    topk_pack_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, static_cast<hipStream_t>(stream)>>>(scores, rows, n, stride, offset, out_packed);
    return mf_check_launch("mf_topk_pack");
}

extern "C" int mf_topk_merge_packed(const int64_t* packed, int G, int64_t Q, int k, float* out_scores, int64_t* out_idx, mf_stream_t stream) {
    if (!packed || !out_scores || !out_idx || G <= 0 || Q <= 0 || k <= 0) return mf_set_error(MF_EINVAL, "mf_topk_merge_packed: bad argument");
    return topk_merge_launch("mf_topk_merge_packed", MergePacked{packed}, G, Q, k, out_scores, out_idx, stream);
}

extern "C" int mf_topk_merge_packed_deep(const int64_t* packed, int G, int64_t Q, int k, float* out_scores, int64_t* out_idx, mf_stream_t stream) {
    if (!packed || !out_scores || !out_idx || G <= 0 || Q <= 0 || k <= 0) return mf_set_error(MF_EINVAL, "mf_topk_merge_packed_deep: bad argument");
    return topk_merge_deep_launch("mf_topk_merge_packed_deep", MergePacked{packed}, G, Q, k, out_scores, out_idx, stream);
}

#ifdef MF_PROBE
static TopkWs g_probe_ws;
extern "C" long long mf_probe_topk_cand() {       // tools/topk_probe.py: candidate keys kept by the last mf_topk
    (void)hipDeviceSynchronize();
    const size_t n = (size_t)g_probe_ws.plan.Xp;
    std::vector<int32_t> h(n);
    (void)hipMemcpy(h.data(), g_probe_ws.cand_cnt, n * 4, hipMemcpyDeviceToHost);
    long long t = 0;
    for (int32_t c : h) t += c;
    return t;
}
extern "C" void mf_probe_sel_counters(unsigned long long* out16, int reset) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out16, HIP_SYMBOL(mf_sel_dbg), 16 * 8);
    if (reset) {
        unsigned long long z[16] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(mf_sel_dbg), z, 16 * 8);
    }
}
#endif

extern "C" int mf_topk(const float* q, int64_t Q, const float* items, int64_t N, int d, int k,
                       const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, void* ws,
                       size_t ws_bytes, float* out_scores, int64_t* out_idx, mf_stream_t stream) {
    if (const int rc = mf_topk_check_args("mf_topk", {64, 32, 31, 0}, q, Q, items, N, d, k, excl_off, excl_idx, idx_base, ws, out_scores, out_idx))
        return rc;
    if (ws_bytes < mf_topk_ws_bytes(Q, N, d, k)) return mf_set_error(MF_ENOSPC, "mf_topk: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    TopkWs w = topk_ws(ws, Q, N, d, k);
    if (!w.plan.ok) return mf_set_error(MF_ENOTSUP, "mf_topk: k = %d too large at d = %d", k, d);
#ifdef MF_PROBE
    g_probe_ws = w;
#endif
    (void)hipMemsetAsync(w.exclW, 0, (size_t)((char*)(w.cand_cnt + w.plan.Xp) - (char*)w.exclW), s);
    if (excl_off) excl_scatter_kernel<<<dim3((unsigned)Q), 256, 0, s>>>(excl_off, excl_idx, idx_base, N, w.plan.Xp, w.exclW);
    RetrievalPolicy::Params rp{w.exclW, w.plan.Xp, N};
    SelectCommon sc{q, Q, items, N, 0, w.NT, w.plan.tpc, w.plan.Xp, k, w.plan.xw, w.gtau, w.priv, w.cand, w.cand_cnt, w.plan.rowcap};
    MF_DISPATCH_D(d, { MF_TIMED("topk_select", s, (mf_select_run<D, RetrievalPolicy>(w.plan, rp, sc, w.seeds, Q, s))); });
    topk_merge_cand_kernel<<<dim3((unsigned)Q), 64, 0, s>>>(w.cand, w.cand_cnt, w.plan.rowcap, k, idx_base, out_scores, out_idx);
    return mf_check_launch("mf_topk");
}

extern "C" int mf_topk_merge(const float* part_scores, const int64_t* part_idx, int G, int64_t Q, int k,
                             float* out_scores, int64_t* out_idx, mf_stream_t stream) {
    if (!part_scores || !part_idx || !out_scores || !out_idx || G <= 0 || Q <= 0 || k <= 0)
        return mf_set_error(MF_EINVAL, "mf_topk_merge: bad argument");
    return topk_merge_launch("mf_topk_merge", MergeParts{part_scores, part_idx}, G, Q, k, out_scores, out_idx, stream);
}

extern "C" int mf_topk_merge_deep(const float* part_scores, const int64_t* part_idx, int G, int64_t Q, int k,
                                  float* out_scores, int64_t* out_idx, mf_stream_t stream) {
    if (!part_scores || !part_idx || !out_scores || !out_idx || G <= 0 || Q <= 0 || k <= 0)
        return mf_set_error(MF_EINVAL, "mf_topk_merge_deep: bad argument");
    return topk_merge_deep_launch("mf_topk_merge_deep", MergeParts{part_scores, part_idx}, G, Q, k, out_scores, out_idx, stream);
}

// ------------------------------------------------------------ retrieval metrics ----
// one wave per query; lane t holds the items retrieved at ranks t + 64 j, j < R (register j)
template <int R>
__global__ __launch_bounds__(64) void retrieval_metrics_kernel(const int64_t* __restrict__ topk_idx, int k,
                                                               const int64_t* __restrict__ tgt_off,
                                                               const int64_t* __restrict__ tgt_idx,
                                                               const float* __restrict__ tgt_rel, float* __restrict__ out) {
    const int64_t q = blockIdx.x;
    const int lane = mf_lane();
    const int64_t e0 = tgt_off[q], e1 = tgt_off[q + 1];
    int64_t item[R];
    float rel[R];                                      // rating of the item at this rank (0: not a target)
    // a target the search missed ranks right below the retrieved items (list order): it only enters the
    // top k when fewer than k items were retrieved, exactly as in the reference's union of both sets
    int slot = 0;                                      // number of retrieved items: where the first missed target ranks
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int t = lane + 64 * j;
        item[j] = t < k ? topk_idx[q * k + t] : -1;
        rel[j] = 0.f;
        slot += __popcll(__ballot(item[j] >= 0));
    }
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t id = tgt_idx[e];
        const float tr = tgt_rel[e];
        bool mine = false;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const bool m = item[j] >= 0 && item[j] == id;
            if (m) rel[j] = tr;
            mine |= m;
        }
        if (!__any(mine)) {
            if (slot < k) {
#pragma unroll
                for (int j = 0; j < R; ++j)
                    if (slot == lane + 64 * j) rel[j] = tr;
            }
            ++slot;
        }
    }
    // ideal DCG: the targets' ratings in descending order (rank by counting), best k of them
    float idcg = 0.f;
    int npos = 0;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        const float r = tgt_rel[e];
        npos += r > 0.f ? 1 : 0;
        int rank = 0;
        for (int64_t f = e0; f < e1; ++f) {
            const float o = tgt_rel[f];
            rank += (o > r || (o == r && f < e)) ? 1 : 0;
        }
        if (rank < k) idcg += r / log2f((float)rank + 2.f);
    }
    float dcg = 0.f, ap = 0.f;                         // ap: precision at every relevant rank
    int hits = 0, first = -1;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int t = lane + 64 * j;
        dcg += rel[j] / log2f((float)t + 2.f);
        const unsigned long long hit = __ballot(rel[j] > 0.f);
        if (rel[j] > 0.f) ap += (float)(hits + __popcll(hit & ((2ull << lane) - 1ull))) / (float)(t + 1);
        if (first < 0 && hit != 0ull) first = 64 * j + __builtin_ctzll(hit);
        hits += __popcll(hit);
    }
    dcg = mf_wave_sum(dcg);
    idcg = mf_wave_sum(idcg);
    ap = mf_wave_sum(ap);
    npos = mf_wave_sum_int(npos);
    if (lane == 0) {
        float* o = out + q * 6;
        const bool any = npos > 0;
        o[0] = (any && idcg > 0.f) ? dcg / idcg : 0.f;
        o[1] = any ? (float)hits / (float)npos : 0.f;
        o[2] = any ? (float)hits / (float)k : 0.f;
        o[3] = hits > 0 ? ap / (float)hits : 0.f;
        o[4] = hits > 0 ? 1.f : 0.f;
        o[5] = hits > 0 ? 1.f / (float)(first + 1) : 0.f;
    }
}

extern "C" int mf_retrieval_metrics(const int64_t* topk_idx, int64_t Q, int k, const int64_t* tgt_off,
                                    const int64_t* tgt_idx, const float* tgt_rel, float* out, mf_stream_t stream) {
    if (!topk_idx || !tgt_off || !tgt_idx || !tgt_rel || !out || Q <= 0) return mf_set_error(MF_EINVAL, "mf_retrieval_metrics: bad argument");
    if (k <= 0 || k > MF_TOPK_DEEP_MAX_K) return mf_set_error(MF_ENOTSUP, "mf_retrieval_metrics: k = %d outside 1..%d", k, MF_TOPK_DEEP_MAX_K);
    auto fn = k <= 64 ? retrieval_metrics_kernel<1> : retrieval_metrics_kernel<MF_TOPK_DEEP_MAX_K / 64>;
    fn<<<dim3((unsigned)Q), 64, 0, static_cast<hipStream_t>(stream)>>>(topk_idx, k, tgt_off, tgt_idx, tgt_rel, out);
    return mf_check_launch("mf_retrieval_metrics");
}

// ------------------------------------------------------- metrics from positions ----
// The same six values at up to POS_METRICS_MAX_K cut-offs at once, and three uncut ones, from every target's exact place
// among the query's admissible rows (mf_target_positions; -1: not admissible) instead of from a list: "retrieved at
// column t" reads "position t < k", so k has no upper limit and a target that is not retrieved needs no place.  One wave
// per query, lane l takes targets l, l + 64, ..; a target's rank among the ratings (IDCG) and the number of relevant
// targets placed above it (MAP, AUC) are counted over the list, once for all cut-offs.
static constexpr int POS_METRICS_MAX_K = 8;
struct PosMetricKs {
    int32_t k[POS_METRICS_MAX_K];
};

__device__ __forceinline__ int64_t mf_wave_sum_i64(int64_t x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}
__device__ __forceinline__ int64_t mf_wave_min_i64(int64_t x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const int64_t o = __shfl_xor(x, s, 64);
        x = o < x ? o : x;
    }
    return x;
}

__global__ __launch_bounds__(64) void position_metrics_kernel(const int64_t* __restrict__ pos, const int64_t* __restrict__ tgt_off,
                                                              const float* __restrict__ tgt_rel, const int64_t* __restrict__ ncand,
                                                              PosMetricKs ks, int nk, float* __restrict__ out) {
    const int64_t q = blockIdx.x;
    const int lane = mf_lane();
    const int64_t e0 = tgt_off[q], e1 = tgt_off[q + 1];
    float dcg[POS_METRICS_MAX_K], idcg[POS_METRICS_MAX_K], ap[POS_METRICS_MAX_K];
    int hits[POS_METRICS_MAX_K];
#pragma unroll
    for (int i = 0; i < POS_METRICS_MAX_K; ++i) dcg[i] = idcg[i] = ap[i] = 0.f, hits[i] = 0;
    int npos = 0, nadm = 0;                            // relevant targets; relevant AND admissible ones
    int64_t first = INT64_MAX, sum_pos = 0, sum_nonrel_above = 0;
    // (every lane runs every round: a round's 64 entries are loaded once, one per lane, and handed round by lane number)
    for (int64_t eb = e0; eb < e1; eb += 64) {
        const int64_t e = eb + lane;
        const float r = e < e1 ? tgt_rel[e] : 0.f;
        const int64_t p = e < e1 ? pos[e] : -1;
        const bool relevant = r > 0.f, placed = relevant && p >= 0;
        const int pi = (int)p;                         // (positions are below 2^31: N is)
        // rank among the ratings, descending, list order among equals: one 64-bit key per entry, larger = earlier
        const unsigned long long ke = ((unsigned long long)mf_orderable(r) << 32) | (unsigned long long)~(unsigned)(e - e0);
        int rank = 0, above = 0;
        for (int64_t fb = e0; fb < e1; fb += 64) {
            const int64_t f = fb + lane;
            const float of = f < e1 ? tgt_rel[f] : 0.f;
            const int64_t pf = f < e1 ? pos[f] : -1;
            const int k_hi = f < e1 ? (int)mf_orderable(of) : 0, k_lo = f < e1 ? (int)~(unsigned)(f - e0) : 0;      // (0: behind every entry)
            const int at = (of > 0.f && pf >= 0) ? (int)pf : INT32_MAX;      // where a relevant target stands; never above anyone else
#pragma unroll 16
            for (int j = 0; j < 64; ++j) {
                const unsigned long long kf = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(k_hi, j) << 32) |
                                              (unsigned long long)(unsigned)__builtin_amdgcn_readlane(k_lo, j);
                rank += kf > ke ? 1 : 0;
                above += __builtin_amdgcn_readlane(at, j) < pi ? 1 : 0;
            }
        }
        if (e >= e1) continue;
        npos += relevant ? 1 : 0;
        if (placed) {
            ++nadm;
            first = p < first ? p : first;
            sum_pos += p;
            sum_nonrel_above += p - above;
        }
        const float gain_ideal = r / log2f((float)rank + 2.f);
        const float gain = p >= 0 ? r / log2f((float)p + 2.f) : 0.f;
        const float prec = placed ? (float)(above + 1) / (float)(p + 1) : 0.f;
#pragma unroll
        for (int i = 0; i < POS_METRICS_MAX_K; ++i) {
            if (i >= nk) continue;
            const int k = ks.k[i];
            if (rank < k) idcg[i] += gain_ideal;
            if (p >= 0 && p < k) {
                dcg[i] += gain;
                ap[i] += prec;
                hits[i] += placed ? 1 : 0;
            }
        }
    }
    npos = mf_wave_sum_int(npos);
    nadm = mf_wave_sum_int(nadm);
    first = mf_wave_min_i64(first);
    sum_pos = mf_wave_sum_i64(sum_pos);
    sum_nonrel_above = mf_wave_sum_i64(sum_nonrel_above);
    float* o = out + q * (6 * nk + 3);
    const bool any = npos > 0;
#pragma unroll
    for (int i = 0; i < POS_METRICS_MAX_K; ++i) {
        if (i >= nk) continue;
        const float d = mf_wave_sum(dcg[i]), id = mf_wave_sum(idcg[i]), a = mf_wave_sum(ap[i]);
        const int h = mf_wave_sum_int(hits[i]);
        if (lane == 0) {
            const int k = ks.k[i];
            o[6 * i + 0] = (any && id > 0.f) ? d / id : 0.f;
            o[6 * i + 1] = any ? (float)h / (float)npos : 0.f;
            o[6 * i + 2] = any ? (float)h / (float)k : 0.f;
            o[6 * i + 3] = h > 0 ? a / (float)h : 0.f;
            o[6 * i + 4] = h > 0 ? 1.f : 0.f;
            o[6 * i + 5] = h > 0 ? 1.f / (float)(first + 1) : 0.f;
        }
    }
    if (lane == 0) {
        const int64_t nonrel = ncand[q] - nadm;                         // admissible rows that are no relevant target
        const double den = (double)nadm * (double)(nonrel > 1 ? nonrel : 1);
        o[6 * nk + 0] = nadm > 0 ? 1.f / (float)(first + 1) : 0.f;
        o[6 * nk + 1] = nadm > 0 ? (float)((double)sum_pos / (double)nadm) : 0.f;
        o[6 * nk + 2] = nadm > 0 ? (float)(1.0 - (double)sum_nonrel_above / den) : 0.f;
    }
}

extern "C" int mf_position_metrics(const int64_t* pos, const int64_t* tgt_off, const float* tgt_rel, const int64_t* ncand, int64_t Q,
                                   const int32_t* ks, int nk, float* out, mf_stream_t stream) {
    if (!pos || !tgt_off || !tgt_rel || !ncand || !ks || !out || Q <= 0) return mf_set_error(MF_EINVAL, "mf_position_metrics: bad argument");
    if (nk < 1 || nk > POS_METRICS_MAX_K)
        return mf_set_error(MF_ENOTSUP, "mf_position_metrics: %d cut-offs outside 1..%d", nk, POS_METRICS_MAX_K);
    PosMetricKs k{};
    for (int i = 0; i < nk; ++i) {
        if (ks[i] < 1) return mf_set_error(MF_EINVAL, "mf_position_metrics: k = %d < 1", ks[i]);
        k.k[i] = ks[i];
    }
    position_metrics_kernel<<<dim3((unsigned)Q), 64, 0, static_cast<hipStream_t>(stream)>>>(pos, tgt_off, tgt_rel, ncand, k, nk, out);
    return mf_check_launch("mf_position_metrics");
}
