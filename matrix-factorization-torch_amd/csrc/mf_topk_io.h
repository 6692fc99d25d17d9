// mf_topk_io.h -- the two ends the exact top-k engines share (mf_topk.hip, mf_topk_small.hip, mf_topk_bf3.hip,
// mf_topk_deep.hip): the argument check every search export opens with (host), and how one entry of a result -- a 64-bit
// retrieval key (mf_numerics.h), or "none" -- is stored (device): in the result arrays, and packed into one int64 for the
// partial lists that the sharded search and the cell scans (mf_cells.h) hand to the packed merges.
#pragma once

#include <cmath>
#include <cstdio>

#include "mf_common.h"

// ---- host: the checks of mf_topk / mf_topk_small / mf_topk_bf3 / mf_topk_deep, in the order their callers rely on:
// pointers and sizes, (queries,) k, width, 32-bit rows, the exclusion pair.  The engine's own geometry and its workspace
// size come after, in the export.
struct MfTopkLimits {
    int max_k;
    int min_width;       // widths min_width, .., 256 (powers of two); an engine that takes fewer than the catalog may have
                         // (min_width > 32) answers MF_ENOTSUP, not MF_EINVAL: "auto" then asks the tile engine
    int log2_max_rows;   // N < 2^this (and idx_base + N <= 2^32: a row is the low half of a key)
    int max_q;           // 0: any number of queries
};

static inline int mf_topk_check_args(const char* who, const MfTopkLimits& lim, const void* q, int64_t Q, const void* items, int64_t N,
                                     int d, int k, const void* excl_off, const void* excl_idx, int64_t idx_base, const void* ws,
                                     const void* out_scores, const void* out_idx) {
    if (!q || !items || !out_scores || !out_idx || !ws || Q <= 0 || N <= 0) return mf_set_error(MF_EINVAL, "%s: bad argument", who);
    if (lim.max_q && Q > lim.max_q) return mf_set_error(MF_ENOTSUP, "%s: Q = %lld > %d (use mf_topk)", who, (long long)Q, lim.max_q);
    if (k <= 0 || k > lim.max_k) return mf_set_error(MF_ENOTSUP, "%s: k = %d outside 1..%d", who, k, lim.max_k);
    if (!mf_width_ok(d) || d < lim.min_width) {
        char set[32];
        int n = 0;
        for (int w = lim.min_width; w <= 256; w *= 2) n += snprintf(set + n, sizeof(set) - n, n ? ",%d" : "%d", w);
        return mf_set_error(lim.min_width > 32 ? MF_ENOTSUP : MF_EINVAL, "%s: embedding width %d not in {%s}", who, d, set);
    }
    if (N >= (1ll << lim.log2_max_rows) || idx_base < 0 || idx_base + N > (1ll << 32)) {
        char also[40] = "";
        if (lim.log2_max_rows < 31) snprintf(also, sizeof(also), " (and a shard 2^%d rows)", lim.log2_max_rows);
        return mf_set_error(MF_ENOTSUP, "%s: item indices must fit 32 bits%s", who, also);
    }
    if ((excl_off == nullptr) != (excl_idx == nullptr)) return mf_set_error(MF_EINVAL, "%s: excl_off/excl_idx mismatch", who);
    return MF_OK;
}

#ifdef __HIPCC__
// ---- device: entry `rank` of query `row`'s k results.  0 is the key of no score a search meets (its high half would be
// mf_orderable of one particular NaN), so 0 stands for "no candidate": fewer than k rows were eligible, and the tail reads
// -inf / -1.  (The place is worked out at each store, behind the value, as the kernels did before they shared this: handing
// in a finished position moved that arithmetic in front of the branch and changed the register allocation of whole kernels.)
__device__ __forceinline__ void mf_store_topk_entry(float* __restrict__ out_scores, int64_t* __restrict__ out_idx, int64_t row, int k, int rank,
                                                    unsigned long long key, int64_t idx_base) {
    out_scores[row * k + rank] = mf_key_retrieval_score(key);
    out_idx[row * k + rank] = idx_base + (int64_t)mf_key_retrieval_col(key);
}
__device__ __forceinline__ void mf_store_topk_none(float* __restrict__ out_scores, int64_t* __restrict__ out_idx, int64_t row, int k, int rank) {
    out_scores[row * k + rank] = -INFINITY;
    out_idx[row * k + rank] = -1;
}
// (a kernel that knows how many entries it holds calls the two above from its own branch; idx_base = 0 for keys that
// carry global rows)
__device__ __forceinline__ void mf_store_topk(float* __restrict__ out_scores, int64_t* __restrict__ out_idx, int64_t row, int k, int rank, unsigned long long key,
                                              int64_t idx_base) {
    if (key != 0ull) mf_store_topk_entry(out_scores, out_idx, row, k, rank, key, idx_base);
    else mf_store_topk_none(out_scores, out_idx, row, k, rank);
}

// ---- device: the packed form of an entry, one int64 where the two arrays above take twelve bytes -- what partial lists
// travel in between a kernel that leaves them and a merge (mf_topk_pack, the cell scans of mf_cells.h -> mf_topk_merge_packed,
// mf_topk_merge_packed_deep): the score's bits << 32 | the GLOBAL row (< 2^32), all ones (-1) for "none" (as an entry
// that would be row 2^32 - 1 under one particular NaN: nothing a search writes).
static constexpr long long MF_PACKED_NONE = -1ll;
__device__ __forceinline__ long long mf_packed_entry(float score, unsigned grow) {
    return (long long)(((unsigned long long)__builtin_bit_cast(unsigned, score) << 32) | (unsigned long long)grow);
}
// the retrieval key of a packed entry, 0 for "none"
__device__ __forceinline__ unsigned long long mf_packed_key(long long v) {
    return v != MF_PACKED_NONE ? mf_key_retrieval(__builtin_bit_cast(float, (unsigned)((unsigned long long)v >> 32)), (unsigned)v) : 0ull;
}
#endif
