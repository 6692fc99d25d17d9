// mf_cells.h -- what the two searches over probed cells share (mf_ivf.hip: exact fp32 rows; mf_pq.hip: one-byte codes): "a
// 256-thread workgroup scans one slice of one probed cell of one query, a 64-row block per wave and pass, lane = row, and
// leaves one ordered list of packed entries (mf_topk_io.h)".  Here: into how many slices a cell is cut and what the scan
// exports refuse (host); the look-up in the query's exclusion list, the allow bitmap's word test and the entry a workgroup writes (device).  How a row is
// scored and how the best keys are kept is each scan's own -- DESIGN.md "Cell scans: what is shared".
#pragma once

#include "mf_common.h"
#include "mf_topk_io.h"

static constexpr int MF_CELLS_NW = 4;               // waves per workgroup, each a 64-row block per pass
static constexpr int MF_CELLS_MAX_PROBE = 64;
static constexpr int MF_CELLS_TARGET_WG = 1024;     // workgroups worth launching: four per CU

// ---- host: what a scan's lists and their merge can hold
struct MfCellsLimits {
    int max_depth;       // entries of a list: k (mf_ivf_scan), R (mf_pq_scan)
    int merge_keys;      // G * depth keys of a query that the merge of the lists holds in LDS
    char depth;          // the depth's letter in the messages
};

// Slices per probed cell: enough workgroups for a single query (MF_CELLS_TARGET_WG over Q * nprobe), never fewer than about
// a block per wave in a slice of the largest cell, never more partial lists than the merge holds.
static inline int mf_cells_slices(const MfCellsLimits& lim, int64_t Q, int nprobe, int depth, int64_t max_cell_blocks) {
    const int64_t cap_merge = lim.merge_keys / ((int64_t)nprobe * depth);
    const int64_t cap = cap_merge < max_cell_blocks ? cap_merge : max_cell_blocks;
    const int64_t want = (MF_CELLS_TARGET_WG + Q * nprobe - 1) / (Q * nprobe);
    const int64_t by_work = max_cell_blocks / MF_CELLS_NW > 1 ? max_cell_blocks / MF_CELLS_NW : 1;
    int64_t S = want < by_work ? want : by_work;
    if (S > cap) S = cap;
    if (S < 1) S = 1;
    return (int)S;
}
static inline bool mf_cells_plan_args_ok(const MfCellsLimits& lim, int64_t Q, int nprobe, int depth, int64_t max_cell_blocks) {
    return Q > 0 && max_cell_blocks > 0 && depth >= 1 && depth <= lim.max_depth && nprobe >= 1 && nprobe <= MF_CELLS_MAX_PROBE;
}
// the plan exports: S, the lists of a query G = nprobe * S, the workgroups, the bytes of the lists
static inline int mf_cells_plan(const char* who, const MfCellsLimits& lim, int64_t Q, int nprobe, int depth, int64_t max_cell_blocks,
                                int64_t* out4) {
    if (!out4) return mf_set_error(MF_EINVAL, "%s: out is NULL", who);
    if (!mf_cells_plan_args_ok(lim, Q, nprobe, depth, max_cell_blocks))
        return mf_set_error(MF_EINVAL, "%s: need Q > 0, max_cell_blocks > 0, %c in 1..%d and nprobe in 1..%d", who, lim.depth, lim.max_depth,
                            MF_CELLS_MAX_PROBE);
    const int S = mf_cells_slices(lim, Q, nprobe, depth, max_cell_blocks);
    out4[0] = S;
    out4[1] = (int64_t)nprobe * S;
    out4[2] = Q * nprobe * S;
    out4[3] = (int64_t)nprobe * S * Q * depth * 8;
    return MF_OK;
}
static inline size_t mf_cells_ws_bytes(const MfCellsLimits& lim, int64_t Q, int nprobe, int depth, int64_t max_cell_blocks) {
    if (!mf_cells_plan_args_ok(lim, Q, nprobe, depth, max_cell_blocks)) return 0;
    return mf_align_up((size_t)nprobe * mf_cells_slices(lim, Q, nprobe, depth, max_cell_blocks) * Q * depth * 8, 256);
}

// The checks of mf_ivf_scan / mf_pq_scan in the order their callers rely on, as mf_topk_check_args for the exact engines --
// in two halves, because mf_pq_scan judges its sub-vector length between them.  First: pointers (`pointers`: every one of the
// export's own is there) and sizes, the depth, nprobe, the width.
static inline int mf_cells_check_shape(const char* who, const MfCellsLimits& lim, bool pointers, int64_t Q, int64_t Npad, int64_t N, int64_t C,
                                       int d, int64_t max_cell_blocks, int nprobe, int depth, int S) {
    if (!pointers || Q <= 0 || N <= 0 || C <= 0 || Npad < N || (Npad & 63) != 0 || max_cell_blocks <= 0 || max_cell_blocks > Npad / 64 || S < 0)
        return mf_set_error(MF_EINVAL, "%s: bad argument", who);
    if (depth <= 0 || depth > lim.max_depth) return mf_set_error(MF_ENOTSUP, "%s: %c = %d outside 1..%d", who, lim.depth, depth, lim.max_depth);
    const int64_t max_probe = C < MF_CELLS_MAX_PROBE ? C : MF_CELLS_MAX_PROBE;
    if (nprobe <= 0 || nprobe > max_probe) return mf_set_error(MF_ENOTSUP, "%s: nprobe = %d outside 1..%lld", who, nprobe, (long long)max_probe);
    if (!mf_width_ok(d)) return mf_set_error(MF_EINVAL, "%s: embedding width %d not in {32,64,128,256}", who, d);
    return MF_OK;
}
// Then: 32-bit rows, the slices (S = 0 becomes the planned number) against the merge's keys, the workspace, the exclusion pair.
static inline int mf_cells_check_lists(const char* who, const MfCellsLimits& lim, int64_t Q, int64_t Npad, int64_t N, int64_t max_cell_blocks,
                                       int nprobe, int depth, int& S, const void* excl_off, const void* excl_idx, int64_t idx_base,
                                       size_t ws_bytes) {
    if (Npad >= (1ll << 31) || idx_base < 0 || idx_base + N > (1ll << 32)) return mf_set_error(MF_ENOTSUP, "%s: item indices must fit 32 bits", who);
    if (S == 0) S = mf_cells_slices(lim, Q, nprobe, depth, max_cell_blocks);
    const int64_t G = (int64_t)nprobe * S;
    if (G * depth > lim.merge_keys || S > max_cell_blocks || Q * G >= (1ll << 31))
        return mf_set_error(MF_ENOTSUP, "%s: nprobe * S * %c too large", who, lim.depth);
    if (ws_bytes < (size_t)G * Q * depth * 8) return mf_set_error(MF_ENOSPC, "%s: workspace too small", who);
    if ((excl_off == nullptr) != (excl_idx == nullptr)) return mf_set_error(MF_EINVAL, "%s: excl_off/excl_idx mismatch", who);
    return MF_OK;
}

// ---- the allow bitmap of mf_ivf_scan_allow / mf_pq_scan_allow: `allow` [n_masks][Npad / 64] 64-bit words, bit `lane` of word
// `blk` of a mask = the row at cell-ordered position blk * 64 + lane may enter a list (mf_filter_cell_bits writes them); query q
// reads mask allow_of[q], mask 0 without allow_of.  What the kernels carry of it:
struct MfCellsAllow {
    const unsigned long long* words;
    const int64_t* of;          // [Q], nullable
    int64_t n_masks, stride;    // stride = Npad / 64 words per mask
};
// The checks the two exports add behind their scans' own (mf_cells_check_lists has seen Npad < 2^31).
static inline int mf_cells_check_allow(const char* who, const void* allow, int64_t n_masks, const void* allow_of, int64_t Npad) {
    if (!allow || n_masks <= 0 || (!allow_of && n_masks != 1)) return mf_set_error(MF_EINVAL, "%s: bad allow argument", who);
    if (n_masks >= (1ll << 31) || n_masks * (Npad / 64) >= (1ll << 31))
        return mf_set_error(MF_ENOTSUP, "%s: n_masks * (Npad / 64) = %lld * %lld words exceed 2^31", who, (long long)n_masks, (long long)(Npad / 64));
    return MF_OK;
}

#ifdef __HIPCC__
// ---- device.  (Which blocks a workgroup walks -- blockIdx.x = (q * nprobe + probe) * S + slice, then the slice's share
// [b0, b1) of the probed cell's blocks -- stands in both kernels, the same lines: as a function here it cost the scans up to
// 2 % of their time whichever way its results left it.  DESIGN.md has the figures.)
// Only a key that would enter the list is looked up (`pass`: the lane's key beats the bound): the wave walks the query's
// exclusion list excl_idx[e0, e1) (GLOBAL rows, any order) for each such lane's row `grow` in turn.  Returns `pass`, false
// where the row is on the list.  Call it with the whole wave active.
__device__ __forceinline__ bool mf_cells_admit(bool pass, unsigned grow, const int64_t* excl_idx, int64_t e0, int64_t e1, int lane) {
    unsigned long long todo = __ballot(pass);
    while (todo) {
        const int src_lane = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int64_t want = (int64_t)(unsigned)__shfl((int)grow, src_lane, 64);
        bool hit = false;
        for (int64_t e = e0 + lane; e < e1; e += 64) hit |= excl_idx[e] == want;
        if (__ballot(hit) != 0ull && lane == src_lane) pass = false;
    }
    return pass;
}

// The words of query q's mask; null where allow_of[q] names no mask: that query admits nothing.  (workgroup-uniform)
__device__ __forceinline__ const unsigned long long* mf_cells_allow_mask(const MfCellsAllow& a, int64_t q) {
    const int64_t m = a.of ? a.of[q] : 0;
    return m >= 0 && m < a.n_masks ? a.words + m * a.stride : nullptr;
}
// The word of block `blk` (wave-uniform: one scalar load a wave), 0 for a query without a mask.  A wave whose word is 0 has
// nothing to read in the block; a lane's key counts only where mf_cells_allowed says so.
typedef const __attribute__((address_space(4))) unsigned long long* mf_const_u64;
__device__ __forceinline__ unsigned long long mf_cells_allow_word(const unsigned long long* mask, int64_t blk) {
    return mask ? ((mf_const_u64)mask)[blk] : 0ull;
}
// The same words for a scan whose pass waits on LDS reads (mf_pq_scan.inc): a scalar load shares their counter, which is waited
// to zero at every barrier, so a word asked for by scalar load costs its whole latency once a pass wherever it is asked for
// (measured: 3 ... 5 % of the all-ones scan at 1024 queries, at the top of the pass, ahead of the table reads and behind them
// alike).  Instead lane l takes the word of block `first + l` -- one coalesced vector load for the next 64 blocks, 16 passes of
// four waves, on the counter of the code loads, which a barrier does not wait for -- and a pass reads its word out of the strip.
// 0 from `end` on and for a query without a mask.
__device__ __forceinline__ unsigned long long mf_cells_allow_strip(const unsigned long long* mask, int64_t first, int64_t end, int lane) {
    return mask && first + lane < end ? mask[first + lane] : 0ull;
}
// the word lane `at` of the strip holds; `at` wave-uniform in [0, 64)
__device__ __forceinline__ unsigned long long mf_cells_strip_word(unsigned long long strip, int at) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)strip, at);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(strip >> 32), at);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ bool mf_cells_allowed(unsigned long long word, int lane) { return (word >> lane) & 1ull; }

// the packed entry of a key that is there (a kernel writes MF_PACKED_NONE from its own branch where there is none)
__device__ __forceinline__ long long mf_cells_entry(unsigned long long key) {
    return mf_packed_entry(mf_key_retrieval_score(key), mf_key_retrieval_col(key));
}
#endif
