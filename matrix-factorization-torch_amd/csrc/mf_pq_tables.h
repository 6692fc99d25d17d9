// mf_pq_tables.h -- what the two scans over quantised cells share: pq_scan_kernel (mf_pq.hip, lists of up to 256 candidates)
// and pq_deep_scan_kernel (mf_ivf_deep.hip, up to 1,024).  The sub-vector geometry and its dispatch, the chain over a
// sub-vector the query's tables are built with, and the scans' parameters.  How the best keys are kept is each scan's own.
#pragma once

#include "mf_cells.h"

static constexpr int PQ_MAX_M = 64;            // 64 KiB of tables

static inline bool pq_dsub_ok(int dsub) { return dsub == 4 || dsub == 8 || dsub == 16; }

#define PQ_DISPATCH_M(DS, d, ...)                                                          \
    switch (d) {                                                                           \
        case 32: { constexpr int M = 32 / DS, DSUB = DS; __VA_ARGS__; } break;              \
        case 64: { constexpr int M = 64 / DS, DSUB = DS; __VA_ARGS__; } break;              \
        case 128: { constexpr int M = 128 / DS, DSUB = DS; __VA_ARGS__; } break;            \
        default: { constexpr int M = 256 / DS, DSUB = DS; __VA_ARGS__; } break;             \
    }
// (d in {32, 64, 128, 256} and dsub in {4, 8, 16} were checked: twelve pairs, M = 2 .. 64)
#define PQ_DISPATCH(d, dsub, ...)                                                     \
    switch (dsub) {                                                                        \
        case 4: PQ_DISPATCH_M(4, d, __VA_ARGS__) break;                                    \
        case 8: PQ_DISPATCH_M(8, d, __VA_ARGS__) break;                                    \
        default: PQ_DISPATCH_M(16, d, __VA_ARGS__) break;                                  \
    }

#ifdef __HIPCC__
// the chain over one sub-vector: mf_dot_chain's order for 8 and 16 channels, ascending for 4
template <int DSUB, class A, class B>
__device__ __forceinline__ float pq_chain(const A& a, const B& b) {
    float acc = 0.f;
    if constexpr (DSUB == 4) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_fmaf(a[t], b[t], acc);
    } else {
#pragma unroll
        for (int g = 0; g < DSUB; g += 8) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc = __builtin_fmaf(a[g + t], b[g + t], acc);
                acc = __builtin_fmaf(a[g + 4 + t], b[g + 4 + t], acc);
            }
        }
    }
    return acc;
}

template <int DSUB>
__device__ __forceinline__ void pq_load_sub(float (&v)[DSUB], const float* __restrict__ src) {
#pragma unroll
    for (int c = 0; c < DSUB / 4; ++c) {
        const f32x4 x = reinterpret_cast<const f32x4*>(src)[c];
#pragma unroll
        for (int t = 0; t < 4; ++t) v[4 * c + t] = x[t];
    }
}
#endif

struct PqScanParams {
    const float* q;             // [Q][D]
    const float* codebooks;     // [M][256][DSUB]
    const unsigned char* codes; // the cell-ordered layout of mf_pq.hip
    const int64_t* cell_blk;    // [C + 1]
    const int64_t* row_of;      // [Npad]
    const int64_t* probes;      // [Q][nprobe]
    const float* probe_scores;  // [Q][nprobe]: chain(q, centroid of the probe)
    int64_t Q, C;
    int nprobe, S, R;
    const int64_t *excl_off, *excl_idx;     // nullable
    int64_t idx_base;
    long long* out;             // [nprobe * S][Q][R] packed entries (mf_topk_io.h) of the approximate scores
    MfCellsAllow allow;         // the ALLOW kernels' bitmap (mf_cells.h); the others never look at it
};
