// mf_bf_split.h -- fp32 as a sum of three bf16 pieces, and the operand images of the split sweeps (backward and forward).
//
// x = p0 + p1 + p2 to 2^-26 |x| (each piece rounds what the pieces before it left; the subtractions are exact).  A product
// x y is then the nine piece products; the six with piece indices i + j <= 2 leave out terms of at most ~2^-23 |x y|, so a
// contraction on v_mfma_f32_32x32x16_bf16 -- exact products, fp32 accumulation -- with those six is fp32-grade at 6/16 of
// the fp32 matrix pipe's time.  Used by the mining prefilter (mf_mine_bf.h) and the d = 128 dense sweeps, forward and backward
// (mf_loss_dense.hip).
#pragma once

#include "mf_common.h"

// The streamed operand of a split backward sweep, per 32-row tile: [piece 3][accumulator block 4][k-step 2][lane 64][8 bf16],
// 24 KiB that LDS-DMA copies linearly and of which every ds_read_b128 at 16 * lane is an A fragment.  The B operand is the
// G' tile in accumulator layout: element j of k-step s in lane (c, h) is stash register 8 s + j, i.e. tile row
// (j & 3) + 8 (2 s + (j >> 2)) + 4 h; the A fragment of lane (r, h) holds the same rows of feature 4 r + block, so that
// register e of accumulator block j stays feature NB row + j (the epilogue's layout).
static constexpr int BSI_TILE_ELEMS = 3 * 32 * 128;          // bf16 slots of a tile
static constexpr int BSI_TILEB = 2 * BSI_TILE_ELEMS;         // 24 KiB
__host__ __device__ static inline int bsi_index(int row, int feature, int piece) {
    const int blk = feature & 3, r = feature >> 2;
    const int h = (row >> 2) & 1, s = row >> 4, j = (row & 3) | (((row >> 3) & 1) << 2);
    return ((((piece * 4 + blk) * 2 + s) * 64 + r + 32 * h) << 3) + j;
}

// The streamed item tile of the split FORWARD sweep contracts over the 128 features, in 8 k-steps of 16, so it has a layout of
// its own, per 32-row tile: [piece 3][k-step 8][lane 64][8 bf16], 24 KiB, copied linearly by LDS-DMA; lane (c, h) of k-step s
// holds features 16 s + 8 h .. + 7 of tile row c, so every ds_read_b128 at 16 * lane is the A fragment of one
// v_mfma_f32_32x32x16_bf16.  The B fragment is the user row in the same feature order, split in registers.
static constexpr int FSI_TILE_ELEMS = 3 * 8 * 64 * 8;        // = BSI_TILE_ELEMS: the two images of a tile have one size
static constexpr int FSI_TILEB = 2 * FSI_TILE_ELEMS;         // 24 KiB
static_assert(FSI_TILE_ELEMS == BSI_TILE_ELEMS, "the forward image of v lives where the backward's does");
__host__ __device__ static inline int fsi_index(int row, int feature, int piece) {
    const int s = feature >> 4, h = (feature >> 3) & 1, j = feature & 7;
    return ((((piece * 8 + s) * 64) + row + 32 * h) << 3) + j;
}

#ifdef __HIPCC__

__device__ __forceinline__ unsigned short mbf_round(float x) {
    const __bf16 b = (__bf16)x;
    return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float mbf_float(unsigned short b) { return __builtin_bit_cast(float, (unsigned)b << 16); }
// x -> three bf16 pieces whose sum is x to 2^-26 |x| (the subtractions are exact)
__device__ __forceinline__ void mbf_split3(float x, unsigned short (&o)[3]) {
    o[0] = mbf_round(x);
    const float r1 = x - mbf_float(o[0]);
    o[1] = mbf_round(r1);
    const float r2 = r1 - mbf_float(o[1]);
    o[2] = mbf_round(r2);
}

#endif  // __HIPCC__
