// mf_loss_masks.hip -- the hit masks of the losses (negative_masks, xfmr_rec/losses.py:92-110): which item columns are NOT
// valid negatives of which user, as B x N BITS, without the reference's B x N x P temp (losses.py:108).  Stage two of the
// forward (mf_loss_ws.h lists the units); also built ahead of it (mf_loss_masks*) or for a caller (mf_negative_masks).
#include "mf_loss_ws.h"

// ------------------------------------------------------------------ hit masks --
// maskW [tj][i]  bit c : item column 32 tj + c is NOT a valid negative of user i
//
// The reference compares every (user, column, positive) triple (B x N x P bools,
// losses.py:108).  Here:
//   1. the batch's item ids go into ONE open-addressing table (M >= 2N slots); every column
//      learns the FIRST column that carries the same item id (duplicates are common: Zipf);
//   2. each user's positives (plus its own item: the accidental-hit term, losses.py:103) are
//      looked up there and set ONE bit, in the bit-vector over users of that first column:
//      ubitsT[first][user / 32] -- positives absent from the batch cost nothing more;
//   3. the 32 columns of a tile then each fetch the user bit-vector of THEIR first column (a
//      duplicate column simply reads another row: no per-duplicate probing) and a 32 x 32 bit
//      transpose across the half-wave turns (lane = column, bit = user) into the mask words
//      (lane = user, bit = column).  No atomics in the sweep, no B x N x P temp.
static constexpr long long HT_EMPTY = (long long)0x8080808080808080ull;   // memset(0x80)

__device__ __forceinline__ unsigned ht_hash(long long id, unsigned slots_mask) {
    return ((((unsigned)id * 2654435761u) ^ ((unsigned)((unsigned long long)id >> 32) * 40503u)) >> 5) & slots_mask;
}

// bit of an id in the batch-membership bitmap (2^bits bits): a second, independent mix of the id
__device__ __forceinline__ unsigned bm_hash(long long id, int bits) {
    return (unsigned)(((unsigned long long)id * 0x9E3779B97F4A7C15ull) >> (64 - bits));
}

// (64-thread workgroups: every thread is one chain of dependent memory operations; spread over all CUs)
// Round trips per column: the id; then the slot, its first-column word and the bitmap word TOGETHER (a Zipf batch repeats its
// popular items hundreds of times: looking before every atomic saves most of them -- a stale read only costs the atomic it
// would have saved; slots never change once taken, gfirst only decreases, bitmap bits are only set); then the claiming CAS
// when the slot was empty.  The two updates behind it return nothing and are not waited for.
__global__ __launch_bounds__(64) void gt_insert_kernel(const int64_t* __restrict__ item_idx, int64_t N, int M,
                                                        long long* __restrict__ gtab, int32_t* __restrict__ gfirst,
                                                        int32_t* __restrict__ colslot, uint32_t* __restrict__ bmap, int bmbits) {
    // Round 4: ONE lane per item and wave talks to the tables.  Every column of the batch runs at once, so "look before the
    // atomic" saves nothing on the popular items (all 700 copies of the first one see an empty slot), and atomics on one word
    // queue up at its L2 channel: 700 claims + 700 minima on two words were most of this kernel's 16.5 us.  The wave's 64
    // columns elect, per item, their lowest lane (a 128-slot LDS table: the key, then the minimum lane among the lanes that
    // find their own key there; two different items in one slot: the loser just acts for itself); the leader probes, claims,
    // publishes the slot; its followers -- later columns of the same item: their minimum is not needed -- take it from LDS.
    __shared__ unsigned long long e_key[128];
    __shared__ int e_lane[128];
    __shared__ unsigned e_hpos[128];
    const int lane = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const bool live = j < N;
    const long long key = live ? item_idx[j] : 0;
    const unsigned es = (unsigned)(((unsigned long long)key * 0x9E3779B97F4A7C15ull) >> 57);      // 7 bits
    e_lane[lane] = 64; e_lane[lane + 64] = 64;
    __syncthreads();
    if (live) e_key[es] = (unsigned long long)key;          // (any one of the slot's writers stays)
    __syncthreads();
    const bool mine_slot = live && e_key[es] == (unsigned long long)key;
    if (mine_slot) atomicMin(&e_lane[es], lane);
    __syncthreads();
    const bool leader = live && (!mine_slot || e_lane[es] == lane);
    unsigned hpos = 0u;
    if (leader) {
        unsigned long long* tab = reinterpret_cast<unsigned long long*>(gtab);
        const volatile unsigned long long* vtab = tab;
        hpos = ht_hash(key, M - 1);
        const unsigned b = bm_hash(key, bmbits);
        const uint32_t bit = 1u << (b & 31);
        unsigned long long old = vtab[hpos];                                   // three independent loads in flight
        int32_t first_seen = *(const volatile int32_t*)&gfirst[hpos];
        const uint32_t bm_seen = *(const volatile uint32_t*)&bmap[b >> 5];
        for (int probe = 0; probe < M; ++probe) {
            if (probe) {
                old = vtab[hpos];
                first_seen = *(const volatile int32_t*)&gfirst[hpos];
            }
            if (old == (unsigned long long)HT_EMPTY)
                old = atomicCAS(&tab[hpos], (unsigned long long)HT_EMPTY, (unsigned long long)key);
            if (old == (unsigned long long)HT_EMPTY || old == (unsigned long long)key) break;
            hpos = (hpos + 1) & (M - 1);
        }
        if (first_seen > (int32_t)j) atomicMin(&gfirst[hpos], (int32_t)j);     // cleared to 0x7f7f7f7f
        if (!(bm_seen & bit)) atomicOr(&bmap[b >> 5], bit);
        if (mine_slot) e_hpos[es] = hpos;
    }
    __syncthreads();
    if (live) colslot[j] = (int32_t)(leader ? hpos : e_hpos[es]);
}

// colfirst[j] = first column with column j's item (-1: padding column)
__device__ __forceinline__ void colfirst_body(int64_t j, const int32_t* __restrict__ colslot,
                                              const int32_t* __restrict__ gfirst, int64_t N, int64_t Np,
                                              int32_t* __restrict__ colfirst) {
    int32_t f = -1;
    if (j < N) f = gfirst[colslot[j]];
    if (j < Np) colfirst[j] = f;
}

// gtab lookup: first column of `key` in the batch, or -1
__device__ __forceinline__ int32_t ht_find(long long key, int M, const long long* __restrict__ gtab,
                                           const int32_t* __restrict__ gfirst) {
    unsigned hpos = ht_hash(key, M - 1);
    for (int probe = 0; probe < M; ++probe) {
        const long long sv = gtab[hpos];
        if (sv == key) return gfirst[hpos];
        if (sv == HT_EMPTY) return -1;        // this positive is not in the batch
        hpos = (hpos + 1) & (M - 1);
    }
    return -1;
}

// One launch for both consumers of the finished hash table.  Blocks [0, nb_col): colfirst.  The rest: `split` blocks per
// group of 32 users.  ubits is laid out [plane][group][column]: a block owns ONE ROW -- word `column` of its group, in its
// plane -- keeps that row in LDS (64 KiB at N = 16,384), sets a bit per hit with a fire-and-forget LDS atomic indexed by the
// hit's first column, and writes the whole row out with coalesced 16-byte stores: nothing needs clearing, no hash table of
// hits, no scattered 4-byte global stores (the [column][group] layout of round 2 scattered ~4 M of them per batch at the
// MovieLens-25M list profile, and per-hit global atomics were 5 x slower still: 967 us).
// The lists of the 32 users are walked as ONE flat range, cut in `split` equal pieces, one block and one plane each (a user
// with 30,000 positives -- and the group it sits in -- is spread over `split` x 1024 threads; list lengths are heavy-tailed:
// with one block per group the heaviest group set the kernel's time); the sweep ORs the planes.  Most positives are not in
// the batch at all: every id is first tested against the batch-membership bitmap (a copy in LDS; ~7 % false positives at
// 8 bits per column), and only the survivors probe the hash table in L2 -- HITS_MLP ids in flight per thread, first probes
// and first-column reads batched.  Batches wider than HITS_WIN columns are handled in windows (the lists are walked once
// per window).
static constexpr int HITS_THREADS = 1024, HITS_MLP = 8, HITS_MAX_SPLIT = HITS_PLANES, HITS_WIN = 32768;

__global__ __launch_bounds__(HITS_THREADS) void hits_kernel(const int64_t* __restrict__ item_idx, PosSrc src,
                                                            int64_t B, int64_t N, int64_t Bp, int64_t Np, int M, int nb_col, int split,
                                                            int win, const long long* __restrict__ gtab,
                                                            const int32_t* __restrict__ gfirst, const int32_t* __restrict__ colslot,
                                                            int32_t* __restrict__ colfirst, uint32_t* __restrict__ ubits,
                                                            const uint32_t* __restrict__ bmap, int bmbits) {
    extern __shared__ __attribute__((aligned(16))) uint32_t hl[];          // [win] the row, then the bitmap
    __shared__ int lstart[33];
    __shared__ const int64_t* lbase[32];
    if ((int)blockIdx.x < nb_col) {
        colfirst_body((int64_t)blockIdx.x * HITS_THREADS + threadIdx.x, colslot, gfirst, N, Np, colfirst);
        return;
    }
    const int grp = (blockIdx.x - nb_col) / split, sub = (blockIdx.x - nb_col) % split;
    const int64_t ngrp = Bp >> 5;
    uint32_t* out_row = ubits + ((int64_t)sub * ngrp + grp) * Np;
    uint32_t* row = hl;
    uint32_t* lbm = hl + win;
    const int bmw = 1 << (bmbits - 5);
    for (int e = threadIdx.x; e < bmw / 4; e += HITS_THREADS) reinterpret_cast<uint4*>(lbm)[e] = reinterpret_cast<const uint4*>(bmap)[e];
    if (threadIdx.x < 64) {                                                // wave 0: the 32 lists and their flat offsets
        const int ul = threadIdx.x & 31;
        const int64_t i = (int64_t)grp * 32 + ul;
        const int64_t* base = nullptr;
        int len = 0;
        if (i < B) len = pos_list(src, i, base);
        int incl = len;                                                    // inclusive scan over the 32 lanes of a half-wave
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (ul >= o) incl += up;
        }
        if (threadIdx.x < 32) {
            lstart[ul + 1] = incl;
            lbase[ul] = base;
            if (ul == 0) lstart[0] = 0;
        }
    }
    for (int64_t w0 = 0; w0 < Np; w0 += win) {
        const int nw = (int)min((int64_t)win, Np - w0);                    // (Np is a multiple of 128)
        for (int e = threadIdx.x; e < nw / 4; e += HITS_THREADS) reinterpret_cast<uint4*>(row)[e] = uint4{0u, 0u, 0u, 0u};
        __syncthreads();
        const int total = lstart[32];
        // flat positions [0, total): the lists; [total, total + 32): every user's own item (the accidental-hit term, losses.py:103)
        const int piece = (total + 32 + split - 1) / split;
        const int p0 = sub * piece, p1 = min(total + 32, p0 + piece);
        for (int t0 = p0 + threadIdx.x; t0 < p1; t0 += HITS_THREADS * HITS_MLP) {
            long long key[HITS_MLP];
            int ulv[HITS_MLP];
            bool live[HITS_MLP];
#pragma unroll
            for (int j = 0; j < HITS_MLP; ++j) {
                const int t = t0 + j * HITS_THREADS;
                live[j] = false; key[j] = 0; ulv[j] = 0;
                if (t < p1 && t < total) {
                    int lo = 0, hi = 32;                                   // the list holding flat position t: last start <= t
#pragma unroll
                    for (int sft = 0; sft < 5; ++sft) {
                        const int mid = (lo + hi) >> 1;
                        if (lstart[mid] <= t) lo = mid; else hi = mid;
                    }
                    ulv[j] = lo;
                    key[j] = lbase[lo][t - lstart[lo]];
                    live[j] = true;
                } else if (t < p1) {
                    ulv[j] = t - total;
                    const int64_t i = (int64_t)grp * 32 + ulv[j];
                    if (i < B) { key[j] = item_idx[i]; live[j] = true; }
                }
            }
            unsigned hpos[HITS_MLP];
            long long sv[HITS_MLP];
#pragma unroll
            for (int j = 0; j < HITS_MLP; ++j) {                           // prefilter, then the first probes, all in flight
                if (live[j]) {
                    const unsigned b = bm_hash(key[j], bmbits);
                    live[j] = (lbm[b >> 5] >> (b & 31)) & 1u;
                }
                hpos[j] = ht_hash(key[j], M - 1);
                sv[j] = live[j] ? gtab[hpos[j]] : HT_EMPTY;
            }
            int32_t f[HITS_MLP];
#pragma unroll
            for (int j = 0; j < HITS_MLP; ++j) {                           // the first columns of the direct hits, all in flight
                f[j] = -1;
                if (live[j] && sv[j] == key[j]) f[j] = gfirst[hpos[j]];
            }
#pragma unroll
            for (int j = 0; j < HITS_MLP; ++j) {
                if (!live[j] || sv[j] == HT_EMPTY) continue;
                if (sv[j] != key[j]) {                                     // collision: walk on (rare at load <= 1/2)
                    unsigned hp = (hpos[j] + 1) & (M - 1);
                    for (int probe = 1; probe < M; ++probe) {
                        const long long v = gtab[hp];
                        if (v == key[j]) { f[j] = gfirst[hp]; break; }
                        if (v == HT_EMPTY) break;
                        hp = (hp + 1) & (M - 1);
                    }
                }
                const int64_t fw = (int64_t)f[j] - w0;
                if (f[j] >= 0 && fw >= 0 && fw < nw) atomicOr(&row[fw], 1u << ulv[j]);   // (LDS, no return value)
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < nw / 4; e += HITS_THREADS)
            reinterpret_cast<uint4*>(out_row + w0)[e] = reinterpret_cast<const uint4*>(row)[e];
        __syncthreads();
    }
}

// 32 x 32 bit transpose across the 32 lanes of a half-wave: lane i holds row i; five block-swap steps
template <int J, uint32_t M0>
__device__ __forceinline__ uint32_t bit_transpose_step(uint32_t w, int lane) {
    const uint32_t p = mf_xor_lane_u32<J>(w);
    return (lane & J) ? ((w & ~M0) | ((p & ~M0) >> J)) : ((w & M0) | ((p & M0) << J));
}
__device__ __forceinline__ uint32_t bit_transpose32(uint32_t w, int lane) {
    w = bit_transpose_step<16, 0x0000FFFFu>(w, lane);
    w = bit_transpose_step<8, 0x00FF00FFu>(w, lane);
    w = bit_transpose_step<4, 0x0F0F0F0Fu>(w, lane);
    w = bit_transpose_step<2, 0x33333333u>(w, lane);
    return bit_transpose_step<1, 0x55555555u>(w, lane);
}

// one half-wave per (column tile, group of 128 users): lane = column fetches word `first column` of the four 32-user groups
// (ubits [plane][group][column]: a coalesced 128-byte read per group and half-wave, duplicates of a column simply read
// another word; the planes of a split group are ORed), four transposes give the mask words of 4 x 32 users
__global__ __launch_bounds__(256) void mask_sweep_kernel(const int32_t* __restrict__ colfirst,
                                                         const uint32_t* __restrict__ ubits, int64_t B, int64_t Bp, int64_t Np,
                                                         int NT, uint32_t* __restrict__ maskW, int planes) {
    const int lane = mf_lane(), c = lane & 31, h = lane >> 5;
    const int ngrp = (int)(Bp >> 7);
    const int64_t unit = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + h;
    if (unit >= (int64_t)NT * ngrp) return;
    const int tj = (int)(unit / ngrp), g = (int)(unit % ngrp);
    const int32_t f = colfirst[tj * 32 + c];                 // -1: padding column, never a negative
    uint32_t in[4] = {~0u, ~0u, ~0u, ~0u};
    if (f >= 0) {
        const int64_t plane_words = (Bp >> 5) * Np;
#pragma unroll
        for (int q = 0; q < 4; ++q) in[q] = ubits[((int64_t)4 * g + q) * Np + f];
        for (int pl = 1; pl < planes; ++pl) {
#pragma unroll
            for (int q = 0; q < 4; ++q) in[q] |= ubits[pl * plane_words + ((int64_t)4 * g + q) * Np + f];
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t word = bit_transpose32(in[q], c);
        const int64_t i = ((int64_t)4 * g + q) * 32 + c;
        maskW[(int64_t)tj * Bp + i] = i < B ? word : ~0u;    // padding users: no negatives at all
    }
}

// ------------------------------------------------------------ host launchers ---
// what mf_negative_masks clears with memsets; the forward and mf_loss_masks* do it inside prep_kernel (loss_clear_tables)
static void clear_mask_tables(const LossWs& w, hipStream_t s) {
    (void)hipMemsetAsync(w.gtab, 0x80, (size_t)w.M * 8, s);
    (void)hipMemsetAsync(w.gfirst, 0x7f, (size_t)w.M * 4, s);
    (void)hipMemsetAsync(w.bmap, 0, (size_t)4 << (w.bmbits - 5), s);
}

// pieces a group's flat list range is cut into (= planes of ubits in use): CSR lists are heavy-tailed and unknown to the
// host -> two; padded lists by their width (P = 64: one piece)
static int hits_split(const PosSrc& src) {
    if (src.pos_off) return 2;
    const int per_group = 32 * (src.P + 1);
    int sp = (per_group + 16383) / 16384;
    return sp < 1 ? 1 : (sp > HITS_MAX_SPLIT ? HITS_MAX_SPLIT : sp);
}

// expects gtab / gfirst / bmap cleared (ubits needs no clearing: every word in use is written)
int loss_build_masks(const LossWs& w, const int64_t* item_idx, const PosSrc& src, hipStream_t s, bool sweep) {
    const int64_t B = w.B, N = w.N;
    gt_insert_kernel<<<dim3((unsigned)((N + 63) / 64)), 64, 0, s>>>(item_idx, N, w.M, w.gtab, w.gfirst, w.colslot, w.bmap, w.bmbits);
    const int split = hits_split(src);
    const int nb_col = (int)((w.Np + HITS_THREADS - 1) / HITS_THREADS);
    const int nb_u = (int)(w.Bp / 32) * split;               // (padding groups too: their rows are read by the sweep)
    const int win = (int)(w.Np < HITS_WIN ? w.Np : HITS_WIN);
    const size_t lds = (size_t)win * 4 + ((size_t)4 << (w.bmbits - 5));
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)hits_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, HITS_WIN * 4 + (4 << 12));
        attr_set = true;
    }
    hits_kernel<<<dim3((unsigned)(nb_col + nb_u)), HITS_THREADS, lds, s>>>(item_idx, src, B, N, w.Bp, w.Np, w.M, nb_col, split, win, w.gtab,
                                                                           w.gfirst, w.colslot, w.colfirst, w.ubits, w.bmap, w.bmbits);
    if (sweep) loss_sweep_masks(w, w.colfirst, split, s);
    return split;
}

void loss_sweep_masks(const LossWs& w, const int32_t* first, int planes, hipStream_t s) {
    const int64_t units = (int64_t)w.NT * (w.Bp >> 7);
    mask_sweep_kernel<<<dim3((unsigned)((units + 7) / 8)), 256, 0, s>>>(first, w.ubits, w.B, w.Bp, w.Np, w.NT, w.maskW, planes);
}

// The hit masks depend on the batch's ids only: built ahead of the forward (on another stream, beside the
// tower gathers) they leave its critical path.  Fills ws's maskW; the forward is then called with
// item_idx = NULL ("masks are in ws").
static int loss_masks_impl(const char* what, int64_t B, int64_t N, int d, int num_negatives, const int64_t* item_idx, const PosSrc& src,
                           void* ws, size_t ws_bytes, mf_stream_t stream) {
    if (int rc = loss_check_shape(what, B, N, d, item_idx && ws, false)) return rc;
    if (ws_bytes < mf_loss_ws_bytes(B, N, d, 0, num_negatives)) return mf_set_error(MF_ENOSPC, "%s: workspace too small", what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const LossWs w = loss_ws(ws, B, N, d, num_negatives);
    loss_clear_tables(w, s);
    loss_build_masks(w, item_idx, src, s);
    return mf_check_launch(what);
}

extern "C" int mf_loss_masks(int64_t B, int64_t N, int d, int P, int num_negatives, const int64_t* item_idx,
                             const int64_t* pos_idx, void* ws, size_t ws_bytes, mf_stream_t stream) {
    const PosSrc src{pos_idx, P, nullptr, nullptr, nullptr, 0};
    if (int rc = pos_src_check("mf_loss_masks", src)) return rc;
    return loss_masks_impl("mf_loss_masks", B, N, d, num_negatives, item_idx, src, ws, ws_bytes, stream);
}

extern "C" int mf_loss_masks_csr(int64_t B, int64_t N, int d, int num_negatives, const int64_t* item_idx, const int64_t* user_ids,
                                 const int64_t* pos_off, const int64_t* pos_items, int64_t num_users, void* ws, size_t ws_bytes,
                                 mf_stream_t stream) {
    const PosSrc src{nullptr, 0, user_ids, pos_off, pos_items, num_users};
    if (!pos_off) return mf_set_error(MF_EINVAL, "mf_loss_masks_csr: pos_off is NULL");
    if (int rc = pos_src_check("mf_loss_masks_csr", src)) return rc;
    return loss_masks_impl("mf_loss_masks_csr", B, N, d, num_negatives, item_idx, src, ws, ws_bytes, stream);
}

// ------------------------------------------------------ public mask helper ----
// API parity with the reference's EmbeddingLoss.negative_masks (losses.py:92-110) on caller-provided tensors (its mining
// methods on a materialised logits matrix: mf_mine_logits, mf_loss_mined.hip).  Not the hot path.
__global__ __launch_bounds__(256) void mask_export_bool_kernel(const uint32_t* __restrict__ maskW, int64_t B, int64_t N,
                                                               int64_t Bp, uint8_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= B * N) return;
    const int64_t i = t / N, j = t % N;
    out[t] = ((maskW[(j >> 5) * Bp + i] >> (j & 31)) & 1u) ? 0 : 1;
}

extern "C" size_t mf_negative_masks_ws_bytes(int64_t B, int64_t N, int P) { return mf_loss_ws_bytes(B, N, 32, P, 1); }

extern "C" int mf_negative_masks(int64_t B, int64_t N, int P, const int64_t* item_idx, const int64_t* pos_idx, void* ws,
                                 size_t ws_bytes, uint8_t* out_mask, mf_stream_t stream) {
    if (int rc = loss_check_shape("mf_negative_masks", B, N, 32, P >= 0 && item_idx && ws && out_mask && (P == 0 || pos_idx), false)) return rc;
    if (ws_bytes < mf_negative_masks_ws_bytes(B, N, P)) return mf_set_error(MF_ENOSPC, "mf_negative_masks: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const LossWs w = loss_ws(ws, B, N, 32, 1);
    const PosSrc src{pos_idx, P, nullptr, nullptr, nullptr, 0};
    clear_mask_tables(w, s);
    loss_build_masks(w, item_idx, src, s);
    mask_export_bool_kernel<<<dim3((unsigned)((B * N + 255) / 256)), 256, 0, s>>>(w.maskW, B, N, w.Bp, out_mask);
    return mf_check_launch("mf_negative_masks");
}
