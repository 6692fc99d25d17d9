// mf_loss_ws.h -- what the units of the loss share: the workspace layout, the shape check, where a user's positives come
// from, and the few HOST functions one unit calls in another.
//
// The loss is cut by stage, and a kernel is launched from the file that defines it (no relocatable device code):
//   mf_loss.hip        per-call set-up (prep_kernel), the tail (finish / rowc / diag_bwd), argument checks, and the two
//                      orchestration functions, which read as a sequence of the stage calls declared at the end of this file
//   mf_loss_masks.hip  the hit masks: hash table, hits, mask sweep; mf_loss_masks*, mf_negative_masks
//   mf_loss_dense.hip  the dense forward, dU and dV sweeps, their split sums, the distinct-column plan's launches and switch
//   mf_loss_mined.hip  the mined path: candidate search (fp32, or through the bf16 prefilter), row top-k, sparse backward
// Process-wide switches live in the unit that owns them (the prefilter mode in mf_loss_mined.hip, the distinct-column mode
// and its per-workspace record in mf_loss_dense.hip): nothing here is a variable.
#pragma once

#include "mf_bf_split.h"
#include "mf_common.h"
#include "mf_loss_cols.h"
#include "mf_loss_math.h"
#include "mf_mine_bf.h"
#include "mf_select.h"
#include "mf_stream.h"

static inline int need_flags(int kind_mask) {
    int f = 0;
    if (kind_mask & ((1 << MF_CONTRASTIVE) | (1 << MF_ALIGNMENT_CONTRASTIVE))) f |= NEED_CONTR;
    if (kind_mask & ((1 << MF_INFONCE) | (1 << MF_MINE))) f |= NEED_LSE;
    if (kind_mask & (1 << MF_PAIRWISE_HINGE)) f |= NEED_HINGE;
    if (kind_mask & (1 << MF_PAIRWISE_LOGISTIC)) f |= NEED_LOGI;
    return f;
}

// ------------------------------------------------------------------ workspace --
struct LossWs {
    int64_t B, N, Bp, Np;
    int BT, NT, d;
    bool mined;
    int nsplit_f, tps_f;          // dense fwd: item-range splits
    int nsplit_u, tps_u;          // dU pass: item-range splits
    int nsplit_v, tps_v;          // dV pass: user-range splits
    int NW;                       // waves per workgroup of the sweeps (mf_nw(d))
    SelectPlan plan;
    float *nu, *nv, *lii, *dii, *sgn, *logq;      // logq: zero-padded NEGATED copy (-logq_j)
    float* tgt;                                  // fp32 copy of the targets (the forward may receive int64)
    long long* gtab;
    int M;
    int32_t *colslot, *gfirst, *colfirst;
    uint32_t* bmap;               // "some column carries an id hashing here": 2^bmbits bits, the positives' prefilter
    int bmbits;
    uint32_t* ubits;
    uint32_t* maskW;
    float *part, *stats, *rowloss, *rowc, *dpart, *rpart, *dpart_v, *rpart_v, *stash, *gstash, *blockpart;
    unsigned* ticket;
    unsigned long long *cand, *priv, *seeds;
    int32_t *cand_cnt, *sel, *sel_cnt;
    unsigned* gtau;
    float* sel_L;
    MineBfPlan mbf;              // the split-bf16 candidate search (mf_mine_bf.h); its arrays exist whenever the shape is eligible
    unsigned short* mbf_plane;
    void* mbf_ufrag;
    void* mbf_rowk;
    int32_t* mbf_flag;
    unsigned* mbf_max;
    unsigned long long* mbf_copybits;
    int32_t *mbf_lastcopy, *mbf_rep, *mbf_spill_cnt, *mbf_gate;
    uint32_t* mbf_spill;
    uint32_t* mbf_plist;
    uint32_t* mbf_pcnt;
    long long* dvfix;            // mined backward: exact fixed-point accumulator of dv [N][d]
    float* dvsc;                 // its unit for this batch: {2^E, clamp, 2^-E} (dv_fix_of, mf_loss_math.h)
    // the column plan (mf_loss_cols.h; dense path at d = 128): geometry words, the plan's scratch, the packed side arrays
    bool cols_ok;                // the shape can be served by the distinct-column sweeps
    ColsLaunch cl;               // what those sweeps launch, whatever N' is
    int wgs_f, wgs_b;            // workgroups the forward / the backward sweeps aim at
    int32_t *geo, *ckept, *ccnt, *ctcnt, *crank, *cfirst;
    float *cv, *cnv, *clq, *cw;
    // the split backward sweeps (mf_bf_split.h; dense path at d = 128): the bf16 piece images of u and of v (or the packed v')
    bool split_ok;               // the shape can be served by them
    unsigned short *bimg_u, *bimg_v;
    size_t total;
};

#ifndef BWD_MIN_WG
#define BWD_MIN_WG 2      // A/B knob: workgroups per CU the backward sweeps are compiled for at d = 128 ...
#define BWD_WGS 512       // ... and their grid size
#endif

static inline bool mining_on(int num_negatives, int64_t N) { return num_negatives > 0 && num_negatives < N; }

static inline LossWs loss_ws(void* base, int64_t B, int64_t N, int d, int num_negatives) {
    LossWs w{};
    w.B = B; w.N = N; w.d = d;
    const int XB = 32 * mf_nw(d);                                 // X rows per workgroup of the sweeps
    w.Bp = (B + XB - 1) / XB * XB; w.Np = (N + XB - 1) / XB * XB;
    w.NW = mf_nw(d);
    w.BT = (int)(w.Bp / 32); w.NT = (int)(w.Np / 32);
    w.mined = mining_on(num_negatives, N);
    // enough workgroups for two waves per SIMD: 256 of eight waves, 512 of four
    const int wgs = 2048 / w.NW;
    w.wgs_f = wgs; w.wgs_b = d == 128 ? BWD_WGS : wgs;
    split_geometry(w.BT / w.NW, w.NT, &w.nsplit_f, &w.tps_f, w.wgs_f);
    split_geometry(w.BT / w.NW, w.NT, &w.nsplit_u, &w.tps_u, w.wgs_b);
    split_geometry(w.NT / w.NW, w.BT, &w.nsplit_v, &w.tps_v, w.wgs_b);
    // (a sweep's buffer descriptor may have to cover the whole streamed operand: tiles per split are only known on the device)
    w.cols_ok = !w.mined && d == 128 && (size_t)w.Np * d * 4 <= MF_SRD_MAX_BYTES;
    w.cl = cols_launch(w.BT, w.NT, w.NW, w.wgs_f, w.wgs_b);
    // (as above: a sweep's descriptor may have to cover the whole image of its streamed operand, 24 KiB per tile)
    w.split_ok = !w.mined && d == 128 && (size_t)w.NT * BSI_TILEB <= MF_SRD_MAX_BYTES;
    const int k = num_negatives;
    w.plan = mf_select_plan(B, N, d, k);
    MfArena a(base);
    w.geo = a.take<int32_t>(CG_WORDS);                            // (first: mf_loss_cols_info finds it without the shape)
    w.nu = a.take<float>(w.Bp); w.nv = a.take<float>(w.Np);
    w.lii = a.take<float>(w.Bp); w.dii = a.take<float>(w.Bp); w.sgn = a.take<float>(w.Bp);
    w.logq = a.take<float>(w.Np);
    w.tgt = a.take<float>(w.Bp);
    w.M = 64;
    while (w.M < 2 * w.Np) w.M *= 2;
    w.gtab = a.take<long long>((size_t)w.M);
    w.gfirst = a.take<int32_t>((size_t)w.M);
    w.colslot = a.take<int32_t>((size_t)w.Np);
    w.colfirst = a.take<int32_t>((size_t)w.Np);
    w.bmbits = 13;                                                // >= 8 bits per column, 1 KiB .. 16 KiB (every block copies it into LDS)
    while (w.bmbits < 17 && (1ll << w.bmbits) < 8 * w.Np) ++w.bmbits;
    w.bmap = a.take<uint32_t>((size_t)1 << (w.bmbits - 5));
    w.ubits = a.take<uint32_t>((size_t)HITS_PLANES * w.Np * (w.Bp / 32));        // ubits [plane][user / 32][column]
    w.maskW = a.take<uint32_t>((size_t)w.NT * w.Bp);
    // (the distinct-column sweeps are launched for the most splits any N' <= N can ask for: >= the uncompacted ones)
    w.part = a.take<float>((size_t)(w.cols_ok ? w.cl.grid_f : w.nsplit_f) * NSTAT * w.Bp);
    w.stats = a.take<float>((size_t)NSTAT * w.Bp);
    w.rowloss = a.take<float>((size_t)MF_NUM_KINDS * w.Bp);
    w.rowc = a.take<float>((size_t)4 * w.Bp);
    w.blockpart = a.take<float>((size_t)MF_NUM_KINDS * (w.Bp / 64 + 1));
    w.ticket = a.take<unsigned>(4);
    w.dvsc = a.take<float>(4);
    if (w.mined) {
        w.cand = a.take<unsigned long long>((size_t)w.Bp * w.plan.rowcap);
        w.priv = a.take<unsigned long long>((size_t)w.plan.nsets * w.Bp * w.plan.CAP);
        w.seeds = a.take<unsigned long long>((size_t)w.Bp * (w.plan.seeds_per_row > 0 ? w.plan.seeds_per_row : 1));
        w.sel = a.take<int32_t>((size_t)w.Bp * KSEL_MAX);
        w.sel_cnt = a.take<int32_t>(w.Bp);
        w.sel_L = a.take<float>((size_t)w.Bp * KSEL_MAX);
        w.dvfix = a.take<long long>((size_t)w.N * d);
        w.gtau = a.take<unsigned>((size_t)w.Bp);
        w.cand_cnt = a.take<int32_t>((size_t)w.Bp);      // right behind gtau: one memset clears both
        w.mbf_max = a.take<unsigned>(MBF_MAXSLOTS * MBF_MAXSTRIDE);  // ... and these maxima
        w.mbf = mine_bf_plan(B, N, d, k);
        if (w.mbf.ok) {
            w.mbf_copybits = a.take<unsigned long long>((size_t)w.mbf.Nq);        // (cleared with the maxima, and the next)
            w.mbf_lastcopy = a.take<int32_t>((size_t)w.mbf.Nq);
            w.mbf_spill_cnt = a.take<int32_t>((size_t)w.mbf.Xq);
            w.mbf_gate = a.take<int32_t>(4);                             // (the cleared range ends here)
            w.mbf_rep = a.take<int32_t>((size_t)w.mbf.Nq);
            w.mbf_spill = a.take<uint32_t>((size_t)w.mbf.Xq * MBF_SPILL);
            w.mbf_plane = a.take<unsigned short>((size_t)w.mbf.Nq * (2 * d + 16) + 64);
            w.mbf_ufrag = a.take<char>((size_t)w.mbf.Xq * d * 4);
            w.mbf_rowk = a.take<char>((size_t)w.mbf.Xq * 16);
            w.mbf_flag = a.take<int32_t>((size_t)w.mbf.Xq);
            w.mbf_plist = a.take<uint32_t>((size_t)w.mbf.nchunk * w.mbf.Xq * w.mbf.lpc * MBF_CAPL);
            w.mbf_pcnt = a.take<uint32_t>((size_t)w.mbf.nchunk * w.mbf.Xq);
        }
        w.dpart = nullptr;
    } else {
        // the two backward sweeps keep their split partials apart: ONE launch adds up both after the second sweep
        size_t rows = (size_t)w.nsplit_u * w.Bp, rows_v = (size_t)w.nsplit_v * w.Np;
        if (w.cols_ok) {
            // the partials are sized by LAUNCHED workgroups (each writes one X block of 32 NW rows), not by nsplit x padded rows
            const size_t xb = (size_t)32 * w.NW;
            rows = (size_t)w.cl.grid_u * w.Bp;
            if ((size_t)w.cl.grid_v * xb > rows_v) rows_v = (size_t)w.cl.grid_v * xb;
            w.ckept = a.take<int32_t>((size_t)w.Np);
            w.ccnt = a.take<int32_t>((size_t)w.Np);
            w.ctcnt = a.take<int32_t>((size_t)w.NT);
            w.crank = a.take<int32_t>((size_t)w.Np);
            w.cfirst = a.take<int32_t>((size_t)w.Np);
            w.cnv = a.take<float>((size_t)w.Np);
            w.clq = a.take<float>((size_t)w.Np);
            w.cw = a.take<float>((size_t)w.Np);
            w.cv = a.take<float>((size_t)w.Np * d);
        }
        w.dpart = a.take<float>(rows * d);
        w.rpart = a.take<float>(rows);
        w.dpart_v = a.take<float>(rows_v * d);
        w.rpart_v = a.take<float>(rows_v);
        w.stash = a.take<float>((size_t)w.Bp * w.Np);
        w.gstash = a.take<float>((size_t)w.Bp * w.Np);
        if (w.split_ok) {
            // A backward either runs the split sweeps, which keep no G' stash (dV derives G' itself), or the fp32 sweeps, which
            // read no image; both are rebuilt by every backward.  So the images live in the G' stash wherever they fit (24 KiB
            // per tile against 4 KiB per pair of tiles: from a few hundred rows on) and the workspace grows for tiny shapes only.
            const size_t nu = (size_t)w.BT * BSI_TILE_ELEMS, nv = (size_t)w.NT * BSI_TILE_ELEMS;
            if ((nu + nv) * sizeof(unsigned short) <= (size_t)w.Bp * w.Np * sizeof(float)) {
                w.bimg_u = reinterpret_cast<unsigned short*>(w.gstash);
                w.bimg_v = w.gstash ? w.bimg_u + nu : nullptr;
            } else {
                w.bimg_u = a.take<unsigned short>(nu);
                w.bimg_v = a.take<unsigned short>(nv);
            }
        }
    }
    w.total = a.used();
    return w;
}

// Where a user's positives come from: the reference's padded matrix pos_idx[B][P] (0-padded on the right,
// data/load.py:38-55; the zeros are looked up like any id: they match a column whose item id is 0, as upstream), or the
// batch producer's own CSR lists -- user_ids[i]'s items are pos_items[pos_off[u] .. pos_off[u + 1]) -- which never
// materialises a [B, P] tensor: a MovieLens-25M user can hold > 10^4 positives.
struct PosSrc {
    const int64_t* pos_idx; int P;
    const int64_t *user_ids, *pos_off, *pos_items; int64_t num_users;
};
__device__ __forceinline__ int pos_list(const PosSrc& s, int64_t i, const int64_t*& base) {
    if (s.pos_off) {
        const int64_t u = s.user_ids[i];
        if (u < 0 || u >= s.num_users) { base = s.pos_items; return 0; }
        const int64_t o = s.pos_off[u];
        base = s.pos_items + o;
        const int64_t len = s.pos_off[u + 1] - o;
        return (int)(len < 0 ? 0 : (len > 0x7FFFFFF ? 0x7FFFFFF : len));
    }
    base = s.pos_idx + i * s.P;
    return s.P;
}

static inline int pos_src_check(const char* what, const PosSrc& src) {
    if (src.pos_off) {
        if (!src.user_ids || !src.pos_items || src.num_users <= 0) return mf_set_error(MF_EINVAL, "%s: CSR positives need user_ids, pos_off, pos_items, num_users > 0", what);
    } else if (src.P < 0 || (src.P > 0 && !src.pos_idx)) {
        return mf_set_error(MF_EINVAL, "%s: bad positives", what);
    }
    return MF_OK;
}

// The one shape check of the loss exports: 0 < B <= N, a supported width, and N < 2^24 (a split holds < 2^19 tiles, a
// scan hit packs its column into 24 bits).  `operands_ok` is the caller's own test of its pointers and counts: it is
// answered between the width and the 2^24 limit, where every export has always answered it.  The forward and the
// backward name what is wrong with the shape (`itemised`); the masks exports say "bad argument" to all of it.
static inline int loss_check_shape(const char* what, int64_t B, int64_t N, int d, bool operands_ok, bool itemised) {
    const bool bn_ok = B > 0 && N >= B;
    if (itemised && !bn_ok) return mf_set_error(MF_EINVAL, "%s: need 0 < B <= N (B=%lld N=%lld)", what, (long long)B, (long long)N);
    if (itemised && !mf_width_ok(d)) return mf_set_error(MF_EINVAL, "%s: embedding width %d not in {32,64,128,256}", what, d);
    if (!bn_ok || !mf_width_ok(d) || !operands_ok) return mf_set_error(MF_EINVAL, "%s: bad argument", what);
    if (N >= (1 << 24)) return mf_set_error(MF_ENOTSUP, "%s: N >= 2^24", what);
    return MF_OK;
}

// ---- the stages: host functions, each in the unit that defines the kernels it launches (all on the caller's stream) ----
// mf_loss.hip: clear the hash table, the first-column table and the membership bitmap (a clears-only prep_kernel)
void loss_clear_tables(const LossWs& w, hipStream_t s);
// mf_loss_masks.hip: the hit masks of these ids into w.maskW (the tables are cleared); returns the planes of w.ubits in use.
// !sweep: stop before the mask words (the column plan sweeps the masks of its packed columns instead) ...
int loss_build_masks(const LossWs& w, const int64_t* item_idx, const PosSrc& src, hipStream_t s, bool sweep = true);
// ... through this: the mask words of the columns whose first columns `first` names
void loss_sweep_masks(const LossWs& w, const int32_t* first, int planes, hipStream_t s);
// mf_loss_dense.hip: does this forward sweep the distinct columns?  Recorded for the backward on the same workspace.
bool dense_fwd_cols(const LossWs& w, const void* ws, bool scores_needed, bool masks_ready, bool export_masks);
// [the column plan,] the score sweep into w.part / w.stash, [the mask export]; *merge_splits: partial sets the tail merges
int dense_fwd(const LossWs& w, const void* ws, bool cols, int planes, const float* u, const float* v, int need, float sigma, float margin,
              uint32_t* out_mask_bits, hipStream_t s, int* merge_splits);
// dU, dV and their split sums, on the path the last forward on `ws` took
int dense_bwd(const LossWs& w, const void* ws, int gmode, const float* u, const float* v, const float* grad_out, float* du,
              float* dv, hipStream_t s);
// a backward that runs no dense sweep (mined, alignment): mf_loss_bwd_path answers 0 for it, not what an earlier one left
void dense_bwd_none(const void* ws);
// mf_loss_mined.hip: candidate search, row top-k into w.sel / w.sel_L / w.stats, [the mask export]
int mined_fwd(const LossWs& w, const float* u, const float* v, int num_negatives, int need, float sigma, float margin,
              uint32_t* out_mask_bits, hipStream_t s);
// du in registers, dv through the fixed-point accumulator
int mined_bwd(const LossWs& w, int gmode, const float* u, const float* v, const float* grad_out, float* du, float* dv,
              hipStream_t s);
