/*
 * mf_hip.h -- C ABI of libmf_hip.so, the gfx950 (MI355X / CDNA4) implementation of
 * the two-tower matrix-factorization hot path.
 *
 * The reference (yxtay/matrix-factorization-torch, package xfmr_rec) is pure Python
 * and has no FFI layer; its boundary for this path is a torch.nn.Module call
 * (SURVEY.md 8b).  Each entry point below names the reference interface it
 * replaces (file:line under /root/reference).  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   * every pointer is a DEVICE pointer (hipMalloc / torch.cuda storage) unless
 *     its name ends in _host; all float data is fp32, all ids are int64;
 *   * matrices are dense row-major, rows 16-byte aligned; the embedding width d
 *     must be one of 32, 64, 128, 256 (callers zero-pad other widths; zero columns
 *     change no value, see mf_numerics.h);
 *   * `stream` is a hipStream_t (NULL = default stream); no entry point allocates,
 *     frees or synchronises -- scratch comes from the caller (`ws`, sized by the
 *     matching *_ws_bytes query), so every call can be captured in a hipGraph;
 *   * return value 0 = ok, otherwise a negative MF_E* code; mf_last_error() gives
 *     the text (thread-local).
 */
#ifndef MF_HIP_H
#define MF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mf_stream_t; /* hipStream_t */

enum {
    MF_OK = 0,
    MF_EINVAL = -1,   /* bad argument (shape, width, NULL pointer) */
    MF_ENOSPC = -2,   /* workspace too small */
    MF_ELAUNCH = -3,  /* HIP launch error */
    MF_ENOTSUP = -4   /* valid request outside the implemented range */
};

/* Loss classes, in the order of get_loss_fns (xfmr_rec/lightning.py:267-287). */
enum mf_loss_kind {
    MF_ALIGNMENT = 0,             /* AlignmentLoss                  losses.py:249-259 */
    MF_CONTRASTIVE = 1,           /* ContrastiveLoss                losses.py:262-274 */
    MF_ALIGNMENT_CONTRASTIVE = 2, /* AlignmentContrastiveLoss       losses.py:277-291 */
    MF_INFONCE = 3,               /* InfomationNoiseContrastive...  losses.py:294-306 */
    MF_MINE = 4,                  /* MutualInformationNeuralEst...  losses.py:309-321 */
    MF_PAIRWISE_HINGE = 5,        /* PairwiseHingeLoss              losses.py:357-359 */
    MF_PAIRWISE_LOGISTIC = 6,     /* PairwiseLogisticLoss           losses.py:352-354 */
    MF_NUM_KINDS = 7
};

const char* mf_last_error(void);
int mf_version(void);

/* Optional HIP-event timing of the dominant kernels ("loss_fwd_dense",
 * "loss_bwd_du", "loss_bwd_dv", "mining_select", "topk_select", "topk_small", "gather_rows",
 * "update_rows"), recorded on the launch stream.  mf_timing_enable(k): 0 = off, k >= 1 = time every
 * k-th launch of each name (an event pair costs a few us of stream time).  mf_timing_get blocks until
 * the recorded spans finished and returns their count (total_ms = summed duration). */
void mf_timing_enable(int every);
void mf_timing_reset(void);
int64_t mf_timing_get(const char* name, double* total_ms);

/* ------------------------------------------------------------------ towers ---
 * Replaces the tower forward `MatrixFactorizationLitModule.forward`
 * (xfmr_rec/lightning.py:60-74: text -> BERT -> mean-pool -> L2-normalise) by an
 * embedding-table row gather (north-star; no reference implementation):
 *   out[r, :] = table[idx[r], :]            (normalize == 0)
 *   out[r, :] = table[idx[r], :] / max(||.||, 1e-12)   (normalize != 0, mirrors
 *               sentence_transformers Normalize, xfmr_rec/models.py:59)
 * out_inv_norm (nullable) receives 1 / max(||row||, 1e-12). */
int mf_gather_rows(const float* table, int64_t n_rows, int d, const int64_t* idx, int64_t n,
                   int normalize, float* out, float* out_inv_norm, mf_stream_t stream);

/* Hash / bloom embedding tower (BASELINE config 5: catalogs too large for one row per id; our spec,
 * mf_numerics.h mf_hash_bucket): id -> num_hashes (1..4) bucket rows of a [num_buckets, d] table,
 *   out[r, :] = sum_j table[bucket_j(idx[r]), :]   (j ascending; then / max(||.||, 1e-12) if normalize)
 * mf_hash_buckets writes the bucket rows themselves, out_buckets[r * num_hashes + j] -- the row ids
 * the sparse update of the table is called with.  mf_normalize_backward turns the gradient w.r.t.
 * the normalised output into the gradient w.r.t. the summed rows (the same for each of the id's
 * rows): graw = (g - u (u . g)) * inv_norm, u = the normalised output row. */
int mf_gather_hashed(const float* table, int64_t num_buckets, int d, const int64_t* idx, int64_t n,
                     int num_hashes, uint64_t seed, int normalize, float* out, float* out_inv_norm,
                     mf_stream_t stream);
int mf_hash_buckets(const int64_t* idx, int64_t n, int num_hashes, uint64_t seed, int64_t num_buckets,
                    int64_t* out_buckets, mf_stream_t stream);
int mf_normalize_backward(const float* out_unit, const float* inv_norm, const float* grad, int64_t n, int d,
                          float* grad_raw, mf_stream_t stream);

/* out[r] = chain-ordered ||x_r||^2 (mf_numerics.h); helper of the loss path. */
int mf_row_sqnorm(const float* x, int64_t n, int d, float* out, mf_stream_t stream);

/* Raw score tile engine exposed for tests: out[i][j] = chain dot(u_i, v_j) computed
 * by the fp32 MFMA path (must equal oracle/chain.c bit for bit). */
int mf_scores(const float* u, int64_t B, const float* v, int64_t N, int d, float* out,
              mf_stream_t stream);

/* --------------------------------------------------------------- batch ids ---
 * Stable sort of n int64 keys (0 <= key < 2^39, n < 2^24): perm[p] = original
 * position of the p-th smallest key, sorted_keys[p] = its key (nullable).
 * Used for duplicate-row handling and for the positive-mask range search that
 * replaces the B x N x P comparison of negative_masks (xfmr_rec/losses.py:108). */
size_t mf_sort_ws_bytes(int64_t n);
int mf_sort_keys(const int64_t* keys, int64_t n, int32_t* perm, int64_t* sorted_keys, void* ws,
                 size_t ws_bytes, mf_stream_t stream);
/* Stable grouping by a SMALL key (0 <= key < nkeys <= 64, n <= 32,768; the owner rank of a routed id, distributed.py): perm
 * and sorted_keys (nullable) as mf_sort_keys, bounds[nkeys + 1] = where each key's group starts.  One launch, one workgroup
 * (a counting sort in LDS); MF_ENOTSUP beyond the limits. */
int mf_group_keys(const int64_t* keys, int64_t n, int nkeys, int32_t* perm, int64_t* sorted_keys, int64_t* bounds,
                  mf_stream_t stream);

/* ------------------------------------------------------------------ losses ---
 * Replaces `EmbeddingLoss.forward` for all seven classes
 * (xfmr_rec/losses.py:39-52; call site xfmr_rec/lightning.py:137-146):
 *   u[B,d] user_embed, v[N,d] item_embed (N >= B; row j < B is the positive of
 *   user j), target[B] (the rating: fp32, or the reference's int64 with MF_LOSS_TARGET_I64),
 *   item_idx[N], pos_idx[B,P] (0-padded, nullable with P = 0), logq (nullable; our logQ
 *   correction L_ij -= logq_j: one value per column, logq[N], when logq_rows = 0, else a
 *   table of logq_rows values looked up by the batch ids, logq_j = logq[item_idx[j]],
 *   ids outside the table counting as 0 -- which needs item_idx != NULL).
 * flags: MF_LOSS_TARGET_I64 (target is int64), MF_LOSS_MASKS_READY (mf_loss_masks already ran on this workspace for
 *   these ids: same as item_idx = NULL, but the ids stay available to a logQ table lookup), MF_LOSS_ROWC (kind_mask has ONE bit set and that
 *   loss will be differentiated: the forward's tail also prepares the backward's per-row
 *   coefficients, and mf_loss_bwd is then called with MF_LOSS_ROWC too and skips that launch).
 * kind_mask selects which losses to evaluate in the one pass (bit k = kind k);
 * out_losses[7] receives them (the entries of the other kinds are set to 0).  The workspace keeps
 * the per-row statistics / mined negatives for mf_loss_bwd and must stay intact
 * between the two calls.  out_mask_bits (nullable, B x ceil(N/32) uint32, bit c of
 * word [i][w] = column 32w+c) receives the post-mining negative mask
 * (negative_masks + semi_hard_mining, losses.py:92-162) for tests.
 * num_negatives follows losses.py:137-141: <= 0 or >= N disables mining.
 * Mining supports num_negatives <= 64 (MF_ENOTSUP beyond).
 *
 * The hit masks (negative_masks, losses.py:92-110) depend on the ids only.  mf_loss_masks builds
 * them into the workspace ahead of time -- typically on a second stream, beside the tower gathers --
 * and the forward is then called with item_idx = NULL on the SAME workspace, after the caller has
 * ordered the two streams (event); with item_idx != NULL mf_loss_fwd builds them itself. */
size_t mf_loss_ws_bytes(int64_t B, int64_t N, int d, int P, int num_negatives);
/* Host-only view of how the dense sweeps split a shape (nothing is launched, no GPU needed): out[8] = {mined (no dense sweep
 * runs), forward splits, tiles per forward split, dU splits, tiles per dU split, dV splits, tiles per dV split, tiles in the
 * LAST split of the three: forward | dU << 20 | dV << 40}.  A tile is 32 columns of the streamed axis (items for the forward
 * and dU, users for dV).  MF_EINVAL for the shapes mf_loss_ws_bytes answers with 0, and for a width outside {32,64,128,256}. */
int mf_loss_plan(int64_t B, int64_t N, int d, int num_negatives, int64_t* out);
int mf_loss_masks(int64_t B, int64_t N, int d, int P, int num_negatives, const int64_t* item_idx,
                  const int64_t* pos_idx, void* ws, size_t ws_bytes, mf_stream_t stream);
/* CSR form of the positives (the batch producer's own lists, mf_sample_batch's pos_off / pos_items): the positives of batch
 * row i are pos_items[pos_off[u] .. pos_off[u + 1]), u = user_ids[i] (a u outside [0, num_users) has none).  No [B, P]
 * tensor exists on this path: the reference pads every batch to its longest list (xfmr_rec/data/lightning.py:274-280,
 * data/load.py:38-55), which for MovieLens-25M means > 10^4 columns.  Same masks, bit for bit, as the padded form of the
 * same lists (order and duplicates inside a list do not matter; lists need not be sorted). */
int mf_loss_masks_csr(int64_t B, int64_t N, int d, int num_negatives, const int64_t* item_idx, const int64_t* user_ids,
                      const int64_t* pos_off, const int64_t* pos_items, int64_t num_users, void* ws, size_t ws_bytes,
                      mf_stream_t stream);
enum { MF_LOSS_TARGET_I64 = 1, MF_LOSS_ROWC = 2, MF_LOSS_MASKS_READY = 4 };
int mf_loss_fwd(int64_t B, int64_t N, int d, int P, int num_negatives, float sigma, float margin,
                int kind_mask, const float* u, const float* v, const void* target,
                const int64_t* item_idx, const int64_t* pos_idx, const float* logq, int64_t logq_rows,
                int flags, void* ws, size_t ws_bytes, float* out_losses, uint32_t* out_mask_bits,
                mf_stream_t stream);

/* mf_loss_fwd with CSR positives (see mf_loss_masks_csr); everything else as above.  mf_loss_ws_bytes(B, N, d, 0, k) sizes ws. */
int mf_loss_fwd_csr(int64_t B, int64_t N, int d, int num_negatives, float sigma, float margin, int kind_mask, const float* u,
                    const float* v, const void* target, const int64_t* item_idx, const int64_t* user_ids, const int64_t* pos_off,
                    const int64_t* pos_items, int64_t num_users, const float* logq, int64_t logq_rows, int flags, void* ws,
                    size_t ws_bytes, float* out_losses, uint32_t* out_mask_bits, mf_stream_t stream);

/* Backward of one loss of the preceding mf_loss_fwd (same shapes/hyper-parameters,
 * same ws): du[B,d] = grad_out * dloss/du, dv[N,d] = grad_out * dloss/dv, with
 * grad_out a device scalar.  Masks and mining are constants of the backward
 * (@torch.no_grad in the reference, losses.py:92,134).  The targets and logQ values are the
 * workspace's copies of the forward's.  flags: MF_LOSS_ROWC as above. */
int mf_loss_bwd(int64_t B, int64_t N, int d, int P, int num_negatives, float sigma, float margin,
                int kind, const float* u, const float* v, int flags, void* ws, size_t ws_bytes,
                const float* grad_out, float* du, float* dv, mf_stream_t stream);

/* The candidate search of the mined losses (0 < num_negatives < N) has two implementations with IDENTICAL results: the fp32
 * streaming selection, and a split-bf16 prefilter on the bf16 matrix cores with exact fp32 rescoring of the few columns that
 * pass (csrc/mf_mine_bf.h; it can serve d in {64, 128}, B >= 256, N >= 2048, num_negatives <= 32).  mode 1 (default): the
 * prefilter where it is the faster one (B >= 4096); mode 2: wherever it can serve (what the parity tests use
 * to compare the two on small shapes); mode 0: the fp32 search everywhere.  MF_MINE_BF=0|1|2 in the environment sets the initial
 * mode.  Process-wide; not a per-stream setting. */
void mf_set_mining_prefilter(int mode);
/* The dense (unmined) losses at d = 128 sweep each DISTINCT item column of the batch once, weighted by its copy count
 * (csrc/mf_loss_cols.h): column j is a copy of the first column f with its item id iff v[j] equals v[f] and logq[j] equals
 * logq[f] bit for bit -- decided on the values, on the device, per batch.  Loss and gradients hold to the tolerances of the
 * uncompacted sweeps, not to their bits (each distinct column is summed once with a weight).  mode 1 (default): from 4096
 * columns upward; mode 2: wherever it can serve (tests); mode 0: never.  Not served, and bit for bit as before: every other
 * width, the mined losses, masks prepared by mf_loss_masks, a forward that exports its mask.  A backward follows the path
 * its forward took on that workspace, whatever the mode is by then.  Process-wide. */
void mf_set_dense_dedup(int mode);
/* Tests and tools only (a device -> host copy; never inside a step): out[9] = {served, N' (distinct columns), NT' (tiles
 * streamed), forward (splits, tiles per split), dU (the same), dV (the same)} of the last forward on this workspace. */
int mf_loss_cols_info(const void* ws, int64_t* out);
/* The two backward sweeps of the dense losses at d = 128 contract on the bf16 matrix cores with fp32-grade results: both
 * operands are split into three bf16 pieces and the six leading piece products are accumulated in fp32 (csrc/mf_bf_split.h;
 * dropped terms ~2^-23 of a product).  The gradients hold to the tolerances of the fp32 sweeps, not to their bits; this
 * switch does not reach the forward, which has its own (mf_set_dense_fwd_split), and a backward reads the logit stash
 * whichever way its forward filled it.  mode 1 (default): from 8192 columns upward; mode 2: wherever d = 128
 * (tests); mode 0: never.  Served with and without the distinct-column plan; not served: every other width, the mined
 * losses.  Read at each backward.  Process-wide. */
void mf_set_dense_bwd_split(int mode);
/* The forward sweep of the dense losses at d = 128 computes its score tiles the same way (three bf16 pieces of both operands,
 * six piece products, fp32 accumulation): loss, logit stash and everything downstream hold to the tolerances of the fp32
 * forward, not to its bits.  mode 1 (default): from 2048 x 4096 scores (B x N) upward; mode 2: wherever d = 128 and the loss is dense
 * (tests); mode 0: never.  Not served, and bit for bit as before: every other width, the mined losses, the one-launch small
 * step.  Read at each forward.  Process-wide. */
void mf_set_dense_fwd_split(int mode);
/* Tests and tools only: the path of the last mf_loss_fwd on this workspace -- bit 0: distinct columns, bit 1: split scores.
 * 0 for a workspace no forward has run on, and after a forward that runs no dense sweep. */
int mf_loss_fwd_path(const void* ws);
/* Tests only: the slot of (row of a 32-row tile, feature, piece) among the 12,288 bf16 of a tile's FORWARD operand image
 * (csrc/mf_bf_split.h); -1 outside 32 x 128 x 3. */
int mf_fwd_split_image_index(int row, int feature, int piece);
/* Tests and tools only: the path of the last mf_loss_bwd on this workspace -- bit 0: distinct columns, bit 1: split
 * contraction, bit 2: dV derived G' from the logit stash itself.  0 for a workspace no backward has run on, and after a
 * backward that runs no dense sweep (a mined loss, the alignment loss). */
int mf_loss_bwd_path(const void* ws);
/* Tests only: the slot of (row of a 32-row tile, feature, piece) among the 12,288 bf16 of a tile's operand image
 * (csrc/mf_bf_split.h); -1 outside 32 x 128 x 3. */
int mf_bwd_split_image_index(int row, int feature, int piece);
/* Host-only: the geometry the device derives for `ncols` distinct columns of a shape, with what is launched and allocated
 * around it: out[16] = {can serve, NT', forward (splits, tps), dU (splits, tps), dV (splits, tps), dV X blocks, launched:
 * forward splits, dU splits, dV workgroups, capacity of the partial buffers: forward splits, dU splits, dV X blocks, 0}.
 * With ncols = N the geometry is mf_loss_plan's. */
int mf_loss_cols_plan(int64_t B, int64_t N, int d, int64_t ncols, int64_t* out);
/* Host-only view of the prefilter's plan for a shape (nothing is launched, no GPU needed): out[8] = {ok (it can serve the
 * shape), pays (mode 1 uses it), item chunks, tiles per chunk, rescoring lanes per chunk, lists per user, capacity of the
 * rescoring wave's key array, its LDS bytes}.  d outside {64, 128}: ok = 0 and the last two are 0. */
int mf_mining_prefilter_plan(int64_t B, int64_t N, int d, int k, int64_t* out);

/* API parity with the public helper methods of EmbeddingLoss, on caller-provided tensors (not the
 * hot path): negative_masks (losses.py:92-110) -> out_mask[B,N] bytes, 1 = valid negative;
 * hard_mining (losses.py:112-132, semi_hard = 0: keep the k highest logits among the valid
 * negatives) and semi_hard_mining (losses.py:134-162, semi_hard = 1) on a MATERIALISED logits[B,N]
 * matrix, mask[B,N] bytes updated in place; k <= 0 or k >= N leaves it unchanged.  Any k. */
size_t mf_negative_masks_ws_bytes(int64_t B, int64_t N, int P);
int mf_negative_masks(int64_t B, int64_t N, int P, const int64_t* item_idx, const int64_t* pos_idx, void* ws,
                      size_t ws_bytes, uint8_t* out_mask, mf_stream_t stream);
int mf_mine_logits(const float* logits, int64_t B, int64_t N, int k, int semi_hard, uint8_t* mask,
                   mf_stream_t stream);

/* --------------------------------------------------------------- optimiser ---
 * Replaces `configure_optimizers` (xfmr_rec/lightning.py:238-239, dense AdamW) by
 * sparse row updates of an embedding table (north-star; our spec):
 * duplicate ids are summed first (batch order), then each touched row is updated
 * once.  `normalized` != 0 means grad is w.r.t. the L2-normalised row and is first
 * mapped through the normalisation Jacobian of the raw row.
 *   sgd : row -= lr * (g + wd * row)
 *   adam: lazy row-wise AdamW (moments of touched rows only, global step for the
 *         bias correction, decoupled weight decay).  The step (1-based) comes by value, or --
 *         step_dev != NULL -- from device memory: a launch captured in a hipGraph freezes its
 *         by-value arguments, a device counter bumped inside the graph keeps counting.  Either
 *         way the bias corrections are evaluated on the device: eager and replayed steps agree
 *         bit for bit. */
size_t mf_update_ws_bytes(int64_t n, int d);
int mf_update_sgd(float* table, int64_t n_rows, int d, const int64_t* idx, int64_t n,
                  const float* grad, int normalized, float lr, float weight_decay, void* ws,
                  size_t ws_bytes, mf_stream_t stream);
int mf_update_adam(float* table, float* exp_avg, float* exp_avg_sq, int64_t n_rows, int d,
                   const int64_t* idx, int64_t n, const float* grad, int normalized, int64_t step,
                   const int64_t* step_dev, float lr, float beta1, float beta2, float eps,
                   float weight_decay, void* ws, size_t ws_bytes, mf_stream_t stream);

/* Both tables of a training step -- the user rows and the item rows touched by one batch (xfmr_rec/lightning.py:189-192: one
 * optimizer.step() per step covers every parameter) -- in ONE launch: the two sparse updates are independent, so their
 * workgroups run side by side.  Same arithmetic, same results as two mf_update_sgd / mf_update_adam calls (adam = 0 / 1), the same
 * hyper-parameters for both tables, one workspace each (mf_update_ws_bytes).  MF_ENOTSUP for lists longer than 65,536 ids or empty
 * ones: callers then update the tables one by one. */
int mf_update_pair(int adam, int d, float* table_a, float* exp_avg_a, float* exp_avg_sq_a, int64_t n_rows_a, const int64_t* idx_a,
                   int64_t n_a, const float* grad_a, int normalized_a, void* ws_a, size_t ws_a_bytes, float* table_b,
                   float* exp_avg_b, float* exp_avg_sq_b, int64_t n_rows_b, const int64_t* idx_b, int64_t n_b, const float* grad_b,
                   int normalized_b, void* ws_b, size_t ws_b_bytes, int64_t step, const int64_t* step_dev, float lr, float beta1,
                   float beta2, float eps, float weight_decay, mf_stream_t stream);

/* Row-wise Adagrad (the "exact row-wise Adagrad" of FBGEMM / torchrec; no reference implementation, our spec: DESIGN.md 2): ONE
 * fp32 of state per row, `sum` [n_rows], instead of Adam's two moment tables.  With acc the row's summed gradient (summed exactly as
 * for sgd / adam), w the row of stored width d, s = sum[row], all in fp32:
 *   g = acc                               (normalized == 0; else the normalisation Jacobian, as for sgd / adam)
 *   g = g + weight_decay * w              (coupled L2; skipped as a whole when weight_decay == 0)
 *   s = s + (1/d) * sum_c g_c^2           (the mean runs over the STORED width: zero padding channels dilute it)
 *   w = w - lr * g / (sqrtf(s) + eps)
 * No step counter, no lr decay: nothing depends on the step number, so a launch captured in a hipGraph replays as it is.
 * MF_EINVAL for sum == NULL, lr < 0, eps <= 0, weight_decay < 0 (and what mf_update_sgd refuses); workspace: mf_update_ws_bytes.
 * mf_update_pair_adagrad: both tables of a step in ONE launch, like mf_update_pair (1..65,536 ids per table, one width, one set of
 * hyper-parameters; MF_ENOTSUP otherwise); same results as two mf_update_adagrad calls. */
int mf_update_adagrad(float* table, float* sum, int64_t n_rows, int d, const int64_t* idx, int64_t n, const float* grad,
                      int normalized, float lr, float eps, float weight_decay, void* ws, size_t ws_bytes, mf_stream_t stream);
int mf_update_pair_adagrad(int d, float* table_a, float* sum_a, int64_t n_rows_a, const int64_t* idx_a, int64_t n_a,
                           const float* grad_a, int normalized_a, void* ws_a, size_t ws_a_bytes, float* table_b, float* sum_b,
                           int64_t n_rows_b, const int64_t* idx_b, int64_t n_b, const float* grad_b, int normalized_b, void* ws_b,
                           size_t ws_b_bytes, float lr, float eps, float weight_decay, mf_stream_t stream);

/* -------------------------------------------------- the default step in one launch ---
 * The reference trains with BATCH_SIZE = 32 pairs (xfmr_rec/params.py:18), PairwiseHingeLoss and 4 mined negatives
 * (xfmr_rec/lightning.py:38-39): a step of ~0.5 MFLOP that the multi-kernel path spends in launch latency.  mf_step_small
 * runs the WHOLE training step -- mf_gather_rows of both towers, mf_loss_fwd (all kinds of kind_mask into out_losses[7]),
 * mf_loss_bwd of `kind` with upstream gradient 1, mf_update_sgd / mf_update_adam of both tables -- in ONE workgroup and one
 * launch, for B <= 128 pairs, N <= 256 columns, tables of < 2^36 rows and a mined loss (0 < num_negatives <= 64, < N).  Results (losses, both
 * tables, Adam moments) are bit-identical to that sequence of calls.  Positives: padded pos_idx[B, P], or -- pos_off != NULL --
 * CSR lists indexed by user_ids (see mf_loss_fwd_csr).  adam = 0: SGD (lr, weight_decay); else lazy row-wise AdamW with the
 * global step by value or from step_dev.  MF_ENOTSUP for shapes / losses outside that range (callers fall back). */
size_t mf_step_small_ws_bytes(int d);
int mf_step_small(float* user_table, float* user_m, float* user_v, int64_t num_users, float* item_table, float* item_m,
                  float* item_v, int64_t num_items, int d, int normalize, const int64_t* user_ids, const int64_t* item_ids,
                  const void* target, int target_i64, const int64_t* pos_idx, int P, const int64_t* pos_off,
                  const int64_t* pos_items, int64_t pos_users, int64_t B, int64_t N, int kind, int kind_mask, int num_negatives,
                  float sigma, float margin, const float* logq, int64_t logq_rows, int adam, int64_t step, const int64_t* step_dev,
                  float lr, float beta1, float beta2, float eps, float weight_decay, void* ws, size_t ws_bytes, float* out_losses,
                  mf_stream_t stream);

/* --------------------------------------------------------------- retrieval ---
 * Replaces `ItemProcessor.search` (xfmr_rec/data/lightning.py:237-259; LanceDB
 * cosine ANN with prefilter) by EXACT brute-force top-k over the indexed item
 * matrix: score = chain dot(q, item) (= 1 - cosine distance for unit-norm rows),
 * exclusion prefilter by per-query id lists (CSR: excl_off[Q+1], excl_idx[],
 * GLOBAL item row indices in any order; both nullable), best first, ties by lowest
 * item index.  `idx_base` is the global index of items[0] (row-sharded catalogs).
 * out_scores[Q,k] fp32, out_idx[Q,k] int64 global indices (-1 / -inf padding when
 * fewer than k candidates).  k <= 64 (deeper lists: mf_topk_deep below). */
size_t mf_topk_ws_bytes(int64_t Q, int64_t N, int d, int k);
/* Host-only geometry query: the number of catalog chunks (one workgroup column each) mf_topk would use for this shape, and
 * the rows per chunk -- a chunk is staged through one 32-bit buffer descriptor, so rows_per_chunk * d * 4 <= ~4 GiB always
 * holds.  0 = unsupported shape. */
int mf_topk_chunks(int64_t Q, int64_t N, int d, int k, int64_t* rows_per_chunk);
int mf_topk(const float* q, int64_t Q, const float* items, int64_t N, int d, int k,
            const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, void* ws,
            size_t ws_bytes, float* out_scores, int64_t* out_idx, mf_stream_t stream);

/* Merge G partial results (e.g. the all-gathered per-shard top-k of a row-sharded
 * catalog) part_*[G,Q,k] into the global top-k with the same order.  Sized for k <= 64 (k selection rounds over the
 * G * k keys of a query, which sit in 64 KiB of LDS: G * k <= 8192, MF_ENOTSUP "G * k too large" beyond); deeper lists:
 * mf_topk_merge_deep below. */
int mf_topk_merge(const float* part_scores, const int64_t* part_idx, int G, int64_t Q, int k,
                  float* out_scores, int64_t* out_idx, mf_stream_t stream);

/* Sharded retrieval in ONE exchange: mf_topk_pack turns a rank's partial result (n = Q * k scores and LOCAL rows of its
 * shard; -1 = none) into one int64 per entry -- score bits << 32 | global row (local * stride + offset, < 2^32), -1 for
 * none -- and mf_topk_merge_packed merges G such blocks [G][Q][k] (as they arrive from one all-to-all) into the global
 * top-k, exactly like mf_topk_merge on (scores, global rows). */
int mf_topk_pack(const float* scores, const int64_t* rows, int64_t n, int64_t stride, int64_t offset, int64_t* out_packed,
                 mf_stream_t stream);
int mf_topk_merge_packed(const int64_t* packed, int G, int64_t Q, int k, float* out_scores, int64_t* out_idx,
                         mf_stream_t stream);

/* The same two merges for deep lists, 1 <= k <= MF_TOPK_DEEP_MAX_K (what mf_topk_deep returns per shard).  Input contract as
 * above: [G][Q][k], GLOBAL rows < 2^32 and distinct across the lists of a query, -1 (all ones in the packed form) for none,
 * each list ordered as the searches return it (score descending, then row ascending, the none-tail last).  Results: the bits,
 * order and -inf / -1 tail of mf_topk_merge / mf_topk_merge_packed.  One 256-thread workgroup per query holds the G * k keys
 * in LDS and gives every entry its place by one binary search per other list (place in its own list + keys above it
 * elsewhere): no selection rounds, no atomics, no float arithmetic; deterministic and capturable.  A key that arrives in
 * several lists (outside the contract) counts as standing before its copies in later lists, so every column is still written
 * exactly once; lists that are not ordered give unspecified results, never an access outside the arrays.  Refused before any
 * launch, in this order: MF_EINVAL "bad argument" (a null pointer, G, Q or k <= 0); MF_ENOTSUP "k = .. outside 1..1024";
 * MF_ENOTSUP "G * k too large" above MF_TOPK_MERGE_DEEP_MAX_KEYS keys (128 KiB of LDS: 16 lists at k = 1024, 64 at
 * k = 256). */
#define MF_TOPK_MERGE_DEEP_MAX_KEYS 16384
int mf_topk_merge_deep(const float* part_scores, const int64_t* part_idx, int G, int64_t Q, int k,
                       float* out_scores, int64_t* out_idx, mf_stream_t stream);
int mf_topk_merge_packed_deep(const int64_t* packed, int G, int64_t Q, int k, float* out_scores, int64_t* out_idx,
                              mf_stream_t stream);

/* Small-batch form of mf_topk: Q <= 32 queries (the reference's search takes ONE query per call,
 * xfmr_rec/data/lightning.py:237-259; recommend, xfmr_rec/lightning.py:76-95).  A matrix-vector scan is
 * bandwidth-bound, so this path streams a BLOCKED copy of the catalog -- [block of 64 rows][16-byte chunk][row],
 * built once per index by mf_topk_blocked_build into mf_topk_blocked_bytes(N, d) bytes -- with one row per lane
 * and the canonical fmaf chain per (query, row): results are bit-identical to mf_topk's (scores, order, rows,
 * exclusion semantics, tail of -inf / -1).  Two launches, no memset, no scatter. */
size_t mf_topk_blocked_bytes(int64_t N, int d);
int mf_topk_blocked_build(const float* items, int64_t N, int d, float* out_blocked, mf_stream_t stream);
size_t mf_topk_small_ws_bytes(int64_t Q, int64_t N, int d, int k);
int mf_topk_small(const float* q, int64_t Q, const float* blocked, int64_t N, int d, int k,
                  const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, void* ws,
                  size_t ws_bytes, float* out_scores, int64_t* out_idx, mf_stream_t stream);

/* Many-query form of mf_topk (Q >= ~64, d in {64, 128, 256}): the catalog is scanned TWICE with bf16 operands
 * (v_mfma_f32_32x32x16_bf16: 16x the fp32 MFMA rate, half the bytes) -- once for per-query bounds, once for the rows
 * above them -- and only those few dozen rows per query are scored with the canonical fp32 fmaf chain.  A rigorous
 * bound on the bf16 error (csrc/mf_topk_bf3.hip) makes the candidate set a superset of the true top k, so scores,
 * order, rows, exclusion semantics and the -inf / -1 tail are IDENTICAL to mf_topk's (finite inputs).  `index`:
 * mf_topk_bf3_index_bytes(N, d) bytes filled once per catalog by mf_topk_bf3_build (bf16 rows + the largest row
 * norm); `items` are the same fp32 rows mf_topk takes.  mf_topk_bf3_plan is host-only: the geometry a search of this
 * shape runs with, out16[0..13] = NT (32-row tiles), nblk (4-tile blocks), XT (query tiles per wave), xw (query-tile sets per
 * workgroup), Qp (padded queries), gy (query workgroups), bs (the seed scan takes one block in every bs), nvb_seed, bpc_seed,
 * nwg_seed (seed scan: blocks, blocks per workgroup, workgroups), bpc, nwg (full scan), nvals (seed maxima per query),
 * windows of the exclusion-word prep; out16[14..15] = 0.  MF_EINVAL for a null out16 or a shape mf_topk_bf3_ws_bytes sizes as 0. */
size_t mf_topk_bf3_index_bytes(int64_t N, int d);
int mf_topk_bf3_build(const float* items, int64_t N, int d, void* index, size_t index_bytes, mf_stream_t stream);
size_t mf_topk_bf3_ws_bytes(int64_t Q, int64_t N, int d, int k);
int mf_topk_bf3_plan(int64_t Q, int64_t N, int d, int64_t* out16);
int mf_topk_bf3(const float* q, int64_t Q, const float* items, const void* index, int64_t N, int d, int k,
                const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, void* ws, size_t ws_bytes,
                float* out_scores, int64_t* out_idx, mf_stream_t stream);

/* Deep candidate lists: the same exact top-k for 1 <= k <= MF_TOPK_DEEP_MAX_K (the three engines above stop at 64: one
 * wavefront holds a row's result).  Scores once, then selects from the scores, in blocks of queries: the fp32 MFMA chain
 * writes a slab of 32-bit ranks [queries per block][N rounded up to 32], exclusions are stored over it, and one workgroup
 * per query finds the k-th best rank by an MSB-first radix select (integer LDS histograms), collects what ranks above it,
 * takes ties in ascending row order and sorts.  Scores, order, rows, exclusion semantics, idx_base and the -inf / -1 tail are
 * IDENTICAL to mf_topk's.  The workspace is the slab: the number of query blocks follows from its size --
 * mf_topk_deep_ws_bytes is the preferred size (one slab of at most 256 MiB), mf_topk_deep_min_ws_bytes one block of 32
 * queries; both are 0 for invalid shapes (k outside 1..1024 included).  mf_topk_deep_plan is host-only: out[0] = queries per
 * block (a multiple of 32), out[1] = blocks, out[2] = slab bytes per block for a workspace of ws_bytes.  Limits as mf_topk
 * (N < 2^31, idx_base + N <= 2^32, d in {32, 64, 128, 256}), and a 32-query slab must stay below 4 GiB (N <= ~33.5 M):
 * MF_ENOTSUP beyond, as for k outside 1..1024; MF_ENOSPC below the minimum workspace; all decided before any launch.
 * Over a row-sharded catalog the per-shard lists of this engine are joined by mf_topk_merge_deep / mf_topk_merge_packed_deep. */
#define MF_TOPK_DEEP_MAX_K 1024
size_t mf_topk_deep_ws_bytes(int64_t Q, int64_t N, int d, int k);
size_t mf_topk_deep_min_ws_bytes(int64_t Q, int64_t N, int d, int k);
int mf_topk_deep_plan(int64_t Q, int64_t N, int d, int k, size_t ws_bytes, int64_t* out);
int mf_topk_deep(const float* q, int64_t Q, const float* items, int64_t N, int d, int k,
                 const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base,
                 void* ws, size_t ws_bytes, float* out_scores, int64_t* out_idx, mf_stream_t stream);

/* Partitioned (inverted-file) retrieval: a query scans only the cells it probes -- and those exactly.  The catalog is kept a
 * second time ordered by cell, every cell padded to whole 64-row blocks: `blocked` = mf_topk_blocked_build of that padded
 * matrix (padding rows zero), cell_blk[C + 1] = the first 64-row block of every cell (cell_blk[c] == cell_blk[c + 1]: an empty
 * cell), row_of[Npad] = the catalog row at a padded position, -1 for padding, max_cell_blocks = the largest cell's blocks.
 *
 * mf_ivf_scan replaces the partition scan of the reference's `search` (xfmr_rec/data/lightning.py:250-259: LanceDB visits
 * num_probes = 8 partitions and scores their rows through a product quantiser).  probes[Q][nprobe] names the cells of every
 * query (a cell outside [0, C) contributes nothing).  Every row of a probed cell is scored with the chain of mf_topk and keyed
 * by its CATALOG row, exclusion lists as for mf_topk (GLOBAL rows, any order); one workgroup per (query, probe, slice of the
 * cell) leaves its k best as a partial list in ws: [G = nprobe * S][Q][k] packed entries as mf_topk_pack writes them (global
 * rows, -1 for none), which mf_topk_merge_packed(ws, G, Q, k, ..) turns into the result -- bit for bit mf_topk's over the
 * union of the probed cells (all cells probed: over the catalog).  S = slices per cell, 0 for the planned number.  One launch,
 * no atomics, nothing to clear, no host read: capturable.
 * Refused before any launch, in this order: MF_EINVAL "bad argument" (a null pointer, Q, N, C or max_cell_blocks <= 0, Npad
 * below N or no multiple of 64, max_cell_blocks > Npad / 64, S < 0); MF_ENOTSUP k outside 1..64; MF_ENOTSUP nprobe outside
 * 1..min(C, 64); MF_EINVAL a width outside {32, 64, 128, 256}; MF_ENOTSUP "item indices must fit 32 bits" (Npad >= 2^31,
 * idx_base < 0 or idx_base + N > 2^32); MF_ENOTSUP "nprobe * S * k too large" (above the 8192 keys of mf_topk_merge, or
 * S > max_cell_blocks); MF_ENOSPC "workspace too small" (below G * Q * k * 8 bytes); MF_EINVAL an exclusion pair of which one
 * is null.
 * mf_ivf_plan is host-only: out[0] = S for this shape -- enough workgroups for a single query, at most max_cell_blocks, and
 * nprobe * S * k <= 8192 (the rule itself: mf_cells_slices of csrc/mf_cells.h, which mf_pq_plan follows too) --, out[1] = G,
 * out[2] = workgroups, out[3] = bytes of the partial lists.  mf_ivf_ws_bytes: those bytes rounded up to 256, 0 for a shape
 * mf_ivf_plan refuses (MF_EINVAL).
 * mf_ivf_cell_mean replaces the centroid update of the k-means behind the reference's `create_index` (:222-229;
 * LanceDB trains its partitions internally): out[c] = the mean of rows items[order[cell_off[c] .. cell_off[c + 1])], added in
 * that order by one thread per dimension (no float atomics: the same bits every run), scaled to unit L2 length when
 * `normalize` (a mean of norm zero stays as it is); an empty cell leaves out[c] untouched. */
size_t mf_ivf_ws_bytes(int64_t Q, int nprobe, int k, int64_t max_cell_blocks);
int mf_ivf_plan(int64_t Q, int nprobe, int k, int64_t max_cell_blocks, int64_t* out4);
int mf_ivf_scan(const float* q, int64_t Q, const float* blocked, const int64_t* cell_blk, const int64_t* row_of, int64_t Npad,
                int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes, int nprobe, int k, int S,
                const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, void* ws, size_t ws_bytes,
                mf_stream_t stream);
int mf_ivf_cell_mean(const float* items, int64_t N, int d, const int64_t* order, const int64_t* cell_off, int64_t C,
                     int normalize, float* out, mf_stream_t stream);
/* mf_ivf_scan_allow: mf_ivf_scan filtered in place -- the reference's `.where(filter, prefilter=True)` (:250-259) without a
 * second copy of the admissible rows.  Every argument of mf_ivf_scan in its order, and before ws the allow bitmap: allow
 * [n_masks][Npad / 64] 64-bit words as mf_filter_cell_bits writes them (bit `lane` of word `blk`: the row at cell-ordered
 * position blk * 64 + lane may enter a list); query q reads mask allow_of[q] (allow_of null: mask 0, which needs n_masks == 1);
 * an allow_of[q] outside [0, n_masks) admits nothing -- that query's lists are all -1.  A row whose bit is clear has key 0
 * before it can compete, as an excluded row's key never enters: the lists -- and after mf_topk_merge_packed the result -- are bit
 * for bit mf_ivf_scan's with every such row on the query's exclusion list.  A wave loads its block's word once (a scalar load)
 * and skips a block whose word is 0: no row, no row_of load.  One launch, no atomics, no host read: capturable.  Refusals:
 * mf_ivf_scan's in its order, then MF_EINVAL "bad allow argument" (allow null, n_masks <= 0, or allow_of null with n_masks
 * != 1); MF_ENOTSUP n_masks * (Npad / 64) >= 2^31. */
int mf_ivf_scan_allow(const float* q, int64_t Q, const float* blocked, const int64_t* cell_blk, const int64_t* row_of, int64_t Npad,
                      int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes, int nprobe, int k, int S,
                      const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, const uint64_t* allow, int64_t n_masks,
                      const int64_t* allow_of, void* ws, size_t ws_bytes, mf_stream_t stream);
/* Deep lists from the cells: mf_ivf_scan and mf_ivf_scan_allow for 1 <= k <= MF_TOPK_DEEP_MAX_K (the reference's
 * `.limit(top_k)` has no cap; the two scans above stop at 64, a list per wavefront).  The argument lists are exactly theirs,
 * the geometry, the chain, the keys by CATALOG row, the exclusion lists, the allow bitmap and the packed lists [G = nprobe * S]
 * [Q][k] too; the workgroup keeps its best keys in one LDS buffer (csrc/mf_ivf_deep.hip) instead of a list per wave.  The lists
 * go to mf_topk_merge_packed_deep(ws, G, Q, k, ..) -- so nprobe * S * k <= MF_TOPK_MERGE_DEEP_MAX_KEYS = 16,384 -- and the
 * result is bit for bit mf_topk_deep's over the union of the probed cells (rows the mask admits).  One launch, no atomics,
 * nothing to clear, no host read: capturable.  Refusals: those of mf_ivf_scan / mf_ivf_scan_allow in their order and words,
 * with "k = .. outside 1..1024" and the 16,384 keys of the deep merge behind "nprobe * S * k too large".
 * mf_ivf_deep_plan / mf_ivf_deep_ws_bytes: the rule of mf_ivf_plan / mf_ivf_ws_bytes with k <= 1024 and nprobe * S * k <=
 * 16,384 (S never below 1: a shape with nprobe * k above 16,384 is planned with S = 1 and refused by the scan). */
size_t mf_ivf_deep_ws_bytes(int64_t Q, int nprobe, int k, int64_t max_cell_blocks);
int mf_ivf_deep_plan(int64_t Q, int nprobe, int k, int64_t max_cell_blocks, int64_t* out4);
int mf_ivf_scan_deep(const float* q, int64_t Q, const float* blocked, const int64_t* cell_blk, const int64_t* row_of, int64_t Npad,
                     int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes, int nprobe, int k, int S,
                     const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, void* ws, size_t ws_bytes,
                     mf_stream_t stream);
int mf_ivf_scan_deep_allow(const float* q, int64_t Q, const float* blocked, const int64_t* cell_blk, const int64_t* row_of, int64_t Npad,
                           int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes, int nprobe, int k, int S,
                           const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base, const uint64_t* allow, int64_t n_masks,
                           const int64_t* allow_of, void* ws, size_t ws_bytes, mf_stream_t stream);

/* Product-quantised cells with an exact refine: the rest of the reference's IVF_PQ index (xfmr_rec/data/lightning.py:162-165,
 * 203-204: num_sub_vectors = embedding_dim // 8, refine_factor = 4; :222-229 create_index; :250-259
 * search(..).nprobes(..).refine_factor(..)).  The cells, cell_blk, row_of, Npad and max_cell_blocks are those of mf_ivf_scan;
 * the cell-ordered fp32 copy is replaced by one byte per dsub channels.  With D = M * dsub (dsub in {4, 8, 16}, M <= 64),
 * codebooks B[M][256][dsub] fp32 and chain = the mf_dot_chain of mf_numerics.h over a sub-vector -- at dsub = 4 its four products
 * in ascending channel order, the chain of the sub-vector zero-padded to 8 --:
 *   residual  r = x - centroids[assign[row]]                               (one fp32 subtraction per channel)
 *   code[m]   = argmax_j (chain(r[m], B[m][j]) - 0.5f * chain(B[m][j], B[m][j])), the lowest j on ties
 *   lut[m][j] = chain(q[m], B[m][j])
 *   approx    = ((base + lut[0][code[0]]) + lut[1][code[1]]) + ..,  base = chain(q, centroid of the cell): plain fp32 adds
 * Code layout (cell-ordered): U = min(M, 4) code bytes make a unit, a row has M / U units, and
 *   byte ((blk * (M / U) + u) * 64 + lane) * U + b  is code u * U + b of padded position blk * 64 + lane,
 * i.e. [64-row block][M / 4][64] 32-bit words with lane = row: a wave loads a unit of a block as one coalesced 256 B; Npad * M
 * bytes in all; padding positions hold code 0 (the scan masks them by row_of < 0).
 *
 * mf_pq_encode replaces the encoding step of LanceDB's create_index.  rows[N][d]; with centroids[C][d] and assign[N] the
 * residuals are formed in the kernel, with both null `rows` are residuals already.  With row_of[Npad] the codes leave in the
 * layout above; with row_of null (then Npad must equal N) as plain bytes [N][M] -- the assignment step of the codebook
 * training.  Refused before any launch, in this order: MF_EINVAL "bad argument" (a null rows / codebooks / codes, N <= 0,
 * Npad below N or no multiple of 64, or Npad != N without row_of); MF_EINVAL "centroids/assign mismatch"; MF_EINVAL a width
 * outside {32, 64, 128, 256}; MF_ENOTSUP a sub-vector length outside {4, 8, 16} or more than 64 sub-vectors; MF_ENOTSUP
 * "too many rows".  The codeword update of the training needs no export of its own: mf_ivf_cell_mean(residuals, T, d, order,
 * cell_off, 256, 0, out[256][d]) with the training rows listed by code of sub-space m gives the means of all channels, of
 * which channels m * dsub .. are the new codewords -- added in list order, divided by (float)count, an empty codeword's row
 * left as it was.
 * mf_pq_scan replaces the quantised partition scan of the reference's search.  probes / probe_scores [Q][nprobe]: the cells of
 * every query and chain(q, their centroid) -- what the exact engines return on the centroid matrix.  One workgroup per (query,
 * probe, slice of the cell) builds the query's M x 256 table in LDS, forms approx for every row of its slice and keeps the R
 * best keys -- mf_key_retrieval of approx and the GLOBAL row --; only a key that beats the current R-th (nothing to beat until a first sort
 * has left R keys: more than 512 keys waiting, or the end of the slice) is looked up in the exclusion list
 * (GLOBAL rows, any order), so an excluded row never takes a place.  It writes an ordered list of R packed entries (approx
 * bits << 32 | global row, -1 for none): ws = [G = nprobe * S][Q][R], which mf_topk_merge_packed_deep(ws, G, Q, R, ..) joins
 * into the R candidates of every query.  S = slices per cell, 0 for the planned number.  One launch, no atomics, nothing to
 * clear, no host read: capturable.  Refused before any launch, in this order: MF_EINVAL "bad argument" (a null pointer, Q, N, C
 * or max_cell_blocks <= 0, Npad below N or no multiple of 64, max_cell_blocks > Npad / 64, S < 0); MF_ENOTSUP R outside
 * 1..256; MF_ENOTSUP nprobe outside 1..min(C, 64); MF_EINVAL a width outside {32, 64, 128, 256}; MF_ENOTSUP a sub-vector length
 * outside {4, 8, 16} or more than 64 sub-vectors; MF_ENOTSUP "item indices must fit 32 bits" (Npad >= 2^31, idx_base < 0 or
 * idx_base + N > 2^32); MF_ENOTSUP "nprobe * S * R too large" (above the MF_TOPK_MERGE_DEEP_MAX_KEYS = 16,384 keys of the
 * merge, S > max_cell_blocks, or 2^31 workgroups and more: Q * nprobe * S >= 2^31); MF_ENOSPC "workspace too small" (below G * Q * R * 8 bytes); MF_EINVAL an exclusion pair of
 * which one is null.
 * mf_pq_plan is host-only and follows the rule of mf_ivf_plan with R in the place of k and that key budget: out[0] = S,
 * out[1] = G, out[2] = workgroups, out[3] = bytes of the partial lists; MF_EINVAL for a null out, Q or max_cell_blocks <= 0, R
 * outside 1..256 or nprobe outside 1..64.  mf_pq_ws_bytes: those bytes rounded up to 256, 0 for a shape mf_pq_plan refuses.
 * mf_pq_refine replaces refine_factor's rescoring: cand[Q][R] GLOBAL rows (-1, or a row outside [idx_base, idx_base + N): no
 * candidate) are scored with the chain of mf_topk on items[N][d] -- the original matrix --, keyed by mf_key_retrieval of
 * that score and the global row, and the k best leave as mf_topk writes them (scores, int64 global rows, the -inf / -1 tail).  One workgroup per
 * query.  Refused before any launch, in this order: MF_EINVAL "bad argument"; MF_ENOTSUP k outside 1..64; MF_ENOTSUP R outside
 * k..256; MF_EINVAL a width outside {32, 64, 128, 256}; MF_ENOTSUP "item indices must fit 32 bits". */
int mf_pq_encode(const float* rows, int64_t N, int d, const float* centroids, const int64_t* assign, const float* codebooks,
                 int dsub, const int64_t* row_of, int64_t Npad, void* codes, mf_stream_t stream);
size_t mf_pq_ws_bytes(int64_t Q, int nprobe, int R, int64_t max_cell_blocks);
int mf_pq_plan(int64_t Q, int nprobe, int R, int64_t max_cell_blocks, int64_t* out4);
int mf_pq_scan(const float* q, int64_t Q, const void* codes, const float* codebooks, int dsub, const int64_t* cell_blk,
               const int64_t* row_of, int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes,
               const float* probe_scores, int nprobe, int R, int S, const int64_t* excl_off, const int64_t* excl_idx,
               int64_t idx_base, void* ws, size_t ws_bytes, mf_stream_t stream);
int mf_pq_refine(const float* q, int64_t Q, const float* items, int64_t N, int d, const int64_t* cand, int R, int k,
                 int64_t idx_base, float* out_scores, int64_t* out_idx, mf_stream_t stream);
/* mf_pq_scan_allow: mf_pq_scan filtered in place -- what the reference's IVF_PQ search runs with `.where(filter,
 * prefilter=True)`.  Every argument of mf_pq_scan in its order, and before ws the allow bitmap of mf_ivf_scan_allow (allow
 * [n_masks][Npad / 64], n_masks, allow_of [Q] nullable; an allow_of[q] outside [0, n_masks) admits nothing).  A row whose bit
 * is clear has key 0 before it meets the bound, so the kept keys, the bound and the lists of approximate scores are bit for
 * bit mf_pq_scan's with every such row on the query's exclusion list -- the argument does not ask whether the scores are exact.
 * A wave takes the words of 64 blocks by one vector load (lane = block) and reads each pass's word out of that strip; a wave whose
 * word is 0 loads neither codes nor row_of and still takes every barrier of the pass.  mf_pq_refine needs no mask:
 * it only sees candidates the scan admitted.  Refusals: mf_pq_scan's in its order, then MF_EINVAL "bad allow argument" (allow
 * null, n_masks <= 0, or allow_of null with n_masks != 1); MF_ENOTSUP n_masks * (Npad / 64) >= 2^31. */
int mf_pq_scan_allow(const float* q, int64_t Q, const void* codes, const float* codebooks, int dsub, const int64_t* cell_blk,
                     const int64_t* row_of, int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes,
                     const float* probe_scores, int nprobe, int R, int S, const int64_t* excl_off, const int64_t* excl_idx,
                     int64_t idx_base, const uint64_t* allow, int64_t n_masks, const int64_t* allow_of, void* ws, size_t ws_bytes,
                     mf_stream_t stream);
/* Deep lists from the quantised cells: the same search where R = refine_factor * k exceeds 256 or k exceeds 64 -- the
 * reference's `.refine_factor(4).limit(top_k)` has no cap.  mf_pq_scan_deep / mf_pq_scan_deep_allow take every argument of
 * mf_pq_scan / mf_pq_scan_allow in its order and score to the bit as they do (tables, plain fp32 adds, the key by the global
 * row); the workgroup keeps its best keys as mf_ivf_scan_deep does -- one LDS buffer of 4,096 keys, the kept part in classes
 * 128 / 256 / 512 / 1024, a bitonic settle -- and every workgroup writes all R entries of its list, "none" where it has fewer:
 * [G = nprobe * S][Q][R] packed, what mf_topk_merge_packed_deep takes.  1 <= R <= 1024 and nprobe * S * R <= 16,384.  Static
 * LDS M KiB + 32 KiB + 16 B (M = d / dsub sub-vectors: 34 KiB at M = 2, 96 KiB at M = 64).  One launch each, no atomics,
 * nothing to clear, no host read, capturable.  Refused before any launch: mf_pq_scan's refusals (then mf_pq_scan_allow's) in
 * their order and words, with "R = .. outside 1..1024" in the place of the 256 limit and the 16,384 keys of the deep merge
 * behind "nprobe * S * R too large".
 * mf_pq_deep_plan / mf_pq_deep_ws_bytes: the rule of mf_pq_plan / mf_pq_ws_bytes with R <= 1024.
 * mf_pq_refine_deep: mf_pq_refine for 1 <= k <= 1024 and k <= R <= 1024, the same arguments and arithmetic: one 256-thread
 * workgroup per query, a thread scores up to four candidates, the keys are sorted in 8 KiB of LDS and the k best leave with
 * the -inf / -1 tail.  The candidates of a query are distinct rows (the merge's output; -1 and rows outside [idx_base,
 * idx_base + N) are no candidates).  Refused before any launch, in this order: MF_EINVAL "bad argument"; MF_ENOTSUP k outside
 * 1..1024; MF_ENOTSUP R outside k..1024; MF_EINVAL a width outside {32, 64, 128, 256}; MF_ENOTSUP "item indices must fit 32
 * bits". */
size_t mf_pq_deep_ws_bytes(int64_t Q, int nprobe, int R, int64_t max_cell_blocks);
int mf_pq_deep_plan(int64_t Q, int nprobe, int R, int64_t max_cell_blocks, int64_t* out4);
int mf_pq_scan_deep(const float* q, int64_t Q, const void* codes, const float* codebooks, int dsub, const int64_t* cell_blk,
                    const int64_t* row_of, int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks, const int64_t* probes,
                    const float* probe_scores, int nprobe, int R, int S, const int64_t* excl_off, const int64_t* excl_idx,
                    int64_t idx_base, void* ws, size_t ws_bytes, mf_stream_t stream);
int mf_pq_scan_deep_allow(const float* q, int64_t Q, const void* codes, const float* codebooks, int dsub, const int64_t* cell_blk,
                          const int64_t* row_of, int64_t Npad, int64_t N, int64_t C, int d, int64_t max_cell_blocks,
                          const int64_t* probes, const float* probe_scores, int nprobe, int R, int S, const int64_t* excl_off,
                          const int64_t* excl_idx, int64_t idx_base, const uint64_t* allow, int64_t n_masks, const int64_t* allow_of,
                          void* ws, size_t ws_bytes, mf_stream_t stream);
int mf_pq_refine_deep(const float* q, int64_t Q, const float* items, int64_t N, int d, const int64_t* cand, int R, int k,
                      int64_t idx_base, float* out_scores, int64_t* out_idx, mf_stream_t stream);

/* Retrieval metrics @k on device, straight from the top-k output.  Replaces the
 * per-example torchmetrics updates of `update_metrics` / `get_metrics` (xfmr_rec/lightning.py:149-187,
 * :289-306: RetrievalNormalizedDCG / Recall / Precision / MAP / HitRate / MRR, top_k = 20).
 * topk_idx[Q,k]: retrieved item ids, best first (-1 = none); the targets of query q are
 * tgt_idx / tgt_rel[tgt_off[q] .. tgt_off[q+1]) (item id, rating); an unretrieved target ranks below
 * every retrieved item (the reference gives it -U(0,1): the same whenever retrieved scores are
 * positive).  out[q][6] = {ndcg, recall, precision, map, hit_rate, mrr} of query q with torchmetrics'
 * definitions: linear gain / log2 discount, binary relevance = rating > 0 for the other five,
 * precision divided by k, a query without positive target scores 0 everywhere.  k <= 1024 (k <= 64: one rank per lane;
 * beyond, lane t walks ranks t, t + 64, ...); MF_ENOTSUP above. */
int mf_retrieval_metrics(const int64_t* topk_idx, int64_t Q, int k, const int64_t* tgt_off,
                         const int64_t* tgt_idx, const float* tgt_rel, float* out, mf_stream_t stream);

/* Positions instead of lists: the exact place of GIVEN rows (a query's targets, CSR tgt_off[Q+1] / tgt_idx[n_targets], global
 * rows) in the query's order of all admissible rows -- the order the searches above select from: key(y) = the
 * retrieval key of mf_numerics.h for (chain score, y), row y admissible iff 0 <= y < N and y + idx_base is not on the query's exclusion list.
 * out_ncand[r] = admissible rows of query r.  For entry e of query r with y = tgt_idx[e] - idx_base: admissible ->
 * out_pos[e] = number of admissible rows with a larger key (0 = best), out_score[e] = its chain score; otherwise -1 / -inf.
 * So 0 <= out_pos[e] < k <= 1024 means mf_topk_deep returns that row at column out_pos[e] with the same score bits, and
 * out_pos[e] >= k that it does not.  Duplicate entries get the same answer, an empty list writes nothing; n_targets (the length
 * of tgt_idx and of both outputs) is only checked, n_targets == 0 still writes out_ncand.  Runs mf_topk_deep's slab stage per
 * block of queries, then one workgroup per query counts over its slab row (lists of any length, 1024 entries per sweep of the
 * row).  Workspace = the slab, sized like mf_topk_deep's: _ws_bytes the preferred size, _min_ws_bytes one block of 32 queries, 0
 * for invalid shapes.  No host read, no allocation, no float atomics; capturable.  MF_EINVAL: a null pointer (the exclusion pair
 * may be null together), Q <= 0, N <= 0, n_targets < 0, a width outside {32, 64, 128, 256}; MF_ENOTSUP: N >= 2^31,
 * idx_base + N > 2^32, a 32-query slab of 4 GiB or more; MF_ENOSPC: a workspace below the minimum; all before any launch. */
size_t mf_target_positions_ws_bytes(int64_t Q, int64_t N, int d);
size_t mf_target_positions_min_ws_bytes(int64_t Q, int64_t N, int d);
int mf_target_positions(const float* q, int64_t Q, const float* items, int64_t N, int d,
                        const int64_t* tgt_off, const int64_t* tgt_idx, int64_t n_targets,
                        const int64_t* excl_off, const int64_t* excl_idx, int64_t idx_base,
                        void* ws, size_t ws_bytes, int64_t* out_pos, float* out_score, int64_t* out_ncand, mf_stream_t stream);

/* Positions over a ROW-SHARDED catalog: every shard holds N rows, local row l = global row g(l) = l * stride + offset
 * (round-robin: stride = shards, offset = shard; contiguous blocks: stride = 1, offset = first row), and the global order is
 * mf_target_positions' on the whole catalog: order word (mf_orderable of the chain score) descending, then global row ascending.
 * Two calls per shard, one exchange between them, one after:
 *
 * mf_target_words: out_word[e] (int64, a value in [0, 2^32)) = the order word of entry e's row against its query when this
 *   shard holds the row -- tgt_idx[e] - offset >= 0, divisible by stride, quotient < N; the bits the slab of the searches
 *   holds -- and 0 otherwise.  Exclusion lists play no part.  The caller takes the MAXIMUM over the shards: at most one holds a row.
 *   One launch, no workspace.
 * mf_key_positions: tgt_word = those maxima.  With L = clamp(ceil((tgt_idx[e] - offset) / stride), 0, N), out_above[e] = this
 *   shard's admissible rows l with word_l > tgt_word[e], or word_l == tgt_word[e] and l < L (g(l) grows with l, so that is
 *   "global row below the target's"); -1 when tgt_word[e] == 0 (no shard holds the row) or when this shard holds it and it is
 *   excluded.  out_score[e] = the score whose order word tgt_word[e] is (mf_unorderable of mf_numerics.h), -inf beside -1.  out_ncand[r] = this shard's admissible rows.
 *   excl_off / excl_local: per-query lists of LOCAL rows (entries outside [0, N) are ignored; both may be null).
 * The caller combines: position = sum of out_above over the shards, or -1 / -inf if any shard wrote -1; ncand = sum of
 * out_ncand.  That equals mf_target_positions on the unsharded catalog: integers equal, scores bit for bit.  mf_key_positions
 * runs mf_target_positions' stages on its workspace sizes (the _ws_bytes pair below returns the same numbers) with the same
 * counting code; no host read, no allocation, integer atomics only, capturable.  Refusals, all before any launch: MF_EINVAL a
 * null pointer (the exclusion pair may be null together), Q <= 0, N <= 0, n_targets < 0, stride < 1, offset < 0, a width outside
 * {32, 64, 128, 256}; MF_ENOTSUP N >= 2^31, (mf_target_words) Q >= 2^31, (mf_key_positions) a 32-query slab of 4 GiB or more; MF_ENOSPC a workspace below
 * the minimum -- in mf_target_positions' order. */
int mf_target_words(const float* q, int64_t Q, const float* items, int64_t N, int d,
                    const int64_t* tgt_off, const int64_t* tgt_idx, int64_t n_targets, int64_t stride, int64_t offset,
                    int64_t* out_word, mf_stream_t stream);
size_t mf_key_positions_ws_bytes(int64_t Q, int64_t N, int d);
size_t mf_key_positions_min_ws_bytes(int64_t Q, int64_t N, int d);
int mf_key_positions(const float* q, int64_t Q, const float* items, int64_t N, int d,
                     const int64_t* tgt_off, const int64_t* tgt_idx, const int64_t* tgt_word, int64_t n_targets,
                     int64_t stride, int64_t offset, const int64_t* excl_off, const int64_t* excl_local,
                     void* ws, size_t ws_bytes, int64_t* out_above, float* out_score, int64_t* out_ncand, mf_stream_t stream);

/* Retrieval metrics from positions (mf_target_positions): pos / tgt_rel[tgt_off[q] .. tgt_off[q+1]), ncand[Q]; ks = nk cut-offs
 * in HOST memory (1 <= nk <= 8, each >= 1, no upper limit: a k above N is legal).  out[q][6 nk + 3]: for every k the six values
 * of mf_retrieval_metrics in its order and with its conventions, "retrieved at column t" read as "position t < k" (a target at
 * -1 is never retrieved but counts among the relevant targets and in IDCG); then, over the relevant targets with a position
 * (rating > 0, pos >= 0), MRR = 1 / (smallest position + 1), MeanPosition, and AUC = mean of 1 - (pos - a) / max(ncand -
 * n, 1) with a = such targets of the query placed above this one and n = their number -- the share of other admissible
 * rows placed above a relevant one; 0 without such a target.  Differs from mf_retrieval_metrics in one case: fewer than k
 * admissible rows AND a target that is not admissible, which that kernel places below the short list and this one never
 * places.  MF_EINVAL: a null pointer, Q <= 0, a k < 1; MF_ENOTSUP: nk outside 1..8. */
int mf_position_metrics(const int64_t* pos, const int64_t* tgt_off, const float* tgt_rel, const int64_t* ncand, int64_t Q,
                        const int32_t* ks, int nk, float* out, mf_stream_t stream);

/* Filtered search over item tags: `lance_table.search(embedding).where(exclude_filter, prefilter=True)` (xfmr_rec/data/lightning.py:
 * 247-259) for predicates beyond `movie_id NOT IN (...)` -- rows that fail the predicate are never candidates.  tags [N]: one
 * int64 per row, 64 boolean attributes; a filter is three 64-bit masks, and row r with tag word t is admissible iff
 *   (t & all_of) == all_of  &&  (any_of == 0 || (t & any_of) != 0)  &&  (t & none_of) == 0.
 * The view of a filter: its admissible rows in ascending row order, gathered (mf_gather_rows, a bit copy) into a dense sub-catalog
 * that the engines above search as they are; the calls below build the view's two index vectors and carry lists into it and
 * results out of it.  Ascending compaction keeps "score descending, row ascending", and copied rows give the same chain scores: a
 * search of the view equals, bit for bit, the search of the catalog with every inadmissible row on every query's exclusion list.
 *
 * mf_filter_rows: out_rows[0 .. M) = the admissible LOCAL rows, ascending (entries from M on are not written); out_rank[r] = row
 *   r's slot in out_rows or -1, every r < N written (8-byte aligned); out_count[0] = M, on the device.  Two launches: flags by
 *   ballot with a count per 2048 rows, then every workgroup takes its base from those counts and a block scan gives each kept row
 *   its slot.  No atomics: a pure function of the inputs.
 * mf_filter_remap: out[e] = out_rank[ids[e] - idx_base] when that row lies in [0, N), else -1 -- target lists: an inadmissible
 *   target stays in place and reads "not in the catalog".  In place (out == ids) is allowed.
 * mf_filter_lists: an exclusion CSR (off [Q + 1], ids [n_entries], GLOBAL rows) mapped into the view: per query the entries whose
 *   row the view holds, in their order (sorted lists stay sorted), as slots; the others are dropped.  out_off [Q + 1] is rebuilt on
 *   the device -- a count per query, a scan over the queries, the write --, out_ids has room for n_entries.  One workgroup per
 *   query, 1024 entries in flight.  Offsets are clamped to [0, n_entries]; n_entries == 0 still writes out_off.
 * mf_filter_unmap: out[e] = idx[e] < 0 ? -1 : idx_base + rows[idx[e]] (rows [M] = out_rows; an idx[e] >= M reads -1) -- result
 *   rows.  In place is allowed.
 * No allocation, no synchronisation, no host read; capturable.  Refusals, all before any launch: MF_EINVAL a null pointer (rows
 * may be null when M == 0), a negative count, N <= 0 (mf_filter_rows: N < 0); MF_ENOTSUP N (or M, or Q) >= 2^31; MF_ENOSPC a
 * short workspace.  A zero count (N, n, Q) is MF_OK with nothing launched.  The _ws_bytes queries return 0 for a size outside
 * [1, 2^31). */
size_t mf_filter_ws_bytes(int64_t N);
int mf_filter_rows(const int64_t* tags, int64_t N, uint64_t any_of, uint64_t all_of, uint64_t none_of, void* ws, size_t ws_bytes,
                   int64_t* out_rows, int32_t* out_rank, int64_t* out_count, mf_stream_t stream);
int mf_filter_remap(const int64_t* ids, int64_t n, int64_t idx_base, const int32_t* rank, int64_t N, int64_t* out,
                    mf_stream_t stream);
size_t mf_filter_lists_ws_bytes(int64_t Q);
int mf_filter_lists(const int64_t* off, const int64_t* ids, int64_t n_entries, int64_t Q, int64_t idx_base, const int32_t* rank,
                    int64_t N, void* ws, size_t ws_bytes, int64_t* out_off, int64_t* out_ids, mf_stream_t stream);
int mf_filter_unmap(const int64_t* idx, int64_t n, const int64_t* rows, int64_t M, int64_t idx_base, int64_t* out,
                    mf_stream_t stream);
/* mf_filter_cell_bits: the same predicate as a bitmap over a cell-ordered catalog (row_of [Npad], Npad a multiple of 64: the
 * layout of mf_ivf_scan), for the scans that filter in place: bit `lane` of out_words[blk] is set iff r = row_of[blk * 64 + lane]
 * >= 0 and tags[r] is admissible -- Npad / 8 bytes per filter where a view copies its rows; padding positions are never set.
 * One launch, a wave per block, the word is the wave's ballot; no atomics, no workspace, no host read, every word written: a
 * pure function of the inputs, capturable.  Refusals before any launch, in this order: MF_EINVAL a null pointer, N <= 0, Npad
 * < N or no multiple of 64; MF_ENOTSUP Npad >= 2^31. */
int mf_filter_cell_bits(const int64_t* tags, int64_t N, uint64_t any_of, uint64_t all_of, uint64_t none_of, const int64_t* row_of,
                        int64_t Npad, uint64_t* out_words, mf_stream_t stream);

/* ------------------------------------------------------------ streaming logQ ---
 * The table the logQ correction reads, estimated from the batches themselves (Yi et al. 2019, Algorithms 2 and 3; our
 * spec, DESIGN.md 4 "Streaming logQ", restated in numpy as tests/_logq_spec.py).  State per bucket h: last_seen[h] (the step of
 * its last sighting, 0 = never) and gap[h] (moving average of the steps between sightings, 0 = never).  One update at
 * step t (>= 1, strictly increasing from call to call) touches every DISTINCT bucket of ids[n] once:
 *     old = last_seen[h];  g = (float)(t - old)                    (int -> fp32, round to nearest even)
 *     gap[h] = old == 0 ? g : fl(fl((1 - alpha) gap[h]) + fl(alpha g))          (1 - alpha computed once in fp32)
 *     last_seen[h] = t
 * and logq(id) = -logf(D), the log of the estimated per-step inclusion rate 1 / D.
 *   direct (num_hashes = 0): arrays [n_buckets], bucket = id, D = gap[id]; ids outside [0, n_buckets) are ignored, read 0.
 *   hashed (num_hashes = 1..4): arrays [num_hashes][n_buckets], bucket j = mf_numerics.h's mf_hash_bucket of (id, j, seed,
 *     n_buckets), D = the largest of the id's gaps; ids sharing a bucket are one sighting; negative ids are ignored.
 *   An id with a bucket never seen (gap == 0) reads 0.0: no estimate, no correction.
 * A second update with the same t changes nothing.  The step is t, or -- t_dev non-null -- *t_dev read on the device (t
 * is then ignored; the caller advances the counter, the kernels never write it; a value outside 1 .. 2^31 - 1 updates
 * nothing): a captured call advances on replay.  logq_table (direct mode, [n_buckets], nullable) receives -logf(gap) of
 * every updated bucket; out_logq (nullable, [n]) the read-out of ids after the update, by a second launch.
 * mf_logq_lookup is that read-out alone.  No allocation, no host read, no synchronisation, integer atomics only;
 * capturable.  Refusals, all before any launch: MF_EINVAL a null last_seen / gap / ids (ids may be null when n == 0) /
 * out_logq of the lookup, n < 0, n_buckets < 1, num_hashes outside 0..4, alpha outside (0, 1], t < 1 without t_dev, a
 * logq_table with num_hashes > 0; MF_ENOTSUP t >= 2^31, n_buckets >= 2^31, n >= 2^39.  n == 0: MF_OK, nothing launched.
 * mf_logq_set_peel: how many of a wave's most repeated buckets are reduced to one lane before the atomic (0..8, default
 * 4; speed only, tools/logq_probe.py). */
int mf_logq_update(int32_t* last_seen, float* gap, int64_t n_buckets, int num_hashes, uint64_t seed, const int64_t* ids,
                   int64_t n, int64_t t, const int64_t* t_dev, float alpha, float* logq_table, float* out_logq,
                   mf_stream_t stream);
int mf_logq_lookup(const float* gap, int64_t n_buckets, int num_hashes, uint64_t seed, const int64_t* ids, int64_t n,
                   float* out_logq, mf_stream_t stream);
void mf_logq_set_peel(int rounds);

/* The batch producer on the device (replaces the host datapipe of
 * xfmr_rec/data/lightning.py:311-363 + data/load.py:38-141 for id-only towers).  The interaction list
 * pair_*[n_pairs] and the users' positive lists (CSR pos_off[num_users + 1], pos_items) stay in HBM;
 * examples start .. start + B - 1 of the reshuffled-every-epoch stream are written as one batch:
 * out_user[B], out_item[2 B] (the pairs' items, then B uniform negatives in 1 .. num_items - 1),
 * out_target[B], out_pos[B, P] (the user's positives, truncated to P, 0-padded on the right).
 * Counter-based: a batch depends on (seed, start) only (mf_data.hip; spec oracle/data.py). */
int mf_sample_batch(const int64_t* pair_user, const int64_t* pair_item, const float* pair_target, int64_t n_pairs,
                    const int64_t* pos_off, const int64_t* pos_items, int64_t num_items, uint64_t seed,
                    int64_t start, int64_t B, int P, int64_t* out_user, int64_t* out_item, float* out_target,
                    int64_t* out_pos, mf_stream_t stream);

/* ----------------------------------------------------------- sharded path ---
 * The reference has no collective; these serve the row-sharded design of distributed.py.
 * mf_init_rows fills a shard on its own device: local row l = global row row_start + l * row_stride of a
 * virtual [rows, d] table of std-scaled normal variates that are a pure function of (seed, global row,
 * column) -- no host copy of the whole table, values independent of the number of ranks.
 * mf_comm_*: RCCL (opened lazily) called on the CALLER'S stream: an exchange is a node between two kernels,
 * not a cross-stream join.  Bootstrap: rank 0 gets 128 bytes from mf_comm_unique_id, every rank receives
 * them by any side channel and calls mf_comm_create (a collective).  mf_comm_all_to_all_rows is a direct
 * all-to-all of row blocks (grouped send / recv: point-to-point xGMI links, no ring) with the per-peer row
 * counts on the host; mf_comm_all_gather the fixed-size gather of the retrieval queries. */
int mf_init_rows(float* table, int64_t n_local, int d, int64_t row_start, int64_t row_stride, uint64_t seed,
                 float std, mf_stream_t stream);
int mf_comm_unique_id(void* out128);
int mf_comm_create(int world, int rank, const void* id128, void** out_comm);
int mf_comm_destroy(void* comm);
int mf_comm_world(void* comm);
/* where the RCCL entry points came from: "shared: ..." (the librccl torch had already mapped: RTLD_NOLOAD),
 * "own: dlopen" (a process without one), "not loaded" */
const char* mf_comm_source(void);
int mf_comm_all_to_all_rows(void* comm, const void* send, const int64_t* send_rows_host, void* recv,
                            const int64_t* recv_rows_host, int64_t row_bytes, mf_stream_t stream);
int mf_comm_all_gather(void* comm, const void* send, void* recv, int64_t bytes, mf_stream_t stream);

/* ------------------------------------------------------------ history-pooled user tower ---
 * The id-only counterpart of PoolingTransformer.forward (xfmr_rec/models.py:81-84, pooling_mode "mean" / "max",
 * models.py:24, then Normalize, models.py:59) over the item rows of a user's history (prepare.py:285-299).  User b's list
 * is items[start[b], end[b]) (clamped to [0, n_items)); ids outside [1, n_rows) are padding; max_history > 0 keeps the last
 * max_history valid entries.  r_e = norm_item ? W[id] / max(|W[id]|, 1e-12) : W[id]; p_b = mean_e r_e (mode 0) or the
 * channel-wise max (mode 1: ties go to the first entry); u_b = norm_user ? p_b / max(|p_b|, 1e-12) : p_b; an empty list
 * gives u_b = 0.  n_entries >= sum_b (end[b] - start[b]) sizes the workspace (mf_pool_ws_bytes).  Outputs: out_u [B, d],
 * out_inv [B] (1 / max(|p_b|, 1e-12), or 1), out_count [B] (valid entries), out_lo [B] (first position pooled), out_off [B + 1]
 * (exclusive prefix of end - lo: the entry numbering of the backward), out_arg [B, d] (mode 1: the winning entry's offset
 * from out_lo, -1 for an empty list).  Deterministic: fixed chunking and combination order, no atomics.  MF_ENOTSUP above
 * 2^20 table rows. */
size_t mf_pool_ws_bytes(int64_t B, int64_t n_entries, int d, int mode);
int mf_pool_forward(const float* table, int64_t n_rows, int d, const int64_t* seg_start, const int64_t* seg_end,
                    const int64_t* items, int64_t n_items, int64_t B, int64_t n_entries, int max_history, int mode,
                    int norm_item, int norm_user, float* out_u, float* out_inv, int32_t* out_count, int64_t* out_lo,
                    int64_t* out_off, int32_t* out_arg, void* ws, size_t ws_bytes, mf_stream_t stream);
/* Backward, coalesced with the rows other towers parked on the same table: grad_p [B, d] = dL/dp (after the normalise
 * backward, mf_normalize_backward); entry e of user b gets grad_p[b] / count[b] (mode 0) or grad_p[b] on the channels it won
 * (mode 1); the extra rows (extra_ids [n_extra], extra_grad [n_extra, d]; valid ids [0, n_rows)) join them.  Every entry is
 * summed per id in entry order (extras first) -- a stable radix sort by id, linear in the entries, no float atomics, no host
 * round trip.  out_ids [capacity] = the unique ids ascending, then -1; out_grad [capacity, d] their summed rows (rows of a -1
 * slot are not written).  capacity must be min(n_rows, n_extra + n_entries). */
size_t mf_pool_backward_ws_bytes(int64_t n_extra, int64_t n_entries, int d);
int mf_pool_backward(int64_t n_rows, int d, int mode, const int64_t* items, int64_t B, const int64_t* lo, const int64_t* ent_off,
                     const int32_t* count, const int32_t* arg, const float* grad_p, int64_t n_entries, const int64_t* extra_ids,
                     const float* extra_grad, int64_t n_extra, int64_t capacity, int64_t* out_ids, float* out_grad, void* ws,
                     size_t ws_bytes, mf_stream_t stream);
/* The history window of each example mf_sample_batch puts in row r (same Feistel permutation, same seed and start):
 * out_start[r] = pair_hist_lo[e], out_end[r] = pair_hist_hi[e] (InteractionTable.history_lo / history_hi of the train pairs). */
int mf_sample_history(const int64_t* pair_hist_lo, const int64_t* pair_hist_hi, int64_t n_pairs, uint64_t seed, int64_t start,
                      int64_t B, int64_t* out_start, int64_t* out_end, mf_stream_t stream);

/* ------------------------------------------------------------ hashed feature-bag towers ---
 * The id-only counterpart of the reference's attribute encoder (xfmr_rec/lightning.py:60-74 over the JSON text of
 * prepare.py:69-127): an EmbeddingBag over hashed attribute tokens.  Entity e's bag is tokens[seg_start[e], seg_end[e])
 * (clamped to [0, n_tokens), at most max_len entries) with weights (null: 1); bag b is entity idx[b] (idx null: b); an
 * entity outside [0, n_seg) is an empty bag; tokens outside [1, n_rows) are padding.  s_b = sum_e w_e F[t_e];
 * combiner 0 / 1 / 2 = sum / mean / sqrtn: c_b = 1, 1 / sum w_e, 1 / sqrt(sum w_e^2), and 0 when sum w_e = 0; p_b = c_b s_b;
 * u_b = normalize ? p_b / max(|p_b|, 1e-12) : p_b.  Outputs out_u [B, d], out_inv [B], out_scale [B] (= c_b).  max_len
 * sizes the workspace and grids (no host read); the summation order depends on the bag lengths only.  MF_ENOTSUP above
 * 2^20 table rows or B * max_len >= 2^31. */
size_t mf_bag_ws_bytes(int64_t B, int64_t max_len, int d);
int mf_bag_forward(const float* table, int64_t n_rows, int d, const int64_t* idx, int64_t B, const int64_t* seg_start,
                   const int64_t* seg_end, int64_t n_seg, const int64_t* tokens, int64_t n_tokens, const float* weights,
                   int64_t max_len, int combiner, int normalize, float* out_u, float* out_inv, float* out_scale, void* ws,
                   size_t ws_bytes, mf_stream_t stream);
/* Backward, coalesced with extra rows parked on the same table (extra_ids [n_extra], extra_grad [n_extra, d]; valid ids
 * [0, n_rows)): grad_p [B, d] = dL/dp (after mf_normalize_backward); entry e of bag b gets w_e * scale[b] * grad_p[b]
 * (entries with w_e = 0 or scale[b] = 0 are dropped).  A stable radix sort by id and a fixed tree of run sums, over the
 * entry count the plan kernel leaves on the device: no float atomics, no host round trip.  out_ids [capacity] = the unique
 * ids ascending, then -1; out_grad [capacity, d] their rows (-1 slots not written).  capacity must be
 * min(n_rows, n_extra + B * max_len). */
size_t mf_bag_backward_ws_bytes(int64_t n_extra, int64_t B, int64_t max_len, int d);
int mf_bag_backward(int64_t n_rows, int d, const int64_t* idx, int64_t B, const int64_t* seg_start, const int64_t* seg_end,
                    int64_t n_seg, const int64_t* tokens, int64_t n_tokens, const float* weights, int64_t max_len,
                    const float* scale, const float* grad_p, const int64_t* extra_ids, const float* extra_grad, int64_t n_extra,
                    int64_t capacity, int64_t* out_ids, float* out_grad, void* ws, size_t ws_bytes, mf_stream_t stream);

/* ------------------------------------------------------------ transformer user tower ---
 * The sequence form of the reference's tower, PoolingTransformer.forward(inputs_embeds) (xfmr_rec/models.py:66-84): a BERT
 * encoder over the item rows of a user's history, pooling_mode mean / max / cls (mode 0 / 1 / 2), then Normalize -- the
 * eval-mode function (no dropout), fp32.  Lists as for mf_pool_forward; the last max_history (<= 64) valid entries are kept,
 * oldest first (position 0), and PACKED: user b owns tokens tok_off[b] .. tok_off[b + 1], T = sum_b n_b <= t_cap, where t_cap
 * (a host bound, min(entries, B * max_history)) sizes every buffer and grid.  x_t = the item row (normalised iff norm_item),
 * e_t = LN((x_t + tok[0]) + pos[t]); per layer Q / K / V dense, `heads` heads, scores / sqrt(h / heads), softmax over the valid
 * keys, context, dense + residual + LN, dense + act (0 gelu, 1 relu, 2 silu, 3 gelu_new), dense + residual + LN; LN eps 1e-12.
 * params: 4 + 16 * layers device pointers: pos [max_pos, h], tok [2, h], LN gamma, beta, then per layer Wq bq Wk bk Wv bv Wo bo
 * g1 b1 Wi [I, h] bi Wo2 [h, I] bo2 g2 b2 (torch Linear layout [out, in]).  Outputs: out_u [B, h], out_inv [B], out_arg [B, h]
 * (mode 1: the winning position, -1 for an empty list); `stash` (mf_xfmr_ws_bytes) keeps the plan and the activations for
 * the backward.  h in {32, 64, 128}, head width in {8, 16, 32, 64}, I a multiple of 32 <= 4 h, 1..4 layers: MF_ENOTSUP
 * otherwise, and above 2^20 table rows.  Deterministic: no atomics. */
size_t mf_xfmr_ws_bytes(int64_t B, int64_t t_cap, int h, int layers, int intermediate);
int mf_xfmr_forward(const float* table, int64_t n_rows, int h, const int64_t* seg_start, const int64_t* seg_end,
                    const int64_t* items, int64_t n_items, int64_t B, int64_t t_cap, int max_history, int layers, int heads,
                    int intermediate, int act, int mode, int norm_item, int norm_user, const float* const* params, float* out_u,
                    float* out_inv, int32_t* out_arg, void* stash, size_t stash_bytes, mf_stream_t stream);
/* Backward of the dense part: grads = one buffer per parameter (the parameters' order and shapes), every element written;
 * grad_x [t_cap, h] = dL/dx_t of the packed tokens.  Weight gradients are split-K sums over a fixed number of token slices
 * added in slice order: bit-reproducible, no float atomics. */
size_t mf_xfmr_backward_ws_bytes(int64_t t_cap, int h, int intermediate);
int mf_xfmr_backward(int h, int64_t B, int64_t t_cap, int max_history, int max_pos, int layers, int heads, int intermediate,
                     int act, int mode, int norm_user, const float* const* params, float* const* grads, const void* stash,
                     const float* grad_u, const float* out_u, const float* out_inv, const int32_t* out_arg, float* grad_x,
                     void* ws, size_t ws_bytes, mf_stream_t stream);
/* Training dropout (BertModel's four sites; mf_xfmr_forward / mf_xfmr_backward are the case p_hidden = p_attn = 0 of the same
 * implementation): p_hidden drops the embeddings after their LayerNorm and the attention-output and FFN-output dense results
 * before their residual adds, p_attn the attention probabilities.  A probability counts as thr / 65536, thr = round(p * 65536)
 * (halves up, at most 65535); thr = 0 switches the site off; p outside [0, 1) is MF_EINVAL.  The masks are the counter-based
 * words of include/mf_numerics.h, keyed by (seed, call, site) and indexed by (user, position, column) or (user, query, head,
 * key) -- not by the packed token number, so they do not depend on the packing or the input form.  They are generated
 * inside the kernels: no mask tensor, nothing added to the stash (mf_xfmr_ws_bytes, mf_xfmr_coalesce unchanged); the backward,
 * called with the forward's (p_hidden, p_attn, seed, call), regenerates the same bits.  Its workspace holds one more [t_cap, h]
 * buffer than the plain backward's.  Still no float atomics: a step with dropout is bit-reproducible. */
int mf_xfmr_forward_dropout(const float* table, int64_t n_rows, int h, const int64_t* seg_start, const int64_t* seg_end,
                            const int64_t* items, int64_t n_items, int64_t B, int64_t t_cap, int max_history, int layers, int heads,
                            int intermediate, int act, int mode, int norm_item, int norm_user, const float* const* params,
                            float* out_u, float* out_inv, int32_t* out_arg, void* stash, size_t stash_bytes, double p_hidden,
                            double p_attn, uint64_t seed, uint64_t call, mf_stream_t stream);
size_t mf_xfmr_backward_dropout_ws_bytes(int64_t t_cap, int h, int intermediate);
int mf_xfmr_backward_dropout(int h, int64_t B, int64_t t_cap, int max_history, int max_pos, int layers, int heads, int intermediate,
                             int act, int mode, int norm_user, const float* const* params, float* const* grads, const void* stash,
                             const float* grad_u, const float* out_u, const float* out_inv, const int32_t* out_arg, float* grad_x,
                             void* ws, size_t ws_bytes, double p_hidden, double p_attn, uint64_t seed, uint64_t call,
                             mf_stream_t stream);
/* Mixed precision of the six dense layers of every encoder layer (Q, K, V, attention output, FFN in, FFN out).  precision =
 * MF_XFMR_FP32: the calls above (the four of them are this case of the same implementation).  MF_XFMR_BF16_MIXED: BOTH operands
 * of every GEMM of those layers -- Y = X W^T, dX = dY W, dW = dY^T X -- are rounded to bf16 (round-to-nearest-even) where they
 * are staged; the products are exact and accumulate in fp32 (v_mfma_f32_32x32x16_bf16); bias, residual, activation, its
 * derivative and the dropout multiply stay fp32, db stays the fp32 column sum of the unrounded dY, and outputs, stash,
 * parameters and every gradient stay fp32, as does everything that is not one of those GEMMs (LayerNorms, attention, pooling,
 * the position / token-type / table gradients).  Same stash and workspaces (mf_xfmr_ws_bytes, mf_xfmr_backward_dropout_ws_bytes),
 * same fixed split of dW over the tokens, no float atomics: bit-reproducible.  The backward takes the forward's precision.
 * Any other precision: MF_EINVAL. */
#define MF_XFMR_FP32 0
#define MF_XFMR_BF16_MIXED 1
int mf_xfmr_forward_mixed(const float* table, int64_t n_rows, int h, const int64_t* seg_start, const int64_t* seg_end,
                          const int64_t* items, int64_t n_items, int64_t B, int64_t t_cap, int max_history, int layers, int heads,
                          int intermediate, int act, int mode, int norm_item, int norm_user, const float* const* params,
                          float* out_u, float* out_inv, int32_t* out_arg, void* stash, size_t stash_bytes, double p_hidden,
                          double p_attn, uint64_t seed, uint64_t call, int precision, mf_stream_t stream);
int mf_xfmr_backward_mixed(int h, int64_t B, int64_t t_cap, int max_history, int max_pos, int layers, int heads, int intermediate,
                           int act, int mode, int norm_user, const float* const* params, float* const* grads, const void* stash,
                           const float* grad_u, const float* out_u, const float* out_inv, const int32_t* out_arg, float* grad_x,
                           void* ws, size_t ws_bytes, double p_hidden, double p_attn, uint64_t seed, uint64_t call, int precision,
                           mf_stream_t stream);
/* Serving encode: out_u [B, h] of mf_xfmr_forward -- the eval-mode function, fp32 -- and nothing else, in ONE launch: one
 * workgroup per user carries the user's <= 64 tokens from the cut of the list to the pooled, normalised vector in LDS.  No t_cap,
 * no stash, no workspace, no out_inv / out_arg, no host read; nothing per token is written to memory.  Same lists, params
 * (4 + 16 * layers pointers, same order), shape rules and MF_ENOTSUP cases as mf_xfmr_forward; null pointers, B <= 0, act
 * outside 0..3 or mode outside 0..2 are MF_EINVAL; all decided before any GPU call.  It calls the forward's own arithmetic in
 * the forward's order (each GEMM element one k-ascending v_mfma_f32_32x32x2_f32 chain): out_u is BIT-IDENTICAL to
 * mf_xfmr_forward's on the same inputs.  An empty list gives a zero row.  fp32 only: there is no bf16-mixed form. */
int mf_xfmr_encode(const float* table, int64_t n_rows, int h, const int64_t* seg_start, const int64_t* seg_end,
                   const int64_t* items, int64_t n_items, int64_t B, int max_history, int layers, int heads, int intermediate,
                   int act, int mode, int norm_item, int norm_user, const float* const* params, float* out_u, mf_stream_t stream);
/* ONE dense operation of that engine on the caller's row-major fp32 buffers, through the tower's own launches (for tests of
 * the arithmetic contract).  M tokens in [1, 2^31), N and K multiples of 32 in [32, 512] (MF_ENOTSUP otherwise).
 *   form 0: out [M, N] = a [M, K] b[N, K]^T + bias [N] (bias may be null)
 *   form 1: out [M, K] = a [M, N] b[N, K]
 *   form 2: out [N, K] = a [M, N]^T b[M, K], out_bias [N] = the column sums of a
 * form outside 0..2 or an unknown precision: MF_EINVAL, decided before any GPU call. */
size_t mf_xfmr_dense_ws_bytes(int form, int N, int K);
int mf_xfmr_dense(int form, int precision, int64_t M, int N, int K, const float* a, const float* b, const float* bias, float* out,
                  float* out_bias, void* ws, size_t ws_bytes, mf_stream_t stream);
/* Host only (no GPU call): out[i] = the mask word idx0 + i of (seed, call, stream), i < n -- what the kernels compute, for tests. */
int mf_dropout_words(uint64_t seed, uint64_t call, uint64_t stream, uint64_t idx0, int64_t n, uint64_t* out);
/* grad_x lands on the item table through the coalesce engine of the pooled towers (one entry per token, key = its item id),
 * together with the extra rows parked on the table: outputs as mf_pool_backward; capacity = min(n_rows, n_extra + t_cap). */
size_t mf_xfmr_coalesce_ws_bytes(int64_t n_extra, int64_t t_cap, int d);
int mf_xfmr_coalesce(int64_t n_rows, int d, int64_t B, int64_t t_cap, int layers, int intermediate, const void* stash,
                     const float* grad_x, const int64_t* extra_ids, const float* extra_grad, int64_t n_extra, int64_t capacity,
                     int64_t* out_ids, float* out_grad, void* ws, size_t ws_bytes, mf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MF_HIP_H */
