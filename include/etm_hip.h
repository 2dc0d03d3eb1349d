/*
 * etm_hip.h -- C ABI of libetm_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * PPO + TransformerXL episodic-memory training path.
 *
 * The reference (MarcoMeter/episodic-transformer-memory-ppo) has no native/FFI layer; each entry point
 * below replaces a stock-PyTorch op sequence of the reference (cited as file:line into the upstream
 * repository) and is what a reference-side ctypes binding would call.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch); the library borrows it for the
 *     duration of the enqueue and allocates nothing (exceptions: the event pool of etm_profile_*, the RCCL communicator
 *     of etm_comm_init);
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); no synchronisation;
 *   - return value: 0 on success, a hipError_t (> 0) from the launch (ETM_ERCCL_BASE + an ncclResult_t from the
 *     communicator entries), or a negative ETM_E* code for argument errors; nothing throws across the ABI;
 *   - fp32 tensors are dense row-major unless strides are given; indices are int64 (torch.long);
 *     masks are one byte per element (0 = masked);
 *   - thread-safety: calls are re-entrant; ordering is the stream's.
 */
#ifndef ETM_HIP_H
#define ETM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ETM_OK 0
#define ETM_EINVAL (-1)      /* bad dimension / null pointer */
#define ETM_EUNSUPPORTED (-2) /* shape outside what the gfx950 kernels are built for */
#define ETM_EWORKSPACE (-3)  /* workspace too small */
#define ETM_ENOCOMM (-4)     /* librccl could not be loaded / communicator entry used before etm_comm_init */
#define ETM_ETIMEOUT (-5)    /* etm_rollout_drive: a worker group did not publish a step within the time limit */
#define ETM_EABORTED (-6)    /* etm_rollout_drive: an environment worker reported an error / the abort word was set */
#define ETM_ERCCL_BASE 100000 /* ETM_ERCCL_BASE + ncclResult_t: an RCCL call failed */

/* ABI version of this header (bumped on any signature change, and when the meaning of an argument widens: 52 = the greedy
 * sentinel of the `uniforms` tables; 53 = + etm_gae_truncated; 54 = + the running-normalisation entries; 55 = + etm_grouped_dw_tile_map;
 * 56 = + etm_arena_digest; 57 = + the gated optimiser pair; 58 = + the *_masked entries of invalid-action masking;
 * 59 = + etm_grad_sqnorm_adaptive; 60 = + etm_block_row_groups; 61 = + the *_gaussian_means sampling entries and
 * etm_heads_loss_gaussian_kl of the exact Gaussian KL; still 61, added without a change to any signature above: the *_logps sampling
 * entries, etm_heads_loss_kl / etm_heads_loss_branched_kl and etm_ppo_loss_kl of the exact categorical KL). */
int etm_abi_version(void);

/* Human-readable name for a negative ETM_E* code or a hipError_t. Static storage. */
const char *etm_error_string(int code);

/* ---------------------------------------------------------------------------------------------
 * Kernel #1: episodic single-query multi-head attention over the sliding memory window.
 *
 * Replaces, for one transformer block, the reference sequence
 *   utils.py:52-75 batched_index_select (window gather, [N,L,nb,D] materialised)
 *   transformer.py:237-242 (+ positional rows indexed by the absolute episode index)
 *   transformer.py:131      (pre-LN: LayerNorm `norm_kv` over the window)
 *   transformer.py:50-51    (K = X Wk^T, V = X Wv^T  -- the dense [N*L, D] x [D, D] contractions)
 *   transformer.py:59-75    (energy = Q.K, masked_fill(mask == 0, -1e20), softmax(energy / sqrt(D)), att.V)
 * The query projection (transformer.py:52) and fc_out (:83) stay plain library GEMMs on the caller side.
 *
 * Window row (n, l) of the block is
 *     X[n,l,:] = bank[ep[n] * ep_stride + win[n,l] * row_stride + 0..D)   (+ pos[pidx[n,l], :])   (then LayerNorm)
 * so the caller passes `bank` already offset to the block (bank_base + block * D).
 *
 *   ep      [N]     episode slot per sample, or NULL for ep[n] = n
 *   win     [N,L]   row inside the episode (memory_indices of the reference)
 *   pidx    [N,L]   positional row (== win in training; differs in get_last_value, trainer.py:236), NULL iff pos == NULL
 *   mask    [N,L]   0 => masked (transformer.py:66)
 *   pos     [P,D]   positional table or NULL
 *   ln_g/ln_b [D]   norm_kv gain / bias or both NULL; ln_eps = 1e-5 in the reference
 *   q       [N,D]   projected queries
 *   wk, wv  [D,D]   torch Linear layout [out, in]
 * outputs
 *   ctx     [N,D]   attention output before fc_out
 *   att     [N,H,L] attention weights (the reference returns [N,H,1,L])
 *   k_save, v_save [N,L,D]  projected keys / values kept for the backward pass, or both NULL (inference)
 *   ln_stats [N,L,2] (mean, rstd) per window row: scratch written by a pre-pass, required iff ln_g != NULL
 *                    (kept by the caller for the backward pass)
 *
 * Shape support: D % 32 == 0, head_dim = D / H in {32,64,96,128}, 1 <= L <= 128.
 */
int etm_mha_fwd(const float *bank, int64_t ep_stride, int64_t row_stride,
                const int64_t *ep, const int64_t *win, const int64_t *pidx, const uint8_t *mask,
                const float *pos, const float *ln_g, const float *ln_b, float ln_eps,
                const float *q, const float *wk, const float *wv,
                float *ctx, float *att, float *k_save, float *v_save, float *ln_stats,
                int N, int L, int D, int H, void *stream);

/* Backward of etm_mha_fwd wrt q, Wk, Wv (and optionally norm_kv gain/bias and a learned positional
 * table).  The memory window itself is detached in the reference (transformer.py:248), so there is no
 * gradient into `bank`.
 *
 *   d_ctx  [N,D]    gradient wrt ctx
 *   att, k_save, v_save, ln_stats: as produced by the forward
 * outputs (all overwritten, not accumulated, except d_pos / d_ln_* which are ACCUMULATED into)
 *   d_q    [N,D]
 *   d_e    [N,H,L]  scratch/output: gradient wrt the masked, unscaled energies
 *   d_wk, d_wv [D,D]
 *   d_ln_g, d_ln_b [D]  or NULL   (accumulated; caller zero-fills)
 *   d_pos  [P,D]        or NULL   (accumulated; only for the learned table, transformer.py:213)
 *   workspace: etm_mha_bwd_workspace_bytes(N, L, D) bytes of scratch
 */
int64_t etm_mha_bwd_workspace_bytes(int N, int L, int D);

int etm_mha_bwd(const float *bank, int64_t ep_stride, int64_t row_stride,
                const int64_t *ep, const int64_t *win, const int64_t *pidx, const uint8_t *mask,
                const float *pos, const float *ln_g, const float *ln_b,
                const float *q, const float *wk, const float *wv,
                const float *att, const float *k_save, const float *v_save, const float *ln_stats,
                const float *d_ctx,
                float *d_q, float *d_e, float *d_wk, float *d_wv,
                float *d_ln_g, float *d_ln_b, float *d_pos,
                void *workspace, int64_t workspace_bytes,
                int N, int L, int D, int H, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Kernel #1, folded form (default training path): the same reference sequence as etm_mha_fwd / etm_mha_bwd
 * (utils.py:52-75, transformer.py:237-242, :131, :50-51, :59-75) for a SINGLE query per sample, without ever forming the
 * key / value projections of the window.  With u[n,h,:] = q[n,h,:] . Wk_h and z[n,h,:] = sum_l att[n,h,l] X[n,l,:]
 *     energy[n,h,l] = X[n,l,:] . u[n,h,:]          (== Q_h . K_h of transformer.py:59-62)
 *     ctx[n,h,:]    = z[n,h,:] . Wv_h^T            (== att . V_h of transformer.py:72-75)
 * so one pass over the gathered window rows (L*D*4 bytes per sample and block: HBM-bound) replaces the
 * two [N*L, D] x [D, D] contractions; the [hd, D] products per head (u, ctx and their gradients) are library GEMMs on the
 * caller side (etm/ops.py).  Results differ from the dense form only by fp32 summation order.
 *
 *   bank/ep/win/pidx/mask/pos/ln_g/ln_b/ln_eps/ln_stats: exactly as for etm_mha_fwd
 *   u, z, gz, du: element (h, n, c) at base[h * head_stride + n * sample_stride + c]   (strides in floats, even)
 * etm_window_fwd:  u -> att [N,H,L] (softmax(masked_fill(energy, -1e20) / sqrt(D))), z
 * etm_window_bwd:  gz = d loss / d z, att (saved) -> d_e [N,H,L] (gradient of the pre-scale logits; 0 where masked),
 *                  du[h,n,:] = sum_l d_e[n,h,l] X[n,l,:]
 * etm_window_dx:   LayerNorm gain / bias and learned positional table gradients (accumulated; caller zero-fills):
 *                  dX[n,l,:] = sum_h d_e[n,h,l] u[n,h,:] + att[n,h,l] gz[n,h,:] pushed through the LayerNorm;
 *                  uw = [2, N, H, D] contiguous (u, then gz).  No-op when d_ln_g and d_pos are both NULL.
 * Shape support: D % 32 == 0, head_dim even, L <= 128 for D <= 512, L <= 64 for D <= 1024 (ETM_EUNSUPPORTED otherwise:
 * use the dense pair above).
 */
int etm_window_fwd(const float *bank, int64_t ep_stride, int64_t row_stride,
                   const int64_t *ep, const int64_t *win, const int64_t *pidx, const uint8_t *mask,
                   const float *pos, const float *ln_g, const float *ln_b, float ln_eps,
                   const float *u, int64_t u_head_stride, int64_t u_sample_stride,
                   float *att, float *z, int64_t z_head_stride, int64_t z_sample_stride,
                   float *ln_stats, int stats_ready, int N, int L, int D, int H, void *stream);
/* (stats_ready != 0, round 5: ln_stats [N, L, 2] already holds (mean, 1 / sqrt(var + eps)) of every window row -- gathered by the
 * caller from per-BANK-row statistics computed once per update with etm_ln_row_stats -- and the pass over the window rows that
 * computes them is skipped; 0: computed here, as before.) */
/* Gradients of norm_kv's gain / bias for the folded pre-LN attention (transformer.py:128-131 under trainer.py:310; round 5,
 * csrc/window_ln_grad.hip; replaces etm_window_dx where the positional table is not learnable): partial
 * [etm_window_ln_grad_rows(N)][2 D] = per-workgroup sums [d gain | d bias]; the caller adds the rows in a fixed order
 * (etm_colsum_reduce_grouped).  u / gz = the folded vectors [H, N, D] (strides in floats), att / d_e [N, H, L] as etm_window_bwd
 * leaves them, ln_stats [N, L, 2]; pos / pidx NULL when the bank rows already contain their positional rows.  D % 128 == 0,
 * D <= 512, H <= 8, L <= 128, else ETM_EUNSUPPORTED.  Deterministic (no atomics). */
int etm_window_ln_grad_rows(int N);
int etm_window_ln_grad(const float *bank, int64_t ep_stride, int64_t row_stride, const int64_t *ep, const int64_t *win,
                       const int64_t *pidx, const float *pos, const float *ln_stats, const float *att, const float *d_e,
                       const float *u, const float *gz, int64_t vec_head_stride, int64_t vec_sample_stride, float *partial,
                       int N, int L, int D, int H, void *stream);
/* Round 6: the same partial rows from the window passes' OUTPUTS, without reading a window row: with xfull = xhat g + b,
 * d gain = (1 / g) sum_{n,h} u (du - b sdE) + gz (z - b satt) and d bias = sum_{n,h} u sdE + gz satt (sdE / satt: row sums of d_e / att;
 * du = etm_window_bwd's output, z = etm_window_fwd's).  u / gz / du / z [H, N, D] (one pair of strides), att / d_e [N, H, L], ln_g / ln_b
 * [D].  D % 128 == 0, D <= 512.  The identity divides by the gain: a column with |g| < tau max(1, |b|) (a zero gain included) needs
 * etm_window_ln_grad_guarded on the same `partial` afterwards. */
int etm_window_ln_grad_from_outputs(const float *u, const float *gz, const float *du, const float *z, const float *att, const float *d_e,
                                    const float *ln_g, const float *ln_b, int64_t vec_head_stride, int64_t vec_sample_stride,
                                    float *partial, int N, int L, int D, int H, void *stream);
/* The guard of etm_window_ln_grad_from_outputs (launched right after it, same stream, same `partial`): etm_window_ln_grad's arguments
 * plus norm_kv's ln_g / ln_b [D] and tau >= 0.  Does nothing unless some column c has |ln_g[c]| < tau max(1, |ln_b[c]|); then
 * overwrites the d gain entry partial[r][c] of exactly those columns, in every row r, with etm_window_ln_grad's sums (other entries
 * are not written).  Same limits as etm_window_ln_grad. */
int etm_window_ln_grad_guarded(const float *bank, int64_t ep_stride, int64_t row_stride, const int64_t *ep, const int64_t *win,
                               const int64_t *pidx, const float *pos, const float *ln_stats, const float *att, const float *d_e,
                               const float *u, const float *gz, int64_t vec_head_stride, int64_t vec_sample_stride,
                               const float *ln_g, const float *ln_b, float tau, float *partial, int N, int L, int D, int H, void *stream);
/* stats [R, 2] = (mean, 1 / sqrt(var + eps)) of the R contiguous rows of x [R, D]: LayerNorm statistics of the memory bank's rows,
 * once per update (norm_kv's statistics do not depend on its gain / bias).  D % 128 == 0, D <= 1024. */
int etm_ln_row_stats(const float *x, float eps, float *stats, int64_t R, int D, void *stream);
int etm_window_bwd(const float *bank, int64_t ep_stride, int64_t row_stride,
                   const int64_t *ep, const int64_t *win, const int64_t *pidx, const uint8_t *mask,
                   const float *pos, const float *ln_g, const float *ln_b, const float *ln_stats,
                   const float *att, const float *gz, int64_t gz_head_stride, int64_t gz_sample_stride,
                   float *d_e, float *du, int64_t du_head_stride, int64_t du_sample_stride,
                   int N, int L, int D, int H, void *stream);
int etm_window_dx(const float *bank, int64_t ep_stride, int64_t row_stride,
                  const int64_t *ep, const int64_t *win, const int64_t *pidx,
                  const float *pos, const float *ln_g, const float *ln_b, const float *ln_stats,
                  const float *att, const float *d_e, const float *uw,
                  float *d_ln_g, float *d_ln_b, float *d_pos,
                  int N, int L, int D, int H, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Rollout-time variant of kernel #1 over CACHED key/value projections (inference only, no backward).
 * During sampling the weights are frozen and an item's positional row is fixed by its absolute episode index
 * (transformer.py:237-239), so the trainer projects each new memory item once (library GEMM) into a cache
 * [W, T, blocks, 2D] (K in [0,D), V in [D,2D)) and this kernel performs transformer.py:59-75 for the single query.
 *   kv: cache already offset to the block (base + block * 2D); ep_stride/row_stride in floats; ep NULL => ep[n] = n
 *   ctx [N,D]; att [N,H,L] or NULL.   Shape support: head_dim % 4 == 0, head_dim <= 256, L <= 128.
 * etm_reset_rows: dst[w, 0..row_elems) = init[0..row_elems) for every w with step[w] == 0 (a new episode starts from
 * the projection of an all-zero memory); touches only the flagged workers.
 */
int etm_attn_cached(const float *kv, int64_t ep_stride, int64_t row_stride, const int64_t *ep, const int64_t *win,
                    const uint8_t *mask, const float *q, float *ctx, float *att, int N, int L, int D, int H, void *stream);
int etm_reset_rows(float *dst, const float *init, const int64_t *step, int W, int64_t row_elems, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Rollout-step glue (trainer.py:161-186).  At n_workers = 32 a step is bound by the number of launches, so these fuse
 * what would be ~8 / ~17 / 2 framework launches into one each.  All operands have fixed addresses (HIP-graph friendly);
 * `t_dev` is a device-resident step counter, staging arrays are time-major [S, W, ...].
 * Worker GROUPS: the staging arrays and `uniforms` are stage_W workers wide per time row; a call handles W <= stage_W
 * consecutive workers and receives those pointers already offset to its first worker (the trainer steps two groups of
 * workers as a software pipeline: one group's head graph runs while the host steps the other group's environments).
 *   etm_rollout_window: mask_t[w] = mask_table[clip(step[w], 0, L-1)], win_t[w] = index_table[step[w]] (trainer.py:165-166),
 *                       also stored to row *t_dev of st_mask / st_idx.  Optional riders of the same launch: *t_row = *t_dev
 *                       (t_row non-NULL), etm_reset_rows(reset_dst, reset_init, step, W, reset_row_elems) (reset_dst non-NULL), and
 *                       the (step, slot) LATCH (latch non-NULL): `step` is then row 0 of a contiguous [2, W] block whose row 1
 *                       holds the workers' episode slots, and latch[2, W] receives a copy of the block.  The tail of the step
 *                       (bank / cache writes, trainer.py:174) indexes the latch, so the host may upload the next step's block
 *                       on another stream while the tail is still running.
 *   etm_rollout_sample: per worker log-softmax of logits [W,A], categorical sample by inverse CDF with the pre-drawn
 *                       uniform uniforms[*t_dev, w], log-prob; writes actions [W] and row *t_dev
 *                       (forced, optional: time-major int64 table like `uniforms`; a non-negative entry forced[*t_dev, w] is
 *                       taken instead of sampling -- teacher forcing for parity tests -- a negative entry means "sample")
 *                       of st_actions / st_logp / st_values, then *t_dev += 1 (trainer.py:179-186).
 *                       GREEDY SENTINEL (ABI 52), at every `uniforms` parameter of this header (etm_rollout_sample[_branched],
 *                       etm_rollout_policy[_branched], etm_rollout_trxl[_branched], the group kernels): an entry u < 0 that is not
 *                       forced selects the MODE of its branch, the smallest index whose logit equals the branch's fp32 maximum;
 *                       the log-prob is that action's, as for a draw.  Entries in [0, 1) (and NaN) take the inverse CDF with the
 *                       operations of ABI 51, bit for bit.  The sentinel is per (step, worker, branch) entry of the fixed-address
 *                       table, so one captured step graph serves sampled and greedy rollouts.  Box policies (`normals`) have no
 *                       sentinel: a zero normal stores the mean.
 *   etm_add_layernorm:  out = LayerNorm(act(a + a_bias) + b) (residual + post-LN, transformer.py:145-149 / :166-170), forward only,
 *                       D <= 1024; a_bias [D] (or NULL) and relu fold the bias / ReLU of the linear layer that produced `a`.
 */
int etm_rollout_window(const int64_t *step, const uint8_t *mask_table, const int64_t *index_table, const int64_t *t_dev,
                       uint8_t *mask_t, int64_t *win_t, uint8_t *st_mask, int64_t *st_idx,
                       int64_t *t_row, int64_t *latch, float *reset_dst, const float *reset_init, int64_t reset_row_elems,
                       int W, int L, int stage_W, void *stream);
/* REFUSALS of the six etm_rollout_sample* entries, in the order in which they win (a refused call launches nothing):
 *   categorical: a NULL mandatory action_mask (*_masked); a NULL or 4-byte-misaligned st_logps (*_logps); a NULL mandatory pointer
 *   (all but forced), W <= 0 or A <= 0 -- a branch table that is NULL, holds a size <= 0 or has more than 16 entries makes A = 0 --:
 *   ETM_EINVAL; an action_mask that is not 8-byte aligned: ETM_EINVAL, then one over more than 63 columns: ETM_EUNSUPPORTED.
 *   Gaussian: a NULL mandatory pointer (all but forced, low, high) or W <= 0; a NULL or misaligned st_means (*_means): ETM_EINVAL;
 *   the Box table: A <= 0 ETM_EINVAL, A > 8 ETM_EUNSUPPORTED, a low above its high ETM_EINVAL. */
int etm_rollout_sample(const float *logits, const float *value, const float *uniforms, const int64_t *forced, int64_t *t_dev,
                       int64_t *actions, int64_t *st_actions, float *st_logp, float *st_values, int W, int A, void *stream);
/* MultiDiscrete (ABI 48): logits [W, sum sizes] hold the B = n_branches branches' segments side by side (branch b: columns
 * [off_b, off_b + sizes[b]), sizes = branch_sizes, a HOST array of B <= 16 entries).  Per branch: log-softmax over its own segment, the
 * inverse CDF of etm_rollout_sample at its own uniform uniforms[*t_dev, w, b] (or forced[*t_dev, w, b] when >= 0); actions [W, B],
 * st_actions / st_logp [S, W, B], st_values [S, W].  B = 1 is exactly etm_rollout_sample. */
int etm_rollout_sample_branched(const float *logits, const float *value, const float *uniforms, const int64_t *forced, int64_t *t_dev,
                                int64_t *actions, int64_t *st_actions, float *st_logp, float *st_values, int W, const int32_t *branch_sizes,
                                int n_branches, void *stream);
/* Invalid-action masks (ABI 58): the workers' words for this step, action_mask [W] int64 -- bit j set = column j of the concatenated
 * logits is allowed; branch b owns bits [off_b, off_b + sizes[b]); bits >= sum sizes are ignored; every branch has a valid action (the
 * caller's duty: a word with an empty branch must not reach the device).  Per branch the logit of an invalid action reads as -inf in
 * front of the same sampling arithmetic: the draw (sampled, greedy) is the unmasked draw on the branch compacted to its valid
 * actions, the staged log-prob is l_a - lse over the valid actions; a forced action is taken as it is.  A Discrete policy is one
 * branch (n_branches = 1).  sum sizes <= 63.  Refusals: see above. */
int etm_rollout_sample_branched_masked(const float *logits, const float *value, const float *uniforms, const int64_t *forced,
                                       int64_t *t_dev, int64_t *actions, int64_t *st_actions, float *st_logp, float *st_values, int W,
                                       const int32_t *branch_sizes, int n_branches, const int64_t *action_mask, void *stream);
/* The exact categorical KL (`exact_kl: true`; added at ABI 61): the *_logps form of each of the four categorical sampling entries takes
 * its *_branched_masked twin's arguments with action_mask OPTIONAL (NULL: no masks -- then the unmasked twin's refusals hold) and
 * st_logps before the stream: [S, W, sum sizes] (or [S, stage_W, sum sizes] at this group's first worker) next to st_actions.  It
 * receives l_j - lse of every column of every branch of the row -- the policy's distribution whether the action was sampled, taken
 * greedily (u < 0) or forced; exactly -inf for a masked-out column; at the taken action the st_logp entry's bits (the same expression
 * with the same lse).  Every other output is the twin's, bit for bit.  A Discrete policy is one branch.  Refusals: the family's
 * comment of each entry. */
int etm_rollout_sample_branched_logps(const float *logits, const float *value, const float *uniforms, const int64_t *forced,
                                      int64_t *t_dev, int64_t *actions, int64_t *st_actions, float *st_logp, float *st_values, int W,
                                      const int32_t *branch_sizes, int n_branches, const int64_t *action_mask, float *st_logps,
                                      void *stream);
/* Box policies (ABI 49): a diagonal Gaussian over A <= 8 dimensions.  mean [W, A] = the policy head's outputs; x = mean + exp(log_std)
 * normals[*t_dev, w] (log_std [A] on the device; normals / forced / st_actions time-major [S, W, A]; a forced row entry that is not NaN
 * replaces the draw of its dimension); st_logp[*t_dev, w] = log p(x) = sum_a [-((x_a - mean_a) / sigma_a)^2 / 2 - log sigma_a - log(2 pi) / 2]
 * of the stored x; st_values [S, W]; actions [W, A] = clip(x, low, high) (low / high: HOST arrays of A floats, NULL = unbounded). */
int etm_rollout_sample_gaussian(const float *mean, const float *value, const float *log_std, const float *normals, const float *forced,
                                int64_t *t_dev, float *actions, float *st_actions, float *st_logp, float *st_values, const float *low,
                                const float *high, int W, int A, void *stream);
/* The exact Gaussian KL (ABI 61; `kl_estimator: analytic`): the *_gaussian_means form of each of the four Gaussian sampling entries
 * takes its twin's arguments and st_means before the stream -- [S, W, A] (or [S, stage_W, A] at this group's first worker) next to
 * st_actions -- and stores the policy's mean of every dimension there as well, forced action or not; every other output is the twin's,
 * bit for bit.  Refusals: the family's comment of each entry. */
int etm_rollout_sample_gaussian_means(const float *mean, const float *value, const float *log_std, const float *normals, const float *forced,
                                      int64_t *t_dev, float *actions, float *st_actions, float *st_logp, float *st_values, const float *low,
                                      const float *high, int W, int A, float *st_means, void *stream);
int etm_add_layernorm(const float *a, const float *a_bias, int relu, const float *b, const float *gamma, const float *beta, float eps,
                      float *out, int N, int D, void *stream);
/* Elementwise parts of the GTrXL GRU gate on the rollout path (transformer.py:287-298), around concatenated library GEMMs
 * a = y [Wr;Wz;Wg]^T [N,3D], b = x [Ur;Uz]^T [N,2D], c = rx Ug^T [N,D]:
 *   etm_gru_gate_rz : r = sigmoid(a_r + b_r); z = sigmoid(a_z + b_z - bg); rx = r * x        (writes rx, z)
 *   etm_gru_gate_out: out = (1 - z) * x + z * tanh(a_g + c) */
int etm_gru_gate_rz(const float *a, const float *b, const float *bg, const float *x, float *rx, float *z, int N, int D, void *stream);
int etm_gru_gate_out(const float *a, const float *c, const float *z, const float *x, float *out, int N, int D, void *stream);
/* ---------------------------------------------------------------------------------------------
 * Training-side epilogues of a transformer block, forward and backward (transformer.py:117-172, :287-298); csrc/block_train.hip.
 * Called from the autograd functions behind TransformerBlock / GRUGate (etm/ops.py: fused_layernorm, gru_gate_train); the
 * dense [N, D] x [D, D] products in between stay library GEMMs.
 *   etm_ln_train_fwd: y = LayerNorm(act(a + a_bias) + b) * gamma + beta.  a [N,D] = raw output of the linear layer in front
 *                     (a_bias [D] / relu = its bias / ReLU; NULL / 0 for none), b [N,D] = residual branch (or NULL).
 *                     s_out [N,D] (optional) receives the LayerNorm input, stats [N,2] (optional) = (mean, 1/std) per row:
 *                     what etm_ln_train_bwd needs.  Replaces `self.norm1(attention + query)`, `self.norm2(forward + h)`
 *                     (post-LN, transformer.py:145-149, :166-170) and the plain `self.norm1(query)` / `self.norm2(h)` of the
 *                     pre-LN layout (:131-141).
 *   etm_ln_train_bwd: dy (+ dy2, optional: the output's second consumer -- a GEMM and the next residual branch both read it --
 *                     whose gradient is added on load instead of by a launch of its own) [N,D] -> ds [N,D] (gradient of the
 *                     LayerNorm input = gradient of the residual branch b, and of `a`
 *                     when relu == 0), da [N,D] (relu != 0 only: ds where a + a_bias > 0), and dgamma_dbeta_dbias [3,D] =
 *                     column sums of (dy * xhat, dy, da).  Two launches (rows, then a fixed-order sum of per-workgroup
 *                     partial sums held in `workspace`, etm_ln_train_bwd_workspace_bytes(N, D) bytes): deterministic.
 *                     dgamma_dbeta_dbias NULL: the second launch is left out -- `workspace` then holds
 *                     etm_ln_train_bwd_partial_rows(N) rows of 3 D partial sums for etm_colsum_reduce_grouped.
 *   etm_gate_train_*: the GTrXL GRU gate around three concatenated GEMMs A = y [Wr;Wz;Wg]^T [N,3D], B = x [Ur;Uz]^T [N,2D],
 *                     C = (r x) Ug^T [N,D]:
 *       rz  : r = sigmoid(A_r + B_r), z = sigmoid(A_z + B_z - bg), rx = r x              (writes r, z, rx)
 *       out : hh = tanh(A_g + C), out = (1 - z) x + z hh                                  (writes hh, out)
 *       bwd1: dout (+ dout2 when not NULL: the gate's output fed two consumers and their gradients arrive separately)
 *             -> dA[:, 2D:3D] = dout z (1 - hh^2); dA[:, D:2D] = dB[:, D:2D] = dout (hh - x) z (1 - z);
 *             dx1 = dout (1 - z); dbg [D] = - column sums of dA[:, D:2D]   (then the caller forms drx = dA[:, 2D:3D] Ug);
 *             dbg == NULL: `workspace` keeps etm_gate_train_bwd_partial_rows(N) rows of D partial sums for etm_colsum_reduce_grouped
 *       bwd2: drx -> dA[:, 0:D] = dB[:, 0:D] = drx x r (1 - r); dx2 = dx1 + drx r
 *             (then dy = dA [Wr;Wz;Wg], dx = dx2 + dB [Ur;Uz], d[Wr;Wz;Wg] = dA^T y, d[Ur;Uz] = dB^T x, dUg = dA[:, 2D:3D]^T rx)
 *   etm_block_row_groups (ABI 60, host only): the row kernels (ln_train_fwd / ln_train_bwd / gate_train_bwd1) are instantiated for
 *                     NJ in {1, 2, 4, 6, 8, 12, 16} column groups of 64 per lane; this returns the NJ a launch at width D runs (the
 *                     smallest member >= ceil(D / 64)), evaluated by the launches' own dispatch.  ETM_EUNSUPPORTED for D > 1024 (as the
 *                     launches), ETM_EINVAL for D <= 0.  For tests that must reach every instantiation.
 */
int etm_block_row_groups(int D);
int etm_ln_train_fwd(const float *a, const float *a_bias, int relu, const float *b, const float *gamma, const float *beta, float eps,
                     float *y, float *s_out, float *stats, int N, int D, void *stream);
int64_t etm_ln_train_bwd_workspace_bytes(int N, int D);
int etm_ln_train_bwd(const float *dy, const float *dy2, const float *s, const float *stats, const float *gamma, const float *a, const float *a_bias,
                     int relu, float *ds, float *da, float *dgamma_dbeta_dbias, float *workspace, int64_t workspace_bytes, int N, int D,
                     void *stream);
int etm_ln_train_bwd_partial_rows(int N);
/* Second stage of several column-sum gradients in ONE launch (the LayerNorm / bias gradients of a whole backward pass, collected by
 * etm/ops.py DeferredDw): out[i][c] = sum over p < P[i] of partial[i][p * ld[i] + c], c < C[i]; host arrays of n <=
 * etm_colsum_reduce_max_problems() entries; the summation tree of the per-call reductions (bit-identical results). */
int etm_colsum_reduce_max_problems(void);
int etm_colsum_reduce_grouped(const float *const *partial, const int *P, const int *C, const int *ld, float *const *out, int n, void *stream);
int etm_gate_train_rz(const float *A, const float *B, const float *bg, const float *x, float *r, float *z, float *rx, int N, int D,
                      void *stream);
int etm_gate_train_out(const float *A, const float *C, const float *z, const float *x, float *hh, float *out, int N, int D, void *stream);
int64_t etm_gate_train_bwd_workspace_bytes(int N, int D);
int etm_gate_train_bwd_partial_rows(int N);
int etm_gate_train_bwd1(const float *dout, const float *dout2, const float *z, const float *hh, const float *x, float *dA, float *dB, float *dx1, float *dbg,
                        float *workspace, int64_t workspace_bytes, int N, int D, void *stream);
int etm_gate_train_bwd2(const float *drx, const float *x, const float *r, const float *dx1, float *dA, float *dB, float *dx2, int N, int D,
                        void *stream);

/* ---------------------------------------------------------------------------------------------
 * Policy / value heads + PPO loss, forward and backward in one pass: replaces, for a single-branch policy, model.py:101-110 (bias +
 * ReLU of lin_policy / lin_value, the policy branch, the value head) together with the loss section of trainer.py:276-304, :315-316
 * (= etm_ppo_loss) and the first steps of `loss.backward()` (trainer.py:310) back to the pre-activations of the two hidden heads.
 *   pre_p / pre_v [N, hid] = h lin_policy.weight^T / h lin_value.weight^T WITHOUT bias (plain GEMMs of the caller); b_lp / b_lv [hid];
 *   wb [A, hid], bb [A]: policy branch; wv [hid], bv [1]: value head; actions / old_logp / adv / old_value / adv_stats3 / clip /
 *   vf_coef / beta / scales / dyn_clip_beta: as etm_ppo_loss.
 *   Outputs: gm_p / gm_v [N, hid] = d loss / d (pre + bias) of the hidden heads (the caller continues with d h = gm_p Wlp + gm_v Wlv and
 *   d Wlp = gm_p^T h ...); sums [etm_heads_loss_row_floats(hid, A)] = [d b_lp (hid) | d b_lv (hid) | d wv (hid) | d Wb (A x hid) |
 *   d bb (A) | d bv | 5 raw statistic sums]; out8 as etm_ppo_loss; logits [N, A] / value [N] optional (NULL: not written).
 *   workspace: etm_heads_loss_workspace_bytes(N, hid, A) bytes (one partial row per 8 samples, summed in row order: deterministic).
 * Shapes: etm_heads_loss_supported(N, hid, A) == 1 (hid % 64 == 0, hid <= 512, A <= 8).
 *
 * Refusals of the loss entries.  Every etm_heads_loss* entry refuses a defective call with nothing launched and nothing written; of
 * two defects the one earlier in this list decides the code.  Each step applies to the entries that take the operand it names:
 *   1. kl_coef NULL or not 4-byte aligned                                                              -> ETM_EINVAL
 *   2. old_logps NULL or not 4-byte aligned; etm_heads_loss_kl[_penalty]: old_logps_stride < A; xact, old_mean or old_log_std
 *      NULL, old_mean / old_log_std not 4-byte aligned; the action_mask of the *_masked entries NULL        -> ETM_EINVAL
 *   3. *_branched*: etm_heads_loss_supported_branched(...) == 0 (a NULL or non-positive size table too)     -> ETM_EUNSUPPORTED
 *   4. *_branched*: action_stride or logp_stride < n_branches, old_logps_stride < sum sizes; *_gaussian*: action_stride < A,
 *      logp_stride < 1, old_mean_stride < A                                                                -> ETM_EINVAL
 *   5. a NULL among the other pointers (logits, value and dyn_clip_beta may be NULL)                        -> ETM_EINVAL
 *   6. action_mask not 8-byte aligned -> ETM_EINVAL (more than 63 columns under a mask: ETM_EUNSUPPORTED)
 *   7. etm_heads_loss_supported / _supported_gaussian(N, hid, A) == 0                                       -> ETM_EUNSUPPORTED
 *   8. workspace_bytes below the entry's *_workspace_bytes(N, hid, A)                                       -> ETM_EWORKSPACE
 * The etm_ppo_loss* entries follow the same list without the steps on shapes of the heads: 1; 2 with logps_off < 0 and
 * old_logps_stride < logps_off + A; 5 with value, old_value and d_value required when include_value != 0, then N <= 0 or A <= 0
 * -> ETM_EINVAL; a mask with mask_shift < 0 or mask_shift + A > 63 -> ETM_EUNSUPPORTED; 6; 8. */
int etm_heads_loss_supported(int N, int hid, int A);
int etm_heads_loss_row_floats(int hid, int A);
int64_t etm_heads_loss_workspace_bytes(int N, int hid, int A);
int etm_heads_loss(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb, const float *bb,
                   const float *wv, const float *bv, const int64_t *actions, int64_t action_stride, const float *old_logp,
                   int64_t logp_stride, const float *adv, const float *old_value, const float *adv_stats3, double clip, float vf_coef,
                   float beta, float pol_scale, float ent_scale, float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v,
                   float *sums, float *out8, float *logits, float *value, void *workspace, int64_t workspace_bytes, int N, int hid,
                   int A, void *stream);
/* MultiDiscrete policies (ABI 48): the same pass over B = n_branches action branches of sizes branch_sizes[B] (HOST array).  wb / bb =
 * the branches' heads concatenated ([sum sizes, hid], [sum sizes]; branch b owns the rows after those of branches < b); actions /
 * old_logp rows carry one entry per branch (strides >= B).  Per branch: log-softmax over its own logits and a ratio, the sample's
 * normalised advantage repeated over the branches; the policy term, KL and clip fraction are summed over (sample, branch) and scaled
 * by pol_scale (1 / (N B) for ref_algo.ppo_loss), the entropy is the sum over the branches (ent_scale 1 / N).  The sums row is laid
 * out as in etm_heads_loss with A = sum sizes (d Wb / d bb: the concatenated heads).  Shapes: etm_heads_loss_supported_branched
 * (sum sizes <= 8, B <= 8, hid as etm_heads_loss). */
int etm_heads_loss_supported_branched(int N, int hid, const int32_t *branch_sizes, int n_branches);
int etm_heads_loss_branched(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb, const float *bb,
                            const float *wv, const float *bv, const int64_t *actions, int64_t action_stride, const float *old_logp,
                            int64_t logp_stride, const float *adv, const float *old_value, const float *adv_stats3, double clip, float vf_coef,
                            float beta, float pol_scale, float ent_scale, float val_scale, const double *dyn_clip_beta, float *gm_p,
                            float *gm_v, float *sums, float *out8, float *logits, float *value, void *workspace, int64_t workspace_bytes,
                            int N, int hid, const int32_t *branch_sizes, int n_branches, void *stream);
/* Invalid-action masks (ABI 58): etm_heads_loss / etm_heads_loss_branched with action_mask [N] int64, the samples' words in the layout
 * of etm_rollout_sample_branched_masked (the word the sample was drawn under; the taken action is among its set bits).  Per branch
 * with valid set V: lse_V over V only, log p_j = l_j - lse_V on V and p_j = 0 elsewhere, entropy -sum_{j in V} p_j log p_j (invalid
 * columns are skipped, not multiplied), d loss / d l_j = 0 exactly for j outside V -- so that sample adds nothing to those rows of
 * d Wb / d bb; a branch with one valid action has log p = 0, entropy 0 and a zero gradient.  Ratio, clipping, KL, clip fraction, value
 * loss and scales as without masks; the optional logits output stays raw.  Refusals: the list above. */
int etm_heads_loss_masked(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb, const float *bb,
                          const float *wv, const float *bv, const int64_t *actions, int64_t action_stride, const float *old_logp,
                          int64_t logp_stride, const float *adv, const float *old_value, const float *adv_stats3, double clip, float vf_coef,
                          float beta, float pol_scale, float ent_scale, float val_scale, const double *dyn_clip_beta, float *gm_p,
                          float *gm_v, float *sums, float *out8, float *logits, float *value, void *workspace, int64_t workspace_bytes,
                          int N, int hid, int A, const int64_t *action_mask, void *stream);
int etm_heads_loss_branched_masked(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                   const float *bb, const float *wv, const float *bv, const int64_t *actions, int64_t action_stride,
                                   const float *old_logp, int64_t logp_stride, const float *adv, const float *old_value,
                                   const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                                   float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v, float *sums, float *out8,
                                   float *logits, float *value, void *workspace, int64_t workspace_bytes, int N, int hid,
                                   const int32_t *branch_sizes, int n_branches, const int64_t *action_mask, void *stream);
/* The exact categorical KL (added at ABI 61): etm_heads_loss_masked / etm_heads_loss_branched_masked with action_mask OPTIONAL (NULL:
 * no masks) and old_logps [N, A] (row stride old_logps_stride >= A floats; A = sum sizes), every column's log-prob under the policy
 * that drew the samples (the *_logps sampling entries).  The same launch also reduces KL(old || new): per sample n and branch b with
 * valid columns V, KL_nb = sum_{j in V} t_j, t_j = p_old_j (expm1(-d_j) + d_j) for d_j = old_logp_j - logp_j >= -60, t_j = p_j below
 * (the limit p_old_j -> 0); every term >= 0, no term of size 1 cancels, equal policies give exactly 0, a masked-out column is skipped,
 * a branch with one valid action contributes 0.  out8[4] = pol_scale sum_n sum_b KL_nb (pol_scale = 1 / (N B): the mean over samples
 * AND branches, the convention of the k3 value; the joint KL is B times it), out8[6] = the k3 value that the twin puts into out8[4].
 * A statistic only (unless `kl_penalty`, the *_kl_penalty entries): the loss, gm_p, gm_v, out8[0..3], out8[5] and the twin's row are
 * the twin's bit for bit; sums
 * [etm_heads_loss_kl_row_floats = etm_heads_loss_row_floats + 1] carries the raw KL sum as its last element.  Refusals: the list
 * above. */
int etm_heads_loss_kl_row_floats(int hid, int A);
int64_t etm_heads_loss_kl_workspace_bytes(int N, int hid, int A);
int etm_heads_loss_kl(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb, const float *bb,
                      const float *wv, const float *bv, const int64_t *actions, int64_t action_stride, const float *old_logp,
                      int64_t logp_stride, const float *adv, const float *old_value, const float *adv_stats3, double clip, float vf_coef,
                      float beta, float pol_scale, float ent_scale, float val_scale, const double *dyn_clip_beta, float *gm_p,
                      float *gm_v, float *sums, float *out8, float *logits, float *value, void *workspace, int64_t workspace_bytes,
                      int N, int hid, int A, const int64_t *action_mask, const float *old_logps, int64_t old_logps_stride,
                      void *stream);
int etm_heads_loss_branched_kl(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                               const float *bb, const float *wv, const float *bv, const int64_t *actions, int64_t action_stride,
                               const float *old_logp, int64_t logp_stride, const float *adv, const float *old_value,
                               const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                               float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v, float *sums, float *out8,
                               float *logits, float *value, void *workspace, int64_t workspace_bytes, int N, int hid,
                               const int32_t *branch_sizes, int n_branches, const int64_t *action_mask, const float *old_logps,
                               int64_t old_logps_stride, void *stream);
/* Box policies (ABI 49): the same pass for a diagonal Gaussian (A <= 8): wb / bb = the mean head; xact [N, A] (row stride
 * action_stride >= A) the stored raw float actions; log_std [A]; old_logp [N] (logp_stride).  Per sample one ratio of the joint
 * log-probs; d log p / d mean_a = (x_a - mean_a) / sigma_a^2, d log p / d log sigma_a = ((x_a - mean_a) / sigma_a)^2 - 1, the entropy
 * sum_a (1/2 + log(2 pi) / 2 + log sigma_a) adds -beta ent_scale per sample to every d log sigma_a.  sums
 * [etm_heads_loss_gaussian_row_floats = etm_heads_loss_row_floats + A] = the etm_heads_loss row followed by d log_std (A), summed in
 * the same fixed order (no atomics). */
int etm_heads_loss_supported_gaussian(int N, int hid, int A);
int etm_heads_loss_gaussian_row_floats(int hid, int A);
int64_t etm_heads_loss_gaussian_workspace_bytes(int N, int hid, int A);
int etm_heads_loss_gaussian(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb, const float *bb,
                            const float *wv, const float *bv, const float *xact, int64_t action_stride, const float *log_std,
                            const float *old_logp, int64_t logp_stride, const float *adv, const float *old_value, const float *adv_stats3,
                            double clip, float vf_coef, float beta, float pol_scale, float ent_scale, float val_scale,
                            const double *dyn_clip_beta, float *gm_p, float *gm_v, float *sums, float *out8, float *logits, float *value,
                            void *workspace, int64_t workspace_bytes, int N, int hid, int A, void *stream);
/* The exact Gaussian KL (ABI 61): etm_heads_loss_gaussian with old_mean [N, A] (row stride old_mean_stride >= A floats), the means of
 * the policy that drew the samples (the *_gaussian_means sampling entries), and old_log_std [A], a snapshot of its log sigma.  The
 * same launch also reduces KL(old || new) = mean_n sum_a [(expm1(2 d_a) / 2 - d_a) + ((old_mean_na - mean_na) / sigma_a)^2 / 2],
 * d_a = old_log_std_a - log_std_a (nothing cancels: equal policies give exactly 0): out8[4] = that KL, out8[6] = the k3 sample
 * estimate that etm_heads_loss_gaussian puts into out8[4].  A statistic only (unless `kl_penalty`): the loss, gm_p, gm_v, out8[0..3], out8[5] and the
 * etm_heads_loss_gaussian row are that entry's bit for bit; sums [etm_heads_loss_gaussian_kl_row_floats =
 * etm_heads_loss_gaussian_row_floats + 1] carries the raw KL sum as its last element.  Shapes: etm_heads_loss_supported_gaussian.
 * Refusals: the list above. */
int etm_heads_loss_gaussian_kl_row_floats(int hid, int A);
int64_t etm_heads_loss_gaussian_kl_workspace_bytes(int N, int hid, int A);
int etm_heads_loss_gaussian_kl(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                               const float *bb, const float *wv, const float *bv, const float *xact, int64_t action_stride,
                               const float *log_std, const float *old_logp, int64_t logp_stride, const float *adv, const float *old_value,
                               const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                               float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v, float *sums, float *out8,
                               float *logits, float *value, void *workspace, int64_t workspace_bytes, int N, int hid, int A,
                               const float *old_mean, int64_t old_mean_stride, const float *old_log_std, void *stream);
/* The KL penalty (`kl_penalty`; added with the ABI left at 61 -- no signature above changes): each entry is its *_kl twin's argument
 * list with kl_coef in front of the stream, ONE device float32 (4-byte aligned) that the kernels read in place, in eager launches and
 * captured graphs alike.  The loss is L + coef K, K = out8[4], the exact KL exactly as the twin reports it, coef = *kl_coef:
 *   categorical  d K / d logit_k = pol_scale (p_k - p_old_k) on a branch's valid columns, exactly 0 on the others
 *   Box          d K / d mean_na = ent_scale (-q_na / sigma_a), d K / d log_std_a = ent_scale sum_n (-expm1(2 d_a) - q_na^2),
 *                q_na = (old_mean_na - mean_na) / sigma_a, d_a = old_log_std_a - log_std_a
 * join d logits before the heads' backward: gm_p, gm_v and every gradient element of sums (Box: d log_std too) are those of L + coef K;
 * equal policies add exactly 0.  out8[2] = the twin's loss + coef K, out8[7] = coef (0 elsewhere); logits, value, out8[0, 1, 3, 4, 5,
 * 6], the statistic sums, the row layout and the workspace are the twin's.  No launch is added.  Refusals: the list above. */
int etm_heads_loss_kl_penalty(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                              const float *bb, const float *wv, const float *bv, const int64_t *actions, int64_t action_stride,
                              const float *old_logp, int64_t logp_stride, const float *adv, const float *old_value,
                              const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                              float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v, float *sums, float *out8,
                              float *logits, float *value, void *workspace, int64_t workspace_bytes, int N, int hid, int A,
                              const int64_t *action_mask, const float *old_logps, int64_t old_logps_stride, const float *kl_coef,
                              void *stream);
int etm_heads_loss_branched_kl_penalty(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                       const float *bb, const float *wv, const float *bv, const int64_t *actions, int64_t action_stride,
                                       const float *old_logp, int64_t logp_stride, const float *adv, const float *old_value,
                                       const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale,
                                       float ent_scale, float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v,
                                       float *sums, float *out8, float *logits, float *value, void *workspace, int64_t workspace_bytes,
                                       int N, int hid, const int32_t *branch_sizes, int n_branches, const int64_t *action_mask,
                                       const float *old_logps, int64_t old_logps_stride, const float *kl_coef, void *stream);
int etm_heads_loss_gaussian_kl_penalty(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                       const float *bb, const float *wv, const float *bv, const float *xact, int64_t action_stride,
                                       const float *log_std, const float *old_logp, int64_t logp_stride, const float *adv,
                                       const float *old_value, const float *adv_stats3, double clip, float vf_coef, float beta,
                                       float pol_scale, float ent_scale, float val_scale, const double *dyn_clip_beta, float *gm_p,
                                       float *gm_v, float *sums, float *out8, float *logits, float *value, void *workspace,
                                       int64_t workspace_bytes, int N, int hid, int A, const float *old_mean, int64_t old_mean_stride,
                                       const float *old_log_std, const float *kl_coef, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Weight gradients of the dense layers of one optimisation step as ONE grouped launch: replaces the `dW = dy^T x` products that
 * `loss.backward()` (trainer.py:310) issues one by one for transformer.py:26-29 (queries / keys / values / fc_out), :115 (fc),
 * :201 (linear_embedding) and model.py:97-107 (lin_policy, lin_value) -- contractions over the N samples of the minibatch with a
 * small [out, in] result, which only fill the chip when all layers' gradients are computed together.
 *   C[p] (Ma x Nb, row stride ldc) = A[p]^T B[p];  A[p] [N, Ma] (row stride lda) = the layer's output gradient, B[p] [N, Nb] (row
 *   stride ldb) = its input; per-head key / value folds are H problems each (the head's columns of A, the head's plane of B, the
 *   head's rows of C).  A / B / C: HOST arrays of n_problems device pointers; dims: HOST array of 5 ints per problem
 *   (Ma, Nb, lda, ldb, ldc).  Shapes: etm_grouped_dw_supported(N, Ma, Nb, lda, ldb, ldc) == 1 (Ma % 96 == 0, Nb % 128 == 0, strides
 *   multiples of 4 floats, byte offsets below 2^31); B and C 16-byte aligned; n_problems <= etm_grouped_dw_max_problems().
 *   C is overwritten; fp32 MFMA; the four k-ranges of a workgroup are summed in a fixed order (deterministic). */
int etm_grouped_dw_supported(int N, int Ma, int Nb, int lda, int ldb, int ldc);
int etm_grouped_dw_max_problems(void);
int etm_grouped_dw(const float *const *A, const float *const *B, float *const *C, const int32_t *dims, int n_problems, int N,
                   void *stream);

/* The workgroup -> tile map of both grouped launches (ABI 55): out[b] = the tile that workgroup b of a launch with n_tiles tiles
 * computes, b < n_tiles -- die b % 8 takes the contiguous run [x T / 8, (x + 1) T / 8) of the tiles (csrc/grouped_dw_tiles.h).  The
 * entry evaluates the function the kernels call (one body), on the host: no GPU call, so the map can be checked for every tile count
 * (tests/test_grouped_dw_host.py).  ETM_EINVAL for n_tiles <= 0 or out == NULL. */
int etm_grouped_dw_tile_map(int n_tiles, int32_t *out);

/* The tail launch (ABI 50; DESIGN section 4 "The ends of the step"): etm_grouped_dw with the grouped column-sum reduction that ends a
 * backward pass on extra workgroups of the SAME launch, numbered after the tile workgroups -- it runs on the CUs the tiles leave
 * idle (216 tiles on 256 CUs at config 3) instead of alone on the chip in front of it.
 *   A .. N: as etm_grouped_dw, n_problems <= etm_grouped_dw_tail_max_problems() (the job table shares the 4 KB of kernel arguments);
 *   cs_*, n_cs (1 .. 64): the arguments of etm_colsum_reduce_grouped, P / C / ld below 65536.
 * The reduction runs the device body of that entry point (csrc/tail_jobs.h: 256 threads in both launches, the same code), so every
 * output holds the bits the two separate launches give.  No workgroup reads what another writes. */
int etm_grouped_dw_tail_max_problems(void);
int etm_grouped_dw_tail(const float *const *A, const float *const *B, float *const *C, const int32_t *dims, int n_problems, int N,
                        const float *const *cs_partial, const int *cs_P, const int *cs_C, const int *cs_ld, float *const *cs_out, int n_cs,
                        void *stream);

/* ---------------------------------------------------------------------------------------------
 * Optimiser step on flat fp32 arenas, replaces `clip_grad_norm_(parameters, max_grad_norm)` + `optimizer.step()` of
 * trainer.py:311-312 (torch.optim.AdamW: betas (0.9, 0.999), eps 1e-8, weight_decay 0.01 unless the caller says otherwise).
 * p / g / m / v: parameter, gradient, exp_avg, exp_avg_sq arenas of n floats (n % 4 == 0, 16-byte aligned; padding zero).
 *   etm_grad_sqnorm: partial[i] = sum of g^2 over chunk i (n_partial <= 4096 workgroups, fixed chunking), *step += 1 (step may
 *                    be NULL).  Runs after the data-parallel all-reduce of g.
 *   etm_adamw_clip : total norm = sqrt(sum partial) -> coef = min(1, max_norm / (norm + 1e-6)) (max_norm <= 0: no clipping);
 *                    g *= coef (written back), decoupled weight decay, AdamW update with bias corrections from *step, lr read
 *                    from *lr_dev.  norm_out (optional) receives the un-clipped total norm.  grad_scale > 0: the arena holds
 *                    gradient / grad_scale (data parallel: the all-reduced SUM over `world` ranks, grad_scale = 1 / world); norm
 *                    and written-back gradient are those of arena * grad_scale (the division rides in the clip coefficient
 *                    instead of costing a pass over the arena); 1.0f leaves every bit as without it.
 * Device-resident lr / step make the pair replayable inside a captured HIP graph. */
int etm_grad_sqnorm(const float *g, int64_t n, float *partial, int n_partial, int64_t *step, void *stream);
int etm_adamw_clip(float *p, float *g, float *m, float *v, int64_t n, const float *partial, int n_partial, const float *lr_dev,
                   const int64_t *step, double beta1, double beta2, double eps, double weight_decay, float max_norm, float grad_scale, float *norm_out,
                   void *stream);

/* The same pair under a KL early stop (ABI 57): the step is dropped when an earlier step of this update was dropped, or when
 * !(*kl <= kl_limit) -- *kl is the step's own k3 estimate (out8[4] of the loss entries); a NaN stops too.  gate: three 64-bit words, 8-byte
 * aligned, zeroed by the caller at the start of every update: gate[0] stopped (0 / 1), gate[1] steps applied in this update, gate[2] the
 * bit pattern of the kl that tripped.  No launch is added: the decision rides in the two launches.
 *   etm_grad_sqnorm_gated: partial[] as etm_grad_sqnorm.  Workgroup 0, thread 0 decides (no other workgroup of the launch reads gate or
 *                    step).  Not halted: *step += 1, gate[1] += 1.  Halted for the first time: gate[0] = 1, gate[2] = bits of *kl and,
 *                    host_word not NULL, gate[1] + 1 is stored into that pinned host word (system scope, release).
 *   etm_adamw_clip_gated : every workgroup reads gate[0]; set: norm_out is written and nothing else (p, g, m, v keep every bit);
 *                    clear: the arithmetic of etm_adamw_clip (one definition in the source, a compile-time switch).
 * ETM_EINVAL: kl or gate NULL, gate or host_word not 8-byte aligned, and whatever the ungated entries refuse. */
int etm_grad_sqnorm_gated(const float *g, int64_t n, float *partial, int n_partial, int64_t *step, const float *kl, float kl_limit,
                          uint64_t *gate, uint64_t *host_word, void *stream);
int etm_adamw_clip_gated(float *p, float *g, float *m, float *v, int64_t n, const float *partial, int n_partial, const float *lr_dev,
                         const int64_t *step, double beta1, double beta2, double eps, double weight_decay, float max_norm, float grad_scale,
                         float *norm_out, const uint64_t *gate, void *stream);

/* The norm launch under a KL-adaptive learning rate (ABI 59; `adaptive_lr`, the `schedule: adaptive` / `desired_kl` of rsl_rl and
 * rl_games), with or without the KL early stop.  partial[] and *step as etm_grad_sqnorm.  Workgroup 0, thread 0 decides -- it asks for
 * *lr_dev, *kl, lr_state and the gate words before the sum, and no other workgroup of the launch reads lr_dev, lr_state, gate or step --
 * in this order:
 *   1. gate not NULL and gate[0] set (an earlier step of this update was dropped): nothing happens, no lr change, no step.
 *   2. the rule on k = *kl (the step's own k3 estimate, out8[4] of the loss entries), in fp32:
 *        k > kl_high           : *lr_dev = fmaxf(lr_min, *lr_dev / factor)   (correctly rounded division), lr_state[1] += 1
 *        k < kl_low and k > 0  : *lr_dev = fminf(lr_max, *lr_dev * factor),                                lr_state[0] += 1
 *        otherwise (a NaN, k <= 0, k at a limit): nothing.  +Inf cuts.  The clamps act on a change only: an *lr_dev outside
 *        [lr_min, lr_max] stays until the rule moves it.  lr_state counts decisions, also those a clamp left without effect.
 *   3. gate not NULL: the test of etm_grad_sqnorm_gated, !(k <= kl_limit), with its stores (gate[0], gate[2], host_word); the step that
 *      trips the stop has already cut the lr when k > kl_high.  gate NULL: kl_limit and host_word are not looked at.
 *   4. not halted: *step += 1 (and gate[1] += 1).
 * lr_state: two 64-bit words, 8-byte aligned, zeroed by the caller at the start of every update ([0] raises, [1] cuts).  The AdamW launch
 * that follows -- etm_adamw_clip with gate NULL, etm_adamw_clip_gated otherwise, both as they are -- reads the new *lr_dev: the step that
 * saw the kl is the first one taken with the new rate.  No launch is added.
 * ETM_EINVAL, nothing launched: kl, lr_dev or lr_state NULL; kl or lr_dev not 4-byte aligned; lr_state, gate or host_word not 8-byte
 * aligned; host_word without gate; rule values outside factor > 1, 0 <= kl_low < kl_high, 0 < lr_min <= lr_max, all finite; and
 * whatever etm_grad_sqnorm refuses. */
int etm_grad_sqnorm_adaptive(const float *g, int64_t n, float *partial, int n_partial, int64_t *step, const float *kl, float *lr_dev,
                             float kl_low, float kl_high, float factor, float lr_min, float lr_max,
                             uint64_t *lr_state,                       /* [0] raises, [1] cuts in this update */
                             float kl_limit, uint64_t *gate, uint64_t *host_word,   /* gate NULL: no early stop */
                             void *stream);

/* Digest of a flat fp32 arena taken as raw bits (ABI 56; checkpoints: what is written, what is read back and what two runs compare).
 * One pass over the n words b_i of x (any n >= 1, any 4-byte-aligned base; 16-byte loads on the aligned middle only) writes
 *   out4[0] = sum over i of mix(i * 0x9E3779B97F4A7C15 + b_i) mod 2^64, mix(z): z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27,
 *             z *= 0x94D049BB133111EB, z ^= z >> 31 -- depends on the position of every word and tells -0 from +0;
 *   out4[1] = the number of words whose exponent field is all ones (Inf, NaN);
 *   out4[2] = the bit pattern of the largest |x| among the finite words (0 when there is none);
 *   out4[3] = n.
 * Integer sums and one integer maximum: the result does not depend on the order of summation, so neither on n_partial.
 * partial: 3 * n_partial 64-bit words of scratch (n_partial in 1 .. 4096 workgroups); partial and out4 8-byte aligned.  Two launches
 * (per-workgroup partial words, then one workgroup adds them), no atomics, nothing allocated: graph-capturable.  ETM_EINVAL for a null
 * pointer, n <= 0, n_partial outside 1 .. 4096 or a misaligned pointer. */
int etm_arena_digest(const float *x, int64_t n, uint64_t *partial, int n_partial, uint64_t *out4, void *stream);

/* Output heads on the rollout path (model.py:108-110): h [W, 2*hid] = [relu(lin_policy) | relu(lin_value)] rows;
 * logits [W,A] = h_pol Wp^T + bp, value [W] = h_val . wv + bv.  One launch instead of two small library GEMMs. */
int etm_rollout_heads(const float *h, const float *wp, const float *bp, const float *wv, const float *bv, float *logits, float *value,
                      int W, int A, int hid, void *stream);
/* etm_rollout_heads + etm_rollout_sample of a single-branch policy in one launch.  host_actions (PINNED host memory, optional):
 * the sampled actions are also stored to host_actions[W] -- visible to the host once the launch has completed (event), which
 * saves the device-to-host copy launch of every environment step.  h_bias [2*hid] (optional): h holds the PRE-activations of the
 * hidden heads and relu(h + h_bias) is applied on the fly (the concatenated hidden-head GEMM then runs without an epilogue).  host_flag (optional, needs host_actions): after a
 * system-scope fence the new step counter (*t_dev after the increment) is stored to *host_flag, so the host can spin on
 * the flag instead of waiting for an event.  sync_counter: one device int32, zero before the first call (the workgroups of a
 * launch count themselves in; the last one advances *t_dev and resets the counter).  forced: as in etm_rollout_sample, a
 * time-major table [S, stage_W] already offset to the group's first worker.
 * REFUSALS of the six etm_rollout_policy* entries, in the order in which they win (a refused call launches nothing):
 *   categorical: a NULL mandatory action_mask (*_masked); a NULL or 4-byte-misaligned st_logps (*_logps); a NULL mandatory pointer
 *   (all but h_bias, forced, host_actions, host_flag), W, A or hid <= 0 (a bad branch table makes A = 0, as for etm_rollout_sample*),
 *   stage_W < W; host_flag without host_actions: ETM_EINVAL; an action_mask that is not 8-byte aligned: ETM_EINVAL, then one over more
 *   than 63 columns: ETM_EUNSUPPORTED.
 *   Gaussian: a NULL or misaligned st_means (*_means); a NULL mandatory pointer (as above, and not low, high), W or hid <= 0,
 *   stage_W < W; host_flag without host_actions: ETM_EINVAL; then the Box table as for etm_rollout_sample_gaussian. */
int etm_rollout_policy(const float *h, const float *h_bias, const float *wp, const float *bp, const float *wv, const float *bv,
                       const float *uniforms, const int64_t *forced, int64_t *t_dev, int64_t *actions, int64_t *st_actions,
                       float *st_logp, float *st_values, int64_t *host_actions, int64_t *host_flag, int32_t *sync_counter,
                       int W, int A, int hid, int stage_W, void *stream);
/* MultiDiscrete (ABI 48): wp / bp = the branches' heads concatenated ([sum sizes, hid], [sum sizes]); sampling per branch as in
 * etm_rollout_sample_branched; uniforms / forced / st_actions / st_logp [S, stage_W, B], actions / host_actions [W, B]. */
int etm_rollout_policy_branched(const float *h, const float *h_bias, const float *wp, const float *bp, const float *wv, const float *bv,
                                const float *uniforms, const int64_t *forced, int64_t *t_dev, int64_t *actions, int64_t *st_actions,
                                float *st_logp, float *st_values, int64_t *host_actions, int64_t *host_flag, int32_t *sync_counter,
                                int W, int hid, int stage_W, const int32_t *branch_sizes, int n_branches, void *stream);
/* Invalid-action masks (ABI 58): as etm_rollout_sample_branched_masked; action_mask [W] int64 of THIS group's workers, in device or
 * pinned host memory (each workgroup reads its worker's word in place, in front of the dot products). */
int etm_rollout_policy_branched_masked(const float *h, const float *h_bias, const float *wp, const float *bp, const float *wv,
                                       const float *bv, const float *uniforms, const int64_t *forced, int64_t *t_dev, int64_t *actions,
                                       int64_t *st_actions, float *st_logp, float *st_values, int64_t *host_actions, int64_t *host_flag,
                                       int32_t *sync_counter, int W, int hid, int stage_W, const int32_t *branch_sizes, int n_branches,
                                       const int64_t *action_mask, void *stream);
/* (added at ABI 61) with every column's log-prob staged, see etm_rollout_sample_branched_logps */
int etm_rollout_policy_branched_logps(const float *h, const float *h_bias, const float *wp, const float *bp, const float *wv,
                                      const float *bv, const float *uniforms, const int64_t *forced, int64_t *t_dev, int64_t *actions,
                                      int64_t *st_actions, float *st_logp, float *st_values, int64_t *host_actions, int64_t *host_flag,
                                      int32_t *sync_counter, int W, int hid, int stage_W, const int32_t *branch_sizes, int n_branches,
                                      const int64_t *action_mask, float *st_logps, void *stream);
/* Box policies (ABI 49): wp / bp = the mean head [A, hid], [A]; the draw of etm_rollout_sample_gaussian (normals / forced / st_actions
 * [S, stage_W, A]); actions and host_actions (pinned, optional) [W, A] receive the clipped actions, host_actions before the flag. */
int etm_rollout_policy_gaussian(const float *h, const float *h_bias, const float *wp, const float *bp, const float *wv, const float *bv,
                                const float *log_std, const float *normals, const float *forced, int64_t *t_dev, float *actions,
                                float *st_actions, float *st_logp, float *st_values, float *host_actions, int64_t *host_flag,
                                int32_t *sync_counter, const float *low, const float *high, int W, int A, int hid, int stage_W, void *stream);
/* (ABI 61) with the means staged, see etm_rollout_sample_gaussian_means */
int etm_rollout_policy_gaussian_means(const float *h, const float *h_bias, const float *wp, const float *bp, const float *wv, const float *bv,
                                      const float *log_std, const float *normals, const float *forced, int64_t *t_dev, float *actions,
                                      float *st_actions, float *st_logp, float *st_values, float *host_actions, int64_t *host_flag,
                                      int32_t *sync_counter, const float *low, const float *high, int W, int A, int hid, int stage_W,
                                      float *st_means, void *stream);

/* The transformer, the hidden / output heads and the sampling of one rollout step of a worker group as ONE launch (post-LN
 * blocks without gates; trainer.py:163-186 -> model.py:96-112 -> transformer.py:222-253), csrc/rollout_fused.hip: a TEAM of
 * P = etm_rollout_trxl_team(H) workgroups per worker (4 at H % 4 == 0) walks the whole chain as matrix-vector products, every
 * member owning D / P columns of each product and H / P heads, the members exchanging their pieces through memory (16-byte
 * packets that carry their own sequence number, bounded polling) -- instead of 6 dependent launches per block.
 *   h_in [W, D]: transformer input (model.py:96-100); wemb_t [P][D][D / P], bemb [D]: linear_embedding (transposed, member-blocked);
 *   blocks: HOST array of nb x 19 device pointers (wq_t, wo_t, bo, norm1 gain, norm1 bias, wfc_t, bfc, norm2 gain, norm2 bias; gate1:
 *           wy_t = [Wr | Wz | Wg]^T, ux_t = [Ur | Uz]^T, ug_t, bg; gate2: the same four; norm_kv gain, norm_kv bias).  Layouts: *_t =
 *           the weight TRANSPOSED ([in, out]); every matrix that is split by COLUMNS over the team (wemb_t, wq_t, wfc_t, ug_t, wh_t)
 *           is MEMBER-BLOCKED: [P][in][out / P], member m's columns m * out / P ... as one contiguous block (wo_t is
 *           split by rows and stays [D, D]); wy_t / ux_t are [P][D][j * D / P] (j = 3 / 2 maps side by side per member) if
 *           etm_rollout_trxl_gate_merged(D, H) and [P][j][D][D / P] otherwise; the
 *           gate pointers are read with gtrxl != 0 (GRU gates instead of residuals, transformer.py:255-298), the norm_kv pair by the
 *           tail of a pre-LN model (pre_ln != 0: LayerNorm in front of the sub-layers, transformer.py:128-150);   kv / strides / win / mask: the K | V cache rows as in etm_attn_cached (rows of all blocks: the
 *           kernel adds b * 2D);   items [nb, W, D]: receives every block's input = the new memory items (block-major);
 *   wh_t [P][D][2 hid / P] (member-blocked), bh [2 hid]: [lin_policy ; lin_value] transposed;  wp / bp / wv / bv and everything from `uniforms` to
 *   `sync_counter`: as in etm_rollout_policy;
 *   scratch: etm_rollout_trxl_scratch_bytes(W, D, H, nb) bytes that the caller ZEROES ONCE and then leaves to the kernel
 *           (int64 launch counter, int64 error word -- non-zero after a launch = a team member timed out --, 48 bytes of padding,
 *           then the exchange slots).
 *   window lookup inside the launch (ss non-NULL; then win / mask may be NULL and no etm_rollout_window is needed in front): ss [2, W]
 *           = (episode step, slot) of the workers (device or pinned host memory, read in place); every team looks its window rows /
 *           mask up in index_table [T, L] / mask_table [L, L] (trainer.py:165-169), member 0 also writes them to win_t / mask_t [W, L]
 *           and to row *t_dev of the staging arrays st_idx / st_mask [S, stage_W, L], latches ss into latch [2, W] and *t_dev into
 *           t_row; a worker at episode step 0 first gets its cache rows reset to kv_init [T, nb, 2D] (NULL: no reset);
 *   h_splits > 0: h_in is [h_splits, W, D] from etm_rollout_hidden_partial and the input is relu(sum over slices + h_bias [D]);
 *   tail (wkv non-NULL; NULL = none): after the action hand-over the launch also writes bank[slot_l[w], step_l[w], b, :] = item_b
 *           (bank [slots, T, nb, D] with the given slot / row strides in floats) and kv[w, step_l[w], b, :] = (item_b +
 *           pos[step_l[w]]) [Wk ; Wv]^T  (wkv [nb][P][D][2D / P]: member m's block of a block's [Wk^T | Wv^T] = its D / P columns of Wk^T
 *           followed by its D / P columns of Wv^T -- the cache columns member m reads are written by member m only; pos [T, D] or NULL;
 *           transformer.py:236-237 for the one new row) -- the memory-bank write and K | V projection of trainer.py:174.
 * Shape support: etm_rollout_trxl_supported(D, H, L, hid, A, nb) == 1 (D % (4 P) == 0, D <= 512, D / P <= 128, 2 hid / P <= 256,
 * H <= 8, L <= 128, nb <= 8, A < 64) and at most 256 workgroups (etm_rollout_trxl_grid(W, H)); ETM_EUNSUPPORTED otherwise.
 * REFUSALS of the twelve etm_rollout_trxl* / etm_rollout_trxl_group* entries, in the order in which they win (a refused call launches
 * nothing and writes nothing):
 *    1. a NULL mandatory action_mask (*_masked): ETM_EINVAL; the Box table of the Gaussian entries: A <= 0 ETM_EINVAL, A > 8
 *       ETM_EUNSUPPORTED, a low above its high ETM_EINVAL;
 *    2. a NULL or 4-byte-misaligned st_means (*_means) or st_logps (*_logps): ETM_EINVAL;
 *    3. ss without mask_table, index_table, st_mask, st_idx, latch, mask_t, win_t or with T <= 0; no ss and no win or no mask: ETM_EINVAL;
 *    4. a NULL mandatory pointer -- h_in, wemb_t, bemb, blocks, kv, items, wh_t, bh, wp, bp, wv, bv, uniforms (Gaussian: log_std,
 *       normals), actions, st_actions, t_dev, st_logp, st_values, sync_counter, scratch: ETM_EINVAL;
 *    5. W, nb, D, H, L, hid or A <= 0 (a branch table that is NULL, holds a size <= 0 or has more than 16 entries makes A = 0),
 *       stage_W < W, D % H != 0: ETM_EINVAL;
 *    6. host_flag without host_actions: ETM_EINVAL;
 *    7. an action_mask that is not 8-byte aligned: ETM_EINVAL, then one over more than 63 columns: ETM_EUNSUPPORTED;
 *    8. wkv without step_l, slot_l or bank: ETM_EINVAL;   9. h_splits < 0, > 64, or > 0 without h_bias: ETM_EINVAL;
 *   10. a shape outside the form's predicate (the worker form: or more than 256 workgroups; the group form: or a tail with
 *       etm_rollout_trxl_team(H) != H): ETM_EUNSUPPORTED;   11. scratch_bytes below the form's scratch size: ETM_EWORKSPACE;
 *   12. per block: a NULL among the first 9 pointers, with gtrxl != 0 among pointers 9 .. 16, or one of the two norm_kv pointers
 *       without the other: ETM_EINVAL. */
int etm_rollout_trxl_team(int H);
/* Workgroup placement of the step kernel (process-wide; results do not depend on it): 0 (default) = the P members of a worker's
 * team on one XCD, 1 = XCD x hosts member x % P of an 8 / P-th of the workers, so that an XCD only ever reads one member's slice of
 * every matrix.  etm_rollout_trxl_grid(W, H): workgroups of one launch
 * under the current placement -- all of them must be resident at once (<= 256 on the MI355X), else ETM_EUNSUPPORTED. */
int etm_rollout_trxl_set_placement(int mode);
int etm_rollout_trxl_grid(int W, int H);
int etm_rollout_trxl_supported(int D, int H, int L, int hid, int A, int nb);
int etm_rollout_trxl_gate_merged(int D, int H);   /* packing of the GRU-gate matrices that the kernel expects for this shape, see below */
int64_t etm_rollout_trxl_scratch_bytes(int W, int D, int H, int nb);
int etm_rollout_trxl(const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb, float *kv,
                     int64_t kv_worker_stride, int64_t kv_row_stride, const int64_t *win, const uint8_t *mask, float *items,
                     const float *wh_t, const float *bh, const float *wp, const float *bp, const float *wv, const float *bv,
                     const float *uniforms, const int64_t *forced, int64_t *t_dev, int64_t *actions, int64_t *st_actions,
                     float *st_logp, float *st_values, int64_t *host_actions, int64_t *host_flag, int32_t *sync_counter, float ln_eps,
                     void *scratch, int64_t scratch_bytes, const float *wkv, const float *pos, const int64_t *step_l,
                     const int64_t *slot_l, float *bank, int64_t bank_slot_stride, int64_t bank_row_stride, int64_t bank_block_stride,
                     const float *h_bias, int h_splits, const int64_t *ss, const uint8_t *mask_table, const int64_t *index_table, uint8_t *st_mask,
                     int64_t *st_idx, int64_t *latch, int64_t *t_row, uint8_t *mask_t, int64_t *win_t, const float *kv_init, int T,
                     int pre_ln, int gtrxl, int W, int D, int H, int L, int hid, int A, int stage_W, void *stream);
/* The group form of the step for GRU-gated blocks (round 5, csrc/rollout_group.hip; replaces the same reference lines as
 * etm_rollout_trxl: trainer.py:163-186 -> model.py:96-112 -> transformer.py:222-253 with the gates of :287-298): the W <= 8 workers of a
 * group are the ROWS of every product and its columns are dealt to 32 workgroups, so every matrix leaves L2 / the Infinity Cache once
 * per GROUP and step (the per-worker form streams 8.85 MB per worker and step at config 5).  Same arguments as etm_rollout_trxl with
 * OTHER matrix packings: every [in = D, out] map (wemb_t, wq_t, wo_t, wfc_t, ug_t) transposed and COLUMN-BLOCKED [32][D][D / 32];
 * wy_t = [32][3][D][D / 32] (Wr, Wz, Wg), ux_t = [32][2][D][D / 32] (Ur, Uz) -- EXCEPT gate 1 (the attention gate), whose wy_t
 * holds the products with fc_out folded in, (Wr Wo, Wz Wo, Wg Wo) rounded once from float64, followed by the three bias rows
 * [3][D] = (Wr bo, Wz bo, Wg bo): the kernel never multiplies by wo_t / adds bo (one product and one exchange fewer per block;
 * both pointers are still passed and ignored); wh_t = [32][NCH][D][CH], CH = 2 hid / 32 / NCH <= 16,
 * NCH = ceil(2 hid / 32 / 16); wkv [nb][H][D][2 D / H] (per head: its K columns | its V columns); scratch:
 * etm_rollout_trxl_group_scratch_bytes(nb) bytes, zeroed once.  Shapes: etm_rollout_trxl_group_supported (gtrxl != 0, W <= 8,
 * W * H <= 32, D in {128, 384}, L <= 128); the launch is etm_rollout_trxl_group_grid() = 32 workgroups that must all be resident. */
int etm_rollout_trxl_group_supported(int D, int H, int L, int hid, int A, int nb, int W, int gtrxl);
int etm_rollout_trxl_group_grid(void);
int64_t etm_rollout_trxl_group_scratch_bytes(int nb);
int etm_rollout_trxl_group(const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb, float *kv,
                     int64_t kv_worker_stride, int64_t kv_row_stride, const int64_t *win, const uint8_t *mask, float *items,
                     const float *wh_t, const float *bh, const float *wp, const float *bp, const float *wv, const float *bv,
                     const float *uniforms, const int64_t *forced, int64_t *t_dev, int64_t *actions, int64_t *st_actions,
                     float *st_logp, float *st_values, int64_t *host_actions, int64_t *host_flag, int32_t *sync_counter, float ln_eps,
                     void *scratch, int64_t scratch_bytes, const float *wkv, const float *pos, const int64_t *step_l,
                     const int64_t *slot_l, float *bank, int64_t bank_slot_stride, int64_t bank_row_stride, int64_t bank_block_stride,
                     const float *h_bias, int h_splits, const int64_t *ss, const uint8_t *mask_table, const int64_t *index_table, uint8_t *st_mask,
                     int64_t *st_idx, int64_t *latch, int64_t *t_row, uint8_t *mask_t, int64_t *win_t, const float *kv_init, int T,
                     int pre_ln, int gtrxl, int W, int D, int H, int L, int hid, int A, int stage_W, void *stream);
/* MultiDiscrete forms of the two step kernels (ABI 48): the arguments of etm_rollout_trxl / etm_rollout_trxl_group with A replaced by
 * the branch table (branch_sizes: HOST array, n_branches <= 16); wp / bp = the branches' heads concatenated; sampling per branch as in
 * etm_rollout_sample_branched (uniforms / forced / st_actions / st_logp [S, stage_W, B], actions / host_actions [W, B]).  Shapes: the
 * predicates below = the single-branch ones at A = sum sizes (per-worker kernel: sum sizes + 1 <= 64; group kernel: 8 (sum sizes + 1) + 1
 * <= 128, the floats of one exchange piece, i.e. sum sizes <= 14). */
int etm_rollout_trxl_supported_branched(int D, int H, int L, int hid, const int32_t *branch_sizes, int n_branches, int nb);
int etm_rollout_trxl_group_supported_branched(int D, int H, int L, int hid, const int32_t *branch_sizes, int n_branches, int nb, int W,
                                              int gtrxl);
int etm_rollout_trxl_branched(const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb, float *kv,
                              int64_t kv_worker_stride, int64_t kv_row_stride, const int64_t *win, const uint8_t *mask, float *items,
                              const float *wh_t, const float *bh, const float *wp, const float *bp, const float *wv, const float *bv,
                              const float *uniforms, const int64_t *forced, int64_t *t_dev, int64_t *actions, int64_t *st_actions,
                              float *st_logp, float *st_values, int64_t *host_actions, int64_t *host_flag, int32_t *sync_counter, float ln_eps,
                              void *scratch, int64_t scratch_bytes, const float *wkv, const float *pos, const int64_t *step_l,
                              const int64_t *slot_l, float *bank, int64_t bank_slot_stride, int64_t bank_row_stride, int64_t bank_block_stride,
                              const float *h_bias, int h_splits, const int64_t *ss, const uint8_t *mask_table, const int64_t *index_table,
                              uint8_t *st_mask, int64_t *st_idx, int64_t *latch, int64_t *t_row, uint8_t *mask_t, int64_t *win_t,
                              const float *kv_init, int T, int pre_ln, int gtrxl, int W, int D, int H, int L, int hid, int stage_W,
                              const int32_t *branch_sizes, int n_branches, void *stream);
int etm_rollout_trxl_group_branched(const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb, float *kv,
                                    int64_t kv_worker_stride, int64_t kv_row_stride, const int64_t *win, const uint8_t *mask, float *items,
                                    const float *wh_t, const float *bh, const float *wp, const float *bp, const float *wv, const float *bv,
                                    const float *uniforms, const int64_t *forced, int64_t *t_dev, int64_t *actions, int64_t *st_actions,
                                    float *st_logp, float *st_values, int64_t *host_actions, int64_t *host_flag, int32_t *sync_counter,
                                    float ln_eps, void *scratch, int64_t scratch_bytes, const float *wkv, const float *pos, const int64_t *step_l,
                                    const int64_t *slot_l, float *bank, int64_t bank_slot_stride, int64_t bank_row_stride,
                                    int64_t bank_block_stride, const float *h_bias, int h_splits, const int64_t *ss, const uint8_t *mask_table,
                                    const int64_t *index_table, uint8_t *st_mask, int64_t *st_idx, int64_t *latch, int64_t *t_row,
                                    uint8_t *mask_t, int64_t *win_t, const float *kv_init, int T, int pre_ln, int gtrxl, int W, int D, int H,
                                    int L, int hid, int stage_W, const int32_t *branch_sizes, int n_branches, void *stream);
/* Invalid-action masks (ABI 58): the two branched step launches with action_mask [W] int64 before the stream, the words of this
 * group's workers for this step in the layout of etm_rollout_sample_branched_masked (a Discrete policy is one branch).  Device or
 * pinned host memory: the sampling workgroup reads its words in place at the start of the launch, where the (step, slot) block is
 * read, so a read over the host link is hidden under the transformer.  Everything else as without masks; refusals: the list above. */
int etm_rollout_trxl_branched_masked(const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb, float *kv,
                              int64_t kv_worker_stride, int64_t kv_row_stride, const int64_t *win, const uint8_t *mask, float *items,
                              const float *wh_t, const float *bh, const float *wp, const float *bp, const float *wv, const float *bv,
                              const float *uniforms, const int64_t *forced, int64_t *t_dev, int64_t *actions, int64_t *st_actions,
                              float *st_logp, float *st_values, int64_t *host_actions, int64_t *host_flag, int32_t *sync_counter, float ln_eps,
                              void *scratch, int64_t scratch_bytes, const float *wkv, const float *pos, const int64_t *step_l,
                              const int64_t *slot_l, float *bank, int64_t bank_slot_stride, int64_t bank_row_stride, int64_t bank_block_stride,
                              const float *h_bias, int h_splits, const int64_t *ss, const uint8_t *mask_table, const int64_t *index_table,
                              uint8_t *st_mask, int64_t *st_idx, int64_t *latch, int64_t *t_row, uint8_t *mask_t, int64_t *win_t,
                              const float *kv_init, int T, int pre_ln, int gtrxl, int W, int D, int H, int L, int hid, int stage_W,
                              const int32_t *branch_sizes, int n_branches, const int64_t *action_mask, void *stream);
int etm_rollout_trxl_group_branched_masked(const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb, float *kv,
                                    int64_t kv_worker_stride, int64_t kv_row_stride, const int64_t *win, const uint8_t *mask, float *items,
                                    const float *wh_t, const float *bh, const float *wp, const float *bp, const float *wv, const float *bv,
                                    const float *uniforms, const int64_t *forced, int64_t *t_dev, int64_t *actions, int64_t *st_actions,
                                    float *st_logp, float *st_values, int64_t *host_actions, int64_t *host_flag, int32_t *sync_counter,
                                    float ln_eps, void *scratch, int64_t scratch_bytes, const float *wkv, const float *pos, const int64_t *step_l,
                                    const int64_t *slot_l, float *bank, int64_t bank_slot_stride, int64_t bank_row_stride,
                                    int64_t bank_block_stride, const float *h_bias, int h_splits, const int64_t *ss, const uint8_t *mask_table,
                                    const int64_t *index_table, uint8_t *st_mask, int64_t *st_idx, int64_t *latch, int64_t *t_row,
                                    uint8_t *mask_t, int64_t *win_t, const float *kv_init, int T, int pre_ln, int gtrxl, int W, int D, int H,
                                    int L, int hid, int stage_W, const int32_t *branch_sizes, int n_branches,
                                    const int64_t *action_mask, void *stream);
/* (added at ABI 61) with every column's log-prob staged, see etm_rollout_sample_branched_logps: the sampling thread stores the columns
 * as it draws (measured against storing them behind the action's hand-over, which was not faster); the shapes of the predicates above */
int etm_rollout_trxl_branched_logps(const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb, float *kv,
                                    int64_t kv_worker_stride, int64_t kv_row_stride, const int64_t *win, const uint8_t *mask, float *items,
                                    const float *wh_t, const float *bh, const float *wp, const float *bp, const float *wv, const float *bv,
                                    const float *uniforms, const int64_t *forced, int64_t *t_dev, int64_t *actions, int64_t *st_actions,
                                    float *st_logp, float *st_values, int64_t *host_actions, int64_t *host_flag, int32_t *sync_counter,
                                    float ln_eps, void *scratch, int64_t scratch_bytes, const float *wkv, const float *pos, const int64_t *step_l,
                                    const int64_t *slot_l, float *bank, int64_t bank_slot_stride, int64_t bank_row_stride,
                                    int64_t bank_block_stride, const float *h_bias, int h_splits, const int64_t *ss, const uint8_t *mask_table,
                                    const int64_t *index_table, uint8_t *st_mask, int64_t *st_idx, int64_t *latch, int64_t *t_row,
                                    uint8_t *mask_t, int64_t *win_t, const float *kv_init, int T, int pre_ln, int gtrxl, int W, int D, int H,
                                    int L, int hid, int stage_W, const int32_t *branch_sizes, int n_branches,
                                    const int64_t *action_mask, float *st_logps, void *stream);
int etm_rollout_trxl_group_branched_logps(const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb, float *kv,
                                    int64_t kv_worker_stride, int64_t kv_row_stride, const int64_t *win, const uint8_t *mask, float *items,
                                    const float *wh_t, const float *bh, const float *wp, const float *bp, const float *wv, const float *bv,
                                    const float *uniforms, const int64_t *forced, int64_t *t_dev, int64_t *actions, int64_t *st_actions,
                                    float *st_logp, float *st_values, int64_t *host_actions, int64_t *host_flag, int32_t *sync_counter,
                                    float ln_eps, void *scratch, int64_t scratch_bytes, const float *wkv, const float *pos, const int64_t *step_l,
                                    const int64_t *slot_l, float *bank, int64_t bank_slot_stride, int64_t bank_row_stride,
                                    int64_t bank_block_stride, const float *h_bias, int h_splits, const int64_t *ss, const uint8_t *mask_table,
                                    const int64_t *index_table, uint8_t *st_mask, int64_t *st_idx, int64_t *latch, int64_t *t_row,
                                    uint8_t *mask_t, int64_t *win_t, const float *kv_init, int T, int pre_ln, int gtrxl, int W, int D, int H,
                                    int L, int hid, int stage_W, const int32_t *branch_sizes, int n_branches,
                                    const int64_t *action_mask, float *st_logps, void *stream);
/* Box forms of the two step kernels (ABI 49): the arguments of etm_rollout_trxl / etm_rollout_trxl_group with log_std [A] after bv,
 * float normals / forced / actions / st_actions / host_actions in place of uniforms / forced / actions / st_actions / host_actions (the
 * layouts of etm_rollout_policy_gaussian) and the HOST bound arrays low / high after stage_W; wp / bp = the mean head.  Shapes: the
 * predicates below = the Discrete ones at A, and A <= 8. */
int etm_rollout_trxl_supported_gaussian(int D, int H, int L, int hid, int A, int nb);
int etm_rollout_trxl_group_supported_gaussian(int D, int H, int L, int hid, int A, int nb, int W, int gtrxl);
int etm_rollout_trxl_gaussian(const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb, float *kv,
                              int64_t kv_worker_stride, int64_t kv_row_stride, const int64_t *win, const uint8_t *mask, float *items,
                              const float *wh_t, const float *bh, const float *wp, const float *bp, const float *wv, const float *bv,
                              const float *log_std, const float *normals, const float *forced, int64_t *t_dev, float *actions,
                              float *st_actions, float *st_logp, float *st_values, float *host_actions, int64_t *host_flag,
                              int32_t *sync_counter, float ln_eps, void *scratch, int64_t scratch_bytes, const float *wkv, const float *pos,
                              const int64_t *step_l, const int64_t *slot_l, float *bank, int64_t bank_slot_stride, int64_t bank_row_stride,
                              int64_t bank_block_stride, const float *h_bias, int h_splits, const int64_t *ss, const uint8_t *mask_table,
                              const int64_t *index_table, uint8_t *st_mask, int64_t *st_idx, int64_t *latch, int64_t *t_row,
                              uint8_t *mask_t, int64_t *win_t, const float *kv_init, int T, int pre_ln, int gtrxl, int W, int D, int H,
                              int L, int hid, int A, int stage_W, const float *low, const float *high, void *stream);
int etm_rollout_trxl_group_gaussian(const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb,
                                    float *kv, int64_t kv_worker_stride, int64_t kv_row_stride, const int64_t *win, const uint8_t *mask,
                                    float *items, const float *wh_t, const float *bh, const float *wp, const float *bp, const float *wv,
                                    const float *bv, const float *log_std, const float *normals, const float *forced, int64_t *t_dev,
                                    float *actions, float *st_actions, float *st_logp, float *st_values, float *host_actions,
                                    int64_t *host_flag, int32_t *sync_counter, float ln_eps, void *scratch, int64_t scratch_bytes,
                                    const float *wkv, const float *pos, const int64_t *step_l, const int64_t *slot_l, float *bank,
                                    int64_t bank_slot_stride, int64_t bank_row_stride, int64_t bank_block_stride, const float *h_bias,
                                    int h_splits, const int64_t *ss, const uint8_t *mask_table, const int64_t *index_table,
                                    uint8_t *st_mask, int64_t *st_idx, int64_t *latch, int64_t *t_row, uint8_t *mask_t, int64_t *win_t,
                                    const float *kv_init, int T, int pre_ln, int gtrxl, int W, int D, int H, int L, int hid, int A,
                                    int stage_W, const float *low, const float *high, void *stream);
/* (ABI 61) with the means staged, see etm_rollout_sample_gaussian_means; the shapes of the predicates above */
int etm_rollout_trxl_gaussian_means(const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb,
                                    float *kv, int64_t kv_worker_stride, int64_t kv_row_stride, const int64_t *win, const uint8_t *mask,
                                    float *items, const float *wh_t, const float *bh, const float *wp, const float *bp, const float *wv,
                                    const float *bv, const float *log_std, const float *normals, const float *forced, int64_t *t_dev,
                                    float *actions, float *st_actions, float *st_logp, float *st_values, float *host_actions,
                                    int64_t *host_flag, int32_t *sync_counter, float ln_eps, void *scratch, int64_t scratch_bytes,
                                    const float *wkv, const float *pos, const int64_t *step_l, const int64_t *slot_l, float *bank,
                                    int64_t bank_slot_stride, int64_t bank_row_stride, int64_t bank_block_stride, const float *h_bias,
                                    int h_splits, const int64_t *ss, const uint8_t *mask_table, const int64_t *index_table,
                                    uint8_t *st_mask, int64_t *st_idx, int64_t *latch, int64_t *t_row, uint8_t *mask_t, int64_t *win_t,
                                    const float *kv_init, int T, int pre_ln, int gtrxl, int W, int D, int H, int L, int hid, int A,
                                    int stage_W, const float *low, const float *high, float *st_means, void *stream);
int etm_rollout_trxl_group_gaussian_means(const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb,
                                    float *kv, int64_t kv_worker_stride, int64_t kv_row_stride, const int64_t *win, const uint8_t *mask,
                                    float *items, const float *wh_t, const float *bh, const float *wp, const float *bp, const float *wv,
                                    const float *bv, const float *log_std, const float *normals, const float *forced, int64_t *t_dev,
                                    float *actions, float *st_actions, float *st_logp, float *st_values, float *host_actions,
                                    int64_t *host_flag, int32_t *sync_counter, float ln_eps, void *scratch, int64_t scratch_bytes,
                                    const float *wkv, const float *pos, const int64_t *step_l, const int64_t *slot_l, float *bank,
                                    int64_t bank_slot_stride, int64_t bank_row_stride, int64_t bank_block_stride, const float *h_bias,
                                    int h_splits, const int64_t *ss, const uint8_t *mask_table, const int64_t *index_table,
                                    uint8_t *st_mask, int64_t *st_idx, int64_t *latch, int64_t *t_row, uint8_t *mask_t, int64_t *win_t,
                                    const float *kv_init, int T, int pre_ln, int gtrxl, int W, int D, int H, int L, int hid, int A,
                                    int stage_W, const float *low, const float *high, float *st_means, void *stream);
/* Window pass (etm_window_*): 0 = load and multiply the window rows of fully masked waves too (A/B diagnostics; the results are
 * bit-identical either way); default 1 = skip them.  Process-wide, read at launch. */
int etm_window_set_skip_masked(int on);

/* lin_hidden of a rollout step (model.py:94-100) as K-slice partial sums: part [splits, W, D], splits =
 * etm_rollout_hidden_splits(F) (<= 16), = the slice sums of x [W, F] @ wt [F, D] (wt = the weight TRANSPOSED, 16-byte aligned,
 * D % 32 == 0).  etm_rollout_trxl(h_in = part, h_bias = the layer's bias, h_splits = splits) adds the slices in slice order,
 * the bias and the ReLU: one memory round trip on 12 x splits workgroups instead of a 49-step K walk on 24. */
int etm_rollout_hidden_splits(int F);
int etm_rollout_hidden_partial(const float *x, const float *wt, float *part, int W, int F, int D, void *stream);
/* Rollout only: the last encoder layer (model.py:92, Conv2d(64, 64, 3, 1) + ReLU) and lin_hidden's partial sums (model.py:94-97) as
 * ONE launch: one workgroup per output pixel finishes the pixel's 64 channels for every image and multiplies them with the pixel's
 * 64 rows of lin_hidden^T.  x2 [W, Hi, Wi, 64] NHWC (output of the second etm_conv_relu), w3k [(ky, kx, c), co] = [576, 64],
 * hid_t [64 * Ho * Wo, D] (feature = co * Ho * Wo + pixel), part [Ho * Wo, W, D] -- the consumer (etm_rollout_trxl with
 * h_splits = Ho * Wo <= 64) adds the slices, the bias and the ReLU.  etm_rollout_conv3_hidden_supported: 1 for this geometry. */
int etm_rollout_conv3_hidden_supported(int C, int Hi, int Wi, int Cout, int KH, int KW, int S, int D);
int etm_rollout_conv3_hidden(const float *x2, const float *w3k, const float *b3, const float *hid_t, float *part, int W, int Hi, int Wi,
                             int D, void *stream);

/* Backward of y = relu(x W^T + b) (model.py:94-107, transformer.py:232) up to its two GEMMs, in two launches: gm [N, C] =
 * g * (y > 0) and db [C] = column sums of gm (fixed summation order).  y NULL: plain linear layer (gm = g; gm may be NULL, only
 * db is produced).  workspace: etm_relu_bwd_colsum_workspace_bytes(N, C).  db NULL: the reduction is left to
 * etm_colsum_reduce_grouped (etm_relu_bwd_colsum_partial_rows(N) rows of C partial sums in `workspace`). */
int64_t etm_relu_bwd_colsum_workspace_bytes(int N, int C);
int etm_relu_bwd_colsum_partial_rows(int N);
int etm_relu_bwd_colsum(const float *g, const float *y, float *gm, float *db, float *workspace, int64_t workspace_bytes, int N, int C,
                        void *stream);

/* previous_step_input (csrc/prev_input.hip; added without a change to any signature above, the ABI version stays): the previous
 * step's action(s) and raw reward as an addend of lin_hidden's pre-activation, from a learned table T [R, D] -- branch b owns rows
 * off_b .. off_b + sizes[b] - 1, the reward row (rewards non-NULL) is row R - 1; sum(sizes) + (rewards ? 1 : 0) <= R <= 64.
 * utils.previous_step_rows / previous_step_table_grad are the host definitions.
 *   etm_prev_input_supported: 1 for 1 <= R <= 64 and 1 <= D <= 65536, else 0.
 *   etm_prev_input_rows: out[n, :] (row stride out_stride >= D floats) = sum_b T[off_b + actions[n, b], :] + rewards[n] T[R - 1, :]
 *       (+ bias [D] when not NULL), started at +0, branches in ascending b, the reward term last, every product and sum rounded on
 *       its own; +0 (+ bias) for a sample without a previous step.  actions [N, n_branches] int64 with row stride act_stride (in
 *       elements; NULL with n_branches == 0: no action rows are fed back, rewards is then required).  Which samples have a previous
 *       step: ep_step non-NULL (rollout form; [N] int64, device or pinned host memory, read in place -- row 0 of the step kernels'
 *       (episode step, slot) block): those whose word is not 0; ep_step NULL (training form): those with actions[n, 0] >= 0 (all,
 *       with n_branches == 0).  One launch; bit for bit the host rule in float32.
 *   etm_prev_input_grad: d_table [R, D] = sum_n c_n^T gm[n, :] (gm row stride gm_stride >= D), c_n the coefficients of sample n in
 *       the rule above (training form).  No float atomics: workgroups own chunks of etm_prev_input_grad_chunk() samples, added in
 *       ascending order, and the chunks' partial tables are added in chunk order by a second launch (none for a single chunk).
 *       Rows no sample touched are exactly 0; two calls give the same bits.  workspace: etm_prev_input_grad_workspace_bytes(N, R, D)
 *       bytes, always required.  d_table NULL: the second launch is left out -- `workspace` then holds
 *       etm_prev_input_grad_partial_rows(N) rows of R D partial sums for etm_colsum_reduce_grouped.
 * Valid input only: an action outside its branch (>= sizes[b], or negative in a sample that has a previous step -- in the training
 * form only column 0 decides that) is the caller's error; it is clamped into the branch's rows so that nothing outside the table is
 * read or written, where the host rule raises.  The bit-for-bit statement holds on what the host rule accepts.
 * Profiling (etm_profile_*): the rows kernel is booked under the gather_rows slot, the gradient kernel and its reduction under the
 * colsum slot -- the slot table lives in a source file this addition leaves untouched; with the key on, those two rows of the
 * per-kernel profile include these launches.
 * ETM_EINVAL, with nothing launched: a NULL or misaligned pointer, a stride below n_branches / D, R outside 1 .. 64, sizes that do not
 * fit R, N <= 0; ETM_EWORKSPACE: a workspace below the stated size. */
int etm_prev_input_supported(int R, int D);
int etm_prev_input_rows(const float *table, int R, int D, const int64_t *actions, int64_t act_stride, const int32_t *sizes, int n_branches,
                        const float *rewards, const int64_t *ep_step, const float *bias, float *out, int64_t out_stride, int64_t N,
                        void *stream);
int etm_prev_input_grad_chunk(void);
int etm_prev_input_grad_partial_rows(int64_t N);
int64_t etm_prev_input_grad_workspace_bytes(int64_t N, int R, int D);
int etm_prev_input_grad(const float *gm, int64_t gm_stride, const int64_t *actions, int64_t act_stride, const int32_t *sizes, int n_branches,
                        const float *rewards, float *d_table, int R, int D, int64_t N, float *workspace, int64_t workspace_bytes,
                        void *stream);

/* ---------------------------------------------------------------------------------------------
 * obs_reconstruction (csrc/obs_recon.hip; absent upstream's model.py, the auxiliary loss of its author's Memory Gym runs): the
 * decoder's last layer z = ConvTranspose2d(32, C, 8, 4)(a2) + bias fused with the sigmoid cross-entropy against the observation.
 * a2 NHWC [N, Hi, Wi, 32]; w [32, C, 8, 8] and bias [C] in the parameters' own layouts; Ho = 4 (Hi - 1) + 8, Wo likewise; 1 <= C <= 4.
 * utils.transposed_conv_last / utils.obs_reconstruction_loss are the host definitions.
 *   etm_obs_recon_supported: 1 for 1 <= C <= 4 and 1 <= Hi, Wi <= 4096, else 0.
 *   etm_obs_recon_fwd_loss: the target is taken as the first encoder layer takes its input: x NHWC [N or x_images, Ho, Wo, C], float32
 *       (x_is_u8 == 0) or bytes (byte k = float(k) / 255.f correctly rounded), x_index (device int64 [N] or NULL): image n is image
 *       x_index[n] of x, which then holds x_images images.  z[n, Y, X, c] sums a2[n, iy, ix, ci] w[ci][c][Y - 4 iy][X - 4 ix] over the
 *       at most 2 x 2 input pixels with 0 <= Y - 4 iy < 8, 0 <= X - 4 ix < 8 and the 32 channels, in ascending (iy, ix, ci), bias last.
 *       Per element l = max(z, 0) - z t + log1p(exp(-|z|)); sigma(z) is formed from exp(-|z|).  Written:
 *         dz [N, Ho, Wo, C] = ((sigma(z) - t) / (N Ho Wo C)) * *coef   (float32, the layout of an NHWC image; the difference, the
 *                             quotient and the product in double, rounded once; coef: one device float read in place --
 *                             doubling it doubles dz bit for bit, 0 gives zeros)
 *         out [4]: out[0] = mean of l (NOT scaled by coef), out[1] = *coef, out[2] = out[1] * out[0] (the term of the training
 *                             loss), out[3] = 0;  db [C] = the sums of dz over (n, Y, X).
 *       z is never stored; it is accumulated in double.  Three launches: a copy of w as doubles into the workspace, the pass, and the
 *       sum of the pass's per-workgroup partial sums (doubles, in `workspace`, at least
 *       etm_obs_recon_workspace_bytes(N, C, Hi, Wi) bytes, 8-byte aligned) in a fixed order.  No float atomics: two calls give the
 *       same bits.
 *   etm_obs_recon_dgrad: da2[n, iy, ix, ci] = (a2 > 0) sum_{ky, kx, c} dz[n, 4 iy + ky, 4 ix + kx, c] w[ci][c][ky][kx] -- the first
 *       encoder layer's forward on the gradient image without bias, masked by the ReLU pattern of a2.  One launch.
 *   The weight gradient needs no entry of its own: dW[ci][c][ky][kx] = sum a2[n, iy, ix, ci] dz[n, 4 iy + ky, 4 ix + kx, c] is the
 *       first encoder layer's weight gradient with the roles exchanged -- etm_conv_train_wgrad(x := dz, x_index NULL, dy := a2, ...,
 *       N, C, H = Ho, W = Wo, Cout = 32, KH = KW = 8, S = 4) returns it as [32, C, 8, 8], the decoder parameter's layout.  The 32
 *       trailing floats (that entry's "bias gradient") are the column sums of a2: discard them, db comes from etm_obs_recon_fwd_loss.
 * ETM_EINVAL, with nothing launched: a NULL pointer (x_index may be NULL), a NULL coef, a misaligned pointer (a2, dz, da2 and a float
 * x: 16 bytes; a byte x: 4; workspace and x_index: 8; the others: 4), N < 1, C outside 1 .. 4, an x_index with x_images < 1.
 * ETM_EUNSUPPORTED: Hi / Wi outside etm_obs_recon_supported; ETM_EWORKSPACE: a workspace below the stated size.
 * Profiling (etm_profile_*): booked under the conv_train_fwd / colsum / conv_train_dgrad slots. */
int etm_obs_recon_supported(int C, int Hi, int Wi);
int64_t etm_obs_recon_workspace_bytes(int64_t N, int C, int Hi, int Wi);
int etm_obs_recon_fwd_loss(const float *a2, const float *w, const float *bias, const void *x, int x_is_u8, const int64_t *x_index,
                           int64_t x_images, const float *coef, float *dz, float *out, float *db, void *workspace, int64_t workspace_bytes,
                           int64_t N, int C, int Hi, int Wi, void *stream);
int etm_obs_recon_dgrad(const float *dz, const float *w, const float *a2, float *da2, int64_t N, int C, int Hi, int Wi, void *stream);

/* Device-resident environments (csrc/device_env.hip; added with the ABI left at 61 -- no signature above changes): CueRoom, the image
 * memory task whose one host definition is environments/cue_room_env.py, stepped, auto-reset and rendered by ONE launch per call, one
 * workgroup per environment.  G x G cells (G odd) of P x P pixels (P % 4 == 0); a frame is [3, G P, G P] bytes, CHW.
 *   etm_cue_room_supported: 1 for odd 3 <= G <= 31 and P % 4 == 0, 4 <= P <= 64, else 0.
 *   etm_cue_room_state_bytes: bytes of device memory the caller owns for W environments (32 each; 0 for W < 1), 8-byte aligned.
 *   etm_cue_room_reset: every environment w < W starts episode 0 of the stream stream0 + w (stream0 = seed + first worker id, taken
 *       mod 2^64) and writes the outputs below with rewards, flags, returns and lengths zero.
 *   etm_cue_room_step: environment w reads actions[w * act_stride] (the int64 rows the sampling kernels write; a value outside 0 .. 3
 *       is clamped -- the host rule raises), advances its state exactly once, decides reward, done, truncated and success, starts the
 *       next episode where done, then renders the NEW state.  Bit for bit the host rule on valid actions.
 * Outputs (every pointer may be pinned host memory): frames -- environment w's frame at frames + w * frame_pitch bytes, written
 * with 4-byte stores, nothing outside [w * frame_pitch, w * frame_pitch + 3 G P G P) is touched; rewards [W] float32 (1.0 for the
 * target, else 0.0); flags [W] bytes (bit 0 done, bit 1 truncated, bit 2 success); returns [W] float32 and lengths [W] int32 of the
 * episode that ended (0 where none did); masks [W] int64 of the frame written (bit a set when move a stays on the grid).
 * done_word (optional, 8-byte aligned, host-visible): receives done_value after every result, by a one-thread launch behind the step
 * on the same stream (one system-scope fence, then a system-scope release store: the sampling kernels' hand-over).
 * Integer arithmetic only, no atomics: two calls from equal state give equal bytes.
 * ETM_EINVAL, with nothing launched: a NULL pointer (done_word may be NULL), a misaligned pointer (state, actions, masks, done_word:
 * 8 bytes; frames, rewards, returns, lengths: 4), W < 1, act_stride < 1, frame_pitch below 3 G P G P or no multiple of 4, cue_steps
 * or max_steps < 1, (G, P) outside etm_cue_room_supported. */
int etm_cue_room_supported(int G, int P);
int64_t etm_cue_room_state_bytes(int W);
int etm_cue_room_reset(void *state, uint8_t *frames, int64_t frame_pitch, float *rewards, uint8_t *flags, float *returns, int32_t *lengths,
                       int64_t *masks, int64_t *done_word, int64_t done_value, int W, int G, int P, int cue_steps, int max_steps,
                       int64_t stream0, void *stream);
int etm_cue_room_step(void *state, const int64_t *actions, int64_t act_stride, uint8_t *frames, int64_t frame_pitch, float *rewards,
                      uint8_t *flags, float *returns, int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W,
                      int G, int P, int cue_steps, int max_steps, int64_t stream0, void *stream);

/* CommandRoom (same file, added with the ABI left at 61): the command-sequence memory task whose one host definition is
 * environments/command_room_env.py -- K commands (up, right, down, left, stay) are shown one after the other, show_steps observations
 * each with gap_steps floor-only observations between, then executed from memory, one per step.  Same launch shape, outputs, order of
 * outputs, completion word and alignment rules as etm_cue_room_*; the state is 32 bytes per environment (episode u64, packed commands
 * u64 with 3 bits each, row, col, observation index t, commands completed n).
 *   etm_command_room_supported: 1 where etm_cue_room_supported(G, P) and 1 <= K <= 16, else 0.
 *   etm_command_room_step: actions outside 0 .. 4 are clamped (the host rule raises).  rewards: 0.1f for the correct command in the
 *       execute phase, else 0; flags: bit 0 done, bit 2 success (all K commands executed), bit 1 never set (no time limit); returns:
 *       float(n) * 0.1f of the episode that ended, one multiply; lengths: its steps; masks: all five bits while commands are shown,
 *       else bit a set when move a stays on the grid and bit 4 (stay).
 * Integer arithmetic apart from the reward constant and that multiply, no atomics: two calls from equal state give equal bytes.
 * ETM_EINVAL, with nothing launched: the classes of etm_cue_room_*, (G, P, K) outside etm_command_room_supported, show_steps < 1,
 * gap_steps < 0. */
int etm_command_room_supported(int G, int P, int K);
int64_t etm_command_room_state_bytes(int W);
int etm_command_room_reset(void *state, uint8_t *frames, int64_t frame_pitch, float *rewards, uint8_t *flags, float *returns,
                           int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W, int G, int P, int K,
                           int show_steps, int gap_steps, int64_t stream0, void *stream);
int etm_command_room_step(void *state, const int64_t *actions, int64_t act_stride, uint8_t *frames, int64_t frame_pitch, float *rewards,
                          uint8_t *flags, float *returns, int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W,
                          int G, int P, int K, int show_steps, int gap_steps, int64_t stream0, void *stream);

/* PathRoom (same file, added with the ABI left at 61): the hidden-path memory task whose one host definition is
 * environments/path_room_env.py -- an invisible path of at most M moves (up, right, down) leads from an origin in column 0 to a goal;
 * a move onto a path cell pays the progress beyond the best index reached, a move onto any other cell is a fall back to the origin.
 * Same launch shape, outputs, order of outputs, completion word and alignment rules as etm_cue_room_*; the state is 32 bytes per
 * environment (episode u64, packed moves u64 with 2 bits each, agent cell, observation index t, best index, and one word that packs
 * the origin row, the number of moves n, the goal cell and the mark cell + 1; a cell is row << 5 | column there).
 *   etm_path_room_supported: 1 where etm_cue_room_supported(G, P) and 1 <= M <= 32, else 0.
 *   etm_path_room_step: actions outside 0 .. 3 are clamped (the host rule raises).  rewards: float(k) * 0.1f, one multiply, k the
 *       tenths earned (progress, plus 10 on the goal); flags: bit 0 done, bit 1 truncated (t + 1 >= max_steps without the goal), bit 2
 *       success; returns: float(best + 10 success) * 0.1f of the episode that ended, one multiply; lengths: its steps; masks: bit a
 *       set when move a stays on the grid.
 * Integer arithmetic apart from those two multiplies, no atomics: two calls from equal state give equal bytes.
 * ETM_EINVAL, with nothing launched: the classes of etm_cue_room_*, (G, P, M) outside etm_path_room_supported, max_steps < 1. */
int etm_path_room_supported(int G, int P, int M);
int64_t etm_path_room_state_bytes(int W);
int etm_path_room_reset(void *state, uint8_t *frames, int64_t frame_pitch, float *rewards, uint8_t *flags, float *returns, int32_t *lengths,
                        int64_t *masks, int64_t *done_word, int64_t done_value, int W, int G, int P, int M, int max_steps,
                        int64_t stream0, void *stream);
int etm_path_room_step(void *state, const int64_t *actions, int64_t act_stride, uint8_t *frames, int64_t frame_pitch, float *rewards,
                       uint8_t *flags, float *returns, int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W,
                       int G, int P, int M, int max_steps, int64_t stream0, void *stream);

/* SpotRoom (same file, added with the ABI left at 61): the dark-room task with moving spotlights whose one host definition is
 * environments/spot_room_env.py -- the agent takes a coin, then leaves through an exit; from observation light_steps on the room is
 * dark, N spotlights sweep a lane each as a triangle wave (one cell every spot_period observations) and light the 3 x 3 block around
 * their centre; the agent is drawn only where a spotlight is on it, and every such observation costs one of its `health` points.
 * Same launch shape, outputs, order of outputs, completion word and alignment rules as etm_cue_room_*; the state is 32 bytes per
 * environment (episode u64, the spotlights u64 with 12 bits each -- axis 1, lane 5, phase 6 --, agent cell, observation index t, one
 * word that packs the coin cell, the exit cell, the health lost, coin-taken and the wave's common offset, and the observations the
 * spotlights have rested; a cell is row << 5 | column there).
 *   etm_spot_room_supported: 1 where etm_cue_room_supported(G, P), 0 <= N <= 4 and 1 <= H <= 15, else 0.
 *   etm_spot_room_step: actions outside 0 .. 4 are clamped (the host rule raises).  rewards: float(k) * 0.1f, one multiply, k the
 *       signed tenths earned (+5 the coin, +10 the exit with the coin, -1 a lit observation); flags: bit 0 done, bit 1 truncated
 *       (t + 1 >= max_steps, neither left nor dead), bit 2 success; returns: float(5 coin + 10 success - health lost) * 0.1f of the
 *       episode that ended, one multiply; lengths: its steps; masks: bit a < 4 set when move a stays on the grid, bit 4 (stay) set.
 * Integer arithmetic apart from those two multiplies, no atomics: two calls from equal state give equal bytes.
 * ETM_EINVAL, with nothing launched: the classes of etm_cue_room_*, (G, P, N, health) outside etm_spot_room_supported, light_steps < 1,
 * spot_period < 1, max_steps < 1. */
int etm_spot_room_supported(int G, int P, int N, int H);
int64_t etm_spot_room_state_bytes(int W);
int etm_spot_room_reset(void *state, uint8_t *frames, int64_t frame_pitch, float *rewards, uint8_t *flags, float *returns, int32_t *lengths,
                        int64_t *masks, int64_t *done_word, int64_t done_value, int W, int G, int P, int N, int light_steps,
                        int spot_period, int health, int max_steps, int64_t stream0, void *stream);
int etm_spot_room_step(void *state, const int64_t *actions, int64_t act_stride, uint8_t *frames, int64_t frame_pitch, float *rewards,
                       uint8_t *flags, float *returns, int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W,
                       int G, int P, int N, int light_steps, int spot_period, int health, int max_steps, int64_t stream0, void *stream);

/* Attention statistics (csrc/attn_stats.hip; added with the ABI left at 61 -- no signature above changes): where the attention
 * probabilities att [N, H, L] of a training pass (the tensor every training attention kernel writes, contiguous) land in the memory
 * window, per head, ADDED to table [H, ETM_ATTN_STATS_WORDS] doubles.  mask [N, L] bytes, non-zero = valid (WindowSpec.mask); v = the
 * number of valid entries of mask[n].  A row (n, h) counts when the mask is a prefix (entries 0 .. v - 1 set, no others) and
 * v >= 1; v = 0 is an empty row (its att is the uniform 1 / L a fully masked softmax leaves), any other mask an irregular row: both
 * are counted as such and add nothing else.  The age of entry l is v - l: the newest stored step has age 1.  Words of a head:
 *   0 counted rows; 1 counted rows with v >= 2; 2 empty rows; 3 irregular rows;
 *   4 sum over counted rows of the entropy -sum_l p ln p (valid entries with p > 0, nats; fp32 logf, products and row sum);
 *   5 sum over rows with v >= 2 of entropy / ln v; 6 sum over counted rows of max_l p over valid entries; 7 reserved (unchanged);
 *   8 .. 135 age[a - 1] = sum over counted rows of p at age a; 136 .. 263 index[l] = the same at window entry l (words beyond L
 *   receive + 0).  Sums across rows are double.
 * Two launches on `stream` (per-workgroup partials in the workspace, then one thread per word adds the partials in index order to
 * table), no atomics, nothing allocated: graph-capturable; the partial layout is a function of (N, H, L) alone, two calls on equal
 * inputs give equal bits, and words of table outside the H heads are not touched.  Nothing is booked in the per-kernel profile.
 *   etm_attn_stats_workspace_bytes: bytes of workspace a call needs (0 for arguments the call refuses).
 * ETM_EINVAL, with nothing launched: a NULL att, mask, table or workspace; N < 1; H outside 1 .. 32; L outside 1 .. 128; table or
 * workspace not 8-byte aligned; workspace_bytes below etm_attn_stats_workspace_bytes(N, H, L). */
#define ETM_ATTN_STATS_WORDS 264
int64_t etm_attn_stats_workspace_bytes(int N, int H, int L);
int etm_attn_stats(const float *att, const uint8_t *mask, double *table, void *workspace, int64_t workspace_bytes, int N, int H, int L,
                   void *stream);

/* Monitored gradient norms of the module groups (model.py:128-151) from the flat gradient arena in two launches:
 * out[g] = sqrt(sum_s member[g][s] * ||flat[seg_start[s] .. seg_start[s] + seg_len[s])||^2).  Segments: runs of <= 4096 floats, each
 * inside one parameter tensor (device arrays seg_start int64 [n_segs], seg_len int32 [n_segs]); member [n_groups, n_segs] float
 * (how often the group lists the segment's tensor); partial: n_segs floats of scratch. */
int etm_group_norms(const float *flat, const int64_t *seg_start, const int32_t *seg_len, int n_segs, const float *member, int n_groups,
                    float *partial, float *out, void *stream);

/* Minibatch gather of the per-sample fields in one launch (buffer.py:84-91 `samples_flat[key][mini_batch_indices]`):
 * dst[f][i, :] = src[f][idx[i], :] for f < n_fields (<= 16) and i < n.  src / dst / row_bytes: HOST arrays of n_fields device
 * pointers / byte counts; rows are contiguous, row_bytes % 4 == 0; every src[f] has src_rows rows.  Bit-exact data movement. */
int etm_gather_rows(const void *const *src, void *const *dst, const int64_t *row_bytes, int n_fields, const int64_t *idx, int64_t n,
                    int64_t src_rows, void *stream);

/* The two ends of the captured optimisation step (ABI 50; DESIGN section 4 "The ends of the step"): a replayed graph walks through the
 * minibatches of an update by itself, under a device-resident step counter, with no copy in front of or behind a replay.
 *
 * etm_step_head: the jobs at the front of the step that depend only on the minibatch indices, in ONE launch, a workgroup range per
 * job.  idx = row (*counter % table_rows) of idx_table [table_rows, n] int64 (the index vectors of a whole epoch; counter NULL: row 0).
 *   - etm_gather_rows(src, dst, row_bytes, n_fields, idx, n, src_rows) (same arguments, same limits; n_fields may be 0);
 *   - idx_out [n] (may be NULL) = idx: the fixed-address index vector that later kernels of the step read;
 *   - stats3 (may be NULL, then adv_src too) = etm_adv_stats of the vector adv_src[idx[i]], i < n (adv_src: src_rows floats), bit for
 *     bit: the same workgroup, the same order.  n >= ETM_ADV_STATS_SPLIT_MIN with stats3: ETM_EUNSUPPORTED.
 * No job reads what another writes.  Out-of-range indices are clamped as etm_gather_rows clamps them. */
int etm_step_head(const void *const *src, void *const *dst, const int64_t *row_bytes, int n_fields, const int64_t *idx_table, int table_rows,
                  const int64_t *counter, int64_t n, int64_t src_rows, int64_t *idx_out, const float *adv_src, float *stats3, void *stream);

/* etm_group_norms (same arguments, same bits in `out`) that also ends the minibatch step: with r = *counter,
 * stats_table [table_rows, n_stats] row r = stats [n_stats], norm_table [table_rows, n_groups] row r = out, *counter = r + 1.  The
 * counter is advanced with a plain store by the one workgroup of the first launch that reads it; the second launch files its row
 * under *counter - 1.  r outside the table: its nearest row.  The host resets the counter at the start of an update and reads the
 * tables after its last step.  etm_step_end: the statistics row and the counter alone (steps without the norm monitor). */
int etm_group_norms_step(const float *flat, const int64_t *seg_start, const int32_t *seg_len, int n_segs, const float *member, int n_groups,
                         float *partial, float *out, float *norm_table, const float *stats, int n_stats, float *stats_table, int table_rows,
                         int64_t *counter, void *stream);
int etm_step_end(const float *stats, int n_stats, float *stats_table, int table_rows, int64_t *counter, void *stream);

/* Host-side helper of the in-process environment front-ends (no device work): a memcpy split over `threads` threads (the
 * caller + threads - 1 helpers that spin briefly after a job and sleep otherwise).  The reference produces the observations of a
 * step in n_workers processes at once (worker.py:5-45); here one process writes a worker group's rows into the pinned staging
 * buffer, and a single core's memcpy was the largest host item of a rollout step.  csrc/host_copy.hip.
 *   etm_host_copier_create: 1 <= threads <= 64, NULL on failure;  etm_host_copy: dst / src non-overlapping, returns when all
 *   bytes are written; one job at a time per copier. */
void *etm_host_copier_create(int threads);
void etm_host_copier_destroy(void *copier);
/* Spin budget of the copier's helper threads between jobs in _mm_pause iterations (default 40,000 ~ 1 ms; 0: sleep on the condition
 * variable at once).  The trainer lowers it to 0 when the rank's CPU share (affinity mask, cgroup quota, ranks per node) does not
 * cover spinning helpers (etm/hostcpu.py). */
int etm_host_copier_set_spin(void *copier, int pauses);
int etm_host_copy(void *copier, void *dst, const void *src, int64_t bytes);

/* Rollout-only encoder convolution with fused bias + ReLU (one `relu(conv2d(x))` of model.py:90-92; forward, no grad):
 * implicit GEMM on fp32 MFMA, no padding/dilation/groups.  in: NCHW [N,C,H,W] (in_nhwc = 0) or NHWC [N,H,W,C]; with
 * in_index non-NULL the input is in + (*in_index) * in_index_stride floats (a row of a staging array chosen on the device);
 * w: the [Cout, K] weight matrix, K ordered (c, ky, kx) for NCHW input (= the native torch layout) or (ky, kx, c) for NHWC
 *    input, PACKED in MFMA fragment order: packed[((g * Cout/32 + t) * 64 + half * 32 + col) * 4 + j]
 *    = w2d[t * 32 + col][g * 8 + half * 4 + j]   (g < K/8, t < Cout/32, half < 2, col < 32, j < 4), so that a wave reads the
 *    B fragment of one 8-wide k-group with one contiguous 1 KB load (etm.ops.conv_pack_weights does the packing);
 * out: NHWC [N,Ho,Wo,Cout] or NCHW (out_nchw = 1).  Shape support: Cout in {32, 64}; NCHW input: KW % 8 == 0, W % 4 == 0,
 * S % 4 == 0; NHWC input: (KW * C) % 8 == 0, C % 4 == 0.  (Covers the three layers of the Atari-style encoder.) */
int etm_conv_relu(const float *in, const int64_t *in_index, int64_t in_index_stride, const float *w, const float *bias, float *out,
                  int N, int C, int H, int W, int Cout, int KH, int KW, int S, int in_nhwc, int out_nchw, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Training-side encoder (model.py:40-56, :90-94): `relu(conv2d(x))` forward, backward-data and backward-weight as fp32-MFMA
 * implicit GEMMs with bias / ReLU / ReLU mask / bias gradient fused (csrc/conv_train.hip).  Activations are NHWC; no padding,
 * dilation or groups; Cout in {32, 64}; (KW * C) % 8 == 0, (W * C) % 4 == 0, (S * C) % 4 == 0; fewer than 2^24 output pixels.
 *   etm_conv_train_fwd  : y = relu(conv(x) + bias).  x NHWC [N,H,W,C]; w_packed = the [Cout, KH*KW*C] matrix (k ordered
 *                         (ky, kx, c)) in the fragment order of etm_conv_relu; y NHWC [N,Ho,Wo,Cout] (out_nchw must be 0: the
 *                         consumer of the last layer permutes its weight columns instead of the features, model.py:94).
 *                         x_index (device int64 [N], or NULL): image n of the batch is image x_index[n] of x (x then holds
 *                         x_images images) -- the minibatch gather of the observations fused into the first layer's loads; the
 *                         same argument of etm_conv_train_wgrad.
 *   etm_conv_train_dgrad: dx = conv_transpose(dy) * (y_below > 0): gradient wrt the layer INPUT x [N,H,W,C], multiplied by the
 *                         ReLU mask of the layer below (y_below = x itself, the post-ReLU output of that layer; NULL: no mask),
 *                         i.e. the pre-activation gradient the next etm_conv_train_wgrad / _dgrad call consumes.  dy NHWC
 *                         [N,Ho,Wo,Cout] is a pre-activation gradient.  Needs KH == KW, KH % S == 0, H % S == 0, W % S == 0,
 *                         C in {32, 64}.  w_packed: S*S blocks, one per stride-parity class (py, px) of the input pixels, each the
 *                         fragment-order packing of Wd[c][(a*T + j)*Cout + co] = w[co][c][py + S a][px + S (T-1-j)], T = KH / S
 *                         (etm.ops.conv_pack_dgrad_weights).
 *   etm_conv_train_wgrad: dw[co][c][ky][kx] = sum over pixels of x-window[(ky, kx, c)] * dy[co] in the parameter's own layout
 *                         [Cout, C, KH, KW], followed by dbias[Cout] = column sums of dy, in one buffer `dw_kc_dbias` of
 *                         KH*KW*C*Cout + Cout floats.  Pixel slices are summed in a fixed order through `workspace`
 *                         (etm_conv_train_wgrad_workspace_bytes): deterministic.
 *   etm_relu_mask       : out = g * (y > 0) over n floats (n % 4 == 0, 16-byte aligned): the ReLU backward of the last layer.
 *   etm_conv_pack_weights: w [Cout, C, KH, KW] -> `fwd` (the w_packed of etm_conv_train_fwd) and / or `dgrad` (the w_packed of
 *                         etm_conv_train_dgrad, all S*S classes), KH*KW*C*Cout floats each, either may be NULL; one launch
 *                         (the weights change every optimiser step). */
int etm_conv_train_fwd(const float *x, const int64_t *x_index, int64_t x_images, const float *w_packed, const float *bias, float *y, int N,
                       int C, int H, int W, int Cout, int KH, int KW, int S, int out_nchw, void *stream);
/* Which forward passes of the three layers of model.py:29-31 on 84 x 84 observations (N >= 512) keep groups of input images resident
 * in LDS (csrc/conv_fwd_lds.hip): bit 0 / 1 / 2 = layer 1 / 2 / 3; 0: the direct-from-L2 kernel for every shape; negative: the
 * default (2: layer 2 only, the one layer where it is faster).  Layers 2 / 3 with x_index keep the direct kernel.  Results differ in
 * summation order only. */
int etm_conv_train_set_fwd_lds(int layer_mask);
/* Likewise for the weight gradients (csrc/conv_wgrad_lds.hip: layer input and gradient image both resident in LDS, one partial result
 * per workgroup): bit per layer, negative = the default (1: the first layer, where it is faster).  A gather index (x_index) is taken on the first layer only; other layers
 * called with one keep conv_wgrad_kernel -- etm_conv_train_wgrad_slices reports the count for x_index == NULL there. */
int etm_conv_train_set_wgrad_lds(int layer_mask);
/* Backward-data of the 4 x 4 / stride 2 layer (model.py:30) at N >= 512 from gradient images resident in LDS
 * (csrc/conv_dgrad_lds.hip): 1 (default) / 0; negative = the default. */
int etm_conv_train_set_dgrad_lds(int on);
/* Grouped forms for the three layers (a launch of this size costs ~5 us whatever it does): etm_conv_pack_weights for n <= 4 layers
 * in one launch; etm_conv_train_wgrad with dw_kc_dbias == NULL leaves etm_conv_train_wgrad_slices(...) pixel slices in its workspace
 * and etm_conv_wgrad_reduce_grouped sums the slices of n <= 4 such calls in one launch into dw[i] [Cout, C, KH, KW] / db[i] [Cout]
 * (the per-call summation order: bit-identical).  Host arrays throughout. */
int etm_conv_pack_weights_grouped(const float *const *w, float *const *fwd, float *const *dgrad, const int *Cout, const int *C,
                                  const int *KH, const int *KW, const int *S, int n, void *stream);
int etm_conv_train_wgrad_slices(int N, int C, int H, int W, int Cout, int KH, int KW, int S);
int etm_conv_wgrad_reduce_grouped(const float *const *partial, const int *slices, float *const *dw, float *const *db, const int *Cout,
                                  const int *C, const int *KH, const int *KW, int n, void *stream);
int etm_conv_train_dgrad(const float *dy, const float *w_packed, const float *y_below, float *dx, int N, int C, int H, int W, int Cout,
                         int KH, int KW, int S, void *stream);
int etm_conv_pack_weights(const float *w, float *fwd, float *dgrad, int Cout, int C, int KH, int KW, int S, void *stream);
int64_t etm_conv_train_wgrad_workspace_bytes(int N, int C, int H, int W, int Cout, int KH, int KW, int S);
int etm_conv_train_wgrad(const float *x, const int64_t *x_index, const float *dy, float *dw_kc_dbias, float *workspace,
                         int64_t workspace_bytes, int N, int C, int H, int W, int Cout, int KH, int KW, int S, void *stream);
int etm_relu_mask(const float *g, const float *y, float *out, int64_t n, void *stream);
/* ---------------------------------------------------------------------------------------------
 * The same encoder passes on the bf16 matrix pipe at fp32 accuracy (round 6, csrc/conv_b3.hip; model.py:40-56, :90-92 and their
 * autograd backward).  Every fp32 operand is split EXACTLY into three bf16 terms and every product accumulated in fp32 as six bf16
 * MFMA products (v_mfma_f32_32x32x16_bf16: 6 x 32 cycles per 16 k against 8 x 64 for v_mfma_f32_32x32x2_f32); the error against
 * float64 is at or below the fp32 MFMA chain's (tools/microbench/b3_gemm.hip).  x / y / dy / dx / dw stay fp32 NHWC tensors exactly
 * as for etm_conv_train_*: the split is internal (images once per group at the LDS fill, weights once per step by etm_conv_b3_pack).
 *   etm_conv_b3_pack : w[i] [Cout, C, KS, KS] -> out[i], 3 * numel bf16 in fragment order ([k / 16][channel tile][plane][lane][8]);
 *                      dgrad[i] != 0: the backward-data operand of that layer (classes x channels as the output columns).
 *   etm_conv_b3_fwd  : y = relu(conv(x) + bias), arguments as etm_conv_train_fwd (the three layers of model.py:29-31 on 84 x 84
 *                      observations; ETM_EUNSUPPORTED otherwise -- the caller keeps the fp32 kernels).
 *                      relu_bits (optional): N * Ho * Wo * Cout / 32 words, bit c % 32 of word [n][y][x][c / 32] = (y > 0).
 *   etm_conv_b3_dgrad: dx = conv_transpose(dy) * (y_below > 0), arguments as etm_conv_train_dgrad (layers 2 / 3); the ReLU pattern of
 *                      the layer below comes from relu_bits (the words its etm_conv_b3_fwd wrote: 1 / 32 of y_below's bytes, requested
 *                      in front of the k loop) if given, else from y_below's values, else there is none. */
int etm_conv_b3_pack(const float *const *w, uint16_t *const *out, const int *dgrad, const int *Cout, const int *C, const int *KS,
                     const int *S, int n, void *stream);
int etm_conv_b3_fwd(const float *x, const int64_t *x_index, const uint16_t *w_b3, const float *bias, float *y, uint32_t *relu_bits, int N,
                    int C, int H, int W, int Cout, int KH, int KW, int S, void *stream);
int etm_conv_b3_dgrad(const float *dy, const uint32_t *dy_relu_bits, const uint16_t *w_b3, const float *y_below, const uint32_t *relu_bits,
                      float *dx, int N, int C, int H, int W, int Cout, int KH, int KW, int S, void *stream);
/*   etm_conv_b3_wgrad: the weight-gradient slices of one layer (csrc/conv_b3_wgrad.hip: both images NHWC in LDS as bf16 planes, the
 *                      pixel contraction fed by transposing LDS reads): workspace [etm_conv_b3_wgrad_slices(...)][K * Cout + Cout], dW in
 *                      (k, co) order (k = (ky, kx, c)) followed by the column sums of dy -- the layout etm_conv_wgrad_reduce_grouped
 *                      sums.  x / x_index / dy as etm_conv_train_wgrad.
 *   dy_relu_bits (etm_conv_b3_dgrad, etm_conv_b3_wgrad; optional): the ReLU pattern words of the layer's OWN output.  dy is then the
 *                      gradient of the ACTIVATION and dy * (y > 0) is formed while the gradient images are filled -- for the last layer
 *                      this replaces the etm_relu_mask launch in front of the backward pass (and its 77 MB of traffic). */
int etm_conv_b3_wgrad_slices(int N, int C, int H, int W, int Cout, int KH, int KW, int S);
int etm_conv_b3_wgrad(const float *x, const int64_t *x_index, const float *dy, const uint32_t *dy_relu_bits, float *workspace,
                      int64_t workspace_bytes, int N, int C, int H, int W, int Cout, int KH, int KW, int S, void *stream);

/* ---------------------------------------------------------------------------------------------
 * uint8 image observations (byte observations).  A byte k stands for the fp32 value float(k) / 255.f, CORRECTLY ROUNDED -- what
 * `obs.astype(np.float32) / 255.` of an image wrapper computes on the host (k * (1 / 255.f) is a different value for 126 of the 256
 * bytes).  Every kernel below forms it at its load with the one conversion helper of csrc/etm_common.h and is otherwise the code of its fp32 twin:
 * same tiles, same split into bf16 terms, same product and reduction order, hence bit-identical results.
 *   etm_bytes_to_unit   : dst[r][j] = unit(src[(index ? index[r] : r)][j]) for r < rows, j < row_bytes -- the general fallback in
 *                         front of every fp32 kernel that has no byte form.  Any row length, any alignment of src; dst dense, 16-byte
 *                         aligned (16-byte stores); index (optional, device int64 [rows]) gathers source rows.
 *   etm_conv_relu_u8    : etm_conv_relu on an NCHW byte input (the first layer; in_nhwc must be 0): per 8-wide k-group a lane reads
 *                         its four consecutive window bytes as one 4-byte load at the fp32 kernel's element offsets.  `in` 4-byte
 *                         aligned, in_index_stride in elements (= bytes) and a multiple of 4; W % 4 == 0, S % 4 == 0 as before;
 *                         Cout == 32 (the first layer's width; ETM_EUNSUPPORTED otherwise).
 *   etm_conv_b3_fwd_u8  : etm_conv_b3_fwd of the FIRST layer (3 x 84 x 84, 8 x 8 / 4, 32 channels) on NHWC byte images: the fill
 *                         loads 16 bytes = 16 elements per lane.  x 16-byte aligned; x_index as etm_conv_b3_fwd.
 *   etm_conv_b3_wgrad_u8: etm_conv_b3_wgrad of the first layer on NHWC byte images; slices = etm_conv_b3_wgrad_slices.
 * ETM_EUNSUPPORTED for every other geometry: the caller expands with etm_bytes_to_unit and runs the fp32 kernels. */
int etm_bytes_to_unit(const uint8_t *src, const int64_t *index, float *dst, int64_t rows, int64_t row_bytes, void *stream);
int etm_conv_relu_u8(const uint8_t *in, const int64_t *in_index, int64_t in_index_stride, const float *w, const float *bias, float *out,
                     int N, int C, int H, int W, int Cout, int KH, int KW, int S, int in_nhwc, int out_nchw, void *stream);
int etm_conv_b3_fwd_u8(const uint8_t *x, const int64_t *x_index, const uint16_t *w_b3, const float *bias, float *y, uint32_t *relu_bits,
                       int N, int C, int H, int W, int Cout, int KH, int KW, int S, void *stream);
int etm_conv_b3_wgrad_u8(const uint8_t *x, const int64_t *x_index, const float *dy, const uint32_t *dy_relu_bits, float *workspace,
                         int64_t workspace_bytes, int N, int C, int H, int W, int Cout, int KH, int KW, int S, void *stream);

/* hipMemcpyAsync(dst, src, bytes, host-to-device) on `stream`: pinned observation rows are streamed into the time-major
 * staging array while the environments still step (trainer.py:190 of the reference uploads per worker, synchronously). */
int etm_upload(void *dst, const void *src, int64_t bytes, void *stream);
/* ---------------------------------------------------------------------------------------------
 * Native rollout driver (round 4): the per-step host loop of the sampler, upstream trainer.py:159-218, for environment workers
 * that are PROCESSES over a shared segment (episodic-transformer-memory-ppo_amd/environments/shm_env.py; upstream worker.py:20-48
 * speaks to them over pipes).  The device hands the actions to the workers itself (the sampling kernel of etm_rollout_trxl /
 * etm_rollout_policy stores them and the step's sequence number into the segment); the workers publish `ready = t + 1` when
 * the observation rows, rewards and done flags of step t are final.
 *
 * etm_host_register / etm_host_unregister: hipHostRegister (portable | mapped) of the shared segment, so that the device can
 *   write the action / sequence words and the copy engine can read the observation rows.  The kernels are handed HOST addresses:
 *   ETM_EUNSUPPORTED if the device address of the registered range differs from the host address.
 * etm_rollout_drive: for t = t_first .. S - 1 and every group -- in the order in which the groups become ready (default; G <= 16,
 *   n_procs <= 64), except that a group with an episode end in step t is served after every lower-numbered group: memory slots
 *   are numbered in the (step, group) order of the loop this replaces (upstream's `len(self.buffer.memories) - 1`, trainer.py:211),
 *   so the results do not depend on the service order:
 *     wait until the group's n_procs `ready` words (ready_stride int64 apart) equal t + 1;
 *     bookkeeping of upstream :195-213 over dones[t, lo..hi): ep_step += 1, or (done) ep_step = 0 and slot = (*next_slot)++ with
 *       an event (t, worker, slot) appended to `events` [max_events][3] / *n_events (ETM_EWORKSPACE when the bank -- `capacity`
 *       slots -- or the event list is full);
 *     if t + 1 < S: (ep_step, slot) of the group -> ss_dst [2, Wg] (pinned), hipMemcpyAsync of the group's observation rows
 *       (obs_src, Wg * row_bytes) to stage_dst + (t + 1) * stage_step_bytes and hipGraphLaunch(graph_exec) -- both on the group's
 *       `stream`.
 *   Blocking; returns when the bookkeeping of step S - 1 is done (the last launched step may still run).  abort_words: n words,
 *   abort_stride int64 apart (the workers' error words + the segment's abort word), polled while waiting -> ETM_EABORTED;
 *   ETM_ETIMEOUT after timeout_s without progress.  timing (optional): [0] seconds waiting for workers, [1] seconds of
 *   bookkeeping + enqueueing; chain_log (optional, [S][4] doubles): step start / group 0's service start (twice) / launched. */
typedef struct etm_rollout_group {
  void *graph_exec;               /* hipGraphExec_t of the group's captured rollout step */
  void *stream;                   /* hipStream_t of the group (step graph and observation upload) */
  const volatile int64_t *ready;  /* first `ready` word of the group's worker processes */
  int32_t n_procs, ready_stride;
  int32_t lo, hi;                 /* worker range of the group */
  const void *obs_src;            /* the group's observation rows in the shared segment */
  void *stage_dst;                /* device: staging row 0 of the group's first worker */
  int64_t *ss_dst;                /* pinned [2, hi - lo]: where the step kernel reads (episode step, slot) */
} etm_rollout_group;
/* hipGraphLaunch(graph_exec, stream) without the framework's per-replay bookkeeping (stream switches, generator checks): the
 * in-process rollout loop launches a group's captured step with it (same call the native driver makes). */
int etm_graph_launch(void *graph_exec, void *stream);
/* Observation rows written by the host straight into device memory (round 6, large-BAR systems; csrc/host_copy.hip): the staging
 * row of the next step is the environment front-end's output buffer, no pinned intermediate and no copy-engine transfer.
 * etm_host_direct_write_init(device): 2 usable + an HDP flush register to write, 1 usable (the device reports none), 0 not usable (the
 * caller keeps pinned memory + etm_upload).  etm_host_store_fence(device):
 * after the rows are written and before the step is launched -- drains the core's write-combining buffers and writes the
 * device's HDP flush register (a posted write behind the rows). */
int etm_host_direct_write_init(int device);
int etm_host_store_fence(int device);
int etm_host_register(void *ptr, int64_t bytes);
int etm_host_unregister(void *ptr);
int etm_rollout_drive(const etm_rollout_group *groups, int G, int t_first, int S, int W, int64_t row_bytes, int64_t stage_step_bytes,
                      const uint8_t *dones, int64_t *ep_step, int64_t *slot, int64_t *next_slot, int64_t capacity, int64_t *events,
                      int64_t max_events, int64_t *n_events, const volatile int64_t *abort_words, int n_abort_words, int abort_stride,
                      double timeout_s, double *timing, double *chain_log);

/* ---------------------------------------------------------------------------------------------
 * Kernel #2: generalized advantage estimation, replaces Buffer.calc_advantages (buffer.py:95-113).
 *   rewards, values, advantages [W,S] fp32 row-major (time contiguous, the reference layout)
 *   dones [W,S] one byte each; last_value [W]
 * The per-worker recurrence is evaluated in the reference's operation order without FMA contraction,
 * so the result is bit-identical to the reference loop.  gamma_lambda = (float)(gamma * lamda) with
 * the product formed in double precision by the caller (python float semantics of buffer.py:111).
 */
int etm_gae(const float *rewards, const uint8_t *dones, const float *values, const float *last_value,
            float gamma, float gamma_lambda, float *advantages, int W, int S, void *stream);
/* Time-limit truncations (ABI 53): the same scan with the next value of a step taken from elsewhere where its episode was only CUT.
 *   truncated [W,S] one byte each, meaningful only where dones is set; boot [W,S] fp32, both laid out like the other arrays
 *     next  = truncated[w,t] ? boot[w,t] : v_{t+1} * (1 - done_t)      (v_S = last_value)
 *     delta = (r_t + gamma * next) - v_t
 *     la    = delta + gamma_lambda * (la * (1 - done_t))
 * in etm_gae's operation order without FMA contraction.  A select, not arithmetic on boot: elements of boot whose flag is clear may
 * hold anything (NaN included) and influence no output; the kernel loads boot only around set flags.  The running advantage is cut
 * at every done, truncated or not.  With every flag clear the result is etm_gae's, bit for bit. */
int etm_gae_truncated(const float *rewards, const uint8_t *dones, const uint8_t *truncated, const float *values, const float *boot,
                      const float *last_value, float gamma, float gamma_lambda, float *advantages, int W, int S, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Running normalisation (ABI 54; absent upstream -- the `VecNormalize` pair of PPO libraries: observations standardised with running
 * per-feature statistics, rewards divided by a running estimate of the spread of the discounted return).  Statistics are
 * (count, mean, M2 = sum (x - mean)^2) triples in DOUBLE, combined with the pairwise update of Chan et al. in an order fixed by the
 * algorithm (never by the grid): no floating-point atomics, identical bits from run to run.  Every entry is a sequence of ordinary
 * launches on `stream`; no workgroup waits for another inside a kernel.
 *
 * etm_obs_stats_update: stands for the host-side `RunningMeanStd.update(batch)` over the rows of one update.
 *   x [R,F] fp32 dense; stats [3,F] doubles (count row, mean row, M2 row) IN/OUT, merged in place with the R rows;
 *   mean [F], rstd [F] fp32 OUT: the frozen table, mean = fp32(mean), rstd = fp32(1 / sqrt(M2 / count + epsilon)) (population
 *   variance; formed in double, rounded once).  Rows are cut into chunks of 256 (a property of the algorithm); launch 1 forms one
 *   triple per (chunk, feature), launch 2 combines them in chunk order, merges into `stats` and writes the table.
 *   workspace: etm_obs_stats_workspace_bytes(R, F) bytes, 8-byte aligned.  etm_obs_stats_supported(F): 1 <= F <= 1024.
 * etm_obs_normalize: stands for `np.clip((obs - mean) / sqrt(var + epsilon), -clip, clip)` in front of the encoder.
 *   out[n][f] = clamp((x[(index ? index[n] : n)][f] - mean[f]) * rstd[f], -clip, +clip), n < N, f < F, in fp32 with the subtraction and
 *   the product rounded separately (no FMA contraction); NaN stays NaN.  index: optional device int64 [N] row gather (a minibatch
 *   taken through indices costs no extra pass).  out dense [N,F].  One launch, capturable.
 * etm_return_scale: stands for the return-based reward scaling of `VecNormalize`, in batch form over one rollout.
 *   rewards [W,S] fp32, dones [W,S] one byte each (the layout of etm_gae); ret_carry [W] doubles IN/OUT: the running discounted return
 *   of every worker, R_t = gamma * R_{t-1} + r_t in double (product and sum rounded separately), R = 0 AFTER a step whose done is set;
 *   stats [3] doubles IN/OUT: all W * S values R_t are merged into it; scale = fp32(1 / sqrt(M2 / count + epsilon)) of the MERGED
 *   triple; scaled [W,S] fp32 OUT = clamp(r * scale, -clip, +clip) in fp32.  Launch 1: the per-worker scan (the shape of etm_gae's)
 *   and one partial triple per workgroup of 16 workers; launch 2: the partials in a fixed order, the merge, the scale; launch 3: the
 *   scaling.  workspace: etm_return_scale_workspace_bytes(W) bytes, 16-byte aligned; its first 4 bytes hold the fp32 scale after the call.
 */
int etm_obs_stats_supported(int F);
int64_t etm_obs_stats_workspace_bytes(int R, int F);
int etm_obs_stats_update(const float *x, int R, int F, double *stats, float *mean, float *rstd, double epsilon, void *workspace,
                         int64_t workspace_bytes, void *stream);
int etm_obs_normalize(const float *x, const int64_t *index, const float *mean, const float *rstd, float clip, float *out, int64_t N,
                      int F, void *stream);
int64_t etm_return_scale_workspace_bytes(int W);
int etm_return_scale(const float *rewards, const uint8_t *dones, double *ret_carry, double *stats, double gamma, double epsilon,
                     float clip, float *scaled, int W, int S, void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Kernel #3: PPO clipped-surrogate + clipped value + entropy loss, forward and backward in one pass.
 * Replaces trainer.py:276-304 and :315-316 for ONE action branch.
 *
 * etm_adv_stats: (count, mean, M2 = sum (a - mean)^2) of `adv` -> stats[3] (fp32).  Kept separate so a
 *   data-parallel caller can merge per-rank statistics before normalising.
 * etm_ppo_loss:
 *   logits [N,A]; actions [N] (stride `action_stride` int64 elements); old_logp [N] (stride
 *   `logp_stride`); adv, old_value, value [N]
 *   adv_stats3 [3]    device scalars (count, mean, M2) of the (global) minibatch, as written by etm_adv_stats;
 *                     the kernel normalises with the unbiased std sqrt(M2 / (count - 1)) + 1e-8 (trainer.py:285)
 *   clip (double: the bounds 1 -/+ clip are formed in double like the reference's python floats), vf_coef, beta:
 *                     hyper-parameters of trainer.py:289-304
 *   pol_scale = 1 / (N * branches), ent_scale = val_scale = 1 / N  (the `.mean()`s of the reference)
 *   include_value: 0 to skip the value term (2nd.. branch of a multi-discrete policy)
 *   dyn_clip_beta: NULL, or device doubles (clip, beta) that override the two scalars at run time with the same arithmetic
 *                  (a captured training step is replayed across updates while the schedules of trainer.py:117-119 decay)
 * outputs
 *   out[8]   : policy, value_loss, loss, entropy, kl, clip_fraction, 0, 0   (trainer.py:318-323 order)
 *   d_logits [N,A], d_value [N] : gradient of `loss` (d_value untouched when include_value == 0)
 *   partials : scratch of etm_ppo_loss_workspace_bytes(N) bytes
 */
int etm_adv_stats(const float *adv, int N, float *stats3, void *stream);
/* The same statistics over many workgroups for large N (>= ETM_ADV_STATS_SPLIT_MIN: per-chunk (count, mean, M2) + a fixed-order
 * merge, Chan et al.; deterministic).  workspace: etm_adv_stats_workspace_bytes(N) bytes (0 for small N: then, and with a NULL
 * workspace, this IS etm_adv_stats, bit for bit). */
#define ETM_ADV_STATS_SPLIT_MIN 65536
int64_t etm_adv_stats_workspace_bytes(int N);
int etm_adv_stats_ws(const float *adv, int N, float *stats3, void *workspace, int64_t workspace_bytes, void *stream);

int64_t etm_ppo_loss_workspace_bytes(int N);

int etm_ppo_loss(const float *logits, const int64_t *actions, int64_t action_stride,
                 const float *old_logp, int64_t logp_stride,
                 const float *adv, const float *old_value, const float *value,
                 const float *adv_stats3,
                 double clip, float vf_coef, float beta,
                 float pol_scale, float ent_scale, float val_scale, int include_value,
                 float *out8, float *d_logits, float *d_value,
                 void *partials, int64_t partials_bytes, const double *dyn_clip_beta,
                 int N, int A, void *stream);
/* Invalid-action masks (ABI 58): etm_ppo_loss of one branch with action_mask [N] int64 (layout of etm_rollout_sample_branched_masked);
 * the branch's A actions are bits [mask_shift, mask_shift + A), mask_shift = its first column of the concatenated policy head (0 for
 * Discrete), mask_shift + A <= 63.  The rule of etm_heads_loss_masked: lse, log-prob and entropy over the valid actions, d_logits = 0
 * exactly on the invalid ones.  One sample per thread (no 16-byte form).  Refusals: "Refusals of the loss entries" (etm_heads_loss). */
int etm_ppo_loss_masked(const float *logits, const int64_t *actions, int64_t action_stride, const float *old_logp, int64_t logp_stride,
                        const float *adv, const float *old_value, const float *value, const float *adv_stats3, double clip, float vf_coef,
                        float beta, float pol_scale, float ent_scale, float val_scale, int include_value, float *out8, float *d_logits,
                        float *d_value, void *partials, int64_t partials_bytes, const double *dyn_clip_beta, int N, int A,
                        const int64_t *action_mask, int mask_shift, void *stream);
/* The exact categorical KL (added at ABI 61) of one branch: etm_ppo_loss_masked with action_mask OPTIONAL (NULL: no masks, mask_shift
 * ignored) and old_logps [N, rows of old_logps_stride floats] (the *_logps sampling entries' rows), the branch's A columns starting at
 * column logps_off.  out8[4] = pol_scale sum_n KL_n (the rule of etm_heads_loss_kl), out8[6] = the k3 value; the loss, d_logits,
 * d_value, out8[0..3], out8[5] and partial slots 0..4 are those of the twin's one-sample-per-thread form, bit for bit; slot 5 of a
 * workgroup's 8 partial floats carries its raw KL sum.  Refusals: "Refusals of the loss entries" (etm_heads_loss). */
int etm_ppo_loss_kl(const float *logits, const int64_t *actions, int64_t action_stride, const float *old_logp, int64_t logp_stride,
                    const float *adv, const float *old_value, const float *value, const float *adv_stats3, double clip, float vf_coef,
                    float beta, float pol_scale, float ent_scale, float val_scale, int include_value, float *out8, float *d_logits,
                    float *d_value, void *partials, int64_t partials_bytes, const double *dyn_clip_beta, int N, int A,
                    const int64_t *action_mask, int mask_shift, const float *old_logps, int64_t old_logps_stride, int logps_off,
                    void *stream);
/* The KL penalty (`kl_penalty`) of one branch: etm_ppo_loss_kl with kl_coef in front of the stream (etm_heads_loss_kl_penalty: ONE
 * device float32 read in place).  d_logits is the gradient of L + coef K (a valid column gains coef pol_scale (p_j - p_old_j), an
 * invalid one stays exactly 0), out8[2] = the twin's loss + coef out8[4], out8[7] = coef; d_value, out8[0, 1, 3, 4, 5, 6] and the
 * partial slots are the twin's.  The term's p_j is exp((logit_j - max) - log(sum)), exact at the largest column (logit_j - lse would
 * carry half a spacing of lse, times coef): equal policies add a term of rounding size here, exactly 0 in the fused entries.
 * Refusals: "Refusals of the loss entries" (etm_heads_loss). */
int etm_ppo_loss_kl_penalty(const float *logits, const int64_t *actions, int64_t action_stride, const float *old_logp,
                            int64_t logp_stride, const float *adv, const float *old_value, const float *value, const float *adv_stats3,
                            double clip, float vf_coef, float beta, float pol_scale, float ent_scale, float val_scale, int include_value,
                            float *out8, float *d_logits, float *d_value, void *partials, int64_t partials_bytes,
                            const double *dyn_clip_beta, int N, int A, const int64_t *action_mask, int mask_shift, const float *old_logps,
                            int64_t old_logps_stride, int logps_off, const float *kl_coef, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient exchange of the data-parallel optimiser step (absent upstream -- the call goes between
 * loss.backward() and clip_grad_norm_, trainer.py:310-311): RCCL over xGMI, one communicator per process (= per GPU).
 *   etm_comm_unique_id(id_out[ETM_COMM_ID_BYTES])   rank 0 creates the rendezvous id; the caller distributes the bytes to all ranks
 *   etm_comm_init(id, rank, world, &comm)           collective over all ranks; binds to the caller's current HIP device
 *   etm_allreduce_f32(comm, send, recv, count, stream)   sum over ranks, in place when send == recv, enqueued on `stream`
 *   etm_comm_destroy(comm)
 * RCCL is dlopen()ed at the first of these calls (no link-time dependency; single-GPU use never loads it).  Errors: ETM_ENOCOMM,
 * or ETM_ERCCL_BASE + ncclResult_t. */
#define ETM_COMM_ID_BYTES 128
int etm_comm_unique_id(void *id_out);
int etm_comm_init(const void *id, int rank, int world, void **comm_out);
int etm_allreduce_f32(void *comm, const float *send, float *recv, int64_t count, void *stream);
int etm_comm_destroy(void *comm);

/* ---------------------------------------------------------------------------------------------
 * Optional per-kernel timing with HIP events on the launch stream (used by bench.py for the roofline numbers).
 *   etm_profile_enable(1/0)      start/stop recording an event pair around every internal kernel launch
 *   etm_profile_set_tag(0/1)     tag subsequent launches (bench: 0 = rollout/inference, 1 = training minibatch)
 *   etm_profile_kernel_count()   number K of internal kernels; etm_profile_kernel_name(k) their names
 *   etm_profile_collect(total_ms[2*K], count[2*K])  synchronise the recorded events, sum per (tag, kernel), reset
 * Not thread-safe; off by default (zero overhead when off apart from one branch per launch).
 */
int etm_profile_enable(int on);
int etm_profile_set_tag(int tag);
int etm_profile_kernel_count(void);
const char *etm_profile_kernel_name(int kernel);
int etm_profile_collect(double *total_ms, int64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* ETM_HIP_H */
