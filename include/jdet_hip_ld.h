/* jdet_hip_ld.h -- the localization-distillation entry points of libjdet_hip.so: the integral over a discretised
 * regression distribution, its L1 / smooth-L1 level loss, and the knowledge-distillation KL divergence of one level.
 *
 * A header of its own for the reason jdet_hip_atss.h has one: every name of include/jdet_hip.h has a row in the
 * buffer-contract table (tests/abi_cases.py), and that table is revised as a whole.  These entry points are exported
 * by the same library, follow every convention stated at the top of jdet_hip.h (status codes, no synchronisation, no
 * allocation, inputs never written, outputs fully overwritten, bad arguments refused before any launch) and have
 * their contract rows in tests/test_gpu_ld.py.  When the contract table is next revised, fold this file into
 * jdet_hip.h together with those rows (and LD_SIGNATURES of jdet_amd/_lib.py into SIGNATURES).
 *
 * Common to all four (csrc/dist_loss.hip, csrc/dist_softmax.h):
 *   - every tensor is fp32; logits are contiguous row-major; a row of K <= JDET_DIST_MAX_BINS values is one softmax;
 *   - a row's arithmetic (max-subtracted softmax in the log-softmax form, the integral, the loss term, the gradient)
 *     runs in double and is rounded once on output; sums are double, two stages in a fixed order (csrc/reduce.h), no
 *     floating-point atomics: two runs give the same bits;
 *   - targets / weights sit behind the blocked row index of jdet_smooth_l1_loss_level: logical row r lives at
 *     (r / rows_per_block) * block_stride + r % rows_per_block, so a level's window [:, s:e] of the per-image arrays
 *     is read in place;
 *   - `workspace` is the one of jdet_sigmoid_focal_loss_workspace().
 */
#ifndef JDET_HIP_LD_H_
#define JDET_HIP_LD_H_

#include "jdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* most values of one softmax row: reg_max + 1 of the distribution heads, K of the KL divergence */
#define JDET_DIST_MAX_BINS 32

/* box_ops.integral / integral_angle (models/boxes/box_ops.py:L709-723) of all five sides in ONE launch.  Forward only.
 *
 *   logits   (rows, 5 * (reg_max + 1)): side s of a row is the reg_max + 1 values from s * (reg_max + 1) on
 *   deltas   (rows, 5); every element is written
 *   delta[r, s] = sum_k softmax(side s of row r)_k * e_k,  e_k = lo + k * ((hi - lo) / reg_max) evaluated in fp32
 *   with (lo, hi) for the sides s < 4 and (lo_angle, hi_angle) for s == 4: (-2, 2) and (-5, 2) in the reference.
 *
 * Refused before any launch: JDET_E_BADARG for rows < 0, reg_max < 1, an end that is not finite, a null logits /
 * deltas with rows > 0; JDET_E_UNSUPPORTED for reg_max + 1 > JDET_DIST_MAX_BINS.  rows == 0 is a success. */
int jdet_dist_integral(const float* logits, long rows, int reg_max, float lo, float hi, float lo_angle, float hi_angle,
                       float* deltas, jdet_stream_t stream);

/* The integral above followed by the weighted L1 / smooth-L1 of one pyramid level as ONE node, TWO launches.
 *
 *   logits       as above
 *   target, weight   (rows, 5) behind blocked row indices (rows of 5 contiguous values); weight may be NULL (ones)
 *   beta         0: L1; otherwise smooth-L1, |d| < beta ? 0.5 d^2 / beta : |d| - 0.5 beta
 *   avg_factor   DEVICE pointer, one float
 *   loss         one float: (sum_{r,s} w * l(E - t) / *avg_factor) * loss_weight, E = delta[r, s] of the integral
 *   grad_logits  (rows, 5 * (reg_max + 1)), the UNIT gradient d sum / d logits = w * l'(E - t) * p_k * (e_k - E); every
 *                element is written.  Backward is jdet_loss_grad_scale of it.
 *
 * An element of weight 0 contributes nothing and gets gradient 0, whatever its logits and target hold (NaN included);
 * the target of such an element is not read, and no 16-byte piece of logits that lies wholly in rows whose five weights
 * are all 0 is read.
 *
 * Refused before any launch: JDET_E_BADARG for rows < 0, reg_max < 1, beta < 0 or not finite, an end that is not
 * finite, a null loss, and with rows > 0 a null logits / target / avg_factor / grad_logits / workspace or a window
 * with rows_per_block <= 0 or block_stride < 0; JDET_E_UNSUPPORTED for reg_max + 1 > JDET_DIST_MAX_BINS;
 * JDET_E_WORKSPACE for a short workspace.  rows == 0 is a success with *loss = 0. */
int jdet_dist_bbox_loss_level(const float* logits, const float* target, long target_rows_per_block,
                              long target_block_stride, const float* weight, long weight_rows_per_block,
                              long weight_block_stride, long rows, int reg_max, float lo, float hi, float lo_angle,
                              float hi_angle, float beta, const float* avg_factor, float loss_weight, float* loss,
                              float* grad_logits, void* workspace, size_t workspace_bytes, jdet_stream_t stream);

/* knowledge_distillation_kl_div_loss (models/losses/kd_loss.py:L7-39) of one level, the mean over ALL elements of
 * KLDivLoss's default reduction included.  THREE launches with a weight, TWO without.
 *
 *   pred, soft   (M, K) student and teacher logits
 *   weight       M floats behind a blocked index (rows of ONE value), or NULL
 *   T            the temperature, >= 1
 *   sel   = the rows with weight > 0; every row when weight is NULL -- and every row when NO weight is > 0 (the
 *           reference falls through to the full maps there; levels without a positive anchor are routine)
 *   count = |sel|, written to *count (one int32 on the device; the backward reads it, the host never does)
 *   loss  = ((sum_{r in sel} sum_k t_k (log t_k - log p_k)) / float(count * K)) * (T * T) * loss_weight
 *           with p = softmax(pred_r / T), t = softmax(soft_r / T)
 * No 16-byte piece of pred / soft that lies wholly in unselected rows is read.
 *
 * Refused before any launch: JDET_E_BADARG for M < 0, K < 1, T not >= 1 or not finite, a null loss / count, and with
 * M > 0 a null pred / soft / workspace or a bad weight window; JDET_E_UNSUPPORTED for K > JDET_DIST_MAX_BINS or
 * M > 2^31 - 1; JDET_E_WORKSPACE for a short workspace.  M == 0 is a success with
 * *loss = 0 and *count = 0. */
int jdet_kd_kl_div_level_forward(const float* pred, const float* soft, const float* weight, long weight_rows_per_block,
                                 long weight_block_stride, long M, int K, float T, float loss_weight, float* loss,
                                 int32_t* count, void* workspace, size_t workspace_bytes, jdet_stream_t stream);

/* The gradient of the loss above with respect to pred, ONE launch; both softmaxes are recomputed.
 *
 *   count        the forward's output (DEVICE pointer); count == M selects every row
 *   grad_out     DEVICE pointer, one float: the upstream gradient
 *   grad_pred    (M, K): grad_out * loss_weight * T * (p_j - t_j) / float(count * K) on selected rows, 0 elsewhere;
 *                every element is written
 *
 * Refused as the forward (no workspace), and JDET_E_BADARG for a null count / grad_out, or a null grad_pred with M > 0. */
int jdet_kd_kl_div_level_backward(const float* pred, const float* soft, const float* weight, long weight_rows_per_block,
                                  long weight_block_stride, long M, int K, float T, float loss_weight,
                                  const int32_t* count, const float* grad_out, float* grad_pred, jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_LD_H_ */
