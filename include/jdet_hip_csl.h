/* jdet_hip_csl.h -- the Circular Smooth Label entry points of libjdet_hip.so (csrc/csl.hip): the angle branch of
 * models/roi_heads/csl_rretina_head.py (CSLRRetinaHead) -- CSLCoder.encode / decode and the SmoothFocalLoss of a pyramid
 * level on labels that are never materialised.  Conventions, error codes and jdet_stream_t are those of jdet_hip.h:
 * nothing is launched on an argument error, inputs are never written, every output element is written, no entry point
 * synchronises or allocates.  All of them are deterministic (no atomics; every sum in a fixed order) and none records a
 * memset node.  Pointers need 4-byte alignment only.
 *
 * THE RULES (restated in float64 by tests/csl_ref.py; L = coding_len = int(180 // omega)):
 *
 * Bin of a target.  a is the encoded angle delta as DeltaXYWHABBoxCoder gives it (the reference feeds it in
 * unconverted).  t = trunc(((a * float32(180 / pi)) + 45) / float32(omega)), every operation in float32 in that order,
 * truncated toward zero, then wrapped by floor-mod L.  (A target whose quotient is NaN or beyond +-2e9 -- the
 * reference's cast is undefined there -- takes bin 0.)
 *
 * Label of bin j for the target bin t.  Offsets b are added to t in bins, (t + b) floor-mod L:
 *   JDET_CSL_PULSE     b in {0}                       value 1
 *   JDET_CSL_RECT      b in -radius .. radius - 1     value 1
 *   JDET_CSL_TRIANGLE  b in -radius .. radius - 1     value 1 - |b| / radius
 *   JDET_CSL_GAUSSIAN  b in -90 .. 89, whatever L is  value exp(-b^2 / (2 radius^2))
 * every other bin 0.  For L < 180 the gaussian offsets reach a bin several times; the reference writes them with a
 * scatter whose winner among duplicate indices is undefined.  HERE THE LARGEST VALUE WINS: exp(-d^2 / (2 radius^2)) of
 * the circular distance d = min((j - t) mod L, (t - j) mod L), which is the label of the CSL paper and equals the
 * reference wherever the reference is defined (L = 180).  RECT / TRIANGLE need an integer radius >= 1 with
 * 2 * radius <= L (no bin is reached twice); GAUSSIAN any finite radius > 0.  Labels are evaluated in double and used in
 * double by the loss; jdet_csl_encode rounds them once.
 *
 * Loss of a level.  A row is selected when column 4 of its weight row is > 0; the weight is a mask, never a factor.
 * Per selected row and bin, with x the logit, y the label, e = exp(-|x|), p = sigmoid(x), q = 1 - p (both from e, so
 * neither cancels), pt = q y + p (1 - y), aw = alpha y + (1 - alpha)(1 - y), bce = max(x, 0) - x y + log1p(e):
 *   l      = bce * aw * pt^gamma
 *   dl/dx  = aw * [gamma pt^(gamma - 1) p q (1 - 2 y) bce + pt^gamma (p (1 - y) - q y)]       (p - y, without the cancellation)
 * in double, each gradient element rounded once.  loss = ((sum l) / *avg_factor) * loss_weight, rounded once; the sum runs
 * in a fixed order (lane, wave, workgroup partials in the workspace, one finishing launch), so two runs agree bit for bit.
 * Of an unselected row only the weight is read -- neither its logits nor its target: NaN there reaches nothing -- and its
 * gradient row is exact zeros.  No selected row: loss 0 (avg_factor finite and non-zero), gradient all zeros.
 * gamma == 0 or gamma >= 1 (pt^(gamma - 1) at pt = 0); 1 <= L <= 180: anything else is JDET_E_UNSUPPORTED.
 *
 * Decode.  idx = the FIRST index of the row maximum of the LOGITS; angle = (((idx + 0.5) * omega) mod 180 - 45) * pi / 180
 * in double, rounded once.  The reference takes the argmax after a float32 sigmoid: the two differ only where the sigmoid
 * rounds two different logits to one float (then the reference takes the earlier bin).  A row of NaN gives idx 0.
 */
#ifndef JDET_HIP_CSL_H_
#define JDET_HIP_CSL_H_

#include "jdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JDET_CSL_PULSE 0
#define JDET_CSL_RECT 1
#define JDET_CSL_TRIANGLE 2
#define JDET_CSL_GAUSSIAN 3
#define JDET_CSL_MAX_BINS 180

/* CSLCoder.encode: angle (n) -> labels_out (n, coding_len), fully written.  n = 0 is a no-op.
 * JDET_E_BADARG: null pointer with n > 0, n < 0, coding_len < 1, omega / radius not as above, unknown window;
 * JDET_E_UNSUPPORTED: coding_len > JDET_CSL_MAX_BINS, n * coding_len >= 2^31. */
int jdet_csl_encode(const float* angle, long n, int coding_len, double omega, int window, double radius,
                    float* labels_out, jdet_stream_t stream);

/* CSLCoder.decode of n rows of a contiguous (rows, coding_len) array of logits: row index[i] (int64), or row i when
 * index is null (then n <= rows) -> angle_out (n).  An index outside [0, rows) reads nothing and gives NaN.
 * n = 0 is a no-op.  Errors as jdet_csl_encode; rows < 0 is JDET_E_BADARG. */
int jdet_csl_decode(const float* logits, long rows, const int64_t* index, long n, int coding_len, double omega,
                    float* angle_out, jdet_stream_t stream);

/* The angle loss of one pyramid level, forward and unit gradient in one pass.
 *   logits (rows, coding_len) contiguous; target / weight: (rows, 5) windows of the level's bbox_targets / bbox_weights,
 *   blocked as in jdet_dist_bbox_loss_level (logical row r is row r % rows_per_block of block r / rows_per_block, blocks
 *   block_stride rows apart); column 4 is read in place, the other columns never.
 *   avg_factor: one float on the DEVICE.  loss (1).  grad_logits (rows, coding_len): d (sum l) / d logits, fully written;
 *   the backward is jdet_loss_grad_scale on it.
 *   workspace: jdet_sigmoid_focal_loss_workspace() bytes, any content (the double partial sums, at most
 *   workspace / 8 workgroups of 64-row tiles).
 * rows = 0 writes loss = 0.  JDET_E_BADARG: null pointer, rows < 0, a window with rows_per_block <= 0 or
 * block_stride < 0, coding_len < 1, gamma < 0, non-finite gamma / alpha / loss_weight, label parameters as in
 * jdet_csl_encode; JDET_E_UNSUPPORTED: coding_len > JDET_CSL_MAX_BINS, 0 < gamma < 1, rows * coding_len >= 2^40;
 * JDET_E_WORKSPACE. */
int jdet_csl_angle_loss_level(const float* logits, const float* target, long target_rows_per_block,
                              long target_block_stride, const float* weight, long weight_rows_per_block,
                              long weight_block_stride, long rows, int coding_len, double omega, int window,
                              double radius, float gamma, float alpha, const float* avg_factor, float loss_weight,
                              float* loss, float* grad_logits, void* workspace, size_t workspace_bytes,
                              jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_CSL_H_ */
