/* jdet_hip_h2rbox.h -- the H2RBox entry points of libjdet_hip.so: the rotated, centre-cropped second view and the
 * view-consistency loss.
 *
 * A header of its own for the reason jdet_hip_atss.h has one: every name of include/jdet_hip.h has a row in the
 * buffer-contract table (tests/abi_cases.py), and that table is revised as a whole.  These entry points are exported
 * by the same library, follow every convention stated at the top of jdet_hip.h (status codes, no synchronisation, no
 * allocation, inputs never written, outputs fully overwritten, bad arguments refused before any launch) and have
 * their contract rows in tests/test_gpu_h2rbox.py.  When the contract table is next revised, fold this file into
 * jdet_hip.h together with those rows (and H2RBOX_SIGNATURES of jdet_amd/_lib.py into SIGNATURES).
 */
#ifndef JDET_HIP_H2RBOX_H_
#define JDET_HIP_H2RBOX_H_

#include "jdet_hip.h"
#include "jdet_hip_fcos.h" /* JDET_FCOS_MAX_LEVELS: the level table is jdet_fcos_targets' */

#ifdef __cplusplus
extern "C" {
#endif

/* padding modes of jdet_rotate_crop (the order of torch.nn.functional.grid_sample's) */
#define JDET_PAD_ZEROS 0
#define JDET_PAD_BORDER 1
#define JDET_PAD_REFLECTION 2
/* most rotation-agnostic classes of one jdet_h2rbox_aug_loss_forward call */
#define JDET_H2RBOX_MAX_AGNOSTIC 16

/* H2RBox.rotate_crop (models/networks/h2rbox.py:L35-75) of an image batch in ONE launch: only the out_h x out_w window
 * that survives the centre crop is computed, the (n, h, w, 2) grid never exists.  Forward only (images carry no
 * gradient).
 *
 *   img      (N, C, H, W) fp32, NCHW
 *   out      (N, C, out_h, out_w) fp32; every element is written
 *   cos_t, sin_t   cos / sin of the angle, computed on the host in double and rounded to float (the reference stores
 *            math.cos / math.sin in a float tensor, L42-43)
 *
 * Per output pixel (n, y, x), the same coordinates for all C channels:
 *   (X, Y)   = (x + (W - out_w) / 2, y + (H - out_h) / 2)                     (integer division: the crop offset, L39-40)
 *   (gx, gy) = (-1 + 2 X / (W - 1), -1 + 2 Y / (H - 1))                       (linspace(-1, 1, .), L45-46)
 *   (sx, sy) = (gx * cos + gy * sin, -gx * sin + gy * cos)                    (row vector times [[cos, -sin], [sin, cos]],
 *                                                                              L43-49; no isometry when H != W: kept)
 *   (ix, iy) = ((sx + 1) / 2 * (W - 1), (sy + 1) / 2 * (H - 1))               (align_corners = True)
 *   padding  reflection about 0 and size - 1 followed by a clip to [0, size - 1]; border: that clip alone; zeros: a
 *            corner outside the frame contributes 0
 *   value    bilinear over the four corners floor(ix), floor(ix) + 1, floor(iy), floor(iy) + 1, as grid_sample
 * The coordinates are computed in double (a dozen operations per pixel, shared by the channels), the interpolation in
 * fp32.  cos_t == 1 && sin_t == 0 (theta == 0) is a bit-exact cropped copy: the reference skips the sampling there.
 *
 * Refused before any launch: JDET_E_BADARG for a null img / out, N, C, out_h or out_w <= 0, H < 2 or W < 2,
 * out_h > H or out_w > W, an unknown padding mode, cos_t or sin_t not finite; JDET_E_UNSUPPORTED for N > 65535 or
 * N * C * H * W beyond 2^31 - 1. */
int jdet_rotate_crop(const float* img, int N, int C, int H, int W, int out_h, int out_w, float cos_t, float sin_t,
                     int padding, float* out, jdet_stream_t stream);

/* The consistency branch of H2RBoxHead.loss (models/roi_heads/h2rbox_head.py:L399-506) with H2RBoxLoss.execute
 * (models/losses/h2rbox_loss.py:L42-66), dense over all B * N points in the image-major order jdet_fcos_targets writes,
 * one thread per view-1 point, ONE launch.
 *
 *   levels        HOST pointer, L rows of 3 ints (H, W, stride), as for jdet_fcos_targets: N = sum H * W
 *   pred          (B, N, 5) rows [l, t, r, b, theta] of view 1, as the head emits them
 *   pred_aug      (B, N, 5) the same of view 2 (the rotated view)
 *   weight        (B, N) the centerness targets; a row takes part when weight > 0
 *   labels        (B, N) int32 as jdet_fcos_targets writes them (0-based), or NULL when n_agnostic == 0
 *   agnostic      HOST pointer, n_agnostic 1-BASED class ids (the reference compares rotation_agnostic_classes with
 *                 labels + 1, L387/L440/L487-491), or NULL when n_agnostic == 0
 *   rot, cos_r, sin_r   the angle of view 2 and its cos / sin computed on the host in double, rounded to float
 *   crop_h, crop_w      the size of both views in pixels
 *   shape_weight, angle_weight   loss_weight of H2RBoxLoss's shape_loss and angle_loss (1 and 1 in the config)
 *   eps           the clamp of the IoU and of its union (1e-6 in the reference)
 *   out           terms (B, N, 4): [centre, branch 1, branch 2, weight] of a valid row, zeros otherwise;
 *                 aug_index (B, N) int32: the view-2 point, in 0 .. N - 1 of the same image, of a valid row, -1
 *                 otherwise.  Every element is written.
 *
 * Cell map.  A row with weight > 0 at cell (x, y) of a level (h, w) goes to
 *   (xa, ya) = round(((x, y) - ctr) . [[cos, sin], [-sin, cos]] + ctr),  ctr = ((w - 1) / 2, (h - 1) / 2)
 * i.e. xa = round(dx * cos + dy * (-sin) + cx), ya = round(dx * sin + dy * cos + cy), in fp32 without contraction.
 * TIE RULE: round is round-half-to-EVEN (rintf, torch.round); both Python routes follow it.  The row is VALID when
 * 0 <= xa < w and 0 <= ya < h; its view-2 point is off[level] + ya * w + xa.
 *
 * A valid row decodes both predictions with distance2obb (boxes/box_ops.py:L694-707, regular_obb included) at their
 * own points (x * stride + stride / 2, y * stride + stride / 2).  The TARGET is view 1's decoded box [cx, cy, w, h, a]
 * with (cx, cy) turned about ((crop_w - 1) / 2, (crop_h - 1) / 2) by the same matrix, w and h kept, and the angle
 * a + rot, times 0 for a rotation-agnostic row (_process_rotation_agnostic(dim=None), L312-319).  With P the decoded
 * view-2 box, da = P.a - T.a and iou(.) of bbox_overlaps(is_aligned=True) (its max(union, eps) included) clamped
 * below by eps:
 *   centre    weight * (|P.cx - T.cx| + |P.cy - T.cy|)
 *   branch 1  weight * (shape_weight * -log(iou([-w, -h, w, h] of P, the same of T)) + angle_weight * |sin da|)
 *   branch 2  the same with P's w and h swapped and |cos da|
 * Rows of weight <= 0 and invalid rows read neither prediction (NaN there is harmless).
 * The cell map is fp32 (so that the fp32 tensor program decides as the kernel does); a row's arithmetic after it runs
 * in double and is rounded once on output.
 *
 * The scalar minimum of the reference is the caller's: H2RBoxLoss reduces each sub-loss before jt.minimum, so the loss
 * is loss_weight * (w_c * sum centre + min(sum branch 1, sum branch 2)) / max(sum terms[..., 3], 1) -- NOT a per-row
 * minimum.
 *
 * Refused before any launch: JDET_E_BADARG for a null levels / pred / pred_aug / weight / terms / aug_index, B <= 0,
 * L <= 0, a level with H, W or stride <= 0, crop_h or crop_w <= 0, n_agnostic < 0, n_agnostic > 0 with a null labels
 * or agnostic, eps not > 0, rot / cos_r / sin_r / shape_weight / angle_weight not finite; JDET_E_UNSUPPORTED for
 * L > JDET_FCOS_MAX_LEVELS, n_agnostic > JDET_H2RBOX_MAX_AGNOSTIC, B > 65535 or B * N * 5 beyond 2^31 - 1. */
int jdet_h2rbox_aug_loss_forward(const int32_t* levels, int L, const float* pred, const float* pred_aug,
                                 const float* weight, const int32_t* labels, const int32_t* agnostic, int n_agnostic,
                                 int B, float rot, float cos_r, float sin_r, int crop_h, int crop_w, float shape_weight,
                                 float angle_weight, float eps, float* terms, int32_t* aug_index,
                                 jdet_stream_t stream);

/* The gradient of  scale_centre * sum centre + scale_branch * sum branch[*branch]  of the forward above, TWO launches.
 *
 *   (levels .. eps)   as the forward's
 *   aug_index     (B, N) int32, the forward's output
 *   branch        DEVICE pointer, one int32: 0 selects branch 1, anything else branch 2 (the scalar minimum taken on
 *                 the device); the other branch contributes nothing
 *   scale_centre, scale_branch   DEVICE pointers, one float each: the upstream scales
 *                 (grad_out * loss_weight * w_c / avg and grad_out * loss_weight / avg)
 *   out           grad_pred (B, N, 5), grad_pred_aug (B, N, 5); every element is written.
 *
 * The view-1 side is NOT detached (the reference builds the target from pos_decoded_bbox_preds, L480-494): gradient
 * flows into both views.  regular_obb's swap and floor-mod pass gradient with factor 1; abs has gradient 0 at 0, as in
 * autograd.  At the exact ties of the piecewise pieces the kernel's rule is its own and DIFFERS from autograd's: where
 * the prediction's and the target's half-extent are equal (pw == tw or ph == th) the whole gradient of the min / max
 * goes to the TARGET's side (torch.minimum / torch.maximum split it evenly there), and a union or IoU exactly at eps
 * counts as clamped, gradient 0 (torch.clamp passes the gradient at equality).  Away from ties the two agree; the
 * test fixtures keep every such quantity at least 1e-3 from its tie, so nothing pins the tie rule.
 *
 * Several view-1 rows may share a view-2 point.  Launch 1, one thread per view-1 point p, writes grad_pred[p] and its
 * contribution to its view-2 point into row p of a scratch the caller provides (contrib).  Launch 2, one thread per
 * view-2 point q, sums the rows p with aug_index[p] == q among the 3 x 3 cells around round(R^-1 (q - ctr) + ctr) in
 * ascending p (if round(R (p - ctr) + ctr) == q then |p - R^-1 (q - ctr) - ctr| <= sqrt(2) / 2 per coordinate, so p
 * lies in that block): no floating-point atomics, a fixed summation order, bit-identical runs.
 *
 *   contrib       (B, N, 5) fp32 scratch, fully overwritten
 *
 * Refused as the forward, and JDET_E_BADARG for a null aug_index / branch / scale_centre / scale_branch / grad_pred /
 * grad_pred_aug / contrib. */
int jdet_h2rbox_aug_loss_backward(const int32_t* levels, int L, const float* pred, const float* pred_aug,
                                  const float* weight, const int32_t* labels, const int32_t* agnostic, int n_agnostic,
                                  int B, float rot, float cos_r, float sin_r, int crop_h, int crop_w,
                                  float shape_weight, float angle_weight, float eps, const int32_t* aug_index,
                                  const int32_t* branch, const float* scale_centre, const float* scale_branch,
                                  float* grad_pred, float* grad_pred_aug, float* contrib, jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_H2RBOX_H_ */
