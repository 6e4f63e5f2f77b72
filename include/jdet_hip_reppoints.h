/* jdet_hip_reppoints.h -- the Rotated RepPoints entry points of libjdet_hip.so: the init-stage point assigner and the
 * dense convex GIoU loss.
 *
 * A header of its own for the reason jdet_hip_atss.h and jdet_hip_fcos.h have one: every name of include/jdet_hip.h
 * has a row in the buffer-contract table (tests/abi_cases.py), and that table is revised as a whole.  These entry
 * points are exported by the same library, follow every convention stated at the top of jdet_hip.h (status codes, no
 * synchronisation, no allocation, inputs never written, outputs fully overwritten, bad arguments refused before any
 * launch) and have their contract rows in tests/test_gpu_reppoints.py.  When the contract table is next revised, fold
 * this file into jdet_hip.h together with those rows (and REPPOINTS_SIGNATURES of jdet_amd/_lib.py into SIGNATURES).
 */
#ifndef JDET_HIP_REPPOINTS_H_
#define JDET_HIP_REPPOINTS_H_

#include "jdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* most points one gt may claim in its level (the reference config uses 1, the assigner's default is 3) */
#define JDET_CONVEX_ASSIGN_MAX_POS 16
/* most pyramid levels of one call (the reference config has 5) */
#define JDET_CONVEX_ASSIGN_MAX_LEVELS 8

/* ConvexAssigner.assign (models/boxes/assigner.py:L433-548) for ALL images of a batch in three launches, instead of
 * the reference's host loop over the gts of one image (a mask, a gather, a distance tensor, a topk and two scatter
 * writes per gt).
 *
 *   points         (N, point_stride >= 2) rows [x, y, ...], shared by all images, all levels concatenated.  Only
 *                  columns 0 and 1 are read; the others may hold anything.
 *   level_offsets  HOST pointer, L + 1 ints: level l is the rows [level_offsets[l], level_offsets[l+1]);
 *                  [0] = 0, non-decreasing, [L] = N
 *   level_ids      HOST pointer, L ints: the integer log2(stride) of each level, computed by the caller on the host
 *                  (the reference's jt.log2(points_stride).int(), L482, applied to exact powers of two).  Distinct.
 *   gt             (B, Kmax, 8) polygons [x0, y0, .. x3, y3]; gt_labels (B, Kmax) int32 or NULL
 *   gt_count       DEVICE pointer, (B) int32: image b has the gts [0, gt_count[b]) of its Kmax rows (read in the
 *                  kernel, clamped to [0, Kmax]: no host sync).  Rows beyond it are never read.
 *   out            gt_inds (B, N) int32: 0, or g + 1; labels (B, N) int32 or NULL: gt_labels[b][g], or labels_filled
 *                  where unassigned (labels != NULL needs gt_labels != NULL).  Every element is written.
 *
 * The rules, all in fp32 without contraction and with IEEE division and square root:
 *   box         the horizontal box of a gt is the min / max of its four x and of its four y (L422-431); centre
 *               (cx, cy) = ((xmin + xmax) / 2, (ymin + ymax) / 2); w = max(xmax - xmin, 1e-6f), h likewise (L489-491).
 *   level       gt_lvl = (int)((lg(w / scale) + lg(h / scale)) / 2), truncated toward zero as .int() does (L493-494),
 *               then clamped to [min(level_ids), max(level_ids)] (L495).  lg(x) is log2f(x), except that an exact
 *               power of two (frexpf gives the mantissa 0.5f) returns its exponent as an exactly converted integer: a
 *               gt with w / scale and h / scale exact powers of two lands on the mathematically exact level whatever
 *               the last bit of log2f is.
 *   distance    sqrtf(dx * dx + dy * dy) with dx = (px - cx) / w, dy = (py - cy) / h (L516).
 *   candidates  the min(pos_num, n_level) points of smallest distance in the level whose id is gt_lvl; equal
 *               distances go to the LOWER point index.  The clamp to n_level and the tie rule are this project's (the
 *               reference's topk fails on a level of fewer than pos_num points, and nothing pins its tie order).
 *               A gt whose level id equals no entry of level_ids (a gap in the pyramid) claims nothing.
 *   conflicts   a point claimed by several gts goes to the smallest distance, equal distances to the LOWER gt index:
 *               exactly what the reference's sequential loop with its strict < (L527) leaves.  Resolved
 *               order-independently by a 64-bit integer atomicMin on a per-(image, point) key
 *               (float_bits(distance) << 32) | g; distances are >= 0, so their bit patterns order as integers; the
 *               key ~0 = unclaimed.  The keys are cleared by the first launch (no memset node in a captured step).
 *   no gts      an image with gt_count == 0 writes gt_inds 0 and labels_filled everywhere.  (The reference returns
 *               labels -1 there, L474-476; its caller never reads them.)
 * Launches: clear the keys; one wavefront per (image, gt) finds its candidates -- rank r is the smallest packed key
 * (distance bits << 32 | point index) above rank r - 1's, by a wave-wide 64-bit minimum over the recomputed
 * distances of the level -- and claims them; one lane per (image, point) turns its key into gt_inds / labels.
 *
 * Refused before any launch: JDET_E_BADARG for a null points / level_offsets / level_ids / gt_count / gt_inds /
 * workspace pointer, a null gt with Kmax > 0, labels without gt_labels, a workspace that is not 8-byte aligned,
 * N <= 0, B <= 0, Kmax < 0, L <= 0, point_stride < 2, pos_num <= 0, scale not > 0 or not finite, level_offsets not as
 * above, two equal level_ids; JDET_E_UNSUPPORTED for L > JDET_CONVEX_ASSIGN_MAX_LEVELS, pos_num >
 * JDET_CONVEX_ASSIGN_MAX_POS, B > 65535, B * N or B * Kmax beyond 2^31 - 1; JDET_E_WORKSPACE for fewer bytes than
 * jdet_convex_point_assign_workspace(B, N) (0 for B <= 0 or N <= 0).  The workspace may hold anything. */
size_t jdet_convex_point_assign_workspace(int B, int N);
int jdet_convex_point_assign(const float* points, int N, int point_stride, const int32_t* level_offsets,
                             const int32_t* level_ids, int L, const float* gt, const int32_t* gt_labels,
                             const int32_t* gt_count, int B, int Kmax, float scale, int pos_num, int labels_filled,
                             int32_t* gt_inds, int32_t* labels, void* workspace, size_t workspace_bytes,
                             jdet_stream_t stream);

/* ConvexGIoULossFunction.execute (models/losses/convex_giou_loss.py:L10-53) of P aligned (point set, polygon) rows in
 * its dense form: forward and gradient in ONE launch over ALL rows, the positives marked by their weight, so the step
 * has no nonzero() host round trip.  Half a wavefront per row, the dual-number evaluation of jdet_convex_giou
 * (csrc/convex_giou.h): the GIoU and its 18 derivatives of a row are bit-equal to that entry point's on the same
 * normalised operands.
 *
 *   pred     (P, 18) decoded points [x0, y0, .. x8, y8];  target (P, 8) polygons;  weight (P);  norm (P), the
 *            normalize_term = point_base_scale * stride of each row (rotated_reppoints_head.py:L598, L620-622)
 *   out      loss (P): weight * (1 - giou), unreduced;  grad_pred (P, 18): d loss[row] / d pred[row]
 *
 * Per row, in fp32 with IEEE division:
 *   p = pred / norm, t = target / norm                    (both operands are divided, L620-622)
 *   giou, g[18] = the GIoU of (p, t) and its raw gradient w.r.t. the NORMALISED points p, rounded to fp32
 *   loss = (1 - giou) * weight                            (L33-35)
 *   g = g * weight                                        (L36)
 *   THEN a row with any component g[k] > 1 has all 18 components set to 1e-6f   (L47-48)
 *   then g = -g                                           (L51)
 *   then grad_pred = g / norm                             (the chain rule through p = pred / norm)
 * avg_factor, loss_weight and the incoming gradient are NOT applied here: the autograd node multiplies by them from
 * device scalars.
 * A row of weight == 0 writes loss 0 and gradient 0 without reading pred, target or norm (they may hold anything,
 * NaN included): the rule of jdet_poly_iou_loss.
 *
 * Refused before any launch: JDET_E_BADARG for P < 0, a null pred / target / weight / norm / loss / grad_pred pointer
 * with P > 0; JDET_E_UNSUPPORTED for P beyond 2^32 - 2.  P == 0 is JDET_OK and launches nothing. */
int jdet_convex_giou_loss(const float* pred, const float* target, const float* weight, const float* norm, long P,
                          float* loss, float* grad_pred, jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_REPPOINTS_H_ */
