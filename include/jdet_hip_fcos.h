/* jdet_hip_fcos.h -- the rotated FCOS entry points of libjdet_hip.so: point targets and the polygon IoU loss.
 *
 * A header of its own for the reason jdet_hip_atss.h has one: every name of include/jdet_hip.h has a row in the
 * buffer-contract table (tests/abi_cases.py), and that table is revised as a whole.  These entry points are exported
 * by the same library, follow every convention stated at the top of jdet_hip.h (status codes, no synchronisation, no
 * allocation, inputs never written, outputs fully overwritten, bad arguments refused before any launch) and have
 * their contract rows in tests/test_gpu_fcos.py.  When the contract table is next revised, fold this file into
 * jdet_hip.h together with those rows (and FCOS_SIGNATURES of jdet_amd/_lib.py into SIGNATURES).
 */
#ifndef JDET_HIP_FCOS_H_
#define JDET_HIP_FCOS_H_

#include "jdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gts of one image staged in LDS at a time; an image of more gts is walked in chunks of this size, so any K works */
#define JDET_FCOS_GT_CHUNK 64
/* most pyramid levels of one call (the reference config has 5) */
#define JDET_FCOS_MAX_LEVELS 8

/* FCOSHead.get_targets (models/roi_heads/fcos_head.py:L535-670) for all images and all levels in ONE launch, one
 * thread per (image, point), without the (points x gts) tensors of areas, ranges, offsets, matrices and distances.
 *
 *   levels          HOST pointer, L rows of 3 ints (H, W, stride): level l has H * W points, row-major, point (x, y) at
 *                   (x * stride + stride / 2, y * stride + stride / 2) (integer division, L532); the points of all
 *                   levels concatenated are the N = sum H * W points of an image
 *   regress_ranges  HOST pointer, L rows of 2 floats (lo, hi)
 *   gt              (B, Kmax, 5) rows [xc, yc, w, h, theta]; gt_labels (B, Kmax) int32, 1-based as everywhere here
 *   gt_count        DEVICE pointer, (B) int32: image b has the gts [0, gt_count[b]) of its Kmax rows (read in the
 *                   kernel, clamped to [0, Kmax]: no host sync).  Rows beyond it are never read.
 *   out             labels (B, N) int32: gt_labels - 1 of the winner in 0 .. num_classes - 1, or num_classes
 *                   (background); bbox_targets (B, N, 5) [l, t, r, b, theta], l..b divided by the level's stride when
 *                   norm_on_bbox; centerness (B, N): sqrtf(min(l,r)/max(l,r) * (min(t,b)/max(t,b))) of the values
 *                   written to bbox_targets, 0 for background; gt_inds (B, N) int32 or NULL: the winner's index, -1
 *                   for background.  Every element is written.
 *
 * Each gt is prepared once by the thread that stages it: mintheta_obb (boxes/box_ops.py:L679-692, with its
 * pi = 3.141592), one sincosf of the resulting angle, the area w * h of the INPUT box, label - 1.  Per (point, gt), in
 * fp32 without contraction:
 *   (ox, oy) = point - centre;  rx = cos * ox + (-sin) * oy;  ry = sin * ox + cos * oy      ([cos, -sin; sin, cos], L619)
 *   l = w/2 + rx, r = w/2 - rx, t = h/2 + ry, b = h/2 - ry
 *   inside  min(l, t, r, b) > 0; with center_sampling also |rx| < stride * radius and |ry| < stride * radius (L635-649)
 *   range   max(l, t, r, b) >= lo && max(l, t, r, b) <= hi, inclusive on both sides (L652-655)
 * The rules the reference leaves open or gets wrong are this project's:
 *   winner      the smallest area among the gts that pass both tests; equal areas go to the LOWER gt index (the first
 *               minimum, as an argmin that scans upwards).
 *   background  a point no gt survives at gets the label num_classes, bbox_targets 0 0 0 0 0, centerness 0 and
 *               gt_inds -1.  (The reference's argmin over an all-INF row picks gt 0 and keeps its distances; nothing
 *               reads them.  The general route of FCOSHead.get_targets writes the same zeros.)
 *   no gts      an image with gt_count == 0 is background everywhere.  (The reference returns label 0 there, L604-606,
 *               which marks every point as class 0: not reproduced.)
 *
 * Refused before any launch: JDET_E_BADARG for a null levels / regress_ranges / gt_count / labels / bbox_targets /
 * centerness pointer, null gt or gt_labels with Kmax > 0, B <= 0, Kmax < 0, L <= 0, num_classes <= 0, a level with
 * H, W or stride <= 0, radius <= 0 or not finite with center_sampling; JDET_E_UNSUPPORTED for L > JDET_FCOS_MAX_LEVELS,
 * B > 65535 or B * N beyond 2^31 - 1. */
int jdet_fcos_targets(const int32_t* levels, const float* regress_ranges, int L, const float* gt,
                      const int32_t* gt_labels, const int32_t* gt_count, int B, int Kmax, int num_classes,
                      int norm_on_bbox, int center_sampling, float radius, int32_t* labels, float* bbox_targets,
                      float* centerness, int32_t* gt_inds, jdet_stream_t stream);

/* poly_iou_loss (models/losses/poly_iou_loss.py:L39-123) of P box pairs, forward and gradient in ONE launch, one
 * thread per row.
 *
 *   pred, target   (P, 5) rows [xc, yc, w, h, theta]
 *   weight         (P) or NULL (= 1)
 *   out            loss (P): weight * (linear ? 1 - iou : -logf(iou)), unreduced; grad_pred (P, 5):
 *                  d loss[row] / d pred[row], weight included.  The target gets no gradient.
 *
 * A row of weight == 0 writes loss 0 and gradient 0 without reading pred or target (they may hold anything, NaN
 * included), so a dense call over all points does the geometry for the positives only.
 *
 * The mathematics is the reference's, line by line, in fp32 without contraction and with IEEE division: obb -> poly as
 * ops/bbox_transforms.obb2poly; the 16 edge-pair intersections with t = den_t / (num + eps) for the point and the
 * masks from the plain quotients den_t / num and den_u / num (parallel edges give +-inf or NaN, which compare false);
 * the two vertex-inside masks by the triangle-area sums against 1e-3 * area; the Graham scan of jdet_convex_sort over
 * the 24 masked points; the shoelace sum; iou = max(overlap / (a1 + a2 - overlap + eps), eps) with a = w * h.
 * The gradient is the reverse of exactly that: through the abs of the shoelace sum (sign 0 at 0), through the
 * gathered hull points (the indices and masks are constants), through t into the pred-side edge endpoints and through
 * the pred vertices directly, through a1; zero where the clamp is active (overlap / union < eps), so a disjoint pair
 * gets -log(eps) and gradient 0.
 *
 * Refused before any launch: JDET_E_BADARG for P < 0, a null pred / target / loss / grad_pred pointer with P > 0, eps
 * not > 0.  P == 0 is JDET_OK and launches nothing. */
int jdet_poly_iou_loss(const float* pred, const float* target, const float* weight, long P, int linear, float eps,
                       float* loss, float* grad_pred, jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_FCOS_H_ */
