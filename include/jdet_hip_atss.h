/* jdet_hip_atss.h -- the ATSS assigner entry points of libjdet_hip.so.
 *
 * Why a header of its own: every name of include/jdet_hip.h has a row in the buffer-contract table
 * (tests/abi_cases.py), and that table is revised as a whole.  These two entry points arrived between two revisions:
 * they are exported by the same library, follow every convention stated at the top of jdet_hip.h (status codes, no
 * synchronisation, no allocation, inputs never written, outputs fully overwritten) and have their contract rows in
 * tests/test_gpu_atss.py.  When the contract table is next revised, fold this file into jdet_hip.h together with
 * those rows (and ATSS_SIGNATURES of jdet_amd/_lib.py into SIGNATURES).
 */
#ifndef JDET_HIP_ATSS_H_
#define JDET_HIP_ATSS_H_

#include "jdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Most candidates (levels x topk) one gt may have: one wavefront lane per candidate.  The reference config has 5 x 9. */
#define JDET_ATSS_MAX_CANDIDATES 64

/* ATSSAssignerRbbox.assign (models/boxes/assigner.py:L314-391; points_in_rotated_boxes, boxes/box_ops.py:L725-741) in
 * three launches, without the (A, K) IoU / distance / inside matrices, the five topk calls, the per-gt loop and the
 * second "-INF" matrix of the reference: only the K x C candidate pairs are ever evaluated.
 *
 *   anchors        (A, anchor_stride >= 5) rows [xc, yc, w, h, theta], all levels concatenated
 *   level_offsets  HOST pointer, L + 1 ints: level l is the rows [level_offsets[l], level_offsets[l+1]);
 *                  [0] = 0, non-decreasing, [L] = A
 *   gt             (K, 5); gt_labels (K) int32 or NULL
 *   overlaps       NULL: the IoU of a candidate pair is computed in the kernel by the device function
 *                  jdet_box_iou_rotated uses (version 0, sort_mode 0; argument order (anchor, gt)), bit-equal to
 *                  that entry point's matrix element.  Non-NULL: an (A, K) row-major matrix the caller computed
 *                  with any iou_calculator; its values are read instead.  They must be >= 0.
 *   out            gt_inds (A) int32: 0 or g + 1; max_overlaps (A): the winning IoU, or -1e8f (the reference's
 *                  -INF, L374) where unassigned; labels (A) int32 or NULL: gt_labels[g], or labels_filled where
 *                  unassigned (labels != NULL needs gt_labels != NULL).  Every element is written.
 *
 * The rules, step by step.  Those the reference leaves open are this project's:
 *   distance     sqrtf(dx*dx + dy*dy) of the centres in fp32, no contraction (L329-330).
 *   candidates   per (gt, level) the min(topk, n_level) anchors of smallest distance; equal distances go to the
 *                LOWER anchor index (Jittor's topk tie order is not pinned by anything; this one is ours).  The
 *                clamp to n_level is mmdet's (the reference's topk would fail on a level of fewer than topk
 *                anchors); a level of 0 anchors contributes nothing.  Candidate order: level-major, then rank;
 *                C = sum_l min(topk, n_l) per gt.
 *   threshold    mean and unbiased variance (/(C-1), L350-356) summed serially in candidate order in fp32:
 *                s = 0; s += iou[c]; mean = s / C; v = 0; d = iou[c] - mean; v += d * d; var = v / (C - 1);
 *                thr = mean + sqrtf(fmaxf(var, 1e-6f)).
 *   inside       |dx*cos(a) + dy*sin(a)| < w/2 and |-dx*sin(a) + dy*cos(a)| < h/2 with (dx, dy) = anchor centre
 *                - gt centre and one sincosf per gt.  This is the algebraic form of L734-740, which takes
 *                r = |(dx, dy)|, phi = atan2(dy, dx) and tests |r cos(phi - a)| < w/2, |r sin(phi - a)| < h/2:
 *                r cos(phi - a) = dx cos a + dy sin a and r sin(phi - a) = -dx sin a + dy cos a.  The two forms can
 *                differ only for a centre within rounding of a gt's edge.
 *   positive     iou >= thr, inside and iou > 0 (thr >= 1e-3 whenever the IoUs are >= 0).
 *   conflicts    an anchor claimed by several gts goes to the highest IoU, equal IoUs to the LOWER gt index (the
 *                first index, as jt.argmax).  Resolved by a 64-bit integer atomicMax on a per-anchor key
 *                (float_bits(iou) << 32) | (0xFFFFFFFF - g): order-independent, hence deterministic; key 0 =
 *                unassigned.  The keys are cleared by the first launch (no memset node in a captured step).
 *
 * Refused before any launch: JDET_E_BADARG for a null anchors / level_offsets / gt / gt_inds / max_overlaps /
 * workspace pointer, labels without gt_labels, a workspace that is not 8-byte aligned, A <= 0, K <= 0, L <= 0,
 * topk <= 0, anchor_stride < 5, level_offsets not as above; JDET_E_UNSUPPORTED for L * topk >
 * JDET_ATSS_MAX_CANDIDATES or C < 2 (the variance divides by C - 1); JDET_E_WORKSPACE for fewer bytes than
 * jdet_atss_assign_workspace(A, K, L, topk).  The workspace may hold anything. */
size_t jdet_atss_assign_workspace(int A, int K, int L, int topk);
int jdet_atss_assign(const float* anchors, int A, int anchor_stride, const int32_t* level_offsets, int L,
                     const float* gt, int K, const int32_t* gt_labels, const float* overlaps, int topk,
                     int labels_filled, int32_t* gt_inds, float* max_overlaps, int32_t* labels, void* workspace,
                     size_t workspace_bytes, jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_ATSS_H_ */
