/* jdet_hip_retina.h -- the RetinaNet-v1d entry points of libjdet_hip.so (csrc/retina.hip,
 * csrc/upsample_add_bilinear.hip): the dense side of models/roi_heads/retina_head.py (RetinaHead, head mode "R" on
 * horizontal anchors) and the bilinear top-down merge of its FPN.  Conventions, error codes and jdet_stream_t are
 * those of jdet_hip.h: nothing is launched on an argument error, inputs are never written, every output element is
 * written, no entry point synchronises or allocates.  All of them are deterministic (no float atomics, no
 * append-by-atomic ordering) and none records a memset node.
 */
#ifndef JDET_HIP_RETINA_H_
#define JDET_HIP_RETINA_H_

#include "jdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Ground-truth preparation of RetinaNet.execute (models/networks/retinanet.py:L31-51).
 *   gts      : (K, 5) [x, y, w, h, a]
 *   rboxes   : (K, 5) -- a >= 0 -> a -= pi; a < -pi/2 -> a += pi/2 and w <-> h; then
 *              cvt2_w_greater_than_h(., reverse_hw=False): w > h -> (x, y, w, h, a - pi/2), else (x, y, h, w, a)
 *   rboxes_h : (K, 4) [x0, y0, x1, y1], the enclosing horizontal box of rboxes with a + pi/2 (rotated_box_to_bbox)
 * Arithmetic in double from the fp32 inputs, every output rounded once.  K = 0 is a no-op. */
int jdet_retina_gt_prepare(const float* gts, int K, float* rboxes, float* rboxes_h, jdet_stream_t stream);

/* RetinaHead.assign_labels + bbox2loc_r (retina_head.py:L136-166, box_ops.py:L66-86, L117-129) for every image and
 * every pyramid level at once: one thread per (image, anchor), the image's horizontal gts staged through LDS in
 * chunks of JDET_RETINA_GT_CHUNK, no (A, K) matrix.
 *   anchors    : (A, 4) [x0, y0, x1, y1], all levels concatenated
 *   rboxes     : (total_gts, 5), rboxes_h (total_gts, 4), gt_labels (total_gts) int32: the prepared gts of all images
 *   gt_offsets : (N + 1) int32 on the DEVICE, non-decreasing, [0] = 0, [N] <= total_gts; image n owns the gts
 *                [gt_offsets[n], gt_offsets[n+1]) (values are clamped to [0, total_gts] before any use)
 * IoU in fp32 in the operations and order of bbox_iou: area_i = (br.x - tl.x) * (br.y - tl.y) * [tl < br in both],
 * area_i / (area_a + area_b - area_i); argmax ties go to the first gt.  Label: max >= pos_iou -> gt_labels[g];
 * neg_lo <= max < neg_hi -> 0; otherwise -1; an image without gts labels every anchor 0.  Location target of a
 * positive: bbox2loc_r(roi, rboxes[g]) with roi = (x, y, h, w, -pi) when the anchor's h > w, else (x, y, w, h, -pi/2)
 * (the reference's +1 on the source sides and eps = 1e-5 inside the logs), in double, rounded once; zeros elsewhere.
 * Outputs, in the form the level-loss nodes of jdet_hip.h read:
 *   labels (N, A) int32 with -1 stored as 0; label_weights (N, A) = [label >= 0]; loc_targets (N, A, 5);
 *   loc_weights (N, A, 5) = [label > 0]; raw_labels (N, A) int32 with the -1 kept;
 *   normalizer (N) = max(#(label > 0), 1) as float, from an integer sum in fixed order.
 * workspace: jdet_retina_targets_workspace(N, A) bytes (per-workgroup positive counts), any content.
 * N = 0 is a no-op; A = 0 writes only the normalizer (1). */
#define JDET_RETINA_GT_CHUNK 256
size_t jdet_retina_targets_workspace(int N, int A);
int jdet_retina_targets(const float* anchors, int A, const float* rboxes, const float* rboxes_h,
                        const int32_t* gt_labels, const int32_t* gt_offsets, int N, int total_gts,
                        float pos_iou_thresh, float neg_iou_thresh_hi, float neg_iou_thresh_lo, int32_t* labels,
                        float* label_weights, float* loc_targets, float* loc_weights, int32_t* raw_labels,
                        float* normalizer, void* workspace, size_t workspace_bytes, jdet_stream_t stream);

/* Front of RetinaHead.get_bboxes (retina_head.py:L198-239) for one image: decode every anchor once with loc2bbox_r
 * (box_ops.py:L36-64) from the proposal (x, y, h, w, -pi/2) when the anchor's h > w, else (x, y, w, h, 0), keeping the
 * reference's (x1+x2)/2, x2-x1 round trip, in double, rounded once; then columns 0, 2 are multiplied by scale_x and
 * columns 1, 3 by scale_y in fp32.  Selected: every (class j, anchor) with sigmoid(logit) > score_thresh (the sigmoid
 * in double, rounded once, compared in fp32) and -pi/2 < angle < pi/2 (the rounded angle against (float)(pi/2)).
 *   anchors (A, 4); loc (A, 5); logits (A, C)
 *   jdet_retina_detect_count: counts (C) int32 = selected anchors per class; the workspace
 *       (jdet_retina_detect_workspace(A, C) bytes, any content on entry) receives the per-workgroup partial counts and
 *       their exclusive prefix sums in class-major order.
 *   jdet_retina_detect_fill: after the caller has read the counts (M = their sum) and with the SAME arguments and the
 *       workspace count left: boxes (M, 5), scores (M), labels (M) int32 = j, class-major, anchor-ascending.  Nothing
 *       is stored at or beyond row M.
 * A = 0: counts are zeroed, fill is a no-op. */
size_t jdet_retina_detect_workspace(int A, int C);
int jdet_retina_detect_count(const float* anchors, const float* loc, const float* logits, int A, int C,
                             float score_thresh, int32_t* counts, void* workspace, size_t workspace_bytes,
                             jdet_stream_t stream);
int jdet_retina_detect_fill(const float* anchors, const float* loc, const float* logits, int A, int C,
                            float score_thresh, float scale_x, float scale_y, const void* workspace,
                            size_t workspace_bytes, int M, float* boxes, float* scores, int32_t* labels,
                            jdet_stream_t stream);

/* Bilinear counterpart of jdet_upsample_add_nhwc_*: out = (lateral + resize(top)) / div_factor on channels-last fp32
 * maps, lateral / out (N, H, W, C), top (N, Ht, Wt, C), C % 4 == 0, 16-byte aligned; H >= Ht and W >= Wt, anything
 * else is JDET_E_UNSUPPORTED.  The resize is nn.resize(mode="bilinear", tf_mode=True) of the reference's framework as
 * DESIGN.md section 5 records it: row coordinate x = float(i) * (float(Ht) / float(H)) in fp32, clamped to [0, Ht - 1]
 * when H > Ht; i0 = floor(x), dx = x - i0, i1 = min(i0 + 1, Ht - 1); columns likewise (y, j0, j1, dy);
 * v = (dx*b + (1-dx)*a) * (1-dy) + (dx*d + (1-dx)*c) * dy with a = (i0, j0), b = (i1, j0), c = (i0, j1), d = (i1, j1).
 * No half-pixel offset.  Backward: grad_top (N, Ht, Wt, C) is a gather -- every coarse pixel sums its pre-image in a
 * fixed order, the candidate rows and columns re-tested with the forward's own coordinate code; grad_lateral is
 * grad_out / div_factor and needs no launch. */
int jdet_upsample_add_bilinear_nhwc_forward(const float* lateral, const float* top, int N, int C, int H, int W,
                                            int Ht, int Wt, float div_factor, float* out, jdet_stream_t stream);
int jdet_upsample_add_bilinear_nhwc_backward(const float* grad_out, int N, int C, int H, int W, int Ht, int Wt,
                                             float div_factor, float* grad_top, jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_RETINA_H_ */
