/* jdet_hip.h -- C ABI of libjdet_hip.so: the MI355X (gfx950) implementation of the
 * rotated-box hot path of Jittor/JDet (reference snapshot 2025-03-10).
 *
 * The reference has no C ABI: every operator below is a `jt.code(...)` call whose C++/CUDA
 * body lives in a Python string (python/jdet/ops/<op>.py).  Each entry point here replaces
 * one such `jt.code` site; the citation on each declaration is the reference call site a
 * maintainer would rebind (see INTEGRATION.md for the ctypes stub).
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes; no framework types.  `stream` is a hipStream_t passed
 *     as void* (NULL = the legacy default stream).
 *   - return 0 on success, a positive hipError_t value if a launch failed, or a negative
 *     JDET_E_* code for argument errors.  Nothing is launched on error.
 *   - asynchronous: no entry point synchronises the device or allocates memory; scratch
 *     comes from the caller (see the *_workspace queries).
 *   - all floating-point tensors are fp32 (the reference is fp32 everywhere); boxes are
 *     [xc, yc, w, h, theta(rad)]; RoIs are [batch, xc, yc, w, h, theta] (rotated) or
 *     [batch, x1, y1, x2, y2] (horizontal).
 *   - inputs are never written; outputs are fully overwritten (backward kernels zero-fill
 *     their accumulation target themselves, as the reference's cudaMemsetAsync does).
 */
#ifndef JDET_HIP_H_
#define JDET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* jdet_stream_t; /* hipStream_t */

#define JDET_OK 0
#define JDET_E_BADARG (-1)   /* null pointer, negative size, unknown enum value        */
#define JDET_E_UNSUPPORTED (-2) /* shape outside what the kernels handle (documented below) */
#define JDET_E_WORKSPACE (-3) /* workspace too small                                     */

/* RoIAlign dialects */
#define JDET_ROI_ROTATED 0    /* ROIAlignRotated     ops/roi_align_rotated.py:L61-127,L165-255    */
#define JDET_ROI_ROTATED_V1 1 /* ROIAlignRotated_v1  ops/roi_align_rotated_v1.py:L71-145,L193-298 */
#define JDET_ROI_RIROI 2      /* RiRoIAlign          ops/riroi_align.py:L70-163,L228-358          */
#define JDET_ROI_HBB_V0 3     /* ROIAlign version=0  ops/roi_align.py:L93-204                     */
#define JDET_ROI_HBB_V1 4     /* ROIAlign version=1  (same file, ROI_ALIGN_VERSION 1)             */

/* Feature-map memory layouts.  NHWC ("channels last") is the native layout of the kernels:
 * one bilinear tap is a contiguous C-vector.  NCHW inputs go through jdet_nchw_to_nhwc. */
#define JDET_LAYOUT_NCHW 0
#define JDET_LAYOUT_NHWC 1

int jdet_version(void);

/* Layout conversion helpers (tiled transposes), x: (N,C,H,W) <-> y: (N,H,W,C). */
int jdet_nchw_to_nhwc(const float* x, int N, int C, int H, int W, float* y, jdet_stream_t stream);
int jdet_nhwc_to_nchw(const float* x, int N, int C, int H, int W, float* y, jdet_stream_t stream);

/* RoIAlign forward.  Replaces the jt.code sites roi_align_rotated.py:L265-283,
 * roi_align_rotated_v1.py:L308-326, riroi_align.py:L425-427, roi_align.py:L217-237.
 *   feat    : (N, C, H, W) values stored NHWC, i.e. feat[((n*H+y)*W+x)*C + c]   [layout NHWC]
 *             C is the TOTAL plane count (RiRoIAlign: C = channels * n_orient).
 *   rois    : (R, 6) rotated dialects, (R, 5) horizontal dialects
 *   out     : (R, C, PH, PW) contiguous (the reference's output layout)
 *   sample_num : >0 fixed grid, <=0 adaptive ceil(roi_size / pooled_size)
 *   n_orient   : RiRoIAlign only (C % n_orient == 0); pass 1 otherwise
 *   order      : optional (R) int32 permutation from jdet_roi_spatial_order, or NULL
 * A RoI whose batch index is negative is skipped: its rows of `out` are left untouched and it adds
 * nothing in backward.  (FPN level routing: call once per level on the SAME `out`, with the batch
 * index of off-level RoIs set to -1 -- no mask / gather / scatter-add round trip and no host sync,
 * cf. oriented_single_level.py:L105-112.)
 * Limits: PH*PW <= 256; any C >= 1 (C % 4 == 0 takes the vector path). */
int jdet_roi_align_forward(int variant, const float* feat_nhwc, int N, int C, int H, int W,
                           const float* rois, int R, int PH, int PW, float spatial_scale,
                           int sample_num, int n_orient, const int32_t* order, float* out,
                           jdet_stream_t stream);

/* RoI-stationary forward (the kernels of jdet_roi_align_forward) with the channels-last result layout
 * out_cl (R, PH, PW, C): each wave stores a bin's channel chunk straight from registers (1 KiB contiguous,
 * non-temporal) instead of transposing the RoI's block through LDS.  Rotated v0 / v1, horizontal v0 / v1 and
 * RiRoIAlign with n_orient 4 or 8 (ignored for the other dialects), C % 4 == 0, any sample_num (<= 0 adaptive);
 * otherwise JDET_E_UNSUPPORTED.  `order` as in jdet_roi_align_forward. */
int jdet_roi_align_forward_cl_roi(int variant, const float* feat_nhwc, int N, int C, int H, int W,
                                  const float* rois, int R, int PH, int PW, float spatial_scale, int sample_num,
                                  int n_orient, const int32_t* order, float* out_cl, jdet_stream_t stream);

/* Forward with the channels-last result out_cl (R, PH, PW, C) and the schedule computed inside; same call sites as
 * jdet_roi_align_forward (roi_align_rotated.py:L265-283, roi_align_rotated_v1.py:L308-326, riroi_align.py:L425-427,
 * roi_align.py:L217-237): jdet_roi_spatial_order (R >= 64) + the kernels of jdet_roi_align_forward_cl_roi.
 * workspace: jdet_roi_align_forward_cl_workspace(R, PH, PW) bytes (8 R + 256 for the schedule), any content, 256-byte
 * aligned; too small a buffer returns JDET_E_WORKSPACE.
 * RoIs with a negative batch index are skipped as in jdet_roi_align_forward. */
size_t jdet_roi_align_forward_cl_workspace(int R, int PH, int PW);
int jdet_roi_align_forward_cl(int variant, const float* feat_nhwc, int N, int C, int H, int W, const float* rois,
                              int R, int PH, int PW, float spatial_scale, int sample_num, int n_orient,
                              float* out_cl, void* workspace, size_t workspace_bytes, jdet_stream_t stream);

/* The reference's OPERATION ORDER (roi_align_rotated.py:L70-118: w1*lt + w2*rt + w3*lb + w4*rb per sample, samples summed
 * iy-major, then / count) behind its own entry points -- same arguments as jdet_roi_align_forward /
 * jdet_roi_align_forward_cl, results bit-identical to the CPU oracle: the parity twin the tests and smoke() call.  The
 * product entry points above merge duplicate taps inside a bin before loading (fewer vector-memory requests; equal to
 * the reference up to fp32 re-association of the bilinear weights, <= 2e-6 on N(0,1) maps).  The library holds no
 * process-wide arithmetic mode. */
int jdet_roi_align_forward_reference(int variant, const float* feat_nhwc, int N, int C, int H, int W,
                                     const float* rois, int R, int PH, int PW, float spatial_scale, int sample_num,
                                     int n_orient, const int32_t* order, float* out, jdet_stream_t stream);
int jdet_roi_align_forward_cl_reference(int variant, const float* feat_nhwc, int N, int C, int H, int W,
                                        const float* rois, int R, int PH, int PW, float spatial_scale, int sample_num,
                                        int n_orient, float* out_cl, void* workspace, size_t workspace_bytes,
                                        jdet_stream_t stream);

/* XCD-aware spatial schedule for the RoIAlign kernels (no reference counterpart: the reference
 * processes output elements in index order).  Writes a permutation `order` of [0,R): workgroup b
 * processes RoI order[b].  RoIs are bucketed by the Morton code of their centre and contiguous
 * runs are dealt to the 8 XCDs so that each XCD's private L2 sweeps one compact region of the
 * map.  Pure performance hint: any permutation (or NULL = identity) gives identical results.
 * `workspace`: R int32 of scratch.  roi_cols 6 (rotated) or 5 (horizontal). */
int jdet_roi_spatial_order(const float* rois, int R, int roi_cols, float spatial_scale, int N,
                           int H, int W, int32_t* order, int32_t* workspace, jdet_stream_t stream);

/* RoIAlign backward w.r.t. the feature map.  Replaces roi_align_rotated.py:L286-307 (and the
 * _v1 / riroi / hbb twins).  grad_in_nhwc (N,H,W,C) is fully overwritten.
 * With a workspace of jdet_roi_align_backward_workspace(...) bytes the scatter is inverted once on the
 * (roi, sample, tap) index space and executed as a sorted GATHER (integer atomics only, one store per
 * pixel); with workspace = NULL, or when the query returns 0 (RiRoIAlign, sample_num <= 0, C % 4 != 0),
 * it is the reference's scheme: zero-fill + hardware fp32 atomics.  Either way the last bits depend on
 * accumulation order, as in the reference.
 * Workspace size: counters and offsets of the 2x2 pixel patches, two record arrays of R * PH * PW * samples * 4 x 32
 * bytes, the (R, PH*PW, C) transposed gradient, and the patches' direct rows (at most 256 MiB; csr_gather.h) -- 268 MB
 * at 2000 RoIs on a 256 x 256 x 256 map.  The size grows monotonically with R, so a buffer sized for the largest R of a
 * map serves every smaller call on it. */
size_t jdet_roi_align_backward_workspace(int variant, int R, int N, int C, int H, int W, int PH, int PW,
                                         int sample_num);
int jdet_roi_align_backward(int variant, const float* grad_out, const float* rois, int R, int N,
                            int C, int H, int W, int PH, int PW, float spatial_scale,
                            int sample_num, int n_orient, const int32_t* order, float* grad_in_nhwc,
                            void* workspace, size_t workspace_bytes, jdet_stream_t stream);

/* Same as jdet_roi_align_backward for a channels-last gradient grad_out_cl (R, PH, PW, C): the sorted gather
 * reads it directly (no (R,C,bin) -> (R,bin,C) transpose pass).  Needs the workspace of
 * jdet_roi_align_backward_workspace(); returns JDET_E_UNSUPPORTED where that query returns 0.
 * workspace_clean != 0: the caller keeps this workspace between calls and guarantees that its first
 * jdet_roi_align_backward_clean_bytes() bytes are zero on entry (zero-fill it once); the call hands them back zeroed
 * (stream order), so no memset launch is needed.  workspace_clean == 0: any content, the call zeroes what it needs. */
size_t jdet_roi_align_backward_clean_bytes(int variant, int R, int N, int C, int H, int W, int PH, int PW,
                                           int sample_num);
int jdet_roi_align_backward_cl(int variant, const float* grad_out_cl, const float* rois, int R, int N, int C,
                               int H, int W, int PH, int PW, float spatial_scale, int sample_num, int n_orient,
                               float* grad_in_nhwc, void* workspace, size_t workspace_bytes, int workspace_clean,
                               jdet_stream_t stream);

/* The PLAN of a backward, separated from the gather (round 6).  jdet_roi_align_backward[_cl] inverts the scatter on every
 * call (a third of its time at the north-star point) although the inversion depends only on the RoIs, the map size and
 * the bin grid -- all known at the forward (ROIAlignBackward's arguments besides the gradient, roi_align_rotated.py:L284-308).
 *   jdet_roi_align_backward_plan       builds the plan into `plan` (jdet_roi_align_backward_plan_bytes() bytes, any
 *                                      content on entry; 0 bytes = shape served by the atomic path only)
 *   jdet_roi_align_backward_cl_planned the gather alone from a channels-last gradient (R, PH, PW, C); the plan is left
 *                                      intact: any number of gathers (any C) per plan.  RiRoIAlign: JDET_E_UNSUPPORTED
 *                                      (its rows need the orientation mix: use jdet_roi_align_backward_cl).
 * Same values as jdet_roi_align_backward_cl (same rows, same order of accumulation). */
size_t jdet_roi_align_backward_plan_bytes(int variant, int R, int N, int H, int W, int PH, int PW, int sample_num);
int jdet_roi_align_backward_plan(int variant, const float* rois, int R, int N, int H, int W, int PH, int PW,
                                 float spatial_scale, int sample_num, void* plan, size_t plan_bytes,
                                 jdet_stream_t stream);
int jdet_roi_align_backward_cl_planned(int variant, const float* grad_out_cl, int R, int N, int C, int H, int W, int PH,
                                       int PW, int sample_num, float* grad_in_nhwc, const void* plan, size_t plan_bytes,
                                       jdet_stream_t stream);

/* Pairwise rotated IoU, ious (n1, n2) row-major.  Replaces box_iou_rotated.py:L507 and
 * box_iou_rotated_v1.py:L512 (the python-side "too small" zeroing L515-523 stays in the
 * host wrapper).  version 0/1 selects the vertex convention; sort_mode 0 reproduces the
 * reference CPU path (std::sort, L316-325), 1 the reference CUDA exchange sort (L338-351).
 * stride = floats per box row (>= 5). */
int jdet_box_iou_rotated(const float* boxes1, int n1, const float* boxes2, int n2, int stride,
                         int version, int sort_mode, float* ious, jdet_stream_t stream);

/* Rotated NMS.  Replaces nms_rotated.py:L497-503 (nms_rotated_cpu) / L506-513 (cuda).
 *   dets (n, box_len) box_len 5, or 6 with a label in column 5 (cross-label IoU := 0, L283-286)
 *   order: int32 visiting order = indices by descending score (the caller's argsort, nms_rotated.py:L519,L532).
 *          With labels (box_len 6) any order that is descending in score INSIDE each label gives the same keep
 *          set; visiting class by class lets the kernel skip every 64x64 tile whose label ranges are disjoint.
 *   cmp_ge 1: suppress when iou >= thr (reference CPU rule L444); 0: iou > thr (CUDA rule L403)
 *   keep : n bytes, 1 = kept, indexed by ORIGINAL detection index
 * Entirely on device: zero fill + tile bitmask kernel + one-workgroup greedy scan, no host synchronisation. */
size_t jdet_nms_rotated_workspace(int n);
int jdet_nms_rotated(const float* dets, int n, int box_len, const int32_t* order,
                     float iou_threshold, int cmp_ge, int sort_mode, uint8_t* keep,
                     void* workspace, size_t workspace_bytes, jdet_stream_t stream);

/* jdet_nms_rotated with two more switches (same workspace, same keep contract).
 * horizontal != 0: the caller promises every angle is 0; the overlap is the rectangle formula
 *   inter / (a + b - inter) instead of polygon clipping (the horizontal proposal NMS of the two-stage RPNs --
 *   `jt.nms`, nms.py:L4-9 -- and of level-offset tricks such as oriented_rpn_head.py:L214-219).
 * n_labels > 1 (box_len 6): the labels are the integers 0 .. n_labels-1 and `order` visits the boxes label by label
 *   (descending score inside a label): each label is scanned by its own workgroup.  n_labels == 1: any labels. */
int jdet_nms_labeled(const float* dets, int n, int box_len, const int32_t* order, float iou_threshold, int cmp_ge,
                     int sort_mode, int horizontal, int n_labels, uint8_t* keep, void* workspace,
                     size_t workspace_bytes, jdet_stream_t stream);

/* Deformable-conv v1 sampling.  Replace dcn_v1.py:L309-338 (im2col), L374-410 (col2im),
 * L340-372 (col2im_coord).  im (B,C,H,W) NCHW; offset (B, dg*2*kh*kw, Ho, Wo) ordered
 * (dy,dx) per tap; col (C*kh*kw, B, Ho, Wo). */
int jdet_deform_im2col(const float* im, const float* offset, int B, int C, int H, int W, int kh,
                       int kw, int pad_h, int pad_w, int stride_h, int stride_w, int dil_h,
                       int dil_w, int deform_groups, float* col, jdet_stream_t stream);
int jdet_deform_col2im(const float* col, const float* offset, int B, int C, int H, int W, int kh,
                       int kw, int pad_h, int pad_w, int stride_h, int stride_w, int dil_h,
                       int dil_w, int deform_groups, float* grad_im, jdet_stream_t stream);
int jdet_deform_col2im_coord(const float* col, const float* im, const float* offset, int B, int C,
                             int H, int W, int kh, int kw, int pad_h, int pad_w, int stride_h,
                             int stride_w, int dil_h, int dil_w, int deform_groups,
                             float* grad_offset, jdet_stream_t stream);

/* Modulated deformable conv (DCN v2) sampling.  Replace modulated_deformable_im2col / _col2im / _col2im_coord of
 * ops/dcn_v2.py:L86-149, L506-558, L560-627.  Layouts as jdet_deform_* plus mask (B, dg*kh*kw, Ho, Wo): the column
 * element, the column gradient and the offset gradient are multiplied by the tap's mask; grad_mask (same shape as
 * mask) = sum over the group's channels of column gradient x unmasked bilinear sample. */
int jdet_modulated_deform_im2col(const float* im, const float* offset, const float* mask, int B, int C, int H,
                                 int W, int kh, int kw, int pad_h, int pad_w, int stride_h, int stride_w, int dil_h,
                                 int dil_w, int deform_groups, float* col, jdet_stream_t stream);
int jdet_modulated_deform_col2im(const float* col, const float* offset, const float* mask, int B, int C, int H,
                                 int W, int kh, int kw, int pad_h, int pad_w, int stride_h, int stride_w, int dil_h,
                                 int dil_w, int deform_groups, float* grad_im, jdet_stream_t stream);
int jdet_modulated_deform_col2im_coord(const float* col, const float* im, const float* offset, const float* mask,
                                       int B, int C, int H, int W, int kh, int kw, int pad_h, int pad_w,
                                       int stride_h, int stride_w, int dil_h, int dil_w, int deform_groups,
                                       float* grad_offset, float* grad_mask, jdet_stream_t stream);

/* Deformable position-sensitive RoI pooling.  Replace DeformablePSROIPoolForwardKernel / ...BackwardAccKernel of
 * ops/dcn_v2.py:L855-932, L1007-1116.  CHANNELS-LAST memory (round 6): input / grad_input (N, H, W, C) with
 * C = output_dim * group_size^2 [the reference: (N,C,H,W)]; rois (R,5) [batch,x1,y1,x2,y2]; trans
 * (R, trans_channels, part, part) or NULL with no_trans; out / top_count / grad_out (R, P, P, output_dim) [the reference's
 * (R, output_dim, P, P) stored channels-last] (top_count = samples counted per bin, consumed by the backward).  One wave
 * per (RoI, bin, class, channel chunk), output channels across the lanes.  The backward zero-fills grad_input and
 * grad_trans (shape of trans); grad_input collects lane-contiguous fp32 atomics, grad_trans two atomics per wave. */
int jdet_deform_psroi_pool_forward(const float* input, const float* rois, const float* trans, int N, int C, int H,
                                   int W, int R, int no_trans, float spatial_scale, int output_dim, int group_size,
                                   int pooled_size, int part_size, int sample_per_part, float trans_std,
                                   int trans_channels, float* out, float* top_count, jdet_stream_t stream);
int jdet_deform_psroi_pool_backward(const float* grad_out, const float* top_count, const float* input,
                                    const float* rois, const float* trans, int N, int C, int H, int W, int R,
                                    int no_trans, float spatial_scale, int output_dim, int group_size,
                                    int pooled_size, int part_size, int sample_per_part, float trans_std,
                                    int trans_channels, float* grad_input, float* grad_trans, jdet_stream_t stream);

/* Channels-last deformable sampling (groups = 1, deform_groups = 1, C % 4 == 0; else JDET_E_UNSUPPORTED).
 * Same arithmetic as jdet_deform_im2col / jdet_deform_col2im (dcn_v1.py:L130-184, L185-241), different
 * layout: x_nhwc (B,H,W,C); offset stays (B, 2*kh*kw, Ho, Wo); cols / grad_cols are
 * (B*Ho*Wo, kh*kw, C) so that  out_nhwc = cols . W^T  and  grad_cols = grad_out_nhwc . W  are plain
 * row-major GEMMs.  col2im is a sorted gather (no fp atomics); workspace size from the _workspace query. */
int jdet_deform_im2col_nhwc(const float* x_nhwc, const float* offset, int B, int C, int H, int W,
                            int kh, int kw, int pad_h, int pad_w, int stride_h, int stride_w,
                            int dil_h, int dil_w, float* cols, jdet_stream_t stream);
size_t jdet_deform_col2im_nhwc_workspace(int B, int C, int H, int W, int kh, int kw, int pad_h,
                                         int pad_w, int stride_h, int stride_w, int dil_h, int dil_w);
int jdet_deform_col2im_nhwc(const float* grad_cols, const float* offset, int B, int C, int H, int W,
                            int kh, int kw, int pad_h, int pad_w, int stride_h, int stride_w,
                            int dil_h, int dil_w, float* grad_x_nhwc, void* workspace,
                            size_t workspace_bytes, jdet_stream_t stream);

/* 3x3 / stride 1 / pad 1 convolution as an fp32-MFMA implicit GEMM, channels-last, with the epilogue of the dense
 * stack fused: replaces nn.Conv(3x3) [+ bias] [+ ReLU] of ConvModule (models/utils/modules.py:L91-175) as the head
 * towers / FPN output convs / the RPN conv use it, and -- with `offset` non-NULL -- the whole DeformConv forward of
 * ops/dcn_v1.py:L412-454 (deformable im2col L130-184 + matmul) without a column matrix.
 * x (N,H,W,Cin); w (Cout,3,3,Cin) [= torch channels_last memory of a (Cout,Cin,3,3) weight]; bias (Cout) or NULL;
 * rowmask (N*H*W) or NULL multiplies the finished output rows (gap rows of a level pack); offset (N,18,H,W) with
 * (dy,dx) per tap or NULL; y (N,H,W,Cout); tile = 0 (chosen from the problem size), 64 or 128 (edge of the
 * workgroup's output tile; + 1 / + 2 select the 16-deep K step / no intra-workgroup K split, for measurements).  Cin % 16 == 0 and 16-byte aligned x / w, else JDET_E_UNSUPPORTED / JDET_E_BADARG
 * (query: jdet_conv3x3_igemm_supported).  Products are fp32 in, fp32 accumulate (v_mfma_f32_32x32x2). */
int jdet_conv3x3_igemm_supported(int Cin, int Cout);
int jdet_conv3x3_igemm_forward(const float* x_nhwc, int N, int H, int W, int Cin, const float* w_krsc, int Cout,
                               const float* bias, int relu, const float* rowmask, const float* offset,
                               int tile, float* y_nhwc, void* workspace, size_t workspace_bytes,
                               jdet_stream_t stream);
/* optional workspace: maps too small to fill the chip with output tiles are split along K over workgroups (partial
 * tiles summed by a second launch that also applies the epilogue) when a workspace of this size is passed; NULL / 0 =
 * single pass.  0 when the shape is not split.  A non-NULL workspace of fewer bytes than the query: JDET_E_WORKSPACE. */
size_t jdet_conv3x3_igemm_workspace(int N, int H, int W, int Cin, int Cout);

/* Weight gradient of the same convolution, ACCUMULATED into gw: gw (Cout,3,3,Cin) += sum over positions of
 * gy (N,H,W,Cout) x the (shifted | bilinearly gathered, offset non-NULL) input x (N,H,W,Cin).  Replaces the weight
 * gradient Jittor derives for nn.Conv inside ConvModule (models/utils/modules.py:L91-175) and DeformConvFunction.grad's
 * im2col + matmul into grad_weight (ops/dcn_v1.py:L508-556).  The reduction over positions is split over workgroups
 * and meets in gw by float atomics, so several calls (the pyramid levels of a shared tower) may target one buffer --
 * the caller zero-fills it once (or passes p.grad).  ksplit = 0 chooses the split.  Cin % 4 == 0, Cout % 4 == 0,
 * 16-byte aligned x / gy, else JDET_E_UNSUPPORTED / JDET_E_BADARG. */
int jdet_conv3x3_wgrad_supported(int Cin, int Cout);
int jdet_conv3x3_wgrad(const float* x_nhwc, const float* gy_nhwc, const float* offset, int N, int H, int W, int Cin,
                       int Cout, float* gw_krsc, int ksplit, jdet_stream_t stream);

/* ---- The ResNet bottleneck convolutions with the layer's neighbours in the epilogue (csrc/conv_bn.hip) -------------
 * Replaces, for Bottleneck.execute (python/jdet/models/backbones/resnet.py:L61-93) and ResNet._make_layer's downsample
 * pair (L131-154) under `norm_eval` (L177-185), the nn.Conv -> nn.BatchNorm(eval) [-> + identity] [-> relu] chains and
 * the gradients Jittor derives for them: forward, data gradient (the same kernel on jdet_conv_dgrad_weights' flipped /
 * transposed weights) and, through jdet_conv_wgrad, the weight gradient.
 *
 * jdet_bn_params_t: an eval-mode BatchNorm as the affine map a = weight * rsqrt(var + eps), sh = bias - mean * a
 *   (weight NULL = 1, bias NULL = 0; var NULL: a = weight, sh = bias, i.e. a plain convolution bias).
 * jdet_conv_epilogue_t.mode:
 *   JDET_EPI_FORWARD  y = [relu]( [affine: acc * a + sh] [+ residual (M, Cout)] )
 *   JDET_EPI_ADD      y = acc + grad_out * [act > 0]        grad_out, act: (M, Cout) -- the identity branch's gradient
 *                                                            joins the data gradient of conv1 (the block's grad_x)
 *   JDET_EPI_MASK     g = acc * [act > 0];  y = g * a;  sums (rows, 2, Cout) non-NULL: partial column sums of g and of
 *                     g * (act - bias), rows = jdet_conv_bn_sums_rows(...) -- `bn` / `act` are the BatchNorm and the
 *                     activation act = relu(bn(conv)) of the layer BELOW: y is the gradient w.r.t. that conv's output */
typedef struct jdet_bn_params {
  const float* weight;
  const float* bias;
  const float* mean;
  const float* var;
  float eps;
} jdet_bn_params_t;

#define JDET_EPI_FORWARD 0
#define JDET_EPI_ADD 1
#define JDET_EPI_MASK 2

typedef struct jdet_conv_epilogue {
  int mode;
  int affine; /* FORWARD: apply bn to the accumulator */
  int relu;   /* FORWARD */
  jdet_bn_params_t bn;
  const float* residual; /* FORWARD */
  const float* grad_out; /* ADD */
  const float* act;      /* ADD, MASK */
  float* sums;           /* MASK */
} jdet_conv_epilogue_t;

/* x (N,H,W,Cin), w (Cout,R,R,Cin), y (N,Ho,Wo,Cout), Ho = (H + 2*(R/2) - R) / stride + 1; R in {1, 3}, stride in
 * {1, 2}, Cin % 16 == 0, 16-byte aligned x / w, positions * channels < 2^30 (else JDET_E_UNSUPPORTED / _BADARG).
 * tile: as jdet_conv3x3_igemm_forward.  workspace (jdet_conv_bn_workspace bytes, optional): small maps split their K
 * steps over workgroups; NULL / 0 bytes = single pass, a non-NULL workspace of fewer bytes than the query with tile 0:
 * JDET_E_WORKSPACE (the single pass writes more rows of `sums`).  jdet_conv_bn_sums_rows: rows of `sums` a MASK launch
 * with these arguments writes (with_workspace: whether a sufficient workspace will be passed). */
int jdet_conv_bn_supported(int Cin, int Cout, int R, int stride);
size_t jdet_conv_bn_workspace(int N, int H, int W, int Cin, int Cout, int R, int stride);
size_t jdet_conv_bn_sums_rows(int N, int H, int W, int Cin, int Cout, int R, int stride, int tile,
                              int with_workspace);
int jdet_conv_bn_forward(const float* x_nhwc, int N, int H, int W, int Cin, const float* w_krsc, int Cout, int R,
                         int stride, const jdet_conv_epilogue_t* epilogue, int tile, float* y_nhwc, void* workspace,
                         size_t workspace_bytes, jdet_stream_t stream);
/* weights of the data gradient for any number of layers in ONE launch: dst (Cin,R,R,Cout)[ci][R*R-1-tap][co] =
 * src (Cout,R,R,Cin)[co][tap][ci].  jobs_device: DEVICE array of njobs 32-byte records {const float* src; float* dst;
 * int Cout, Cin, taps, tile_begin} with tile_begin the running sum of ceil(Cout/32) * ceil(Cin/32) * taps over the
 * preceding jobs; total_tiles = that sum over all jobs. */
int jdet_conv_dgrad_weights(const void* jobs_device, int njobs, int total_tiles, jdet_stream_t stream);
/* weight gradient, ACCUMULATED: gw (Cout,R,R,Cin) += sum over positions of gy (N,Ho,Wo,Cout) x the input window of
 * x (N,H,W,Cin); the general (R, stride) form of jdet_conv3x3_wgrad, same tiling / split / atomics. */
int jdet_conv_wgrad(const float* x_nhwc, const float* gy_nhwc, int N, int H, int W, int Cin, int Cout, int R,
                    int stride, float* gw_krsc, int ksplit, jdet_stream_t stream);
/* Backward of a BatchNorm whose (possibly summed) output went through a ReLU, from the ACTIVATION y (the fused forward
 * stores no conv output c): grad_c = grad_y * [y > 0] * a; sums non-NULL: partial sums (rows, 2, C) of
 * g = grad_y * [y > 0] and g * t, rows = jdet_bn_act_backward_from_output_rows(P, C), where t / gamma = xhat:
 *   t = y - bias (y = relu(bn(c)));  identity != NULL: t = y - identity - bias (y = relu(bn(c) + identity));
 *   own_output != NULL: t = own_output - bias (y = relu(other + bn(c)), own_output = bn(c): the downsample branch).
 * Channel counts as jdet_frozen_bn_act_forward. */
size_t jdet_bn_act_backward_from_output_rows(long P, int C);
int jdet_bn_act_backward_from_output(const float* grad_y_nhwc, const float* y_nhwc, const float* identity_nhwc,
                                     const float* own_output_nhwc, long P, int C, const float* weight,
                                     const float* bias, const float* running_mean, const float* running_var,
                                     float eps, float* grad_c_nhwc, float* sums, size_t sums_bytes,
                                     jdet_stream_t stream);
/* Second stage of such partial sums for up to 4 BatchNorm layers in one launch (deterministic: fixed summation order):
 * grad_beta = column sums of the first halves, grad_gamma = column sums of the second halves / gamma (gamma NULL = 1;
 * a zero gamma gives inf / NaN on purpose -- xhat is not recoverable from the activation then).  jobs: HOST array. */
typedef struct jdet_bn_sums_job {
  const float* partial; /* (rows, 2, C) */
  long rows;
  int C;
  const float* gamma;
  float* grad_gamma;
  float* grad_beta;
} jdet_bn_sums_job_t;
int jdet_bn_sums_finish(const jdet_bn_sums_job_t* jobs, int njobs, jdet_stream_t stream);

/* RepPoints geometry on 9-point sets (pointsets (N,18) = 9 (x,y) pairs) and the Graham scan of the polygon-IoU loss.
 * jdet_convex_iou: replaces convex_iou_kernel (ops/reppoints_convex_iou/convex_iou_kernel.cu:L258-305): IoU of the
 *   convex hull of every point set with every quadrilateral polygons (M,8) -> ious (N,M), computed in double.
 * jdet_min_area_bbox: replaces minareabbox_kernel (ops/reppoints_min_area_bbox/min_area_bbox.cu:L49-203, L301-461):
 *   minimum-area rectangle of the hull -> bboxes (N,8), corners (xmax,ymin) (xmin,ymin) (xmin,ymax) (xmax,ymax) of the
 *   rotated frame.
 * jdet_convex_sort: replaces convex_sort_gpu (ops/convex_sort.py:L4-65, L159-194): pts (nbs,npts,2), masks (nbs,npts)
 *   as float 0/1 -> index (nbs, npts + circular) int32 hull indices in scan order, -1 in unused slots (the kernel
 *   writes every slot); npts <= 64, else JDET_E_UNSUPPORTED. */
int jdet_convex_iou(const float* pointsets, int N, const float* polygons, int M, float* ious, jdet_stream_t stream);

/* RepPoints convex GIoU with its gradient (reppoints_convex_iou/convex_giou.py:L29-47, replaces the jt.code site L37-43
 * around convex_giou_kernel.cu:L725-821): ALIGNED pairs -- pointsets (N, 18), polygons (N, 8) -> out (N, 19):
 * out[n, 0:18] = d giou / d pointsets[n, :] (zero for points that are not hull vertices), out[n, 18] = giou =
 * I/U - (C - U)/C of the hull of the 9 points with the quadrilateral (C: hull of both).  Gradient by forward-mode dual
 * numbers (half a wave per pair, one lane per coordinate), double precision inside like the reference. */
int jdet_convex_giou(const float* pointsets, const float* polygons, int N, float* out, jdet_stream_t stream);
int jdet_min_area_bbox(const float* pointsets, int N, float* bboxes, jdet_stream_t stream);
int jdet_convex_sort(const float* pts, const float* masks, int nbs, int npts, int circular, int32_t* index,
                     jdet_stream_t stream);

/* Sigmoid focal loss, replaces the tensor-op chain of models/losses/focal_loss.py:L5-96 (sigmoid_focal_loss with
 * binary_cross_entropy_with_logits): logits (M, C) row-major, labels (M) int32 (0 = background, k = class k),
 * weight (M) or NULL; alpha < 0 disables the alpha term.  *loss_sum = sum over all M*C elements (the caller divides
 * by avg_factor and applies loss_weight); grad_logits (M, C) = d loss_sum / d logits.  Deterministic. */
size_t jdet_sigmoid_focal_loss_workspace(void);
int jdet_sigmoid_focal_loss(const float* logits, const int32_t* labels, const float* weight, long M, int C,
                            float alpha, float gamma, float* loss_sum, float* grad_logits,
                            void* workspace, size_t workspace_bytes, jdet_stream_t stream);

/* Weighted smooth-L1 / L1 (models/losses/smooth_l1_loss.py:L5-27, l1_loss.py): element-wise over n values,
 * weight same shape or NULL, beta = 0 -> L1.  *loss_sum = sum; grad_pred = d loss_sum / d pred.  Workspace: the
 * focal-loss query.  Deterministic. */
int jdet_smooth_l1_loss(const float* pred, const float* target, const float* weight, long n, float beta,
                        float* loss_sum, float* grad_pred, void* workspace, size_t workspace_bytes,
                        jdet_stream_t stream);

/* The per-level loss call of a dense head as one node (round 6): what models/roi_heads/s2anet_head.py:L430-508
 * (loss_fam_single / loss_odm_single) composes per pyramid level from reshape + loss + `/ avg_factor` + `* loss_weight`
 * (models/losses/focal_loss.py:L50-53, L86-93; smooth_l1_loss.py:L18-22, L47-53).
 *   - labels / weight / target are read through a BLOCKED row index: logical row r is element
 *     (r / rows_per_block) * block_stride + r % rows_per_block (in rows) of the array -- a level's column window
 *     [:, s:e] of the per-image (N, A[, 5]) target arrays is rows_per_block = e - s, block_stride = A, base + s; a
 *     contiguous array is rows_per_block >= M, any stride.  logits / pred and the gradients are contiguous.
 *   - avg_factor: DEVICE scalar; *loss = (sum / *avg_factor) * loss_weight; grad_* = d sum / d input (the UNIT gradient).
 *   - jdet_loss_grad_scale: out[i] = unit_grad[i] * ((*grad_out * loss_weight) / *avg_factor): the backward of the node.
 * Same operations in the same order as the composition: bit-identical to it.  Workspace: the focal-loss query. */
int jdet_sigmoid_focal_loss_level(const float* logits, const int32_t* labels, long label_rows_per_block,
                                  long label_block_stride, const float* weight, long weight_rows_per_block,
                                  long weight_block_stride, long M, int C, float alpha, float gamma,
                                  const float* avg_factor, float loss_weight, float* loss, float* grad_logits,
                                  void* workspace, size_t workspace_bytes, jdet_stream_t stream);
int jdet_smooth_l1_loss_level(const float* pred, const float* target, long target_rows_per_block,
                              long target_block_stride, const float* weight, long weight_rows_per_block,
                              long weight_block_stride, long rows, int E, float beta, const float* avg_factor,
                              float loss_weight, float* loss, float* grad_pred, void* workspace,
                              size_t workspace_bytes, jdet_stream_t stream);
int jdet_loss_grad_scale(const float* unit_grad, long n, const float* grad_out, const float* avg_factor,
                         float loss_weight, float* out, jdet_stream_t stream);

/* Gaussian box losses of one pyramid level as one node (round 7, csrc/gaussian_loss.hip): replaces GDLoss
 * (models/losses/gaussian_dist_loss.py:L48-276), GDLoss_v1 (gaussian_dist_loss_v1.py:L48-156) and KFLoss
 * (kf_iou_loss.py:L48-99) with the decode in front of them (rotated_retina_head.py `reg_decoded_bbox`,
 * kfiou_rotated_retina_head.py:L96-104).  Contract of jdet_smooth_l1_loss_level:
 *   - pred (rows, 5) contiguous DELTAS; target / weight (rows, 5) behind blocked row indices (a level's window of the
 *     per-image (N, A, 5) arrays read in place); weight NULL = every row.  A row counts when weight.mean(-1) > 0; the
 *     weight is a mask only, never a factor (as in the reference).
 *   - anchors (anchor_rows, 5), row r reads anchor r % anchor_rows; needed when decode_pred / decode_target is set.
 *     decode_pred: the Gaussian of the prediction is that of delta2bbox_rotated(anchor, pred) (bit-identical
 *     arithmetic to jdet_delta2bbox_rotated, means / stds / wh_ratio_clip of the params); decode_target: likewise for
 *     the target (KFLoss's targets_decode).  KFIoU's smooth-L1 term always reads the undecoded xy deltas.
 *   - *loss = (sum over counted rows / *avg_factor) * loss_weight; grad_pred = d sum / d pred (unit gradient, zero on
 *     rows that do not count); the backward is jdet_loss_grad_scale.  KFIoU: det(Sigma) <= 0 gives Vb = 0 (the
 *     reference's NaN -> 0) with a zero gradient.  Workspace: the focal-loss query.  Deterministic. */
#define JDET_GD_GWD 0         /* GDLoss    gwd_loss        */
#define JDET_GD_KLD 1         /* GDLoss    kld_loss        */
#define JDET_GD_JD 2          /* GDLoss    jd_loss         */
#define JDET_GD_KLD_SYMMAX 3  /* GDLoss    kld_symmax_loss */
#define JDET_GD_KLD_SYMMIN 4  /* GDLoss    kld_symmin_loss */
#define JDET_GD1_GWD 5        /* GDLoss_v1 gwd_loss        */
#define JDET_GD1_KLD 6        /* GDLoss_v1 kld_loss        */
#define JDET_GD1_BCD 7        /* GDLoss_v1 bcd_loss        */
#define JDET_KFIOU 8          /* KFLoss    kfiou_loss      */
#define JDET_GD_FUN_NONE 0    /* 'none' (GDLoss, KFLoss), '' (GDLoss_v1) */
#define JDET_GD_FUN_LOG1P 1
#define JDET_GD_FUN_SQRT 2
#define JDET_GD_FUN_LN 3      /* KFLoss */
#define JDET_GD_FUN_EXP 4     /* KFLoss */

typedef struct jdet_gaussian_loss_params {
  int kind;            /* JDET_GD_* / JDET_GD1_* / JDET_KFIOU */
  int fun;             /* JDET_GD_FUN_* */
  float tau, alpha;    /* GDLoss / GDLoss_v1 */
  int normalize;       /* GDLoss gwd */
  int sqrt_dist;       /* GDLoss kld, jd, kld_symmax, kld_symmin: the `sqrt` argument */
  float beta, eps;     /* KFLoss */
  int decode_pred, decode_target;
  float means[5], stds[5], wh_ratio_clip;
} jdet_gaussian_loss_params_t;

int jdet_gaussian_loss_level(const float* pred, const float* target, long target_rows_per_block,
                             long target_block_stride, const float* weight, long weight_rows_per_block,
                             long weight_block_stride, const float* anchors, long anchor_rows, long rows,
                             const jdet_gaussian_loss_params_t* params, const float* avg_factor, float loss_weight,
                             float* loss, float* grad_pred, void* workspace, size_t workspace_bytes,
                             jdet_stream_t stream);

/* Head glue as a single pass (csrc/level_pack.hip; round 6).
 * jdet_level_pack_nhwc: the small pyramid levels of a weight-shared tower (S2ANetHead.execute runs its towers per level,
 *   models/roi_heads/s2anet_head.py:L207-252; here they run once on a packed canvas) -- levels[l] (N, h_l, w_l, C)
 *   contiguous DEVICE pointers in a HOST array (NULL = a window of zeros), level_hw / level_place HOST arrays of
 *   (h, w) / (row, col) per level; every word of canvas (N, Hp, Wp, C) is written: the level's value inside its window,
 *   0 in the gaps.  num_levels <= 8, C % 4 == 0.  Also the backward of the unpacking (level gradients -> canvas gradient). */
int jdet_level_pack_nhwc(const float* const* levels, const int32_t* level_hw, const int32_t* level_place, int num_levels,
                         int N, int C, int Hp, int Wp, float* canvas, jdet_stream_t stream);

/* AlignConv.get_offset (models/roi_heads/s2anet_head.py:L676-713): anchors (N, H*W, 5) [xc,yc,w,h,theta] in image
 * coordinates -> offset (N, 2*k*k, H, W), (dy, dx) per tap of the k x k kernel (k odd). */
int jdet_align_conv_offset(const float* anchors, int N, int H, int W, float stride, int kernel_size,
                           float* offset, jdet_stream_t stream);

/* Inference-mode ("frozen statistics") BatchNorm fused with ReLU and the residual add, channels-last.
 * Replaces the nn.BatchNorm (eval) -> (+identity) -> relu chains of the backbone (models/backbones/resnet.py:
 * L33-59 BasicBlock, L61-93 Bottleneck, L177-185 norm_eval) -- framework primitives in the reference, not jt.code.
 *   y = act((x - mean) * rsqrt(var + eps) * weight + bias (+ residual)),  tensors [P = N*H*W][C], C % 4 == 0,
 *   C/4 a divisor of 256 or in (256, 1024]; weight / bias may be NULL (1 / 0); relu: 0 | 1.
 * backward: grad_x always; grad_residual (= masked grad_y) if non-NULL; grad_weight / grad_bias if non-NULL (then
 * x_nhwc and a workspace from the _workspace query are required); y_nhwc is required when relu = 1. */
int jdet_frozen_bn_act_forward(const float* x_nhwc, const float* residual_nhwc, long P, int C,
                               const float* weight, const float* bias, const float* running_mean,
                               const float* running_var, float eps, int relu, float* y_nhwc,
                               jdet_stream_t stream);
size_t jdet_frozen_bn_act_backward_workspace(long P, int C);
int jdet_frozen_bn_act_backward(const float* grad_y_nhwc, const float* y_nhwc, const float* x_nhwc, long P,
                                int C, const float* weight, const float* bias, const float* running_mean,
                                const float* running_var, float eps, int relu, float* grad_x_nhwc,
                                float* grad_residual_nhwc, float* grad_weight, float* grad_bias,
                                void* workspace, size_t workspace_bytes, jdet_stream_t stream);

/* Bias [+ ReLU] backward of a convolution, channels-last rows (P, C): grad_pre = grad_y * [y > 0] when relu != 0
 * (without ReLU the gradient passes unchanged and grad_pre / y may be NULL) and grad_bias (C) = sum over the P rows of
 * grad_pre.  Replaces the threshold-backward + per-channel-sum pair behind nn.Conv(..., bias=True) [+ relu] of
 * ConvModule (models/utils/modules.py:L91-175): one pass, deterministic two-stage sum.  Workspace:
 * jdet_frozen_bn_act_backward_workspace(P, C); C % 4 == 0 and the same channel counts as the BN kernels. */
int jdet_bias_act_backward(const float* grad_y_nhwc, const float* y_nhwc, long P, int C, int relu,
                           float* grad_pre_nhwc, float* grad_bias, void* workspace, size_t workspace_bytes,
                           jdet_stream_t stream);

/* Per-channel sum over the P rows of a channels-last (P, C) tensor for ANY 1 <= C <= 256: the bias gradient of a
 * convolution WITHOUT an activation whose channel count jdet_bias_act_backward does not take (the 15- and 5-channel
 * output convs of the heads, ConvModule, models/utils/modules.py:L91-175).  Deterministic two-stage sum; workspace:
 * jdet_channel_sum_workspace(P, C) bytes (0 = unsupported). */
size_t jdet_channel_sum_workspace(long P, int C);
int jdet_channel_sum(const float* x_nhwc, long P, int C, float* sums, void* workspace, size_t workspace_bytes,
                     jdet_stream_t stream);

/* Graph-safe forms of two framework operations (csrc/graph_safe.hip): plain kernels where the framework records a memset
 * node into a captured step (memset nodes do not reliably re-execute on replay on this stack).
 *   jdet_zero_fill   : bytes % 4 == 0, p 4-byte aligned (`tensor.zero_()` / `torch.zeros` of a large tensor)
 *   jdet_sum_squares : out[0] = sum x[i]^2 (take_sqrt: its square root = the 2-norm) of a 16-byte aligned fp32 buffer --
 *                      the gradient norm of the clip in optims/optimizer.py:L26-36 (SGD.pre_step); float64 accumulation in
 *                      a fixed order over at most 1024 partial sums (bitwise reproducible); workspace:
 *                      jdet_sum_squares_workspace() bytes, 8-byte aligned, any content. */
int jdet_zero_fill(void* p, size_t bytes, jdet_stream_t stream);
/* Post-capture pass over a hipGraph_t that has NOT been instantiated yet: every memset node (the framework's reduction
 * semaphores, the convolution library's zero fills of atomically adding solvers -- whichever its benchmark picked at
 * capture time) becomes a kernel node with the same destination, pattern, extent, dependencies and dependents.
 * *n_replaced (optional): how many.  Runner's graph mode runs it on every captured step (keep_graph capture). */
int jdet_graph_replace_memset_nodes(void* hip_graph, int* n_replaced);
size_t jdet_sum_squares_workspace(void);
int jdet_sum_squares(const float* x, size_t n, int take_sqrt, float* out, void* workspace, size_t workspace_bytes,
                     jdet_stream_t stream);

/* Active rotating filter.  Replace orn.py:L260-269 (arf_forward) and L271-281 (arf_backward).
 * weight (nOut,nIn,nOri,kH,kW); indices (nOri,kH,kW,nRot) uint8 1-based;
 * out (nOut*nRot, nIn*nOri, kH, kW). */
int jdet_arf_forward(const float* weight, const uint8_t* indices, int nOut, int nIn, int nOri,
                     int kH, int kW, int nRot, float* out, jdet_stream_t stream);
int jdet_arf_backward(const uint8_t* indices, const float* grad_out, int nOut, int nIn, int nOri,
                      int kH, int kW, int nRot, float* grad_weight, jdet_stream_t stream);
/* the same with the expanded bank in channels-last memory (nOut*nRot, kH, kW, nIn*nOri): the layout the channels-last
 * convolution reads (the library otherwise converts the bank inside every forward / gradient call) */
int jdet_arf_forward_cl(const float* weight, const uint8_t* indices, int nOut, int nIn, int nOri, int kH, int kW,
                        int nRot, float* out_cl, jdet_stream_t stream);
int jdet_arf_backward_cl(const uint8_t* indices, const float* grad_out_cl, int nOut, int nIn, int nOri, int kH, int kW,
                         int nRot, float* grad_weight, jdet_stream_t stream);

/* RotationInvariantPooling (orn.py:L595-618: `x.view(N, -1, nOrientation, h, w).max(2)`) on channels-last rows:
 * x (P, C) with C = groups * nO (nO 4 or 8), y (P, groups) = max over each group's nO orientation channels; backward
 * = the gradient autograd derives for that maximum (to the channels equal to it, split evenly among ties). */
int jdet_rip_forward(const float* x_nhwc, long P, int C, int nO, float* y_nhwc, jdet_stream_t stream);
int jdet_rip_backward(const float* x_nhwc, const float* y_nhwc, const float* grad_y_nhwc, long P, int C, int nO,
                      float* grad_x_nhwc, jdet_stream_t stream);

/* Rotated box delta codec (fused elementwise).  Replace the Jittor tensor programs
 * models/boxes/box_ops.py:L229-285 (delta2bbox_rotated: rois (n,5), deltas (n, ncls*5) -> out
 * (n, ncls*5); max_shape / clip_border are accepted by the reference but never applied) and
 * box_ops.py:L180-226 (bbox2delta_rotated: proposals (n,5), gt (n,5) -> (n,5)).
 * means5 / stds5 are HOST pointers to 5 floats.  norm_angle is the floor-mod form L176-178. */
int jdet_delta2bbox_rotated(const float* rois, const float* deltas, int n, int ncls,
                            const float* means5, const float* stds5, float wh_ratio_clip, float* out,
                            jdet_stream_t stream);
int jdet_bbox2delta_rotated(const float* proposals, const float* gt, int n, const float* means5,
                            const float* stds5, float* out, jdet_stream_t stream);

/* Box codecs of the Oriented R-CNN path, one fused launch each.  Replace the Jittor tensor programs
 * models/boxes/coder.py:L332-437 (MidpointOffsetCoder: horizontal anchor (n,4) <-> 6 deltas (dx, dy, dw, dh, da,
 * db) of a rotated box given by its enclosing box and the offsets of its top-most / right-most vertex; decode
 * rebuilds the parallelogram, stretches it to a rectangle and returns the regularised obb (n,5)) and L449-518
 * (OrientedDeltaXYWHTCoder: rotated RoI (n,5) <-> 5 deltas in the RoI's frame, the angle delta taken as the
 * smaller of dtheta / dtheta + pi/2 with a w <-> h swap; decode is class-wise: deltas (n, ncls*5) -> (n, ncls*5)),
 * with obb2hbb / obb2poly / rectpoly2obb / regular_theta / regular_obb of ops/bbox_transforms.py:L499-517,L575-646
 * inlined.  `max_shape` is accepted and ignored by the reference's decoders, so it is not a parameter here.
 * means / stds are HOST pointers (6 resp. 5 floats). */
int jdet_midpoint_offset_decode(const float* anchors_hbb, const float* deltas, long n, const float* means6,
                                const float* stds6, float wh_ratio_clip, float* out_obb, jdet_stream_t stream);
int jdet_midpoint_offset_encode(const float* anchors_hbb, const float* gt_obb, long n, const float* means6,
                                const float* stds6, float* out6, jdet_stream_t stream);
int jdet_oriented_delta_decode(const float* rois, const float* deltas, long n, int ncls, const float* means5,
                               const float* stds5, float wh_ratio_clip, float* out, jdet_stream_t stream);
int jdet_oriented_delta_encode(const float* rois, const float* gt, long n, const float* means5, const float* stds5,
                               float* out, jdet_stream_t stream);

/* Box codecs of the Gliding Vertex detector, one fused launch each (csrc/box_codec_gliding.hip).  Replace the Jittor
 * tensor programs models/boxes/coder.py:L148-205 (GVFixCoder), L213-228 (GVRatioCoder), L242-320
 * (GVDeltaXYWHBBoxCoder) and the target / decode passes of models/roi_heads/gliding_head.py:L287-325, L355-379.
 *   jdet_gliding_targets: rois (n,4) horizontal, gt polygons (n,8) -> bbox_targets (n,4) = delta encode of the roi
 *     against poly2hbb(poly), fix_targets (n,4) = (dt, dr, dd, dl), all 1 on the rows the reference's h_mask marks,
 *     ratio_targets (n,1) = |shoelace area| / area of the enclosing box.  Ties between extreme vertices resolve to the
 *     lowest vertex index (this project's rule: Jittor's argmax tie order is not in the reference tree).
 *   jdet_gliding_decode: per (row, class): delta decode of bbox_pred (n, 4*ncls) with the clamp to (max_h, max_w)
 *     [<= 0: no clamp], GVFixCoder.decode with fix_pred (n, 4*ncls), the box itself (hbb2poly) where ratio_pred
 *     (n, ncls) > ratio_thr, every (x, y) divided by scale4 = (sx, sy, sx, sy) -> polys (n, 8*ncls).
 *   jdet_gv_delta_encode / _decode: the horizontal delta codec alone (the RPN encodes against horizontal gts);
 *     decode is class-wise: deltas (n, 4*ncls) -> (n, 4*ncls).
 * means4 / stds4 / scale4 are HOST pointers to 4 floats.  n == 0: no-op. */
int jdet_gliding_targets(const float* rois_hbb, const float* gt_polys, long n, const float* means4, const float* stds4,
                         float* bbox_targets, float* fix_targets, float* ratio_targets, jdet_stream_t stream);
int jdet_gliding_decode(const float* rois_hbb, const float* bbox_pred, const float* fix_pred, const float* ratio_pred,
                        long n, int ncls, const float* means4, const float* stds4, float wh_ratio_clip, float max_h,
                        float max_w, float ratio_thr, const float* scale4, float* out_polys, jdet_stream_t stream);
int jdet_gv_delta_encode(const float* rois_hbb, const float* gt_hbb, long n, const float* means4, const float* stds4,
                         float* out4, jdet_stream_t stream);
int jdet_gv_delta_decode(const float* rois_hbb, const float* deltas, long n, int ncls, const float* means4,
                         const float* stds4, float wh_ratio_clip, float max_h, float max_w, float* out,
                         jdet_stream_t stream);

/* Dense anchor targets: replaces the index-list scatter of anchor_target_single
 * (models/boxes/anchor_target.py:L137-168) for the PseudoSampler case.  gt_inds (A) is the assigner's
 * output (0 negative, -1 ignored, i+1 = gt i); every anchor gets label (gt_labels[i] or 1 when gt_labels is
 * NULL; 0 otherwise), label weight (pos_weight / 1 / 0), encoded target (bbox2delta_rotated arithmetic, zeros
 * for non-positives) and box weight (1 / 0).  *num_pos (device, zeroed by the caller) += number of positives.
 * means5 / stds5 are HOST pointers. */
int jdet_anchor_targets_rotated(const float* anchors, const float* gt, const int32_t* gt_labels,
                                const int32_t* gt_inds, int A, int K, const float* means5,
                                const float* stds5, float pos_weight, int32_t* labels,
                                float* label_weights, float* bbox_targets, float* bbox_weights,
                                int32_t* num_pos, jdet_stream_t stream);
/* The same for `reg_decoded_bbox=True` (anchor_target.py:L79-80): the box target of a positive anchor is its assigned
 * gt box itself (a copy), zeros elsewhere; labels, label weights, box weights and *num_pos as above.  Lets the dense
 * (sync-free, fixed-shape) target path serve the decoded-box losses (round 7). */
int jdet_anchor_targets_rotated_boxes(const float* gt, const int32_t* gt_labels, const int32_t* gt_inds, int A, int K,
                                      float pos_weight, int32_t* labels, float* label_weights, float* bbox_targets,
                                      float* bbox_weights, int32_t* num_pos, jdet_stream_t stream);

/* FakeBboxOverlaps2D_rotated's conversion (models/boxes/iou_calculator.py:L108-110): out (n, 5) =
 * hbb2obb(obb2hbb(boxes)) (ops/bbox_transforms.py:L639-645, L653-665) -- the enclosing horizontal box as an OBB,
 * (w, h, 0) when w >= h else (h, w, -pi/2); boxes (n, stride >= 5) rows, n = 0: no-op whatever the stride.  One
 * launch (round 7). */
int jdet_obb2hbb2obb(const float* boxes, int n, int stride, float* out, jdet_stream_t stream);

/* MaxIoUAssigner.assign_wrt_overlaps (models/boxes/assigner.py:L160-219) in two launches, no host
 * sync (the reference loops over gts in Python with a masked store per gt and jt.sync_all()).
 *   overlaps (K, A) row-major, gts are rows (assigner.py:L143)
 *   negatives: neg_iou_lo <= max < neg_iou_hi (float threshold: lo = 0)
 *   gt_labels (K) int32 or NULL; labels (A) int32 or NULL; labels_filled = assigned_labels_filled
 *   out: gt_inds (A) int32 in {-1, 0, 1..K}, max_overlaps (A), labels (A)
 * Column argmax ties resolve to the first gt (Jittor's tie rule is unpinned). */
/* Top-down step of the FPN (necks/fpn.py:L160-171: `laterals[i-1] += nn.interpolate(laterals[i], mode="nearest")`, then
 * `/= upsample_div_factor`) as one pass over channels-last maps: out = (lateral + nearest_upsample(top)) / div_factor.
 *   lateral / out (N, H, W, C), top (N, Ht, Wt, C) float32, 16-byte aligned, C % 4 == 0 (else JDET_E_UNSUPPORTED)
 *   nearest rule: src = min(floor(dst * in / out), in - 1) in float32 (= dst >> 1 for an exact 2x)
 * backward: grad_top = sum of grad_out over the pre-image of every coarse pixel, / div_factor (the gradient of `lateral` is
 * grad_out / div_factor itself: no launch). */
int jdet_upsample_add_nhwc_forward(const float* lateral, const float* top, int N, int C, int H, int W, int Ht, int Wt,
                                   float div_factor, float* out, jdet_stream_t stream);
int jdet_upsample_add_nhwc_backward(const float* grad_out, int N, int C, int H, int W, int Ht, int Wt, float div_factor,
                                    float* grad_top, jdet_stream_t stream);

/* Input pipeline on the device: uint8 batch (N, Hs, Ws, 3) -> float32 (N, Hs, Ws, 3) = channels-last memory of a
 * (N, 3, Hs, Ws) tensor, (v - mean[c]) / std[c] with the optional channel reversal first (`Normalize`,
 * data/transforms.py:L467-487), zeros outside each image's valid_hw[n] = (height, width) (`collate_batch`,
 * data/custom.py:L90-106).  mean3 / std3 are HOST pointers indexed by output channel.  Bit-identical to the host
 * arithmetic; a quarter of the PCIe bytes. */
int jdet_normalize_u8_nhwc(const uint8_t* src_nhwc, const int32_t* valid_hw, int N, int Hs, int Ws,
                           const float* mean3, const float* std3, int swap_rb, float* dst_nhwc, jdet_stream_t stream);

/* Feature refinement of R3Det, replaces fr.py:L113-159 (forward) and L161-242 (backward, 1 + 4 * points float
 * atomics per scalar there; a sorted gather here).  feat / out / grads: (N, H, W, C) channels-last, C % 4 == 0;
 * boxes (N, H, W, 5) [x_ctr, y_ctr, w, h, angle]: out = feat + sum over the `points` (1: centre; 5: centre + the four
 * corners) of the bilinear sample of feat at that point, with the reference's coordinate convention (box column 0
 * is used as the row coordinate, fr.py:L134-135). */
int jdet_feature_refine_forward(const float* feat_nhwc, const float* boxes, int N, int C, int H, int W,
                                float spatial_scale, int points, float* out_nhwc, jdet_stream_t stream);
size_t jdet_feature_refine_backward_workspace(int N, int C, int H, int W, int points);
int jdet_feature_refine_backward(const float* grad_out_nhwc, const float* boxes, int N, int C, int H, int W,
                                 float spatial_scale, int points, float* grad_in_nhwc, void* workspace,
                                 size_t workspace_bytes, jdet_stream_t stream);

/* Polygon (4-point) IoU matrix ious (n1, n2) and polygon NMS.  Replaces nms_poly.py: `devPolyIoU` L113-133 /
 * `poly_nms` L187-232 / `multiclass_poly_nms` L234-245 and the per-pair CPU `iou_poly` L247-252 of the DOTA
 * evaluation and tile merging.  polys rows: x1 y1 .. x4 y4 (stride >= 8 floats), any orientation, convex or not.
 * mode 0: the kernel's degenerate rule (union == 0 -> 1), mode 1: iou_poly's (inter / max(union, 0.01)).
 * jdet_nms_poly: rows of row_len 8, or 9 with a label in column 8 (different labels never suppress each other;
 * n_labels > 1: labels are 0 .. n_labels-1 and `order` visits them label by label -- one scan workgroup each);
 * suppression at IoU > thr; keep (n) uint8 over original indices; workspace = jdet_nms_rotated_workspace(n). */
int jdet_poly_iou(const float* polys1, int n1, int stride1, const float* polys2, int n2, int stride2, int mode,
                  float* ious, jdet_stream_t stream);
int jdet_nms_poly(const float* polys, int n, int row_len, const int32_t* order, float iou_threshold, int n_labels,
                  uint8_t* keep, void* workspace, size_t workspace_bytes, jdet_stream_t stream);

/* Axis-aligned overlaps out (K, A) row-major of K gt boxes (K,4) against A boxes (A, box_stride >= 4; the first four
 * columns are x1,y1,x2,y2): the tensor program of `bbox_overlaps` (models/boxes/iou_calculator.py:L235-350, modes
 * "iou" (iof = 0) and "iof" (iof = 1), not aligned) in the same operation order, one launch.  plus_one: the legacy
 * +1 pixel convention (BboxOverlaps2D_v1).  alive (A) or NULL: columns of boxes with alive == 0 are -1. */
int jdet_bbox_overlaps_hbb(const float* gts, int K, const float* boxes, int A, int box_stride, int iof, int plus_one,
                           float eps, const uint8_t* alive, float* out, jdet_stream_t stream);

size_t jdet_assign_max_iou_workspace(int K);
int jdet_assign_max_iou(const float* overlaps, int K, int A, float pos_iou_thr, float neg_iou_lo,
                        float neg_iou_hi, float min_pos_iou, int match_low_quality,
                        int gt_max_assign_all, const int32_t* gt_labels, int labels_filled,
                        int32_t* gt_inds, float* max_overlaps, int32_t* labels, void* workspace,
                        size_t workspace_bytes, jdet_stream_t stream);

/* ---- The ATSS assigner (csrc/atss_assign.hip) -------------------------------------------------------------------- */
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

/* ---- The row-sparse convolution gradients (csrc/conv_rows.hip) ------------------------------------------------------
 * What they are for: the regression towers of the S2ANet head (models/roi_heads/s2anet_head.py:L127-205) are trained by
 * a smooth-L1 loss whose weight is zero for every anchor that is not positive, so the gradient entering their 3x3
 * convolutions is exactly zero on almost every position row.  The three entry points below compute the same data and
 * weight gradients as the dense kernels from the non-zero rows only.  No value is read back to the host and no launch
 * shape depends on device data: the capacity of every list is P = N*H*W rows, so there is no overflow path, and a
 * fully dense gradient is computed correctly (only slower than by the dense kernels).
 */
/* The non-zero rows of a channels-last gradient g (N,H,W,C) = (P, C), in three launches.  Comes before the two
 * entry points below in place of nothing the reference has: Jittor's autograd runs the dense gradients.
 *   flags         (P) bytes, every one written: 1 where any element of the row has (bits & 0x7fffffff) != 0 -- rows
 *                 holding a NaN or an Inf are kept, rows of +0 / -0 are dropped -- else 0
 *   rows          (P) int32: the flagged positions in ASCENDING order in the entries [0, counts[0]), -1 in the rest
 *   rows_dilated  (P) int32: ascending positions whose 3x3 neighbourhood (n, y + dy, x + dx), taken inside the same
 *                 image -- never across a row end or an image boundary -- holds a flagged row, in the entries
 *                 [0, counts[1]), -1 in the rest
 *   counts        2 int32: the two list lengths
 * C % 4 == 0, P * C < 2^30, g 16-byte aligned, else JDET_E_UNSUPPORTED / JDET_E_BADARG.  workspace:
 * jdet_rows_nonzero_workspace(N, H, W) bytes, 4-byte aligned, may hold anything; fewer bytes: JDET_E_WORKSPACE. */
size_t jdet_rows_nonzero_workspace(int N, int H, int W);
int jdet_rows_nonzero(const float* g_nhwc, int N, int H, int W, int C, uint8_t* flags, int32_t* rows,
                      int32_t* rows_dilated, int32_t* counts, void* workspace, size_t workspace_bytes,
                      jdet_stream_t stream);

/* Cin % 4 == 0 and Cout % 16 == 0: what both gradient entry points below take (else JDET_E_UNSUPPORTED). */
int jdet_conv3x3_rows_supported(int Cin, int Cout);

/* gw (Cout,3,3,Cin) += sum over the listed positions r of gy[r, co] * x[nbr(r, tap), ci]; neighbours outside the
 * image contribute zero.  Replaces jdet_conv3x3_wgrad (plain form) where gy is zero outside rows[0 .. *count): the
 * same tiles, fragments and float atomics with the K index taken from the list, so several calls may target one
 * buffer exactly as there.  rows / count: device pointers (jdet_rows_nonzero's `rows` and `counts`); entries past
 * *count are not read; *count == 0 adds nothing.  The grid is fixed by the channel counts; (P + 16) * max(Cin, Cout)
 * < 2^30 and 16-byte aligned x / gy, else JDET_E_UNSUPPORTED / JDET_E_BADARG. */
int jdet_conv3x3_wgrad_rows_workers(int Cin, int Cout); /* K workers per tile: at most this many partial sums are added
                                                           to one element of gw per call (0: unsupported channels) */
int jdet_conv3x3_wgrad_rows(const float* x_nhwc, const float* gy_nhwc, const int32_t* rows, const int32_t* count,
                            int N, int H, int W, int Cin, int Cout, float* gw_krsc, jdet_stream_t stream);

/* gx[r, ci] = sum over taps and co of gy[nbr(r, tap), co] * wd[ci, tap, co] for every r of the list; rows of gx that
 * are not listed are left alone, or -- zero_first != 0 -- zero-filled by a launch of this call, so that gx
 * (N,H,W,Cin) is fully written.  Replaces the library's dense data gradient (convolution_backward, igemm_bwd_*) where
 * gy is zero outside the rows whose dilation the list is (jdet_rows_nonzero's `rows_dilated`, `counts + 1`).  wd
 * (Cin,3,3,Cout): the flipped weights jdet_conv_dgrad_weights writes.  The grid is fixed by P (P / 64 row tiles);
 * tiles past *count leave at once.  P * max(Cin, Cout) < 2^30, 16-byte aligned gy / wd, else JDET_E_UNSUPPORTED /
 * JDET_E_BADARG. */
int jdet_conv3x3_dgrad_rows(const float* gy_nhwc, const float* wd_crsk, const int32_t* rows, const int32_t* count,
                            int N, int H, int W, int Cin, int Cout, int zero_first, float* gx_nhwc,
                            jdet_stream_t stream);

/* ---- The row-sparse convolution forward (csrc/conv_rows.hip) --------------------------------------------------------
 * What they are for: in training, the output of the S2ANet head's ODM regression tower (models/roi_heads/
 * s2anet_head.py:L127-205, odm_reg_convs -> odm_reg) is read by the smooth-L1 loss only, and that loss weighs every
 * anchor that is not positive with 0 (L300-340).  With S0 the positive position rows, the 3x3 prediction layer needs its
 * input on the 3x3 dilation of S0 and the tower layer before it on the dilation of that: the two entry points below
 * make those lists from a flag byte per position and compute conv + bias + ReLU on the listed rows only.  No value is
 * read back to the host and no launch shape depends on device data: every list has capacity P = N*H*W rows, so there is
 * no overflow path, and a dense list is computed correctly (only slower than by the dense kernel).
 */
/* Three ascending row lists from one flag byte per position (non-zero = listed), in four launches (the dilation and
 * list kernels of jdet_rows_nonzero).  Comes in place of nothing the reference has.
 *   flags          (P) bytes, read only
 *   rows           (P) int32: the flagged positions, ascending, in [0, counts[0]); -1 in the rest
 *   rows_dilated   (P) int32: the positions whose 3x3 neighbourhood (n, y + dy, x + dx), taken inside the same image --
 *                  never across a row end or an image boundary -- holds a flagged one, in [0, counts[1]); -1 in the rest
 *   rows_dilated2  (P) int32: the same dilation applied to rows_dilated's set, in [0, counts[2]); -1 in the rest
 *   counts         3 int32: the three list lengths
 * P < 2^30, else JDET_E_UNSUPPORTED.  workspace: jdet_rows_from_flags_workspace(N, H, W) bytes, 4-byte aligned, may
 * hold anything; fewer bytes: JDET_E_WORKSPACE. */
size_t jdet_rows_from_flags_workspace(int N, int H, int W);
int jdet_rows_from_flags(const uint8_t* flags, int N, int H, int W, int32_t* rows, int32_t* rows_dilated,
                         int32_t* rows_dilated2, int32_t* counts, void* workspace, size_t workspace_bytes,
                         jdet_stream_t stream);

/* Cin % 16 == 0 and Cout % 16 == 0: what the entry point below takes (else JDET_E_UNSUPPORTED). */
int jdet_conv3x3_rows_forward_supported(int Cin, int Cout);

/* y[r, co] = [relu](sum over taps and ci of x[nbr(r, tap), ci] * w[co, tap, ci] + bias[co]) * rowmask[r] for every r
 * of the list: 3x3 / stride 1 / pad 1, neighbours outside the image contribute zero.  Replaces
 * jdet_conv3x3_igemm_forward (plain form) where only the listed rows of y are read: w (Cout,3,3,Cin), bias (Cout) or
 * null, rowmask (P) or null with that entry point's meaning (a listed row whose mask is 0 is written as 0).  Rows of y
 * that are not listed are left alone, or -- zero_first != 0 -- zero-filled by a launch of this call, so that y
 * (N,H,W,Cout) is fully written.  rows / count: device pointers (a list of jdet_rows_from_flags and its count);
 * entries past *count are not read; *count == 0 computes nothing.  The grid is fixed by P (P / 64 row tiles); tiles past
 * *count leave at once.  It is the tile of jdet_conv3x3_dgrad_rows with conv_igemm.hip's epilogue.
 * P * max(Cin, Cout) < 2^30, 16-byte aligned x / w, else JDET_E_UNSUPPORTED / JDET_E_BADARG. */
int jdet_conv3x3_rows_forward(const float* x_nhwc, const float* w_krsc, const float* bias, int relu,
                              const float* rowmask, const int32_t* rows, const int32_t* count, int N, int H, int W,
                              int Cin, int Cout, int zero_first, float* y_nhwc, jdet_stream_t stream);

/* ---- Rotated FCOS: point targets and the polygon IoU loss (csrc/fcos_targets.hip, csrc/poly_iou_loss.hip) -------- */
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

/* ---- Rotated RepPoints: point assigner, dense convex GIoU loss (csrc/convex_point_assign.hip, convex_giou_loss.hip) */
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

/* ---- H2RBox: the rotated second view and the view-consistency loss (csrc/rotate_crop.hip, h2rbox_aug_loss.hip) ---- */
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

/* ---- Localization distillation (csrc/dist_loss.hip) -----------------------------------------------------------------
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

/* ---- The 3x3 convolution forward on bf16 MFMA through an exact three-way fp32 split (csrc/conv_bf16x3.hip) ----------
 * Numerics: every fp32 input and weight x is split by truncation into three bf16 values a1 + a2 + a3 == x (exactly);
 * six bf16 products per operand pair (a3b1, a1b3, a2b2, a2b1, a1b2, a1b1, small terms first within a 16-deep K block)
 * go into one fp32 accumulator per output.  The result is as close to the exact sum as an fp32 fma chain's (the bound of
 * jdet_conv3x3_igemm_forward's tests holds with the same headroom), but not bit-equal to that kernel's.  Non-finite
 * inputs give non-finite outputs, possibly NaN where jdet_conv3x3_igemm_forward gives Inf (Inf splits into Inf, NaN, NaN).
 */
/* Cin % 32 == 0, any Cout > 0: what the entry point below takes (else JDET_E_UNSUPPORTED). */
int jdet_conv3x3_bf16x3_supported(int Cin, int Cout);

/* y[m, co] = [relu](sum over taps and ci of x[nbr(m, tap), ci] * w[co, tap, ci] + bias[co]) * rowmask[m]: 3x3 / stride 1 /
 * pad 1, channels last, neighbours outside the image contribute zero.  The plain form of jdet_conv3x3_igemm_forward
 * with that entry point's arguments: x (N,H,W,Cin), w (Cout,3,3,Cin), bias (Cout) or null, rowmask (N*H*W) or null, y
 * (N,H,W,Cout), every element written.  One launch of 128 x 128 output tiles, no workspace, nothing read back, no launch
 * shape taken from device data.  N == 0 is a no-op.  x and w 16-byte aligned, y 4-byte aligned (else JDET_E_BADARG);
 * N*H*W * max(Cin, Cout) < 2^30 and Cout * 9 * Cin < 2^30 (else JDET_E_UNSUPPORTED). */
int jdet_conv3x3_bf16x3_forward(const float* x_nhwc, int N, int H, int W, int Cin, const float* w_krsc, int Cout,
                                const float* bias, int relu, const float* rowmask, float* y_nhwc, jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_H_ */
