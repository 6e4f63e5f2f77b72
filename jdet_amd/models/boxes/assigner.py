"""Max-IoU and ATSS assignment.  Mirrors python/jdet/models/boxes/assigner.py: `AssignResult` L53-65,
`MaxIoUAssigner` L67-219, `MaxIoUAssignerRbbox` L222-274, `ATSSAssignerRbbox` L276-391, `ConvexAssigner` L393-548,
`MaxConvexIoUAssigner` L550-611.

`assign_wrt_overlaps` is the reference's four steps (default -1; negatives; positives; low-quality
matches, later gts overwriting earlier ones) executed as two device launches without a host sync
(csrc/box_codec_assign.hip) instead of the reference's per-gt Python loop with `jt.sync_all()`.  `ATSSAssignerRbbox.assign` is one fused entry
point (csrc/atss_assign.hip, three launches) that evaluates the K x (levels x topk) candidate pairs only.
`ConvexAssigner.assign` is one fused entry point too (csrc/convex_point_assign.hip, three launches for a whole batch)
instead of the reference's host loop over the gts.
"""
import math

import torch

from jdet_amd import _lib as L
from jdet_amd.utils.registry import BOXES, build_from_cfg


class AssignResult:
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts = num_gts
        self.gt_inds = gt_inds
        self.max_overlaps = max_overlaps
        self.labels = labels

    def add_gt_(self, gt_labels):
        self_inds = torch.arange(1, len(gt_labels) + 1, dtype=self.gt_inds.dtype, device=self.gt_inds.device)
        self.gt_inds = torch.cat([self_inds, self.gt_inds])
        self.max_overlaps = torch.cat([self.max_overlaps.new_ones((self.num_gts,)), self.max_overlaps])
        if self.labels is not None:
            self.labels = torch.cat([gt_labels.to(self.labels.dtype), self.labels])


def assign_wrt_overlaps_device(overlaps, pos_iou_thr, neg_iou_thr, min_pos_iou, match_low_quality,
                               gt_max_assign_all, gt_labels, labels_filled):
    """overlaps (K,A) on a HIP device -> (gt_inds int32 (A), max_overlaps (A), labels int32 (A) | None)"""
    L.need_device(overlaps)
    ov = L.f32c(overlaps)
    K, A = ov.shape
    if isinstance(neg_iou_thr, float):
        lo, hi = 0.0, neg_iou_thr
    elif isinstance(neg_iou_thr, tuple):
        assert len(neg_iou_thr) == 2
        lo, hi = float(neg_iou_thr[0]), float(neg_iou_thr[1])
    else:  # neither branch of assigner.py:L187-193 fires: no negatives
        lo, hi = math.inf, -math.inf
    gt_inds = torch.empty((A,), dtype=torch.int32, device=ov.device)
    max_ov = torch.empty((A,), dtype=torch.float32, device=ov.device)
    labels = torch.empty((A,), dtype=torch.int32, device=ov.device) if gt_labels is not None else None
    gl = gt_labels.to(torch.int32).contiguous() if gt_labels is not None else None
    wsb = L.lib().jdet_assign_max_iou_workspace(K)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=ov.device)
    L.check(L.lib().jdet_assign_max_iou(L.ptr(ov), K, A, float(pos_iou_thr), lo, hi, float(min_pos_iou),
                                        int(bool(match_low_quality)), int(bool(gt_max_assign_all)), L.ptr(gl),
                                        int(labels_filled), L.ptr(gt_inds), L.ptr(max_ov), L.ptr(labels),
                                        L.ptr(ws), wsb, L.stream_ptr(ov)), "jdet_assign_max_iou")
    return gt_inds, max_ov, labels


@BOXES.register_module()
class MaxIoUAssigner:
    """-1 don't care, 0 negative, k>0 positive matched to gt k-1."""

    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=.0, gt_max_assign_all=True, ignore_iof_thr=-1,
                 ignore_wrt_candidates=True, match_low_quality=True, assigned_labels_filled=0,
                 iou_calculator=dict(type="BboxOverlaps2D")):
        self.pos_iou_thr = pos_iou_thr
        self.neg_iou_thr = neg_iou_thr
        self.min_pos_iou = min_pos_iou
        self.gt_max_assign_all = gt_max_assign_all
        self.ignore_iof_thr = ignore_iof_thr
        self.ignore_wrt_candidates = ignore_wrt_candidates
        self.match_low_quality = match_low_quality
        self.assigned_labels_filled = assigned_labels_filled
        self.iou_calculator = build_from_cfg(iou_calculator, BOXES)

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        if bboxes.shape[0] == 0 or gt_bboxes.shape[0] == 0:
            raise ValueError("No gt or bboxes")
        overlaps = self.iou_calculator(gt_bboxes, bboxes)
        if (self.ignore_iof_thr > 0) and (gt_bboxes_ignore is not None) and (gt_bboxes_ignore.numel() > 0):
            if self.ignore_wrt_candidates:
                ignore_overlaps = self.iou_calculator(bboxes, gt_bboxes_ignore, mode="iof")
                ignore_max_overlaps = ignore_overlaps.max(dim=1).values
            else:
                ignore_overlaps = self.iou_calculator(gt_bboxes_ignore, bboxes, mode="iof")
                ignore_max_overlaps = ignore_overlaps.max(dim=0).values
            overlaps[:, ignore_max_overlaps > self.ignore_iof_thr] = -1
        return self.assign_wrt_overlaps(overlaps, gt_labels)

    def assign_wrt_overlaps(self, overlaps, gt_labels=None):
        if overlaps.numel() == 0:
            raise ValueError("No gt or proposals")
        num_gts = overlaps.size(0)
        gt_inds, max_overlaps, labels = assign_wrt_overlaps_device(
            overlaps, self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou, self.match_low_quality,
            self.gt_max_assign_all, gt_labels, self.assigned_labels_filled)
        return AssignResult(num_gts, gt_inds, max_overlaps, labels=labels)


@BOXES.register_module()
class MaxIoUAssignerRbbox(MaxIoUAssigner):
    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=.0, gt_max_assign_all=True, ignore_iof_thr=-1,
                 ignore_wrt_candidates=True, iou_calculator=dict(type="BboxOverlaps2D")):
        super().__init__(pos_iou_thr=pos_iou_thr, neg_iou_thr=neg_iou_thr, min_pos_iou=min_pos_iou,
                         gt_max_assign_all=gt_max_assign_all, ignore_iof_thr=ignore_iof_thr,
                         ignore_wrt_candidates=ignore_wrt_candidates, iou_calculator=iou_calculator)

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        if bboxes.shape[0] == 0 or gt_bboxes.shape[0] == 0:
            raise ValueError("No gt or bboxes")
        bboxes = bboxes[:, :5]
        overlaps = self.iou_calculator(gt_bboxes, bboxes)
        # the reference's ignore branch is `assert NotImplementedError` (a no-op), assigner.py:L267-273
        return self.assign_wrt_overlaps(overlaps, gt_labels)


def atss_assign_device(bboxes, num_level_bboxes, gt_bboxes, topk, gt_labels=None, labels_filled=0, overlaps=None):
    """jdet_atss_assign on device tensors: bboxes (A, >= 5) of all levels, gt_bboxes (K, 5), overlaps None (the rotated
    IoU of the candidate pairs is computed in the kernel) or an (A, K) matrix -> (gt_inds int32 (A), max_overlaps (A),
    labels int32 (A) | None).  No host sync: the level sizes are host integers."""
    import ctypes
    L.need_device(bboxes, gt_bboxes, gt_labels, overlaps)
    anchors, gt = L.f32c(bboxes), L.f32c(gt_bboxes[:, :5])
    A, K, nl = anchors.shape[0], gt.shape[0], len(num_level_bboxes)
    offs = [0]
    for n in num_level_bboxes:
        offs.append(offs[-1] + int(n))
    assert offs[-1] == A, "num_level_bboxes sums to %d, %d boxes" % (offs[-1], A)
    ov = L.f32c(overlaps) if overlaps is not None else None
    assert ov is None or tuple(ov.shape) == (A, K)
    gl = gt_labels.to(torch.int32).contiguous() if gt_labels is not None else None
    gt_inds = torch.empty((A,), dtype=torch.int32, device=anchors.device)
    max_ov = torch.empty((A,), dtype=torch.float32, device=anchors.device)
    labels = torch.empty((A,), dtype=torch.int32, device=anchors.device) if gl is not None else None
    wsb = L.lib().jdet_atss_assign_workspace(A, K, nl, int(topk))
    ws = torch.empty((max(wsb, 8),), dtype=torch.uint8, device=anchors.device)
    L.check(L.lib().jdet_atss_assign(L.ptr(anchors), A, anchors.shape[1], (ctypes.c_int32 * (nl + 1))(*offs), nl,
                                     L.ptr(gt), K, L.ptr(gl), L.ptr(ov), int(topk), int(labels_filled), L.ptr(gt_inds),
                                     L.ptr(max_ov), L.ptr(labels), L.ptr(ws), wsb, L.stream_ptr(anchors)),
            "jdet_atss_assign")
    return gt_inds, max_ov, labels


@BOXES.register_module()
class ATSSAssignerRbbox:
    """Adaptive training sample selection on rotated boxes (assigner.py:L276-391): per gt the `topk` anchors of every
    level nearest to its centre are candidates; those whose IoU reaches mean + std of the candidates' IoUs and whose
    centre lies inside the gt are positive; an anchor claimed twice goes to the higher IoU.  0 negative, k > 0 matched
    to gt k - 1 (nothing is ignored).  Tie order, the clamp of topk to a level's size and the form of the inside test
    are this project's rules: include/jdet_hip.h.

    With `BboxOverlaps2D_rotated` as the calculator (the config's) the IoU of the candidate pairs is computed inside
    the kernel, bit-equal to the calculator's matrix; any other calculator is evaluated to its (A, K) matrix and the
    kernel reads the candidates' values from it."""

    def __init__(self, topk, iou_calculator=dict(type="BboxOverlaps2D_rotated"), assigned_labels_filled=0):
        self.topk = topk
        self.iou_calculator = build_from_cfg(iou_calculator, BOXES)
        self.assigned_labels_filled = assigned_labels_filled

    def assign(self, bboxes, num_level_bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        from .iou_calculator import BboxOverlaps2D_rotated
        if bboxes.shape[0] == 0 or gt_bboxes.shape[0] == 0:
            raise ValueError("No gt or bboxes")
        overlaps = None
        if type(self.iou_calculator) is not BboxOverlaps2D_rotated:
            L.need_device(bboxes, gt_bboxes)
            overlaps = self.iou_calculator(bboxes, gt_bboxes)
        gt_inds, max_overlaps, labels = atss_assign_device(
            bboxes, num_level_bboxes, gt_bboxes, self.topk, gt_labels, self.assigned_labels_filled, overlaps)
        return AssignResult(gt_bboxes.shape[0], gt_inds, max_overlaps, labels=labels)


def convex_point_assign_device(points, num_level_points, level_ids, gt, gt_labels, gt_count, scale, pos_num,
                               labels_filled=0):
    """jdet_convex_point_assign on device tensors: points (N, >= 2) of all levels (shared by the images), gt
    (B, Kmax, 8) polygons, gt_labels (B, Kmax) int32 | None, gt_count (B) int32 -> (gt_inds int32 (B, N), labels int32
    (B, N) | None).  No host sync: the level sizes and ids (log2 of the strides) are host integers."""
    import ctypes
    L.need_device(points, gt, gt_labels, gt_count)
    pts, g = L.f32c(points), L.f32c(gt)
    N, nl = pts.shape[0], len(num_level_points)
    assert g.dim() == 3 and g.shape[2] == 8 and len(level_ids) == nl
    B, Kmax = g.shape[0], g.shape[1]
    if Kmax == 0:              # no gt rows at all: one unread row, so that labels still has a gt_labels array behind it
        Kmax = 1
        g = g.new_zeros((B, 1, 8))
        gt_labels = torch.zeros((B, 1), dtype=torch.int32, device=g.device) if gt_labels is not None else None
    offs = [0]
    for n in num_level_points:
        offs.append(offs[-1] + int(n))
    assert offs[-1] == N, "num_level_points sums to %d, %d points" % (offs[-1], N)
    gl = gt_labels.to(torch.int32).contiguous() if gt_labels is not None else None
    gc = gt_count.to(torch.int32).contiguous()
    assert gc.numel() == B and (gl is None or tuple(gl.shape) == (B, Kmax))
    gt_inds = torch.empty((B, N), dtype=torch.int32, device=pts.device)
    labels = torch.empty((B, N), dtype=torch.int32, device=pts.device) if gl is not None else None
    wsb = L.lib().jdet_convex_point_assign_workspace(B, N)
    ws = torch.empty((max(wsb, 8),), dtype=torch.uint8, device=pts.device)
    L.check(L.lib().jdet_convex_point_assign(
        L.ptr(pts), N, pts.shape[1], (ctypes.c_int32 * (nl + 1))(*offs), (ctypes.c_int32 * nl)(*[int(i) for i in level_ids]),
        nl, L.ptr(g), L.ptr(gl), L.ptr(gc), B, Kmax, float(scale), int(pos_num), int(labels_filled), L.ptr(gt_inds),
        L.ptr(labels), L.ptr(ws), wsb, L.stream_ptr(pts)), "jdet_convex_point_assign")
    return gt_inds, labels


def stride_level_id(stride):
    """the integer log2 of a stride that is an exact power of two (assigner.py:L482 applies jt.log2(..).int() to such)"""
    s = int(stride)
    assert s > 0 and s == stride and s & (s - 1) == 0, "point strides must be powers of two, got %r" % (stride,)
    return s.bit_length() - 1


@BOXES.register_module()
class ConvexAssigner:
    """RepPoints init-stage assignment (assigner.py:L393-548): every gt claims the `pos_num` points nearest to the centre
    of its horizontal box, in the pyramid level its size selects; a point claimed twice goes to the nearer gt.  0
    negative, k > 0 matched to gt k - 1.  The level of a gt, the tie order and the clamp of pos_num to a level's size
    are stated in include/jdet_hip.h."""

    def __init__(self, scale=4, pos_num=3, assigned_labels_filled=0):
        self.scale = scale
        self.pos_num = pos_num
        self.assigned_labels_filled = assigned_labels_filled

    @staticmethod
    def _levels(points):
        """(sizes, ids) of the runs of equal stride in column 2 (one host read: the general route)"""
        strides, counts = torch.unique_consecutive(points[:, 2], return_counts=True)
        return counts.tolist(), [stride_level_id(s) for s in strides.tolist()]

    def assign(self, points, gt_rbboxes, gt_rbboxes_ignore=None, gt_labels=None, num_level_points=None,
               level_ids=None):
        """points (n, >= 3) rows [x, y, stride, ...] in level order, gt_rbboxes (k, 8) -> AssignResult.  The level sizes
        and ids are read from the stride column unless the caller passes them."""
        num_points, num_gts = points.shape[0], gt_rbboxes.shape[0]
        if num_points == 0:
            return AssignResult(num_gts, torch.zeros((0,), dtype=torch.int32, device=points.device), None,
                                labels=None if gt_labels is None else torch.zeros((0,), dtype=torch.int32,
                                                                                  device=points.device))
        assert num_gts == 0 or gt_rbboxes.size(1) == 8, "gt_rbboxes should be (N * 8)"
        if num_level_points is None or level_ids is None:
            num_level_points, level_ids = self._levels(points)
        gt = gt_rbboxes.reshape(1, num_gts, 8)
        gl = gt_labels.reshape(1, num_gts) if gt_labels is not None else None
        count = torch.full((1,), num_gts, dtype=torch.int32, device=points.device)
        gt_inds, labels = self.assign_batch(points, num_level_points, level_ids, gt, gl, count)
        return AssignResult(num_gts, gt_inds[0], None, labels=labels[0] if labels is not None else None)

    def assign_batch(self, points, num_level_points, level_ids, gt, gt_labels, gt_count):
        """all images at once (the dense route): gt (B, Kmax, 8), gt_labels (B, Kmax) | None, gt_count (B) int32 on the
        device -> (gt_inds (B, N) int32, labels (B, N) int32 | None)"""
        return convex_point_assign_device(points, num_level_points, level_ids, gt, gt_labels, gt_count, self.scale,
                                          self.pos_num, self.assigned_labels_filled)


@BOXES.register_module()
class MaxConvexIoUAssigner(MaxIoUAssigner):
    """MaxIoUAssigner over point sets (n, 18) and gt polygons (k, 8) (assigner.py:L550-611): the overlaps come from
    `ConvexOverlaps` (jdet_convex_iou), the four steps from jdet_assign_max_iou."""

    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=.0, gt_max_assign_all=True, ignore_iof_thr=-1,
                 ignore_wrt_candidates=True, match_low_quality=True, assigned_labels_filled=0,
                 iou_calculator=dict(type="ConvexOverlaps")):
        super().__init__(pos_iou_thr=pos_iou_thr, neg_iou_thr=neg_iou_thr, min_pos_iou=min_pos_iou,
                         gt_max_assign_all=gt_max_assign_all, ignore_iof_thr=ignore_iof_thr,
                         ignore_wrt_candidates=ignore_wrt_candidates, match_low_quality=match_low_quality,
                         assigned_labels_filled=assigned_labels_filled, iou_calculator=iou_calculator)

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        if bboxes.shape[0] == 0 or gt_bboxes.shape[0] == 0:
            raise ValueError("No gt or bboxes")
        overlaps = self.iou_calculator(gt_bboxes, bboxes)
        # the reference's ignore branch is `assert NotImplementedError` (a no-op), assigner.py:L607-609
        return self.assign_wrt_overlaps(overlaps, gt_labels)
