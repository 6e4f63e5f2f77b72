"""RetinaHead: the head of the reference's own RetinaNet (python/jdet/models/roi_heads/retina_head.py:L16-353;
configs/retinanet_r50v1d_fpn_*.py).  4 + 4 stacked 3x3 conv towers, 3x3 prediction layers, 21 horizontal anchors per
location (AnchorGeneratorRotated, mode "H"), rotated targets through bbox2loc_r (head mode "R"), focal + smooth-L1 per
image divided by that image's positive count.  Parameter names are the reference's (`cls_convs.N.weight`,
`retina_cls.bias`, ...).

Two routes compute the same rules (include/jdet_hip_retina.h states them):
  * fused (device tensors, head mode "R" on anchor mode "H"): one ground-truth preparation launch and one assignment +
    target launch per step for the whole batch and every level (ops/retina.py), then per image one focal and one
    smooth-L1 level node reading those targets in place with the image's normalizer as the device avg_factor; at test
    time one decode / threshold / compaction pair per image, one synchronisation per image instead of three per class;
  * composed: the reference's tensor program (an (A, K) IoU matrix per image, boolean gathers).  Its training side
    (targets and losses) runs on any device; its detection side selects with tensor ops on any device but ends, like
    the fused one, in the device-only NMS of ops/nms_rotated.py -- evaluation on CPU tensors raises, as every op of
    this project does.  The head's mode "H" and rotated-anchor branches exist only composed.
`JDET_RETINA_FUSED=0` selects the composed route on the device; CPU tensors always take it.
The fused route's only host -> device transfer per step is the (N + 1) gt offsets (an ordinary copy from host memory;
the gt counts are the shapes of the target tensors, nothing is read back).

Ours, where the reference is unpinned or fails: argmax ties go to the first gt; an image without gts labels every anchor
0; encode / decode / gt preparation are evaluated in float64 and rounded once (the project's rule for codecs); the
caller's target dicts are not modified (the reference overwrites `rboxes` in place); detections come out class by class
and, inside a class, in the order the NMS received them -- anchor-ascending, or by descending score where the class was
cut to `nms_pre` -- and by descending score once more than `max_dets` survive (the reference returns each class in its
NMS's score order; nothing downstream reads the order)."""
import itertools
import math
import os

import torch
from torch import nn

from jdet_amd.models.boxes.box_ops import (bbox2loc_r, bbox_iou, boxes_x0y0x1y1_to_xywh, loc2bbox_r,
                                           rotated_box_to_bbox, rotated_box_to_poly)
from jdet_amd.models.losses.focal_loss import _FocalLevel, sigmoid_focal_loss
from jdet_amd.models.losses.smooth_l1_loss import _SmoothL1Level, smooth_l1_loss
from jdet_amd.ops import retina as R
from jdet_amd.ops.conv_igemm import conv_module
from jdet_amd.ops.nms_rotated import nms_rotated_keep_mask
from jdet_amd.utils.registry import BOXES, HEADS, build_from_cfg


def fused_enabled():
    return os.environ.get("JDET_RETINA_FUSED", "1") == "1"


def prepare_gts(gts):
    """(K, 5) raw gts -> (rboxes (K, 5), rboxes_h (K, 4)) of RetinaNet.execute (retinanet.py:L31-51), composed: float64
    arithmetic, rounded once to the input's dtype"""
    g = gts.double()
    x, y, w, h, a = g.unbind(dim=1)
    a = torch.where(a >= 0, a - math.pi, a)
    swap = a < -math.pi / 2
    a = torch.where(swap, a + math.pi / 2, a)
    w, h = torch.where(swap, h, w), torch.where(swap, w, h)
    wide = w > h                                            # cvt2_w_greater_than_h(reverse_hw=False)
    ow, oh, oa = torch.where(wide, w, h), torch.where(wide, h, w), torch.where(wide, a - math.pi / 2, a)
    rboxes = torch.stack([x, y, ow, oh, oa], dim=1)
    turned = torch.stack([x, y, ow, oh, oa + math.pi / 2], dim=1)
    return rboxes.to(gts.dtype), rotated_box_to_bbox(turned).to(gts.dtype)


@HEADS.register_module()
class RetinaHead(nn.Module):
    def __init__(self, n_class, in_channels, feat_channels=256, stacked_convs=4, pos_iou_thresh=0.5,
                 neg_iou_thresh_hi=0.4, neg_iou_thresh_lo=0., nms_pre=1000, max_dets=100, anchor_generator=None,
                 mode="H", score_threshold=0.05, nms_iou_threshold=0.5, roi_beta=0., cls_loss_weight=1.,
                 loc_loss_weight=0.2):
        super().__init__()
        self.pos_iou_thresh = pos_iou_thresh
        self.neg_iou_thresh_hi = neg_iou_thresh_hi
        self.neg_iou_thresh_lo = neg_iou_thresh_lo
        self.stacked_convs = stacked_convs
        self.nms_pre = nms_pre
        self.max_dets = max_dets
        self.mode = mode
        self.anchor_generator = build_from_cfg(anchor_generator, BOXES)
        self.anchor_mode = self.anchor_generator.mode
        n_anchor = self.anchor_generator.num_base_anchors[0]
        self.cls_convs = nn.ModuleList()
        self.reg_convs = nn.ModuleList()
        for i in range(self.stacked_convs):
            chn = in_channels if i == 0 else feat_channels
            self.cls_convs.append(nn.Conv2d(chn, feat_channels, 3, stride=1, padding=1))
            self.reg_convs.append(nn.Conv2d(chn, feat_channels, 3, stride=1, padding=1))
        self.n_class = n_class
        self.box_dim = 4 if mode == "H" else 5
        self.retina_cls = nn.Conv2d(feat_channels, n_anchor * n_class, 3, padding=1)
        self.retina_reg = nn.Conv2d(feat_channels, n_anchor * self.box_dim, 3, padding=1)
        self.roi_beta = roi_beta
        self.nms_thresh = nms_iou_threshold
        self.score_thresh = score_threshold
        self.cls_loss_weight = cls_loss_weight
        self.loc_loss_weight = loc_loss_weight
        self._anchors = {}
        self.init_weights()

    def init_weights(self):
        for conv in list(self.cls_convs) + list(self.reg_convs) + [self.retina_reg, self.retina_cls]:
            nn.init.normal_(conv.weight, mean=0, std=0.01)
            nn.init.constant_(conv.bias, 0)
        # the prior of the focal-loss paper: every class starts at probability 0.01
        nn.init.constant_(self.retina_cls.bias, -(math.log((1 - 0.01) / 0.01)))

    # ------------------------------------------------------------------------------------------------ forward pieces
    def execute_single(self, x):
        """one level -> (bbox_pred (n, H * W * anchors, 5 | 4), cls_score (n, H * W * anchors, n_class))"""
        n = x.shape[0]
        cls_feat = reg_feat = x
        for conv in self.cls_convs:
            cls_feat = conv_module(conv, cls_feat, relu=True)
        for conv in self.reg_convs:
            reg_feat = conv_module(conv, reg_feat, relu=True)
        cls_score = conv_module(self.retina_cls, cls_feat)
        bbox_pred = conv_module(self.retina_reg, reg_feat)
        return (bbox_pred.permute(0, 2, 3, 1).reshape(n, -1, self.box_dim),
                cls_score.permute(0, 2, 3, 1).reshape(n, -1, self.n_class))

    def anchors_of(self, sizes, device):
        """all levels' anchors concatenated, (A, 4) (anchor mode "R": (A, 5)); cached per (sizes, device)"""
        key = (tuple(map(tuple, sizes)), str(device))
        hit = self._anchors.get(key)
        if hit is None:
            hit = self._anchors[key] = torch.cat(self.anchor_generator.grid_anchors(sizes, device), dim=0).contiguous()
        return hit

    def cvt2_w_greater_than_h(self, boxes, reverse_hw=True):
        """(n, 5) [x, y, w, h, a]: with reverse_hw the sides are exchanged first; then w > h keeps the sides and turns
        the angle by -pi/2, otherwise the sides are exchanged and the angle kept (retina_head.py:L170-190)"""
        x, y, w, h, a = boxes.unbind(dim=1)
        if reverse_hw:
            w, h = h, w
        wide = w > h
        return torch.stack([x, y, torch.where(wide, w, h), torch.where(wide, h, w),
                            torch.where(wide, a - 0.5 * math.pi, a)], dim=1)

    def _fused_route(self, t):
        return t.is_cuda and t.dtype == torch.float32 and fused_enabled() and self.mode == "R" and \
            self.anchor_mode == "H" and not torch.is_autocast_enabled()

    # ------------------------------------------------------------------------------------------------------- targets
    def assign_labels(self, roi, bbox, bbox_h, label):
        """composed: anchors (A, 4 | 5), one image's prepared gts -> (loc targets (A, 5 | 4), labels (A) int32 with
        -1 = ignored); retina_head.py:L136-166"""
        A = roi.shape[0]
        if bbox.shape[0] == 0:
            return roi.new_zeros((A, self.box_dim)), torch.zeros((A,), dtype=torch.int32, device=roi.device)
        if self.mode == "H":
            iou = bbox_iou(roi[:, :4], bbox)
        elif self.anchor_mode == "H":
            iou = bbox_iou(roi[:, :4], bbox_h)
        else:
            from jdet_amd.ops import box_iou_rotated
            iou = box_iou_rotated(roi, bbox)
        max_iou, assignment = iou.max(dim=1)                # the first gt among equal maxima
        labels = torch.full((A,), -1, dtype=torch.int32, device=roi.device)
        labels[(max_iou < self.neg_iou_thresh_hi) & (max_iou >= self.neg_iou_thresh_lo)] = 0
        pos = max_iou >= self.pos_iou_thresh
        labels = torch.where(pos, label.to(torch.int32)[assignment], labels)
        loc = roi.new_zeros((A, self.box_dim))
        if self.mode == "H":
            from jdet_amd.models.boxes.box_ops import bbox2loc
            loc[pos] = bbox2loc(roi[pos, :4], bbox[assignment[pos]])
        else:
            src = roi.double() if roi.shape[1] == 5 else torch.cat(
                [roi.double(), roi.new_full((A, 1), -0.5 * math.pi, dtype=torch.float64)], dim=1)
            src = self.cvt2_w_greater_than_h(boxes_x0y0x1y1_to_xywh(src))
            loc[pos] = bbox2loc_r(src[pos], bbox.double()[assignment[pos]]).to(loc.dtype)
        return loc, labels

    def loss_fused(self, bbox_pred, cls_score, anchors, targets):
        raw, labels = [t["rboxes"] for t in targets], [t["labels"] for t in targets]
        N = len(targets)
        offsets = torch.tensor([0] + list(itertools.accumulate(int(r.shape[0]) for r in raw)), dtype=torch.int32)
        offsets = offsets.to(anchors.device)                 # the step's one host -> device copy
        rboxes, rboxes_h = R.gt_prepare(torch.cat(raw, dim=0))
        t = R.targets(anchors, rboxes, rboxes_h, torch.cat(labels, dim=0), offsets, self.pos_iou_thresh,
                      self.neg_iou_thresh_hi, self.neg_iou_thresh_lo)
        cls_loss = loc_loss = 0
        for i in range(N):
            avg = t["normalizer"][i]
            cls_loss = cls_loss + _FocalLevel.apply(cls_score[i], t["labels"][i], t["label_weights"][i], 0.25, 2.0, avg,
                                                    self.cls_loss_weight / N)
            loc_loss = loc_loss + _SmoothL1Level.apply(bbox_pred[i], t["loc_targets"][i], t["loc_weights"][i],
                                                       self.roi_beta, avg, self.loc_loss_weight / N)
        return dict(roi_cls_loss=cls_loss, roi_loc_loss=loc_loss)

    def composed_targets(self, anchors, targets):
        """[(loc targets (A, 5 | 4), labels (A) int32)] per image, from the raw target dicts"""
        out = []
        for t in targets:
            # head mode "H" regresses corner boxes: the gts' enclosing horizontal boxes
            rboxes, rboxes_h = prepare_gts(t["rboxes"]) if self.mode == "R" else (t["hboxes"], t["hboxes"])
            out.append(self.assign_labels(anchors, rboxes, rboxes_h, t["labels"]))
        return out

    def losses(self, all_bbox_pred, all_cls_score, all_gt_roi_locs, all_gt_roi_labels):
        """composed: per image focal (alpha 0.25, sum) over label >= 0 and smooth-L1 (roi_beta, sum) over label > 0, each
        divided by max(#positives, 1); then cls_loss_weight / N and loc_loss_weight / N (retina_head.py:L272-294)"""
        N = len(all_bbox_pred)
        cls_loss = loc_loss = 0
        for i in range(N):
            lab = all_gt_roi_labels[i]
            pos, used = lab > 0, lab >= 0
            normalizer = pos.sum().clamp(min=1).to(all_bbox_pred[i].dtype)
            loc = smooth_l1_loss(all_bbox_pred[i][pos], all_gt_roi_locs[i][pos].to(all_bbox_pred[i].dtype),
                                 beta=self.roi_beta, reduction="sum")
            cls = sigmoid_focal_loss(all_cls_score[i][used], lab[used], reduction="sum", alpha=0.25)
            cls_loss = cls_loss + cls / normalizer
            loc_loss = loc_loss + loc / normalizer
        return dict(roi_cls_loss=cls_loss * (self.cls_loss_weight / N), roi_loc_loss=loc_loss * (self.loc_loss_weight / N))

    # ---------------------------------------------------------------------------------------------------- detections
    def _select_composed(self, anchors, bbox_pred, cls_score, scale_x, scale_y):
        """the front of get_bboxes as tensor ops: (boxes, scores, labels, counts) class-major, anchor-ascending"""
        if self.mode == "H":
            from jdet_amd.models.boxes.box_ops import loc2bbox
            bbox = loc2bbox(anchors[:, :4], bbox_pred)
            ok = torch.ones((bbox.shape[0],), dtype=torch.bool, device=bbox.device)
        else:
            A = anchors.shape[0]
            src = anchors.double() if anchors.shape[1] == 5 else torch.cat(
                [anchors.double(), anchors.new_full((A, 1), -0.5 * math.pi, dtype=torch.float64)], dim=1)
            src = self.cvt2_w_greater_than_h(boxes_x0y0x1y1_to_xywh(src))
            if anchors.shape[1] == 4:
                # -pi + pi/2 and -pi/2 + pi/2 stated exactly (the kernel's proposals)
                src[:, 4] = torch.where(src[:, 4] < -0.75 * math.pi, -0.5 * math.pi, 0.0)
            else:
                src[:, 4] = src[:, 4] + 0.5 * math.pi
            bbox = loc2bbox_r(src, bbox_pred.double()).to(bbox_pred.dtype)
            half_pi = torch.tensor(0.5 * math.pi, dtype=bbox.dtype, device=bbox.device)
            ok = (bbox[:, 4] < half_pi) & (bbox[:, 4] > -half_pi)
        bbox = bbox.clone()
        bbox[:, [0, 2]] = bbox[:, [0, 2]] * bbox.new_tensor(scale_x)
        bbox[:, [1, 3]] = bbox[:, [1, 3]] * bbox.new_tensor(scale_y)
        probs = cls_score.double().sigmoid().to(cls_score.dtype)
        sel = ((probs > self.score_thresh) & ok[:, None]).t()          # (C, A): nonzero() walks it class-major
        cls_idx, anchor_idx = sel.nonzero(as_tuple=True)
        counts = sel.sum(dim=1).cpu().tolist()
        return bbox[anchor_idx], probs.t()[sel], cls_idx.to(torch.int32), counts

    def _finish(self, boxes, scores, labels, counts):
        """per class the top nms_pre by score (stable), one labelled rotated NMS over all classes, the global top max_dets"""
        dev = boxes.device
        if boxes.shape[0] == 0:
            return boxes.new_zeros((0, 8)), scores, labels
        if any(c > self.nms_pre for c in counts):
            keep, start = [], 0
            for c in counts:
                idx = torch.arange(start, start + c, device=dev)
                if c > self.nms_pre:
                    idx = idx[torch.argsort(scores[start:start + c], descending=True, stable=True)[:self.nms_pre]]
                keep.append(idx)
                start += c
            keep = torch.cat(keep)
            boxes, scores, labels = boxes[keep], scores[keep], labels[keep]
        if self.mode == "H":
            from jdet_amd.ops.nms import nms
            keep = nms(boxes, scores, self.nms_thresh, labels).sort().values
        else:
            dets = torch.cat([boxes, labels.to(boxes.dtype)[:, None]], dim=1)
            order = torch.argsort(scores, descending=True, stable=True)
            order = order[torch.argsort(labels[order], stable=True)]
            keep = nms_rotated_keep_mask(dets, order, self.nms_thresh, rule="cuda", n_labels=self.n_class).nonzero()[:, 0]
        boxes, scores, labels = boxes[keep], scores[keep], labels[keep]
        if scores.numel() > self.max_dets:
            order = torch.argsort(scores, descending=True, stable=True)[:self.max_dets]
            boxes, scores, labels = boxes[order], scores[order], labels[order]
        return (rotated_box_to_poly(boxes) if self.mode == "R" else boxes), scores, labels

    def get_bboxes(self, anchors, bbox_pred, cls_score, targets):
        results = []
        for i, target in enumerate(targets):
            img_size, ori_img_size = target["img_size"], target["ori_img_size"]
            assert abs(ori_img_size[0] / ori_img_size[1] - img_size[0] / img_size[1]) < 1e-6      # keeps the angle
            sx, sy = ori_img_size[0] / img_size[0], ori_img_size[1] / img_size[1]
            if self._fused_route(cls_score):
                picked = R.detect(anchors, bbox_pred[i], cls_score[i], self.score_thresh, sx, sy)
            else:
                picked = self._select_composed(anchors, bbox_pred[i], cls_score[i], sx, sy)
            results.append(self._finish(*picked))
        return results

    # ------------------------------------------------------------------------------------------------------- forward
    def predict(self, xs):
        """features of every level -> (bbox_pred (N, A, 5 | 4), cls_score (N, A, n_class), anchors (A, 4 | 5)), the levels
        concatenated"""
        per_level = [self.execute_single(x) for x in xs]
        bbox_pred = torch.cat([p[0] for p in per_level], dim=1)
        cls_score = torch.cat([p[1] for p in per_level], dim=1)
        return bbox_pred, cls_score, self.anchors_of([tuple(x.shape[2:]) for x in xs], xs[0].device)

    def loss(self, bbox_pred, cls_score, anchors, targets):
        """dict(roi_cls_loss, roi_loc_loss) of `predict`'s outputs, on the fused or the composed route"""
        if self._fused_route(cls_score):
            return self.loss_fused(bbox_pred, cls_score, anchors, targets)
        assigned = self.composed_targets(anchors, targets)
        return self.losses(list(bbox_pred), list(cls_score), [a[0] for a in assigned], [a[1] for a in assigned])

    def forward(self, xs, targets):
        """features of every level + the target dicts -> training: dict(roi_cls_loss, roi_loc_loss); eval: a list of
        (polys (k, 8), scores (k), labels (k), 0-based) per image"""
        bbox_pred, cls_score, anchors = self.predict(xs)
        if not self.training:
            with torch.no_grad():
                return self.get_bboxes(anchors, bbox_pred, cls_score, targets)
        return self.loss(bbox_pred, cls_score, anchors, targets)

    execute = forward
