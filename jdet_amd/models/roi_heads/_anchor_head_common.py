"""Pieces shared by the rotated single-stage anchor heads (S2ANetHead, RotatedRetinaHead and its ATSS / KFIoU
subclasses): cached grid anchors, valid flags from `pad_shape` (stored (w, h)), the loss of one stage
(targets -> per-level loss; S2ANet runs it twice, FAM and ODM) and the per-image decode in front of the post-processing
that every single-stage head shares (_dense_head_common.py)."""
import numpy as np
import torch

from jdet_amd.models.boxes.anchor_target import anchor_target, images_to_levels
from jdet_amd.models.boxes.box_ops import delta2bbox_rotated
from jdet_amd.utils.general import multi_apply
from jdet_amd.utils.registry import BOXES, build_from_cfg

from ._dense_head_common import cut_level, merge_levels, nms_polys, parse_targets, per_image


class RotatedAnchorHeadMixin:
    def _init_anchors(self, level, featmap_size, device):
        key = (level, tuple(featmap_size), str(device))
        if key not in self.base_anchors:
            self.base_anchors[key] = self.anchor_generators[level].grid_anchors(
                featmap_size, self.anchor_strides[level], device=device)
        return self.base_anchors[key]

    def _valid_flags(self, featmap_sizes, img_metas, device):
        valid_flag_list = []
        cache = self.__dict__.setdefault("_valid_flag_cache", {})
        for img_meta in img_metas:
            # the flags depend on (level sizes, pad_shape) only: DOTA tiles have one shape, so they are built once
            key = (tuple(featmap_sizes), tuple(img_meta["pad_shape"][:2]), str(device))
            if key not in cache:
                multi_level_flags = []
                all_valid = True
                for i in range(len(featmap_sizes)):
                    anchor_stride = self.anchor_strides[i]
                    feat_h, feat_w = featmap_sizes[i]
                    w, h = img_meta["pad_shape"][:2]
                    valid_feat_h = min(int(np.ceil(h / anchor_stride)), feat_h)
                    valid_feat_w = min(int(np.ceil(w / anchor_stride)), feat_w)
                    all_valid = all_valid and valid_feat_h == feat_h and valid_feat_w == feat_w
                    multi_level_flags.append(self.anchor_generators[i].valid_flags(
                        (feat_h, feat_w), (valid_feat_h, valid_feat_w), device=device))
                cache[key] = (multi_level_flags, all_valid)
            multi_level_flags, all_valid = cache[key]
            # host-side fact (no device sync): every anchor is valid -> anchor_target skips the mask gather
            img_meta["_all_valid"] = all_valid
            valid_flag_list.append(list(multi_level_flags))
        return valid_flag_list

    def get_init_anchors(self, featmap_sizes, img_metas, device):
        multi_level_anchors = [self._init_anchors(i, featmap_sizes[i], device) for i in range(len(featmap_sizes))]
        anchor_list = [list(multi_level_anchors) for _ in range(len(img_metas))]
        return anchor_list, self._valid_flags(featmap_sizes, img_metas, device)

    anchor_target = staticmethod(anchor_target)     # (RotatedATSSHead: its own, the level sizes go to the assigner)

    def _stage_loss(self, cls_scores, bbox_preds, anchor_list, valid_flag_list, gt_bboxes, gt_labels, img_metas,
                    gt_bboxes_ignore, cfg, loss_cls_fn, loss_bbox_fn, targets=None, need_anchors=True, extra_preds=()):
        """(losses_cls, losses_bbox) per level of one stage, None where the targets are.  targets: what
        `self.anchor_target` returned for these anchors, else computed here; need_anchors: the per-level anchors, which
        the loss only reads where it regresses decoded boxes; extra_preds: further per-level prediction lists, handed to
        `_loss_single` behind the level's bbox_weights (CSLRRetinaHead: the angle classification maps, and a third loss
        list comes back)"""
        num_level_anchors = [anchors.size(0) for anchors in anchor_list[0]]
        all_anchor_list = [None] * len(num_level_anchors)
        if need_anchors:
            concat_anchor_list = [torch.cat(anchor_list[i]) for i in range(len(anchor_list))]
            all_anchor_list = images_to_levels(concat_anchor_list, num_level_anchors)
        if targets is None:
            label_channels = self.cls_out_channels if self.use_sigmoid_cls else 1
            targets = self.anchor_target(anchor_list, valid_flag_list, gt_bboxes, img_metas, self.target_means,
                                         self.target_stds, cfg, gt_bboxes_ignore_list=gt_bboxes_ignore,
                                         gt_labels_list=gt_labels, label_channels=label_channels,
                                         sampling=self.sampling)
        if targets is None:
            return None
        labels_list, label_weights_list, bbox_targets_list, bbox_weights_list, num_total_pos, num_total_neg = targets
        num_total_samples = num_total_pos + num_total_neg if self.sampling else num_total_pos
        return multi_apply(self._loss_single, cls_scores, bbox_preds, all_anchor_list, labels_list, label_weights_list,
                           bbox_targets_list, bbox_weights_list, *extra_preds, loss_cls_fn=loss_cls_fn,
                           loss_bbox_fn=loss_bbox_fn,
                           num_total_samples=num_total_samples, cfg=cfg)

    def _loss_single(self, cls_score, bbox_pred, anchors, labels, label_weights, bbox_targets, bbox_weights,
                     loss_cls_fn, loss_bbox_fn, num_total_samples, cfg):
        # The level's targets are column windows [:, s:e] of the per-image arrays.  FocalLoss / SmoothL1Loss / L1Loss read
        # such windows in place (one node per level and loss, models/losses/focal_loss.py: _FocalLevel); flattening them
        # here -- what the reference does, s2anet_head.py:L441-450 -- costs a copy per window (40 per S2ANet step).
        from jdet_amd.models.losses.focal_loss import FocalLoss
        from jdet_amd.models.losses.smooth_l1_loss import L1Loss, SmoothL1Loss
        if not isinstance(loss_cls_fn, FocalLoss):
            labels = labels.reshape(-1)
            label_weights = label_weights.reshape(-1)
        cls_score = cls_score.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels)
        loss_cls = loss_cls_fn(cls_score, labels, label_weights, avg_factor=num_total_samples)
        from jdet_amd.models.losses.gaussian_dist_loss import GaussianBoxLoss
        if isinstance(loss_bbox_fn, GaussianBoxLoss):
            # GDLoss / GDLoss_v1 / KFLoss: the deltas, the level's anchors and the target / weight windows go to ONE node
            # per level that decodes in registers (losses/gaussian_dist_loss.py: GaussianBoxLoss.level) -- no torch
            # decode, no flattening copies, no compaction by mask
            bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 5)
            loss_bbox = loss_bbox_fn.level(bbox_pred, anchors, bbox_targets, bbox_weights, num_total_samples,
                                           self._bbox_coder(cfg), cfg.get("reg_decoded_bbox", False))
            return loss_cls, loss_bbox
        if not isinstance(loss_bbox_fn, (SmoothL1Loss, L1Loss)) or cfg.get("reg_decoded_bbox", False):
            bbox_targets = bbox_targets.reshape(-1, 5)
            bbox_weights = bbox_weights.reshape(-1, 5)
        bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 5)
        if cfg.get("reg_decoded_bbox", False):
            bbox_pred = self._bbox_coder(cfg).decode(anchors.reshape(-1, 5), bbox_pred)
        loss_bbox = loss_bbox_fn(bbox_pred, bbox_targets, bbox_weights, avg_factor=num_total_samples)
        return loss_cls, loss_bbox

    def _bbox_coder(self, cfg):
        bbox_coder_cfg = cfg.get("bbox_coder", "")
        if bbox_coder_cfg == "":
            bbox_coder_cfg = dict(type="DeltaXYWHBBoxCoder")
        return build_from_cfg(bbox_coder_cfg, BOXES)

    def _level_scores(self, cls_score):
        """a level's (A * C, H, W) map -> (scores (n, C), rank); rank() is the score the `nms_pre` cut ranks the rows
        by, the best foreground class"""
        cls_score = cls_score.permute(1, 2, 0).reshape(-1, self.cls_out_channels)
        if self.use_sigmoid_cls:
            scores = cls_score.sigmoid()
            return scores, lambda: scores.max(dim=1).values
        scores = cls_score.softmax(-1)
        return scores, lambda: scores[:, 1:].max(dim=1).values

    def get_bboxes_single(self, cls_score_list, bbox_pred_list, mlvl_anchors, img_shape, scale_factor, cfg,
                          rescale=False):
        assert len(cls_score_list) == len(bbox_pred_list) == len(mlvl_anchors)
        mlvl_bboxes, mlvl_scores = [], []
        for cls_score, bbox_pred, anchors in zip(cls_score_list, bbox_pred_list, mlvl_anchors):
            assert cls_score.shape[-2:] == bbox_pred.shape[-2:]
            scores, rank = self._level_scores(cls_score)
            bbox_pred = bbox_pred.permute(1, 2, 0).reshape(-1, 5)
            anchors, bbox_pred, scores = cut_level(cfg.get("nms_pre", -1), rank, anchors, bbox_pred, scores)
            mlvl_bboxes.append(delta2bbox_rotated(anchors, bbox_pred, self.target_means, self.target_stds, img_shape))
            mlvl_scores.append(scores)
        return nms_polys(*merge_levels(mlvl_bboxes, mlvl_scores, scale_factor, rescale, self.use_sigmoid_cls), cfg)

    def _get_bboxes(self, cls_scores, bbox_preds, anchor_list, img_metas, rescale):
        """`get_bboxes_single` of every image on its own anchors (per level) with the test cfg"""
        cfg = self.test_cfg.copy()
        return per_image(lambda b, cls_score_list, bbox_pred_list: self.get_bboxes_single(
            cls_score_list, bbox_pred_list, anchor_list[b], img_metas[b]["img_shape"], img_metas[b]["scale_factor"],
            cfg, rescale), len(img_metas), cls_scores, bbox_preds)

    def parse_targets(self, targets, is_train=True):
        parsed = parse_targets(targets, is_train)
        return parsed if is_train else parsed[2]
