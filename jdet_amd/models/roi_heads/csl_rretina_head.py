"""RetinaNet-OBB head with a Circular Smooth Label angle branch.  Mirrors python/jdet/models/roi_heads/csl_rretina_head.py:
a third prediction layer on the regression tower, `retina_angle_cls` (3x3, num_anchors * coding_len channels), classifies
the angle delta into the bins of `angle_coder` (CSLCoder) under `loss_angle` (SmoothFocalLoss); at test time the angle of
a kept row is the one its best bin stands for, and replaces column 4 of the regressed delta.  Everything else is
RotatedRetinaHead's.

The reference encodes a (anchors, coding_len) label array per image inside anchor_target; here the angle target and weight
of a level are column 4 of its bbox_targets / bbox_weights windows (what the reference encodes from:
`angle_targets[pos] = pos_bbox_targets[:, 4:5]`, `angle_weights[pos] = 1` where bbox_weights is), so anchor_target is
unchanged and the labels exist only inside the loss (models/losses/smooth_focal_loss.py: csl_angle_loss)."""
import torch
from torch import nn

from jdet_amd.models.boxes import coder as _coder
from jdet_amd.models.boxes.box_ops import delta2bbox_rotated
from jdet_amd.models.losses.smooth_focal_loss import csl_angle_loss
from jdet_amd.models.utils.weight_init import bias_init_with_prob, normal_init
from jdet_amd.ops.conv_igemm import conv_module
from jdet_amd.utils.registry import BOXES, HEADS, LOSSES, build_from_cfg

from ._dense_head_common import _DEFAULT_ASSIGN, merge_levels, nms_polys, per_image, topk_rows
from .rotated_retina_head import RotatedRetinaHead


@HEADS.register_module()
class CSLRRetinaHead(RotatedRetinaHead):
    def __init__(self, num_classes, in_channels, feat_channels=256, stacked_convs=4, octave_base_scale=4,
                 scales_per_octave=3, anchor_ratios=[1.0, 0.5, 2.0], anchor_strides=[8, 16, 32, 64, 128],
                 anchor_base_sizes=None, target_means=(.0, .0, .0, .0, .0), target_stds=(1.0, 1.0, 1.0, 1.0, 1.0),
                 loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=1.0),
                 angle_coder=dict(type="CSLCoder", omega=4, window="gaussian", radius=3),
                 loss_angle=dict(type="SmoothFocalLoss", gamma=2.0, alpha=0.25, loss_weight=0.8),
                 test_cfg=dict(nms_pre=2000, min_bbox_size=0, score_thr=0.05, nms=dict(type="nms_rotated", iou_thr=0.1),
                               max_per_img=2000),
                 train_cfg=_DEFAULT_ASSIGN):
        super().__init__(num_classes, in_channels, feat_channels=feat_channels, stacked_convs=stacked_convs,
                         octave_base_scale=octave_base_scale, scales_per_octave=scales_per_octave,
                         anchor_ratios=anchor_ratios, anchor_strides=anchor_strides, anchor_base_sizes=anchor_base_sizes,
                         target_means=target_means, target_stds=target_stds, loss_cls=loss_cls, loss_bbox=loss_bbox,
                         test_cfg=test_cfg, train_cfg=train_cfg)
        self.angle_coder = build_from_cfg(angle_coder, BOXES)
        self.coding_len = self.angle_coder.coding_len
        self.loss_angle = build_from_cfg(loss_angle, LOSSES)
        # (behind the parent's layers and their initialisation, which the parent's constructor has run)
        self.retina_angle_cls = nn.Conv2d(self.feat_channels, self.num_anchors * self.coding_len, 3, padding=1)
        normal_init(self.retina_angle_cls, std=0.01, bias=bias_init_with_prob(0.01))

    def forward_single(self, x, stride=None, mask=None):
        cls_feat, reg_feat = self._towers(x, mask)
        return (conv_module(self.retina_cls, cls_feat), conv_module(self.retina_reg, reg_feat),
                conv_module(self.retina_angle_cls, reg_feat))

    def loss(self, cls_scores, bbox_preds, angle_clses, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        featmap_sizes = [tuple(featmap.shape[-2:]) for featmap in cls_scores]
        assert len(featmap_sizes) == len(self.anchor_generators)
        anchor_list, valid_flag_list = self.get_init_anchors(featmap_sizes, img_metas, cls_scores[0].device)
        losses = self._stage_loss(cls_scores, bbox_preds, anchor_list, valid_flag_list, gt_bboxes, gt_labels, img_metas,
                                  gt_bboxes_ignore, self.train_cfg.copy(), self.loss_cls, self.loss_bbox,
                                  extra_preds=(angle_clses,))
        return None if losses is None else dict(loss_cls=losses[0], loss_bbox=losses[1], loss_angle=losses[2])

    def _loss_single(self, cls_score, bbox_pred, anchors, labels, label_weights, bbox_targets, bbox_weights, angle_cls,
                     loss_cls_fn, loss_bbox_fn, num_total_samples, cfg):
        loss_cls, loss_bbox = super()._loss_single(cls_score, bbox_pred, anchors, labels, label_weights, bbox_targets,
                                                   bbox_weights, loss_cls_fn, loss_bbox_fn, num_total_samples, cfg)
        # a view of the channels-last map the prediction conv returns
        angle_cls = angle_cls.permute(0, 2, 3, 1).reshape(-1, self.coding_len)
        loss_angle = csl_angle_loss(self.loss_angle, self.angle_coder, angle_cls, bbox_targets, bbox_weights,
                                    num_total_samples)
        return loss_cls, loss_bbox, loss_angle

    def get_bboxes(self, cls_scores, bbox_preds, angle_clses, img_metas, rescale=True):
        assert len(cls_scores) == len(bbox_preds) == len(angle_clses)
        featmap_sizes = [tuple(featmap.shape[-2:]) for featmap in cls_scores]
        anchor_list, _ = self.get_init_anchors(featmap_sizes, img_metas, cls_scores[0].device)
        cfg = self.test_cfg.copy()
        return per_image(lambda b, cls_score_list, bbox_pred_list, angle_cls_list: self.get_bboxes_single(
            cls_score_list, bbox_pred_list, angle_cls_list, anchor_list[b], img_metas[b]["img_shape"],
            img_metas[b]["scale_factor"], cfg, rescale), len(img_metas), cls_scores, bbox_preds, angle_clses)

    def _level_angles(self, angle_cls, keep):
        """(A * coding_len, H, W) angle logits of a level -> the decoded angle of its rows, or of the rows `keep`.  Fused:
        the kept rows' logits are read in place.  Composed: the reference's program -- the sigmoid of the whole map, the
        gather, the argmax of the probabilities (it differs from the argmax of the logits only where the float32 sigmoid
        rounds two different logits to one float)"""
        angle_cls = angle_cls.permute(1, 2, 0).reshape(-1, self.coding_len)
        if _coder.CSL_FUSED:
            return self.angle_coder.decode(angle_cls, index=keep)
        probs = angle_cls.sigmoid()
        return self.angle_coder.decode(probs if keep is None else probs[keep])

    def get_bboxes_single(self, cls_score_list, bbox_pred_list, angle_cls_list, mlvl_anchors, img_shape, scale_factor, cfg,
                          rescale=False):
        assert len(cls_score_list) == len(bbox_pred_list) == len(angle_cls_list) == len(mlvl_anchors)
        nms_pre = cfg.get("nms_pre", -1)
        mlvl_bboxes, mlvl_scores = [], []
        for cls_score, bbox_pred, angle_cls, anchors in zip(cls_score_list, bbox_pred_list, angle_cls_list, mlvl_anchors):
            assert cls_score.shape[-2:] == bbox_pred.shape[-2:] == angle_cls.shape[-2:]
            scores, rank = self._level_scores(cls_score)
            bbox_pred = bbox_pred.permute(1, 2, 0).reshape(-1, 5)
            # rank and cut first, then decode the angle of the kept rows only
            keep = topk_rows(rank(), nms_pre) if 0 < nms_pre < scores.shape[0] else None
            angle = self._level_angles(angle_cls, keep)
            if keep is not None:
                anchors, bbox_pred, scores = anchors[keep], bbox_pred[keep], scores[keep]
            bbox_pred = torch.cat([bbox_pred[:, :4], angle[:, None].to(bbox_pred.dtype)], dim=1)
            mlvl_bboxes.append(delta2bbox_rotated(anchors, bbox_pred, self.target_means, self.target_stds, img_shape))
            mlvl_scores.append(scores)
        return nms_polys(*merge_levels(mlvl_bboxes, mlvl_scores, scale_factor, rescale, self.use_sigmoid_cls), cfg)
