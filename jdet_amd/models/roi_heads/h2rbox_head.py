"""H2RBox head: FCOSHead plus a second, rotated view of the same batch and a consistency loss between the two views.
Mirrors python/jdet/models/roi_heads/h2rbox_head.py: H2RBoxHead L30-860 (obb2xyxy L198-214, forward_aug L216-235,
execute_train L237-244, _process_rotation_agnostic L312-319, loss L321-519, the rect_classes rewrite L667-674).
Everything else -- towers, Scale, points, targets, inference -- is FCOSHead's, and so are the three losses both heads
have: FCOSHead._dense_parts / _general_parts compute them through the `_loss_bbox_dense` / `_loss_bbox_general` hooks
overridden here (horizontal boxes, the reference's normalisers) and hand back the intermediates the consistency term
is computed from.

Two routes for the loss, same values, behind FCOSHead's `dense` switch:
  dense    device fp32 tensors -- what the config hits.  Targets by jdet_fcos_targets; focal loss, the horizontal IoU
           loss and the centerness BCE over ALL points as in FCOSHead._dense_parts; the consistency branch in one launch
           over all points (csrc/h2rbox_aug_loss.hip through H2RBoxLoss.dense): cell map, gather of view 2, decoded
           boxes, rotated targets, the three terms; the sums, the scalar minimum and every count stay on the device --
           no nonzero(), no .any(), no host sync.
  general  the reference's tensor program: nonzero() of the positives, the per-level cell map in a Python loop,
           boolean masks, gathers, H2RBoxLoss on the gathered rows.  It keeps the reference's LEVEL-major flattening.

Label conventions (the reference's, kept):
  rotation_agnostic_classes  compared with the 1-BASED labels of the positives (the reference adds 1 to the labels
                             before it gathers them, L387/L440): class ids 1 .. num_classes;
  rect_classes               compared with the labels multiclass_nms_rotated returns at inference: 0-BASED.
Images without gts and background rows follow include/jdet_hip.h (background everywhere / zero targets); the
rounding of the cell map is round-half-to-even (include/jdet_hip.h)."""
import math

import torch

from jdet_amd.models.boxes.box_ops import distance2obb
from jdet_amd.utils.general import multi_apply
from jdet_amd.utils.registry import HEADS, LOSSES, build_from_cfg

from .fcos_head import INF, FCOSHead


@HEADS.register_module()
class H2RBoxHead(FCOSHead):
    def __init__(self, num_classes, in_channels, feat_channels=256, stacked_convs=4, strides=(4, 8, 16, 32, 64),
                 conv_bias="auto", regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512), (512, INF)),
                 center_sampling=False, center_sample_radius=1.5, norm_on_bbox=False, centerness_on_reg=False,
                 scale_theta=True, crop_size=(768, 768), rotation_agnostic_classes=None, rect_classes=None,
                 loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_bbox=dict(type="PolyIoULoss", loss_weight=1.0),
                 loss_centerness=dict(type="CrossEntropyLoss", use_bce=True, loss_weight=1.0),
                 loss_bbox_aug=dict(type="IoULoss", loss_weight=1.0),
                 norm_cfg=dict(type="GN", num_groups=32, is_train=True), test_cfg=None, conv_cfg=None):
        super().__init__(num_classes, in_channels, feat_channels=feat_channels, stacked_convs=stacked_convs,
                         strides=strides, conv_bias=conv_bias, regress_ranges=regress_ranges,
                         center_sampling=center_sampling, center_sample_radius=center_sample_radius,
                         norm_on_bbox=norm_on_bbox, centerness_on_reg=centerness_on_reg, scale_theta=scale_theta,
                         loss_cls=loss_cls, loss_bbox=loss_bbox, loss_centerness=loss_centerness, norm_cfg=norm_cfg,
                         test_cfg=test_cfg, conv_cfg=conv_cfg)
        self.loss_bbox_aug = build_from_cfg(loss_bbox_aug, LOSSES)
        self.crop_size = tuple(crop_size)
        self.rotation_agnostic_classes = list(rotation_agnostic_classes) if rotation_agnostic_classes else None
        self.rect_classes = list(rect_classes) if rect_classes else None

    # ---------------------------------------------------------------------------------------------------------- forward
    def obb2xyxy(self, rbboxes):
        """(n, 5) [cx, cy, w, h, a] -> the circumscribed horizontal boxes (n, 4) <x1, y1, x2, y2>"""
        w = rbboxes[:, 2::5]
        h = rbboxes[:, 3::5]
        a = rbboxes[:, 4::5]
        cosa = torch.cos(a).abs()
        sina = torch.sin(a).abs()
        hbbox_w = cosa * w + sina * h
        hbbox_h = sina * w + cosa * h
        dx = rbboxes[..., 0]
        dy = rbboxes[..., 1]
        dw = hbbox_w.reshape(-1)
        dh = hbbox_h.reshape(-1)
        return torch.stack((dx - dw / 2, dy - dh / 2, dx + dw / 2, dy + dh / 2), -1)

    def forward_aug_single(self, x, scale, stride):
        """the regression branch alone: the rotated view needs no scores and no centerness"""
        reg_feat = x
        for reg_layer in self.reg_convs:
            reg_feat = reg_layer(reg_feat)
        bbox_pred = scale(self.conv_reg(reg_feat))
        if self.norm_on_bbox:
            bbox_pred = torch.relu(bbox_pred)
            if not self.training:
                bbox_pred = bbox_pred * stride
        else:
            bbox_pred = bbox_pred.exp()
        theta_pred = self.conv_theta(reg_feat)
        if self.scale_theta:
            theta_pred = self.scale_t(theta_pred)
        return bbox_pred, theta_pred

    def forward_aug(self, feats):
        return multi_apply(self.forward_aug_single, feats, self.scales, self.strides)

    def execute_train(self, feats1, feats2, rot, targets):
        outs = multi_apply(self.forward_single, feats1, self.scales, self.strides)
        if not self.training:
            return self.get_bboxes(*outs, targets)
        outs_aug = self.forward_aug(feats2)
        return self.loss(outs, outs_aug, rot, targets)

    # ------------------------------------------------------------------------------------------------------------- loss
    def _process_rotation_agnostic(self, tensor, cls, dim=4):
        mask = torch.ones_like(tensor)
        for c in self.rotation_agnostic_classes:
            if dim is None:
                mask[cls == c] = 0
            else:
                mask[cls == c, dim] = 0
        return tensor * mask

    def _aug_dense_ok(self):
        from jdet_amd.models.losses.h2rbox_loss import H2RBoxLoss
        return isinstance(self.loss_bbox_aug, H2RBoxLoss) and self.loss_bbox_aug.dense_ok()

    def loss(self, outs, outs_aug, rot, targets):
        cls_scores, bbox_preds, theta_preds, centernesses = outs
        assert len(cls_scores) == len(bbox_preds) == len(centernesses)
        rot = float(torch.tensor(float(rot), dtype=torch.float32))    # rounded to float once: what the kernel receives
        featmap_sizes = [tuple(featmap.shape[-2:]) for featmap in cls_scores]
        all_level_points = self.get_points(featmap_sizes, bbox_preds[0].dtype, cls_scores[0].device)
        gt_bboxes_list = [t["rboxes"] for t in targets]
        gt_labels_list = [t["labels"] for t in targets]
        if cls_scores[0].is_cuda and bbox_preds[0].dtype == torch.float32 and self._aug_dense_ok() and \
                self._dense_ok(gt_bboxes_list, gt_labels_list):
            return self._loss_dense_aug(outs, outs_aug, rot, featmap_sizes, all_level_points, gt_bboxes_list,
                                        gt_labels_list)
        return self._loss_general(outs, outs_aug, rot, featmap_sizes, all_level_points, targets)

    # FCOSHead's box loss on the circumscribed horizontal boxes, with the reference's normalisers
    def _loss_bbox_dense(self, decoded_preds, decoded_targets, weight):
        return self.loss_bbox(self.obb2xyxy(decoded_preds), self.obb2xyxy(decoded_targets), weight=weight,
                              avg_factor=weight.sum().clamp(min=1e-6))

    def _loss_bbox_general(self, decoded_preds, decoded_targets, weight):
        return self.loss_bbox(self.obb2xyxy(decoded_preds), self.obb2xyxy(decoded_targets), weight=weight,
                              avg_factor=weight.sum().detach().clamp(min=1e-6))

    def _loss_dense_aug(self, outs, outs_aug, rot, featmap_sizes, all_level_points, gt_bboxes_list, gt_labels_list):
        """FCOSHead's dense losses + the consistency term in one launch over all points"""
        d = self._dense_parts(outs, outs_aug, featmap_sizes, all_level_points, gt_bboxes_list, gt_labels_list)
        loss_bbox_aug, _ = self.loss_bbox_aug.dense(featmap_sizes, self.strides, d.preds, d.preds_aug, d.centerness2d,
                                                    d.labels2d, self.rotation_agnostic_classes, rot, self.crop_size)
        return dict(d.losses, loss_bbox_aug=loss_bbox_aug)

    def _loss_general(self, outs, outs_aug, rot, featmap_sizes, all_level_points, targets):
        """FCOSHead's general losses + the consistency term on the positives whose cell lies inside view two"""
        bbox_preds_aug, theta_preds_aug = outs_aug
        num_imgs = outs[0][0].size(0)
        g = self._general_parts(outs, all_level_points, targets)
        losses, pos_inds, pos_bbox_preds, flatten_points = g.losses, g.pos_inds, g.pos_bbox_preds, g.flatten_points
        pos_decoded_bbox_preds, pos_centerness_targets = g.pos_decoded_bbox_preds, g.pos_centerness_targets
        if len(pos_inds) == 0:
            return dict(losses, loss_bbox_aug=losses["loss_bbox"])
        cosa, sina = math.cos(rot), math.sin(rot)
        tf_T = torch.tensor([[cosa, sina], [-sina, cosa]], dtype=torch.float32, device=pos_inds.device)
        tf_T = tf_T.to(pos_bbox_preds.dtype)
        pos_inds_aug = []
        pos_inds_aug_v = torch.zeros(pos_inds.shape, dtype=torch.bool, device=pos_inds.device)
        offset = 0
        for h, w in featmap_sizes:
            level_mask = (offset <= pos_inds) & (pos_inds < offset + num_imgs * h * w)
            pos_ind = pos_inds[level_mask] - offset
            xy = torch.stack((pos_ind % w, (pos_ind // w) % h), dim=-1).to(tf_T.dtype)
            b = pos_ind // (w * h)
            ctr = torch.tensor([[(w - 1) / 2, (h - 1) / 2]], dtype=tf_T.dtype, device=tf_T.device)
            d = xy - ctr
            # (the 2x2 product written out, as the kernel: a matmul may fuse the multiply-adds); torch.round: half to even
            xy_aug = torch.stack([d[:, 0] * tf_T[0, 0] + d[:, 1] * tf_T[1, 0] + ctr[0, 0],
                                  d[:, 0] * tf_T[0, 1] + d[:, 1] * tf_T[1, 1] + ctr[0, 1]], dim=-1).round().long()
            x_aug = xy_aug[..., 0]
            y_aug = xy_aug[..., 1]
            xy_valid_aug = (x_aug >= 0) & (x_aug < w) & (y_aug >= 0) & (y_aug < h)
            pos_ind_aug = (b * h + y_aug) * w + x_aug
            pos_inds_aug_v[level_mask] = xy_valid_aug
            pos_inds_aug.append(pos_ind_aug[xy_valid_aug] + offset)
            offset += num_imgs * h * w
        if not bool(pos_inds_aug_v.any()):
            return dict(losses, loss_bbox_aug=pos_bbox_preds[:0].sum())
        pos_labels = g.focal_labels[pos_inds]
        pos_inds_aug = torch.cat(pos_inds_aug)
        flatten_bbox_preds_aug = torch.cat([b.permute(0, 2, 3, 1).reshape(-1, 4) for b in bbox_preds_aug])
        flatten_theta_preds_aug = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, 1) for t in theta_preds_aug])
        pos_bbox_preds_aug = torch.cat([flatten_bbox_preds_aug[pos_inds_aug], flatten_theta_preds_aug[pos_inds_aug]],
                                       dim=-1)
        pos_points_aug = flatten_points[pos_inds_aug]
        pos_decoded_bbox_preds_aug = distance2obb(pos_points_aug, pos_bbox_preds_aug)
        _h, _w = self.crop_size
        _ctr = flatten_points.new_tensor([[(_w - 1) / 2, (_h - 1) / 2]])
        _xy = pos_decoded_bbox_preds[pos_inds_aug_v, :2]
        _wh = pos_decoded_bbox_preds[pos_inds_aug_v, 2:4]
        pos_angle_targets_aug = pos_decoded_bbox_preds[pos_inds_aug_v, 4:] + rot
        d = _xy - _ctr
        _xy = torch.stack([d[:, 0] * tf_T[0, 0] + d[:, 1] * tf_T[1, 0] + _ctr[0, 0],
                           d[:, 0] * tf_T[0, 1] + d[:, 1] * tf_T[1, 1] + _ctr[0, 1]], dim=-1)
        if self.rotation_agnostic_classes:
            pos_labels_aug = pos_labels[pos_inds_aug_v]
            pos_angle_targets_aug = self._process_rotation_agnostic(pos_angle_targets_aug, pos_labels_aug, dim=None)
        pos_decoded_target_preds_aug = torch.cat([_xy, _wh, pos_angle_targets_aug], dim=-1)
        pos_centerness_targets_aug = pos_centerness_targets[pos_inds_aug_v]
        centerness_denorm_aug = pos_centerness_targets_aug.sum().detach().clamp(min=1.0)
        loss_bbox_aug = self.loss_bbox_aug(pos_decoded_bbox_preds_aug, pos_decoded_target_preds_aug,
                                           weight=pos_centerness_targets_aug, avg_factor=centerness_denorm_aug)
        return dict(losses, loss_bbox_aug=loss_bbox_aug)

    # -------------------------------------------------------------------------------------------------------- inference
    def _get_bboxes_single(self, *args, **kwargs):
        polys, scores, det_labels = super()._get_bboxes_single(*args, **kwargs)
        if self.rect_classes:
            for cid in self.rect_classes:
                inds = (det_labels == cid)[:, None]
                xmin = polys[:, ::2].min(1).values
                ymin = polys[:, 1::2].min(1).values
                xmax = polys[:, ::2].max(1).values
                ymax = polys[:, 1::2].max(1).values
                rect = torch.stack([xmin, ymin, xmin, ymax, xmax, ymax, xmax, ymin], dim=1)
                polys = torch.where(inds, rect, polys)
        return polys, scores, det_labels
