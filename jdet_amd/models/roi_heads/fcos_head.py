"""Rotated FCOS head (anchor-free).  Mirrors python/jdet/models/roi_heads/fcos_head.py: Scale L14-27, FCOSHead L29-688
(constructor arguments, layer names and init are the reference's, so its checkpoints map by name).

Two routes for targets and loss, same values:
  dense    device fp32 tensors -- what every config hits.  ONE launch assigns all images and levels
           (csrc/fcos_targets.hip: jdet_fcos_targets, the gt counts read on the device); focal loss, polygon IoU loss
           and centerness BCE run over ALL points, the IoU loss weighted by the centerness target (zero rows skip
           the geometry in csrc/poly_iou_loss.hip), the counts stay on the device: no nonzero(), no host sync.
  general  the reference's tensor program per image ((points x gts) tensors, argmin, gathers) and its gather of the
           positives through nonzero().
Both routes return their losses together with the intermediates behind them (`_DenseLoss`, `_GeneralLoss`): H2RBoxHead
adds its consistency term to them and overrides only the box-loss hooks.  Padded gts and post-processing are the ones
every single-stage head shares (_dense_head_common.py).
Where the reference leaves a rule open or gets it wrong (ties, background targets, images without gts) both routes
follow include/jdet_hip.h."""
import ctypes
from collections import namedtuple

import torch
from torch import nn

from jdet_amd import _lib as L
from jdet_amd.models.boxes.box_ops import distance2obb, mintheta_obb
from jdet_amd.models.utils.modules import ConvModule
from jdet_amd.models.utils.weight_init import bias_init_with_prob, normal_init
from jdet_amd.utils.general import multi_apply
from jdet_amd.utils.registry import HEADS, LOSSES, build_from_cfg

from ._dense_head_common import _cfg, cut_level, device_counts, merge_levels, nms_polys, pad_gts, per_image

INF = 1e8

# what the shared part of a route hands to a subclass that adds a term (H2RBoxHead): the three losses and the
# intermediates they were computed from
_DenseLoss = namedtuple("_DenseLoss", "losses preds preds_aug labels2d centerness2d")
_GeneralLoss = namedtuple("_GeneralLoss", "losses pos_inds pos_bbox_preds pos_decoded_bbox_preds "
                                          "pos_centerness_targets focal_labels flatten_points")


def fcos_targets_device(featmap_sizes, strides, regress_ranges, gt, gt_labels, gt_count, num_classes, norm_on_bbox=False,
                        center_sampling=False, radius=1.5, with_inds=False):
    """jdet_fcos_targets: gt (B, Kmax, 5), gt_labels (B, Kmax) int32, gt_count (B) int32 on the device ->
    labels (B, N) int32, bbox_targets (B, N, 5), centerness (B, N) [, gt_inds (B, N) int32]"""
    L.need_device(gt, gt_labels, gt_count)
    B, Kmax = gt.shape[0], gt.shape[1]
    nl = len(featmap_sizes)
    N = sum(int(h) * int(w) for h, w in featmap_sizes)
    levels = (ctypes.c_int32 * (3 * nl))(*[int(v) for (h, w), s in zip(featmap_sizes, strides) for v in (h, w, s)])
    ranges = (ctypes.c_float * (2 * nl))(*[float(v) for r in regress_ranges for v in r])
    g, gl, gc = L.f32c(gt), gt_labels.to(torch.int32).contiguous(), gt_count.to(torch.int32).contiguous()
    dev = gc.device
    labels = torch.empty((B, N), dtype=torch.int32, device=dev)
    bbox_targets = torch.empty((B, N, 5), dtype=torch.float32, device=dev)
    centerness = torch.empty((B, N), dtype=torch.float32, device=dev)
    inds = torch.empty((B, N), dtype=torch.int32, device=dev) if with_inds else None
    L.check(L.lib().jdet_fcos_targets(levels, ranges, nl, L.ptr(g), L.ptr(gl), L.ptr(gc), B, Kmax, int(num_classes),
                                      int(bool(norm_on_bbox)), int(bool(center_sampling)), float(radius), L.ptr(labels),
                                      L.ptr(bbox_targets), L.ptr(centerness), L.ptr(inds), L.stream_ptr(gc)),
            "jdet_fcos_targets")
    return (labels, bbox_targets, centerness) + ((inds,) if with_inds else ())


class Scale(nn.Module):
    """a learnable scale factor (the reference keeps it as the attribute `scale`)"""

    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(float(scale)))

    def forward(self, x):
        return x * self.scale

    execute = forward


@HEADS.register_module()
class FCOSHead(nn.Module):
    def __init__(self, num_classes, in_channels, feat_channels=256, stacked_convs=4, strides=(4, 8, 16, 32, 64),
                 conv_bias="auto", regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512), (512, INF)),
                 center_sampling=False, center_sample_radius=1.5, norm_on_bbox=False, centerness_on_reg=False,
                 scale_theta=True,
                 loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_bbox=dict(type="PolyIoULoss", loss_weight=1.0),
                 loss_centerness=dict(type="CrossEntropyLoss", use_bce=True, loss_weight=1.0),
                 norm_cfg=dict(type="GN", num_groups=32, is_train=True), test_cfg=None, conv_cfg=None):
        super().__init__()
        self.regress_ranges = regress_ranges
        self.center_sampling = center_sampling
        self.center_sample_radius = center_sample_radius
        self.norm_on_bbox = norm_on_bbox
        self.centerness_on_reg = centerness_on_reg
        self.scale_theta = scale_theta
        self.num_classes = num_classes
        self.in_channels = in_channels
        self.feat_channels = feat_channels
        self.bbox_type = "obb"
        self.reg_dim = 4
        self.stacked_convs = stacked_convs
        self.strides = strides
        assert conv_bias == "auto" or isinstance(conv_bias, bool)
        self.conv_bias = conv_bias
        self.loss_cls = build_from_cfg(loss_cls, LOSSES)
        self.loss_bbox = build_from_cfg(loss_bbox, LOSSES)
        self.loss_centerness = build_from_cfg(loss_centerness, LOSSES)
        self.test_cfg = _cfg(test_cfg)
        self.conv_cfg = conv_cfg
        # (`is_train` is a Jittor GroupNorm argument)
        self.norm_cfg = {k: v for k, v in norm_cfg.items() if k != "is_train"} if norm_cfg is not None else None
        self.dense = True               # A/B switch of the two routes (tests)
        self._init_layers()

    def _init_layers(self):
        self._init_cls_convs()
        self._init_reg_convs()
        self._init_predictor()
        self.init_weights()

    def init_weights(self):
        for m in self.cls_convs:
            if isinstance(m.conv, nn.Conv2d):
                normal_init(m.conv, std=0.01)
        for m in self.reg_convs:
            if isinstance(m.conv, nn.Conv2d):
                normal_init(m.conv, std=0.01)
        bias_cls = bias_init_with_prob(0.01)
        normal_init(self.conv_cls, std=0.01, bias=bias_cls)
        normal_init(self.conv_reg, std=0.01)
        normal_init(self.conv_centerness, std=0.01)
        normal_init(self.conv_theta, std=0.01)

    def _tower(self):
        convs = nn.ModuleList()
        for i in range(self.stacked_convs):
            chn = self.in_channels if i == 0 else self.feat_channels
            convs.append(ConvModule(chn, self.feat_channels, 3, stride=1, padding=1, conv_cfg=self.conv_cfg,
                                    norm_cfg=self.norm_cfg, bias=self.conv_bias))
        return convs

    def _init_cls_convs(self):
        self.cls_convs = self._tower()

    def _init_reg_convs(self):
        self.reg_convs = self._tower()

    def _init_predictor(self):
        self.conv_cls = nn.Conv2d(self.feat_channels, self.num_classes, 3, padding=1)
        self.conv_reg = nn.Conv2d(self.feat_channels, self.reg_dim, 3, padding=1)
        self.conv_centerness = nn.Conv2d(self.feat_channels, 1, 3, padding=1)
        self.conv_theta = nn.Conv2d(self.feat_channels, 1, 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in self.strides])
        if self.scale_theta:
            self.scale_t = Scale(1.0)

    def forward(self, feats, targets):
        feats = multi_apply(self.forward_single, feats, self.scales, self.strides)
        if self.training:
            return self.loss(*feats, targets)
        return self.get_bboxes(*feats, targets)

    execute = forward

    def forward_single(self, x, scale, stride):
        cls_feat = x
        reg_feat = x
        for cls_layer in self.cls_convs:
            cls_feat = cls_layer(cls_feat)
        cls_score = self.conv_cls(cls_feat)
        for reg_layer in self.reg_convs:
            reg_feat = reg_layer(reg_feat)
        bbox_pred = self.conv_reg(reg_feat)
        if self.centerness_on_reg:
            centerness = self.conv_centerness(reg_feat)
        else:
            centerness = self.conv_centerness(cls_feat)
        bbox_pred = scale(bbox_pred)
        if self.norm_on_bbox:
            bbox_pred = torch.relu(bbox_pred)
            if not self.training:
                bbox_pred = bbox_pred * stride
        else:
            bbox_pred = bbox_pred.exp()
        theta_pred = self.conv_theta(reg_feat)
        if self.scale_theta:
            theta_pred = self.scale_t(theta_pred)
        return cls_score, bbox_pred, theta_pred, centerness

    # ------------------------------------------------------------------------------------------------ points, targets
    def get_points(self, featmap_sizes, dtype, device=None, flatten=False):
        return [self._get_points_single(featmap_sizes[i], self.strides[i], dtype, device)
                for i in range(len(featmap_sizes))]

    def _get_points_single(self, featmap_size, stride, dtype, device=None):
        h, w = featmap_size
        x_range = torch.arange(w, dtype=dtype, device=device)
        y_range = torch.arange(h, dtype=dtype, device=device)
        y, x = torch.meshgrid(y_range, x_range, indexing="ij")
        return torch.stack((x.flatten() * stride, y.flatten() * stride), dim=-1) + stride // 2

    def _dense_ok(self, gt_bboxes_list, gt_labels_list):
        return self.dense and all(g.is_cuda and g.dtype == torch.float32 and g.dim() == 2 and g.shape[-1] == 5
                                  for g in gt_bboxes_list) and all(t.is_cuda for t in gt_labels_list)

    def _dense_targets(self, featmap_sizes, gt_bboxes_list, gt_labels_list):
        """labels (B, N) int32, bbox_targets (B, N, 5), centerness (B, N): one launch, image-major"""
        gt, gl, counts = pad_gts(gt_bboxes_list, gt_labels_list, 5)
        return fcos_targets_device(featmap_sizes, self.strides, self.regress_ranges, gt, gl,
                                   device_counts(counts, gt.device), self.num_classes, self.norm_on_bbox,
                                   self.center_sampling, self.center_sample_radius)

    def get_targets(self, points, targets, dense=True, featmap_sizes=None):
        """labels and [l, t, r, b, theta] targets of every level, the images concatenated inside a level"""
        assert len(points) == len(self.regress_ranges)
        num_levels = len(points)
        num_points = [center.size(0) for center in points]
        gt_bboxes_list = [t["rboxes"] for t in targets]
        gt_labels_list = [t["labels"] for t in targets]
        if dense and points[0].is_cuda and self._dense_ok(gt_bboxes_list, gt_labels_list):
            # the kernel rebuilds a point from its index: it needs the lattice (H, W, stride), not the point list
            sizes = featmap_sizes or [self._lattice(p, s) for p, s in zip(points, self.strides)]
            labels, bbox_targets, _ = self._dense_targets(sizes, gt_bboxes_list, gt_labels_list)
            flat = lambda t: t.reshape(-1, *t.shape[2:])  # noqa: E731
            return ([flat(t) for t in torch.split(labels, num_points, dim=1)],
                    [flat(t) for t in torch.split(bbox_targets, num_points, dim=1)])
        expanded_regress_ranges = [
            points[i].new_tensor(self.regress_ranges[i])[None].expand_as(points[i]) for i in range(num_levels)]
        concat_regress_ranges = torch.cat(expanded_regress_ranges, dim=0)
        concat_points = torch.cat(points, dim=0)
        labels_list, bbox_targets_list = multi_apply(self._get_target_single, gt_bboxes_list, gt_labels_list,
                                                     points=concat_points, regress_ranges=concat_regress_ranges,
                                                     num_points_per_lvl=num_points)
        labels_list = [labels.split(num_points, 0) for labels in labels_list]
        bbox_targets_list = [bbox_targets.split(num_points, 0) for bbox_targets in bbox_targets_list]
        concat_lvl_labels = []
        concat_lvl_bbox_targets = []
        for i in range(num_levels):
            concat_lvl_labels.append(torch.cat([labels[i] for labels in labels_list]))
            bbox_targets = torch.cat([bbox_targets[i] for bbox_targets in bbox_targets_list])
            if self.norm_on_bbox:
                bbox_targets = torch.cat([bbox_targets[:, :4] / self.strides[i], bbox_targets[:, 4:]], dim=1)
            concat_lvl_bbox_targets.append(bbox_targets)
        return concat_lvl_labels, concat_lvl_bbox_targets

    @staticmethod
    def _lattice(points, stride):
        """(H, W) of a level's point list when the caller did not pass `featmap_sizes` (one host read per level; `loss`
        never comes here)"""
        last = points[-1].tolist()
        w = int(round((last[0] - stride // 2) / stride)) + 1
        h = int(round((last[1] - stride // 2) / stride)) + 1
        assert h * w == points.shape[0]
        return (h, w)

    def _get_target_single(self, gt_bboxes, gt_labels, points, regress_ranges, num_points_per_lvl):
        """one image, the reference's tensor program (L599-670); background rows are zeroed, an image without gts is
        background everywhere (include/jdet_hip.h)"""
        num_points = points.size(0)
        num_gts = gt_labels.size(0)
        if num_gts == 0:
            return (torch.full((num_points,), self.num_classes, dtype=torch.int32, device=points.device),
                    gt_bboxes.new_zeros((num_points, 5)))
        areas = gt_bboxes[:, 2] * gt_bboxes[:, 3]
        areas = areas[None].repeat(num_points, 1)
        regress_ranges = regress_ranges[:, None, :].expand(num_points, num_gts, 2)
        points = points[:, None, :].expand(num_points, num_gts, 2)
        gt_bboxes = mintheta_obb(gt_bboxes)
        gt_bboxes = gt_bboxes[None].expand(num_points, num_gts, 5)
        gt_ctr, gt_wh, gt_thetas = torch.split(gt_bboxes, [2, 2, 1], dim=2)
        Cos, Sin = torch.cos(gt_thetas), torch.sin(gt_thetas)
        Matrix = torch.cat([Cos, -Sin, Sin, Cos], dim=-1).reshape(num_points, num_gts, 2, 2)
        offset = points - gt_ctr
        # (the 2x2 product written out: a batched matmul of this shape may fuse the multiply-adds)
        offset = torch.stack([Matrix[..., 0, 0] * offset[..., 0] + Matrix[..., 0, 1] * offset[..., 1],
                              Matrix[..., 1, 0] * offset[..., 0] + Matrix[..., 1, 1] * offset[..., 1]], dim=-1)
        W, H = gt_wh[..., 0], gt_wh[..., 1]
        offset_x, offset_y = offset[..., 0], offset[..., 1]
        left = W / 2 + offset_x
        right = W / 2 - offset_x
        top = H / 2 + offset_y
        bottom = H / 2 - offset_y
        bbox_targets = torch.stack((left, top, right, bottom), -1)
        inside_gt_bbox_mask = bbox_targets.min(-1).values > 0
        if self.center_sampling:
            radius = self.center_sample_radius
            stride = torch.zeros_like(offset)
            lvl_begin = 0
            for lvl_idx, num_points_lvl in enumerate(num_points_per_lvl):
                lvl_end = lvl_begin + num_points_lvl
                stride[lvl_begin:lvl_end] = self.strides[lvl_idx] * radius
                lvl_begin = lvl_end
            inside_center_bbox_mask = (offset.abs() < stride).all(dim=-1)
            inside_gt_bbox_mask = inside_center_bbox_mask & inside_gt_bbox_mask
        max_regress_distance = bbox_targets.max(-1).values
        inside_regress_range = ((max_regress_distance >= regress_ranges[..., 0])
                                & (max_regress_distance <= regress_ranges[..., 1]))
        ok = inside_gt_bbox_mask & inside_regress_range
        # smallest area among the survivors, equal areas to the LOWER index: the first minimum of (area, index)
        order = torch.arange(num_gts, device=areas.device)[None].expand(num_points, num_gts)
        best = torch.where(ok, areas, torch.full_like(areas, float("inf"))).min(dim=1, keepdim=True).values
        min_area_inds = torch.where(ok & (areas == best), order, torch.full_like(order, num_gts)).min(dim=1).values
        bg = min_area_inds == num_gts
        min_area_inds = torch.where(bg, torch.zeros_like(min_area_inds), min_area_inds)
        labels = gt_labels[min_area_inds].to(torch.int32) - 1
        labels = torch.where(bg, torch.full_like(labels, self.num_classes), labels)
        rows = torch.arange(num_points, device=areas.device)
        bbox_targets = torch.cat([bbox_targets[rows, min_area_inds], gt_thetas[rows, min_area_inds]], dim=1)
        bbox_targets = torch.where(bg[:, None], torch.zeros_like(bbox_targets), bbox_targets)
        return labels, bbox_targets

    def centerness_target(self, pos_bbox_targets):
        left_right = pos_bbox_targets[:, [0, 2]]
        top_bottom = pos_bbox_targets[:, [1, 3]]
        centerness_targets = (left_right.min(dim=-1).values / left_right.max(dim=-1).values) * (
            top_bottom.min(dim=-1).values / top_bottom.max(dim=-1).values)
        return torch.sqrt(centerness_targets)

    # ------------------------------------------------------------------------------------------------------------ loss
    def loss(self, cls_scores, bbox_preds, theta_preds, centernesses, targets):
        assert len(cls_scores) == len(bbox_preds) == len(centernesses)
        outs = (cls_scores, bbox_preds, theta_preds, centernesses)
        featmap_sizes = [tuple(featmap.shape[-2:]) for featmap in cls_scores]
        all_level_points = self.get_points(featmap_sizes, bbox_preds[0].dtype, cls_scores[0].device)
        gt_bboxes_list = [t["rboxes"] for t in targets]
        gt_labels_list = [t["labels"] for t in targets]
        if cls_scores[0].is_cuda and bbox_preds[0].dtype == torch.float32 and \
                self._dense_ok(gt_bboxes_list, gt_labels_list):
            return self._dense_parts(outs, None, featmap_sizes, all_level_points, gt_bboxes_list, gt_labels_list).losses
        return self._general_parts(outs, all_level_points, targets).losses

    # the two points where a subclass's box loss differs (H2RBoxHead: horizontal boxes, its own normaliser)
    def _loss_bbox_dense(self, decoded_preds, decoded_targets, weight):
        weight_sum = weight.sum()
        return self.loss_bbox(decoded_preds, decoded_targets, weight=weight,
                              avg_factor=torch.where(weight_sum > 0, weight_sum, torch.ones_like(weight_sum)))

    def _loss_bbox_general(self, decoded_preds, decoded_targets, weight):
        return self.loss_bbox(decoded_preds, decoded_targets, weight=weight, avg_factor=weight.sum(), fused=False)

    def _general_parts(self, outs, all_level_points, targets):
        """the reference's route: level-major rows, the positives gathered through nonzero().  Without positives the
        box and centerness losses are empty sums and the intermediates of the positives None."""
        cls_scores, bbox_preds, theta_preds, centernesses = outs
        num_imgs = cls_scores[0].size(0)
        labels, bbox_targets = self.get_targets(all_level_points, targets, dense=False)
        flatten_cls_scores = torch.cat([c.permute(0, 2, 3, 1).reshape(-1, self.num_classes) for c in cls_scores])
        flatten_bbox_preds = torch.cat([b.permute(0, 2, 3, 1).reshape(-1, 4) for b in bbox_preds])
        flatten_theta_preds = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, 1) for t in theta_preds])
        flatten_centerness = torch.cat([c.permute(0, 2, 3, 1).reshape(-1) for c in centernesses])
        flatten_labels = torch.cat(labels)
        flatten_bbox_targets = torch.cat(bbox_targets)
        flatten_points = torch.cat([points.repeat(num_imgs, 1) for points in all_level_points])
        flatten_bbox_preds = torch.cat([flatten_bbox_preds, flatten_theta_preds], dim=1)
        bg_class_ind = self.num_classes
        pos_inds = ((flatten_labels >= 0) & (flatten_labels < bg_class_ind)).nonzero().reshape(-1)
        num_pos = len(pos_inds)
        # FocalLoss: 1-based classes, 0 = background
        focal_labels = torch.where(flatten_labels == bg_class_ind, torch.zeros_like(flatten_labels), flatten_labels + 1)
        loss_cls = self.loss_cls(flatten_cls_scores, focal_labels, avg_factor=num_pos + num_imgs)
        pos_bbox_preds = flatten_bbox_preds[pos_inds]
        pos_centerness = flatten_centerness[pos_inds]
        if num_pos == 0:
            losses = dict(loss_cls=loss_cls, loss_bbox=pos_bbox_preds.sum(), loss_centerness=pos_centerness.sum())
            return _GeneralLoss(losses, pos_inds, pos_bbox_preds, None, None, focal_labels, flatten_points)
        pos_bbox_targets = flatten_bbox_targets[pos_inds]
        pos_centerness_targets = self.centerness_target(pos_bbox_targets)
        pos_points = flatten_points[pos_inds]
        pos_decoded_bbox_preds = distance2obb(pos_points, pos_bbox_preds)
        pos_decoded_target_preds = distance2obb(pos_points, pos_bbox_targets)
        loss_bbox = self._loss_bbox_general(pos_decoded_bbox_preds, pos_decoded_target_preds, pos_centerness_targets)
        loss_centerness = self.loss_centerness(pos_centerness, pos_centerness_targets)
        losses = dict(loss_cls=loss_cls, loss_bbox=loss_bbox, loss_centerness=loss_centerness)
        return _GeneralLoss(losses, pos_inds, pos_bbox_preds, pos_decoded_bbox_preds, pos_centerness_targets,
                            focal_labels, flatten_points)

    def _dense_parts(self, outs, outs_aug, featmap_sizes, all_level_points, gt_bboxes_list, gt_labels_list):
        """every loss over all points in image-major order (the order jdet_fcos_targets writes); nothing leaves the
        device.  outs_aug: (bbox_preds, theta_preds) of a second view (H2RBoxHead) or None: flattened alike."""
        cls_scores, bbox_preds, theta_preds, centernesses = outs
        B = cls_scores[0].size(0)
        rows = lambda ts, c: torch.cat([t.permute(0, 2, 3, 1).reshape(B, -1, c) for t in ts], dim=1)  # noqa: E731
        flatten_cls_scores = rows(cls_scores, self.num_classes).reshape(-1, self.num_classes)
        preds = torch.cat([rows(bbox_preds, 4), rows(theta_preds, 1)], dim=2)                 # (B, N, 5)
        preds_aug = None if outs_aug is None else torch.cat([rows(outs_aug[0], 4), rows(outs_aug[1], 1)], dim=2)
        flatten_bbox_preds = preds.reshape(-1, 5)
        flatten_centerness = rows(centernesses, 1).reshape(-1)
        labels2d, bbox_targets, centerness2d = self._dense_targets(featmap_sizes, gt_bboxes_list, gt_labels_list)
        labels, bbox_targets, centerness_targets = labels2d.reshape(-1), bbox_targets.reshape(-1, 5), \
            centerness2d.reshape(-1)
        flatten_points = torch.cat(all_level_points).repeat(B, 1)
        pos = (labels >= 0) & (labels < self.num_classes)      # the general route's predicate
        num_pos = pos.sum().to(torch.float32)
        focal_labels = torch.where(pos, labels + 1, torch.zeros_like(labels))
        loss_cls = self.loss_cls(flatten_cls_scores, focal_labels, avg_factor=(num_pos + B).reshape(1))
        decoded_preds = distance2obb(flatten_points, flatten_bbox_preds)
        decoded_targets = distance2obb(flatten_points, bbox_targets)
        loss_bbox = self._loss_bbox_dense(decoded_preds, decoded_targets, centerness_targets)
        loss_centerness = self.loss_centerness(flatten_centerness, centerness_targets, weight=pos.to(torch.float32),
                                               avg_factor=num_pos.clamp(min=1.0))
        losses = dict(loss_cls=loss_cls, loss_bbox=loss_bbox, loss_centerness=loss_centerness)
        return _DenseLoss(losses, preds, preds_aug, labels2d, centerness2d)

    # ------------------------------------------------------------------------------------------------------- inference
    def get_bboxes(self, cls_scores, bbox_preds, theta_preds, centernesses, targets, rescale=True):
        assert len(cls_scores) == len(bbox_preds)
        featmap_sizes = [tuple(featmap.shape[-2:]) for featmap in cls_scores]
        mlvl_points = self.get_points(featmap_sizes, bbox_preds[0].dtype, cls_scores[0].device)
        return per_image(lambda b, *levels: self._get_bboxes_single(
            *levels, mlvl_points, targets[b]["img_size"], targets[b]["scale_factor"], rescale), len(targets),
            cls_scores, bbox_preds, theta_preds, centernesses)

    def _level_scores(self, cls_score, centerness):
        """a level's (C, H, W) and (1, H, W) maps -> (scores (n, C), centerness (n,) with the cfg's `centerness_factor`
        added, rank); rank() is the score the `nms_pre` cut ranks the rows by: the best class score times the
        centerness"""
        scores = cls_score.permute(1, 2, 0).reshape(-1, self.num_classes).sigmoid()
        centerness = centerness.permute(1, 2, 0).reshape(-1).sigmoid()
        centerness = centerness + self.test_cfg.get("centerness_factor", 0.)
        return scores, centerness, lambda: (scores * centerness[:, None]).max(dim=1).values

    def _get_bboxes_single(self, cls_scores, bbox_preds, theta_preds, centernesses, mlvl_points, img_shape, scale_factor,
                           rescale=False):
        cfg = self.test_cfg
        assert len(cls_scores) == len(bbox_preds) == len(mlvl_points)
        mlvl_bboxes, mlvl_scores, mlvl_centerness = [], [], []
        for cls_score, bbox_pred, theta_pred, centerness, points in zip(cls_scores, bbox_preds, theta_preds,
                                                                        centernesses, mlvl_points):
            assert cls_score.shape[-2:] == bbox_pred.shape[-2:]
            scores, centerness, rank = self._level_scores(cls_score, centerness)
            theta_pred = theta_pred.permute(1, 2, 0).reshape(-1, 1)
            bbox_pred = bbox_pred.permute(1, 2, 0).reshape(-1, 4)
            bbox_pred = torch.cat([bbox_pred, theta_pred], dim=1)
            bbox_pred, scores, points, centerness = cut_level(cfg.get("nms_pre", -1), rank, bbox_pred, scores, points,
                                                              centerness)
            mlvl_bboxes.append(distance2obb(points, bbox_pred, max_shape=img_shape))
            mlvl_scores.append(scores)
            mlvl_centerness.append(centerness)
        return nms_polys(*merge_levels(mlvl_bboxes, mlvl_scores, scale_factor, rescale, True, mlvl_centerness), cfg)
