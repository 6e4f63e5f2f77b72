"""The view-consistency loss of H2RBox.  Mirrors python/jdet/models/losses/h2rbox_loss.py:L6-66.

Two routes, same mathematics:
  general  the reference's tensor program on gathered (n, 5) rows: centre L1 + min(shape IoU + |sin da|, shape IoU of the
           swapped prediction + |cos da|), every sub-loss reduced to a SCALAR before the minimum;
  dense    `H2RBoxLoss.dense`, what H2RBoxHead's dense route calls: csrc/h2rbox_aug_loss.hip maps every view-1 point to
           its view-2 point, decodes both rows, builds the target and writes the three weighted terms per point in one
           launch (jdet_h2rbox_aug_loss_forward); the sums (float64), the scalar minimum and the average stay on the device; the
           backward pass is two launches (jdet_h2rbox_aug_loss_backward), gradient into BOTH views, deterministic."""
import ctypes
import math

import torch
from torch import nn

from jdet_amd import _lib as L
from jdet_amd.utils.registry import LOSSES, build_from_cfg


def _level_table(featmap_sizes, strides):
    nl = len(featmap_sizes)
    return (ctypes.c_int32 * (3 * nl))(*[int(v) for (h, w), s in zip(featmap_sizes, strides) for v in (h, w, s)]), nl


def _agnostic_list(classes):
    classes = [int(c) for c in (classes or ())]
    return ((ctypes.c_int32 * len(classes))(*classes) if classes else None), len(classes)


def h2rbox_aug_terms_device(featmap_sizes, strides, pred, pred_aug, weight, labels, agnostic, rot, crop_size,
                            shape_weight=1.0, angle_weight=1.0, eps=1e-6):
    """jdet_h2rbox_aug_loss_forward: pred / pred_aug (B, N, 5), weight (B, N), labels (B, N) int32 or None ->
    terms (B, N, 4) [centre, branch 1, branch 2, weight of a valid row], aug_index (B, N) int32"""
    L.need_device(pred, pred_aug, weight, labels)
    B, N = weight.shape
    lv, nl = _level_table(featmap_sizes, strides)
    ag, na = _agnostic_list(agnostic)
    assert N == sum(int(h) * int(w) for h, w in featmap_sizes) and pred.shape == pred_aug.shape == (B, N, 5)
    terms = torch.empty((B, N, 4), dtype=torch.float32, device=pred.device)
    aug_index = torch.empty((B, N), dtype=torch.int32, device=pred.device)
    L.check(L.lib().jdet_h2rbox_aug_loss_forward(
        lv, nl, L.ptr(pred), L.ptr(pred_aug), L.ptr(weight), L.ptr(labels) if na else None, ag, na, B, float(rot),
        math.cos(rot), math.sin(rot), int(crop_size[0]), int(crop_size[1]), float(shape_weight), float(angle_weight),
        float(eps), L.ptr(terms), L.ptr(aug_index), L.stream_ptr(pred)), "jdet_h2rbox_aug_loss_forward")
    return terms, aug_index


class _AugLoss(torch.autograd.Function):
    """loss (0-dim), aug_index (B, N) int32; everything between the kernel's terms and the loss stays on the device"""

    @staticmethod
    def forward(ctx, pred, pred_aug, weight, labels, featmap_sizes, strides, agnostic, rot, crop_size, centre_weight,
                shape_weight, angle_weight, loss_weight, eps):
        p, pa, w = pred.contiguous(), pred_aug.contiguous(), weight.contiguous()
        lab = labels.to(torch.int32).contiguous() if labels is not None else None
        terms, aug_index = h2rbox_aug_terms_device(featmap_sizes, strides, p, pa, w, lab, agnostic, rot, crop_size,
                                                   shape_weight, angle_weight, eps)
        # centre, branch 1, branch 2, weight of the valid rows: summed and combined in float64 (4 x B x N values, one
        # cast), so that the loss is the float32 nearest to the sum of the kernel's terms, whatever the summation order
        sums = terms.reshape(-1, 4).to(torch.float64).sum(dim=0)
        branch = (sums[2] < sums[1]).to(torch.int32).reshape(1)   # the SCALAR minimum, on the device
        avg = sums[3].clamp(min=1.0)
        loss = (loss_weight * (centre_weight * sums[0] + torch.minimum(sums[1], sums[2])) / avg).to(torch.float32)
        ctx.save_for_backward(p, pa, w, lab, aug_index, branch, avg)
        ctx.args = (featmap_sizes, strides, agnostic, rot, crop_size, centre_weight, shape_weight, angle_weight,
                    loss_weight, eps)
        ctx.mark_non_differentiable(aug_index)
        return loss, aug_index

    @staticmethod
    def backward(ctx, grad_out, _):
        p, pa, w, lab, aug_index, branch, avg = ctx.saved_tensors
        featmap_sizes, strides, agnostic, rot, crop_size, wc, ws, wa, lw, eps = ctx.args
        B, N = w.shape
        lv, nl = _level_table(featmap_sizes, strides)
        ag, na = _agnostic_list(agnostic)
        scale64 = grad_out.to(torch.float64) * lw / avg          # avg: float64, saved by forward
        scale = scale64.to(torch.float32).reshape(1)
        scale_centre = (scale64 * wc).to(torch.float32).reshape(1)
        grad_pred, grad_aug, contrib = torch.empty_like(p), torch.empty_like(pa), torch.empty_like(pa)
        L.check(L.lib().jdet_h2rbox_aug_loss_backward(
            lv, nl, L.ptr(p), L.ptr(pa), L.ptr(w), L.ptr(lab) if na else None, ag, na, B, float(rot), math.cos(rot),
            math.sin(rot), int(crop_size[0]), int(crop_size[1]), float(ws), float(wa), float(eps), L.ptr(aug_index),
            L.ptr(branch), L.ptr(scale_centre), L.ptr(scale), L.ptr(grad_pred), L.ptr(grad_aug), L.ptr(contrib),
            L.stream_ptr(p)), "jdet_h2rbox_aug_loss_backward")
        return (grad_pred, grad_aug) + (None,) * 12


@LOSSES.register_module()
class H2RBoxLoss(nn.Module):
    def __init__(self, center_loss_cfg, shape_loss_cfg, angle_loss_cfg, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.center_loss = build_from_cfg(center_loss_cfg, LOSSES)
        self.shape_loss = build_from_cfg(shape_loss_cfg, LOSSES)
        self.angle_loss = build_from_cfg(angle_loss_cfg, LOSSES)
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        """the general route: pred, target (n, 5) [cx, cy, w, h, a], weight (n,)"""
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        xy_pred = pred[..., :2]
        xy_target = target[..., :2]
        hbb_pred1 = torch.cat([-pred[..., 2:4], pred[..., 2:4]], dim=-1)
        hbb_pred2 = hbb_pred1[..., [1, 0, 3, 2]]
        hbb_target = torch.cat([-target[..., 2:4], target[..., 2:4]], dim=-1)
        d_a_pred = pred[..., 4:5] - target[..., 4:5]          # kept as a column: L1Loss weighs (n, k) rows by (n,)
        zeros = torch.zeros_like(d_a_pred)
        center_loss = self.center_loss(xy_pred, xy_target, weight=weight[:, None].expand_as(xy_pred),
                                       reduction_override=reduction, avg_factor=avg_factor)
        shape_loss1 = self.shape_loss(hbb_pred1, hbb_target, weight=weight, reduction_override=reduction,
                                      avg_factor=avg_factor) + \
            self.angle_loss(d_a_pred.sin(), zeros, weight=weight, reduction_override=reduction, avg_factor=avg_factor)
        shape_loss2 = self.shape_loss(hbb_pred2, hbb_target, weight=weight, reduction_override=reduction,
                                      avg_factor=avg_factor) + \
            self.angle_loss(d_a_pred.cos(), zeros, weight=weight, reduction_override=reduction, avg_factor=avg_factor)
        loss_bbox = center_loss + torch.minimum(shape_loss1, shape_loss2)
        return self.loss_weight * loss_bbox

    execute = forward

    def dense_ok(self):
        """whether `dense` computes this loss: the sub-losses of the reference's config, each averaged"""
        from .iou_loss import IoULoss
        from .smooth_l1_loss import L1Loss
        return (self.reduction == "mean" and isinstance(self.center_loss, L1Loss) and
                isinstance(self.shape_loss, IoULoss) and isinstance(self.angle_loss, L1Loss) and
                all(m.reduction == "mean" for m in (self.center_loss, self.shape_loss, self.angle_loss)))

    def dense(self, featmap_sizes, strides, pred, pred_aug, weight, labels, agnostic, rot, crop_size, eps=1e-6):
        """the dense route: pred / pred_aug (B, N, 5) [l, t, r, b, theta] of the two views in image-major order, weight
        (B, N) the centerness targets, labels (B, N) int32 0-based or None -> (loss, aug_index (B, N) int32);
        avg_factor is max(sum of the valid rows' weight, 1), taken on the device"""
        assert self.dense_ok()
        return _AugLoss.apply(pred, pred_aug, weight, labels, tuple(tuple(int(v) for v in s) for s in featmap_sizes),
                              tuple(int(s) for s in strides), tuple(agnostic or ()), float(rot), tuple(crop_size),
                              float(self.center_loss.loss_weight), float(self.shape_loss.loss_weight),
                              float(self.angle_loss.loss_weight), float(self.loss_weight), float(eps))
