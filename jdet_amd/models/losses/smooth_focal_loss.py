"""Smooth focal loss of Circular Smooth Label.  Mirrors python/jdet/models/losses/smooth_focal_loss.py: the focal loss
on soft targets, `weight` used as a row mask only, sum / avg_factor -- and, for CSLRRetinaHead, the whole angle term of
a pyramid level (CSLCoder.encode + this loss) as one node that never stores a label (csrc/csl.hip)."""
import torch
from torch import nn

from jdet_amd.models.boxes import coder as _coder
from jdet_amd.utils.registry import LOSSES

from . import _level
from ._level import blocked_rows, device_scalar, loss_workspace, scale_unit_grad
from .focal_loss import binary_cross_entropy_with_logits
from .smooth_l1_loss import _flat_rows


def smooth_focal_loss(pred, target, gamma=2.0, alpha=0.25, reduction="mean", avg_factor=None):
    pred_sigmoid = pred.sigmoid()
    target = target.type_as(pred)
    pt = (1 - pred_sigmoid) * target + pred_sigmoid * (1 - target)
    focal_weight = (alpha * target + (1 - alpha) * (1 - target)) * pt.pow(gamma)
    loss = binary_cross_entropy_with_logits(pred, target, weight=None, reduction="none") * focal_weight
    if reduction == "mean":
        loss = loss.sum() / (avg_factor if avg_factor is not None else max(loss.numel(), 1))
    elif reduction == "sum":
        loss = loss.sum()
    return loss


@LOSSES.register_module()
class SmoothFocalLoss(nn.Module):
    def __init__(self, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.gamma = gamma
        self.alpha = alpha
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        """pred, target (n, coding_len); weight (n,) or (n, k): the rows with (mean) weight > 0 count, the value of the
        weight does not"""
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        if weight is not None:
            if weight.dim() > 1:
                weight = weight.mean(-1)
            mask = (weight > 0).detach()
            if reduction != "none" and not bool(mask.any()):
                # the reference's early return: the value 0 with the graph kept
                return (pred[mask] * weight[mask].reshape(-1, 1)).sum()
            pred = pred[mask]
            target = target[mask]
        return self.loss_weight * smooth_focal_loss(pred, target, gamma=self.gamma, alpha=self.alpha,
                                                    reduction=reduction, avg_factor=avg_factor)

    execute = forward


class _CSLAngleLevel(torch.autograd.Function):
    """(sum over the selected rows of smooth_focal(logits, label(target[:, 4])) / avg_factor) * loss_weight of one level
    (csrc/csl.hip: jdet_csl_angle_loss_level): logits (rows, coding_len) contiguous, target / weight the level's
    (rows, 5) or (blocks, rows_per_block, 5) bbox_targets / bbox_weights windows, column 4 read in place"""

    @staticmethod
    def forward(ctx, logits, target, weight, coder, gamma, alpha, avg_factor, loss_weight):
        from jdet_amd import _lib as L
        x = logits.contiguous()
        tb, wb = blocked_rows(target, 5), blocked_rows(weight, 5)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        grad = torch.empty_like(x)
        ws, wsb = loss_workspace(x.device)
        L.check(L.lib().jdet_csl_angle_loss_level(
            L.ptr(x), L.ptr(target), tb[0], tb[1], L.ptr(weight), wb[0], wb[1], x.shape[0], x.shape[1],
            float(coder.omega), L.CSL_WINDOWS[coder.window], float(coder.radius), float(gamma), float(alpha),
            L.ptr(avg_factor), float(loss_weight), out.data_ptr(), L.ptr(grad), L.ptr(ws), wsb, L.stream_ptr(x)),
            "jdet_csl_angle_loss_level")
        ctx.save_for_backward(grad, avg_factor)
        ctx.loss_weight = float(loss_weight)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        grad, avg = ctx.saved_tensors
        return (scale_unit_grad(grad, grad_out, avg, ctx.loss_weight),) + (None,) * 7


def _level_ok(loss_fn, coder, logits, target, weight, avg_factor):
    if not (_level.LEVEL_NODES and _coder.CSL_FUSED and isinstance(loss_fn, SmoothFocalLoss) and
            loss_fn.reduction == "mean" and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and
            logits.numel() > 0 and logits.shape[1] == coder.coding_len and 1 <= coder.coding_len <= 180 and
            (loss_fn.gamma == 0 or loss_fn.gamma >= 1) and not torch.is_autocast_enabled() and
            device_scalar(avg_factor) and avg_factor.device == logits.device and not target.requires_grad):
        return False
    for t in (target, weight):
        if (t is None or t.device != logits.device or t.dtype != torch.float32 or t.numel() != logits.shape[0] * 5 or
                blocked_rows(t, 5) is None):
            return False
    return True


def csl_angle_loss(loss_fn, coder, logits, bbox_targets, bbox_weights, avg_factor):
    """loss_fn(logits, coder.encode(bbox_targets[..., 4:5]), weight=bbox_weights[..., 4], avg_factor): the fused node where
    it applies (JDET_LOSS_LEVEL_NODES, JDET_CSL_FUSED, SmoothFocalLoss with the mean reduction, fp32 on the device, a
    device avg_factor, targets and weights on the logits' device, 1 <= coding_len <= 180, gamma 0 or >= 1, blocked
    windows), otherwise composed -- the reference's tensor program, which also runs on CPU tensors"""
    if _level_ok(loss_fn, coder, logits, bbox_targets, bbox_weights, avg_factor):
        return _CSLAngleLevel.apply(logits, bbox_targets, bbox_weights, coder, loss_fn.gamma, loss_fn.alpha, avg_factor,
                                    loss_fn.loss_weight)
    target, weight = _flat_rows(bbox_targets, 5), _flat_rows(bbox_weights, 5)
    return loss_fn(logits, coder.encode(target[:, 4:5]), weight=weight[:, 4], avg_factor=avg_factor)
