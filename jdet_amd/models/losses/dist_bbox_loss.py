"""The regression loss of the distribution heads (roi_heads/rotated_retina_distribution_head.py): the integral over the
five discretised distributions of an anchor followed by L1Loss / SmoothL1Loss, as one node per pyramid level."""
import torch

from jdet_amd.models.boxes.box_ops import DIST_ANGLE_ENDS, DIST_ENDS, integral_rows

from . import _level
from ._level import blocked_rows, device_scalar, loss_workspace, scale_unit_grad
from .smooth_l1_loss import L1Loss, SmoothL1Loss, _flat_rows


class _DistBBoxLevel(torch.autograd.Function):
    """(sum w * l(integral(logits) - target) / avg_factor) * loss_weight of one level (csrc/dist_loss.hip): logits
    (rows, 5 * (reg_max + 1)) contiguous, target / weight (rows, 5) or (blocks, rows_per_block, 5) windows read in place"""

    @staticmethod
    def forward(ctx, logits, target, weight, reg_max, beta, avg_factor, loss_weight):
        from jdet_amd import _lib as L
        x = logits.contiguous()
        tb = blocked_rows(target, 5)
        wb = blocked_rows(weight, 5) if weight is not None else (1, 0)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        grad = torch.empty_like(x)
        ws, wsb = loss_workspace(x.device)
        L.check(L.lib().jdet_dist_bbox_loss_level(
            L.ptr(x), L.ptr(target), tb[0], tb[1], L.ptr(weight) if weight is not None else None, wb[0], wb[1],
            x.shape[0], int(reg_max), *DIST_ENDS, *DIST_ANGLE_ENDS, float(beta), L.ptr(avg_factor), float(loss_weight),
            out.data_ptr(), L.ptr(grad), L.ptr(ws), wsb, L.stream_ptr(x)), "jdet_dist_bbox_loss_level")
        ctx.save_for_backward(grad, avg_factor)
        ctx.loss_weight = float(loss_weight)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        grad, avg = ctx.saved_tensors
        return (scale_unit_grad(grad, grad_out, avg, ctx.loss_weight),) + (None,) * 6


def _level_ok(loss_fn, logits, target, weight, avg_factor, reg_max):
    if not (_level.LEVEL_NODES and isinstance(loss_fn, (L1Loss, SmoothL1Loss)) and loss_fn.reduction == "mean" and
            logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.numel() > 0 and
            logits.shape[1] == 5 * (reg_max + 1) and 1 <= reg_max < 32 and not torch.is_autocast_enabled() and
            device_scalar(avg_factor) and not target.requires_grad):
        return False
    for t in (target, weight):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.numel() != logits.shape[0] * 5 or blocked_rows(t, 5) is None:
            return False
    return True


def dist_bbox_loss(loss_fn, logits, target, weight, avg_factor, reg_max):
    """loss_fn(integral(logits), target, weight, avg_factor): the fused node where it applies (L1Loss / SmoothL1Loss with
    the mean reduction, fp32 on the device, a device avg_factor, JDET_LOSS_LEVEL_NODES), otherwise composed"""
    if _level_ok(loss_fn, logits, target, weight, avg_factor, reg_max):
        return _DistBBoxLevel.apply(logits, target, weight, reg_max, getattr(loss_fn, "beta", 0.0), avg_factor,
                                    loss_fn.loss_weight)
    return loss_fn(integral_rows(logits, reg_max), _flat_rows(target, 5), _flat_rows(weight, 5), avg_factor=avg_factor)
