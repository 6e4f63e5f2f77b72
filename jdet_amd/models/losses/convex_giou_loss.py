"""Convex GIoU loss of RepPoints point sets.  Mirrors python/jdet/models/losses/convex_giou_loss.py:
ConvexGIoULossFunction L7-58, ConvexGIoULoss L62-110.

Two routes, same per-row values:
  general  the rows it is given (the head gathered the positives through nonzero()): `reppoints_convex_giou`
           (jdet_convex_giou) for the GIoU and its raw gradient, then the reference's rule in torch -- weight, rows with
           a component > 1 set to 1e-6 (L47-48), negated (L51).  `forward` returns early with `(pred * weight).sum()`
           when no weight is > 0 (L103-104; one host read, as in the reference).
  dense    `dense(pred, target, weight, norm, avg_factor)`: ALL rows of a stage in one launch (csrc/convex_giou_loss.hip:
           jdet_convex_giou_loss); the division by the normalising term, the rule and the chain rule through the
           division happen in the kernel, rows of weight 0 skip the geometry, the count of positives is a device tensor
           the caller clamps to >= 1.  No nonzero(), no host sync.

Differences from the reference, on purpose:
  - its `Function.grad` ignores the incoming gradient and returns the stored rows; the nodes here multiply the stored
    rows by the incoming gradient, as torch requires.  With an incoming gradient of 1 the two agree.
  - `loss_weight` appears twice there (inside the stored gradient, L51, and on the forward value, L108); that amounts to
    the forward value carrying it once and the gradient carrying it once, which is what `loss_weight * reduce(node)`
    gives here.  The stored gradient's division by avg_factor (L51) likewise is the derivative of the 'mean' reduction."""
import torch
from torch import nn

from jdet_amd import _lib as L
from jdet_amd.ops.reppoints_convex_iou import reppoints_convex_giou
from jdet_amd.utils.registry import LOSSES


def convex_giou_rows(pred, target, weight=None):
    """unreduced (loss (P,), d loss / d pred (P, 18)) of the general route: L31-36, L47-48 and the sign of L51"""
    gious, grad = reppoints_convex_giou(pred, target)
    loss = 1 - gious
    if weight is not None:
        loss = loss * weight
        grad = grad * weight.reshape(-1, 1)
    invalid = (grad > 1).any(dim=1, keepdim=True)
    grad = torch.where(invalid, torch.full_like(grad, 1e-6), grad)
    return loss, -grad


class _ConvexGIoURows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight):
        loss, grad = convex_giou_rows(pred.detach(), target, weight)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return grad * grad_out[:, None], None, None


def convex_giou_loss_dense_rows(pred, target, weight, norm):
    """jdet_convex_giou_loss on device tensors: pred (P, 18), target (P, 8), weight (P), norm (P) ->
    (loss (P,), d loss / d pred (P, 18))"""
    L.need_device(pred, target, weight, norm)
    p, t, w, n = L.f32c(pred), L.f32c(target), L.f32c(weight), L.f32c(norm)
    P = p.shape[0]
    assert p.dim() == 2 and p.shape[1] == 18 and tuple(t.shape) == (P, 8) and w.numel() == P and n.numel() == P
    loss = torch.empty((P,), dtype=torch.float32, device=p.device)
    grad = torch.empty((P, 18), dtype=torch.float32, device=p.device)
    L.check(L.lib().jdet_convex_giou_loss(L.ptr(p), L.ptr(t), L.ptr(w), L.ptr(n), P, L.ptr(loss), L.ptr(grad),
                                          L.stream_ptr(p)), "jdet_convex_giou_loss")
    return loss, grad


class _ConvexGIoUDense(torch.autograd.Function):
    """unreduced weighted loss (P,) + d loss / d pred in one launch; backward scales the stored gradient rows"""

    @staticmethod
    def forward(ctx, pred, target, weight, norm):
        loss, grad = convex_giou_loss_dense_rows(pred.detach(), target, weight, norm)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return grad * grad_out[:, None], None, None, None


def _reduce(loss, reduction, avg_factor):
    if avg_factor is None:
        avg_factor = max(loss.shape[0], 1)
    if reduction == "sum":
        return loss.sum()
    if reduction == "mean":
        return loss.sum() / avg_factor
    return loss


@LOSSES.register_module()
class ConvexGIoULoss(nn.Module):
    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        if weight is not None and not bool(torch.any(weight > 0)):
            return (pred * weight.unsqueeze(-1)).sum()
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * _reduce(_ConvexGIoURows.apply(pred, target, weight), reduction, avg_factor)

    execute = forward

    def dense_rows(self, pred, target, weight, norm):
        """the unreduced rows of the dense route (every row of a stage; see the module docstring); the caller reduces
        them per level with `reduce_dense`"""
        return _ConvexGIoUDense.apply(pred, target, weight, norm)

    def reduce_dense(self, rows, num_pos):
        """'mean' over the positives of one level: num_pos is a device tensor, clamped to >= 1 here (the general route
        returns 0 for a level without positives, and so does this: every row is 0 there)"""
        return self.loss_weight * (rows.sum() / num_pos.to(torch.float32).clamp(min=1.0))

    def dense(self, pred, target, weight, norm, avg_factor=None):
        rows = self.dense_rows(pred, target, weight, norm)
        if avg_factor is None:
            avg_factor = (weight > 0).sum()
        return self.reduce_dense(rows, avg_factor)
