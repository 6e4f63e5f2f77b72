"""Knowledge-distillation losses.  Mirrors python/jdet/models/losses/kd_loss.py:L7-123.

KnowledgeDistillationKLDivLoss is the reference's `knowledge_distillation_kl_div_loss`: KLDivLoss with its default
reduction -- the mean over ALL elements, not over rows -- of log softmax(pred / T) against softmax(soft / T), times T^2,
over the rows of weight > 0; with a weight and NO row > 0 the reference falls through to every row (its zero loss is
overwritten two lines later), which levels without a positive anchor hit in every step.  `reduction` and `avg_factor`
are accepted and unused, as there.  Neither route compacts rows by a boolean mask or brings the count to the host."""
import torch
from torch import nn

from jdet_amd.utils.registry import LOSSES

from . import _level
from ._level import blocked_rows, loss_workspace


def _row_weight(weight, M):
    """the weight as (M,) / (blocks, rows_per_block) floats, one per row of pred: a view where the layout allows"""
    if weight.dim() > 1 and weight.numel() == M:
        return weight.flatten(1)        # a level's (B, n, 5) / (B, n) window: rows of one image stay contiguous
    return weight.reshape(-1)


def knowledge_distillation_kl_div_loss(pred, soft_label, weight=None, Tem=1, reduction="mean", avg_factor=None,
                                       detach_target=True):
    """the composed route (any device, any dtype): the selection is a mask multiply and the count stays a tensor.

    The rows are worked in float64 and the loss is rounded once.  The KL divergence of two nearly equal distributions is
    second order in their difference while t log t and t log p are not: in float32 an untrained student against an
    untrained teacher (logits of a few 1e-2, T = 10) loses the third digit of loss_LD to that cancellation."""
    assert pred.shape == soft_label.shape and pred.dim() == 2
    M, K = pred.shape
    out_dtype = pred.dtype
    pred, soft_label = pred.double(), soft_label.double()
    target = torch.softmax(soft_label / Tem, dim=1)
    if detach_target:
        target = target.detach()
    logp = torch.log_softmax(pred / Tem, dim=1)
    rows = (torch.xlogy(target, target) - target * logp).sum(dim=1)
    if weight is None:
        return (rows.sum() / float(M * K) * (Tem * Tem)).to(out_dtype)
    sel = weight.reshape(-1) > 0
    count = sel.sum()
    sel = sel | (count == 0)                                 # nothing selected -> every row, as the reference
    count = torch.where(count == 0, torch.full_like(count, M), count)
    total = torch.where(sel, rows, torch.zeros_like(rows)).sum()
    return (total / (count * K).to(rows.dtype) * (Tem * Tem)).to(out_dtype)


class _KLDivLevel(torch.autograd.Function):
    """loss_weight * knowledge_distillation_kl_div_loss of one pyramid level as ONE node (csrc/dist_loss.hip): pred / soft
    (M, K) contiguous, weight M floats behind a blocked index (a level's window, read in place) or None; the count of
    selected rows is saved on the device and the backward recomputes both softmaxes"""

    @staticmethod
    def forward(ctx, pred, soft, weight, T, loss_weight):
        from jdet_amd import _lib as L
        p, s = pred.contiguous(), soft.detach().contiguous()
        M, K = p.shape
        wb = blocked_rows(weight) if weight is not None else (1, 0)
        out = torch.empty((), dtype=torch.float32, device=p.device)
        count = torch.empty((1,), dtype=torch.int32, device=p.device)
        ws, wsb = loss_workspace(p.device)
        L.check(L.lib().jdet_kd_kl_div_level_forward(
            L.ptr(p), L.ptr(s), L.ptr(weight) if weight is not None else None, wb[0], wb[1], M, K, float(T),
            float(loss_weight), out.data_ptr(), count.data_ptr(), L.ptr(ws), wsb, L.stream_ptr(p)),
            "jdet_kd_kl_div_level_forward")
        ctx.save_for_backward(p, s, weight, count)
        ctx.args = (wb, float(T), float(loss_weight))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from jdet_amd import _lib as L
        p, s, weight, count = ctx.saved_tensors
        wb, T, loss_weight = ctx.args
        M, K = p.shape
        go = grad_out.to(torch.float32).contiguous()
        grad = torch.empty_like(p)
        L.check(L.lib().jdet_kd_kl_div_level_backward(
            L.ptr(p), L.ptr(s), L.ptr(weight) if weight is not None else None, wb[0], wb[1], M, K, T, loss_weight,
            count.data_ptr(), L.ptr(go), L.ptr(grad), L.stream_ptr(p)), "jdet_kd_kl_div_level_backward")
        return grad, None, None, None, None


def _kl_level_ok(pred, soft, weight):
    if not (_level.LEVEL_NODES and pred.is_cuda and pred.dtype == torch.float32 and soft.dtype == torch.float32 and
            pred.dim() == 2 and pred.numel() > 0 and pred.shape == soft.shape and pred.shape[1] <= 32 and
            not torch.is_autocast_enabled() and not soft.requires_grad):
        return False
    return weight is None or (weight.dtype == torch.float32 and not weight.requires_grad and
                              weight.numel() == pred.shape[0] and blocked_rows(weight) is not None)


@LOSSES.register_module()
class KnowledgeDistillationKLDivLoss(nn.Module):
    def __init__(self, reduction="mean", loss_weight=1.0, T=10):
        super().__init__()
        assert T >= 1
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.T = T

    def forward(self, pred, soft_label, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, "none", "mean", "sum")
        if weight is not None:
            weight = _row_weight(weight, pred.shape[0])
        if _kl_level_ok(pred, soft_label, weight):
            return _KLDivLevel.apply(pred, soft_label, weight, self.T, self.loss_weight)
        return self.loss_weight * knowledge_distillation_kl_div_loss(pred, soft_label, weight, Tem=self.T,
                                                                      detach_target=True)

    execute = forward


def im_loss(x, soft_target, reduction="mean"):
    return torch.nn.functional.mse_loss(x, soft_target)


@LOSSES.register_module()
class IMLoss(nn.Module):
    """feature imitation: loss_weight * mse_loss(x, soft_target), the elementwise mean (`reduction` is accepted and
    unused, as in the reference).  loss_weight == 0 -- the LD config -- returns a zero without touching the maps."""

    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, x, soft_target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, "none", "mean", "sum")
        if self.loss_weight == 0:
            return torch.zeros((), dtype=x.dtype, device=x.device)
        return self.loss_weight * im_loss(x, soft_target)

    execute = forward
