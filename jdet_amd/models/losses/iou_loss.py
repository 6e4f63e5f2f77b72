"""IoU loss of horizontal boxes.  Mirrors python/jdet/models/losses/iou_loss.py: iou_loss L8-39, IoULoss L42-65.  A plain
elementwise tensor program (a dozen fused-free ops over (n, 4) rows): it is applied densely over all points by
H2RBoxHead with the centerness target as weight, and inside H2RBoxLoss's general route."""
import warnings

from torch import nn

from jdet_amd.models.boxes.iou_calculator import bbox_overlaps
from jdet_amd.utils.registry import LOSSES


def iou_loss(pred, target, weight=None, avg_factor=None, reduction="mean", linear=False, mode="log", eps=1e-6):
    assert mode in ["linear", "square", "log"]
    if linear:
        mode = "linear"
        warnings.warn('DeprecationWarning: Setting "linear=True" in iou_loss is deprecated, please use "mode=`linear`" '
                      "instead.")
    ious = bbox_overlaps(pred, target, is_aligned=True).clamp(min=eps)
    if mode == "linear":
        loss = 1 - ious
    elif mode == "square":
        loss = 1 - ious ** 2
    else:
        loss = -ious.log()
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        avg_factor = max(loss.shape[0], 1)
    if reduction == "mean":
        loss = loss.sum() / avg_factor         # avg_factor: a host number or a device scalar
    elif reduction == "sum":
        loss = loss.sum()
    return loss


@LOSSES.register_module()
class IoULoss(nn.Module):
    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * iou_loss(pred, target, weight, reduction=reduction, avg_factor=avg_factor)

    execute = forward
