"""Polygon IoU loss of rotated boxes.  Mirrors python/jdet/models/losses/poly_iou_loss.py: shoelace L11-16, convex_areas
L19-36, poly_intersection L39-86, poly_iou_loss L97-123, PolyIoULoss L158-198 (PolyGIoULoss is not ported).

Two routes, same mathematics:
  general  the reference's tensor program on `ops.convex_sort`, differentiated by torch autograd (about 60 small ops
           over (P, 24, 2) point sets + the scan kernel);
  fused    one launch for loss and gradient (csrc/poly_iou_loss.hip: jdet_poly_iou_loss), taken for fp32 device
           tensors.  Rows of weight 0 skip the geometry there, so FCOSHead calls it over ALL points with the centerness
           target as weight instead of gathering the positives through nonzero()."""
import torch
from torch import nn

from jdet_amd import _lib as L
from jdet_amd.ops.bbox_transforms import bbox2type, get_bbox_areas
from jdet_amd.utils.registry import LOSSES


def shoelace(pts):
    roll_pts = torch.roll(pts, 1, dims=-2)
    xyxy = pts[..., 0] * roll_pts[..., 1] - roll_pts[..., 0] * pts[..., 1]
    return 0.5 * torch.abs(xyxy.sum(dim=-1))


def convex_areas(pts, masks):
    from jdet_amd.ops.convex_sort import convex_sort
    nbs, npts, _ = pts.size()
    index = convex_sort(pts.detach(), masks).long()
    index = torch.where(index == -1, torch.full_like(index, npts), index)
    index = index[..., None].repeat(1, 1, 2)
    ext_pts = torch.cat([pts, pts.new_zeros((nbs, 1, 2))], dim=1)
    polys = torch.gather(ext_pts, 1, index)
    xyxy = polys[:, 0:-1, 0] * polys[:, 1:, 1] - polys[:, 0:-1, 1] * polys[:, 1:, 0]
    return 0.5 * torch.abs(xyxy.sum(dim=-1))


def poly_intersection(pts1, pts2, areas1=None, areas2=None, eps=1e-6):
    """(B, 4, 2) x (B, 4, 2) -> the 16 edge-pair intersection points + both vertex sets (B, 24, 2) and the mask of
    those that bound the intersection (B, 24)"""
    lines1 = torch.cat([pts1, torch.roll(pts1, -1, dims=1)], dim=2)
    lines2 = torch.cat([pts2, torch.roll(pts2, -1, dims=1)], dim=2)
    lines1, lines2 = lines1.unsqueeze(2), lines2.unsqueeze(1)
    x1, y1, x2, y2 = lines1.unbind(dim=-1)      # (B, 4, 1)
    x3, y3, x4, y4 = lines2.unbind(dim=-1)      # (B, 1, 4)
    num = (x1 - x2) * (y3 - y4) - (y1 - y2) * (x3 - x4)
    den_t = (x1 - x3) * (y3 - y4) - (y1 - y3) * (x3 - x4)
    with torch.no_grad():
        den_u = (x2 - x1) * (y1 - y3) - (y2 - y1) * (x1 - x3)
        t, u = den_t / num, den_u / num
        mask_inter = (t > 0) & (t < 1) & (u > 0) & (u < 1)
    t = den_t / (num + eps)
    pts_inter = torch.stack([x1 + t * (x2 - x1), y1 + t * (y2 - y1)], dim=-1)
    B = pts1.size(0)
    pts_inter = pts_inter.view(B, -1, 2)
    mask_inter = mask_inter.view(B, -1)
    with torch.no_grad():
        areas1 = shoelace(pts1) if areas1 is None else areas1
        areas2 = shoelace(pts2) if areas2 is None else areas2
        triangle_areas1 = 0.5 * torch.abs((x3 - x1) * (y4 - y1) - (y3 - y1) * (x4 - x1))
        sum_areas1 = triangle_areas1.sum(dim=-1)
        mask_inside1 = torch.abs(sum_areas1 - areas2[..., None]) < 1e-3 * areas2[..., None]
        triangle_areas2 = 0.5 * torch.abs((x1 - x3) * (y2 - y3) - (x2 - x3) * (y1 - y3))
        sum_areas2 = triangle_areas2.sum(dim=-2)
        mask_inside2 = torch.abs(sum_areas2 - areas1[..., None]) < 1e-3 * areas1[..., None]
    all_pts = torch.cat([pts_inter, pts1, pts2], dim=1)
    masks = torch.cat([mask_inter, mask_inside1, mask_inside2], dim=1)
    return all_pts, masks


def _reduce(loss, reduction, avg_factor):
    if avg_factor is None:
        avg_factor = loss.numel()
    if reduction == "sum":
        return loss.sum()
    if reduction == "mean":
        return loss.sum() / avg_factor     # avg_factor: a host number or a device scalar
    return loss


def poly_iou_loss_general(pred, target, linear=False, eps=1e-6, weight=None, reduction="mean", avg_factor=None):
    """the reference's tensor program (device tensors: the hull step is ops.convex_sort)"""
    areas1, areas2 = get_bbox_areas(pred), get_bbox_areas(target)
    pred, target = bbox2type(pred, "poly"), bbox2type(target, "poly")
    pred_pts = pred.view(pred.size(0), -1, 2)
    target_pts = target.view(target.size(0), -1, 2)
    inter_pts, inter_masks = poly_intersection(pred_pts, target_pts, areas1, areas2, eps)
    overlap = convex_areas(inter_pts, inter_masks)
    ious = (overlap / (areas1 + areas2 - overlap + eps)).clamp(min=eps)
    loss = 1 - ious if linear else -ious.log()
    if weight is not None:
        loss = loss * weight
    return _reduce(loss, reduction, avg_factor)


class _FusedPolyIoU(torch.autograd.Function):
    """unreduced weighted loss (P,) + d loss / d pred in one launch; backward scales the stored gradient rows"""

    @staticmethod
    def forward(ctx, pred, target, weight, linear, eps):
        p, t = pred.contiguous(), target.contiguous()
        w = weight.contiguous() if weight is not None else None
        P = p.shape[0]
        loss = torch.empty((P,), dtype=torch.float32, device=p.device)
        grad = torch.empty((P, 5), dtype=torch.float32, device=p.device)
        L.check(L.lib().jdet_poly_iou_loss(L.ptr(p), L.ptr(t), L.ptr(w), P, int(bool(linear)), float(eps), L.ptr(loss),
                                           L.ptr(grad), L.stream_ptr(p)), "jdet_poly_iou_loss")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return grad * grad_out[:, None], None, None, None, None


def _fusable(pred, target, weight):
    ok = lambda t, n: t.is_cuda and t.dtype == torch.float32 and t.dim() == n  # noqa: E731
    return (ok(pred, 2) and ok(target, 2) and pred.shape == target.shape and pred.shape[1] == 5 and
            (weight is None or (ok(weight, 1) and weight.shape[0] == pred.shape[0] and not weight.requires_grad)) and
            not target.requires_grad and not torch.is_autocast_enabled())


def poly_iou_loss(pred, target, linear=False, eps=1e-6, weight=None, reduction="mean", avg_factor=None, fused=True):
    if fused and _fusable(pred, target, weight):
        return _reduce(_FusedPolyIoU.apply(pred, target, weight, linear, eps), reduction, avg_factor)
    return poly_iou_loss_general(pred, target, linear, eps, weight, reduction, avg_factor)


@LOSSES.register_module()
class PolyIoULoss(nn.Module):
    def __init__(self, linear=False, eps=1e-6, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.linear = linear
        self.eps = eps
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        if weight is not None and weight.dim() > 1:
            assert weight.shape == pred.shape
            weight = weight.mean(-1)
        return self.loss_weight * poly_iou_loss(pred, target, weight=weight, linear=self.linear, eps=self.eps,
                                                reduction=reduction, avg_factor=avg_factor, **kwargs)

    execute = forward
