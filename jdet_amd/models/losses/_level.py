"""What the per-level loss nodes share (focal_loss._FocalLevel, smooth_l1_loss._SmoothL1Level,
gaussian_dist_loss.GaussianLevel): one autograd node per (pyramid level, loss), targets read in place through their
column windows, `/ avg_factor` and `* loss_weight` inside the finishing launch, one scaling launch in backward."""
import os

import torch

# one autograd node per (level, loss) with the targets read in place (A/B switch; profiles/r06_glue.md)
LEVEL_NODES = os.environ.get("JDET_LOSS_LEVEL_NODES", "1") == "1"


def blocked_rows(t, inner=1):
    """(rows_per_block, block_stride) of `t` -- a (rows,) / (blocks, rows_per_block) array [with `inner` trailing contiguous
    values per row] whose rows of one block are contiguous -- or None.  A level's window [:, s:e] of the per-image target
    arrays is such an array: the level-loss kernels read it in place (include/jdet_hip.h: jdet_*_loss_level)."""
    shape, st = tuple(t.shape), t.stride()
    if inner > 1:
        if not shape or shape[-1] != inner or st[-1] != 1:
            return None
        shape, st = shape[:-1], st[:-1]
        if any(x % inner for x in st):
            return None
        st = tuple(x // inner for x in st)
    if len(shape) == 1:
        return (shape[0], shape[0]) if shape[0] <= 1 or st[0] == 1 else None
    if len(shape) == 2 and (shape[1] <= 1 or st[1] == 1) and st[0] >= 0:
        return (shape[1], st[0]) if shape[0] > 1 else (shape[1], shape[1])
    return None


def device_scalar(x):
    """avg_factor as the 0-dim fp32 device tensor the level-loss kernels divide by (a host number keeps the composed path:
    the framework divides by a host scalar through its reciprocal, another rounding)"""
    return (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.numel() == 1 and not x.requires_grad)


def loss_workspace(device):
    """(workspace of the loss-sum entry points -- one query for all of them --, its size in bytes)"""
    from jdet_amd import _lib as L
    nbytes = L.lib().jdet_sigmoid_focal_loss_workspace()
    return torch.empty((nbytes,), dtype=torch.uint8, device=device), nbytes


def scale_unit_grad(unit_grad, grad_out, avg_factor, loss_weight):
    """backward of a level node: unit_grad * ((grad_out * loss_weight) / avg_factor) in one launch"""
    from jdet_amd import _lib as L
    go = grad_out.to(torch.float32).contiguous()
    out = torch.empty_like(unit_grad)
    L.check(L.lib().jdet_loss_grad_scale(L.ptr(unit_grad), unit_grad.numel(), L.ptr(go), L.ptr(avg_factor), loss_weight,
                                         L.ptr(out), L.stream_ptr(unit_grad)), "jdet_loss_grad_scale")
    return out
