"""`(lateral + nearest_upsample(top)) / div` as one launch per direction (csrc/upsample_add.hip): the top-down step of
the FPN (python/jdet/models/necks/fpn.py:L160-171)."""
import torch

from .. import _lib as L


class _UpsampleAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lateral, top, div):
        N, C, H, W = lateral.shape
        Ht, Wt = top.shape[2], top.shape[3]
        out = torch.empty_like(lateral, memory_format=torch.channels_last)
        L.check(L.lib().jdet_upsample_add_nhwc_forward(L.ptr(lateral), L.ptr(top), N, C, H, W, Ht, Wt, float(div),
                                                       L.ptr(out), L.stream_ptr(lateral)), "jdet_upsample_add_nhwc_forward")
        ctx.shape = (N, C, H, W, Ht, Wt, float(div))
        return out

    @staticmethod
    def backward(ctx, g):
        N, C, H, W, Ht, Wt, div = ctx.shape
        g = g.contiguous(memory_format=torch.channels_last)
        g_lat = g_top = None
        if ctx.needs_input_grad[0]:
            g_lat = g if div == 1.0 else g / div
        if ctx.needs_input_grad[1]:
            g_top = torch.empty((N, C, Ht, Wt), dtype=g.dtype, device=g.device, memory_format=torch.channels_last)
            L.check(L.lib().jdet_upsample_add_nhwc_backward(L.ptr(g), N, C, H, W, Ht, Wt, div, L.ptr(g_top),
                                                            L.stream_ptr(g)), "jdet_upsample_add_nhwc_backward")
        return g_lat, g_top, None


def fusable(lateral, top):
    """channels-last fp32 device maps with C % 4 == 0 (what the conv stack produces)"""
    return (lateral.is_cuda and top.is_cuda and lateral.dtype == torch.float32 and top.dtype == torch.float32
            and lateral.dim() == 4 and lateral.shape[1] % 4 == 0 and lateral.shape[:2] == top.shape[:2]
            and lateral.is_contiguous(memory_format=torch.channels_last)
            and top.is_contiguous(memory_format=torch.channels_last))


def upsample_add(lateral, top, div=1.0):
    """(lateral + top resampled to lateral's size by the nearest rule) / div"""
    return _UpsampleAdd.apply(lateral, top, div)


# ---- the bilinear merge of the RetinaNet-v1d configs: upsample_cfg = dict(mode="bilinear", tf_mode=True) -----------------
class _UpsampleAddBilinear(torch.autograd.Function):
    """csrc/upsample_add_bilinear.hip; the rule is stated in include/jdet_hip_retina.h"""

    @staticmethod
    def forward(ctx, lateral, top, div):
        N, C, H, W = lateral.shape
        Ht, Wt = top.shape[2], top.shape[3]
        out = torch.empty_like(lateral, memory_format=torch.channels_last)
        L.check(L.lib().jdet_upsample_add_bilinear_nhwc_forward(
            L.ptr(lateral), L.ptr(top), N, C, H, W, Ht, Wt, float(div), L.ptr(out), L.stream_ptr(lateral)),
            "jdet_upsample_add_bilinear_nhwc_forward")
        ctx.shape = (N, C, H, W, Ht, Wt, float(div))
        return out

    @staticmethod
    def backward(ctx, g):
        N, C, H, W, Ht, Wt, div = ctx.shape
        g = g.contiguous(memory_format=torch.channels_last)
        g_lat = g_top = None
        if ctx.needs_input_grad[0]:
            g_lat = g / div
        if ctx.needs_input_grad[1]:
            g_top = torch.empty((N, C, Ht, Wt), dtype=g.dtype, device=g.device, memory_format=torch.channels_last)
            L.check(L.lib().jdet_upsample_add_bilinear_nhwc_backward(
                L.ptr(g), N, C, H, W, Ht, Wt, div, L.ptr(g_top), L.stream_ptr(g)),
                "jdet_upsample_add_bilinear_nhwc_backward")
        return g_lat, g_top, None


def _tf_taps(out_size, in_size, device):
    """(i0, i1, d) of the tf_mode rule for every destination index, the coordinate in fp32 as the kernel computes it:
    x = float(i) * (float(in) / float(out)), clamped to [0, in - 1] when out > in"""
    scale = torch.tensor(in_size, dtype=torch.float32) / torch.tensor(out_size, dtype=torch.float32)
    x = torch.arange(out_size, dtype=torch.float32, device=device) * scale.to(device)
    if out_size > in_size:
        x = x.clamp(0, in_size - 1)
    i0 = x.floor()
    d = x - i0
    i0 = i0.long().clamp(0, in_size - 1)
    return i0, (i0 + 1).clamp(max=in_size - 1), d


def resize_bilinear_tf(top, size):
    """`top` (N, C, Ht, Wt) resized to `size` by the same rule as index gathers and three lerps (any device, any float
    dtype, differentiable): the composed form of the kernel"""
    H, W = size
    i0, i1, dx = _tf_taps(H, top.shape[2], top.device)
    j0, j1, dy = _tf_taps(W, top.shape[3], top.device)
    dx, dy = dx.to(top.dtype)[:, None], dy.to(top.dtype)[None, :]
    r0, r1 = top[:, :, i0], top[:, :, i1]
    a, b, c, d = r0[..., j0], r1[..., j0], r0[..., j1], r1[..., j1]
    ab = dx * b + (1 - dx) * a
    cd = dx * d + (1 - dx) * c
    return ab * (1 - dy) + cd * dy


def upsample_add_bilinear_composed(lateral, top, div=1.0):
    return (lateral + resize_bilinear_tf(top, lateral.shape[2:])) / div


def upsample_add_bilinear(lateral, top, div=1.0):
    """(lateral + top resized to lateral's size by the bilinear tf_mode rule) / div as one launch per direction.  Device
    tensors only (`fusable`); callers with other inputs take `upsample_add_bilinear_composed`."""
    L.need_device(lateral, top)
    return _UpsampleAddBilinear.apply(lateral, top, div)
