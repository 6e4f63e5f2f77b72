"""Depthwise convolution of a channels-last map, stride 1 and "same" padding, optionally with the GELU that follows it in
an LSKNet MLP (csrc/dwconv.hip; the order of every addition is stated in include/jdet_hip_lsk.h).  One launch forward;
backward: the same kernel on the flipped weights for the data gradient, a two-stage fixed-order weight / bias gradient,
and with GELU one more launch that recomputes the pre-activation from `x` -- only `x` is saved."""
import os

import torch
import torch.nn.functional as F

from .. import _lib as L

ENABLED = os.environ.get("JDET_DWCONV", "1") == "1"     # A/B switch for measurements (profiles/lsk.md)
# Kernels of more than 25 taps (the 7x7 dilation-3 layer) stay with the library on maps below this many positions
# (N H W): at LSKNet_s stage 4 (2 x 32^2 = 2048 positions, 512 channels) the library's forward + backward measured 0.16 ms
# against 0.25 ms here, at stage 3 (8192 positions) 0.34 ms against 0.22 ms (profiles/lsk.md); the 5x5 and the 3x3 + GELU
# forms measured faster here at every stage.
LARGE_TAPS_MIN_POSITIONS = int(os.environ.get("JDET_DWCONV_LARGE_MIN_POS", "4096"))


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def pack_weight(weight, flip=False):
    """(C, 1, KH, KW) -> the kernels' (KH, KW, C); flip: the data gradient's taps"""
    w = weight[:, 0]
    if flip:
        w = w.flip(1, 2)
    return w.permute(1, 2, 0).contiguous()


def _geometry(x, weight, padding, dilation):
    N, C, H, W = x.shape
    return (N, H, W, C, weight.shape[2], weight.shape[3]) + _pair(padding) + _pair(dilation)


def dwconv_nhwc(x, w_packed, bias, geom, act=0, out=None):
    """x: channels-last (N, C, H, W); w_packed (KH, KW, C); -> act(dwconv(x) + bias), channels-last"""
    y = torch.empty_like(x, memory_format=torch.channels_last) if out is None else out
    L.check(L.lib().jdet_dwconv_nhwc_forward(L.ptr(x), L.ptr(w_packed), L.ptr(bias), *geom, int(act), L.ptr(y),
                                             L.stream_ptr(x)), "jdet_dwconv_nhwc_forward")
    return y


def dwconv_gelu_backward_nhwc(x, w_packed, bias, g_y, geom):
    g_z = torch.empty_like(x, memory_format=torch.channels_last)
    L.check(L.lib().jdet_dwconv_gelu_backward(L.ptr(x), L.ptr(w_packed), L.ptr(bias), L.ptr(g_y), *geom, L.ptr(g_z),
                                              L.stream_ptr(x)), "jdet_dwconv_gelu_backward")
    return g_z


def dwconv_wgrad_nhwc(x, g, geom, with_bias=True):
    """-> (gw (KH, KW, C), gb (C) or None)"""
    N, H, W, C, KH, KW = geom[:6]
    need = L.lib().jdet_dwconv_nhwc_wgrad_workspace(N, H, W, C, KH, KW)
    ws = torch.empty((need,), dtype=torch.uint8, device=x.device)
    gw = torch.empty((KH, KW, C), dtype=torch.float32, device=x.device)
    gb = torch.empty((C,), dtype=torch.float32, device=x.device) if with_bias else None
    L.check(L.lib().jdet_dwconv_nhwc_wgrad(L.ptr(x), L.ptr(g), *geom, L.ptr(gw), L.ptr(gb), L.ptr(ws), need,
                                           L.stream_ptr(x)), "jdet_dwconv_nhwc_wgrad")
    return gw, gb


class _DWConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, padding, dilation, act):
        geom = _geometry(x, weight, padding, dilation)
        y = dwconv_nhwc(x, pack_weight(weight), bias, geom, act)
        ctx.save_for_backward(x, weight, bias)
        ctx.cfg = (geom, act)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, bias = ctx.saved_tensors
        geom, act = ctx.cfg
        g = g.contiguous(memory_format=torch.channels_last)
        if act:
            g = dwconv_gelu_backward_nhwc(x, pack_weight(weight), bias, g, geom)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = dwconv_nhwc(g, pack_weight(weight, flip=True), None, geom, 0)
        if ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2]):
            gw, gb = dwconv_wgrad_nhwc(x, g, geom, bias is not None)
            gw = gw.permute(2, 0, 1).unsqueeze(1)
        return gx, gw, gb, None, None, None


def same_padded(weight, padding, dilation, stride=1):
    (ph, pw), (dh, dw) = _pair(padding), _pair(dilation)
    return (_pair(stride) == (1, 1) and 2 * ph == dh * (weight.shape[2] - 1) and 2 * pw == dw * (weight.shape[3] - 1))


def fusable(x, weight, bias=None, padding=0, dilation=1, stride=1):
    """fp32 channels-last device map, C % 4 == 0, depthwise weights, stride 1, "same" padding, below 2^31 elements"""
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0
            and x.shape[1] % 4 == 0 and tuple(weight.shape[:2]) == (x.shape[1], 1)
            and (bias is None or (bias.is_cuda and bias.dtype == torch.float32))
            and x.is_contiguous(memory_format=torch.channels_last) and x.numel() < 2 ** 31
            and same_padded(weight, padding, dilation, stride) and not torch.is_autocast_enabled())


def preferred(x, weight):
    """is the HIP route the measured faster choice for this (fusable) call?"""
    taps, positions = weight.shape[2] * weight.shape[3], x.shape[0] * x.shape[2] * x.shape[3]
    return taps <= 25 or positions >= LARGE_TAPS_MIN_POSITIONS


def dwconv_composed(x, weight, bias, padding, dilation, act=None, stride=1):
    """the library form (any device, any dtype): grouped convolution, then the erf GELU"""
    y = F.conv2d(x, weight, bias, stride, padding, dilation, groups=x.shape[1])
    return F.gelu(y) if act == "gelu" else y


def dwconv(x, weight, bias, padding, dilation=1, act=None):
    """act(depthwise_conv(x, weight (C, 1, KH, KW)) + bias), stride 1; act: None or "gelu".  The HIP route where
    `ENABLED`, `fusable` and `preferred`, the composed form everywhere else."""
    if act not in (None, "gelu"):
        raise ValueError("dwconv: act is None or 'gelu', got %r" % (act,))
    if ENABLED and fusable(x, weight, bias, padding, dilation) and preferred(x, weight):
        return _DWConv.apply(x, weight, bias, padding, dilation, L.DWCONV_ACTS[act])
    return dwconv_composed(x, weight, bias, padding, dilation, act)
