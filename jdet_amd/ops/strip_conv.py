"""Strip convolution: a depthwise 1 x K or K x 1 kernel over a channels-last map, stride 1, dilation 1, "same" padding
-- the conv_spatial1 / conv_spatial2 layers of a StripNet block (csrc/strip_conv.hip; the order of every addition is
stated in include/jdet_hip_strip.h and is that of csrc/dwconv.hip, bit for bit).  One launch forward; backward: the same
kernel on the flipped weights for the data gradient, and the two-stage fixed-order weight / bias gradient of
ops/dwconv.py.  Only `x`, `weight` and `bias` are saved.

A call that is not `fusable`, not `ENABLED` or not `preferred` goes to ops.dwconv.dwconv unchanged: the generic HIP
kernel where that one is fusable, the library elsewhere."""
import os

import torch

from .. import _lib as L
from . import dwconv as D

ENABLED = os.environ.get("JDET_STRIP_CONV", "1") == "1"     # A/B switch for measurements (profiles/strip.md)
# The strip kernel takes the K x 1 layers (the strip along H) on maps of at least this many positions (N H W).  Measured
# against the generic kernel of ops/dwconv.py at the StripNet_S stage shapes (profiles/strip.md): the 19 x 1 at stage 1
# (2 x 256^2 = 131072 positions, 64 channels) 0.031 ms against 0.095 ms forward and 0.296 ms against 0.351 ms forward +
# backward, both beyond the two spreads; every other layer -- the 1 x 19 at every stage, the 19 x 1 from stage 2
# (32768 positions) down -- was not faster forward + backward by more than the spreads and stays on the generic kernel.
COLUMN_MIN_POSITIONS = int(os.environ.get("JDET_STRIP_CONV_MIN_POS", "131072"))


def strip_axis(weight):
    """0 for a (C, 1, K, 1) weight, 1 for (C, 1, 1, K) (K = 1 counts as axis 1); None if neither dimension is 1"""
    if weight.dim() != 4:
        return None
    return 1 if weight.shape[2] == 1 else (0 if weight.shape[3] == 1 else None)


def pack_weight(weight, flip=False):
    """(C, 1, 1, K) or (C, 1, K, 1) -> the kernel's (K, C); flip: the data gradient's taps"""
    w = weight.reshape(weight.shape[0], -1)
    if flip:
        w = w.flip(1)
    return w.t().contiguous()


def _geometry(x, weight):
    N, C, H, W = x.shape
    return (N, H, W, C, max(weight.shape[2], weight.shape[3]))


def strip_conv_nhwc(x, w_packed, bias, geom, axis, out=None):
    """x: channels-last (N, C, H, W); w_packed (K, C); geom (N, H, W, C, K) -> stripconv(x) + bias, channels-last"""
    y = torch.empty_like(x, memory_format=torch.channels_last) if out is None else out
    L.check(L.lib().jdet_strip_conv_forward(L.ptr(x), L.ptr(w_packed), L.ptr(bias), *geom, int(axis), L.ptr(y),
                                            L.stream_ptr(x)), "jdet_strip_conv_forward")
    return y


def _dw_geometry(geom, axis):
    """the same convolution as ops.dwconv states it: (N, H, W, C, KH, KW, pad_h, pad_w, dil_h, dil_w)"""
    K = geom[4]
    p = (K - 1) // 2
    return geom[:4] + ((K, 1, p, 0) if axis == 0 else (1, K, 0, p)) + (1, 1)


class _StripConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        axis, geom = strip_axis(weight), _geometry(x, weight)
        y = strip_conv_nhwc(x, pack_weight(weight), bias, geom, axis)
        ctx.save_for_backward(x, weight, bias)
        ctx.cfg = (geom, axis)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, bias = ctx.saved_tensors
        geom, axis = ctx.cfg
        g = g.contiguous(memory_format=torch.channels_last)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = strip_conv_nhwc(g, pack_weight(weight, flip=True), None, geom, axis)
        if ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2]):
            gw, gb = D.dwconv_wgrad_nhwc(x, g, _dw_geometry(geom, axis), bias is not None)      # (KH, KW, C)
            gw = gw.permute(2, 0, 1).unsqueeze(1)
        return gx, gw, gb


def fusable(x, weight, bias=None, padding=0, dilation=1, stride=1):
    """the rules of ops.dwconv.fusable, and: one kernel dimension is 1, the other odd, dilation 1 ("same" padding is
    among dwconv's rules)"""
    return (strip_axis(weight) is not None and (weight.shape[2] * weight.shape[3]) % 2 == 1
            and D._pair(dilation) == (1, 1) and D.fusable(x, weight, bias, padding, dilation, stride))


def preferred(x, weight):
    """is the rolling-window kernel the measured faster choice for this (fusable) call?"""
    return weight.shape[2] > 1 and weight.shape[3] == 1 and x.shape[0] * x.shape[2] * x.shape[3] >= COLUMN_MIN_POSITIONS


def strip_conv(x, weight, bias, padding):
    """depthwise_conv(x, weight (C, 1, 1, K) | (C, 1, K, 1)) + bias, stride 1, dilation 1.  The strip kernel where
    `ENABLED`, `fusable` and `preferred`; ops.dwconv.dwconv (its HIP kernel, or the composed form) everywhere else."""
    if ENABLED and fusable(x, weight, bias, padding) and preferred(x, weight):
        return _StripConv.apply(x, weight, bias)
    return D.dwconv(x, weight, bias, padding, 1)
