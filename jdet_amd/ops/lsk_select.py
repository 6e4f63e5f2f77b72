"""The kernel-selection step of an LSK block (csrc/lsk_select.hip, include/jdet_hip_lsk.h) as two autograd nodes around the
library's 2 -> 2 7x7 convolution and sigmoid:

    agg = lsk_squeeze(a1, a2)          channel mean and max of concat(a1, a2), which is never materialised
    sig = conv_squeeze(agg).sigmoid()
    out = lsk_select(a1, a2, sig)      a1 * sig[:, 0:1] + a2 * sig[:, 1:2]

(python/jdet/models/backbones/lsknet.py:L126-131 runs them as two concatenations, a mean, a max, two slices, two products
and a sum.)"""
import os

import torch

from .. import _lib as L

ENABLED = os.environ.get("JDET_LSK_SELECT", "1") == "1"     # A/B switch for measurements (profiles/lsk.md)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


class _LskSqueeze(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a1, a2):
        N, Ch, H, W = a1.shape
        agg = torch.empty((N, 2, H, W), dtype=torch.float32, device=a1.device, memory_format=torch.channels_last)
        argmax = torch.empty((N * H * W,), dtype=torch.int32, device=a1.device)
        L.check(L.lib().jdet_lsk_squeeze_forward(L.ptr(a1), L.ptr(a2), N, H, W, Ch, L.ptr(agg), L.ptr(argmax),
                                                 L.stream_ptr(a1)), "jdet_lsk_squeeze_forward")
        ctx.save_for_backward(argmax)
        ctx.shape = (N, Ch, H, W)
        ctx.mark_non_differentiable(argmax)
        return agg, argmax

    @staticmethod
    def backward(ctx, g_agg, _):
        (argmax,) = ctx.saved_tensors
        N, Ch, H, W = ctx.shape
        g_agg = _cl(g_agg)
        g1, g2 = (L.zero_(torch.empty((N, Ch, H, W), dtype=torch.float32, device=g_agg.device,
                                      memory_format=torch.channels_last)) for _ in range(2))
        L.check(L.lib().jdet_lsk_squeeze_backward(L.ptr(g_agg), L.ptr(argmax), N, H, W, Ch, L.ptr(g1), L.ptr(g2),
                                                  L.stream_ptr(g_agg)), "jdet_lsk_squeeze_backward")
        return g1, g2


class _LskSelect(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a1, a2, sig):
        N, Ch, H, W = a1.shape
        out = torch.empty_like(a1, memory_format=torch.channels_last)
        L.check(L.lib().jdet_lsk_select_forward(L.ptr(a1), L.ptr(a2), L.ptr(sig), N, H, W, Ch, L.ptr(out),
                                                L.stream_ptr(a1)), "jdet_lsk_select_forward")
        ctx.save_for_backward(a1, a2, sig)
        return out

    @staticmethod
    def backward(ctx, g):
        a1, a2, sig = ctx.saved_tensors
        N, Ch, H, W = a1.shape
        g = _cl(g)
        g1, g2 = torch.empty_like(a1, memory_format=torch.channels_last), torch.empty_like(a2, memory_format=torch.channels_last)
        gs = torch.empty_like(sig, memory_format=torch.channels_last)
        L.check(L.lib().jdet_lsk_select_backward(L.ptr(g), L.ptr(a1), L.ptr(a2), L.ptr(sig), N, H, W, Ch, L.ptr(g1),
                                                 L.ptr(g2), L.ptr(gs), L.stream_ptr(g)), "jdet_lsk_select_backward")
        return g1, g2, gs


def _map_ok(t, channels=None):
    return (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.numel() > 0
            and (channels is None or t.shape[1] == channels) and t.is_contiguous(memory_format=torch.channels_last))


def fusable(a1, a2, sig=None):
    """fp32 channels-last device maps of one shape with Ch % 4 == 0 (sig: (N, 2, H, W)), below the kernels' 32-bit sizes"""
    return (_map_ok(a1) and _map_ok(a2) and a1.shape == a2.shape and a1.shape[1] % 4 == 0
            and 2 * a1.numel() < 2 ** 31 and a1.numel() // a1.shape[1] < 2 ** 25
            and (sig is None or (_map_ok(sig, 2) and sig.shape[0] == a1.shape[0] and sig.shape[2:] == a1.shape[2:]))
            and not torch.is_autocast_enabled())


def lsk_squeeze_composed(a1, a2):
    attn = torch.cat([a1, a2], dim=1)
    return torch.cat([attn.mean(dim=1, keepdim=True), attn.max(dim=1, keepdim=True)[0]], dim=1)


def lsk_select_composed(a1, a2, sig):
    return a1 * sig[:, 0:1] + a2 * sig[:, 1:2]


def lsk_squeeze(a1, a2):
    """(N, 2, H, W): channel 0 the mean, channel 1 the max over the channels of concat(a1, a2)"""
    if ENABLED and fusable(a1, a2):
        return _LskSqueeze.apply(a1, a2)[0]
    return lsk_squeeze_composed(a1, a2)


def lsk_select(a1, a2, sig):
    """a1 * sig[:, 0:1] + a2 * sig[:, 1:2]"""
    if ENABLED and fusable(a1, a2, sig):
        return _LskSelect.apply(a1, a2, sig)
    return lsk_select_composed(a1, a2, sig)
