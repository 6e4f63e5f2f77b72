"""Numpy restatements of the rules of include/jdet_hip_lsk.h for tests/test_lsk_cpu.py and tests/test_gpu_lsk.py, written
from the header's rule text, not from the kernels.

  dwconv_f32      the convolution in float32 in the stated order: acc = bias or 0, kh outer, kw inner, a float32 product
                  then a float32 sum, taps outside the map skipped -- the bit-exact pin of act 0 and of the data gradient
  dwconv_f64      float64 F.conv2d(groups=C) and the sum of |terms| that scales the error bounds
  gelu64 / gelu_grad64   the erf forms in float64
  wgrad64         float64 autograd of the weights and the bias, with the sums of |terms|
  squeeze / select       float32 where the rule is exact (max, first argmax, two products and a sum), float64 and
                  sums of |terms| where a sum's order matters (mean, g_sig)

gamma(k) = k u / (1 - k u), u = 2^-24: the classical bound of a float32 sum of k additions in ANY order."""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24


def gamma(k):
    return k * U32 / (1.0 - k * U32)


def flip_taps(w):
    """(KH, KW, C) -> the data gradient's taps"""
    return np.ascontiguousarray(w[::-1, ::-1])


def same_pad(k, dil):
    assert (dil * (k - 1)) % 2 == 0
    return dil * (k - 1) // 2


def _window(size, shift):
    """output range [lo, hi) whose tap `shift` lies inside [0, size)"""
    return max(0, -shift), min(size, size - shift)


def dwconv_f32(x, w, bias, pad, dil):
    """x (N, H, W, C), w (KH, KW, C), bias (C) or None, pad / dil: (h, w) pairs -> float32 (N, H, W, C)"""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    N, H, W, C = x.shape
    acc = np.zeros((N, H, W, C), np.float32)
    if bias is not None:
        acc += np.asarray(bias, np.float32)
    for kh in range(w.shape[0]):
        for kw in range(w.shape[1]):
            sh, sw = kh * dil[0] - pad[0], kw * dil[1] - pad[1]
            (h0, h1), (w0, w1) = _window(H, sh), _window(W, sw)
            if h0 >= h1 or w0 >= w1:
                continue
            prod = (w[kh, kw] * x[:, h0 + sh:h1 + sh, w0 + sw:w1 + sw]).astype(np.float32)
            acc[:, h0:h1, w0:w1] = (acc[:, h0:h1, w0:w1] + prod).astype(np.float32)
    assert acc.dtype == np.float32
    return acc


def _nchw64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64).permute(0, 3, 1, 2)


def _w64(w):
    return torch.tensor(np.asarray(w), dtype=torch.float64).permute(2, 0, 1).unsqueeze(1)


def dwconv_f64(x, w, bias, pad, dil):
    """-> (z float64 (N, H, W, C), sum of |terms| per output: conv(|x|, |w|) + |bias|)"""
    C = x.shape[3]
    b = None if bias is None else torch.tensor(np.asarray(bias), dtype=torch.float64)
    z = F.conv2d(_nchw64(x), _w64(w), b, 1, pad, dil, groups=C)
    mag = F.conv2d(_nchw64(np.abs(x)), _w64(np.abs(w)), None if b is None else b.abs(), 1, pad, dil, groups=C)
    return z.permute(0, 2, 3, 1).numpy(), mag.permute(0, 2, 3, 1).numpy()


def conv_bound(mag, kh, kw):
    """gamma_k * sum |terms|, k = KH KW + 1 (the products' roundings and the additions of one output)"""
    return gamma(kh * kw + 1) * mag


def gelu64(z):
    z = torch.as_tensor(np.asarray(z, np.float64))
    return (0.5 * z * (1.0 + torch.erf(z / np.sqrt(2.0)))).numpy()


def gelu_grad64(z):
    """Phi(z) + z phi(z)"""
    z = torch.as_tensor(np.asarray(z, np.float64))
    return (0.5 * (1.0 + torch.erf(z / np.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)).numpy()


GELU_GRAD_MAX = 1.13        # max |gelu'| = 1.1290 at z = sqrt(2)


def wgrad64(x, g, kh, kw, pad, dil):
    """-> gw (KH, KW, C), gb (C), and the sums of |terms| of each, by float64 autograd of F.conv2d"""
    C = x.shape[3]

    def grads(xv, gv):
        w = torch.zeros((C, 1, kh, kw), dtype=torch.float64, requires_grad=True)
        b = torch.zeros((C,), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(_nchw64(xv), w, b, 1, pad, dil, groups=C)
        gw, gb = torch.autograd.grad(y, (w, b), grad_outputs=_nchw64(gv))
        return gw[:, 0].permute(1, 2, 0).numpy(), gb.numpy()
    gw, gb = grads(x, g)
    gw_mag, gb_mag = grads(np.abs(x), np.abs(g))
    return gw, gb, gw_mag, gb_mag


# ------------------------------------------------------------------------------------------------------------- selection
def squeeze(a1, a2):
    """a1, a2 (N, H, W, Ch) float32 -> mean64 (N, H, W), sum of |terms|, max float32, first argmax int32"""
    cat = np.concatenate([np.asarray(a1, np.float32), np.asarray(a2, np.float32)], axis=3)
    n = cat.shape[3]
    return (cat.astype(np.float64).sum(3) / n, np.abs(cat.astype(np.float64)).sum(3) / n, cat.max(3),
            np.argmax(cat, axis=3).astype(np.int32))


def has_ties(a1, a2):
    cat = np.concatenate([a1, a2], axis=3)
    return (cat == cat.max(3, keepdims=True)).sum(3) > 1


def squeeze_backward64(g_agg, argmax, ch):
    """what the call adds to g_a1, g_a2: g_mean / (2 Ch) everywhere, g_max at the argmax channel -> two float64 arrays
    and the magnitude |g_mean| / (2 Ch) + |g_max| there"""
    g = np.asarray(g_agg, np.float64)
    N, H, W, _ = g.shape
    add = np.repeat(g[..., :1] / (2 * ch), 2 * ch, axis=3)
    mag = np.abs(add)
    hit = np.arange(2 * ch)[None, None, None, :] == np.asarray(argmax).reshape(N, H, W, 1)
    add = add + hit * g[..., 1:2]
    mag = mag + hit * np.abs(g[..., 1:2])
    return add[..., :ch], add[..., ch:], mag[..., :ch], mag[..., ch:]


def select_f32(a1, a2, sig):
    a1, a2, sig = (np.asarray(v, np.float32) for v in (a1, a2, sig))
    out = ((a1 * sig[..., 0:1]).astype(np.float32) + (a2 * sig[..., 1:2]).astype(np.float32)).astype(np.float32)
    assert out.dtype == np.float32
    return out


def select_backward(g, a1, a2, sig):
    """-> g_a1, g_a2 float32 (exact: one product each), g_sig float64 (N, H, W, 2) and its sum of |terms|"""
    g, a1, a2, sig = (np.asarray(v, np.float32) for v in (g, a1, a2, sig))
    g1, g2 = (g * sig[..., 0:1]).astype(np.float32), (g * sig[..., 1:2]).astype(np.float32)
    g64 = g.astype(np.float64)
    gs = np.stack([(g64 * a1).sum(3), (g64 * a2).sum(3)], axis=3)
    mag = np.stack([np.abs(g64 * a1).sum(3), np.abs(g64 * a2).sum(3)], axis=3)
    return g1, g2, gs, mag
