"""Fixtures and buffer-contract cases (tests/guarded.py) of the depthwise-convolution and kernel-selection entry points of
include/jdet_hip_lsk.h.  Importable without a GPU; tests/test_lsk_cpu.py dry-runs the smallest instances,
tests/test_gpu_lsk.py runs every shape.

Bounds (none comes from the code under test; tests/lsk_ref.py has the formulas):
  * act 0 forward and the data gradient (the same entry point on flipped taps): equality with the float32 restatement;
  * GELU forward / backward: gamma(KH KW + 1) * sum |terms| of the convolution times 1.13 (>= max |gelu'| and
    >= max |gelu''|, `gelu_case`), plus an allowance for the device erff: 4 x the error of the framework's own float32
    GELU (forward: F.gelu; backward: its autograd) against float64 on the same pre-activations, measured on the run's
    device when the reference is evaluated;
  * weight / bias gradients: gamma(N H W) * sum |terms| per output (valid for any order of the N H W terms);
  * the mean: gamma(2 Ch + 1) * sum |terms|; g_sig: gamma(Ch + 1) * sum |terms|; max, argmax, select forward, g_a1, g_a2:
    equality; squeeze backward (accumulating, compared as out - base): three roundings of at most
    2^-24 * (|base| + |g_mean| / (2 Ch) + |g_max|) each."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import abi_cases
from tests import lsk_ref as R
from tests.abi_cases import Case, P, Res, ST

# key -> (N, C, H, W, KH, KW, dil, bias)
DW_SHAPES = {
    "a": (2, 8, 5, 7, 7, 7, 3, False),        # map smaller than the 19 x 19 footprint: every tap is outside somewhere
    "b": (1, 4, 1, 1, 5, 5, 1, False),        # a single pixel
    "c": (2, 12, 9, 33, 5, 5, 1, False),      # C a multiple of 4 only; W across a 4-pixel tile edge
    "d": (1, 320, 6, 6, 3, 3, 1, True),       # 80 channel quads: more than one wave; the MLP form (bias, GELU)
    "e": (2, 64, 20, 24, 7, 7, 3, False),     # interior and border both
    "f": (1, 8, 4, 23, 1, 19, 1, False),      # strip kernels
    "g": (1, 8, 23, 4, 19, 1, 1, False),
}
GELU_KEYS = ("d", "a", "c")
SELECT_CH = (2, 16, 160)
SELECT_MAP = (2, 3, 5)                        # N, H, W
ERF_ALLOWANCE = 4.0


def lib():
    return abi_cases.lib()


@functools.lru_cache(maxsize=None)
def dw_fixture(key, with_bias=None):
    """-> dict of float32 arrays x, g (N, H, W, C), w (KH, KW, C), bias (C) or None, and the geometry; shared, never written"""
    N, C, H, W, KH, KW, dil, bias = DW_SHAPES[key]
    bias = bias if with_bias is None else with_bias
    rng = np.random.default_rng([ord(key), N, C, H, W])
    pad = (R.same_pad(KH, dil if KH > 1 else 1), R.same_pad(KW, dil if KW > 1 else 1))
    d = (dil if KH > 1 else 1, dil if KW > 1 else 1)
    f = dict(x=rng.standard_normal((N, H, W, C)).astype(np.float32), g=rng.standard_normal((N, H, W, C)).astype(np.float32),
             w=(rng.standard_normal((KH, KW, C)) * 0.5).astype(np.float32),
             bias=(rng.standard_normal(C) * 0.5).astype(np.float32) if bias else None, pad=pad, dil=d,
             geom=(N, H, W, C, KH, KW) + pad + d)
    for v in f.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return f


def _label(key, extra=""):
    N, C, H, W, KH, KW, dil, _ = DW_SHAPES[key]
    return "%s (%d,%d,%d,%d | %dx%d, %d)%s" % (key, N, C, H, W, KH, KW, dil, extra)


def forward_case(key, flipped=False):
    """act 0: the bit-exact pin.  flipped: the data gradient -- g through the flipped taps, no bias"""
    f = dw_fixture(key)
    src = f["g"] if flipped else f["x"]
    w = R.flip_taps(f["w"]) if flipped else f["w"]
    bias = None if flipped else f["bias"]

    def fn(run):
        xin, win = run.inp("x", src), run.inp("w", w)
        bin_ = run.inp("bias", bias) if bias is not None else None
        y = run.out("y", src.shape)
        run.ok(lib().jdet_dwconv_nhwc_forward(P(xin), P(win), P(bin_), *f["geom"], 0, P(y), ST(xin)),
               "jdet_dwconv_nhwc_forward")
        return Res({"y": y}, lambda: {"y": (R.dwconv_f32(src, w, bias, f["pad"], f["dil"]), 0.0)})
    return Case(("jdet_dwconv_nhwc_forward",), _label(key, " data gradient" if flipped else ""), fn)


def _device_gelu_error(z64, dev, grad):
    """max error of the framework's own float32 GELU (its autograd when `grad`) against float64 on float32(z)"""
    z32 = torch.tensor(np.asarray(z64, np.float32), device=dev)
    if grad:
        z32.requires_grad_(True)
        (got,) = torch.autograd.grad(F.gelu(z32).sum(), z32)
        want = R.gelu_grad64(z32.detach().cpu().numpy())
    else:
        got, want = F.gelu(z32), R.gelu64(z32.cpu().numpy())
    return float(np.abs(got.detach().cpu().double().numpy() - want).max())


MEASURED = {}        # (entry point, key, device type) -> (library GELU error, largest bound): printed by the GPU test


def gelu_case(key, backward=False):
    """forward with GELU / jdet_dwconv_gelu_backward against float64, always with a bias.
    z = conv + bias carries e_z <= gamma(KH KW + 1) * sum |terms|.  Forward: |gelu(z + e) - gelu(z)| <= 1.13 e_z.
    Backward: |g_y| * |gelu'(z + e) - gelu'(z)| <= |g_y| * max |gelu''| * e_z, and max |gelu''| = 2 phi(0) = 0.798 <= 1.13.
    Both plus 4 x the framework GELU's own float32 error (times |g_y| backward: the product's rounding is inside it)."""
    f = dw_fixture(key, with_bias=True)
    name = "jdet_dwconv_gelu_backward" if backward else "jdet_dwconv_nhwc_forward"

    def fn(run):
        xin, win, bin_ = run.inp("x", f["x"]), run.inp("w", f["w"]), run.inp("bias", f["bias"])
        out = run.out("g_z" if backward else "y", f["x"].shape)
        if backward:
            gin = run.inp("g_y", f["g"])
            run.ok(lib().jdet_dwconv_gelu_backward(P(xin), P(win), P(bin_), P(gin), *f["geom"], P(out), ST(xin)), name)
        else:
            run.ok(lib().jdet_dwconv_nhwc_forward(P(xin), P(win), P(bin_), *f["geom"], 1, P(out), ST(xin)), name)

        def ref():
            z, mag = R.dwconv_f64(f["x"], f["w"], f["bias"], f["pad"], f["dil"])
            e_z = R.GELU_GRAD_MAX * R.conv_bound(mag, f["w"].shape[0], f["w"].shape[1])
            lib_err = _device_gelu_error(z, run.dev, backward)
            if backward:
                gy = np.abs(f["g"].astype(np.float64))
                want, bound = f["g"].astype(np.float64) * R.gelu_grad64(z), gy * (e_z + ERF_ALLOWANCE * lib_err)
                bound = bound + R.U32 * np.abs(want)
            else:
                want, bound = R.gelu64(z), e_z + ERF_ALLOWANCE * lib_err
            MEASURED[(name, key, run.dev.type)] = (lib_err, float(np.max(bound)))
            return {("g_z" if backward else "y"): (want, bound)}
        return Res({("g_z" if backward else "y"): out}, ref)
    return Case((name,), _label(key, " bias GELU" + (" backward" if backward else "")), fn)


def wgrad_case(key):
    f = dw_fixture(key)
    N, H, W, C, KH, KW = f["geom"][:6]
    with_bias = f["bias"] is not None

    def fn(run):
        xin, gin = run.inp("x", f["x"]), run.inp("g", f["g"])
        gw = run.out("gw", (KH, KW, C))
        gb = run.out("gb", (C,)) if with_bias else None
        ws, wsb = run.ws("workspace", lib().jdet_dwconv_nhwc_wgrad_workspace(N, H, W, C, KH, KW))
        run.ok(lib().jdet_dwconv_nhwc_wgrad(P(xin), P(gin), *f["geom"], P(gw), P(gb), P(ws), wsb, ST(xin)),
               "jdet_dwconv_nhwc_wgrad")

        def ref():
            rw, rb, mw, mb = R.wgrad64(f["x"], f["g"], KH, KW, f["pad"], f["dil"])
            k = R.gamma(N * H * W)
            out = {"gw": (rw, k * mw + 1e-45)}
            if with_bias:
                out["gb"] = (rb, k * mb + 1e-45)
            return out
        return Res(dict(gw=gw, **({"gb": gb} if with_bias else {})), ref)
    return Case(("jdet_dwconv_nhwc_wgrad_workspace", "jdet_dwconv_nhwc_wgrad"), _label(key, " bias" if with_bias else ""), fn)


# ------------------------------------------------------------------------------------------------------------- selection
@functools.lru_cache(maxsize=None)
def select_fixture(ch, tied=False):
    N, H, W = SELECT_MAP
    rng = np.random.default_rng([ch, int(tied)])
    if tied:      # values on a grid of 4: every pixel's maximum is attained more than once (for Ch >= 4), in both branches
        a1, a2 = (rng.integers(0, 4, (N, H, W, ch)).astype(np.float32) for _ in range(2))
        a2[0, 0, 0] = 0.0
        a1[0, 0, 0], a1[0, 0, 0, ch - 1] = 0.0, 3.0                               # a tie across the two branches
        a2[0, 0, 0, ch - 1] = 3.0
    else:
        a1, a2 = (rng.standard_normal((N, H, W, ch)).astype(np.float32) for _ in range(2))
        assert not R.has_ties(a1, a2).any()
    f = dict(a1=a1, a2=a2, sig=rng.uniform(0.05, 0.95, (N, H, W, 2)).astype(np.float32),
             g=rng.standard_normal((N, H, W, ch)).astype(np.float32),
             g_agg=rng.standard_normal((N, H, W, 2)).astype(np.float32),
             base1=rng.standard_normal((N, H, W, ch)).astype(np.float32),
             base2=rng.standard_normal((N, H, W, ch)).astype(np.float32))
    for v in f.values():
        v.setflags(write=False)
    return f


def squeeze_forward_case(ch, tied=False):
    f = select_fixture(ch, tied)
    N, H, W = SELECT_MAP

    def fn(run):
        a1, a2 = run.inp("a1", f["a1"]), run.inp("a2", f["a2"])
        agg, am = run.out("agg", (N, H, W, 2)), run.out("argmax", (N * H * W,), torch.int32)
        run.ok(lib().jdet_lsk_squeeze_forward(P(a1), P(a2), N, H, W, ch, P(agg), P(am), ST(a1)), "jdet_lsk_squeeze_forward")

        def ref():
            mean, mag, mx, idx = R.squeeze(f["a1"], f["a2"])
            assert tied or not R.has_ties(f["a1"], f["a2"]).any()
            bound = np.stack([R.gamma(2 * ch + 1) * mag + 1e-45, np.zeros_like(mag)], axis=3)
            return {"agg": (np.stack([mean, mx.astype(np.float64)], axis=3), bound), "argmax": (idx.reshape(-1), 0.0)}
        return Res({"agg": agg, "argmax": am}, ref)
    return Case(("jdet_lsk_squeeze_forward",), "Ch %d%s" % (ch, " tied maxima" if tied else ""), fn)


def squeeze_backward_case(ch, tied=False):
    f = select_fixture(ch, tied)
    N, H, W = SELECT_MAP
    _, _, _, idx = R.squeeze(f["a1"], f["a2"])

    def fn(run):
        gin, am = run.inp("g_agg", f["g_agg"]), run.inp("argmax", idx.reshape(-1))
        g1, g2 = run.acc("g_a1", f["base1"]), run.acc("g_a2", f["base2"])
        run.ok(lib().jdet_lsk_squeeze_backward(P(gin), P(am), N, H, W, ch, P(g1), P(g2), ST(gin)), "jdet_lsk_squeeze_backward")

        def ref():
            r1, r2, m1, m2 = R.squeeze_backward64(f["g_agg"], idx, ch)
            return {"g_a1": (r1, 3 * R.U32 * (np.abs(f["base1"]) + m1)), "g_a2": (r2, 3 * R.U32 * (np.abs(f["base2"]) + m2))}
        return Res({"g_a1": g1, "g_a2": g2}, ref)
    return Case(("jdet_lsk_squeeze_backward",), "Ch %d%s" % (ch, " tied maxima" if tied else ""), fn)


def select_forward_case(ch):
    f = select_fixture(ch)
    N, H, W = SELECT_MAP

    def fn(run):
        a1, a2, sig = run.inp("a1", f["a1"]), run.inp("a2", f["a2"]), run.inp("sig", f["sig"])
        out = run.out("out", (N, H, W, ch))
        run.ok(lib().jdet_lsk_select_forward(P(a1), P(a2), P(sig), N, H, W, ch, P(out), ST(a1)), "jdet_lsk_select_forward")
        return Res({"out": out}, lambda: {"out": (R.select_f32(f["a1"], f["a2"], f["sig"]), 0.0)})
    return Case(("jdet_lsk_select_forward",), "Ch %d" % ch, fn)


def select_backward_case(ch):
    f = select_fixture(ch)
    N, H, W = SELECT_MAP

    def fn(run):
        g, a1, a2, sig = (run.inp(k, f[k]) for k in ("g", "a1", "a2", "sig"))
        g1, g2, gs = run.out("g_a1", (N, H, W, ch)), run.out("g_a2", (N, H, W, ch)), run.out("g_sig", (N, H, W, 2))
        run.ok(lib().jdet_lsk_select_backward(P(g), P(a1), P(a2), P(sig), N, H, W, ch, P(g1), P(g2), P(gs), ST(g)),
               "jdet_lsk_select_backward")

        def ref():
            r1, r2, rs, mag = R.select_backward(f["g"], f["a1"], f["a2"], f["sig"])
            return {"g_a1": (r1, 0.0), "g_a2": (r2, 0.0), "g_sig": (rs, R.gamma(ch + 1) * mag + 1e-45)}
        return Res({"g_a1": g1, "g_a2": g2, "g_sig": gs}, ref)
    return Case(("jdet_lsk_select_backward",), "Ch %d" % ch, fn)


def dw_cases():
    out = []
    for key in DW_SHAPES:
        out += [forward_case(key), forward_case(key, flipped=True), wgrad_case(key)]
    for key in GELU_KEYS:
        out += [gelu_case(key), gelu_case(key, backward=True)]
    return out


def select_cases():
    out = []
    for ch in SELECT_CH:
        out += [squeeze_forward_case(ch), squeeze_backward_case(ch), select_forward_case(ch), select_backward_case(ch)]
    return out + [squeeze_forward_case(16, tied=True), squeeze_backward_case(16, tied=True)]


def smallest_cases():
    """one instance per entry point, for the CPU dry run"""
    return [forward_case("b"), gelu_case("a", backward=True), wgrad_case("b"), squeeze_forward_case(2),
            squeeze_backward_case(2), select_forward_case(2), select_backward_case(2)]
