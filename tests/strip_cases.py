"""Fixtures and buffer-contract cases (tests/guarded.py) of the strip-convolution entry point of
include/jdet_hip_strip.h.  Importable without a GPU; tests/test_strip_cpu.py dry-runs the smallest instances,
tests/test_gpu_strip.py runs every shape on both axes.

The one bound: equality.  The header states the order of jdet_dwconv_nhwc_forward with a K x 1 or 1 x K kernel, so the
expected values are tests/lsk_ref.dwconv_f32 (written from that header's rule text) with tolerance 0.0, forward and -- on
flipped taps, without a bias -- data gradient."""
import functools

import numpy as np

from tests import abi_cases
from tests import lsk_ref as R
from tests.abi_cases import Case, P, Res, ST

# key -> (N, C, H, W, K, bias) as axis 1 sees it (the strip along W); axis 0 swaps H and W
STRIP_SHAPES = {
    "a": (2, 8, 3, 23, 19, True),         # a length that is not a multiple of 4
    "b": (1, 8, 2, 5, 19, False),         # an axis shorter than K: every window leaves the map
    "c": (1, 4, 1, 1, 19, False),         # a single pixel
    "d": (1, 320, 3, 6, 19, True),        # 80 channel quads, more than a wave
    "e": (2, 12, 4, 9, 3, False),         # C a multiple of 4 only
    "f": (1, 4, 2, 7, 1, True),           # K = 1
    "g": (1, 8, 2, 40, 19, False),        # interior windows with no tap skipped
}
AXES = (0, 1)


def lib():
    return abi_cases.lib()


@functools.lru_cache(maxsize=None)
def strip_fixture(key, axis):
    """-> dict of float32 arrays x, g (N, H, W, C), w (K, C), bias (C) or None, geom (N, H, W, C, K) and the pad / dil
    pairs and (KH, KW) shape under which tests/lsk_ref states the same convolution; shared, never written"""
    N, C, H, W, K, bias = STRIP_SHAPES[key]
    if axis == 0:
        H, W = W, H
    rng = np.random.default_rng([ord(key), axis, N, C, H, W])
    p = (K - 1) // 2
    f = dict(x=rng.standard_normal((N, H, W, C)).astype(np.float32), g=rng.standard_normal((N, H, W, C)).astype(np.float32),
             w=(rng.standard_normal((K, C)) * 0.5).astype(np.float32),
             bias=(rng.standard_normal(C) * 0.5).astype(np.float32) if bias else None,
             geom=(N, H, W, C, K), axis=axis, pad=(p, 0) if axis == 0 else (0, p), dil=(1, 1),
             kshape=(K, 1, C) if axis == 0 else (1, K, C))
    for v in f.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return f


def flip_taps(w):
    """(K, C) -> the data gradient's taps, in memory of its own (K = 1 included)"""
    return np.array(np.asarray(w)[::-1], order="C", copy=True)


def expected(f, flipped=False):
    """the float32 restatement of the stated order: tests/lsk_ref.dwconv_f32 on the (K, 1, C) / (1, K, C) kernel"""
    w = flip_taps(f["w"]) if flipped else f["w"]
    src, bias = (f["g"], None) if flipped else (f["x"], f["bias"])
    return R.dwconv_f32(src, w.reshape(f["kshape"]), bias, f["pad"], f["dil"])


def _label(key, axis, extra=""):
    N, C, H, W, K, bias = STRIP_SHAPES[key]
    return "%s (%d,%d,%d,%d | %d) axis %d%s%s" % (key, N, C, H, W, K, axis, " bias" if bias else "", extra)


def forward_case(key, axis, flipped=False):
    """flipped: the data gradient -- g through the flipped taps, no bias"""
    f = strip_fixture(key, axis)
    src = f["g"] if flipped else f["x"]
    w = flip_taps(f["w"]) if flipped else f["w"]
    bias = None if flipped else f["bias"]

    def fn(run):
        xin, win = run.inp("x", src), run.inp("w", w)
        bin_ = run.inp("bias", bias) if bias is not None else None
        y = run.out("y", src.shape)
        run.ok(lib().jdet_strip_conv_forward(P(xin), P(win), P(bin_), *f["geom"], axis, P(y), ST(xin)),
               "jdet_strip_conv_forward")
        return Res({"y": y}, lambda: {"y": (expected(f, flipped), 0.0)})
    return Case(("jdet_strip_conv_forward",), _label(key, axis, " data gradient" if flipped else ""), fn)


def strip_cases():
    return [forward_case(key, axis, flipped) for key in STRIP_SHAPES for axis in AXES for flipped in (False, True)]


def smallest_cases():
    """the smallest case of each kind, for the CPU dry run"""
    return [forward_case("c", 1), forward_case("c", 0, flipped=True), forward_case("f", 0), forward_case("f", 1, flipped=True)]
