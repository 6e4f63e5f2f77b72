"""What tests/test_conv_bf16x3_cpu.py and tests/test_gpu_conv_bf16x3.py share: a numpy restatement of the three-way bf16
split and of the six-term convolution of csrc/conv_bf16x3.hip, the shapes, the random inputs and the exactness probes."""
import functools

import numpy as np

BOUND = (2e-5, 1e-6)          # tests/test_gpu_conv_igemm.py: |err| <= 2e-5 * max|ref| + 1e-6
# (N, H, W, Cin, Cout)
CASES = {
    "a": (1, 16, 8, 32, 128),        # one exact M tile, the shortest K
    "b": (1, 7, 9, 32, 128),         # 63 rows: a partial tile
    "c": (2, 13, 5, 64, 15),         # Cout below a tile, an image boundary inside a tile
    "d": (3, 20, 12, 96, 200),       # Cout across two N tiles, Cin not a power of two
    "e": (1, 1, 1, 32, 32),          # every tap but one is padding
    "f": (2, 16, 16, 256, 256),      # the towers' channels
}
# (plane of a, plane of b) in the kernel's order: a3b1, a1b3, a2b2, a2b1, a1b2, a1b1
TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))


def split3(x):
    """fp32 array -> (a1, a2, a3) fp32 arrays: truncation on the bits, exact remainders"""
    x = np.ascontiguousarray(x, np.float32)
    a1 = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r = x - a1
    a2 = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    a3 = r - a2
    return a1, a2, a3


def is_bf16(a):
    return not np.any(np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF))


def conv_restated(x, w_krsc, terms=TERMS):
    """x (N,H,W,Cin) fp32, w (Cout,3,3,Cin) fp32 -> (N,H,W,Cout) fp32 as the kernel forms it: K blocks of 16 channels of
    one tap in the kernel's order; within a block the listed terms in turn, each term's 16 products summed exactly
    (float64 holds them) and added to the fp32 accumulator with one rounding"""
    N, H, W, Cin = x.shape
    Cout = w_krsc.shape[0]
    xs = [np.pad(p, ((0, 0), (1, 1), (1, 1), (0, 0))).astype(np.float64) for p in split3(x)]
    ws = [p.astype(np.float64) for p in split3(w_krsc)]
    acc = np.zeros((N * H * W, Cout), np.float32)
    for tap in range(9):
        r, s = divmod(tap, 3)
        for c in range(0, Cin, 16):
            for pa, pb in terms:
                a = xs[pa][:, r:r + H, s:s + W, c:c + 16].reshape(-1, 16)
                b = ws[pb][:, r, s, c:c + 16]
                acc = (acc.astype(np.float64) + a @ b.T).astype(np.float32)
    return acc.reshape(N, H, W, Cout)


def conv_ref64(x, w_krsc, bias=None):
    """float64 conv2d of the fp32 data: (N,H,W,Cout) float64"""
    import torch
    import torch.nn.functional as F
    y = F.conv2d(torch.from_numpy(np.array(x)).double().permute(0, 3, 1, 2),
                 torch.from_numpy(np.array(w_krsc)).double().permute(0, 3, 1, 2),
                 None if bias is None else torch.from_numpy(np.array(bias)).double(), 1, 1)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(x, w_krsc, bias, rowmask) of a case: signed normal data, He-scaled weights; read only"""
    N, H, W, Cin, Cout = CASES[case]
    rng = np.random.default_rng(ord(case))
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((Cout, 3, 3, Cin)) * (2.0 / (9 * Cin)) ** 0.5).astype(np.float32)
    b = (0.3 * rng.standard_normal(Cout)).astype(np.float32)
    mask = (rng.random(N * H * W) > 0.3).astype(np.float32)
    for a in (x, w, b, mask):
        a.setflags(write=False)
    return x, w, b, mask


@functools.lru_cache(maxsize=None)
def reference(case, bias):
    x, w, b, _ = inputs(case)
    ref = conv_ref64(x, w, b if bias else None)
    ref.setflags(write=False)
    return ref


def _mantissa_values(rng, shape, bits):
    """random fp32 values with `bits` significant bits (1 = a power of two), exponents 2^-30 .. 2^10, random signs"""
    m = rng.integers(1 << (bits - 1), 1 << bits, size=shape).astype(np.float64) if bits > 1 else np.ones(shape)
    e = rng.integers(-30, 11, size=shape)
    sign = rng.choice([-1.0, 1.0], size=shape)
    v = (sign * np.ldexp(m, e - (bits - 1))).astype(np.float32)
    assert np.all(v.astype(np.float64) == sign * np.ldexp(m, e - (bits - 1)))
    return v


@functools.lru_cache(maxsize=None)
def probe(which):
    """(x, w_krsc, float64 reference) of an exactness probe at case (d)'s shape: at most one non-zero product per output
    and that product exact in fp32, so the kernel's y must equal the reference bit for bit.
      i   24-bit inputs, one non-zero weight per output channel, a power of two
      ii  one-hot x (a power of two), 24-bit weights
      iii 12-bit inputs, one non-zero 12-bit weight per output channel"""
    N, H, W, Cin, Cout = CASES["d"]
    rng = np.random.default_rng({"i": 101, "ii": 102, "iii": 103}[which])
    if which == "ii":
        x = np.zeros((N, H, W, Cin), np.float32)
        x[1, 7, 5, 37] = _mantissa_values(rng, (), 1)
        w = _mantissa_values(rng, (Cout, 3, 3, Cin), 24)
    else:
        bits = 24 if which == "i" else 12
        x = _mantissa_values(rng, (N, H, W, Cin), bits)
        w = np.zeros((Cout, 3, 3, Cin), np.float32)
        taps, chans = rng.integers(0, 9, Cout), rng.integers(0, Cin, Cout)
        taps[:9] = np.arange(9)                   # every tap and both ends of the channel range are used
        chans[:2] = (0, Cin - 1)
        w[np.arange(Cout), taps // 3, taps % 3, chans] = _mantissa_values(rng, (Cout,), 1 if which == "i" else 12)
    ref = conv_ref64(x, w)
    assert np.all(ref.astype(np.float32).astype(np.float64) == ref), "the probe's results are fp32 values"
    for a in (x, w, ref):
        a.setflags(write=False)
    return x, w, ref
