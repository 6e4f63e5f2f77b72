"""Case table of the fused conv module's routing tests: every leaf of the routing tree of jdet_amd/ops/conv_igemm.py
(`conv_module`, `masked_conv_module`, `conv3x3_bias_act`, `_ConvBiasAct`, `_conv_backward`, `_conv1x1_backward`,
`shared_wgrad`) at the smallest shape that reaches it.  No kernel calls; importable without a GPU.  Expected values are
float64 autograd of F.conv2d [+ relu] [* mask] on the host, summed over the uses of a shared weight and over the
backward passes of an accumulating case.

`label(case)` restates the host rules of ops/conv_igemm.py and the `*_supported` rules of the C sources.  It NAMES the
leaf a case is in (forward: igemm | bf16x3 | gemm1x1 | library; bias: bias_act | channel_sum | framework | none; dgrad:
rows | bf16x3 | gemm1x1 | library | none; wgrad: own | rows | gemm1x1 | library | none) and never produces expected
values.

EXACT tier: integer x in [-8, 8], weights / bias / incoming gradient in [-4, 4]: every product and every partial sum is
an integer below 2^24 in any order (tests/test_conv_route_cases_cpu.py proves it from the sums of absolute terms), the
operands are exact in bf16 and every ReLU decision is exact, so every output the label gives to one of the project's own
kernels has to EQUAL the float64 reference rounded to fp32.  Where the FORWARD is the library's or a GEMM (which need
not be exact) under a ReLU, the incoming gradient is zero where the float64 pre-activation is exactly 0: the one place
where a forward within rounding of the reference could decide the mask differently.
TOLERANCE tier: normal x, He-scaled weights, bias 0.1 * normal, normal gradient; under a ReLU the gradient is zero where
the float64 pre-activation has |z| < BAND * max|z| (taken from the reference; at most KEEP_CAP of a case's outputs).  A
gradient that is an expanded scalar cannot be zeroed per output: there the bias of a channel is redrawn until no
output of the channel lies in the band."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

TIERS = ("exact", "tolerance")
SWITCHES = ("ENABLED", "TRAIN", "WGRAD", "BIAS_ACT_BWD", "ROWS", "BF16X3", "BF16X3_DGRAD", "CONV1X1_GEMM")
FORWARD = ("igemm", "bf16x3", "gemm1x1", "library")
BIAS = ("bias_act", "channel_sum", "framework", "none")
DGRAD = ("rows", "bf16x3", "gemm1x1", "library", "none")
WGRAD = ("own", "rows", "gemm1x1", "library", "none")
OWN = {"y": ("igemm", "bf16x3"), "grad_b": ("bias_act", "channel_sum"), "grad_x": ("rows", "bf16x3"),
       "grad_w": ("own", "rows")}
KINDS = ("y", "grad_x", "grad_w", "grad_b")
LABEL_OF = {"y": "forward", "grad_x": "dgrad", "grad_w": "wgrad", "grad_b": "bias"}

BAND = 1e-4
KEEP_CAP = 0.005

# ------------------------------------------------------------------------------------------- bounds
# own kernels: |err| <= 2e-5 * max|ref| + 1e-6 (BOUND of tests/bf16x3_cases.py, from tests/test_gpu_conv_igemm.py)
OWN_BOUND = (2e-5, 1e-6)
# The framework route (F.conv2d [+ relu] [* mask] and its autograd on the device, fp32, every case of this table, tolerance
# tier) against the float64 reference: the largest |err| / max|ref| per output kind over two runs on an MI355X of
# scripts/conv_routes_errors.py, rounded up (per case: profiles/conv_routes.md).
LIBRARY_ERR = {"y": 7.7e-7, "grad_x": 9.3e-7, "grad_w": 7.5e-7, "grad_b": 2.7e-7}
# outputs the label gives to the library, a GEMM or the framework: four times that figure (another summation order, as
# tests/test_gpu_fcos.py allows), or the own kernels' bound where that is larger
LIBRARY_BOUND = {k: (max(4.0 * LIBRARY_ERR[k], OWN_BOUND[0]), OWN_BOUND[1]) for k in KINDS}


def exact_of(kind, lab):
    """does the label give this output to an own kernel?  (exact tier: it has to equal the reference; tolerance tier:
    OWN_BOUND, else LIBRARY_BOUND[kind] in both tiers)"""
    return getattr(lab, LABEL_OF[kind]) in OWN[kind]


# ------------------------------------------------------------------------------------------- the table
def _c(name, cin, cout, maps=((2, 13, 17),), k=3, stride=1, pad=None, dil=1, groups=1, bias=True, relu=True,
       need=(True, True, True), xfmt="cl", wfmt="cl", row_sparse=False, grad="cl", entry="forward", igemm=True,
       nonleaf=False, side=None, passes=1, rescale=1.0, switches=None, data=None, reaches=""):
    """maps: one (N, H, W) per use of the weight inside one backward pass.  need: which of x / weight / bias require a
    gradient.  xfmt / wfmt: "cl" (channels-last memory) | "nchw".  row_sparse, grad: one value, or one per use; grad is
    "cl" | "nchw" (dense, that memory order) | "scalar" (an expanded scalar, what y.sum().backward() sends) | "rows13"
    (channels-last, non-zero on 13 position rows).  entry: "forward" (ConvModule.forward) | "masked" (ConvModule.masked
    with a 0 / 1 row mask) | "bias_act" (conv3x3_bias_act) | "apply" (_ConvBiasAct.apply with `igemm` as given).
    nonleaf: the function sees weight * 1.0.  side: the use whose forward runs on a side stream.  passes: backward passes
    without clearing .grad, the weight multiplied by `rescale` in place through .data between them.  switches: module
    attributes of ops/conv_igemm set for the case.  data: the case whose inputs this one shares."""
    n = len(maps)
    per_use = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * n
    return NS(name=name, cin=cin, cout=cout, maps=tuple(maps), k=k, stride=stride, pad=dil * (k // 2) if pad is None else pad,
              dil=dil, groups=groups, bias=bias, relu=relu, need=tuple(need), xfmt=xfmt, wfmt=wfmt,
              row_sparse=per_use(row_sparse), grad=per_use(grad), entry=entry, igemm=igemm, nonleaf=nonleaf, side=side,
              passes=passes, rescale=rescale, switches=dict(switches or {}), data=data or name, reaches=reaches)


_M3 = ((2, 13, 17), (1, 5, 30), (2, 3, 3))
_BIG = ((2, 64, 64),)
CASES = [
    _c("1", 64, 64, reaches="igemm / bias_act / library dgrad / own wgrad"),
    _c("1/scalar", 64, 64, grad="scalar", reaches="case 1 under y.sum().backward()"),
    _c("1/nchw", 64, 64, xfmt="nchw", wfmt="nchw", grad="nchw", reaches="case 1 from NCHW-contiguous x, weight and gradient"),
    _c("2/rows13", 64, 64, row_sparse=True, grad="rows13", reaches="rows / rows"),
    _c("2/dense", 64, 64, row_sparse=True, grad="nchw", reaches="rows / rows under a dense gradient (the flag is a hint)"),
    _c("3/x-frozen", 64, 64, row_sparse=True, grad="rows13", need=(False, True, True), reaches="rows, need_x false"),
    _c("3/w-frozen", 64, 64, row_sparse=True, grad="rows13", need=(True, False, True), reaches="rows, need_w false"),
    _c("3/x-frozen-dense", 64, 64, need=(False, True, True), reaches="no data gradient next to the own wgrad"),
    _c("4/relu", 64, 60, reaches="bias framework under the fused forward"),
    _c("4/linear", 64, 60, relu=False, reaches="bias channel_sum under the fused forward"),
    _c("5", 64, 34, relu=False, grad="nchw", reaches="igemm forward, wgrad library, channel_sum"),
    _c("6/c15", 64, 15, relu=False, reaches="library forward through _ConvBiasAct, channel_sum"),
    _c("6/c15/scalar", 64, 15, relu=False, grad="scalar", reaches="the same under y.sum().backward()"),
    _c("6/c5", 64, 5, relu=False, reaches="library forward through _ConvBiasAct, channel_sum"),
    _c("7", 64, 15, reaches="the plain framework path"),
    _c("8/no-bias", 64, 64, bias=False, need=(True, True, False), reaches="threshold_backward, no bias"),
    _c("8/bias-frozen", 64, 64, need=(True, True, False), reaches="threshold_backward, frozen bias"),
    _c("9", 32, 1024, _BIG, reaches="forward bf16x3 (512 tiles), own wgrad, bias_act at C = 1024"),
    _c("10", 1024, 32, _BIG, reaches="dgrad bf16x3 on the flipped weights"),
    _c("11", 256, 64, ((2, 9, 7),), k=1, reaches="forward / dgrad / wgrad gemm1x1"),
    _c("11/scalar", 256, 64, ((2, 9, 7),), k=1, relu=False, grad="scalar", reaches="gemm1x1 under y.sum().backward()"),
    _c("12", 64, 128, ((2, 9, 7),), k=1, relu=False, wfmt="nchw", grad="nchw", reaches="library forward with k1, gemm1x1 gradients"),
    _c("13", 256, 64, ((1, 70, 70),), k=1, reaches="wgrad library next to dgrad gemm1x1 (4900 > 4096 positions)"),
    _c("14/x-nchw", 256, 64, ((2, 9, 7),), k=1, xfmt="nchw", reaches="not _is_1x1: NCHW-contiguous x"),
    _c("14/c32", 64, 32, ((2, 9, 7),), k=1, reaches="not _is_1x1: 32 output channels"),
    _c("14/no-bias", 256, 64, ((2, 9, 7),), k=1, bias=False, need=(True, True, False), reaches="1x1 without bias: framework"),
    _c("15/stride2", 64, 128, stride=2, reaches="library forward, one-pass bias backward"),
    _c("15/dil2", 64, 64, dil=2, reaches="library forward, one-pass bias backward"),
    _c("15/groups2", 64, 64, groups=2, reaches="library forward, one-pass bias backward"),
    _c("15/cin40", 40, 64, reaches="library forward (Cin % 16), one-pass bias backward"),
    _c("16", 64, 64, relu=False, entry="apply", igemm=False, nonleaf=True, reaches="a non-leaf weight (ORConv's bank)"),
    _c("17", 64, 64, entry="masked", reaches="relu(conv) * mask in one kernel"),
    _c("18", 64, 64, _M3, reaches="shared_wgrad: one buffer, two in-place adds"),
    _c("19/side0", 64, 64, _M3, side=0, reaches="the side-stream use runs last in backward"),
    _c("19/side1", 64, 64, _M3, side=1, reaches="the side-stream use between two sharing uses"),
    _c("19/side2", 64, 64, _M3, side=2, reaches="the side-stream use runs first in backward"),
    _c("20", 64, 64, _M3, entry="bias_act", row_sparse=(False, True, False), grad=("cl", "rows13", "nchw"),
       reaches="dense and row-list uses in one buffer"),
    _c("21/1", 64, 64, passes=2, reaches="accumulation into .grad"),
    _c("21/1/rescale", 64, 64, passes=2, rescale=2.0, reaches="the weight scaled through .data between two passes"),
    _c("21/2/rescale", 64, 64, row_sparse=True, grad="rows13", passes=2, rescale=2.0, reaches="the flipped-weight bank follows (rows)"),
    _c("21/10/rescale", 1024, 32, _BIG, passes=2, rescale=2.0, reaches="the flipped-weight bank follows (bf16x3 dgrad)"),
    _c("22/1x1x1", 64, 64, ((1, 1, 1),), reaches="a single position"),
    _c("22/n0", 64, 64, ((0, 13, 17),), reaches="an empty batch"),
    _c("23/1/ENABLED", 64, 64, switches={"ENABLED": False}, data="1", reaches="case 1, switch off"),
    _c("23/1/TRAIN", 64, 64, switches={"TRAIN": False}, data="1", reaches="case 1, switch off"),
    _c("23/1/WGRAD", 64, 64, switches={"WGRAD": False}, data="1", reaches="case 1, switch off"),
    _c("23/1/BIAS_ACT_BWD", 64, 64, switches={"BIAS_ACT_BWD": False}, data="1", reaches="case 1, switch off"),
    _c("23/2/ROWS", 64, 64, row_sparse=True, grad="rows13", switches={"ROWS": False}, data="2/rows13", reaches="case 2, switch off"),
    _c("23/9/BF16X3", 32, 1024, _BIG, switches={"BF16X3": False}, data="9", reaches="case 9, switch off"),
    _c("23/10/BF16X3_DGRAD", 1024, 32, _BIG, switches={"BF16X3_DGRAD": False}, data="10", reaches="case 10, switch off"),
    _c("23/11/CONV1X1_GEMM", 256, 64, ((2, 9, 7),), k=1, switches={"CONV1X1_GEMM": False}, data="11", reaches="case 11, switch off"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SWITCH_CASES = [c for c in CASES if c.switches]
SHARED_CASES = [c for c in CASES if len(c.maps) > 1]
# (name, tier) in an order that keeps the cases that share inputs next to each other
PARAMS = [(c.name, t) for c in sorted(CASES, key=lambda c: (c.data, c.name)) for t in TIERS]


# ------------------------------------------------------------------------------------------- the rules, restated
def igemm_supported(cin, cout):         # csrc/conv_igemm.hip
    return cin > 0 and cin % 16 == 0 and cout > 0


def bf16x3_supported(cin, cout):        # csrc/conv_bf16x3.hip
    return cin > 0 and cin % 32 == 0 and cout > 0


def wgrad_supported(cin, cout):         # csrc/conv_wgrad.hip
    return cin > 0 and cout > 0 and cin % 4 == 0 and cout % 4 == 0


def rows_supported(cin, cout):          # csrc/conv_rows.hip
    return cin > 0 and cout > 0 and cin % 4 == 0 and cout % 16 == 0


def bias_bwd_supported(c):              # ops/conv_igemm._bias_bwd_supported
    q = c // 4
    return c % 4 == 0 and ((q <= 256 and 256 % q == 0) or 256 < q <= 1024)


def fits_32bit(positions, cin, cout, pad=0):
    return (positions + pad) * max(cin, cout) < 2 ** 30


def bf16x3_big(positions, cin, cout):   # ops/conv_igemm.bf16x3_big
    tiles = ((positions + 127) // 128) * ((cout + 127) // 128)
    return tiles >= 512 and cin % 32 == 0 and fits_32bit(positions, cin, cout) and bf16x3_supported(cin, cout)


def out_hw(c, H, W):
    f = lambda n: (n + 2 * c.pad - c.dil * (c.k - 1) - 1) // c.stride + 1
    return f(H), f(W)


def switches_of(c):
    sw = {s: True for s in SWITCHES}
    sw.update(c.switches)
    return sw


def label(c, use=0):
    """-> NS(forward, bias, dgrad, wgrad; function: the call goes through _ConvBiasAct; k1: `_is_1x1` held) for one use"""
    sw = switches_of(c)
    N, H, W = c.maps[use]
    P = N * H * W                                        # (stride 1 wherever P matters)
    grad = any(c.need)
    is3 = (c.k, c.stride, c.pad, c.dil, c.groups) == (3, 1, 1, 1, 1)
    preferred = sw["ENABLED"] and is3 and igemm_supported(c.cin, c.cout) and fits_32bit(P, c.cin, c.cout) and P >= 1
    bias_grad = c.bias and c.need[2]
    # ---- which function the entry point calls
    if c.entry == "forward":
        if is3 and c.cout >= 32 and preferred and (sw["TRAIN"] or not grad):
            function, igemm = grad, True
        elif grad and sw["BIAS_ACT_BWD"] and c.bias and (bias_bwd_supported(c.cout) or (not c.relu and c.cout <= 256)):
            function, igemm = True, False
        else:
            function, igemm = False, False
    elif c.entry == "masked":
        assert c.relu and is3 and preferred and (sw["TRAIN"] or not grad), "masked_conv_module would return None"
        assert not grad or (sw["BIAS_ACT_BWD"] and bias_grad and bias_bwd_supported(c.cout)), "masked_conv_module would return None"
        function, igemm = grad, True
    elif c.entry == "bias_act":
        function, igemm = grad, True
    else:
        function, igemm = True, c.igemm
    if not function and not igemm:                       # conv(x) [+ relu] of the framework
        return NS(forward="library", bias="framework" if bias_grad else "none", dgrad="library" if c.need[0] else "none",
                  wgrad="library" if c.need[1] else "none", function=False, k1=False)
    # ---- forward
    k1 = (sw["CONV1X1_GEMM"] and (c.k, c.stride, c.pad, c.groups) == (1, 1, 0, 1) and c.cout >= 64 and c.xfmt == "cl")
    if igemm:
        forward = "bf16x3" if sw["BF16X3"] and bf16x3_big(P, c.cin, c.cout) else "igemm"
    elif k1 and c.cin >= 256 and P <= 32768:
        forward = "gemm1x1"
    else:
        forward = "library"
    # ---- bias
    if not bias_grad:
        bias = "none"
    elif sw["BIAS_ACT_BWD"] and not c.relu and not bias_bwd_supported(c.cout) and c.cout <= 256 and P > 0:
        bias = "channel_sum"
    elif sw["BIAS_ACT_BWD"] and bias_bwd_supported(c.cout) and P > 0:
        bias = "bias_act"
    else:
        bias = "framework"
    # ---- data and weight gradients
    need_x, need_w = c.need[0], c.need[1]
    if k1:
        dgrad = "gemm1x1" if need_x else "none"
        wgrad = ("gemm1x1" if P <= 4096 else "library") if need_w else "none"
    elif (igemm and c.row_sparse[use] and sw["ROWS"] and (need_x or need_w) and rows_supported(c.cin, c.cout)
          and fits_32bit(P, c.cout, c.cin, 16)):
        dgrad, wgrad = "rows" if need_x else "none", "rows" if need_w else "none"
    else:
        dgrad = "none" if not need_x else ("bf16x3" if igemm and sw["BF16X3_DGRAD"] and bf16x3_big(P, c.cout, c.cin)
                                            else "library")
        wgrad = "none" if not need_w else ("own" if igemm and sw["WGRAD"] and wgrad_supported(c.cin, c.cout) else "library")
    return NS(forward=forward, bias=bias, dgrad=dgrad, wgrad=wgrad, function=True, k1=k1)


def labels(c):
    return [label(c, u) for u in range(len(c.maps))]


def zero_at_threshold(c):
    """exact tier: is the incoming gradient zeroed where the pre-activation is exactly 0?  (a ReLU behind a forward that
    need not be exact)"""
    return c.relu and any(l.forward not in OWN["y"] for l in labels(c))


# ------------------------------------------------------------------------------------------- inputs
def seed_of(name):
    """a seed that does not depend on the interpreter's string hashing"""
    return int.from_bytes(name.encode()[:8].ljust(8, b"\0"), "little") % (2 ** 31) + len(name)


def _conv64(c, x, w, b):
    return F.conv2d(x, w, b, c.stride, c.pad, c.dil, c.groups)


def _rows13(rng, N, H, W):
    """13 position rows: both ends of the map, the ends of an image row, both sides of an image boundary"""
    P = N * H * W
    fixed = {0, P - 1, W - 1, W, H * W - 1, min(H * W, P - 1)}
    rest = [p for p in rng.permutation(P) if p not in fixed]
    return np.array(sorted(fixed) + rest[:13 - len(fixed)])


def _draw_g(rng, c, tier, form, shape):
    N, C, H, W = shape
    if form == "scalar":
        return np.full(shape, 3.0 if tier == "exact" else 0.7, np.float32)
    g = (rng.integers(-4, 5, size=shape) if tier == "exact" else rng.standard_normal(shape)).astype(np.float32)
    if form == "rows13":
        keep = np.zeros(N * H * W, np.float32)
        keep[_rows13(rng, N, H, W)] = 1
        g *= keep.reshape(N, 1, H, W)
    return g


@functools.lru_cache(maxsize=6)
def inputs(data, tier, zero_thr=False):
    """-> NS(case, x: per use (N, Cin, H, W), g: per use (N, Cout, Ho, Wo), mask: per use (N*H*W,) or None, w, b or None,
    zeroed: the fraction of outputs whose gradient the ReLU band zeroed); fp32 numpy, read only.  `data` names the case
    that owns the inputs, `zero_thr`: see zero_at_threshold"""
    c = BY_NAME[data]
    assert c.data == data
    rng = np.random.default_rng(seed_of(data + tier))
    wshape = (c.cout, c.cin // c.groups, c.k, c.k)
    if tier == "exact":
        xs = [rng.integers(-8, 9, size=(N, c.cin, H, W)).astype(np.float32) for N, H, W in c.maps]
        w = rng.integers(-4, 5, size=wshape).astype(np.float32)
        b = rng.integers(-4, 5, size=c.cout).astype(np.float32) if c.bias else None
    else:
        xs = [rng.standard_normal((N, c.cin, H, W)).astype(np.float32) for N, H, W in c.maps]
        w = (rng.standard_normal(wshape) * (2.0 / (c.k * c.k * c.cin)) ** 0.5).astype(np.float32)
        b = (0.1 * rng.standard_normal(c.cout)).astype(np.float32) if c.bias else None
    masks = [(rng.random(N * H * W) > 0.3).astype(np.float32) if c.entry == "masked" else None for N, H, W in c.maps]
    gs = [_draw_g(rng, c, tier, form, (N, c.cout) + out_hw(c, H, W)) for form, (N, H, W) in zip(c.grad, c.maps)]
    zeroed, total = 0, 0
    if c.relu:
        # float64 pre-activations of every pass: (channel, in the band?) decides what is zeroed / redrawn
        with torch.no_grad():
            zs = [[_conv64(c, torch.from_numpy(x).double(), torch.from_numpy(w).double() * c.rescale ** p, None).numpy()
                   for p in range(c.passes)] for x in xs]

        def in_band(u, bias):
            hit = np.zeros(zs[u][0].shape, bool)
            for z in zs[u]:
                z = z + (0.0 if bias is None else bias.astype(np.float64).reshape(1, -1, 1, 1))
                if z.size:
                    hit |= (z == 0) if tier == "exact" else (np.abs(z) < BAND * np.abs(z).max())
            return hit

        if "scalar" in c.grad and (tier == "tolerance" or zero_thr):
            assert tier == "tolerance" and c.bias, "an expanded scalar cannot be zeroed per output"
            for _ in range(50):
                bad = np.flatnonzero(sum(in_band(v, b).any(axis=(0, 2, 3)) for v in range(len(xs))))
                if not bad.size:
                    break
                b[bad] = (0.1 * rng.standard_normal(bad.size)).astype(np.float32)
            else:
                raise AssertionError("%s: the bias does not clear the ReLU band" % data)
        for u, form in enumerate(c.grad):
            total += gs[u].size
            if form != "scalar" and (tier == "tolerance" or zero_thr):
                hit = in_band(u, b)
                gs[u][hit] = 0
                zeroed += int(hit.sum())
    for a in xs + gs + [w] + [m for m in masks if m is not None] + ([b] if b is not None else []):
        a.setflags(write=False)
    return NS(case=c, x=xs, g=gs, mask=masks, w=w, b=b, zeroed=zeroed / max(total, 1))


def inputs_of(c, tier):
    return inputs(c.data, tier, tier == "exact" and zero_at_threshold(c))


# ------------------------------------------------------------------------------------------- the reference
def host_autograd(c, inp, dtype=torch.float64, magnitudes=False, uses=None):
    """autograd of [relu](conv2d(x, w, b)) [* mask] on the host in `dtype`, summed over `uses` (default: all) and over the
    passes -> NS(y[pass][use], grad_x[use] or None, grad_w or None, grad_b or None) as numpy.  magnitudes: every operand
    replaced by its absolute value and the ReLU left out -- the sums of absolute terms of y and of each gradient"""
    prep = (lambda a: torch.from_numpy(np.abs(a) if magnitudes else np.array(a)).to(dtype))
    uses = range(len(c.maps)) if uses is None else uses
    ys, gx = [], {u: None for u in uses}
    gw = gb = None
    for p in range(c.passes):
        w = (prep(inp.w) * c.rescale ** p).requires_grad_(c.need[1])
        b = prep(inp.b).requires_grad_(c.need[2]) if c.bias else None
        row = {}
        for u in uses:
            x = prep(inp.x[u]).requires_grad_(c.need[0])
            y = _conv64(c, x, w, b)
            if c.relu and not magnitudes:
                y = torch.relu(y)
            if inp.mask[u] is not None:
                N, H, W = c.maps[u]
                y = y * prep(inp.mask[u]).view(N, 1, H, W)
            row[u] = y.detach().numpy()
            if any(c.need):
                y.backward(prep(inp.g[u]))
            if c.need[0]:
                gx[u] = x.grad.numpy() if gx[u] is None else gx[u] + x.grad.numpy()
        ys.append(row)
        if c.need[1]:
            gw = w.grad.numpy() if gw is None else gw + w.grad.numpy()
        if c.bias and c.need[2]:
            gb = b.grad.numpy() if gb is None else gb + b.grad.numpy()
    return NS(y=ys, grad_x=gx, grad_w=gw, grad_b=gb)


@functools.lru_cache(maxsize=6)
def _reference(data, tier, zero_thr, passes, rescale):
    c = BY_NAME[data]
    assert (c.passes, c.rescale) == (passes, rescale)
    return host_autograd(c, inputs(data, tier, zero_thr))


def reference(c, tier):
    """the float64 reference of a case (shared by the cases that share its inputs)"""
    return _reference(c.data, tier, tier == "exact" and zero_at_threshold(c), c.passes, c.rescale)
