"""GPU: every route of the fused conv module (jdet_amd/ops/conv_igemm.py: conv_module, masked_conv_module,
conv3x3_bias_act, _ConvBiasAct, _conv_backward, _conv1x1_backward, _rows_backward, shared_wgrad) against float64
autograd of F.conv2d on the host.  tests/conv_route_cases.py is the case table; tests/test_conv_route_cases_cpu.py
proves, without a GPU, that the table reaches every leaf and that its EXACT tier is exact.

Every case and tier runs forward and backward through its entry point.  y and every requested gradient are compared
with the reference: EXACT tier, outputs the label gives to an own kernel: array_equal; everything else: the bounds of
the case module (own kernels 2e-5 * max|ref| + 1e-6; library / GEMM / framework outputs four times the framework
route's measured error, or the own bound where that is larger).  A gradient that was not requested is None; the no-grad
forward of an own-kernel forward is bit-equal to the training forward.

THE ROUTE TAKEN EQUALS THE LABEL: a recording proxy in place of `_lib.lib()` notes the jdet_* entry points called,
counting wrappers sit on _conv_backward / _conv1x1_backward / _rows_backward / shared_wgrad and on the alias through
which both backwards call the library's convolution_backward, and a dispatch mode notes the library convolution / GEMM
of the forward.  What was seen has to equal, call for call, what the labels of the case's uses and passes predict.
Layout contracts where the route ran: y channels-last under a fused forward; the weight gradient of a channels-last
parameter channels-last memory, and the very buffer shared_wgrad returned, under own / rows; the 1x1 weight gradient
in the parameter's own strides."""
import collections

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from tests import conv_route_cases as K

pytestmark = pytest.mark.gpu
CL = torch.channels_last
KERNELS = ("jdet_conv3x3_igemm_forward", "jdet_conv3x3_bf16x3_forward", "jdet_conv3x3_wgrad", "jdet_conv3x3_wgrad_rows",
           "jdet_conv3x3_dgrad_rows", "jdet_bias_act_backward", "jdet_channel_sum")
HOST = ("_conv_backward", "_conv1x1_backward", "_rows_backward", "shared_wgrad", "_convolution_backward")
FORWARD_OPS = {"convolution": "convolution", "addmm": "gemm", "mm": "gemm"}


# ------------------------------------------------------------------------------------------- observation
class _LibProxy:
    """stands in for the loaded library: every attribute is the library's own, the watched entry points note their call"""

    def __init__(self, real, seen, phase):
        self._real, self._seen, self._phase = real, seen, phase

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in KERNELS:
            return fn

        def call(*args):
            self._seen[(self._phase[0], name)] += 1
            return fn(*args)
        return call


class _ForwardOps(TorchDispatchMode):
    def __init__(self, seen, phase):
        super().__init__()
        self._seen, self._phase = seen, phase

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kind = FORWARD_OPS.get(getattr(getattr(func, "overloadpacket", None), "__name__", ""))
        if kind:
            self._seen[(self._phase[0], kind)] += 1
        return func(*args, **(kwargs or {}))


def _observe(monkeypatch):
    """-> (seen: Counter of (phase, what), phase: [name], buffers: data pointers shared_wgrad returned)"""
    from jdet_amd import _lib as L
    from jdet_amd.ops import conv_igemm as CI
    seen, phase, buffers = collections.Counter(), ["off"], []
    proxy = _LibProxy(L.lib(), seen, phase)
    monkeypatch.setattr(L, "lib", lambda: proxy)

    def wrap(name):
        real = getattr(CI, name)

        def call(*args, **kwargs):
            out = real(*args, **kwargs)
            what = name
            if name == "_convolution_backward":
                what = "library dgrad=%d wgrad=%d" % (bool(args[-1][0]), bool(args[-1][1]))
            elif name == "shared_wgrad":
                buffers.append(None if out is None else out.data_ptr())
            seen[(phase[0], what)] += 1
            return out
        monkeypatch.setattr(CI, name, call)

    for name in HOST:
        wrap(name)
    return seen, phase, buffers


def _predicted(c):
    """what the labels say is called, per (phase, what)"""
    want = collections.Counter()
    for lab in K.labels(c):
        fwd = {"igemm": "jdet_conv3x3_igemm_forward", "bf16x3": "jdet_conv3x3_bf16x3_forward", "gemm1x1": "gemm",
               "library": "convolution"}[lab.forward]
        want[("forward", fwd)] += 1
        if not (lab.function and any(c.need)):
            continue                                     # the framework's own backward: none of the watched calls
        want[("backward", "_conv_backward")] += 1
        if lab.bias in ("bias_act", "channel_sum"):
            want[("backward", {"bias_act": "jdet_bias_act_backward", "channel_sum": "jdet_channel_sum"}[lab.bias])] += 1
        if lab.k1:
            want[("backward", "_conv1x1_backward")] += 1
        if "rows" in (lab.dgrad, lab.wgrad):
            want[("backward", "_rows_backward")] += 1
        if lab.dgrad == "rows":
            want[("backward", "jdet_conv3x3_dgrad_rows")] += 1
        if lab.dgrad == "bf16x3":
            want[("backward", "jdet_conv3x3_bf16x3_forward")] += 1
        if lab.wgrad in ("own", "rows"):
            want[("backward", "shared_wgrad")] += 1
            want[("backward", {"own": "jdet_conv3x3_wgrad", "rows": "jdet_conv3x3_wgrad_rows"}[lab.wgrad])] += 1
        if "library" in (lab.dgrad, lab.wgrad):
            want[("backward", "library dgrad=%d wgrad=%d" % (lab.dgrad == "library", lab.wgrad == "library"))] += 1
    return collections.Counter({k: v * c.passes for k, v in want.items()})


# ------------------------------------------------------------------------------------------- running a case
def _fmt(t, fmt):
    return t.contiguous(memory_format=CL) if fmt == "cl" else t.contiguous()


def _param(dev, a, fmt, requires_grad):
    t = torch.empty(a.shape, dtype=torch.float32, device=dev, memory_format=CL if fmt == "cl" and a.ndim == 4
                    else torch.contiguous_format)
    t.copy_(torch.from_numpy(np.array(a)))
    return torch.nn.Parameter(t, requires_grad=requires_grad)


def _gradient(dev, g, form):
    if form == "scalar":
        return torch.full((), float(g.flat[0]), dtype=torch.float32, device=dev).expand(g.shape)
    return _fmt(torch.from_numpy(np.array(g)).to(dev), "nchw" if form == "nchw" else "cl")


def _entry(c, dev, w, b):
    """-> call(use, x, mask): the case's entry point"""
    from jdet_amd.models.utils.modules import ConvModule
    from jdet_amd.ops import conv_igemm as CI
    if c.entry in ("forward", "masked"):
        m = ConvModule(c.cin, c.cout, c.k, stride=c.stride, padding=c.pad, dilation=c.dil, groups=c.groups, bias=c.bias,
                       act_cfg=dict(type="ReLU") if c.relu else None).to(dev)
        m.conv.weight, m.conv.bias = w, b
        m.row_sparse_grad = c.row_sparse[0]
        assert len(set(c.row_sparse)) == 1
        if c.entry == "forward":
            return lambda u, x, mask: m(x)

        def masked(u, x, mask):
            y = m.masked(x, mask)
            assert y is not None, "ConvModule.masked declined the case"
            return y
        return masked
    if c.entry == "bias_act":
        return lambda u, x, mask: CI.conv3x3_bias_act(x, w, b, c.relu, mask, c.row_sparse[u])
    pair = lambda v: (v, v)
    return lambda u, x, mask: CI._ConvBiasAct.apply(x, w * 1.0 if c.nonleaf else w, b, c.relu, pair(c.stride), pair(c.pad),
                                                    pair(c.dil), c.groups, c.igemm, mask, c.row_sparse[u])


def run_case(dev, c, tier, monkeypatch):
    """-> NS(y[pass][use], x, w, b: the leaves with their .grad, y_last: device tensors of the last pass, seen, buffers,
    call)"""
    from jdet_amd.ops import conv_igemm as CI
    inp = K.inputs_of(c, tier)
    for name, value in c.switches.items():
        assert hasattr(CI, name)
        monkeypatch.setattr(CI, name, value)
    seen, phase, buffers = _observe(monkeypatch)
    w = _param(dev, inp.w, c.wfmt, c.need[1])
    b = _param(dev, inp.b, "nchw", c.need[2]) if c.bias else None
    xs = [_fmt(torch.from_numpy(np.array(x)).to(dev), c.xfmt).requires_grad_(c.need[0]) for x in inp.x]
    gs = [_gradient(dev, g, form) for g, form in zip(inp.g, c.grad)]
    masks = [None if m is None else torch.from_numpy(np.array(m)).to(dev) for m in inp.mask]
    call = _entry(c, dev, w, b)
    main = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(dev) if c.side is not None else None
    ys_host = []
    for p in range(c.passes):
        phase[0] = "forward"
        ys = []
        with _ForwardOps(seen, phase):
            for u in range(len(xs)):
                if u == c.side:
                    side.wait_stream(main)
                    with torch.cuda.stream(side):
                        ys.append(call(u, xs[u], masks[u]))
                    main.wait_stream(side)               # joined before the loss
                else:
                    ys.append(call(u, xs[u], masks[u]))
        phase[0] = "backward"
        if any(c.need):
            torch.autograd.backward(ys, gs)              # ONE backward pass over every use
        torch.cuda.synchronize(dev)
        phase[0] = "off"
        ys_host.append([y.detach().cpu().numpy() for y in ys])
        if p + 1 < c.passes and c.rescale != 1.0:
            version = w._version
            w.data.mul_(c.rescale)
            assert w._version == version                 # (what the fused optimizer step does: no version moves)
    return K.NS(y=ys_host, y_last=[y.detach() for y in ys], x=xs, w=w, b=b, masks=masks, seen=seen, buffers=buffers, call=call)


def errors(got, ref):
    """largest |got - ref| / max|ref| (0 for an empty array), max|ref|"""
    if not ref.size:
        return 0.0, 0.0
    scale = float(np.abs(ref).max())
    return float(np.abs(got.astype(np.float64) - ref).max()) / max(scale, 1e-300), scale


def _compare(got, ref, tier, kind, labs, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape, "%s %s: shape %r, reference %r" % (what, kind, got.shape, ref.shape)
    assert got.dtype == np.float32 and np.isfinite(got).all(), "%s %s" % (what, kind)
    axis = K.LABEL_OF[kind]
    own = all(K.exact_of(kind, l) for l in labs)
    rel, absolute = K.OWN_BOUND if own else K.LIBRARY_BOUND[kind]
    err, scale = errors(got, ref)
    exact = tier == "exact" and own
    print("conv_routes | %s | %s | %s | %s | device err %.3e | %s" % (
        what, tier, kind, "+".join(sorted({getattr(l, axis) for l in labs})), err,
        "equal" if exact else "bound %.3e" % (rel + absolute / max(scale, 1e-300))))
    if exact:
        ref32 = ref.astype(np.float32)
        bad = np.argwhere(got != ref32)
        assert bad.shape[0] == 0, "%s %s: %d of %d values differ, first at %s: got %r, reference %r" % (
            what, kind, bad.shape[0], ref.size, tuple(bad[0]), got[tuple(bad[0])], ref32[tuple(bad[0])])
    else:
        worst = float(np.abs(got.astype(np.float64) - ref).max()) if ref.size else 0.0
        assert worst <= rel * scale + absolute, "%s %s: error %.3e, bound %.3e (max|ref| %.4g)" % (
            what, kind, worst, rel * scale + absolute, scale)


def _is_cl(t):
    return t.permute(0, 2, 3, 1).is_contiguous()


@pytest.mark.parametrize("name,tier", K.PARAMS, ids=["%s-%s" % p for p in K.PARAMS])
def test_route(dev, monkeypatch, name, tier):
    c = K.BY_NAME[name]
    labs = K.labels(c)
    ref = K.reference(c, tier)
    r = run_case(dev, c, tier, monkeypatch)
    what = "%s [%s]" % (name, c.reaches)
    # ---- the route taken equals the label
    seen = {k: v for k, v in r.seen.items() if k[0] != "off" and v}
    want = dict(_predicted(c))
    print("conv_routes | %s | %s | route | %s" % (what, tier, " ".join("%s:%s=%d" % (k[0][0], k[1], v) for k, v in sorted(seen.items()))))
    assert seen == want, "%s: the route taken differs from the label\n  seen     %r\n  labelled %r" % (what, seen, want)
    # ---- values
    for p in range(c.passes):
        for u, lab in enumerate(labs):
            _compare(r.y[p][u], ref.y[p][u], tier, "y", [lab], "%s pass %d use %d" % (what, p, u))
    for u, lab in enumerate(labs):
        if c.need[0]:
            _compare(r.x[u].grad, ref.grad_x[u], tier, "grad_x", [lab], "%s use %d" % (what, u))
        else:
            assert r.x[u].grad is None
    if c.need[1]:
        _compare(r.w.grad, ref.grad_w, tier, "grad_w", labs, what)
    else:
        assert r.w.grad is None
    if c.bias and c.need[2]:
        _compare(r.b.grad, ref.grad_b, tier, "grad_b", labs, what)
    else:
        assert r.b is None or r.b.grad is None
    # ---- layout contracts, where their route ran
    for u, lab in enumerate(labs):
        if lab.forward in K.OWN["y"]:
            assert _is_cl(r.y_last[u]), "y of a fused forward is channels-last"
    if c.need[1] and c.wfmt == "cl" and all(l.wgrad in K.OWN["grad_w"] for l in labs):
        assert _is_cl(r.w.grad), "the weight gradient of a channels-last parameter is channels-last memory"
        assert len(r.buffers) == len(labs) * c.passes
        if c.side is None:
            assert [b is None for b in r.buffers] == [i % len(labs) != 0 for i in range(len(r.buffers))], \
                "one buffer per backward pass, every later use adds into it"
            if not c.nonleaf:
                assert r.w.grad.data_ptr() == r.buffers[0], "the parameter took the kernel's buffer without a copy"
    if c.need[1] and any(l.k1 for l in labs):
        assert r.w.grad.stride() == r.w.stride(), "the 1x1 weight gradient has the parameter's own strides"
    # ---- the no-grad forward of an own-kernel forward is the training forward
    with torch.no_grad():
        for u, lab in enumerate(labs):
            if lab.forward in K.OWN["y"]:
                assert torch.equal(r.call(u, r.x[u].detach(), r.masks[u]), r.y_last[u]), "no-grad forward, use %d" % u
    if c.entry == "masked" and c.need[0]:
        N, H, W = c.maps[0]
        off = (r.masks[0] == 0).view(N, 1, H, W).expand_as(r.y_last[0])
        assert not r.y_last[0][off].any(), "masked rows of y are zero"
