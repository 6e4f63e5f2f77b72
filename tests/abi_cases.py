"""One table row per entry point of include/jdet_hip.h for the buffer-contract protocol of tests/guarded.py: a builder
`fn(run)` that takes every buffer from the run, calls the entry point and returns the outputs with their reference.
Importable without a GPU (tests/test_guarded_cpu.py checks that no entry point is left out); the rows run in
tests/test_gpu_abi_buffers.py.

Every bound below is the bound of the existing test of that kernel, cited next to it; bit-exact kernels (copies,
codec-free index work, NMS keep sets) are compared for equality.

The detector features (ATSS, FCOS, RepPoints, H2RBox, localization distillation) and the row-sparse / bf16x3
convolutions have factories that return a `Case`: their smallest instances are rows here, and their feature tests
(tests/test_gpu_<feature>.py) run the same factories over every regime of the kernel.  Every builder reaches the
library through this module's `lib()`: the CPU dry run replaces it."""
import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as F

from jdet_amd import _lib as L

CASES = []
I32, U8, F32 = torch.int32, torch.uint8, torch.float32


class Case:
    def __init__(self, entry_points, label, fn):
        self.entry_points, self.label, self.fn = tuple(entry_points), label, fn
        self.id = "%s[%s]" % (self.entry_points[0], label)


def row(entry_points, label):
    if isinstance(entry_points, str):
        entry_points = (entry_points,)

    def deco(fn):
        CASES.append(Case(entry_points, label, fn))
        return fn
    return deco


def lib():
    return L.lib()


def P(t):
    return None if t is None else t.data_ptr()


def ST(t):
    """the stream argument: the current HIP stream of the tensor's device"""
    return L.stream_ptr(t) if t.is_cuda else None


def Res(outs, ref, atomic=False):
    from tests import guarded
    return guarded.Result(outs, ref, atomic)


def rel(ref, r, a=0.0):
    """(ref, bound) with bound = r * max|ref| + a"""
    ref = np.asarray(ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref, np.float64)
    return ref, r * (float(np.abs(ref).max()) if ref.size else 0.0) + a


def exact(ref):
    return (ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)), 0.0


def rng_of(*key):
    return np.random.default_rng(abs(hash(tuple(int(k * 16) if isinstance(k, float) else k for k in key))) % (2 ** 31))


def randn(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


# ======================================================================================================================
# the MFMA convolutions and their neighbours
# ======================================================================================================================
CONV_FWD = (2e-5, 1e-6)      # tests/test_gpu_conv_igemm.py:45, tests/test_gpu_conv_bn.py:22 (_close, rel 2e-5 at :86)
CONV_WGRAD3 = (2e-5, 1e-6)   # tests/test_gpu_conv_wgrad.py:48
CONV_WGRAD = (5e-5, 1e-5)    # tests/test_gpu_conv_bn.py:136
BN_SUMS = (5e-5, 1e-6)       # tests/test_gpu_conv_bn.py:111 (_close at 5e-5)


def conv64(x_nhwc, w_krsc, stride=1):
    R = w_krsc.shape[1]
    y = F.conv2d(t64(x_nhwc).permute(0, 3, 1, 2), t64(w_krsc).permute(0, 3, 1, 2), None, stride, R // 2)
    return y.permute(0, 2, 3, 1).contiguous()


def deform_cols(x_nhwc, offset, k=3, pad=1, stride=1, dil=1):
    """deformable im2col of a channels-last map from the oracle's sampling (the reference's fp32 arithmetic, bit-equal to
    its kernel: tests/test_gpu_reference_kernels.py:158), as (B*Ho*Wo, k*k, C) like tests/test_gpu_dcn_arf.py:40 --
    the reference of the existing tests of the fused deformable forms (column matrix, then the product in float64)"""
    from oracle import oracle as O
    x = np.asarray(x_nhwc, np.float32)
    B, H, W, C = x.shape
    Ho, Wo = offset.shape[2:]
    col = O.deform_im2col(x.transpose(0, 3, 1, 2), offset, k, k, (pad, pad), (stride, stride), (dil, dil), 1)
    return col.reshape(C, k * k, B, Ho, Wo).transpose(2, 3, 4, 1, 0).reshape(B * Ho * Wo, k * k, C).astype(np.float64)


def _igemm(shape, Cout, tile, ws_mode, deform=False, plain=False):
    N, H, W, Cin = shape
    rng = rng_of(N, H, W, Cin, Cout, deform)
    x0 = randn(rng, N, H, W, Cin)
    w0 = randn(rng, Cout, 3, 3, Cin, scale=(2.0 / (9 * Cin)) ** 0.5)
    b0 = None if plain else randn(rng, Cout)
    m0 = None if plain else (rng.random(N * H * W) > 0.3).astype(np.float32)
    off0 = randn(rng, N, 18, H, W, scale=2.5) if deform else None
    relu = 0 if plain else 1

    def fn(run):
        x, w = run.inp("x", x0), run.inp("w", w0)
        b = None if b0 is None else run.inp("bias", b0)
        m = None if m0 is None else run.inp("rowmask", m0)
        off = None if off0 is None else run.inp("offset", off0)
        y = run.out("y", (N, H, W, Cout))
        ws, wsb = None, 0
        if ws_mode == "ws":
            need = lib().jdet_conv3x3_igemm_workspace(N, H, W, Cin, Cout)
            assert need > 0, "this shape must split its K steps over workgroups"
            ws, wsb = run.ws("workspace", need)
        run.ok(lib().jdet_conv3x3_igemm_forward(P(x), N, H, W, Cin, P(w), Cout, P(b), relu, P(m), P(off), tile, P(y),
                                                P(ws), wsb, ST(x)), "jdet_conv3x3_igemm_forward")

        def ref():
            if deform:
                r = torch.from_numpy(deform_cols(x0, off0).reshape(N * H * W, -1) @
                                     w0.reshape(Cout, -1).astype(np.float64).T).view(N, H, W, Cout)
            else:
                r = conv64(x0, w0)
            if b0 is not None:
                r = torch.relu(r + t64(b0)) * t64(m0).view(N, H, W, 1)
            return {"y": rel(r, *CONV_FWD)}
        return Res({"y": y}, ref)
    return fn


for _cout in (15, 40):
    for _tile in (0, 64, 65, 66, 128, 129, 130):
        row("jdet_conv3x3_igemm_forward", "x(1,7,9,32) Cout %d bias relu rowmask tile %d" % (_cout, _tile))(
            _igemm((1, 7, 9, 32), _cout, _tile, None))
row("jdet_conv3x3_igemm_forward", "x(1,7,9,32) Cout 40 tile 0 dirty workspace")(_igemm((1, 7, 9, 32), 40, 0, "ws"))
for _tile in (0, 65):
    row("jdet_conv3x3_igemm_forward", "x(1,6,6,48) Cout 40 tile %d" % _tile)(_igemm((1, 6, 6, 48), 40, _tile, None))
row("jdet_conv3x3_igemm_forward", "x(1,6,6,48) Cout 40 tile 0 dirty workspace")(_igemm((1, 6, 6, 48), 40, 0, "ws"))
for _tile in (0, 64):
    row("jdet_conv3x3_igemm_forward", "deformable x(1,7,9,32) Cout 40 tile %d" % _tile)(
        _igemm((1, 7, 9, 32), 40, _tile, None, deform=True, plain=True))


def bn_arrays(rng, C):
    return (rng.random(C).astype(np.float32) + 0.5, randn(rng, C, scale=0.3), randn(rng, C, scale=0.2),
            rng.random(C).astype(np.float32) + 0.5)


def bn_affine64(bn, eps=1e-5):
    g, b, m, v = (np.asarray(a, np.float64) for a in bn)
    a = g / np.sqrt(v + eps)
    return a, b - m * a


def _epilogue(mode, affine=0, relu=0, bn=None, residual=None, grad_out=None, act=None, sums=None, eps=1e-5):
    ep = L.ConvEpilogue()
    ep.mode, ep.affine, ep.relu = mode, affine, relu
    if bn is not None:
        ep.bn.weight, ep.bn.bias, ep.bn.mean, ep.bn.var = (P(t) for t in bn)
    ep.bn.eps = eps
    ep.residual, ep.grad_out, ep.act, ep.sums = P(residual), P(grad_out), P(act), P(sums)
    return ep


def _out_dim(H, R, s):
    return (H + 2 * (R // 2) - R) // s + 1


def _conv_bn(shape, Cout, R, stride, mode, tile=0, use_ws=False, expect_ws=None):
    N, H, W, Cin = shape
    Ho, Wo = _out_dim(H, R, stride), _out_dim(W, R, stride)
    rng = rng_of(N, H, W, Cin, Cout, R, stride, mode)
    x0 = randn(rng, N, H, W, Cin)
    w0 = randn(rng, Cout, R, R, Cin, scale=1.0 / (R * Cin ** 0.5))
    bn0 = bn_arrays(rng, Cout)
    res0 = randn(rng, N, Ho, Wo, Cout)              # FORWARD: residual; ADD: grad_out
    below0 = randn(rng, N, Ho, Wo, Cout)            # the conv output of the layer below (ADD / MASK)
    a64, sh64 = bn_affine64(bn0)
    act0 = np.maximum(below0.astype(np.float64) * a64 + sh64, 0).astype(np.float32)

    def fn(run):
        need = lib().jdet_conv_bn_workspace(N, H, W, Cin, Cout, R, stride)
        if expect_ws is not None:
            assert (need > 0) == expect_ws, "workspace query %d" % need
        x, w = run.inp("x", x0), run.inp("w", w0)
        bn = [run.inp(n, a) for n, a in zip(("bn.weight", "bn.bias", "bn.mean", "bn.var"), bn0)]
        y = run.out("y", (N, Ho, Wo, Cout))
        outs = {"y": y}
        sums = None
        if mode == L.EPI_FORWARD:
            res = run.inp("residual", res0)
            ep = _epilogue(mode, 1, 1, bn, residual=res)
        elif mode == L.EPI_ADD:
            go, act = run.inp("grad_out", res0), run.inp("act", act0)
            ep = _epilogue(mode, grad_out=go, act=act)
        else:
            act = run.inp("act", act0)
            rows = lib().jdet_conv_bn_sums_rows(N, H, W, Cin, Cout, R, stride, tile, 1 if use_ws else 0)
            sums = run.out("sums", (rows, 2, Cout))                 # exactly the rows the query names
            ep = _epilogue(mode, bn=bn, act=act, sums=sums)
        ws, wsb = None, 0
        if use_ws:
            ws, wsb = run.ws("workspace", need)
        run.ok(lib().jdet_conv_bn_forward(P(x), N, H, W, Cin, P(w), Cout, R, stride, ctypes.byref(ep), tile, P(y),
                                          P(ws), wsb, ST(x)), "jdet_conv_bn_forward")
        if mode == L.EPI_MASK:
            dgamma, dbeta = run.out("dgamma", (Cout,)), run.out("dbeta", (Cout,))
            job = (L.BnSumsJob * 1)()
            job[0].partial, job[0].rows, job[0].C = P(sums), sums.shape[0], Cout
            job[0].gamma, job[0].grad_gamma, job[0].grad_beta = P(bn[0]), P(dgamma), P(dbeta)
            run.ok(lib().jdet_bn_sums_finish(job, 1, ST(x)), "jdet_bn_sums_finish")
            outs.update(dgamma=dgamma, dbeta=dbeta)

        def ref():
            conv = conv64(x0, w0, stride)
            if mode == L.EPI_FORWARD:
                return {"y": rel(torch.relu(conv * torch.from_numpy(a64) + torch.from_numpy(sh64) + t64(res0)), *CONV_FWD)}
            live = t64(act0) > 0
            if mode == L.EPI_ADD:
                return {"y": rel(conv + t64(res0) * live, *CONV_FWD)}
            gm = conv * live
            xhat = (t64(below0) - t64(bn0[2])) / torch.sqrt(t64(bn0[3]) + 1e-5)
            ref_gamma = (gm * xhat).sum((0, 1, 2))
            # tests/test_gpu_conv_bn.py:113-114: dgamma = (sum g * (act - beta)) / gamma cancels against sum |g|
            gamma_bound = 5e-5 * max(float(ref_gamma.abs().max()), float(gm.abs().sum((0, 1, 2)).max()) * 1e-2) + 1e-5
            return {"y": rel(gm * torch.from_numpy(a64), *CONV_FWD), "dbeta": rel(gm.sum((0, 1, 2)), *BN_SUMS),
                    "dgamma": (ref_gamma.numpy(), gamma_bound)}
        return Res(outs, ref)
    return fn


row("jdet_conv_bn_forward", "FORWARD residual relu x(1,17,9,64) Cout 40 R1")(
    _conv_bn((1, 17, 9, 64), 40, 1, 1, L.EPI_FORWARD, expect_ws=False))
for _shape, _cout, _r, _s in (((1, 15, 13, 64), 64, 3, 2), ((1, 9, 7, 48), 40, 3, 1)):
    for _ws in (False, True):
        row("jdet_conv_bn_forward", "FORWARD x%s Cout %d R%d s%d%s" % (str(_shape).replace(" ", ""), _cout, _r, _s,
                                                                     " dirty workspace" if _ws else ""))(
            _conv_bn(_shape, _cout, _r, _s, L.EPI_FORWARD, use_ws=_ws, expect_ws=True))
row("jdet_conv_bn_forward", "ADD x(1,9,7,48) Cout 40 R3 dirty workspace")(
    _conv_bn((1, 9, 7, 48), 40, 3, 1, L.EPI_ADD, use_ws=True, expect_ws=True))
row("jdet_conv_bn_forward", "ADD x(1,17,9,64) Cout 40 R1")(_conv_bn((1, 17, 9, 64), 40, 1, 1, L.EPI_ADD, expect_ws=False))
for _tile in (0, 64, 128):
    row(("jdet_conv_bn_forward", "jdet_bn_sums_finish"), "MASK sums x(1,9,7,48) Cout 40 R3 tile %d" % _tile)(
        _conv_bn((1, 9, 7, 48), 40, 3, 1, L.EPI_MASK, tile=_tile, expect_ws=True))
    row(("jdet_conv_bn_forward", "jdet_bn_sums_finish"), "MASK sums x(1,17,9,64) Cout 40 R1 tile %d" % _tile)(
        _conv_bn((1, 17, 9, 64), 40, 1, 1, L.EPI_MASK, tile=_tile, expect_ws=False))
row(("jdet_conv_bn_forward", "jdet_bn_sums_finish"), "MASK sums x(1,9,7,48) Cout 40 R3 K split, dirty workspace")(
    _conv_bn((1, 9, 7, 48), 40, 3, 1, L.EPI_MASK, use_ws=True, expect_ws=True))


def _wgrad(general, Cout, R, stride, ksplit, deform=False):
    N, H, W, Cin = 1, 7, 9, 32
    Ho, Wo = _out_dim(H, R, stride), _out_dim(W, R, stride)
    rng = rng_of(Cout, R, stride, deform, general)
    x0, gy0 = randn(rng, N, H, W, Cin), randn(rng, N, Ho, Wo, Cout)
    base0 = randn(rng, Cout, R, R, Cin)
    off0 = randn(rng, N, 18, H, W, scale=2.5) if deform else None

    def fn(run):
        x, gy = run.inp("x", x0), run.inp("gy", gy0)
        off = None if off0 is None else run.inp("offset", off0)
        gw = run.acc("gw", base0)
        if general:
            rc = lib().jdet_conv_wgrad(P(x), P(gy), N, H, W, Cin, Cout, R, stride, P(gw), ksplit, ST(x))
        else:
            rc = lib().jdet_conv3x3_wgrad(P(x), P(gy), P(off), N, H, W, Cin, Cout, P(gw), ksplit, ST(x))
        run.ok(rc, "wgrad")

        def ref():
            if deform:
                r = (gy0.reshape(-1, Cout).astype(np.float64).T @ deform_cols(x0, off0).reshape(N * H * W, -1))
                return {"gw": rel(r.reshape(Cout, 3, 3, Cin), *CONV_WGRAD3)}
            w64 = torch.zeros(Cout, Cin, R, R, dtype=torch.float64, requires_grad=True)
            yy = F.conv2d(t64(x0).permute(0, 3, 1, 2), w64, None, stride, R // 2)
            (g,) = torch.autograd.grad(yy, w64, t64(gy0).permute(0, 3, 1, 2))
            return {"gw": rel(g.permute(0, 2, 3, 1), *(CONV_WGRAD if general else CONV_WGRAD3))}
        return Res({"gw": gw}, ref, atomic=True)
    return fn


for _cout in (8, 128):
    for _ks in (0, 1, 3):
        row("jdet_conv3x3_wgrad", "x(1,7,9,32) Cout %d ksplit %d" % (_cout, _ks))(_wgrad(False, _cout, 3, 1, _ks))
        for _r, _s in ((1, 1), (3, 2)):
            row("jdet_conv_wgrad", "x(1,7,9,32) Cout %d R%d s%d ksplit %d" % (_cout, _r, _s, _ks))(
                _wgrad(True, _cout, _r, _s, _ks))
    row("jdet_conv3x3_wgrad", "offset x(1,7,9,32) Cout %d ksplit 0" % _cout)(_wgrad(False, _cout, 3, 1, 0, deform=True))


@row("jdet_conv_dgrad_weights", "jobs (40,48,9 taps) + (64,16,1 tap)")
def _dgrad_weights(run):
    import struct
    rng = rng_of(40, 48, 64, 16)
    specs = [(40, 48, 9), (64, 16, 1)]
    srcs0 = [randn(rng, co, taps, ci) for co, ci, taps in specs]
    srcs = [run.inp("src%d" % k, a) for k, a in enumerate(srcs0)]
    dsts = [run.out("dst%d" % k, (ci, taps, co)) for k, (co, ci, taps) in enumerate(specs)]
    rec, tiles = b"", 0
    for (co, ci, taps), s, d in zip(specs, srcs, dsts):
        rec += struct.pack("<QQiiii", s.data_ptr(), d.data_ptr(), co, ci, taps, tiles)
        tiles += -(-co // 32) * -(-ci // 32) * taps
    table = run.inp("jobs", np.frombuffer(rec, np.uint8).copy())
    run.ok(lib().jdet_conv_dgrad_weights(P(table), len(specs), tiles, ST(table)), "jdet_conv_dgrad_weights")
    # dst[ci][taps-1-tap][co] = src[co][tap][ci]: flip / permute, a copy
    return Res({"dst%d" % k: d for k, d in enumerate(dsts)},
               lambda: {"dst%d" % k: exact(a[:, ::-1, :].transpose(2, 1, 0)) for k, a in enumerate(srcs0)})


def close(ref, rtol, atol):
    """(ref, element-wise bound atol + rtol * |ref|): the allclose form of the cited tests"""
    ref = np.asarray(ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref, np.float64)
    return ref, atol + rtol * np.abs(ref)


# ---- eval-mode BatchNorm / bias passes (csrc/frozen_bn.hip), P = 333 rows ----------------------------------------------
BN_P = 333
BN_Y = (1e-5, 1e-5)          # tests/test_gpu_frozen_bn.py:55   (rtol, atol)
BN_GRAD_RTOL = 1e-4          # tests/test_gpu_frozen_bn.py:59-60: rtol 1e-4, atol 2e-5 * max(1, max|ref|)


def bn_grad(ref):
    ref = np.asarray(ref, np.float64)
    return close(ref, BN_GRAD_RTOL, 2e-5 * max(1.0, float(np.abs(ref).max())))


def _bn_inputs(C, seed):
    rng = rng_of(BN_P, C, seed)
    bn0 = bn_arrays(rng, C)
    x0, r0, gy0 = randn(rng, BN_P, C), randn(rng, BN_P, C), randn(rng, BN_P, C)
    return rng, bn0, x0, r0, gy0


def _frozen_fwd(C, with_res, relu, null_affine):
    rng, bn0, x0, r0, _ = _bn_inputs(C, 1)

    def fn(run):
        x = run.inp("x", x0)
        r = run.inp("residual", r0) if with_res else None
        bn = [run.inp(n, a) for n, a in zip(("weight", "bias", "mean", "var"), bn0)]
        y = run.out("y", (BN_P, C))
        run.ok(lib().jdet_frozen_bn_act_forward(P(x), P(r), BN_P, C, None if null_affine else P(bn[0]),
                                                None if null_affine else P(bn[1]), P(bn[2]), P(bn[3]), 1e-5, relu, P(y),
                                                ST(x)), "jdet_frozen_bn_act_forward")

        def ref():
            g = np.ones(C) if null_affine else bn0[0].astype(np.float64)
            b = np.zeros(C) if null_affine else bn0[1].astype(np.float64)
            v = (x0.astype(np.float64) - bn0[2]) / np.sqrt(bn0[3].astype(np.float64) + 1e-5) * g + b
            if with_res:
                v = v + r0
            return {"y": close(np.maximum(v, 0) if relu else v, *BN_Y)}
        return Res({"y": y}, ref)
    return fn


def _relu_act(rng, P_, C):
    """an activation map with exact zeros (the ReLU mask) and no value within rounding of zero"""
    y = randn(rng, P_, C)
    return np.where(y > 0, y + 0.01, 0).astype(np.float32)


def _frozen_bwd(C, full):
    rng, bn0, x0, _, gy0 = _bn_inputs(C, 2)
    y0 = _relu_act(rng, BN_P, C)

    def fn(run):
        gy, y, x = run.inp("grad_y", gy0), run.inp("y", y0), run.inp("x", x0)
        bn = [run.inp(n, a) for n, a in zip(("weight", "bias", "mean", "var"), bn0)]
        gx = run.out("grad_x", (BN_P, C))
        outs = {"grad_x": gx}
        gr = gw = gb = ws = None
        wsb = 0
        if full:
            gr, gw, gb = run.out("grad_residual", (BN_P, C)), run.out("grad_weight", (C,)), run.out("grad_bias", (C,))
            ws, wsb = run.ws("workspace", lib().jdet_frozen_bn_act_backward_workspace(BN_P, C))
            outs.update(grad_residual=gr, grad_weight=gw, grad_bias=gb)
        run.ok(lib().jdet_frozen_bn_act_backward(P(gy), P(y), P(x), BN_P, C, P(bn[0]), P(bn[1]), P(bn[2]), P(bn[3]), 1e-5,
                                                 1, P(gx), P(gr), P(gw), P(gb), P(ws), wsb, ST(x)),
               "jdet_frozen_bn_act_backward")

        def ref():
            g = gy0.astype(np.float64) * (y0 > 0)
            inv = 1.0 / np.sqrt(bn0[3].astype(np.float64) + 1e-5)
            out = {"grad_x": bn_grad(g * (bn0[0] * inv))}
            if full:
                out.update(grad_residual=bn_grad(g), grad_bias=bn_grad(g.sum(0)),
                           grad_weight=bn_grad((g * ((x0.astype(np.float64) - bn0[2]) * inv)).sum(0)))
            return out
        return Res(outs, ref)
    return fn


def _bias_act_bwd(C, relu):
    rng, _, _, _, gy0 = _bn_inputs(C, 3)
    y0 = _relu_act(rng, BN_P, C)

    def fn(run):
        gy = run.inp("grad_y", gy0)
        y = run.inp("y", y0) if relu else None
        gp = run.out("grad_pre", (BN_P, C)) if relu else None
        gb = run.out("grad_bias", (C,))
        ws, wsb = run.ws("workspace", lib().jdet_frozen_bn_act_backward_workspace(BN_P, C))
        run.ok(lib().jdet_bias_act_backward(P(gy), P(y), BN_P, C, relu, P(gp), P(gb), P(ws), wsb, ST(gy)),
               "jdet_bias_act_backward")

        def ref():
            g = gy0.astype(np.float64) * (y0 > 0) if relu else gy0.astype(np.float64)
            # tests/test_gpu_conv_igemm.py:197 (the masked gradient is a copy) and :199
            out = {"grad_bias": (g.sum(0), 1e-5 * float(np.abs(g).sum(0).max()) + 1e-6)}
            if relu:
                out["grad_pre"] = exact(gy0 * (y0 > 0))
            return out
        return Res({"grad_bias": gb, "grad_pre": gp} if relu else {"grad_bias": gb}, ref)
    return fn


def _bn_out_bwd(C, form, with_sums):
    rng, bn0, _, other0, gy0 = _bn_inputs(C, 4 + len(form))
    y0 = _relu_act(rng, BN_P, C)

    def fn(run):
        gy, y = run.inp("grad_y", gy0), run.inp("y", y0)
        idn = run.inp("identity", other0) if form == "identity" else None
        own = run.inp("own_output", other0) if form == "own_output" else None
        bn = [run.inp(n, a) for n, a in zip(("weight", "bias", "mean", "var"), bn0)]
        gc = run.out("grad_c", (BN_P, C))
        outs = {"grad_c": gc}
        sums, sb = None, 0
        if with_sums:
            rows = lib().jdet_bn_act_backward_from_output_rows(BN_P, C)
            assert rows > 0
            sums = run.out("sums", (rows, 2, C))
            sb = sums.numel() * 4
        run.ok(lib().jdet_bn_act_backward_from_output(P(gy), P(y), P(idn), P(own), BN_P, C, P(bn[0]), P(bn[1]), P(bn[2]),
                                                      P(bn[3]), 1e-5, P(gc), P(sums), sb, ST(gy)),
               "jdet_bn_act_backward_from_output")
        if with_sums:
            dgamma, dbeta = run.out("dgamma", (C,)), run.out("dbeta", (C,))
            job = (L.BnSumsJob * 1)()
            job[0].partial, job[0].rows, job[0].C = P(sums), sums.shape[0], C
            job[0].gamma, job[0].grad_gamma, job[0].grad_beta = P(bn[0]), P(dgamma), P(dbeta)
            run.ok(lib().jdet_bn_sums_finish(job, 1, ST(gy)), "jdet_bn_sums_finish")
            outs.update(dgamma=dgamma, dbeta=dbeta)

        def ref():
            g = gy0.astype(np.float64) * (y0 > 0)
            a = bn0[0] / np.sqrt(bn0[3].astype(np.float64) + 1e-5)
            t = {"plain": y0.astype(np.float64), "identity": y0.astype(np.float64) - other0,
                 "own_output": other0.astype(np.float64)}[form] - bn0[1]
            out = {"grad_c": bn_grad(g * a)}
            if with_sums:        # tests/test_gpu_conv_bn.py:242 (_close at 1e-4: every BatchNorm gradient of a block)
                out.update(dbeta=rel(g.sum(0), 1e-4, 1e-6), dgamma=rel((g * t).sum(0) / bn0[0], 1e-4, 1e-6))
            return out
        return Res(outs, ref)
    return fn


for _c in (8, 64, 1028):
    row("jdet_frozen_bn_act_forward", "(333,%d) residual relu" % _c)(_frozen_fwd(_c, True, 1, False))
    row("jdet_frozen_bn_act_forward", "(333,%d) weight/bias NULL" % _c)(_frozen_fwd(_c, False, 0, True))
    row("jdet_frozen_bn_act_backward", "(333,%d) every gradient, dirty workspace" % _c)(_frozen_bwd(_c, True))
    row("jdet_frozen_bn_act_backward", "(333,%d) optional outputs NULL" % _c)(_frozen_bwd(_c, False))
    row("jdet_bias_act_backward", "(333,%d) relu, dirty workspace" % _c)(_bias_act_bwd(_c, 1))
    row("jdet_bias_act_backward", "(333,%d) no relu, grad_pre NULL" % _c)(_bias_act_bwd(_c, 0))
    for _form in ("plain", "identity", "own_output"):
        row(("jdet_bn_act_backward_from_output", "jdet_bn_sums_finish"), "(333,%d) t: %s, sums" % (_c, _form))(
            _bn_out_bwd(_c, _form, True))
    row("jdet_bn_act_backward_from_output", "(333,%d) sums NULL" % _c)(_bn_out_bwd(_c, "plain", False))


def _channel_sum(C):
    x0 = randn(rng_of(BN_P, C, 9), BN_P, C)

    def fn(run):
        x, out = run.inp("x", x0), run.out("sums", (C,))
        ws, wsb = run.ws("workspace", lib().jdet_channel_sum_workspace(BN_P, C))
        run.ok(lib().jdet_channel_sum(P(x), BN_P, C, P(out), P(ws), wsb, ST(x)), "jdet_channel_sum")
        # tests/test_gpu_frozen_bn.py:123
        return Res({"sums": out}, lambda: {"sums": (x0.astype(np.float64).sum(0),
                                                    1e-5 * max(1.0, float(np.abs(x0).sum(0).max())))})
    return fn


for _c in (5, 15):
    row("jdet_channel_sum", "(333,%d) dirty workspace" % _c)(_channel_sum(_c))


# ======================================================================================================================
# scans, sorted gathers, reductions
# ======================================================================================================================
def ulps(ref, n):
    """(ref, element-wise bound of n float32 ulps of the reference value)"""
    ref = np.asarray(ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref, np.float32)
    return ref.astype(np.float64), n * np.spacing(np.abs(ref)).astype(np.float64)


NMS_N = 130                  # three 64-box column blocks, the last one ragged; `keep` is 130 bytes


def _nms_boxes(rng, horizontal=False):
    from tests import inputs as I
    b = I.clustered_obbs(rng, NMS_N, n_clusters=6, extent=120.0, jitter=5.0, wh=(20.0, 60.0))
    if horizontal:
        b[:, 4] = 0.0
    scores = (rng.uniform(0, 1, NMS_N) + np.arange(NMS_N) * 1e-6).astype(np.float32)
    return b, scores


def _label_order(scores, labels):
    order = np.argsort(-scores, kind="stable")
    return order[np.argsort(labels[order], kind="stable")].astype(np.int32)


def _greedy_hbb_keep(boxes5, order, labels, thr):
    """greedy NMS on horizontal boxes [xc, yc, w, h, 0] with inter / (a + b - inter) in float64, suppression at
    iou > thr; different labels never suppress.  No decision may sit within fp32 reach of the threshold."""
    b = boxes5.astype(np.float64)
    x1, y1, x2, y2 = b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2
    w = np.clip(np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]), 0, None)
    h = np.clip(np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]), 0, None)
    area = b[:, 2] * b[:, 3]
    iou = w * h / (area[:, None] + area[None] - w * h)
    assert np.abs(iou - thr).min() > 1e-5
    keep, dead = np.zeros(len(b), np.uint8), np.zeros(len(b), bool)
    for i in order:
        if dead[i]:
            continue
        keep[i] = 1
        dead |= (iou[i] > thr) & (labels == labels[i])
    return keep


def _nms(kind, box_len=5, horizontal=0, n_labels=1):
    rng = rng_of(NMS_N, box_len, horizontal, n_labels, len(kind))
    boxes0, scores = _nms_boxes(rng, bool(horizontal))
    thr = 0.3
    if box_len == 6:
        labels = rng.integers(0, 4, NMS_N)
        labels[labels == 2] = 3                           # label 2 absent
        if n_labels == 1:
            order0 = np.argsort(-scores, kind="stable").astype(np.int32)
        else:
            order0 = _label_order(scores, labels)
        dets0 = np.concatenate([boxes0, labels[:, None].astype(np.float32)], 1)
    else:
        labels = np.zeros(NMS_N, np.int64)
        order0 = np.argsort(-scores, kind="stable").astype(np.int32)
        dets0 = boxes0

    def fn(run):
        dets, order = run.inp("dets", dets0), run.inp("order", order0, guard=0)
        keep = run.out("keep", (NMS_N,), U8)
        ws, wsb = run.ws("workspace", lib().jdet_nms_rotated_workspace(NMS_N))
        if kind == "rotated":
            rc = lib().jdet_nms_rotated(P(dets), NMS_N, box_len, P(order), thr, 0, 0, P(keep), P(ws), wsb, ST(dets))
        else:
            rc = lib().jdet_nms_labeled(P(dets), NMS_N, box_len, P(order), thr, 0, 0, horizontal, n_labels, P(keep),
                                        P(ws), wsb, ST(dets))
        run.ok(rc, "jdet_nms_" + kind)

        def ref():
            from oracle import oracle as O
            if horizontal:
                return {"keep": exact(_greedy_hbb_keep(boxes0, order0, labels, thr))}
            return {"keep": exact(O.nms_rotated_keep(dets0, order0, thr, cmp_ge=0).astype(np.uint8))}
        return Res({"keep": keep}, ref)
    return fn


row("jdet_nms_rotated", "n 130 box_len 5")(_nms("rotated"))
row("jdet_nms_rotated", "n 130 box_len 6")(_nms("rotated", 6))
for _hz in (0, 1):
    for _nl in (1, 4):
        row("jdet_nms_labeled", "n 130 horizontal %d n_labels %d (label 2 absent)" % (_hz, _nl))(
            _nms("labeled", 6, _hz, _nl))


_POLY_CACHE = {}


def _nms_polys():
    """130 near-rectangles with heavy overlap (tests/test_gpu_poly.py:64-72), their scores, and the smallest distance
    of a pairwise IoU from the threshold -- computed once for the three rows that use them"""
    if not _POLY_CACHE:
        rng = rng_of(NMS_N, 8)
        base = np.array([0, 0, 30, 0, 30, 12, 0, 12], np.float64).reshape(4, 2)
        polys = []
        for _ in range(NMS_N):
            ang = rng.uniform(-0.5, 0.5)
            c, s = math.cos(ang), math.sin(ang)
            p = base @ np.array([[c, s], [-s, c]]) + rng.uniform(0, 90, 2)
            p[rng.integers(0, 4)] += rng.uniform(-2, 2, 2)
            polys.append(p.reshape(8))
        _POLY_CACHE["polys"] = np.stack(polys).astype(np.float32)
        _POLY_CACHE["scores"] = (rng.uniform(0, 1, NMS_N) + np.arange(NMS_N) * 1e-6).astype(np.float32)
    return _POLY_CACHE


def _nms_poly_margin(thr):
    from oracle import poly_oracle as PO
    c = _nms_polys()
    if "iou" not in c:
        p64 = c["polys"].astype(np.float64)
        c["iou"] = PO.poly_iou_matrix(p64, p64, 0)
    return float(np.abs(c["iou"] - thr).min())


def _nms_poly(row_len, n_labels):
    rng = rng_of(NMS_N, row_len, n_labels)
    polys0, scores = _nms_polys()["polys"], _nms_polys()["scores"]
    thr = 0.25
    if row_len == 9:
        labels = rng.integers(0, 4, NMS_N)
        labels[labels == 2] = 3
        rows0 = np.concatenate([polys0, labels[:, None].astype(np.float32)], 1)
        order0 = _label_order(scores, labels) if n_labels > 1 else np.argsort(-scores, kind="stable").astype(np.int32)
    else:
        labels, rows0 = None, polys0
        order0 = np.argsort(-scores, kind="stable").astype(np.int32)

    def fn(run):
        rows, order = run.inp("polys", rows0), run.inp("order", order0, guard=0)
        keep = run.out("keep", (NMS_N,), U8)
        ws, wsb = run.ws("workspace", lib().jdet_nms_rotated_workspace(NMS_N))
        run.ok(lib().jdet_nms_poly(P(rows), NMS_N, row_len, P(order), thr, n_labels, P(keep), P(ws), wsb, ST(rows)),
               "jdet_nms_poly")

        def ref():
            from oracle import poly_oracle as PO
            p64 = polys0.astype(np.float64)
            assert _nms_poly_margin(thr) > 1e-4                                   # tests/test_gpu_poly.py:77
            k = np.zeros(NMS_N, np.uint8)
            k[PO.poly_nms(p64, scores, thr, labels=labels)] = 1
            return {"keep": exact(k)}
        return Res({"keep": keep}, ref)
    return fn


row("jdet_nms_poly", "n 130 row_len 8")(_nms_poly(8, 1))
row("jdet_nms_poly", "n 130 row_len 9 n_labels 1")(_nms_poly(9, 1))
row("jdet_nms_poly", "n 130 row_len 9 n_labels 4 (label 2 absent)")(_nms_poly(9, 4))


@row("jdet_box_iou_rotated", "3 x 67 stride 6")
def _box_iou(run):
    from tests import inputs as I
    rng = rng_of(3, 67)
    both = I.clustered_obbs(rng, 70, 3, 100.0)
    b1, b2 = both[:3], both[3:]
    t1, t2 = run.strided("boxes1", b1, 6), run.strided("boxes2", b2, 6)
    out = run.out("ious", (3, 67))
    run.ok(lib().jdet_box_iou_rotated(P(t1), 3, P(t2), 67, 6, 0, 0, P(out), ST(t1)), "jdet_box_iou_rotated")

    def ref():
        from oracle import oracle as O
        r = O.box_iou_rotated(b1, b2)                      # tests/test_gpu_iou_nms.py:53: bit-exact
        assert (r > 0).mean() > 0.05
        return {"ious": exact(r)}
    return Res({"ious": out}, ref)


@row("jdet_poly_iou", "5 x 67 strides 9 and 8")
def _poly_iou(run):
    rng = rng_of(5, 67, 9)

    def quads(n):
        c = rng.uniform(0, 50, (n, 1, 2))
        ang = np.sort(rng.uniform(0, 2 * math.pi, (n, 4)), 1)
        r = rng.uniform(6, 30, (n, 4))
        return (c + np.stack([r * np.cos(ang), r * np.sin(ang)], 2)).reshape(n, 8).astype(np.float32)
    a, b = quads(5), quads(67)
    ta, tb = run.strided("polys1", a, 9), run.inp("polys2", b)
    out = run.out("ious", (5, 67))
    run.ok(lib().jdet_poly_iou(P(ta), 5, 9, P(tb), 67, 8, 1, P(out), ST(ta)), "jdet_poly_iou")

    def ref():
        from oracle import poly_oracle as PO
        return {"ious": (PO.poly_iou_matrix(a.astype(np.float64), b.astype(np.float64), 1), 2e-5)}   # tests/test_gpu_poly.py:42
    return Res({"ious": out}, ref)


def _hbb_overlaps(with_alive):
    rng = rng_of(5, 257, with_alive)
    K, A = 5, 257
    c, wh = rng.uniform(0, 200, (K, 2)), rng.uniform(0, 80, (K, 2))
    gts0 = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    gts0[3, 2:] = gts0[3, :2]                                  # zero-area gt
    c, wh = rng.uniform(0, 200, (A, 2)), rng.uniform(0, 100, (A, 2))
    boxes0 = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    boxes0[:K] = gts0                                          # exact duplicates
    alive0 = (rng.uniform(size=A) > 0.3).astype(np.uint8)

    def fn(run):
        gts, boxes = run.inp("gts", gts0), run.strided("boxes", boxes0, 5)
        alive = run.inp("alive", alive0, guard=1) if with_alive else None
        out = run.out("overlaps", (K, A))
        run.ok(lib().jdet_bbox_overlaps_hbb(P(gts), K, P(boxes), A, 5, 0, 0, 1e-6, P(alive), P(out), ST(gts)),
               "jdet_bbox_overlaps_hbb")

        def ref():
            # the kernel's operations in its order in float32 (add, sub, mul, max, min and a correctly rounded divide,
            # contraction off): equality, as tests/test_gpu_boxes.py:369 demands against the tensor program
            f = np.float32
            g, b = gts0[:, None, :], boxes0[None, :, :]
            a1 = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
            a2 = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
            w = np.maximum(np.minimum(g[..., 2], b[..., 2]) - np.maximum(g[..., 0], b[..., 0]), f(0))
            h = np.maximum(np.minimum(g[..., 3], b[..., 3]) - np.maximum(g[..., 1], b[..., 1]), f(0))
            ov = w * h
            r = ov / np.maximum(a1 + a2 - ov, f(1e-6))
            assert r.dtype == np.float32
            if with_alive:
                r = np.where(alive0[None, :] != 0, r, f(-1))
            return {"overlaps": exact(r)}
        return Res({"overlaps": out}, ref)
    return fn


row("jdet_bbox_overlaps_hbb", "5 x 257 box_stride 5")(_hbb_overlaps(False))
row("jdet_bbox_overlaps_hbb", "5 x 257 box_stride 5 alive")(_hbb_overlaps(True))


@row("jdet_obb2hbb2obb", "n 257 stride 6")
def _obb2hbb2obb(run):
    from tests import inputs as I
    b0 = I.random_obbs(rng_of(257, 6), 257, extent=1024.0, wh=(8.0, 512.0))
    boxes, out = run.strided("boxes", b0, 6), run.out("out", (257, 5))
    run.ok(lib().jdet_obb2hbb2obb(P(boxes), 257, 6, P(out), ST(boxes)), "jdet_obb2hbb2obb")

    def ref():
        # tests/test_gpu_gaussian_losses.py:247-248: at most 1 ulp from the fp32 tensor program, angles equal
        from jdet_amd.ops.bbox_transforms import hbb2obb, obb2hbb
        r = hbb2obb(obb2hbb(torch.from_numpy(b0).to(run.dev))).cpu().numpy()
        ref, bound = ulps(r, 1)
        bound = bound.reshape(257, 5)
        bound[:, 4] = 0.0
        return {"out": (ref, bound)}
    return Res({"out": out}, ref)


ASSIGN_FLAGS = (       # tests/test_gpu_boxes.py:58-61
    dict(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.0),
    dict(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.3, match_low_quality=True, assigned_labels_filled=-1),
    dict(pos_iou_thr=0.7, neg_iou_thr=(0.1, 0.3), min_pos_iou=0.3, match_low_quality=False),
    dict(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.0, gt_max_assign_all=False),
)


def _assign(kw):
    K, A = 5, 257
    rng = rng_of(K, A)
    ov0 = np.round(rng.uniform(0, 1, (K, A)) ** 2, 2).astype(np.float32)      # two decimals: ties in rows and columns
    gl0 = rng.integers(1, 16, K).astype(np.int32)
    neg = kw["neg_iou_thr"]
    lo, hi = (0.0, neg) if isinstance(neg, float) else neg

    def fn(run):
        ov, gl = run.inp("overlaps", ov0), run.inp("gt_labels", gl0, guard=1)
        gi, mo, lab = run.out("gt_inds", (A,), I32), run.out("max_overlaps", (A,)), run.out("labels", (A,), I32)
        ws, wsb = run.ws("workspace", lib().jdet_assign_max_iou_workspace(K))
        run.ok(lib().jdet_assign_max_iou(P(ov), K, A, kw["pos_iou_thr"], lo, hi, kw["min_pos_iou"],
                                         int(kw.get("match_low_quality", True)), int(kw.get("gt_max_assign_all", True)),
                                         P(gl), kw.get("assigned_labels_filled", 0), P(gi), P(mo), P(lab), P(ws), wsb,
                                         ST(ov)), "jdet_assign_max_iou")

        def ref():
            from oracle import box_oracle as B
            g, m, l = B.assign_wrt_overlaps(ov0, kw["pos_iou_thr"], neg, kw["min_pos_iou"], kw.get("match_low_quality", True),
                                            kw.get("gt_max_assign_all", True), gl0, kw.get("assigned_labels_filled", 0))
            return {"gt_inds": exact(g), "max_overlaps": exact(m), "labels": exact(l)}    # tests/test_gpu_boxes.py:67-69
        return Res({"gt_inds": gi, "max_overlaps": mo, "labels": lab}, ref)
    return fn


for _k, _kw in enumerate(ASSIGN_FLAGS):
    row("jdet_assign_max_iou", "K 5 A 257 flag set %d, dirty workspace" % _k)(_assign(_kw))


# ---- sorted gathers on (1, 9, 11, C = 8) ---------------------------------------------------------------------------------
# Their per-pixel sums run in the order in which integer atomics handed out the entries' places (csr_gather.h), which
# differs from run to run: A and B are compared with the reference, like the float-atomic paths.
GATHER = (1, 9, 11, 8)


@row("jdet_deform_im2col_nhwc", "x(1,9,11,8) 3x3 pad 1")
def _im2col_nhwc(run):
    B, H, W, C = GATHER
    rng = rng_of(*GATHER, 1)
    x0, off0 = randn(rng, B, H, W, C), randn(rng, B, 18, H, W, scale=2.5)
    x, off = run.inp("x", x0), run.inp("offset", off0)
    cols = run.out("cols", (B * H * W, 9, C))
    run.ok(lib().jdet_deform_im2col_nhwc(P(x), P(off), B, C, H, W, 3, 3, 1, 1, 1, 1, 1, 1, P(cols), ST(x)),
           "jdet_deform_im2col_nhwc")
    return Res({"cols": cols}, lambda: {"cols": exact(deform_cols(x0, off0).astype(np.float32))})  # tests/test_gpu_dcn_arf.py:41


@row("jdet_deform_col2im_nhwc", "x(1,9,11,8) 3x3 pad 1, dirty workspace")
def _col2im_nhwc(run):
    B, H, W, C = GATHER
    rng = rng_of(*GATHER, 2)
    gc0, off0 = randn(rng, B * H * W, 9, C), randn(rng, B, 18, H, W, scale=2.5)
    gc, off = run.inp("grad_cols", gc0), run.inp("offset", off0)
    gx = run.out("grad_x", (B, H, W, C))
    ws, wsb = run.ws("workspace", lib().jdet_deform_col2im_nhwc_workspace(B, C, H, W, 3, 3, 1, 1, 1, 1, 1, 1))
    run.ok(lib().jdet_deform_col2im_nhwc(P(gc), P(off), B, C, H, W, 3, 3, 1, 1, 1, 1, 1, 1, P(gx), P(ws), wsb, ST(gc)),
           "jdet_deform_col2im_nhwc")

    def ref():
        from oracle import oracle as O
        col = gc0.reshape(B, H, W, 9, C).transpose(4, 3, 0, 1, 2).reshape(C * 9, B, H, W)
        g = O.deform_col2im(col, off0, (B, C, H, W), 3, 3, (1, 1), (1, 1), (1, 1), 1)
        return {"grad_x": (g.transpose(0, 2, 3, 1).astype(np.float64), 2e-5)}          # tests/test_gpu_dcn_arf.py:44
    return Res({"grad_x": gx}, ref, atomic=True)


def _fr_boxes(rng, N, H, W, stride):
    """tests/test_gpu_fr.py:12-20"""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    b = np.stack([ys * stride + rng.normal(0, 2.0 * stride, (N, H, W)), xs * stride + rng.normal(0, 2.0 * stride, (N, H, W)),
                  np.exp(rng.normal(np.log(4 * stride), 0.6, (N, H, W))),
                  np.exp(rng.normal(np.log(4 * stride), 0.6, (N, H, W))), rng.uniform(-1.6, 1.6, (N, H, W))], -1)
    b[0, 0, 0, :2] = -1000.0
    b[0, 0, 1, :2] = (H + 0.5) * stride
    return b.astype(np.float32)


def _feature_refine(points, backward):
    N, H, W, C = GATHER
    rng = rng_of(*GATHER, points, backward)
    feat0, boxes0 = randn(rng, N, H, W, C), _fr_boxes(rng, N, H, W, 8.0)

    def fn(run):
        from oracle import fr_oracle as FO
        x, boxes = run.inp("grad_out" if backward else "feat", feat0), run.inp("boxes", boxes0)
        out = run.out("grad_in" if backward else "out", (N, H, W, C))
        if backward:
            ws, wsb = run.ws("workspace", lib().jdet_feature_refine_backward_workspace(N, C, H, W, points))
            rc = lib().jdet_feature_refine_backward(P(x), P(boxes), N, C, H, W, 0.125, points, P(out), P(ws), wsb, ST(x))
        else:
            rc = lib().jdet_feature_refine_forward(P(x), P(boxes), N, C, H, W, 0.125, points, P(out), ST(x))
        run.ok(rc, "jdet_feature_refine")

        def ref():
            nchw = feat0.transpose(0, 3, 1, 2)
            f = FO.feature_refine_backward if backward else FO.feature_refine_forward
            r = np.asarray(f(nchw, boxes0, 0.125, points), np.float64).transpose(0, 2, 3, 1)
            # tests/test_gpu_fr.py:39 (forward) and :42 (backward)
            return {"grad_in" if backward else "out": (r, (3e-5 if backward else 2e-5) * max(1.0, float(np.abs(r).max())))}
        return Res({"grad_in" if backward else "out": out}, ref, atomic=backward)
    return fn


for _pts in (1, 5):
    row("jdet_feature_refine_forward", "x(1,9,11,8) points %d" % _pts)(_feature_refine(_pts, False))
    row("jdet_feature_refine_backward", "x(1,9,11,8) points %d, dirty workspace" % _pts)(_feature_refine(_pts, True))


# ---- the loss calls --------------------------------------------------------------------------------------------------------
FOCAL_LOSS = (2e-5, 1e-6)    # tests/test_gpu_boxes.py:200   (rtol, atol)
FOCAL_GRAD = (2e-4, 1e-7)    # tests/test_gpu_boxes.py:203
SL1_LOSS = (2e-5, 1e-6)      # tests/test_gpu_boxes.py:244
SL1_GRAD = (1e-5, 1e-7)      # tests/test_gpu_boxes.py:247
LOSS_SIZES = ((37, 1), (1000, 15))


def focal64(x, labels, w, alpha, gamma):
    """models/losses/focal_loss.py:L15-49 in float64, element by element: ce = BCE-with-logits against the one-hot of
    `label == class + 1` (the max_val form equals softplus; its 1e-10 floor is never reached), p_t = the probability
    of the true outcome, loss = alpha_t * w * ce * (1 - p_t)^gamma; with s = +1 on the true class and -1 elsewhere,
    p_t = sigmoid(s x), 1 - p_t = sigmoid(-s x), ce = softplus(-s x), and
    d loss / d x = alpha_t * w * (-s) * ((1 - p_t)^(gamma + 1) + gamma * (1 - p_t)^gamma * p_t * ce)."""
    x = np.asarray(x, np.float64)
    M, C = x.shape
    t = np.asarray(labels)[:, None] == np.arange(1, C + 1)[None, :]
    s = np.where(t, 1.0, -1.0)
    z = s * x
    ce = np.logaddexp(0.0, -z)
    pt = np.exp(-np.logaddexp(0.0, -z))
    q = np.exp(-np.logaddexp(0.0, z))
    at = np.where(t, alpha, 1 - alpha) if alpha >= 0 else np.ones_like(x)
    ww = (np.ones(M) if w is None else np.asarray(w, np.float64))[:, None]
    mod = np.power(q, gamma)
    return float((at * ww * ce * mod).sum()), at * ww * (-s) * (mod * q + gamma * mod * pt * ce)


def smooth_l1_64(pred, target, w, beta):
    """models/losses/smooth_l1_loss.py:L5-27 (beta = 0: l1_loss.py) in float64 and its derivative"""
    d = np.asarray(pred, np.float64) - np.asarray(target, np.float64)
    ad = np.abs(d)
    ww = 1.0 if w is None else np.asarray(w, np.float64)
    if beta == 0:
        return float((ad * ww).sum()), np.sign(d) * ww
    small = ad < beta
    return (float((np.where(small, 0.5 * d * d / beta, ad - 0.5 * beta) * ww).sum()),
            np.where(small, d / beta, np.sign(d)) * ww)


def _focal_inputs(M, C, seed):
    rng = rng_of(M, C, seed)
    x0 = randn(rng, M, C, scale=3.0)
    x0[0, 0], x0[1, 0] = 40.0, -40.0                         # saturated logits ...
    lab0 = rng.integers(0, C + 1, M).astype(np.int32)
    lab0[0], lab0[1], lab0[2], lab0[3] = 1, 1, 0, 0         # ... on the true class and off it
    x0[2, 0], x0[3, 0] = 40.0, -40.0
    w0 = (rng.uniform(0, 1, M) > 0.2).astype(np.float32)
    w0[:4] = 1.0
    return x0, lab0, w0


def _focal(M, C, alpha, gamma):
    x0, lab0, w0 = _focal_inputs(M, C, 1)

    def fn(run):
        x, lab, w = run.inp("logits", x0), run.inp("labels", lab0, guard=0), run.inp("weight", w0)
        loss, grad = run.out("loss_sum", (1,)), run.out("grad_logits", (M, C))
        ws, wsb = run.ws("workspace", lib().jdet_sigmoid_focal_loss_workspace())
        run.ok(lib().jdet_sigmoid_focal_loss(P(x), P(lab), P(w), M, C, alpha, gamma, P(loss), P(grad), P(ws), wsb, ST(x)),
               "jdet_sigmoid_focal_loss")

        def ref():
            l, g = focal64(x0, lab0, w0, alpha, gamma)
            return {"loss_sum": close(np.asarray([l]), *FOCAL_LOSS), "grad_logits": close(g, *FOCAL_GRAD)}
        return Res({"loss_sum": loss, "grad_logits": grad}, ref)
    return fn


for _m, _c in LOSS_SIZES:
    for _gamma in (0.0, 1.5, 2.0):
        for _alpha in (0.25, -1.0):
            row("jdet_sigmoid_focal_loss", "%d x %d gamma %g alpha %g, dirty workspace" % (_m, _c, _gamma, _alpha))(
                _focal(_m, _c, _alpha, _gamma))


def _sl1_inputs(n, seed):
    rng = rng_of(n, seed)
    p0, t0 = randn(rng, n), randn(rng, n, scale=0.5)
    p0[0] = t0[0]                                            # zero difference: sign(0) = 0
    w0 = (rng.uniform(0, 1, n) > 0.3).astype(np.float32) * rng.uniform(0.5, 2, n).astype(np.float32)
    return p0, t0, w0


def _smooth_l1(M, C, beta):
    n = M * C
    p0, t0, w0 = _sl1_inputs(n, 2)

    def fn(run):
        p, t, w = run.inp("pred", p0), run.inp("target", t0), run.inp("weight", w0)
        loss, grad = run.out("loss_sum", (1,)), run.out("grad_pred", (n,))
        ws, wsb = run.ws("workspace", lib().jdet_sigmoid_focal_loss_workspace())
        run.ok(lib().jdet_smooth_l1_loss(P(p), P(t), P(w), n, beta, P(loss), P(grad), P(ws), wsb, ST(p)),
               "jdet_smooth_l1_loss")

        def ref():
            l, g = smooth_l1_64(p0, t0, w0, np.float32(beta).astype(np.float64))
            return {"loss_sum": close(np.asarray([l]), *SL1_LOSS), "grad_pred": close(g, *SL1_GRAD)}
        return Res({"loss_sum": loss, "grad_pred": grad}, ref)
    return fn


for _m, _c in LOSS_SIZES:
    for _beta in (0.0, 1.0 / 9.0, 1.0):
        row("jdet_smooth_l1_loss", "%d x %d beta %.3g, dirty workspace" % (_m, _c, _beta))(_smooth_l1(_m, _c, _beta))


# the blocked row index of the *_loss_level calls: an (N = 3, A = 700) array, window [300:650]
LV_N, LV_A, LV_S, LV_E = 3, 700, 300, 650
LV_M = LV_N * (LV_E - LV_S)


def windowed(run, name, inside, cols, poison, guard=None):
    """the rows `inside` (N, e - s[, cols]) as the window [s:e] of an (N, A[, cols]) array; every row outside the window
    holds `poison` in the hostile runs (NaN weights / targets, a valid but different label), 0 in run A.  Returns the
    array and the address of the window's first row."""
    shape = (LV_N, LV_A) + ((cols,) if cols else ())
    full = np.full(shape, poison if run.hostile else 0, inside.dtype)
    full[:, LV_S:LV_E] = inside
    t = run.inp(name, full, guard=guard)
    return t, t.data_ptr() + LV_S * max(cols, 1) * t.element_size()


def _focal_level(alpha, gamma):
    C = 15
    x0, lab0, w0 = _focal_inputs(LV_M, C, 3)
    avg0, lw = np.asarray([37.0], np.float32), 0.7

    def fn(run):
        x = run.inp("logits", x0)
        _, lab_p = windowed(run, "labels", lab0.reshape(LV_N, -1), 0, 7, guard=0)
        _, w_p = windowed(run, "weight", w0.reshape(LV_N, -1), 0, np.nan)
        avg = run.inp("avg_factor", avg0)
        loss, grad = run.out("loss", (1,)), run.out("grad_logits", (LV_M, C))
        ws, wsb = run.ws("workspace", lib().jdet_sigmoid_focal_loss_workspace())
        rpb = LV_E - LV_S
        run.ok(lib().jdet_sigmoid_focal_loss_level(P(x), lab_p, rpb, LV_A, w_p, rpb, LV_A, LV_M, C, alpha, gamma, P(avg), lw,
                                                   P(loss), P(grad), P(ws), wsb, ST(x)), "jdet_sigmoid_focal_loss_level")

        def ref():
            l, g = focal64(x0, lab0, w0, alpha, gamma)
            return {"loss": close(np.asarray([l / 37.0 * np.float64(np.float32(lw))]), *FOCAL_LOSS),
                    "grad_logits": close(g, *FOCAL_GRAD)}
        return Res({"loss": loss, "grad_logits": grad}, ref)
    return fn


row("jdet_sigmoid_focal_loss_level", "(3,700) window [300:650] x 15 gamma 2 alpha 0.25")(_focal_level(0.25, 2.0))
row("jdet_sigmoid_focal_loss_level", "(3,700) window [300:650] x 15 gamma 1.5 alpha -1")(_focal_level(-1.0, 1.5))


def _sl1_level(beta):
    E = 5
    p0, t0, w0 = _sl1_inputs(LV_M * E, 4)
    avg0, lw = np.asarray([23.0], np.float32), 1.3

    def fn(run):
        p = run.inp("pred", p0.reshape(LV_M, E))
        _, t_p = windowed(run, "target", t0.reshape(LV_N, -1, E), E, np.nan)
        _, w_p = windowed(run, "weight", w0.reshape(LV_N, -1, E), E, np.nan)
        avg = run.inp("avg_factor", avg0)
        loss, grad = run.out("loss", (1,)), run.out("grad_pred", (LV_M, E))
        ws, wsb = run.ws("workspace", lib().jdet_sigmoid_focal_loss_workspace())
        rpb = LV_E - LV_S
        run.ok(lib().jdet_smooth_l1_loss_level(P(p), t_p, rpb, LV_A, w_p, rpb, LV_A, LV_M, E, beta, P(avg), lw, P(loss),
                                               P(grad), P(ws), wsb, ST(p)), "jdet_smooth_l1_loss_level")

        def ref():
            l, g = smooth_l1_64(p0, t0, w0, np.float32(beta).astype(np.float64))
            return {"loss": close(np.asarray([l / 23.0 * np.float64(np.float32(lw))]), *SL1_LOSS),
                    "grad_pred": close(g, *SL1_GRAD)}
        return Res({"loss": loss, "grad_pred": grad}, ref)
    return fn


for _beta in (0.0, 1.0 / 9.0):
    row("jdet_smooth_l1_loss_level", "(3,700,5) window [300:650] beta %.3g" % _beta)(_sl1_level(_beta))


@row("jdet_gaussian_loss_level", "GWD log1p, decoded prediction, (3,700,5) window [300:650]")
def _gaussian_level(run):
    from jdet_amd.models.losses.gaussian_dist_loss import level_params
    rng = rng_of(LV_M, 5, 8)
    A_l = LV_E - LV_S
    anchors0 = np.concatenate([rng.uniform(0, 1024, (A_l, 2)), np.exp(rng.uniform(np.log(16), np.log(512), (A_l, 2))),
                               rng.uniform(-math.pi / 4, 3 * math.pi / 4, (A_l, 1))], 1).astype(np.float32)
    deltas0 = randn(rng, LV_M, 5, scale=0.3)
    all_anc = np.tile(anchors0, (LV_N, 1))
    target0 = np.concatenate([all_anc[:, :2] + randn(rng, LV_M, 2, scale=8.0),
                              all_anc[:, 2:4] * np.exp(randn(rng, LV_M, 2, scale=0.3)),
                              all_anc[:, 4:] + randn(rng, LV_M, 1, scale=0.3)], 1).astype(np.float32)
    weight0 = np.zeros((LV_M, 5), np.float32)
    weight0[rng.uniform(size=LV_M) < 0.2] = 1.0
    avg0, lw = np.asarray([float((weight0.mean(-1) > 0).sum()) + 3.0], np.float32), 5.0
    pred = run.inp("pred", deltas0)
    _, t_p = windowed(run, "target", target0.reshape(LV_N, A_l, 5), 5, np.nan)
    _, w_p = windowed(run, "weight", weight0.reshape(LV_N, A_l, 5), 5, np.nan)
    anc, avg = run.inp("anchors", anchors0), run.inp("avg_factor", avg0)
    loss, grad = run.out("loss", (1,)), run.out("grad_pred", (LV_M, 5))
    ws, wsb = run.ws("workspace", lib().jdet_sigmoid_focal_loss_workspace())
    params = level_params("gwd", "log1p", decode_pred=True, tau=0.0)
    run.ok(lib().jdet_gaussian_loss_level(P(pred), t_p, A_l, LV_A, w_p, A_l, LV_A, P(anc), A_l, LV_M, ctypes.byref(params),
                                          P(avg), lw, P(loss), P(grad), P(ws), wsb, ST(pred)), "jdet_gaussian_loss_level")

    def ref():
        from tests import gaussian_loss_ref as R
        want, g = R.masked_loss_and_grad("gwd", deltas0, target0, weight0, float(avg0[0]), lw, anchors=all_anc,
                                         decode_pred=True, fun="log1p", tau=0.0)
        unit = g * float(avg0[0]) / lw                       # the kernel stores d sum / d pred, the unit gradient
        # tests/test_gpu_gaussian_losses.py:23 (gwd: loss 1e-5 relative, gradient 1e-4 of its scale)
        return {"loss": (np.asarray([want]), 1e-5 * abs(want)), "grad_pred": rel(unit, 1e-4)}
    return Res({"loss": loss, "grad_pred": grad}, ref)


def _grad_scale(n):
    rng = rng_of(n, 12)
    u0, go0, avg0, lw = randn(rng, n), np.asarray([0.625], np.float32), np.asarray([37.0], np.float32), 0.7

    def fn(run):
        u, go, avg = run.inp("unit_grad", u0), run.inp("grad_out", go0), run.inp("avg_factor", avg0)
        out = run.out("out", (n,))
        run.ok(lib().jdet_loss_grad_scale(P(u), n, P(go), P(avg), lw, P(out), ST(u)), "jdet_loss_grad_scale")
        # unit * ((grad_out * loss_weight) / avg_factor): three correctly rounded fp32 operations in this order (contraction
        # off) -- equality, as tests/test_gpu_boxes.py:285-286 demands of the level nodes against the composition
        return Res({"out": out}, lambda: {"out": exact(u0 * ((go0[0] * np.float32(lw)) / avg0[0]))})
    return fn


def _sum_squares(n, take_sqrt):
    x0 = randn(rng_of(n, 13), n)

    def fn(run):
        x, out = run.inp("x", x0), run.out("out", (1,))
        ws, wsb = run.ws("workspace", lib().jdet_sum_squares_workspace())
        run.ok(lib().jdet_sum_squares(P(x), n, take_sqrt, P(out), P(ws), wsb, ST(x)), "jdet_sum_squares")

        def ref():
            r = float((x0.astype(np.float64) ** 2).sum())
            r = math.sqrt(r) if take_sqrt else r
            return {"out": (np.asarray([r]), 1e-6 * max(1.0, r))}            # tests/test_gpu_graph_safe.py:20
        return Res({"out": out}, ref)
    return fn


for _m, _c in LOSS_SIZES:
    row("jdet_loss_grad_scale", "n %d" % (_m * _c))(_grad_scale(_m * _c))
    row("jdet_sum_squares", "n %d sqrt, dirty workspace" % (_m * _c))(_sum_squares(_m * _c, 1))
row("jdet_sum_squares", "n 15000 no sqrt, dirty workspace")(_sum_squares(15000, 0))


# ======================================================================================================================
# one row each
# ======================================================================================================================
def c5(v):
    return L.vec5(v)


@row("jdet_level_pack_nhwc", "sizes [(5,9),(3,4),(2,2),(1,1)] C 4, level 1 NULL")
def _level_pack(run):
    from jdet_amd.models.utils.level_pack import LevelPack
    sizes, N, C = [(5, 9), (3, 4), (2, 2), (1, 1)], 2, 4
    places = LevelPack._place(sizes)
    Hp = max(r + h for (r, _), (h, _) in zip(places, sizes))
    Wp = max(c + w for (_, c), (_, w) in zip(places, sizes))
    rng = rng_of(5, 9, 4)
    lv0 = [randn(rng, N, h, w, C) for h, w in sizes]
    lv = [None if k == 1 else run.inp("level%d" % k, a) for k, a in enumerate(lv0)]
    canvas = run.out("canvas", (N, Hp, Wp, C))
    ptrs = (ctypes.c_void_p * 4)(*[P(t) for t in lv])
    hw = (ctypes.c_int32 * 8)(*[v for s in sizes for v in s])
    place = (ctypes.c_int32 * 8)(*[v for s in places for v in s])
    run.ok(lib().jdet_level_pack_nhwc(ptrs, hw, place, 4, N, C, Hp, Wp, P(canvas), ST(canvas)), "jdet_level_pack_nhwc")

    def ref():
        r = np.zeros((N, Hp, Wp, C), np.float32)
        for k, ((h, w), (r0, c0)) in enumerate(zip(sizes, places)):
            if k != 1:
                r[:, r0:r0 + h, c0:c0 + w] = lv0[k]
        return {"canvas": exact(r)}                                   # copies: tests/test_gpu_level_pack.py:40
    return Res({"canvas": canvas}, ref)


def _nearest(dst, n_in, n_out):
    """csrc/upsample_add.hip nearest_src: min(floor(dst * (in / out)), in - 1) in float32"""
    s = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(dst, dtype=np.float32) * s).astype(np.int64), n_in - 1)


UPS = (2, 8, 17, 9, 5, 4, 2.0)       # tests/test_gpu_fpn.py:13: N, C, H, W, Ht, Wt, div


@row("jdet_upsample_add_nhwc_forward", "17 x 9 from 5 x 4, C 8, div 2")
def _upsample_fwd(run):
    N, C, H, W, Ht, Wt, div = UPS
    rng = rng_of(*UPS)
    lat0, top0 = randn(rng, N, H, W, C), randn(rng, N, Ht, Wt, C)
    lat, top, out = run.inp("lateral", lat0), run.inp("top", top0), run.out("out", (N, H, W, C))
    run.ok(lib().jdet_upsample_add_nhwc_forward(P(lat), P(top), N, C, H, W, Ht, Wt, div, P(out), ST(lat)), "upsample_add")
    # one add and one multiply by 1 / 2 per element: same bits (tests/test_gpu_fpn.py:29)
    return Res({"out": out}, lambda: {"out": exact((lat0 + top0[:, _nearest(H, Ht, H)][:, :, _nearest(W, Wt, W)]) *
                                                   np.float32(0.5))})


@row("jdet_upsample_add_nhwc_backward", "17 x 9 onto 5 x 4, C 8, div 2")
def _upsample_bwd(run):
    N, C, H, W, Ht, Wt, div = UPS
    go0 = randn(rng_of(*UPS, 1), N, H, W, C)
    go, gt = run.inp("grad_out", go0), run.out("grad_top", (N, Ht, Wt, C))
    run.ok(lib().jdet_upsample_add_nhwc_backward(P(go), N, C, H, W, Ht, Wt, div, P(gt), ST(go)), "upsample_add_backward")

    def ref():
        r = np.zeros((N, Ht, Wt, C))
        ys, xs = _nearest(H, Ht, H), _nearest(W, Wt, W)
        for y in range(H):
            for x in range(W):
                r[:, ys[y], xs[x]] += go0[:, y, x]
        return {"grad_top": close(r / div, 1e-6, 1e-6)}                # tests/test_gpu_fpn.py:31
    return Res({"grad_top": gt}, ref)


@row("jdet_normalize_u8_nhwc", "N 2, 5 x 7 (210 bytes), valid_hw inside the canvas, swap_rb")
def _normalize(run):
    N, Hs, Ws = 2, 5, 7
    rng = rng_of(N, Hs, Ws)
    src0 = rng.integers(0, 256, (N, Hs, Ws, 3)).astype(np.uint8)
    valid0 = np.asarray([[4, 7], [5, 3]], np.int32)
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
    src, valid = run.inp("src", src0, guard=1), run.inp("valid_hw", valid0, guard=0)
    dst = run.out("dst", (N, Hs, Ws, 3))
    run.ok(lib().jdet_normalize_u8_nhwc(P(src), P(valid), N, Hs, Ws, L.vecn(mean, 3), L.vecn(std, 3), 1, P(dst), ST(src)),
           "jdet_normalize_u8_nhwc")

    def ref():
        # (v - mean[c]) / std[c] in float32 after the channel reversal, zeros outside valid_hw: "bit-identical to the host
        # arithmetic" (include/jdet_hip.h), one subtraction and one correctly rounded division
        v = src0[..., ::-1].astype(np.float32)
        r = (v - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
        for n in range(N):
            r[n, valid0[n, 0]:] = 0
            r[n, :, valid0[n, 1]:] = 0
        return {"dst": exact(r.astype(np.float32))}
    return Res({"dst": dst}, ref)


@row("jdet_align_conv_offset", "N 2, 9 x 13, stride 16, k 3")
def _align_offset(run):
    N, H, W, stride = 2, 9, 13, 16.0
    rng = rng_of(N, H, W, 16)
    anc0 = np.concatenate([rng.uniform(0, 200, (N, H * W, 2)), np.exp(rng.uniform(np.log(8), np.log(200), (N, H * W, 2))),
                           rng.uniform(-1.6, 1.6, (N, H * W, 1))], -1).astype(np.float32)     # tests/test_gpu_boxes.py:212
    anc, off = run.inp("anchors", anc0), run.out("offset", (N, 18, H, W))
    run.ok(lib().jdet_align_conv_offset(P(anc), N, H, W, stride, 3, P(off), ST(anc)), "jdet_align_conv_offset")

    def ref():
        from oracle import box_oracle as B
        r = np.stack([B.align_conv_offsets(anc0[n], (H, W), stride) for n in range(N)])
        return {"offset": close(r, 1e-5, 2e-5)}                        # tests/test_gpu_boxes.py:218
    return Res({"offset": off}, ref)


ARF = (3, 2, 8, 3, 3, 8)             # nOut, nIn, nOri, kH, kW, nRot


def _arf(backward, cl):
    nOut, nIn, nOri, kH, kW, nRot = ARF
    from tests import inputs as I
    idx0 = I.arf_indices(nOri, nRot, kH)
    rng = rng_of(*ARF, backward, cl)
    w0 = randn(rng, nOut, nIn, nOri, kH, kW)
    g0 = randn(rng, nOut * nRot, nIn * nOri, kH, kW)                   # the bank's gradient, logical (O, I, kH, kW)

    def fn(run):
        idx = run.inp("indices", idx0, guard=1)                        # 1-based table: 1 is in range
        if backward:
            g = run.inp("grad_out", g0.transpose(0, 2, 3, 1) if cl else g0)
            out = run.out("grad_weight", w0.shape)
            f = lib().jdet_arf_backward_cl if cl else lib().jdet_arf_backward
            rc = f(P(idx), P(g), nOut, nIn, nOri, kH, kW, nRot, P(out), ST(g))
        else:
            w = run.inp("weight", w0)
            out = run.out("out", (nOut * nRot, kH, kW, nIn * nOri) if cl else (nOut * nRot, nIn * nOri, kH, kW))
            f = lib().jdet_arf_forward_cl if cl else lib().jdet_arf_forward
            rc = f(P(w), P(idx), nOut, nIn, nOri, kH, kW, nRot, P(out), ST(w))
        run.ok(rc, "jdet_arf")

        def ref():
            from oracle import oracle as O
            if backward:                                               # tests/test_gpu_dcn_arf.py:118, :214
                return {"grad_weight": exact(O.arf_backward(idx0, g0))}
            r = O.arf_forward(w0, idx0)                                # tests/test_gpu_dcn_arf.py:117, :210
            return {"out": exact(r.transpose(0, 2, 3, 1) if cl else r)}
        return Res({"grad_weight" if backward else "out": out}, ref)
    return fn


row("jdet_arf_forward", "nOut 3 nIn 2 nOri 8 3x3 nRot 8")(_arf(False, False))
row("jdet_arf_backward", "nOut 3 nIn 2 nOri 8 3x3 nRot 8")(_arf(True, False))
row("jdet_arf_forward_cl", "nOut 3 nIn 2 nOri 8 3x3 nRot 8")(_arf(False, True))
row("jdet_arf_backward_cl", "nOut 3 nIn 2 nOri 8 3x3 nRot 8")(_arf(True, True))


def _rip(backward, nO):
    P_, C = 117, 8 * nO
    rng = rng_of(P_, C, nO, backward)
    x0 = randn(rng, P_, C)
    x0[::2] = np.round(x0[::2] * 2) / 2                                # ties (tests/test_gpu_dcn_arf.py:186)
    y0 = x0.reshape(P_, C // nO, nO).max(2)
    gy0 = randn(rng, P_, C // nO)

    def fn(run):
        x = run.inp("x", x0)
        if backward:
            y, gy = run.inp("y", y0), run.inp("grad_y", gy0)
            out = run.out("grad_x", (P_, C))
            rc = lib().jdet_rip_backward(P(x), P(y), P(gy), P_, C, nO, P(out), ST(x))
        else:
            out = run.out("y", (P_, C // nO))
            rc = lib().jdet_rip_forward(P(x), P_, C, nO, P(out), ST(x))
        run.ok(rc, "jdet_rip")

        def ref():
            if not backward:
                return {"y": exact(y0)}                                # tests/test_gpu_dcn_arf.py:191
            hit = x0.reshape(P_, C // nO, nO) == y0[..., None]
            g = hit * (gy0.astype(np.float64) / hit.sum(2))[..., None]
            return {"grad_x": (g.reshape(P_, C), 1e-7)}                # tests/test_gpu_dcn_arf.py:195
        return Res({"grad_x" if backward else "y": out}, ref)
    return fn


for _no in (4, 8):
    row("jdet_rip_forward", "(117,%d) nO %d" % (8 * _no, _no))(_rip(False, _no))
    row("jdet_rip_backward", "(117,%d) nO %d, ties" % (8 * _no, _no))(_rip(True, _no))


def _layout(to_nhwc):
    N, C, H, W = 3, 37, 19, 23                                         # tests/test_gpu_roi_align.py:288
    x0 = randn(rng_of(N, C, H, W, to_nhwc), *((N, C, H, W) if to_nhwc else (N, H, W, C)))

    def fn(run):
        x = run.inp("x", x0)
        y = run.out("y", (N, H, W, C) if to_nhwc else (N, C, H, W))
        f = lib().jdet_nchw_to_nhwc if to_nhwc else lib().jdet_nhwc_to_nchw
        run.ok(f(P(x), N, C, H, W, P(y), ST(x)), "layout")
        return Res({"y": y}, lambda: {"y": exact(x0.transpose(0, 2, 3, 1) if to_nhwc else x0.transpose(0, 3, 1, 2))})
    return fn


row("jdet_nchw_to_nhwc", "(3,37,19,23)")(_layout(True))
row("jdet_nhwc_to_nchw", "(3,37,19,23)")(_layout(False))


# ---- box codecs ----------------------------------------------------------------------------------------------------------
def wrapped(ref, cols, rtol, atol, angle_tol, period, stride=5, angle_col=4, skip_rows=None):
    """error measure of a decoded box table (rows of `stride` columns per class): position / size columns against
    atol + rtol * |ref|, the angle column against angle_tol modulo the wrap `period` of its range (the existing tests'
    rule).  Returns (error function, bound array)."""
    ref = np.asarray(ref, np.float64)
    flat = ref.reshape(-1, stride)
    bound = atol + rtol * np.abs(flat)
    bound[:, angle_col] = angle_tol

    def err(v):
        d = np.abs(np.asarray(v, np.float64).reshape(-1, stride) - flat)
        a = d[:, angle_col]
        d[:, angle_col] = np.minimum(a, np.abs(a - period))
        if skip_rows is not None:
            d.reshape(ref.shape[0], -1)[skip_rows] = 0.0
        return d
    return err, bound.reshape(-1)


CODEC_MEANS, CODEC_STDS = (0.1, -0.2, 0.3, 0.0, 0.05), (0.1, 0.2, 0.2, 0.1, 0.5)     # tests/test_gpu_boxes.py:25


@row("jdet_delta2bbox_rotated", "n 7 ncls 15")
def _delta2bbox(run):
    from tests import inputs as I
    rng = rng_of(7, 15)
    rois0, d0 = I.random_obbs(rng, 7), randn(rng, 7, 75, scale=0.5)
    rois, d, out = run.inp("rois", rois0), run.inp("deltas", d0), run.out("out", (7, 75))
    run.ok(lib().jdet_delta2bbox_rotated(P(rois), P(d), 7, 15, c5(CODEC_MEANS), c5(CODEC_STDS), 16 / 1000, P(out), ST(d)),
           "jdet_delta2bbox_rotated")

    def ref():
        from oracle import box_oracle as B
        # tests/test_gpu_boxes.py:33-35: rtol 3e-5 atol 2e-3 on x y w h, angles 1e-4 modulo pi
        return {"out": wrapped(B.delta2bbox_rotated(rois0, d0, CODEC_MEANS, CODEC_STDS, 16 / 1000), 75, 3e-5, 2e-3, 1e-4, math.pi)}
    return Res({"out": out}, ref)


@row("jdet_bbox2delta_rotated", "n 257")
def _bbox2delta(run):
    from tests import inputs as I
    rng = rng_of(257, 5)
    p0, g0 = I.random_obbs(rng, 257), I.random_obbs(rng, 257)
    p, g, out = run.inp("proposals", p0), run.inp("gt", g0), run.out("out", (257, 5))
    run.ok(lib().jdet_bbox2delta_rotated(P(p), P(g), 257, c5(CODEC_MEANS), c5(CODEC_STDS), P(out), ST(p)),
           "jdet_bbox2delta_rotated")

    def ref():
        from oracle import box_oracle as B
        return {"out": close(B.bbox2delta_rotated(p0, g0, CODEC_MEANS, CODEC_STDS), 2e-5, 2e-5)}   # tests/test_gpu_boxes.py:28
    return Res({"out": out}, ref)


def _obbs(n, seed, regular=True):
    """tests/test_gpu_boxes.py:295-302"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(50, 950, (n, 2))
    wh = np.exp(rng.uniform(np.log(8), np.log(300), (n, 2)))
    if regular:
        wh = np.stack([wh.max(1), wh.min(1)], 1)
    th = rng.uniform(-math.pi / 2, math.pi / 2, (n, 1)) if regular else rng.uniform(-4, 4, (n, 1))
    return np.concatenate([c, wh, th], 1).astype(np.float32)


ORI_N = 257
M6, S6 = [0.] * 6, [1., 1., 1., 1., .5, .5]
M5, S5 = [0.] * 5, [0.1, 0.1, 0.2, 0.2, 0.1]


def _sin_err(ref):
    """position / size against rtol 1e-4 atol 5e-3, |sin(angle difference)| < 2e-4 (tests/test_gpu_boxes.py:322-323, :339-340)"""
    ref = np.asarray(ref, np.float64).reshape(-1, 5)
    bound = 5e-3 + 1e-4 * np.abs(ref)
    bound[:, 4] = 2e-4

    def err(v):
        d = np.abs(np.asarray(v, np.float64).reshape(-1, 5) - ref)
        d[:, 4] = np.abs(np.sin(d[:, 4]))
        return d
    return err, bound.reshape(-1)


def _oriented(which):
    from oracle import box_oracle as BO
    g0 = _obbs(ORI_N, 1)
    anchors0 = (BO.obb2hbb(g0) + np.random.default_rng(2).uniform(-3, 3, (ORI_N, 4))).astype(np.float32)   # every anchor keeps a positive size
    p0 = _obbs(ORI_N, 4, regular=False)
    d6 = np.random.default_rng(3).normal(0, 0.5, (ORI_N, 6)).astype(np.float32)
    d15 = np.random.default_rng(5).normal(0, 1, (ORI_N, 15)).astype(np.float32)

    def fn(run):
        n = ORI_N
        if which == "mid_decode":
            a, d, out = run.inp("anchors", anchors0), run.inp("deltas", d6), run.out("out", (n, 5))
            rc = lib().jdet_midpoint_offset_decode(P(a), P(d), n, L.vecn(M6, 6), L.vecn(S6, 6), 16 / 1000, P(out), ST(a))
            ref = lambda: {"out": _sin_err(BO.midpoint_offset_decode(anchors0, d6, M6, S6))}
        elif which == "mid_encode":
            a, g, out = run.inp("anchors", anchors0), run.inp("gt", g0), run.out("out", (n, 6))
            rc = lib().jdet_midpoint_offset_encode(P(a), P(g), n, L.vecn(M6, 6), L.vecn(S6, 6), P(out), ST(a))
            ref = lambda: {"out": close(BO.midpoint_offset_encode(anchors0, g0, M6, S6), 2e-5, 2e-5)}   # tests/test_gpu_boxes.py:317
        elif which == "ori_decode":
            r, d, out = run.inp("rois", p0), run.inp("deltas", d15), run.out("out", (n, 15))
            rc = lib().jdet_oriented_delta_decode(P(r), P(d), n, 3, c5(M5), c5(S5), 16 / 1000, P(out), ST(r))
            ref = lambda: {"out": _sin_err(BO.oriented_delta_decode(p0, d15, M5, S5))}
        else:
            r, g, out = run.inp("rois", p0), run.inp("gt", g0), run.out("out", (n, 5))
            rc = lib().jdet_oriented_delta_encode(P(r), P(g), n, c5(M5), c5(S5), P(out), ST(r))

            def ref():
                want = np.asarray(BO.oriented_delta_encode(p0, g0, M5, S5), np.float64)
                # rows where |dtheta| and |dtheta + pi/2| tie within rounding may take the other branch: exact ties only
                d1 = np.abs(BO.regular_theta(g0[:, 4] - p0[:, 4]))
                d2 = np.abs(BO.regular_theta(g0[:, 4] - p0[:, 4] + np.float32(math.pi / 2)))
                ok = np.abs(d1 - d2) > 1e-4                            # tests/test_gpu_boxes.py:331-335
                assert ok.mean() > 0.99

                def err(v):
                    d = np.abs(np.asarray(v, np.float64).reshape(n, 5) - want)
                    d[~ok] = 0.0
                    return d
                return {"out": (err, (2e-4 + 2e-4 * np.abs(want)).reshape(-1))}
        run.ok(rc, "oriented codec")
        return Res({"out": out}, ref)
    return fn


row("jdet_midpoint_offset_decode", "n 257")(_oriented("mid_decode"))
row("jdet_midpoint_offset_encode", "n 257")(_oriented("mid_encode"))
row("jdet_oriented_delta_decode", "n 257 ncls 3")(_oriented("ori_decode"))
row("jdet_oriented_delta_encode", "n 257")(_oriented("ori_encode"))


def _codec64(name):
    """what the rows above leave out -- 15 classes on 257 rois (no multiple of 15) and wh_ratio_clip 0.25 -- on the first
    257 rows of a fixture of tests/codec_ref.py: the float64 restatement, the error measures and the bound (4 x the
    float32 restatement's own error on the fixture) of tests/test_gpu_codecs.py; elements the fixture's retention
    margins keep out are not compared"""
    def fn(run):
        from tests import codec_ref as CR
        f = CR.fixture(name)
        n, C = ORI_N, f.ncls
        a0, d0 = (np.array(a[:n]) for a in f.args)                    # writable copies of the read-only fixture
        a, d, out = run.inp("boxes", a0), run.inp("deltas", d0), run.out("out", (n, 5 * C))
        m, s, clip = f.kw["means"], f.kw["stds"], f.kw["wh_ratio_clip"]
        assert clip == 0.25
        if f.codec == "d2b":
            rc = lib().jdet_delta2bbox_rotated(P(a), P(d), n, C, c5(m), c5(s), clip, P(out), ST(d))
        elif f.codec == "ori_dec":
            rc = lib().jdet_oriented_delta_decode(P(a), P(d), n, C, c5(m), c5(s), clip, P(out), ST(d))
        else:
            rc = lib().jdet_midpoint_offset_decode(P(a), P(d), n, L.vecn(m, 6), L.vecn(s, 6), clip, P(out), ST(d))
        run.ok(rc, CR.ENTRY_POINT[f.codec])

        def ref():
            keep, b = f.keep[:n], f.bound()

            def err(v):
                e = CR.errors(f.codec, np.asarray(v, np.float64).reshape(n, -1), f.ref[:n])
                return np.stack([np.where(keep, e["xywh"], 0.0), np.where(keep, e["angle"], 0.0)], -1)
            return {"out": (err, np.broadcast_to(np.asarray([b["xywh"], b["angle"]]), (n, C, 2)).reshape(-1).copy())}
        return Res({"out": out}, ref)
    return fn


row("jdet_delta2bbox_rotated", "n 257 ncls 15 wh_ratio_clip 0.25, float64 reference")(_codec64("d2b_lo15"))
row("jdet_oriented_delta_decode", "n 257 ncls 15 wh_ratio_clip 0.25, float64 reference")(_codec64("ori_dec_lo15"))
row("jdet_midpoint_offset_decode", "n 257 wh_ratio_clip 0.25, float64 reference")(_codec64("mid_dec_lo"))


def gv_bound(f32, f64):
    """tests/test_gpu_gliding.py:25-26: 4 x the largest float32-vs-float64 difference of the restatement, floor 1e-6"""
    return np.asarray(f64, np.float64), max(4.0 * float(np.abs(np.asarray(f32).astype(np.float64) - f64).max()), 1e-6)


def _gliding(which):
    from tests import gliding_ref as R
    n, ncls = 257, 3
    f4 = lambda v: L.vecn(v, 4)                                        # noqa: E731
    F = np.float32

    def fn(run):
        if which in ("targets", "encode"):
            rois0, polys0 = R.target_case(n, seed=3)
            gts0 = R.poly_hbb(polys0)
            rois = run.inp("rois", rois0.astype(F))
            if which == "targets":
                polys = run.inp("polys", polys0.astype(F))
                bt, ft, rt = run.out("bbox_targets", (n, 4)), run.out("fix_targets", (n, 4)), run.out("ratio_targets", (n, 1))
                rc = lib().jdet_gliding_targets(P(rois), P(polys), n, f4(R.MEANS), f4(R.STDS), P(bt), P(ft), P(rt), ST(rois))
                outs = {"bbox_targets": bt, "fix_targets": ft, "ratio_targets": rt}

                def ref():
                    for p in (polys0, polys0.astype(F)):               # tests/test_gpu_gliding.py:46-47: no row on a tie
                        assert not R.fix_encode(p, with_flags=True)[1].any() and not R.has_vertex_tie(p).any()
                    f64 = R.targets(rois0, polys0, R.MEANS, R.STDS)
                    f32 = R.targets(rois0.astype(F), polys0.astype(F), np.asarray(R.MEANS, F), np.asarray(R.STDS, F))
                    return {k: gv_bound(a, b) for k, a, b in zip(outs, f32, f64)}
            else:
                gts = run.inp("gts", gts0.astype(F))
                out = run.out("out", (n, 4))
                rc = lib().jdet_gv_delta_encode(P(rois), P(gts), n, f4(R.MEANS), f4(R.STDS), P(out), ST(rois))
                outs = {"out": out}
                g32 = gts0.astype(F)
                ref = lambda: {"out": gv_bound(R.delta_encode(rois0.astype(F), g32, np.asarray(R.MEANS, F), np.asarray(R.STDS, F)),
                                               R.delta_encode(rois0, g32.astype(np.float64), R.MEANS, R.STDS))}
        else:
            rois0, bbox0, fix0, ratio0 = R.decode_case(n, ncls, seed=4)
            rois, bbox = run.inp("rois", rois0.astype(F)), run.inp("bbox_pred", bbox0.astype(F))
            if which == "decode":
                fix, ratio = run.inp("fix_pred", fix0.astype(F)), run.inp("ratio_pred", ratio0.astype(F))
                out = run.out("out", (n, 8 * ncls))
                rc = lib().jdet_gliding_decode(P(rois), P(bbox), P(fix), P(ratio), n, ncls, f4(R.MEANS), f4(R.STDS), 16 / 1000,
                                               1024.0, 1024.0, 0.8, f4((1., 1., 1., 1.)), P(out), ST(rois))
                args = (rois0, bbox0, fix0, ratio0)
                ref = lambda: {"out": gv_bound(R.decode_polys(*(a.astype(F) for a in args), R.MEANS, R.STDS, (1024, 1024), ratio_thr=0.8),
                                               R.decode_polys(*args, R.MEANS, R.STDS, (1024, 1024), ratio_thr=0.8))}
            else:
                out = run.out("out", (n, 4 * ncls))
                rc = lib().jdet_gv_delta_decode(P(rois), P(bbox), n, ncls, f4(R.MEANS), f4(R.STDS), 16 / 1000, 1024.0, 1024.0,
                                                P(out), ST(rois))
                ref = lambda: {"out": gv_bound(R.delta_decode(rois0.astype(F), bbox0.astype(F), R.MEANS, R.STDS, (1024, 1024)),
                                               R.delta_decode(rois0, bbox0, R.MEANS, R.STDS, (1024, 1024)))}
            outs = {"out": out}
        run.ok(rc, "gliding codec")
        return Res(outs, ref)
    return fn


row("jdet_gliding_targets", "n 257")(_gliding("targets"))
row("jdet_gliding_decode", "n 257 ncls 3 max_shape 1024")(_gliding("decode"))
row("jdet_gv_delta_encode", "n 257")(_gliding("encode"))
row("jdet_gv_delta_decode", "n 257 ncls 3 max_shape 1024")(_gliding("gv_decode"))


def _anchor_targets(boxes):
    from tests import inputs as I
    A, K = 257, 5
    rng = rng_of(A, K, boxes)
    anchors0, gt0 = I.random_obbs(rng, A), I.random_obbs(rng, K)
    gl0 = rng.integers(1, 16, K).astype(np.int32)
    gi0 = rng.integers(-1, K + 1, A).astype(np.int32)                  # -1 ignored, 0 negative, i + 1 = gt i
    base0 = np.asarray([11], np.int32)
    stds = (0.5, 0.5, 1., 1., 2.)

    def fn(run):
        gt, gl, gi = run.inp("gt", gt0), run.inp("gt_labels", gl0, guard=1), run.inp("gt_inds", gi0, guard=0)
        lab, lw = run.out("labels", (A,), I32), run.out("label_weights", (A,))
        bt, bw = run.out("bbox_targets", (A, 5)), run.out("bbox_weights", (A, 5))
        npos = run.acc("num_pos", base0)
        if boxes:
            rc = lib().jdet_anchor_targets_rotated_boxes(P(gt), P(gl), P(gi), A, K, 2.0, P(lab), P(lw), P(bt), P(bw), P(npos),
                                                         ST(gt))
        else:
            anc = run.inp("anchors", anchors0)
            rc = lib().jdet_anchor_targets_rotated(P(anc), P(gt), P(gl), P(gi), A, K, c5((0,) * 5), c5(stds), 2.0, P(lab),
                                                   P(lw), P(bt), P(bw), P(npos), ST(gt))
        run.ok(rc, "jdet_anchor_targets_rotated")

        def ref():
            from oracle import box_oracle as B
            pos = gi0 > 0
            t = np.zeros((A, 5), np.float32)
            if boxes:
                t[pos] = gt0[gi0[pos] - 1]
                bt_ref = exact(t)                                      # a copy of the assigned gt box
            else:
                t[pos] = B.bbox2delta_rotated(anchors0[pos], gt0[gi0[pos] - 1], (0,) * 5, stds)
                bt_ref = close(t, 2e-5, 2e-5)                          # tests/test_gpu_boxes.py:137
            return {"labels": exact(np.where(pos, gl0[np.maximum(gi0, 1) - 1], 0).astype(np.int32)),     # :134-136: bit-exact
                    "label_weights": exact(np.where(pos, 2.0, np.where(gi0 == 0, 1.0, 0.0)).astype(np.float32)),
                    "bbox_targets": bt_ref, "bbox_weights": exact(np.repeat(pos[:, None], 5, 1).astype(np.float32)),
                    "num_pos": exact(np.asarray([int(pos.sum())]))}
        return Res({"labels": lab, "label_weights": lw, "bbox_targets": bt, "bbox_weights": bw, "num_pos": npos}, ref)
    return fn


row("jdet_anchor_targets_rotated", "A 257 K 5, num_pos on a base of 11")(_anchor_targets(False))
row("jdet_anchor_targets_rotated_boxes", "A 257 K 5, num_pos on a base of 11")(_anchor_targets(True))


# ---- NCHW deformable sampling (csrc/deform_nchw.hip) ---------------------------------------------------------------------
DCN = dict(B=2, C=4, H=9, W=11, k=3, pad=1, stride=1, dil=1, dg=2)
DCN_ATOL = 2e-5
# v1: tests/test_gpu_reference_kernels.py:158 / :162 pin the product's and the oracle's columns to the same bits and
# :159-160 / :163-165 each of the two gradients within 1e-5 of the reference kernels -- 2e-5 between product and oracle
# (the bound of tests/test_gpu_dcn_arf.py:23).  v2: :251 (columns 1e-6), :258-260 (2e-5).


def _dcn_inputs(seed):
    d = DCN
    rng = rng_of(seed, *d.values())
    kk = d["k"] ** 2
    im = randn(rng, d["B"], d["C"], d["H"], d["W"])
    off = randn(rng, d["B"], d["dg"] * 2 * kk, d["H"], d["W"], scale=2.0)
    off.flat[::7] = np.round(off.flat[::7])                            # samples exactly on pixel centres
    mask = rng.uniform(0, 1, (d["B"], d["dg"] * kk, d["H"], d["W"])).astype(np.float32)
    gcol = randn(rng, d["C"] * kk, d["B"], d["H"], d["W"])
    return im, off, mask, gcol


def _dcn_geom():
    d = DCN
    return (d["B"], d["C"], d["H"], d["W"], d["k"], d["k"], d["pad"], d["pad"], d["stride"], d["stride"], d["dil"], d["dil"],
            d["dg"])


def _dcn_oracle_args():
    d = DCN
    return (d["k"], d["k"], (d["pad"],) * 2, (d["stride"],) * 2, (d["dil"],) * 2, d["dg"])


def _mask_cols(mask):
    """mask (B, dg*kk, Ho, Wo) -> the factor of every column element (C*kk, B, Ho, Wo): channel c belongs to
    deformable group c // (C / dg)"""
    d = DCN
    kk, per = d["k"] ** 2, d["C"] // d["dg"]
    m = mask.reshape(d["B"], d["dg"], kk, d["H"], d["W"])
    return np.stack([m[:, c // per] for c in range(d["C"])], 0).transpose(0, 2, 1, 3, 4).reshape(d["C"] * kk, d["B"], d["H"], d["W"])


def _deform_nchw(which, modulated):
    im0, off0, mask0, gcol0 = _dcn_inputs(modulated)
    d = DCN
    kk = d["k"] ** 2

    def fn(run):
        from oracle import oracle as O
        off = run.inp("offset", off0)
        mask = run.inp("mask", mask0) if modulated else None
        lead = (P(off), P(mask)) if modulated else (P(off),)
        oa = _dcn_oracle_args()
        mc = _mask_cols(mask0).astype(np.float64) if modulated else 1.0
        if which == "im2col":
            im, col = run.inp("im", im0), run.out("col", gcol0.shape)
            f = lib().jdet_modulated_deform_im2col if modulated else lib().jdet_deform_im2col
            rc = f(P(im), *lead, *_dcn_geom(), P(col), ST(im))
            outs = {"col": col}

            def ref():
                c = O.deform_im2col(im0, off0, *oa)
                return {"col": ((c * mc), 1e-6) if modulated else exact(c)}
        elif which == "col2im":
            col, gim = run.inp("col", gcol0), run.out("grad_im", im0.shape)
            f = lib().jdet_modulated_deform_col2im if modulated else lib().jdet_deform_col2im
            rc = f(P(col), *lead, *_dcn_geom(), P(gim), ST(col))
            outs = {"grad_im": gim}
            ref = lambda: {"grad_im": (O.deform_col2im((gcol0 * mc).astype(np.float32), off0, im0.shape, *oa).astype(np.float64),
                                       DCN_ATOL)}
        else:
            col, im = run.inp("col", gcol0), run.inp("im", im0)
            goff = run.out("grad_offset", off0.shape)
            outs = {"grad_offset": goff}
            if modulated:
                gmask = run.out("grad_mask", mask0.shape)
                outs["grad_mask"] = gmask
                rc = lib().jdet_modulated_deform_col2im_coord(P(col), P(im), *lead, *_dcn_geom(), P(goff), P(gmask), ST(col))
            else:
                rc = lib().jdet_deform_col2im_coord(P(col), P(im), *lead, *_dcn_geom(), P(goff), ST(col))

            def ref():
                out = {"grad_offset": (O.deform_col2im_coord((gcol0 * mc).astype(np.float32), im0, off0, *oa).astype(np.float64),
                                       DCN_ATOL)}
                if modulated:      # grad_mask = sum over the group's channels of column gradient x unmasked sample
                    prod = gcol0.astype(np.float64) * O.deform_im2col(im0, off0, *oa)
                    per = d["C"] // d["dg"]
                    gm = prod.reshape(d["dg"], per, kk, d["B"], d["H"], d["W"]).sum(1).transpose(2, 0, 1, 3, 4)
                    out["grad_mask"] = (gm.reshape(mask0.shape), DCN_ATOL)
                return out
        run.ok(rc, "deform " + which)
        return Res(outs, ref, atomic=which != "im2col")                # col2im and the coord forms add with float atomics
    return fn


for _mod, _pre in ((False, "jdet_deform_"), (True, "jdet_modulated_deform_")):
    for _which in ("im2col", "col2im", "col2im_coord"):
        row(_pre + _which, "im(2,4,9,11) 3x3 pad 1 dg 2")(_deform_nchw(_which, _mod))


# ---- deformable PS RoI pooling, channels-last ------------------------------------------------------------------------
PS = dict(R=14, N=2, H=20, W=24, od=8, G=2, P=4, part=4, ncls=2, spp=3, tstd=0.2, scale=0.25)     # tests/test_gpu_reference_kernels.py:267


def _psroi_inputs():
    p = PS
    rng = rng_of(*[int(v * 100) for v in p.values()])
    x = randn(rng, p["N"], p["od"] * p["G"] ** 2, p["H"], p["W"])
    rois = np.zeros((p["R"], 5), np.float32)
    rois[:, 0] = rng.integers(0, p["N"], p["R"])
    x1, y1 = rng.uniform(-12, p["W"] / p["scale"], p["R"]), rng.uniform(-12, p["H"] / p["scale"], p["R"])
    rois[:, 1], rois[:, 2] = x1, y1
    rois[:, 3], rois[:, 4] = x1 + rng.uniform(0, p["W"] / p["scale"] / 2, p["R"]), y1 + rng.uniform(0, p["H"] / p["scale"] / 2, p["R"])
    trans = randn(rng, p["R"], 2 * p["ncls"], p["part"], p["part"])
    g = randn(rng, p["R"], p["od"], p["P"], p["P"])
    return x, rois, trans, g


def _psroi(backward):
    p = PS
    x0, rois0, trans0, g0 = _psroi_inputs()
    cfg = (False, p["scale"], p["od"], p["G"], p["P"], p["part"], p["spp"], p["tstd"])
    C = p["od"] * p["G"] ** 2
    args = (p["N"], C, p["H"], p["W"], p["R"], 0, p["scale"], p["od"], p["G"], p["P"], p["part"], p["spp"], p["tstd"],
            2 * p["ncls"])
    cl = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))      # noqa: E731  (R | N, C, h, w) -> channels-last

    def fn(run):
        from oracle import oracle as O
        x, rois, trans = run.inp("input", cl(x0)), run.inp("rois", rois0), run.inp("trans", trans0)
        if not backward:
            out, cnt = run.out("out", (p["R"], p["P"], p["P"], p["od"])), run.out("top_count", (p["R"], p["P"], p["P"], p["od"]))
            run.ok(lib().jdet_deform_psroi_pool_forward(P(x), P(rois), P(trans), *args, P(out), P(cnt), ST(x)), "psroi forward")

            def ref():
                y, c = O.deform_psroi_forward(x0, rois0, trans0, *cfg)
                # tests/test_gpu_reference_kernels.py:283 + :290 (oracle and product each within 2e-6 of the reference
                # kernel), :282 (counts equal)
                return {"out": (cl(y).astype(np.float64), 4e-6), "top_count": exact(cl(c))}
            return Res({"out": out, "top_count": cnt}, ref)
        _, c0 = O.deform_psroi_forward(x0, rois0, trans0, *cfg)
        go, cnt = run.inp("grad_out", cl(g0)), run.inp("top_count", cl(c0))
        gi, gt = run.out("grad_input", (p["N"], p["H"], p["W"], C)), run.out("grad_trans", trans0.shape)
        run.ok(lib().jdet_deform_psroi_pool_backward(P(go), P(cnt), P(x), P(rois), P(trans), *args, P(gi), P(gt), ST(x)),
               "psroi backward")

        def ref():
            o_gi, o_gt = O.deform_psroi_backward(g0, c0, x0, rois0, trans0, *cfg)
            # tests/test_gpu_reference_kernels.py:285 + :291 (2e-5 each), :294-295 (1e-4 of the scale each)
            return {"grad_input": (cl(o_gi).astype(np.float64), 4e-5),
                    "grad_trans": (o_gt.astype(np.float64), 2e-4 * max(1.0, float(np.abs(o_gt).max())))}
        return Res({"grad_input": gi, "grad_trans": gt}, ref, atomic=True)
    return fn


row("jdet_deform_psroi_pool_forward", "R 14 on (2,20,24,32) P 4 part 4")(_psroi(False))
row("jdet_deform_psroi_pool_backward", "R 14 on (2,20,24,32) P 4 part 4")(_psroi(True))


# ---- RepPoints geometry ------------------------------------------------------------------------------------------------
def _pointsets(rng, n, extent=200.0, spread=40.0):
    """tests/test_gpu_convex_ops.py:13-15"""
    c = rng.uniform(spread, extent - spread, size=(n, 1, 2))
    return (c + rng.normal(0, spread / 3, size=(n, 9, 2))).reshape(n, 18).astype(np.float32)


def _quads(rng, m, extent=200.0):
    """tests/test_gpu_convex_ops.py:18-26"""
    c = rng.uniform(30, extent - 30, size=(m, 2))
    w, h, t = rng.uniform(10, 80, m), rng.uniform(6, 50, m), rng.uniform(-np.pi, np.pi, m)
    d = np.asarray([[-.5, -.5], [.5, -.5], [.5, .5], [-.5, .5]])
    out = []
    for i in range(m):
        r = np.asarray([[np.cos(t[i]), np.sin(t[i])], [-np.sin(t[i]), np.cos(t[i])]])
        out.append(((d * [w[i], h[i]]) @ r + c[i]).reshape(8))
    return np.asarray(out, np.float32)


@row("jdet_convex_iou", "67 point sets x 17 quadrilaterals")
def _convex_iou(run):
    rng = rng_of(67, 17)
    ps0, q0 = _pointsets(rng, 67), _quads(rng, 17)
    q0[::3] = q0[::3].reshape(-1, 4, 2)[:, ::-1].reshape(-1, 8)        # some clockwise quadrilaterals
    ps, q, out = run.inp("pointsets", ps0), run.inp("polygons", q0), run.out("ious", (67, 17))
    run.ok(lib().jdet_convex_iou(P(ps), 67, P(q), 17, P(out), ST(ps)), "jdet_convex_iou")

    def ref():
        from oracle import oracle as O
        return {"ious": (O.convex_iou(ps0, q0).astype(np.float64), 1e-6)}          # tests/test_gpu_convex_ops.py:38
    return Res({"ious": out}, ref)


_GIOU_CACHE = {}


def _giou_pairs(n):
    """n aligned (point set, quadrilateral) pairs with the float64 value and central-difference gradient of the
    definition (oracle/convex_giou_oracle.py).  Central differences are a reference only where GIoU is smooth inside
    the step: a point within the step of entering or leaving the hull, or of changing the clip's topology, sits on a
    kink and the quotient there is the mean of two one-sided slopes.  Such pairs are recognised by the reference alone
    -- the quotients of step 1e-3 and 2.5e-4 differ by more than a tenth of the gradient bound -- and are not used."""
    if n not in _GIOU_CACHE:
        from oracle import convex_giou_oracle as G
        m = n + 16
        rng = rng_of(n, 19)
        ps, q = _pointsets(rng, m, spread=30.0), _quads(rng, m)
        q[: m // 2] += (ps[: m // 2].reshape(-1, 9, 2).mean(1) - q[: m // 2].reshape(-1, 4, 2).mean(1))[:, None, :].repeat(4, 1).reshape(-1, 8)
        val, g = G.convex_giou(ps.astype(np.float64), q.astype(np.float64), h=1e-3)
        _, g2 = G.convex_giou(ps.astype(np.float64), q.astype(np.float64), h=2.5e-4)
        smooth = np.abs(g - g2).max(1) <= 0.1 * 2e-3 * max(1e-3, float(np.abs(g).max()))
        keep = np.flatnonzero(smooth)[:n]
        assert keep.size == n and (val[keep] > 0).sum() >= n // 4        # enough smooth pairs, overlapping ones among them
        _GIOU_CACHE[n] = (ps[keep], q[keep], val[keep], g[keep])
    return _GIOU_CACHE[n]


@row("jdet_convex_giou", "37 aligned pairs")
def _convex_giou(run):
    n = 37
    ps0, q0, val, gref = _giou_pairs(n)
    ps, q, out = run.inp("pointsets", ps0), run.inp("polygons", q0), run.out("out", (n, 19))
    run.ok(lib().jdet_convex_giou(P(ps), P(q), n, P(out), ST(ps)), "jdet_convex_giou")

    def ref():
        bound = np.full((n, 19), 2e-3 * max(1e-3, float(np.abs(gref).max())))     # tests/test_gpu_convex_ops.py:124
        bound[:, 18] = 1e-5                                                        # tests/test_gpu_convex_ops.py:121
        return {"out": (np.concatenate([gref, val[:, None]], 1), bound)}
    return Res({"out": out}, ref)


@row("jdet_min_area_bbox", "67 point sets")
def _min_area_bbox(run):
    ps0 = _pointsets(rng_of(67, 8), 67)
    ps, out = run.inp("pointsets", ps0), run.out("bboxes", (67, 8))
    run.ok(lib().jdet_min_area_bbox(P(ps), 67, P(out), ST(ps)), "jdet_min_area_bbox")

    def ref():
        from oracle import oracle as O
        want = O.min_area_bbox(ps0).astype(np.float64)
        area = lambda b: np.linalg.norm(b[:, 0:2] - b[:, 2:4], axis=1) * np.linalg.norm(b[:, 4:6] - b[:, 2:4], axis=1)   # noqa: E731
        # two edge directions can give rectangles of nearly the same area: the areas agree everywhere
        # (tests/test_gpu_convex_ops.py:66: rtol 1e-4)
        return {"bboxes": (lambda v: np.abs(area(np.asarray(v, np.float64).reshape(67, 8)) - area(want)), 1e-4 * area(want))}
    return Res({"bboxes": out}, ref)


def _convex_sort(npts, circular):
    nbs = 33
    rng = rng_of(nbs, npts, circular)
    pts0 = rng.uniform(0, 50, size=(nbs, npts, 2)).astype(np.float32)
    pts0[:, -1] = pts0[:, 0]                                           # a duplicate point in every set
    masks0 = (rng.uniform(size=(nbs, npts)) > 0.3).astype(np.float32)
    masks0[:, 0] = 1

    def fn(run):
        pts, masks = run.inp("pts", pts0), run.inp("masks", masks0)
        out = run.out("index", (nbs, npts + circular), I32)
        run.ok(lib().jdet_convex_sort(P(pts), P(masks), nbs, npts, circular, P(out), ST(pts)), "jdet_convex_sort")

        def ref():
            from oracle import oracle as O
            return {"index": exact(O.convex_sort(pts0, masks0, bool(circular)))}   # tests/test_gpu_convex_ops.py:83
        return Res({"index": out}, ref)
    return fn


for _npts in (9, 64):
    for _circ in (1, 0):
        row("jdet_convex_sort", "nbs 33 npts %d circular %d" % (_npts, _circ))(_convex_sort(_npts, _circ))


# ======================================================================================================================
# the ATSS assigner (tests/test_gpu_atss.py): the restatement of tests/atss_ref.py as the reference, everything exact
# ======================================================================================================================
def atss_case(name, matrix):
    from tests import atss_ref as R
    anchors, num_level, gts, labels, ref = R.fixture(name)
    A, K, nl = anchors.shape[0], gts.shape[0], len(num_level)
    offs = R.level_offsets(num_level)
    ov0 = R.iou_matrix(anchors, gts) if matrix else None

    def fn(run):
        a, g, gl = run.inp("anchors", anchors.copy()), run.inp("gt", gts.copy()), run.inp("gt_labels", labels.copy())
        ov = run.inp("overlaps", ov0) if matrix else None
        gt_inds, max_ov, lab = run.out("gt_inds", (A,), I32), run.out("max_overlaps", (A,)), run.out("labels", (A,), I32)
        ws, wsb = run.ws("workspace", lib().jdet_atss_assign_workspace(A, K, nl, R.TOPK))
        run.ok(lib().jdet_atss_assign(P(a), A, 5, (ctypes.c_int32 * (nl + 1))(*offs.tolist()), nl, P(g), K, P(gl), P(ov),
                                      R.TOPK, 0, P(gt_inds), P(max_ov), P(lab), P(ws), wsb, ST(a)), "jdet_atss_assign")
        return Res({"gt_inds": gt_inds, "max_overlaps": max_ov, "labels": lab},
                   lambda: {"gt_inds": exact(ref["gt_inds"]), "max_overlaps": exact(ref["max_overlaps"]),
                            "labels": exact(ref["labels"])})
    return Case(("jdet_atss_assign",), "%s %s dirty workspace" % (name, "matrix" if matrix else "fused"), fn)


CASES.append(atss_case("256a", False))
CASES.append(atss_case("256a", True))


# ======================================================================================================================
# the row-sparse 3x3 convolutions (csrc/conv_rows.hip): lists of 3 % and of all rows, the corners and the image boundary
# among them; position 0 next to every list
# ======================================================================================================================
ROWS_BOUND = (2e-5, 1e-6)     # tests/test_gpu_conv_rows.py, test_gpu_conv_rows_fwd.py (= tests/test_gpu_conv_igemm.py:45, test_gpu_conv_wgrad.py:48)
ROWS_SHAPES = [(2, 13, 17, 64, 64), (1, 8, 8, 256, 256), (2, 20, 24, 32, 256)]
ROWS_FRACS = (0.03, 1.0)


def dilate3x3(nz):
    """(N, H, W) bool -> the 3x3 dilation inside each image"""
    N, H, W = nz.shape
    pad = np.pad(nz, ((0, 0), (1, 1), (1, 1)))
    out = np.zeros_like(nz)
    for dy in range(3):
        for dx in range(3):
            out |= pad[:, dy:dy + H, dx:dx + W]
    return out


def _listed_rows(rng, N, H, W, frac):
    P_ = N * H * W
    rows = np.sort(rng.choice(P_, max(1, int(round(frac * P_))), replace=False))
    return np.unique(np.concatenate([rows, [0, W - 1, H * W - 1, P_ - 1]]))       # corners and the image boundary


def _padded_list(a, n):
    out = np.full(n, -1, np.int32)
    out[:len(a)] = a
    return out


def rows_inputs(shape, frac):
    """x, w (Cout,Cin,3,3), gy zero outside the listed rows, the list, the list of its dilation"""
    N, H, W, Cin, Cout = shape
    P_ = N * H * W
    rng = np.random.default_rng(N * 1000 + H * 100 + W + Cin + int(frac * 64))
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * (2.0 / (9 * Cin)) ** 0.5).astype(np.float32)
    rows = _listed_rows(rng, N, H, W, frac)
    g = np.zeros((P_, Cout), np.float32)
    g[rows] = rng.standard_normal((len(rows), Cout)).astype(np.float32)
    nz = np.zeros(P_, bool)
    nz[rows] = True
    dil = dilate3x3(nz.reshape(N, H, W))
    return x, w, g.reshape(N, H, W, Cout), rows.astype(np.int32), np.flatnonzero(dil.reshape(-1)).astype(np.int32)


def _rows_grads64(x, w, g):
    x64 = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = torch.from_numpy(w).double().requires_grad_(True)
    gx, gw = torch.autograd.grad(F.conv2d(x64, w64, None, 1, 1), (x64, w64), torch.from_numpy(g).double().permute(0, 3, 1, 2))
    return gx.permute(0, 2, 3, 1).contiguous(), gw.permute(0, 2, 3, 1).contiguous()


def rows_case(entry, shape, frac):
    N, H, W, Cin, Cout = shape
    P_ = N * H * W
    x0, w0, g0, rows0, drows0 = rows_inputs(shape, frac)

    def nonzero(run):
        g = run.inp("g", g0)
        flags, rows, drows = run.out("flags", (P_,), U8), run.out("rows", (P_,), I32), run.out("rows_dilated", (P_,), I32)
        counts = run.out("counts", (2,), I32)
        ws, wsb = run.ws("workspace", lib().jdet_rows_nonzero_workspace(N, H, W))
        run.ok(lib().jdet_rows_nonzero(P(g), N, H, W, Cout, P(flags), P(rows), P(drows), P(counts), P(ws), wsb, ST(g)),
               entry)
        want = np.zeros(P_, np.uint8)
        want[rows0] = 1
        return Res({"flags": flags, "rows": rows, "rows_dilated": drows, "counts": counts},
                   lambda: {"flags": exact(want), "rows": exact(_padded_list(rows0, P_)),
                            "rows_dilated": exact(_padded_list(drows0, P_)),
                            "counts": exact(np.asarray([len(rows0), len(drows0)], np.int32))})

    def wgrad(run):
        x, g = run.inp("x", x0), run.inp("gy", g0)
        rows, count = run.inp("rows", rows0), run.inp("count", np.asarray([len(rows0)], np.int32))     # no entry past the count
        base = np.random.default_rng(5).standard_normal((Cout, 3, 3, Cin)).astype(np.float32)
        gw = run.acc("gw", base)
        run.ok(lib().jdet_conv3x3_wgrad_rows(P(x), P(g), P(rows), P(count), N, H, W, Cin, Cout, P(gw), ST(x)), entry)

        def ref():
            # the value is out - base in float64, so the fp32 roundings of adding onto the base count as error: at most
            # jdet_conv3x3_wgrad_rows_workers() workgroups add to an element, each addition rounds by at most 2^-24 of the
            # running value
            r, bound = rel(_rows_grads64(x0, w0, g0)[1], *ROWS_BOUND)
            return {"gw": (r, bound + lib().jdet_conv3x3_wgrad_rows_workers(Cin, Cout) * 2.0 ** -24 * float(np.abs(base).max() + np.abs(r).max()))}
        return Res({"gw": gw}, ref, atomic=True)

    def dgrad(run):
        g = run.inp("gy", g0)
        wd = run.inp("wd", np.ascontiguousarray(w0[:, :, ::-1, ::-1].transpose(1, 2, 3, 0)))
        rows, count = run.inp("rows", drows0), run.inp("count", np.asarray([len(drows0)], np.int32))
        gx = run.out("gx", (N, H, W, Cin))
        run.ok(lib().jdet_conv3x3_dgrad_rows(P(g), P(wd), P(rows), P(count), N, H, W, Cin, Cout, 1, P(gx), ST(g)), entry)
        return Res({"gx": gx}, lambda: {"gx": rel(_rows_grads64(x0, w0, g0)[0], *ROWS_BOUND)})

    fn = {"jdet_rows_nonzero": nonzero, "jdet_conv3x3_wgrad_rows": wgrad, "jdet_conv3x3_dgrad_rows": dgrad}[entry]
    return Case((entry,), "x(%d,%d,%d,%d) Cout %d rows %.0f%%" % (N, H, W, Cin, Cout, 100 * frac), fn)


def rows_fwd_inputs(shape, frac):
    N, H, W, Cin, Cout = shape
    P_ = N * H * W
    rng = np.random.default_rng(N * 1000 + H * 100 + W + Cin + int(frac * 64) + 1)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * (2.0 / (9 * Cin)) ** 0.5).astype(np.float32)
    b = (0.3 * rng.standard_normal(Cout)).astype(np.float32)
    rows = _listed_rows(rng, N, H, W, frac)
    mask = (rng.random(P_) > 0.2).astype(np.float32)
    return x, w, b, rows.astype(np.int32), mask


def rows_fwd_case(entry, shape, frac):
    N, H, W, Cin, Cout = shape
    P_ = N * H * W
    x0, w0, b0, rows0, mask0 = rows_fwd_inputs(shape, frac)

    def from_flags(run):
        f0 = np.zeros(P_, np.uint8)
        f0[rows0] = 1 + (rows0 % 200).astype(np.uint8)          # any non-zero byte is a flag
        flags = run.inp("flags", f0)
        outs = [run.out(n, (P_,), I32) for n in ("rows", "rows_dilated", "rows_dilated2")]
        counts = run.out("counts", (3,), I32)
        ws, wsb = run.ws("workspace", lib().jdet_rows_from_flags_workspace(N, H, W))
        run.ok(lib().jdet_rows_from_flags(P(flags), N, H, W, P(outs[0]), P(outs[1]), P(outs[2]), P(counts), P(ws), wsb,
                                          ST(flags)), entry)
        nz = (f0 != 0).reshape(N, H, W)
        want = [np.flatnonzero(nz), np.flatnonzero(dilate3x3(nz)), np.flatnonzero(dilate3x3(dilate3x3(nz)))]
        return Res({"rows": outs[0], "rows_dilated": outs[1], "rows_dilated2": outs[2], "counts": counts},
                   lambda: {"rows": exact(_padded_list(want[0], P_)), "rows_dilated": exact(_padded_list(want[1], P_)),
                            "rows_dilated2": exact(_padded_list(want[2], P_)),
                            "counts": exact(np.asarray([len(v) for v in want], np.int32))})

    def forward(run):
        x = run.inp("x", x0)
        w = run.inp("w", np.ascontiguousarray(w0.transpose(0, 2, 3, 1)))
        b, mask = run.inp("bias", b0), run.inp("rowmask", mask0)
        rows, count = run.inp("rows", rows0), run.inp("count", np.asarray([len(rows0)], np.int32))   # no entry past the count
        y = run.out("y", (N, H, W, Cout))
        run.ok(lib().jdet_conv3x3_rows_forward(P(x), P(w), P(b), 1, P(mask), P(rows), P(count), N, H, W, Cin, Cout, 1,
                                               P(y), ST(x)), entry)

        def ref():
            pre = F.conv2d(torch.from_numpy(x0).double().permute(0, 3, 1, 2), torch.from_numpy(w0).double(),
                           torch.from_numpy(b0).double(), 1, 1).permute(0, 2, 3, 1).reshape(P_, Cout).numpy()
            keep = np.zeros(P_)
            keep[rows0] = mask0[rows0]
            full = np.maximum(pre, 0.0)
            r, bound = rel(full, *ROWS_BOUND)          # the bound of the whole map's scale; unlisted / masked rows are 0
            return {"y": ((full * keep[:, None]).reshape(N, H, W, Cout), bound)}
        return Res({"y": y}, ref)

    fn = {"jdet_rows_from_flags": from_flags, "jdet_conv3x3_rows_forward": forward}[entry]
    return Case((entry,), "x(%d,%d,%d,%d) Cout %d rows %.0f%%" % (N, H, W, Cin, Cout, 100 * frac), fn)


for _make, _entries in ((rows_case, ("jdet_rows_nonzero", "jdet_conv3x3_wgrad_rows", "jdet_conv3x3_dgrad_rows")),
                        (rows_fwd_case, ("jdet_rows_from_flags", "jdet_conv3x3_rows_forward"))):
    for _entry in _entries:
        for _shape in ROWS_SHAPES:
            for _frac in ROWS_FRACS:
                CASES.append(_make(_entry, _shape, _frac))


# ======================================================================================================================
# the 3x3 convolution on bf16 MFMA through the three-way split (tests/test_gpu_conv_bf16x3.py, tests/bf16x3_cases.py)
# ======================================================================================================================
def bf16x3_case(case):
    from tests import bf16x3_cases as BC
    N, H, W, Cin, Cout = BC.CASES[case]
    x0, w0, b0, mask0 = BC.inputs(case)

    def fn(run):
        x, w = run.inp("x", np.array(x0)), run.inp("w", np.array(w0))
        b, mask = run.inp("bias", np.array(b0)), run.inp("rowmask", np.array(mask0))
        y = run.out("y", (N, H, W, Cout))
        run.ok(lib().jdet_conv3x3_bf16x3_forward(P(x), N, H, W, Cin, P(w), Cout, P(b), 1, P(mask), P(y), ST(x)),
               "jdet_conv3x3_bf16x3_forward")

        def ref():
            full = np.maximum(BC.reference(case, True), 0.0)
            bound = BC.BOUND[0] * np.abs(full).max() + BC.BOUND[1]
            return {"y": (full * mask0.astype(np.float64).reshape(N, H, W, 1), bound)}
        return Res({"y": y}, ref)
    return Case(("jdet_conv3x3_bf16x3_forward",), "case " + case, fn)


CASES.append(bf16x3_case("b"))


# ======================================================================================================================
# rotated FCOS (tests/test_gpu_fcos.py states the bounds): point targets against the restatement of tests/fcos_ref.py,
# the polygon IoU loss at 4 x the float32 restatement's own error
# ======================================================================================================================
def fcos_ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def fcos_padded(gts, labels, dev, poison=True):
    """(B, Kmax, 5), (B, Kmax) int32, (B,) int32 on the device; the rows beyond an image's count hold NaN / a wild label"""
    B, Kmax = len(gts), max(max(len(g) for g in gts), 1)
    g = np.full((B, Kmax, 5), np.nan if poison else 0.0, np.float32)
    lab = np.full((B, Kmax), 77 if poison else 0, np.int32)
    for b in range(B):
        g[b, :len(gts[b])] = gts[b]
        lab[b, :len(gts[b])] = labels[b]
    cnt = np.asarray([len(x) for x in gts], np.int32)
    return torch.from_numpy(g).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(cnt).to(dev)


def fcos_centerness_bound(ref, tol, norm_on_bbox):
    """c = sqrt(m1/M1 * m2/M2) with every distance off by at most d: |dc| <= c * d * (1/m1 + 1/m2) to first order (doubled
    here), + 4 ulp for the closed form itself; d = tol, divided by the stride where the targets are"""
    from tests import fcos_ref as R
    t = ref["bbox_targets"]
    d = tol / (np.asarray(R.STRIDES, np.float64)[R.points_of()[1]] if norm_on_bbox else 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        b = 2 * ref["centerness"] * d * (1 / np.minimum(t[:, 0], t[:, 2]) + 1 / np.minimum(t[:, 1], t[:, 3]))
    return np.where(ref["inds"] >= 0, b + 4 * fcos_ulp(1.0), 0.0)


def fcos_targets_case(name, norm_on_bbox, center_sampling):
    from tests import fcos_ref as R
    gts, labels = R.target_fixture(name)
    B, N = len(gts), 341
    refs = [R.targets(g, gl, norm_on_bbox, center_sampling) for g, gl in zip(gts, labels)]
    tol = 8 * fcos_ulp(max([float(R.IMG)] + [float(np.abs(g[:, :4]).max()) for g in gts if len(g)]))
    lv = (ctypes.c_int32 * 15)(*[int(v) for (h, w), s in zip(R.SIZES, R.STRIDES) for v in (h, w, s)])
    rr = (ctypes.c_float * 10)(*[float(v) for r in R.RANGES for v in r])

    def fn(run):
        g0, l0, c0 = fcos_padded(gts, labels, "cpu", poison=run.hostile)
        g, gl, gc = run.inp("gt", g0.numpy()), run.inp("gt_labels", l0.numpy(), guard=99), run.inp("gt_count", c0.numpy(),
                                                                                                   guard=100)
        lab, tgt = run.out("labels", (B, N), I32), run.out("bbox_targets", (B, N, 5))
        ctr, inds = run.out("centerness", (B, N)), run.out("gt_inds", (B, N), I32)
        run.ok(lib().jdet_fcos_targets(lv, rr, 5, P(g), P(gl), P(gc), B, g0.shape[1], R.NUM_CLASSES, int(norm_on_bbox),
                                       int(center_sampling), R.RADIUS, P(lab), P(tgt), P(ctr), P(inds), ST(g)),
               "jdet_fcos_targets")
        return Res({"labels": lab, "bbox_targets": tgt, "centerness": ctr, "gt_inds": inds},
                   lambda: {"labels": exact(np.stack([r["labels"] for r in refs])),
                            "gt_inds": exact(np.stack([r["inds"] for r in refs])),
                            "bbox_targets": (np.stack([r["bbox_targets"] for r in refs]), tol),
                            "centerness": (np.stack([r["centerness"] for r in refs]),
                                           np.stack([fcos_centerness_bound(r, tol, norm_on_bbox) for r in refs]))})
    return Case(("jdet_fcos_targets",), "%s norm %d cs %d" % (name, norm_on_bbox, center_sampling), fn)


def fcos_loss_case(weighted):
    from tests import fcos_ref as R
    prd, tgt, _ = R.loss_fixture()
    ref, e_loss, e_grad = R.loss_reference(False, weighted)
    n = len(prd)

    def fn(run):
        p, t = run.inp("pred", np.array(prd)), run.inp("target", np.array(tgt))
        w = run.inp("weight", np.array(R.loss_weights())) if weighted else None
        loss, grad = run.out("loss", (n,)), run.out("grad_pred", (n, 5))
        run.ok(lib().jdet_poly_iou_loss(P(p), P(t), P(w), n, 0, 1e-6, P(loss), P(grad), ST(p)), "jdet_poly_iou_loss")
        gmax = np.abs(ref["grad"]).max(1, keepdims=True)
        return Res({"loss": loss, "grad_pred": grad},
                   lambda: {"loss": (ref["loss"], 4 * e_loss),
                            "grad_pred": (ref["grad"], np.broadcast_to(4 * e_grad * gmax, ref["grad"].shape).copy())})
    return Case(("jdet_poly_iou_loss",), "257 rows%s" % (" weighted" if weighted else ""), fn)


FCOS_CONTRACTS = {
    "targets k7_k0": lambda: fcos_targets_case("k7_k0", True, False),
    "targets k7_k0 cs": lambda: fcos_targets_case("k7_k0", True, True),
    "targets k70 cs": lambda: fcos_targets_case("k70", False, True),
    "loss": lambda: fcos_loss_case(False),
    "loss weighted": lambda: fcos_loss_case(True),
}
for _k in sorted(FCOS_CONTRACTS):
    CASES.append(FCOS_CONTRACTS[_k]())


# ======================================================================================================================
# Rotated RepPoints (tests/test_gpu_reppoints.py): the assigner against the sequential loop of tests/reppoints_ref.py,
# the dense GIoU loss against the general route on the device, both bit for bit
# ======================================================================================================================
def giou_loss_rows(seed=5, P=300, n_pos=100):
    """pred (P, 18), target (P, 8), weight (P), norm (P): n_pos positive rows at random positions (a rotated box and
    nine points scattered over it), the rest weight 0 with NaN in pred and target; norm per row in {16, 32, 64}"""
    from tests import reppoints_ref as R
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(P, n_pos, replace=False))
    norm = rng.choice(np.asarray([16.0, 32.0, 64.0], np.float32), P).astype(np.float32)
    pred = np.full((P, 18), np.nan, np.float32)
    target = np.full((P, 8), np.nan, np.float32)
    weight = np.zeros(P, np.float32)
    c = rng.uniform(50, 200, (n_pos, 2))
    wh = np.exp(rng.uniform(np.log(16.0), np.log(160.0), (n_pos, 2)))
    target[pos] = R.obb_poly(c, wh, rng.uniform(-np.pi / 2, np.pi / 2, n_pos))
    spread = rng.uniform(0.15, 0.8, (n_pos, 1, 1)) * wh.mean(1)[:, None, None]
    shift = rng.uniform(-0.5, 0.5, (n_pos, 1, 2)) * wh[:, None, :]
    pred[pos] = (c[:, None, :] + shift + rng.normal(0, 1, (n_pos, 9, 2)) * spread).reshape(n_pos, 18).astype(np.float32)
    weight[pos] = rng.uniform(0.5, 2.0, n_pos).astype(np.float32)
    return pred, target, weight, norm, pos


def giou_general_rows(pred, target, weight, norm):
    """the general route on device tensors of the positive rows: torch fp32 division, reppoints_convex_giou, the rule"""
    from jdet_amd.models.losses.convex_giou_loss import convex_giou_rows
    loss, grad = convex_giou_rows(pred / norm[:, None], target / norm[:, None], weight)
    return loss, grad / norm[:, None]


def point_assign_case(name, pos_num, with_labels, stride):
    from tests import reppoints_ref as R
    fx = R.fixture(name)
    B, Kmax, N = fx["gt"].shape[0], fx["gt"].shape[1], len(fx["points"])
    refs = [R.assign_loop(fx["points"], fx["sizes"], fx["level_ids"], fx["gt"][b, :k], fx["labels"][b, :k],
                          pos_num=pos_num, labels_filled=-1) for b, k in enumerate(fx["counts"])]
    offs = (ctypes.c_int32 * 6)(*np.concatenate([[0], np.cumsum(fx["sizes"])]).tolist())
    ids = (ctypes.c_int32 * 5)(*fx["level_ids"])

    def fn(run):
        gt = fx["gt"].copy()
        if run.hostile:                                     # rows beyond an image's count are never read
            for b, k in enumerate(fx["counts"]):
                gt[b, k:] = np.nan
        pts = run.strided("points", fx["points"], stride)
        g, gl = run.inp("gt", gt), run.inp("gt_labels", fx["labels"], guard=99)
        gc = run.inp("gt_count", np.asarray(fx["counts"], np.int32), guard=100)
        gi = run.out("gt_inds", (B, N), I32)
        lab = run.out("labels", (B, N), I32) if with_labels else None
        ws, wsb = run.ws("workspace", lib().jdet_convex_point_assign_workspace(B, N))
        run.ok(lib().jdet_convex_point_assign(P(pts), N, stride, offs, ids, 5, P(g), P(gl) if with_labels else None,
                                              P(gc), B, Kmax, R.SCALE, pos_num, -1, P(gi), P(lab), P(ws), wsb, ST(g)),
               "jdet_convex_point_assign")
        outs = {"gt_inds": gi}
        want = {"gt_inds": exact(np.stack([r["gt_inds"] for r in refs]))}
        if with_labels:
            outs["labels"] = lab
            want["labels"] = exact(np.stack([r["labels"] for r in refs]))
        return Res(outs, lambda: want)
    return Case(("jdet_convex_point_assign",), "%s pos_num %d%s stride %d" % (name, pos_num,
                                                                               " labels" if with_labels else "", stride), fn)


def giou_loss_case():
    pred, target, weight, norm, pos = giou_loss_rows(seed=7, P=131, n_pos=40)

    def fn(run):
        nm = norm.copy()
        if run.hostile:                                     # a row of weight 0 does not read its norm either
            nm[weight == 0] = np.nan
        p, tg, w, n = run.inp("pred", pred), run.inp("target", target), run.inp("weight", weight), run.inp("norm", nm)
        loss, grad = run.out("loss", (131,)), run.out("grad_pred", (131, 18))
        run.ok(lib().jdet_convex_giou_loss(P(p), P(tg), P(w), P(n), 131, P(loss), P(grad), ST(p)),
               "jdet_convex_giou_loss")

        def ref():
            want_loss, want_grad = np.zeros(131, np.float32), np.zeros((131, 18), np.float32)
            # the reference of the positive rows is the general route, which is device code: a run on host buffers
            # (tests/test_guarded_cpu.py) has the zero rows and the shapes only
            if run.dev.type == "cuda":
                t = lambda a: torch.from_numpy(a).to(run.dev)  # noqa: E731
                ref_loss, ref_grad = giou_general_rows(t(pred[pos]), t(target[pos]), t(weight[pos]), t(norm[pos]))
                want_loss[pos], want_grad[pos] = ref_loss.cpu().numpy(), ref_grad.cpu().numpy()
            return {"loss": exact(want_loss), "grad_pred": exact(want_grad)}
        return Res({"loss": loss, "grad_pred": grad}, ref)
    return Case(("jdet_convex_giou_loss",), "131 rows, 40 positive", fn)


REPPOINTS_CONTRACTS = {
    "assign b2_256": lambda: point_assign_case("b2_256", 3, True, 4),
    "assign k70_k0": lambda: point_assign_case("k70_k0", 1, False, 2),
    "loss": giou_loss_case,
}
for _k in sorted(REPPOINTS_CONTRACTS):
    CASES.append(REPPOINTS_CONTRACTS[_k]())


# ======================================================================================================================
# H2RBox (tests/test_gpu_h2rbox.py states the bounds): every bound is 4 x the error of the float32 restatement of
# tests/h2rbox_ref.py against the float64 one
# ======================================================================================================================
# the issue's two frames, and the non-square one again with a margin of 1 px: there every padding rule acts where H != W
H2RBOX_FRAMES = {"37x37->32x32": ((37, 37), (32, 32)), "40x56->24x40": ((40, 56), (24, 40)),
                 "40x56->38x54": ((40, 56), (38, 54))}


def rotate_crop_case(frame, theta, padding):
    from tests import h2rbox_ref as R
    from jdet_amd.ops.rotate_crop import PADDING
    (h, w), size = H2RBOX_FRAMES[frame]
    img = R.image_fixture(h, w)

    def fn(run):
        x = run.inp("img", img.copy())
        out = run.out("out", (2, 3) + size)
        cs, sn = (1.0, 0.0) if theta == 0 else (math.cos(theta), math.sin(theta))
        run.ok(lib().jdet_rotate_crop(P(x), 2, 3, h, w, size[0], size[1], cs, sn, PADDING[padding], P(out), ST(x)),
               "jdet_rotate_crop")
        if theta == 0:
            ch, cw = (h - size[0]) // 2, (w - size[1]) // 2
            return Res({"out": out}, lambda: {"out": exact(img[..., ch:ch + size[0], cw:cw + size[1]])})
        ref, e32 = R.rotate_crop_reference(h, w, size, theta, padding)
        return Res({"out": out}, lambda: {"out": (ref, 4 * e32)})
    return Case(("jdet_rotate_crop",), "%s theta %.1f %s" % (frame, theta, padding), fn)


def _aug_args(run, rot, win, hostile_rows):
    from tests import h2rbox_ref as R
    pred, pred_aug, weight, labels, _ = R.loss_fixture(rot, win)
    ref = R.loss_reference(rot, win)[0]
    p1, p2 = pred.copy(), pred_aug.copy()
    if hostile_rows and run.hostile:                         # the rows nobody may read hold NaN in the hostile runs
        hit = np.zeros((R.B, R.N), bool)
        for b in range(R.B):
            hit[b, ref["aug_index"][b][ref["aug_index"][b] >= 0]] = True
        p1[weight == 0] = np.nan
        p2[~hit] = np.nan
    lv = (ctypes.c_int32 * (3 * len(R.SIZES)))(*[int(v) for (h, w), s in zip(R.SIZES, R.STRIDES) for v in (h, w, s)])
    ag = (ctypes.c_int32 * len(R.AGNOSTIC))(*R.AGNOSTIC)
    t = [run.inp("pred", p1), run.inp("pred_aug", p2), run.inp("weight", weight.copy()),
         run.inp("labels", labels.copy(), guard=99)]
    rf = R.f32(rot)
    head = (lv, len(R.SIZES), P(t[0]), P(t[1]), P(t[2]), P(t[3]), ag, len(R.AGNOSTIC), R.B, rf, math.cos(rf), math.sin(rf),
            R.CROP[0], R.CROP[1], R.WEIGHTS["shape"], R.WEIGHTS["angle"], R.EPS)
    return head, t, ref, (pred, pred_aug, weight, labels)


def _terms64(ref, data, rot):
    """the error measure of `terms` for the contract rows: exact zeros in the rows that take no part, the weight in
    column 3 and finite, non-negative terms in the valid rows (the VALUES are held to the float64 column sums in
    test_aug_terms_select_the_scalar_minimum and, through the loss, in the float64 comparison of
    tests/test_gpu_h2rbox.py; the contract row adds the guard bands, the full overwrite and B == A bit for bit with NaN
    in the rows nobody may read)"""
    from tests import h2rbox_ref as R
    pred, pred_aug, weight, labels = data
    valid = ref["aug_index"] >= 0

    def err(v):
        v = v.reshape(R.B, R.N, 4)
        bad = np.zeros_like(v)
        bad[~valid] = np.abs(v[~valid])                      # must be 0
        bad[valid, 3] = np.abs(v[valid, 3] - weight[valid])  # must be the weight
        bad[valid, :3] = np.where(np.isfinite(v[valid, :3]) & (v[valid, :3] >= 0), 0.0, 1.0)
        return bad
    return err


def aug_forward_case(rot, win):
    from tests import h2rbox_ref as R

    def fn(run):
        head, t, ref, data = _aug_args(run, rot, win, True)
        terms, idx = run.out("terms", (R.B, R.N, 4)), run.out("aug_index", (R.B, R.N), I32)
        run.ok(lib().jdet_h2rbox_aug_loss_forward(*head, P(terms), P(idx), ST(t[0])), "jdet_h2rbox_aug_loss_forward")
        return Res({"terms": terms, "aug_index": idx},
                   lambda: {"aug_index": exact(ref["aug_index"]), "terms": (_terms64(ref, data, rot), 0.0)})
    return Case(("jdet_h2rbox_aug_loss_forward",), "rot %.1f branch %d" % (rot, win), fn)


def aug_backward_case(rot, win):
    from tests import h2rbox_ref as R

    def fn(run):
        head, t, ref, data = _aug_args(run, rot, win, True)
        _, e_loss, e_g1, e_g2 = R.loss_reference(rot, win)
        scale = R.WEIGHTS["loss_weight"] / ref["avg"]
        idx = run.inp("aug_index", ref["aug_index"].copy(), guard=100)
        br = run.inp("branch", np.array([win - 1], np.int32), guard=101)
        sc = run.inp("scale_centre", np.array([scale * R.WEIGHTS["centre"]], np.float32))
        sb = run.inp("scale_branch", np.array([scale], np.float32))
        g1, g2 = run.out("grad_pred", (R.B, R.N, 5)), run.out("grad_pred_aug", (R.B, R.N, 5))
        scratch = run.out("contrib", (R.B, R.N, 5))
        run.ok(lib().jdet_h2rbox_aug_loss_backward(*head, P(idx), P(br), P(sc), P(sb), P(g1), P(g2), P(scratch),
                                                   ST(t[0])), "jdet_h2rbox_aug_loss_backward")
        # the scales enter as float32: one more rounding each (2^-24 relative) on top of the gradient bound
        m1, m2 = np.abs(ref["grad_pred"]).max(), np.abs(ref["grad_aug"]).max()
        return Res({"grad_pred": g1, "grad_pred_aug": g2},
                   lambda: {"grad_pred": (ref["grad_pred"], (4 * e_g1 + 2.0 ** -23) * m1),
                            "grad_pred_aug": (ref["grad_aug"], (4 * e_g2 + 2.0 ** -23) * m2)})
    return Case(("jdet_h2rbox_aug_loss_backward",), "rot %.1f branch %d" % (rot, win), fn)


H2RBOX_CONTRACTS = {
    "rotate 37 reflection": lambda: rotate_crop_case("37x37->32x32", -2.5, "reflection"),
    "rotate 40x56 zeros": lambda: rotate_crop_case("40x56->24x40", 0.3, "zeros"),
    "rotate 40x56 copy": lambda: rotate_crop_case("40x56->24x40", 0.0, "border"),
    "rotate 40x56 thin border": lambda: rotate_crop_case("40x56->38x54", -2.5, "border"),
    "forward branch 1": lambda: aug_forward_case(0.3, 1),
    "forward branch 2": lambda: aug_forward_case(-2.5, 2),
    "backward branch 1": lambda: aug_backward_case(0.3, 1),
    "backward branch 2": lambda: aug_backward_case(math.pi / 2, 2),
}
for _k in sorted(H2RBOX_CONTRACTS):
    CASES.append(H2RBOX_CONTRACTS[_k]())


# ======================================================================================================================
# localization distillation (tests/test_gpu_ld.py states the bounds and the regimes): every bound is 4 x the error of the
# float32 restatement of tests/ld_ref.py against the float64 one
# ======================================================================================================================
def dist_integral_case(rows, reg_max):
    from tests import ld_ref as R
    x0 = R.bbox_fixture(rows, reg_max, 0.0, "ones")["logits"]
    ref = R.integral(x0, reg_max).numpy()
    e32 = float(np.abs(R.integral(x0, reg_max, torch.float32).double().numpy() - ref).max())

    def fn(run):
        x, out = run.inp("logits", x0), run.out("deltas", (rows, 5))
        run.ok(lib().jdet_dist_integral(P(x), rows, reg_max, *R.ENDS, *R.ANGLE_ENDS, P(out), ST(x)), "jdet_dist_integral")
        assert e32 > 0
        return Res({"deltas": out}, lambda: {"deltas": (ref, 4 * e32)})          # tests/test_gpu_ld.py: test_integral_against_float64
    return Case(("jdet_dist_integral",), "rows %d R %d" % (rows, reg_max), fn)


def dist_bbox_case(rows, reg_max, beta, wmode, windowed=False, unaligned=False):
    """contract row of jdet_dist_bbox_loss_level.  windowed: rows = 2 n, target / weight the windows [:, 7:7 + n] of
    (2, n + 69, 5) arrays whose other rows are NaN; unaligned: logits and gradient 4 bytes off a 16-byte boundary.
    Hostile runs: NaN in the logits of rows whose five weights are 0 and in the targets of weight 0."""
    from tests import ld_ref as R
    f = R.bbox_fixture(rows, reg_max, beta, "ones" if wmode == "zeros" else wmode)
    weight = np.zeros_like(f["weight"]) if wmode == "zeros" else f["weight"]
    K5 = 5 * (reg_max + 1)

    def fn(run):
        x, t = f["logits"].copy(), f["target"].copy()
        if run.hostile:
            x[(weight == 0).all(axis=1)] = np.nan
            t[weight == 0] = np.nan
        n, total, start = rows, rows, 0
        tw = [t, weight]
        if windowed:
            n = rows // 2
            total, start = n + 69, 7
            tw = [R.window(a.reshape(2, n, 5), total, start) for a in tw]
        pad = 1 if unaligned else 0
        xin = run.inp("logits", np.concatenate([np.zeros(pad, np.float32), x.reshape(-1)]))
        tin, win = run.inp("target", tw[0]), run.inp("weight", tw[1])
        avg = run.inp("avg_factor", np.array([R.AVG], np.float32))
        loss, grad = run.out("loss", (1,)), run.out("grad_logits", (rows * K5 + pad,))
        ws, wsb = run.ws("workspace", lib().jdet_sigmoid_focal_loss_workspace())
        off = start * 5 * 4
        run.ok(lib().jdet_dist_bbox_loss_level(
            P(xin) + 4 * pad, P(tin) + off, n, total, P(win) + off, n, total, rows, reg_max, *R.ENDS, *R.ANGLE_ENDS,
            float(beta), P(avg), R.LOSS_WEIGHT, P(loss), P(grad) + 4 * pad, P(ws), wsb, ST(xin)),
            "jdet_dist_bbox_loss_level")
        if pad:                                              # the word in front of the unaligned gradient is nobody's
            grad[:1].zero_()
        if wmode == "zeros":
            return Res({"loss": loss, "grad_logits": grad},
                       lambda: {"loss": exact(np.zeros(1)), "grad_logits": exact(np.zeros(rows * K5 + pad))})
        unit = np.concatenate([np.zeros(pad), f["ref"][1].reshape(-1) * (R.AVG / R.LOSS_WEIGHT)])
        print("bbox rows %d reg_max %d beta %.3f %s: bounds loss %.3e grad %.3e" % (rows, reg_max, beta, wmode, 4 * f["e_loss"], 4 * f["e_grad"]))
        assert f["e_loss"] > 0 and f["e_grad"] > 0
        return Res({"loss": loss, "grad_logits": grad},
                   lambda: {"loss": (np.array([f["ref"][0]]), 4 * f["e_loss"]),
                            "grad_logits": (unit, 4 * f["e_grad"] * np.abs(unit).max())})
    return Case(("jdet_dist_bbox_loss_level",), "rows %d R %d beta %.2f %s%s%s" % (
        rows, reg_max, beta, wmode, " window" if windowed else "", " unaligned" if unaligned else ""), fn)


def _kl_blocks(M):
    return 5 if M % 5 == 0 and M > 5 else (4 if M % 4 == 0 and M > 4 else 1)


def _kl_args(run, f, M, K, windowed, unaligned=False):
    """inputs of both KL entry points -> (pred, soft, weight pointer, rows_per_block, block_stride, tensors)"""
    from tests import ld_ref as R
    pred, soft, weight = f["pred"].copy(), f["soft"].copy(), f["weight"]
    if run.hostile and weight is not None and (weight > 0).any():
        pred[weight <= 0] = np.nan                           # rows nobody may use
        soft[weight <= 0] = np.nan
    pad = 1 if unaligned else 0
    p = run.inp("pred", np.concatenate([np.zeros(pad, np.float32), pred.reshape(-1)]))
    s = run.inp("soft", np.concatenate([np.zeros(pad, np.float32), soft.reshape(-1)]))
    if weight is None:
        return (P(p) + 4 * pad, P(s) + 4 * pad, None, 1, 0), p
    if windowed:
        B = _kl_blocks(M)
        n = M // B
        w = run.inp("weight", R.window(weight.reshape(B, n), n + 13, 3))
        return (P(p) + 4 * pad, P(s) + 4 * pad, P(w) + 3 * 4, n, n + 13), p
    w = run.inp("weight", weight)
    return (P(p) + 4 * pad, P(s) + 4 * pad, P(w), M, M), p


def kl_forward_case(M, K, T, wmode, windowed=False, unaligned=False):
    from tests import ld_ref as R
    f = R.kl_fixture(M, K, T, wmode)

    def fn(run):
        head, p = _kl_args(run, f, M, K, windowed, unaligned)
        loss, count = run.out("loss", (1,)), run.out("count", (1,), I32)
        ws, wsb = run.ws("workspace", lib().jdet_sigmoid_focal_loss_workspace())
        run.ok(lib().jdet_kd_kl_div_level_forward(*head, M, K, float(T), R.LOSS_WEIGHT, P(loss), P(count), P(ws), wsb,
                                                  ST(p)), "jdet_kd_kl_div_level_forward")
        print("kl forward M %d K %d T %d %s: bound %.3e" % (M, K, T, wmode, 4 * f["e_loss"]))
        assert f["e_loss"] > 0
        return Res({"loss": loss, "count": count},
                   lambda: {"loss": (np.array([f["ref"][0]]), 4 * f["e_loss"]), "count": exact(np.array([f["ref"][2]]))})
    return Case(("jdet_kd_kl_div_level_forward",), "M %d K %d T %d %s" % (M, K, T, wmode), fn)


def kl_backward_case(M, K, T, wmode, windowed=False, unaligned=False):
    from tests import ld_ref as R
    f = R.kl_fixture(M, K, T, wmode)
    go = 0.75

    def fn(run):
        head, p = _kl_args(run, f, M, K, windowed, unaligned)
        pad = 1 if unaligned else 0
        count = run.inp("count", np.array([f["ref"][2]], np.int32), guard=1)
        gout = run.inp("grad_out", np.array([go], np.float32))
        grad = run.out("grad_pred", (M * K + pad,))
        run.ok(lib().jdet_kd_kl_div_level_backward(*head, M, K, float(T), R.LOSS_WEIGHT, P(count), P(gout),
                                                   P(grad) + 4 * pad, ST(p)), "jdet_kd_kl_div_level_backward")
        if pad:
            grad[:1].zero_()
        ref = np.concatenate([np.zeros(pad), f["ref"][1].reshape(-1) * go])
        print("kl backward M %d K %d T %d %s: bound %.3e" % (M, K, T, wmode, 4 * f["e_grad"]))
        assert f["e_grad"] > 0

        def err(v):                                          # unselected rows: exactly 0; the others within the bound
            d = np.abs(v - ref)
            if f["weight"] is not None and (f["weight"] > 0).any():
                unsel = np.concatenate([np.zeros(pad, bool), np.repeat(f["weight"] <= 0, K)])
                d[unsel] = np.where(v[unsel] == 0, 0.0, np.inf)
            return d
        return Res({"grad_pred": grad}, lambda: {"grad_pred": (err, 4 * f["e_grad"] * np.abs(ref).max())})
    return Case(("jdet_kd_kl_div_level_backward",), "M %d K %d T %d %s" % (M, K, T, wmode), fn)


# the smallest instances; the capped grids (60 000 anchors, 270 001 KL rows) stay parametrisations of tests/test_gpu_ld.py
CASES.append(dist_integral_case(63, 8))
CASES.append(dist_bbox_case(63, 8, 0.0, "ones"))
CASES.append(kl_forward_case(64, 9, 2, "mixed", windowed=True))
CASES.append(kl_backward_case(64, 9, 2, "mixed", windowed=True))
