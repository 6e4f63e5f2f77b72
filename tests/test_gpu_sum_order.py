"""GPU: the ORDER of summation of the two-stage sum kernels, bit for bit against the float32 emulation
of tests/sum_order_ref.py (held to the float64 sums by tests/test_sum_order_cpu.py, which also shows that these inputs
exercise the order).  tests/test_gpu_dense_losses.py and tests/test_gpu_bn_sums.py allow counted rounding bounds on
normal inputs; a kernel that reassociated its sums would pass them and still move every loss and every BatchNorm / bias
gradient in its last bits.  Here the per-element terms are exactly reproducible on the host (L1 with weights, masked
gradients, g * x with mean 0 / var 1 / eps 0), so every output must EQUAL the emulation: loss totals, the partial sums
in the workspace, per-channel sums.  Outputs sit between guard bands and start as canaries; each case runs once."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import sum_order_ref as S

pytestmark = pytest.mark.gpu

F32 = np.float32


def _out(name, shape, dev):
    return G.Buf(name, "out", shape, torch.float32, dev, G.CANARY_WORD, payload_word=G.CANARY_WORD)


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _done(bufs, written):
    torch.cuda.synchronize()
    for b in bufs:
        b.check_guards()
    for b in written:
        b.check_written()


def _equal(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want, F32).reshape(-1))
    got = got.detach().cpu().reshape(-1)[:want.numel()]
    if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero().reshape(-1)
        k = int(bad[0])
        raise AssertionError("%s: %d of %d values differ in bits from the emulated order, first at %d: got %r, emulated %r"
                             % (what, bad.numel(), want.numel(), k, float(got[k]), float(want[k])))


def _loss_workspace(L, dev):
    nbytes = L.lib().jdet_sigmoid_focal_loss_workspace()
    return _out("ws", (nbytes // 4,), dev), nbytes


# ---- (a) the loss tree ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.L1_SIZES)
def test_l1_loss_sum_order(dev, n):
    """one thread; one workgroup with a ragged last wave; several ragged workgroups; past the 1024-workgroup cap"""
    from jdet_amd import _lib as L
    pred, target, weight, total, partial = S.l1_case(n)
    dp, dt, dw = _d(pred, dev), _d(target, dev), _d(weight, dev)
    loss, grad = _out("loss", (1,), dev), _out("grad", (n,), dev)
    ws, wsb = _loss_workspace(L, dev)
    L.check(L.lib().jdet_smooth_l1_loss(L.ptr(dp), L.ptr(dt), L.ptr(dw), n, 0.0, L.ptr(loss.t), L.ptr(grad.t), L.ptr(ws.t),
                                        wsb, L.stream_ptr(dp)), "jdet_smooth_l1_loss")
    _done([loss, grad, ws], [loss, grad])
    _equal(ws.t, partial, "partial sums")
    _equal(loss.t, total, "loss sum")


@pytest.mark.parametrize("s,e", S.L1_WINDOWS)
def test_l1_loss_level_sum_order(dev, s, e):
    """the window [:, s:e, :] of (3, 30 000, 5) target / weight arrays (NaN outside), (total / avg_factor) * loss_weight"""
    from jdet_amd import _lib as L
    E = S.E
    rows = S.N_IMG * (e - s)
    pred, tgt, w, total, partial = S.l1_case(rows * E)
    targets = np.full((S.N_IMG, S.ANCHORS, E), np.nan, F32)
    weights = np.full((S.N_IMG, S.ANCHORS, E), np.nan, F32)
    targets[:, s:e], weights[:, s:e] = tgt.reshape(S.N_IMG, -1, E), w.reshape(S.N_IMG, -1, E)
    dp, dt, dw, davg = _d(pred, dev), _d(targets, dev), _d(weights, dev), _d(np.array([S.AVG], F32), dev)
    loss, grad = _out("loss", (1,), dev), _out("grad", (rows, E), dev)
    ws, wsb = _loss_workspace(L, dev)
    L.check(L.lib().jdet_smooth_l1_loss_level(
        L.ptr(dp), dt.data_ptr() + 4 * s * E, e - s, S.ANCHORS, dw.data_ptr() + 4 * s * E, e - s, S.ANCHORS, rows, E, 0.0,
        L.ptr(davg), S.LOSS_WEIGHT, L.ptr(loss.t), L.ptr(grad.t), L.ptr(ws.t), wsb, L.stream_ptr(dp)),
        "jdet_smooth_l1_loss_level")
    _done([loss, grad, ws], [loss, grad])
    _equal(ws.t, partial, "partial sums")
    _equal(loss.t, S.level_scale(total, S.AVG, S.LOSS_WEIGHT), "loss")


# ---- (b) the channel-quad tree -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("C,P", S.BIAS_SHAPES)
def test_bias_act_backward_sum_order(dev, C, P, relu):
    """C 64: 1024-thread workgroups; C 1536: 384-thread workgroups; 256 partial rows both"""
    from jdet_amd import _lib as L
    dy, y, grad_bias, part = S.bias_case(C, P, relu)
    ddy, dy_ = _d(dy, dev), _d(y, dev)
    wsb = L.lib().jdet_frozen_bn_act_backward_workspace(P, C)
    pre = _out("grad_pre", (P, C), dev) if relu else None
    gb, ws = _out("grad_bias", (C,), dev), _out("ws", (wsb // 4,), dev)
    L.check(L.lib().jdet_bias_act_backward(L.ptr(ddy), L.ptr(dy_) if relu else None, P, C, relu,
                                           L.ptr(pre.t) if relu else None, L.ptr(gb.t), L.ptr(ws.t), wsb,
                                           L.stream_ptr(ddy)), "jdet_bias_act_backward")
    _done([b for b in (pre, gb, ws) if b is not None], [gb] + ([pre] if relu else []))
    got = ws.t.view(-1, 2, C)[:part.shape[0], 0]
    _equal(got, part, "partial rows")
    _equal(gb.t, grad_bias, "grad_bias")


@pytest.mark.parametrize("C,P", S.CHANNEL_SUM_SHAPES)
def test_channel_sum_order(dev, C, P):
    """one workgroup; 21 workgroups of 255 threads with the four-accumulator body and its tail; the 256-workgroup cap"""
    from jdet_amd import _lib as L
    x, sums, part = S.channel_sum_case(C, P)
    dx = _d(x, dev)
    wsb = L.lib().jdet_channel_sum_workspace(P, C)
    assert wsb == 4 * part.shape[0] * 2 * C
    out, ws = _out("sums", (C,), dev), _out("ws", (wsb // 4,), dev)
    L.check(L.lib().jdet_channel_sum(L.ptr(dx), P, C, L.ptr(out.t), L.ptr(ws.t), wsb, L.stream_ptr(dx)), "jdet_channel_sum")
    _done([out, ws], [out])
    _equal(ws.t.view(-1, 2, C)[:, 0], part, "partial rows")
    _equal(out.t, sums, "sums")


@pytest.mark.parametrize("C,P", S.BN_SHAPES)
def test_frozen_bn_act_backward_sum_order(dev, C, P):
    """mean 0, var 1, eps 0: grad_bias = sum g, grad_weight = sum g x.  C 64: 1024-thread workgroups, 256 partial rows;
    C 1536: 384-thread workgroups, 512 partial rows and the second stage's tail loop"""
    from jdet_amd import _lib as L
    dy, y, x, grad_bias, grad_weight, rows = S.frozen_bn_case(C, P)
    ddy, dy_, dx_ = _d(dy, dev), _d(y, dev), _d(x, dev)
    one, zero = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    wsb = L.lib().jdet_frozen_bn_act_backward_workspace(P, C)
    assert wsb >= 4 * rows * 2 * C
    gx, gw, gb, ws = _out("dx", (P, C), dev), _out("dgamma", (C,), dev), _out("dbeta", (C,), dev), _out("ws", (wsb // 4,), dev)
    L.check(L.lib().jdet_frozen_bn_act_backward(
        L.ptr(ddy), L.ptr(dy_), L.ptr(dx_), P, C, L.ptr(one), L.ptr(zero), L.ptr(zero), L.ptr(one), 0.0, 1, L.ptr(gx.t),
        None, L.ptr(gw.t), L.ptr(gb.t), L.ptr(ws.t), wsb, L.stream_ptr(ddy)), "jdet_frozen_bn_act_backward")
    _done([gx, gw, gb, ws], [gx, gw, gb])
    _equal(gx.t, S.masked(dy, y), "dx")                  # a = 1: the masked gradient itself
    _equal(gb.t, grad_bias, "grad_bias")
    _equal(gw.t, grad_weight, "grad_weight")


# ---- (c) jdet_bn_sums_finish ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("njobs", [1, 4])
@pytest.mark.parametrize("C", S.FINISH_CS)
@pytest.mark.parametrize("rows", S.FINISH_ROWS)
def test_bn_sums_finish_order(dev, rows, C, njobs):
    """synthetic partial rows on both sides of every loop bound; one job, and four in one launch (the others with the
    next row counts and the other channel count); gamma given and NULL in turn"""
    from jdet_amd import _lib as L
    jobs, keep = [], []
    for j in range(njobs):
        r = S.FINISH_ROWS[(S.FINISH_ROWS.index(rows) + j) % len(S.FINISH_ROWS)]
        c = C if j % 2 == 0 else S.FINISH_CS[1 - S.FINISH_CS.index(C)]
        part, gamma, grad_beta, grad_gamma, grad_gamma_plain = S.finish_case(r, c, j)
        with_gamma = (rows + j) % 2 == 0
        pin = G.Buf("partial", "in", part.shape, torch.float32, dev, G.QNAN_WORD, payload=part)
        dgam = _d(gamma, dev) if with_gamma else None
        gg, gb = _out("grad_gamma", (c,), dev), _out("grad_beta", (c,), dev)
        jobs.append(L.BnSumsJob(partial=pin.raw.data_ptr() + G.GUARD, rows=r, C=c, gamma=L.ptr(dgam) if with_gamma else None,
                                grad_gamma=L.ptr(gg.t), grad_beta=L.ptr(gb.t)))
        keep.append((pin, dgam, gg, gb, grad_beta, grad_gamma if with_gamma else grad_gamma_plain, r, c))
    arr = (L.BnSumsJob * njobs)(*jobs)
    L.check(L.lib().jdet_bn_sums_finish(arr, njobs, L.stream_ptr(keep[0][0].raw)), "jdet_bn_sums_finish")
    _done([b for k in keep for b in (k[0], k[2], k[3])], [b for k in keep for b in k[2:4]])
    for pin, _, gg, gb, grad_beta, grad_gamma, r, c in keep:
        pin.check_input()
        _equal(gb.t, grad_beta, "grad_beta (rows %d, C %d)" % (r, c))
        _equal(gg.t, grad_gamma, "grad_gamma (rows %d, C %d)" % (r, c))
