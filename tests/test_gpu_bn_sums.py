"""GPU: the per-channel sum kernels of csrc/frozen_bn.hip at CAPPED grids against the float64 restatements of
tests/bn_sums_ref.py (held to float64 autograd by tests/test_bn_sums_cpu.py), through the C ABI.

Every entry runs at the smallest sizes that reach its grid cap, several grid-stride iterations per thread (unrolled body
and scalar tail: P is ragged throughout), and its full count of partial rows, on two input families:

  lattice  small integers, gamma a power of two, 1 / sqrt(var) = 2: every product and every partial sum in any order is
           an integer below 2^24, so every output must EQUAL the float64 reference.  A lost, repeated or mis-channelled
           element fails however long the sum (the values of a channel carry a pattern of c % 7 and c // 4).
  normal   standard normal inputs, compared within the bounds derived in tests/bn_sums_ref.py: elementwise outputs
           k u sum|terms| with k the float32 roundings of the header's formula, per-channel sums (L + k) u sum|terms| with
           L = chain_length(P, rows), rows = the partial rows the call wrote (counted in the canary-filled workspace,
           which is allocated at exactly the size of the ABI's query between guard bands).

Each call runs twice and must give the same bits.  Outputs sit between guard bands and start as canaries.

The ReLU mask comes from the y array handed in; y carries exact 0.0, -0.0 and the smallest positive subnormal at known
positions under a non-zero gradient.  The gradient is zero at both zeros.  For the subnormal the expectation is what
`y > 0` answers on the device for a float32 tensor holding it, outside the library (fixture `subnormal_positive`).
Measured on an MI355X: True -- the comparison does not flush float32 denormals, and the kernels pass the gradient
through at the subnormal like the framework's threshold backward does.

Partial rows written on an MI355X (workspace query in rows / rows written):
  frozen_bn_act_backward  C 64 P 83 333: 512 / 256   C 256 P 20 011: 512 / 256   C 2048 P 2 605: 512 / 256
                          C 1536 P 2 605: 512 / 512 (the second stage's b >= 256 tail)
  bias_act_backward       C 64 P 83 333: 512 / 256   C 1536 P 2 605: 512 / 256
  bn_act_backward_from_output  C 64, 256, 2048: 256 = jdet_bn_act_backward_from_output_rows"""
import functools

import numpy as np
import pytest
import torch

from tests import bn_sums_ref as R
from tests import guarded as G

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
CANARY_I32 = G.CANARY_WORD - (1 << 32) if G.CANARY_WORD >= (1 << 31) else G.CANARY_WORD


@pytest.fixture(scope="module")
def subnormal_positive(dev):
    """what `y > 0` answers on the device for the smallest positive float32 subnormal, measured outside the library"""
    y = torch.tensor([float(R.SUBNORMAL), 0.0, -0.0, 1.0], dtype=torch.float32)
    assert y[0].item() != 0.0 and (y.view(torch.int32)[0].item() == 1)
    got = (y.to(dev) > 0).cpu().tolist()
    assert got[1:] == [False, False, True]
    print("device: (smallest positive subnormal > 0) is", got[0])
    return bool(got[0])


@functools.lru_cache(maxsize=2)
def _inputs(family, P, C, dev):
    t = (R.lattice_inputs if family == "lattice" else R.normal_inputs)(P, C)
    t["d"] = {k: torch.from_numpy(t[k]).to(dev) for k in ("dy", "x", "y", "residual", "identity", "own_output")}
    t["dp"] = [torch.from_numpy(p).to(dev) for p in t["params"][:4]]
    return t


def _out(name, shape, dev):
    return G.Buf(name, "out", shape, torch.float32, dev, G.CANARY_WORD, payload_word=G.CANARY_WORD)


def _rows_written(ws, width):
    """rows of a canary-filled [rows][width] workspace that the call wrote anything into, which must be the leading ones"""
    if ws.t.numel() == 0:
        return 0
    touched = (ws.t.view(torch.int32).view(-1, width) != CANARY_I32).any(1).cpu().numpy()
    n = int(touched.sum())
    assert touched[:n].all(), "the written partial rows are not the leading ones"
    return n


def _finish(bufs):
    torch.cuda.synchronize()
    for b in bufs:
        b.check_guards()


def _np(t):
    return t.detach().cpu().numpy()


def _check(got, ref, bound, what):
    """|got - ref| <= bound element-wise (bound 0: equality); prints the largest error as a fraction of its bound"""
    g = _np(got).astype(F64).reshape(ref.shape)
    err = np.abs(g - ref)
    bound = np.broadcast_to(np.asarray(bound, F64), ref.shape)
    bad = ~(err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, 0.0)
    print("  %-12s max |err| %.3e, %.3g of its bound at most%s" % (what, float(err.max()) if err.size else 0.0,
                                                                  float(frac.max()) if err.size else 0.0,
                                                                  " (exact)" if not np.any(bound) else ""))
    if bad.any():
        k = np.unravel_index(int(np.flatnonzero(bad.reshape(-1))[0]), ref.shape)
        raise AssertionError("%s: %d of %d elements beyond their bound, first at %r: got %r, reference %r, bound %.3e"
                             % (what, int(bad.sum()), ref.size, k, float(g[k]), float(ref[k]), float(bound[k])))


def _same(a, b, what):
    for k in a:
        if a[k] is not None:
            assert G.same_bits(a[k].t, b[k].t), "%s: two calls differ in '%s'" % (what, k)


def _planted_gradients(t, g, relu, subnormal_positive, scale=None):
    """the masked gradient at the planted positions: zero at 0.0 and -0.0, and what the device's own `y > 0` says at
    the subnormal"""
    g = _np(g)
    for kind, (r, c) in t["planted"].items():
        want = t["dy"][r, c] * (scale[c] if scale is not None else 1.0)
        if relu and (kind != "subnormal" or not subnormal_positive):
            want = np.zeros_like(want)
        assert (g[r, c] == want).all(), "gradient at the planted %s: %r, expected %r" % (kind, g[r, c], want)


# ---- jdet_frozen_bn_act_backward ---------------------------------------------------------------------------------------
BWD_X = [(64, 83333, 1, 1, 1), (64, 83333, 1, 1, 0), (2048, 2605, 1, 1, 1), (1536, 2605, 1, 1, 1)] + \
        [(256, 20011, relu, res, aff) for relu in (1, 0) for res in (1, 0) for aff in (1, 0)]


@pytest.mark.parametrize("family", ["lattice", "normal"])
@pytest.mark.parametrize("C,P,relu,res,affine", BWD_X)
def test_frozen_bn_act_backward(dev, subnormal_positive, C, P, relu, res, affine, family):
    """64 x 83 333: n4 = 5.09 strides of 256 x 1024 threads: the two-deep body runs more than twice, then the tail, 256
    partial rows; without the affine gradient the 512 x 256 grid.  2048: C/4 = 512 in 1024-thread workgroups.  1536:
    384-thread workgroups and 512 partial rows.  256 x 20 011: every template instance at a capped grid."""
    from jdet_amd import _lib as L
    t = _inputs(family, P, C, str(dev))
    d, dp, eps = t["d"], t["dp"], float(t["params"][4])
    wsb = L.lib().jdet_frozen_bn_act_backward_workspace(P, C)
    assert wsb % (8 * C) == 0 and wsb > 0

    def call():
        o = {"dx": _out("dx", (P, C), dev), "dres": _out("dres", (P, C), dev) if res else None,
             "dgamma": _out("dgamma", (C,), dev) if affine else None, "dbeta": _out("dbeta", (C,), dev) if affine else None,
             "ws": _out("ws", (wsb // 4,), dev) if affine else None}
        p = lambda k: L.ptr(o[k].t) if o[k] is not None else None
        L.check(L.lib().jdet_frozen_bn_act_backward(
            L.ptr(d["dy"]), L.ptr(d["y"]) if relu else None, L.ptr(d["x"]) if affine else None, P, C, L.ptr(dp[0]),
            L.ptr(dp[1]), L.ptr(dp[2]), L.ptr(dp[3]), eps, relu, p("dx"), p("dres"), p("dgamma"), p("dbeta"), p("ws"),
            wsb if affine else 0, L.stream_ptr(d["dy"])), "jdet_frozen_bn_act_backward")
        live = [b for b in o.values() if b is not None]
        _finish(live)
        for b in live:
            if b.name != "ws":
                b.check_written()
        return o

    a, b = call(), call()
    _same(a, b, "frozen_bn_act_backward")
    ref = R.backward_from_x(t["dy"], t["y"], t["x"] if affine else None, *t["params"], relu, subnormal_positive)
    exact = family == "lattice"
    print("frozen_bn_act_backward C %d P %d relu %d res %d affine %d %s" % (C, P, relu, res, affine, family))
    _check(a["dx"].t, ref["dx"], 0.0 if exact else R.K_DX * R.U * ref["dx_mag"], "dx")
    if res:
        _check(a["dres"].t, ref["dres"], 0.0, "dres")
        _planted_gradients(t, a["dres"].t, relu, subnormal_positive)
    if exact:
        _planted_gradients(t, a["dx"].t, relu, subnormal_positive, scale=2.0 * t["params"][0])
    if affine:
        rows = _rows_written(a["ws"], 2 * C)
        chain = R.chain_length(P, rows)
        print("  workspace query %d rows, written %d, chain bound %d" % (wsb // (8 * C), rows, chain))
        assert 1 <= rows <= wsb // (8 * C)
        _check(a["dbeta"].t, ref["dbeta"], 0.0 if exact else chain * R.U * ref["dbeta_mag"], "dbeta")
        _check(a["dgamma"].t, ref["dgamma"], 0.0 if exact else (chain + R.K_GXHAT) * R.U * ref["dgamma_mag"], "dgamma")
        if exact:       # every partial row is summed: the written rows add up to the result
            part = _np(a["ws"].t)[:rows * 2 * C].reshape(rows, 2, C)
            s0, s1, _, _ = R.column_sums(part)
            assert (s0 == ref["dbeta"]).all() and (s1 == ref["dgamma"]).all()


# ---- jdet_frozen_bn_act_forward ----------------------------------------------------------------------------------------
FWD_FLAGS = [(1, 1, 0), (1, 0, 1), (0, 1, 1), (0, 0, 0)]       # relu, residual, weight / bias NULL


@pytest.mark.parametrize("family", ["lattice", "normal"])
@pytest.mark.parametrize("relu,res,null_wb", FWD_FLAGS)
@pytest.mark.parametrize("C,P", [(1536, 2605), (2048, 2605), (8, 333)])
def test_frozen_bn_act_forward(dev, C, P, relu, res, null_wb, family):
    """workgroup = one row of quads (C/4 = 384, 512) and the smallest channel count; NULL weight / bias = 1 / 0"""
    from jdet_amd import _lib as L
    t = _inputs(family, P, C, str(dev))
    d, dp, eps = t["d"], t["dp"], float(t["params"][4])
    w, b, m, v, _ = t["params"]
    if null_wb:
        w = b = None

    def call():
        y = _out("y", (P, C), dev)
        L.check(L.lib().jdet_frozen_bn_act_forward(
            L.ptr(d["x"]), L.ptr(d["residual"]) if res else None, P, C, None if null_wb else L.ptr(dp[0]),
            None if null_wb else L.ptr(dp[1]), L.ptr(dp[2]), L.ptr(dp[3]), eps, relu, L.ptr(y.t), L.stream_ptr(d["x"])),
            "jdet_frozen_bn_act_forward")
        _finish([y])
        y.check_written()
        return {"y": y}

    a, b2 = call(), call()
    _same(a, b2, "frozen_bn_act_forward")
    ref, mag = R.forward(t["x"], t["residual"] if res else None, w, b, m, v, eps, relu)
    print("frozen_bn_act_forward C %d P %d relu %d res %d null_wb %d %s" % (C, P, relu, res, null_wb, family))
    _check(a["y"].t, ref, 0.0 if family == "lattice" else R.K_FWD * R.U * mag, "y")


def _forward_torch64(x, res, params, relu, dev):
    """R.forward restated on the device in float64 (the big case's arrays stay there): (y, sum of |terms|)"""
    w, b, m, v, eps = params
    w, b, m, v = (torch.from_numpy(p).to(dev).double() for p in (w, b, m, v))
    a = w * (1.0 / torch.sqrt(v + float(F32(eps))))
    x64 = x.double()
    y = (x64 - m) * a + b + res.double()
    mag = (x64.abs() + m.abs()) * a.abs() + b.abs() + res.double().abs()
    return (y.clamp_min(0.0) if relu else y), mag


def test_frozen_bn_act_forward_past_its_cap(dev):
    """C 64, P 460 003, relu + residual: n4 = 7.02 strides of 4096 x 256 threads: the four-deep body runs twice (i = g
    and g + 4 s: g + 7 s < n4 only for the first threads), then the tail.  Both families; float64 reference computed on the device
    (118 MB per float32 tensor), and held to the numpy restatement on the first and last rows."""
    from jdet_amd import _lib as L
    C, P = 64, 460003
    assert 7 * 4096 * 256 < P * (C // 4) < 8 * 4096 * 256
    gen = torch.Generator(device=dev).manual_seed(11)
    for family in ("lattice", "normal"):
        if family == "lattice":
            params = R.lattice_params(C)
            x = torch.randint(-3, 4, (P, C), device=dev, generator=gen).float()
            res = torch.randint(-3, 4, (P, C), device=dev, generator=gen).float()
        else:
            params = R.normal_params(C)
            x = torch.randn((P, C), device=dev, generator=gen)
            res = torch.randn((P, C), device=dev, generator=gen)
        dp = [torch.from_numpy(p).to(dev) for p in params[:4]]
        ys = []
        for _ in range(2):
            y = _out("y", (P, C), dev)
            L.check(L.lib().jdet_frozen_bn_act_forward(L.ptr(x), L.ptr(res), P, C, L.ptr(dp[0]), L.ptr(dp[1]), L.ptr(dp[2]),
                                                       L.ptr(dp[3]), float(params[4]), 1, L.ptr(y.t), L.stream_ptr(x)),
                    "jdet_frozen_bn_act_forward")
            _finish([y])
            y.check_written()
            ys.append(y)
        assert G.same_bits(ys[0].t, ys[1].t)
        ref, mag = _forward_torch64(x, res, params, True, dev)
        for sl in (slice(0, 500), slice(P - 500, P)):
            r2, m2 = R.forward(_np(x[sl]), _np(res[sl]), *params, True)
            assert np.abs(_np(ref[sl]) - r2).max() <= 1e-12 and np.abs(_np(mag[sl]) - m2).max() <= 1e-12
        err = (ys[0].t.double() - ref).abs()
        bound = mag * (0.0 if family == "lattice" else R.K_FWD * R.U)
        bad = ~(err <= bound)
        print("frozen_bn_act_forward C %d P %d %s: max |err| %.3e, %d beyond the bound" % (C, P, family, float(err.max()),
                                                                                         int(bad.sum())))
        assert not bool(bad.any()), "first bad flat index %d" % int(bad.view(-1).nonzero()[0])
        del ref, mag, err, bound, bad, ys, x, res


# ---- jdet_bias_act_backward --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["lattice", "normal"])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("C,P", [(64, 83333), (1536, 2605)])
def test_bias_act_backward(dev, subnormal_positive, C, P, relu, family):
    """capped grids; without ReLU grad_pre and y are NULL and the gradient is only summed"""
    from jdet_amd import _lib as L
    t = _inputs(family, P, C, str(dev))
    d = t["d"]
    wsb = L.lib().jdet_frozen_bn_act_backward_workspace(P, C)

    def call():
        o = {"grad_pre": _out("grad_pre", (P, C), dev) if relu else None, "grad_bias": _out("grad_bias", (C,), dev),
             "ws": _out("ws", (wsb // 4,), dev)}
        L.check(L.lib().jdet_bias_act_backward(L.ptr(d["dy"]), L.ptr(d["y"]) if relu else None, P, C, relu,
                                               L.ptr(o["grad_pre"].t) if relu else None, L.ptr(o["grad_bias"].t),
                                               L.ptr(o["ws"].t), wsb, L.stream_ptr(d["dy"])), "jdet_bias_act_backward")
        live = [b for b in o.values() if b is not None]
        _finish(live)
        for b in live:
            if b.name != "ws":
                b.check_written()
        return o

    a, b = call(), call()
    _same(a, b, "bias_act_backward")
    ref = R.bias_act_backward(t["dy"], t["y"], relu, subnormal_positive)
    rows = _rows_written(a["ws"], 2 * C)
    chain = R.chain_length(P, rows)
    print("bias_act_backward C %d P %d relu %d %s: workspace query %d rows, written %d, chain bound %d"
          % (C, P, relu, family, wsb // (8 * C), rows, chain))
    assert 1 <= rows <= wsb // (8 * C)
    if relu:
        _check(a["grad_pre"].t, ref["grad_pre"], 0.0, "grad_pre")
        _planted_gradients(t, a["grad_pre"].t, relu, subnormal_positive)
    _check(a["grad_bias"].t, ref["grad_bias"], 0.0 if family == "lattice" else chain * R.U * ref["grad_bias_mag"],
           "grad_bias")


def test_bias_act_backward_of_no_rows_zeroes_the_bias_gradient(dev):
    from jdet_amd import _lib as L
    for C in (64, 1536):
        gb = _out("grad_bias", (C,), dev)
        L.check(L.lib().jdet_bias_act_backward(None, None, 0, C, 1, None, L.ptr(gb.t), None, 0, L.stream_ptr(gb.t)),
                "jdet_bias_act_backward")
        _finish([gb])
        assert (gb.t == 0).all()


# ---- jdet_bn_act_backward_from_output + jdet_bn_sums_finish ---------------------------------------------------------------
def _job(L, partial_ptr, rows, C, gamma, grad_gamma, grad_beta):
    p = lambda x: L.ptr(x) if x is not None else None
    return L.BnSumsJob(partial=partial_ptr, rows=rows, C=C, gamma=p(gamma), grad_gamma=p(grad_gamma), grad_beta=p(grad_beta))


def _sums_finish(L, jobs, t):
    arr = (L.BnSumsJob * len(jobs))(*jobs)
    L.check(L.lib().jdet_bn_sums_finish(arr, len(jobs), L.stream_ptr(t)), "jdet_bn_sums_finish")


@pytest.mark.parametrize("family", ["lattice", "normal"])
@pytest.mark.parametrize("form", ["plain", "identity", "own_output", "no_sums"])
@pytest.mark.parametrize("C,P", [(64, 83333), (256, 20011), (2048, 2605)])
def test_bn_act_backward_from_output(dev, subnormal_positive, C, P, form, family):
    """t = y - beta | y - identity - beta | own_output - beta, the sums finished by jdet_bn_sums_finish (its division by
    gamma); sums NULL: grad_c alone, whatever identity is passed"""
    from jdet_amd import _lib as L
    t = _inputs(family, P, C, str(dev))
    d, dp, eps = t["d"], t["dp"], float(t["params"][4])
    rows = L.lib().jdet_bn_act_backward_from_output_rows(P, C)
    assert rows >= 1
    idn = d["identity"] if form in ("identity", "no_sums") else None
    own = d["own_output"] if form == "own_output" else None
    sums_on = form != "no_sums"

    def call():
        o = {"dc": _out("dc", (P, C), dev), "sums": _out("sums", (rows, 2, C), dev) if sums_on else None,
             "dgamma": _out("dgamma", (C,), dev) if sums_on else None, "dbeta": _out("dbeta", (C,), dev) if sums_on else None}
        L.check(L.lib().jdet_bn_act_backward_from_output(
            L.ptr(d["dy"]), L.ptr(d["y"]), L.ptr(idn) if idn is not None else None, L.ptr(own) if own is not None else None,
            P, C, L.ptr(dp[0]), L.ptr(dp[1]), L.ptr(dp[2]), L.ptr(dp[3]), eps, L.ptr(o["dc"].t),
            L.ptr(o["sums"].t) if sums_on else None, rows * 2 * C * 4 if sums_on else 0, L.stream_ptr(d["dy"])),
            "jdet_bn_act_backward_from_output")
        if sums_on:
            _sums_finish(L, [_job(L, L.ptr(o["sums"].t), rows, C, dp[0], o["dgamma"].t, o["dbeta"].t)], d["dy"])
        live = [b for b in o.values() if b is not None]
        _finish(live)
        for b in live:
            b.check_written()          # the sums too: every row the query names is written
        return o

    a, b = call(), call()
    _same(a, b, "bn_act_backward_from_output")
    ref = R.backward_from_output(t["dy"], t["y"], t["identity"] if form == "identity" else None,
                                 t["own_output"] if form == "own_output" else None, *t["params"], subnormal_positive)
    exact = family == "lattice"
    chain = R.chain_length(P, rows)
    print("bn_act_backward_from_output C %d P %d %s %s: %d partial rows, chain bound %d" % (C, P, form, family, rows, chain))
    _check(a["dc"].t, ref["dc"], 0.0 if exact else R.K_DX * R.U * ref["dc_mag"], "dc")
    if exact:
        _planted_gradients(t, a["dc"].t, 1, subnormal_positive, scale=2.0 * t["params"][0])
    if sums_on:
        part = _np(a["sums"].t)
        s0, s1, _, _ = R.column_sums(part)
        _check(torch.from_numpy(s0), ref["s0"], 0.0 if exact else chain * R.U * ref["s0_mag"], "sum g")
        _check(torch.from_numpy(s1), ref["s1"], 0.0 if exact else (chain + R.K_GT) * R.U * ref["s1_mag"], "sum g t")
        _check(a["dbeta"].t, ref["dbeta"], 0.0 if exact else chain * R.U * ref["s0_mag"], "dbeta")
        g = np.abs(ref["gamma"])
        _check(a["dgamma"].t, ref["dgamma"],
               0.0 if exact else (chain + R.K_GT) * R.U * ref["s1_mag"] / g + R.K_DIV * R.U * np.abs(ref["dgamma"]), "dgamma")


FINISH_ROWS = [0, 1, 31, 32, 97, 128, 129, 256, 512]
FINISH_CALLS = [(4, i) for i in range(len(FINISH_ROWS))] + [(1, 6), (2, 6), (3, 6)]       # (jobs, index of job 0's rows)


@pytest.mark.parametrize("family", ["lattice", "normal"])
@pytest.mark.parametrize("njobs,first", FINISH_CALLS)
def test_bn_sums_finish_on_synthetic_partials(dev, njobs, first, family):
    """1 to 4 jobs of C = 40, 100, 4, 64 in one call (first_block = 0, 2, 6, 7: a workgroup finds its job and its 32
    channels; C no multiple of 32), row counts from both sides of every loop bound of a 32-row-group sum (four rows in
    flight from 97 on), gamma / grad_gamma / grad_beta NULL in turn, rows = 0 gives zeros"""
    from jdet_amd import _lib as L
    rng = np.random.default_rng(100 * njobs + first)
    Cs = [40, 100, 4, 64][:njobs] if njobs > 1 else [100]
    jobs, keep = [], []
    for j, C in enumerate(Cs):
        rows = FINISH_ROWS[(first + 3 * j) % len(FINISH_ROWS)]
        if family == "lattice":
            part = (rng.integers(-1000, 1001, (rows, 2, C)) * R.channel_pattern(C)).astype(F32)
            gamma = R.lattice_params(C)[0]
        else:
            part = (100.0 * rng.standard_normal((rows, 2, C))).astype(F32)
            gamma = R.normal_params(C, seed=j)[0]
        null = (first + j) % 4                      # 0: nothing NULL, 1: gamma, 2: grad_gamma, 3: grad_beta
        pin = G.Buf("partial", "in", part.shape, torch.float32, dev, G.QNAN_WORD, payload=part)
        dgam = torch.from_numpy(gamma).to(dev) if null != 1 else None
        gg = _out("grad_gamma", (C,), dev) if null != 2 else None
        gb = _out("grad_beta", (C,), dev) if null != 3 else None
        # rows = 0: a valid pointer to no rows (the NaN guard behind the empty payload)
        jobs.append(_job(L, pin.raw.data_ptr() + G.GUARD, rows, C, dgam, gg.t if gg else None, gb.t if gb else None))
        keep.append((part, gamma if null != 1 else None, pin, gg, gb, rows, C, dgam))      # dgam: kept alive for the call
    first_pass = None
    for _ in range(2):
        for k in keep:
            for o in k[3:5]:
                if o is not None:
                    o.t.view(torch.int32).fill_(CANARY_I32)
        _sums_finish(L, jobs, keep[0][2].raw)
        _finish([b for k in keep for b in k[2:5] if b is not None])
        got = [tuple(None if o is None else o.t.clone() for o in k[3:5]) for k in keep]
        if first_pass is None:
            first_pass = got
    for (part, gamma, pin, gg, gb, rows, C, _), one, two in zip(keep, first_pass, got):
        pin.check_input()
        s0, s1, m0, m1 = R.column_sums(part, gamma)
        chain = R.finish_chain_length(rows)
        exact = family == "lattice"
        assert not exact or max(m0.max(), np.abs(part[:, 1].astype(F64)).sum(0).max()) < R.LATTICE_LIMIT
        print("bn_sums_finish job C %d rows %d gamma %s" % (C, rows, "NULL" if gamma is None else "given"))
        for name, o, x, y, ref, mag in (("grad_gamma", gg, one[0], two[0], s1, m1), ("grad_beta", gb, one[1], two[1], s0, m0)):
            if o is None:
                continue
            o.check_written()
            assert G.same_bits(x, y), name
            bound = 0.0 if exact else chain * R.U * mag + (R.K_DIV * R.U * np.abs(ref) if name == "grad_gamma" else 0.0)
            _check(x, ref, bound, name)
            if rows == 0:
                assert (x == 0).all()


def test_bn_sums_finish_with_a_zero_gamma_is_not_finite(dev):
    """with gamma = 0 the normalised input is not recoverable from the activation; a silent zero would be a
    wrong gradient, so a non-zero second sum over a zero gamma must come out NON-FINITE -- never zero"""
    from jdet_amd import _lib as L
    rows, C = 5, 8
    part = np.ones((rows, 2, C), F32)
    part[:, 1, 6] = -1.0
    gamma = np.array([1, 2, 0, 1, -1, 1, 0, 0.5], F32)
    dpart, dgamma = torch.from_numpy(part).to(dev), torch.from_numpy(gamma).to(dev)
    gg, gb = _out("grad_gamma", (C,), dev), _out("grad_beta", (C,), dev)
    _sums_finish(L, [_job(L, L.ptr(dpart), rows, C, dgamma, gg.t, gb.t)], dpart)
    _finish([gg, gb])
    g = _np(gg.t)
    assert not np.isfinite(g[2]) and not np.isfinite(g[6]) and g[2] != 0 and g[6] != 0
    ok = gamma != 0
    assert (g[ok] == part[:, 1].sum(0)[ok] / gamma[ok]).all() and (_np(gb.t) == rows).all()
