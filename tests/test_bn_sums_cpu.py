"""No GPU: the float64 restatements of tests/bn_sums_ref.py and their input families.

  * forward / backward-from-x / bias backward agree with float64 autograd of F.batch_norm(..., training=False)
    [+ residual] [+ relu] on the host (1e-12 of the largest value);
  * the three backward-from-the-output forms give the from-x form's dgamma / dbeta / dx when the activation handed in is
    the forward's own (y > 0 wherever the gradient counts, gamma != 0);
  * column_sums is the plain sum, / gamma;
  * lattice inputs: every value is an integer of magnitude <= 3 (parameters as the issue lists them), the planted
    0.0 / -0.0 / subnormal sit where `plant` says, and for every (C, P) the GPU tests run the per-channel sums of |terms|
    stay below 2^24 -- so every partial sum in any order is exact and the GPU comparison can be `==`;
  * the channel pattern tells apart the channels a thread could confuse."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_sums_ref as R

F32, F64 = np.float32, np.float64


def _t(a, grad=False):
    return None if a is None else torch.from_numpy(np.asarray(a, F64)).requires_grad_(grad)


def _autograd(x, res, params, relu, dy):
    w, b, m, v, eps = params
    eps = float(F32(eps))
    C = x.shape[1]
    tx, tr = _t(x, True), _t(res, res is not None)
    tw = _t(np.ones(C) if w is None else w, True)
    tb = _t(np.zeros(C) if b is None else b, True)
    y = F.batch_norm(tx, _t(m), _t(v), tw, tb, False, 0.0, eps)
    if tr is not None:
        y = y + tr
    if relu:
        y = F.relu(y)
    y.backward(_t(dy))
    return (y.detach().numpy(), tx.grad.numpy(), None if tr is None else tr.grad.numpy(), tw.grad.numpy(), tb.grad.numpy())


def _close(a, b, what):
    scale = max(1.0, float(np.abs(b).max()))
    assert float(np.abs(a - b).max()) <= 1e-12 * scale, what


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("null_wb", [True, False])
def test_reference_equals_float64_autograd(relu, with_res, null_wb):
    P, C = 257, 24
    t = R.normal_inputs(P, C, seed=5)
    w, b, m, v, eps = t["params"]
    if null_wb:
        w = b = None
    params = (w, b, m, v, eps)
    res = t["residual"] if with_res else None
    y64, mag = R.forward(t["x"], res, *params, relu)
    ya, dxa, dra, dwa, dba = _autograd(t["x"], res, params, relu, t["dy"])
    _close(y64, ya, "y")
    assert (mag >= np.abs(y64) - 1e-12).all()
    y32 = y64.astype(F32)                      # the activation the backward entries are handed
    assert not relu or ((y32 > 0) == (y64 > 0)).all()
    r = R.backward_from_x(t["dy"], y32, t["x"], *params, relu)
    _close(r["dx"], dxa, "dx")
    _close(r["dgamma"], dwa, "dgamma")
    _close(r["dbeta"], dba, "dbeta")
    if with_res:
        _close(r["dres"], dra, "dres")
    assert (r["dgamma_mag"] >= np.abs(r["dgamma"])).all() and (r["dbeta_mag"] >= np.abs(r["dbeta"])).all()
    # bias [+ ReLU]: batch_norm with unit statistics is x + bias
    bb = R.bias_act_backward(t["dy"], y32, relu)
    _close(bb["grad_pre"], r["dres"], "grad_pre")
    _close(bb["grad_bias"], dba, "grad_bias")


@pytest.mark.parametrize("form", ["plain", "identity", "own_output"])
def test_from_output_forms_equal_the_from_x_form(form):
    """where y > 0 the normalised input is recoverable from the activation, so every form gives the from-x form's sums
    (gamma != 0).  The entry reads FLOAT32 activations; to test the algebra and not that rounding, inputs and parameters
    sit on a 2^-10 grid with 1 / sqrt(var) = 2, so the forward's output is exact in float32."""
    P, C, q = 301, 16, 2.0 ** -10
    t = R.normal_inputs(P, C, seed=6)
    grid = lambda a: (np.round(a.astype(F64) / q) * q).astype(F32)
    gamma, beta, mean = (grid(p) for p in t["params"][:3])
    assert (gamma != 0).all()
    params = (gamma, beta, mean, np.full(C, 0.25, F32), 0.0)
    x = grid(t["x"])
    other = grid(t["identity"]) if form != "plain" else None
    bn64, _ = R.forward(x, None, *params, False)                   # this BatchNorm's own output
    pre = bn64 + (other.astype(F64) if other is not None else 0.0)
    y = np.maximum(pre, 0.0).astype(F32)
    assert (y.astype(F64) == np.maximum(pre, 0.0)).all() and (bn64.astype(F32).astype(F64) == bn64).all()
    ref = R.backward_from_x(t["dy"], y, x, *params, True)
    got = R.backward_from_output(t["dy"], y, other if form == "identity" else None,
                                 bn64.astype(F32) if form == "own_output" else None, *params)
    _close(got["dc"], ref["dx"], "dc")
    _close(got["dbeta"], ref["dbeta"], "dbeta")
    _close(got["dgamma"], ref["dgamma"], "dgamma")
    assert (got["s1_mag"] >= np.abs(got["s1"])).all()


def test_column_sums():
    rng = np.random.default_rng(0)
    part = rng.standard_normal((37, 2, 20)).astype(F32)
    gamma = rng.uniform(0.5, 2, 20).astype(F32)
    s0, s1, m0, m1 = R.column_sums(part, gamma)
    assert np.allclose(s0, part[:, 0].astype(F64).sum(0), rtol=0, atol=1e-12)
    assert np.allclose(s1 * gamma, part[:, 1].astype(F64).sum(0), rtol=1e-14, atol=1e-12)
    assert (m0 >= np.abs(s0)).all() and (m1 >= np.abs(s1)).all()
    z = R.column_sums(np.zeros((0, 2, 5), F32), np.ones(5, F32))
    assert all((a == 0).all() for a in z)
    # a zero gamma with a non-zero second sum is non-finite on purpose, never a silent zero
    _, g, _, _ = R.column_sums(np.ones((3, 2, 2), F32), np.array([0.0, 1.0], F32))
    assert not np.isfinite(g[0]) and g[1] == 3.0


@pytest.mark.parametrize("C,P", R.SUM_SHAPES)
def test_lattice_inputs_stay_exact(C, P):
    t = R.lattice_inputs(P, C)
    gamma, beta, mean, var, eps = t["params"]
    for k in ("dy", "x", "y", "residual", "identity", "own_output"):
        v = t[k].astype(F64)
        whole = v == np.round(v)
        if k == "y":
            r, c = t["planted"]["subnormal"]
            assert (t[k][r, c] == R.SUBNORMAL).all()
            whole[r, c] = True
        assert whole.all() and np.abs(v).max() <= 3, k
    assert set(np.unique(gamma)) <= {-2.0, -1.0, -0.5, 0.5, 1.0, 2.0} and len(np.unique(gamma)) == 6
    assert (beta == np.round(beta)).all() and (beta != 0).all() and (mean == np.round(mean)).all()
    assert (var == 0.25).all() and eps == 0.0
    _, _, _, invstd, _, _ = R.constants(C, *t["params"])
    assert (invstd == 2.0).all()
    r, c = t["planted"]["zero"]
    assert (t["y"][r, c] == 0).all() and not np.signbit(t["y"][r, c]).any()
    r, c = t["planted"]["negzero"]
    assert (t["y"][r, c] == 0).all() and np.signbit(t["y"][r, c]).all()
    for kind in t["planted"]:
        r, c = t["planted"][kind]
        assert (t["dy"][r, c] != 0).all() and P - 1 in r and 0 in r
    worst = R.lattice_sum_magnitudes(t)
    print("C %d P %d: largest sum of |terms| %.0f of %d" % (C, P, worst, R.LATTICE_LIMIT))
    assert worst < R.LATTICE_LIMIT
    # float32 sums in two different orders equal the float64 sum: the lattice is exact
    ref = R.backward_from_x(t["dy"], t["y"], t["x"], *t["params"], True)
    g = t["dy"] * (t["y"] > 0)
    term = g * ((t["x"] - mean) * F32(2.0))
    assert term.dtype == F32
    assert (np.add.reduce(term, 0, dtype=F32) == ref["dgamma"]).all()
    assert (np.add.reduce(term[::-1], 0, dtype=F32) == ref["dgamma"]).all()


def test_channel_pattern_separates_confusable_channels():
    for C in (8, 64, 256, 1536, 2048):
        pat = R.channel_pattern(C)
        gamma, beta, mean, _, _ = R.lattice_params(C)
        assert (pat != 0).all() and np.abs(pat).max() <= 3
        key = np.stack([pat, gamma, beta, mean], 1)
        c = np.arange(C - 4)
        assert (key[c] != key[c + 4]).any(1).mean() > 0.95          # the same lane of the next quad
        c = np.arange(C - 1)
        assert (key[c] != key[c + 1]).any(1).mean() > 0.95          # the next lane
        # a thread that changes quad between iterations mixes the sums of two quads: no two quads carry the same four keys
        if C >= 64:
            quads = key.reshape(C // 4, -1)
            assert len(np.unique(quads[:16], axis=0)) == 16


def test_chain_lengths():
    assert R.finish_chain_length(512) == 48 and R.finish_chain_length(1) == 33
    assert R.chain_length(83333, 256) == 326 + 1024 + 8 + 32
