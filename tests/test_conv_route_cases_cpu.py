"""CPU: the case table of the fused conv module's routing tests (tests/conv_route_cases.py) reaches every leaf of the
four label axes, every switch of case 23 moves its case to another leaf, the EXACT tier is exact (sums of absolute terms
below 2^24, the fp32 host convolution equal to the float64 reference), the TOLERANCE tier zeroes at most 0.5 % of a
case's outputs, and the reference of a shared case is the sum of its per-use references."""
import numpy as np
import pytest
import torch

from tests import conv_route_cases as K

LIMIT = float(2 ** 24)


def _ids(cases):
    return [c.name for c in cases]


def test_every_leaf_of_the_four_axes_is_reached():
    seen = {"forward": {}, "bias": {}, "dgrad": {}, "wgrad": {}}
    for c in K.CASES:
        for lab in K.labels(c):
            for axis in seen:
                seen[axis].setdefault(getattr(lab, axis), c.name)
    for axis, values in (("forward", K.FORWARD), ("bias", K.BIAS), ("dgrad", K.DGRAD), ("wgrad", K.WGRAD)):
        for v in values:
            print("conv_routes | leaf | %s | %s | first reached by case %s" % (axis, v, seen[axis].get(v)))
        assert set(seen[axis]) == set(values), "%s: reached %r of %r" % (axis, sorted(seen[axis]), values)


def test_the_table_states_what_the_issue_states():
    lab = lambda n, u=0: (lambda l: (l.forward, l.bias, l.dgrad, l.wgrad))(K.label(K.BY_NAME[n], u))
    assert lab("1") == ("igemm", "bias_act", "library", "own")
    assert lab("2/rows13") == lab("2/dense") == ("igemm", "bias_act", "rows", "rows")
    assert lab("3/x-frozen")[2:] == ("none", "rows") and lab("3/w-frozen")[2:] == ("rows", "none")
    assert lab("4/relu")[1] == "framework" and lab("4/linear")[1] == "channel_sum"
    assert lab("5") == ("igemm", "channel_sum", "library", "library")
    assert lab("6/c15") == lab("6/c5") == ("library", "channel_sum", "library", "library")
    assert K.label(K.BY_NAME["6/c15"]).function and not K.label(K.BY_NAME["7"]).function
    assert lab("8/no-bias")[1] == lab("8/bias-frozen")[1] == "none"
    assert lab("9") == ("bf16x3", "bias_act", "library", "own")
    assert lab("10") == ("igemm", "bias_act", "bf16x3", "own")
    assert lab("11") == ("gemm1x1", "bias_act", "gemm1x1", "gemm1x1")
    assert lab("12") == ("library", "bias_act", "gemm1x1", "gemm1x1")
    assert lab("13") == ("gemm1x1", "bias_act", "gemm1x1", "library")
    for n in ("14/x-nchw", "14/c32", "14/no-bias", "15/stride2", "15/dil2", "15/groups2", "15/cin40"):
        assert lab(n)[0] == "library" and lab(n)[2:] == ("library", "library") and not K.label(K.BY_NAME[n]).k1
        assert lab(n)[1] == ("none" if n == "14/no-bias" else "bias_act")
    assert lab("17") == lab("18") == lab("1")
    assert [lab("20", u)[3] for u in range(3)] == ["own", "rows", "own"]
    assert lab("22/n0") == ("library", "framework", "library", "library")
    # the incoming gradient takes its three forms, the expanded scalar at cases 1, 6 and 11
    forms = {f for c in K.CASES for f in c.grad}
    assert {"cl", "nchw", "scalar", "rows13"} <= forms
    assert all(K.BY_NAME[n].grad == ("scalar",) for n in ("1/scalar", "6/c15/scalar", "11/scalar"))


@pytest.mark.parametrize("name", _ids(K.SWITCH_CASES))
def test_every_switch_moves_its_case_to_another_leaf(name):
    c = K.BY_NAME[name]
    base = K.BY_NAME[c.data]
    key = lambda l: (l.forward, l.bias, l.dgrad, l.wgrad)
    assert key(K.label(c)) != key(K.label(base)), "%r leaves %s where it was" % (c.switches, base.name)
    same = {k: v for k, v in vars(c).items() if k not in ("name", "switches", "data", "reaches")}
    assert same == {k: v for k, v in vars(base).items() if k in same}, "the case shares the inputs of its base"


def test_the_switch_cases_cover_every_switch():
    assert {s for c in K.SWITCH_CASES for s in c.switches} == set(K.SWITCHES)


@pytest.mark.parametrize("name", _ids(K.CASES))
def test_exact_tier_is_exact(name):
    """sums of absolute terms of y and of every gradient below 2^24, and the fp32 host result equal to the float64 one"""
    c = K.BY_NAME[name]
    inp = K.inputs_of(c, "exact")
    for a in inp.x + inp.g + [inp.w] + ([inp.b] if c.bias else []):
        assert np.array_equal(a, np.round(a))
    mag = K.host_autograd(c, inp, magnitudes=True)
    ref = K.reference(c, "exact")
    f32 = K.host_autograd(c, inp, dtype=torch.float32)
    peak = {}
    for p in range(c.passes):
        for u in range(len(c.maps)):
            peak["y"] = max(peak.get("y", 0.0), float(mag.y[p][u].max()) if mag.y[p][u].size else 0.0)
            assert np.array_equal(f32.y[p][u], ref.y[p][u].astype(np.float32))
    for kind, m, a, b in (("grad_w", mag.grad_w, f32.grad_w, ref.grad_w), ("grad_b", mag.grad_b, f32.grad_b, ref.grad_b)):
        assert (m is None) == (b is None) == (not c.need[{"grad_w": 1, "grad_b": 2}[kind]])
        if b is not None:
            peak[kind] = float(m.max())
            assert np.array_equal(a, b.astype(np.float32)), kind
    for u in range(len(c.maps)):
        assert (ref.grad_x[u] is None) == (not c.need[0])
        if c.need[0] and ref.grad_x[u].size:
            peak["grad_x"] = max(peak.get("grad_x", 0.0), float(mag.grad_x[u].max()))
            assert np.array_equal(f32.grad_x[u], ref.grad_x[u].astype(np.float32))
    print("conv_routes | exact | %s | sums of absolute terms %s" % (name, {k: int(v) for k, v in peak.items()}))
    assert all(v < LIMIT for v in peak.values()), peak


@pytest.mark.parametrize("name", _ids(K.CASES))
def test_tolerance_tier_zeroes_few_outputs(name):
    c = K.BY_NAME[name]
    inp = K.inputs_of(c, "tolerance")
    print("conv_routes | tolerance | %s | gradient zeroed at %.2e of the outputs" % (name, inp.zeroed))
    assert inp.zeroed <= K.KEEP_CAP
    if not c.relu:
        assert inp.zeroed == 0
    exact = K.inputs_of(c, "exact")
    if K.zero_at_threshold(c):
        assert exact.zeroed <= K.KEEP_CAP
    else:
        assert exact.zeroed == 0


@pytest.mark.parametrize("tier", K.TIERS)
@pytest.mark.parametrize("name", _ids(K.SHARED_CASES))
def test_shared_reference_is_the_sum_of_its_uses(name, tier):
    c = K.BY_NAME[name]
    inp = K.inputs_of(c, tier)
    ref = K.reference(c, tier)
    parts = [K.host_autograd(c, inp, uses=[u]) for u in range(len(c.maps))]
    for u, part in enumerate(parts):
        assert np.array_equal(part.y[0][u], ref.y[0][u]) and np.array_equal(part.grad_x[u], ref.grad_x[u])
    for kind in ("grad_w", "grad_b"):
        total = sum(getattr(p, kind) for p in parts)
        whole = getattr(ref, kind)
        assert np.abs(total - whole).max() <= 1e-12 * np.abs(whole).max()
        if tier == "exact":
            assert np.array_equal(total, whole)
    assert min(np.abs(p.grad_w).max() for p in parts) > 0, "every use contributes"
