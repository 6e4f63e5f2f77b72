"""CPU: the case table of tests/dcn_v2_cases.py and the float64 references of tests/dcn_v2_ref.py, validated from the
oracles alone (no GPU): the table reaches every regime it claims (one assertion per regime, on the labels), the exact
tier IS exact (the fp32 oracle equals the rounded float64 reference bit for bit, and the sums of absolute terms stay
below 2^24 units, so every summation order gives that value), the tolerance tier's decisions are the same in fp32 and
float64, and the oracle's own error against the reference -- the figure the GPU bounds are built from -- is measured."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import closed_form as CF
from tests import dcn_v2_cases as K
from tests import dcn_v2_ref as RF

F = np.float32


def _labels(kind=None, tier=None):
    return [(c, nt, K.pool_labels(c, nt)) for c in K.POOL_CASES for nt in c.modes
            if (kind is None or c.kind == kind) and (tier is None or c.tier == tier)]


def _some(pred, **kw):
    return any(pred(c, nt, l) for c, nt, l in _labels(**kw))


# ------------------------------------------------------------------------------------------- the table's reach
def test_pooling_table_reaches_every_channel_regime():
    for tier in K.TIERS:
        kw = dict(kind="channel", tier=tier)
        assert _some(lambda c, nt, l: (l.group, l.cec, l.vec, l.chunks, l.ncls) == (1, 8, 4, 1, 1) and not nt, **kw), "baseline"
        assert _some(lambda c, nt, l: (l.group, l.cec, l.vec, l.chunks, l.ncls) == (1, 8, 4, 1, 3), **kw), "classes > 1, VEC 4"
        assert _some(lambda c, nt, l: (l.cec, l.vec, l.chunks, l.tail_lanes) == (520, 4, 3, 2) and nt, **kw), "3 chunks, 2-lane tail"
        assert _some(lambda c, nt, l: (l.cec, l.vec, l.chunks, l.tail_lanes, l.ncls) == (512, 4, 2, 64, 2), **kw), "2 full chunks"
        assert _some(lambda c, nt, l: (l.group, l.cec, l.vec, l.ncls) == (1, 3, 1, 2), **kw), "group 1, scalar lanes"
        assert _some(lambda c, nt, l: (l.group, l.cec, l.vec, l.C % 4) == (1, 10, 1, 2), **kw), "C % 4 != 0, group 1"
        assert _some(lambda c, nt, l: (l.group, l.cec, l.vec, l.chunks, l.tail_lanes) == (2, 70, 1, 2, 6), **kw), "group 2, 2 chunks"
        assert _some(lambda c, nt, l: (l.group, l.cec, l.ncls, l.vec) == (3, 4, 2, 1), **kw), "group 3, 4 per class"
        assert _some(lambda c, nt, l: (l.group, l.cec, l.ncls, l.vec) == (2, 1, 4, 1), **kw), "group 2, one channel per class"
        assert _some(lambda c, nt, l: nt, **kw) and _some(lambda c, nt, l: not nt, **kw)
    # every channel case but the no-trans tail case runs both ways
    for c in K.POOL_CASES:
        if c.kind == "channel":
            assert c.modes == ((True,) if c.od == 520 else (False, True)), c.name
            assert (c.N, c.H, c.W, c.R) == (2, 9, 11, 6), c.name
    # no channel case takes a second lap (that is the lap case's job)
    assert all(l.laps == 1 for _, _, l in _labels(kind="channel"))


def test_pooling_table_reaches_the_part_and_lap_regimes():
    parts = {(c.P, c.part, c.tier) for c in K.POOL_CASES}
    assert (4, 2, "exact") in parts, "part < P, P = 4"
    assert (6, 4, "tolerance") in parts, "part < P, P = 6"
    assert any(p[1] == 1 for p in parts), "part = 1"
    # the text's own float expression decides the cell: with P = 6, part = 4 it is not the identity and not a halving
    assert RF._part_cells(6, 4).tolist() == [0, 0, 1, 2, 2, 3]
    assert RF._part_cells(4, 2).tolist() == [0, 0, 1, 1]
    c = K.POOL_BY_NAME["lap2"]
    for nt in c.modes:
        l = K.pool_labels(c, nt)
        assert (c.R, c.P, c.od, c.N, c.H, c.W) == (5500, 7, 4, 4, 16, 16)
        assert l.waves == 269500 and l.waves > K.WAVE_CAP == 262144 and l.laps == 2
    assert c.modes == (False, True) and c.tier == "tolerance"
    assert K.pool_device_inputs("lap2").rois.shape == (5500, 5)
    assert np.unique(K.pool_device_inputs("lap2").rois, axis=0).shape[0] == K.LAP_DISTINCT


def test_pooling_table_reaches_every_geometry_regime():
    ref = K.pool_reference("geo/P2", False)
    m = ref.margins
    inp = K.pool_inputs("geo/P2")
    assert (ref.count[0] == 0).all() and (ref.out[0] == 0).all(), "RoI wholly outside"
    gi_alone = RF.psroi_backward(inp.grad[:1], ref.count[:1], inp.x, inp.rois[:1], inp.trans[:1], *K._cfg(inp.case, False))
    assert not gi_alone[0].any() and not gi_alone[1].any(), "no gradient flows from it"
    assert set(np.unique(ref.count[1])) == {1, 2, 4}, "RoI half outside (P = 2)"
    assert set(np.unique(K.pool_reference("geo/P4", True).count[0])) == {0, 1, 2, 4}, "RoI half outside (P = 4)"
    assert m.on_low > 0, "a kept sample exactly at -0.5"
    assert m.on_high > 0, "a kept sample exactly at W - 0.5 / H - 0.5"
    assert m.clamped >= m.on_low + m.on_high
    assert m.on_integer > 0, "kept samples on integer coordinates (floor == ceil)"
    assert m.on_last > 0, "a kept sample exactly at W - 1 / H - 1"
    assert m.crossed > 0, "a shift carries a bin across the border"
    assert m.skip.min() == 0 and m.floor.min() == 0, "the exact tier sits ON the thresholds"
    a, b, c = K.GEO_ROUNDING_ROWS
    assert inp.rois[a, 1:].tolist() == [2.5, -2.5, 9.5, 4.5]
    r = lambda n: RF.psroi_forward(inp.x, inp.rois[n:n + 1], inp.trans[a:a + 1], *K._cfg(inp.case, False))[0]
    assert np.array_equal(r(a), r(c)) and not np.array_equal(r(a), r(b)), "x.5 rounds away from zero: as x.51, not x.49"
    assert RF.round_half_away([2.5, -2.5, 3.5, 2.49, 2.51]).tolist() == [3, -3, 4, 2, 3]
    w = K.pool_reference("geo/width-clamp", False).margins
    assert w.width_clamped >= 8 and K.POOL_BY_NAME["geo/width-clamp"].tier == "tolerance", "max(width, 0.1)"
    assert (K.pool_reference("geo/width-clamp", False).count[:5].reshape(5, -1).max(1) > 0).all(), "the clamped RoIs pool samples"


def test_bad_batch_rows_pool_nothing_and_change_no_gradient():
    inp = K.pool_inputs("geo/bad-batch")
    c = inp.case
    bad = (inp.rois[:, 0] < 0) | (inp.rois[:, 0] >= c.N)
    assert bad.sum() == 5 and (inp.rois[bad, 0] < 0).any() and (inp.rois[bad, 0] >= c.N).any() and not bad.all()
    for nt in c.modes:
        ref = K.pool_reference(c.name, nt)
        assert not ref.out[bad].any() and not ref.count[bad].any()
        assert ref.count[~bad].any()
        v = ~bad
        gi, gt, _ = RF.psroi_backward(inp.grad[v], ref.count[v], inp.x, inp.rois[v], inp.trans[v], *K._cfg(c, nt))
        assert np.array_equal(gi, ref.grad_input)
        if not nt:
            assert np.array_equal(gt, ref.grad_trans[v]) and not ref.grad_trans[bad].any()
        # the oracle states the same rule
        o_out, o_cnt = O.deform_psroi_forward(inp.x, inp.rois, inp.trans, *K._cfg(c, nt))
        assert not o_out[bad].any() and not o_cnt[bad].any()


def test_convolution_table_reaches_every_regime():
    lab = {c.name: K.conv_labels(c) for c in K.CONV_CASES}
    tails = {(l.x_blocks, l.tail_lanes) for l in lab.values()}
    assert {l.Wo for l in lab.values()} >= {64, 65, 70, 130}
    assert (1, 64) in tails, "full blocks"
    assert (2, 1) in tails, "a 1-lane tail"
    assert (2, 6) in tails, "a 6-lane tail"
    assert (3, 2) in tails, "two blocks plus a tail"
    assert all(l.Ho == 3 for n, l in lab.items() if n.startswith("wo") and "pad21" not in n)
    assert {l.cpg for l in lab.values()} >= {1, 2, 3, 5, 8}, "fewer than, equal to (with 8: twice) and not a multiple of 4 waves"
    assert {l.dg for l in lab.values()} == {1, 2, 3}
    geoms = {(c.k, c.pad, c.stride[0], c.dil[0]) for c in K.CONV_CASES}
    assert geoms >= {(3, (1, 1), 1, 1), (3, (2, 2), 2, 2), (1, (0, 0), 1, 1), (3, (2, 1), 1, 1)}
    assert all(K.conv_labels(c).x_blocks > 1 or c.name == "wo64-cpg8" for c in K.CONV_CASES)


def test_border_fixture_crosses_every_class_on_both_axes():
    inp = K.border_inputs()
    c = inp.case
    assert (c.H, c.W, c.k, c.pad, c.stride, c.dg) == (5, 6, 3, (1, 1), (1, 1), 1)
    h, w = K.conv_reference(c.name, "exact", True).margins.positions
    ch, cw = K.border_class(h, c.H), K.border_class(w, c.W)
    assert ch.min() >= 0 and cw.min() >= 0
    for b in range(c.B):
        pairs = set(zip(ch[b].ravel().tolist(), cw[b].ravel().tolist()))
        assert len(pairs) == 100, "image %d: %d of the 100 (row class, column class) pairs" % (b, len(pairs))
    assert len(K.BORDER_CLASSES) == 10 and np.array_equal(K.border_class(K.border_positions(5), 5), np.arange(10))
    assert np.array_equal(inp.off * 4, np.round(inp.off * 4))


# ------------------------------------------------------------------------------------------- exact tier IS exact
def _units(terms):
    """smallest k with every term a multiple of 2^-k"""
    for k in range(0, 24):
        s = terms * 2.0 ** k
        if np.array_equal(s, np.round(s)):
            return k
    raise AssertionError("terms are not dyadic")


def _eq(got, ref, what):
    ref32 = np.asarray(ref, np.float64).astype(F)
    assert np.array_equal(ref32.astype(np.float64), ref), what + ": the float64 reference is not an fp32 number"
    bad = np.argwhere(np.asarray(got) != ref32)
    assert bad.shape[0] == 0, "%s: %d differ, first at %s" % (what, bad.shape[0], tuple(bad[0]) if bad.size else ())


@pytest.mark.parametrize("name", [c.name for c in K.POOL_CASES if c.tier == "exact"])
def test_exact_pooling_fixtures_equal_the_fp32_oracle_bit_for_bit(name):
    inp = K.pool_inputs(name)
    c = inp.case
    for nt in c.modes:
        ref = K.pool_reference(name, nt)
        cfg = K._cfg(c, nt)
        out, cnt = O.deform_psroi_forward(inp.x, inp.rois, inp.trans, *cfg)
        _eq(cnt, ref.count, name + " count")
        _eq(out, ref.out, name + " out")
        assert set(np.unique(ref.count)) <= {0, 1, 2, 4}
        gi, gt = O.deform_psroi_backward(inp.grad, cnt, inp.x, inp.rois, inp.trans, *cfg)
        _eq(gi, ref.grad_input, name + " grad_input")
        if not nt:
            _eq(gt, ref.grad_trans, name + " grad_trans")
        # any order: every term is a multiple of 2^-k and the absolute terms of one accumulator sum below 2^(24 - k)
        k = _units(ref.abs["terms"])
        top = max(ref.abs["gi_abs"].max(), 0.0 if nt else ref.abs["gt_abs"].max())
        assert top * 2.0 ** k < 2.0 ** 24, "%s: %g units of 2^-%d in one accumulator" % (name, top * 2.0 ** k, k)
        assert np.abs(inp.x).max() <= 8 and np.abs(inp.grad).max() <= 8 and np.array_equal(inp.trans * 8, np.round(inp.trans * 8))
        assert c.scale in (1.0, 0.25) and c.P in (2, 4) and c.spp in (1, 2) and c.tstd == 0.25


def _identity_weight(c):
    n = c.C * c.k * c.k
    return np.eye(n, dtype=F).reshape(n, c.C, c.k, c.k)


def _oracle_conv(inp, masked):
    """the fp32 oracle's col, grad_im, grad_offset, grad_mask.  Masked: the operator-level restatement with an identity
    weight (its GEMMs then copy); unmasked: the v1 sampling oracles (mask == nullptr is the v1 arithmetic)"""
    c = inp.case
    if not masked:
        a = K.conv_args(c)
        return (O.deform_im2col(inp.im, inp.off, *a), O.deform_col2im(inp.gcol, inp.off, inp.im.shape, *a),
                O.deform_col2im_coord(inp.gcol, inp.im, inp.off, *a), None)
    w = _identity_weight(c)
    a = (c.pad, c.stride, c.dil, c.dg)
    y = O.dcn_v2_forward(inp.im, inp.off, inp.mask, w, np.zeros(w.shape[0], F), *a)
    gi, go, gm, _, _ = O.dcn_v2_backward(inp.im, inp.off, inp.mask, w, np.ascontiguousarray(inp.gcol.transpose(1, 0, 2, 3)), *a)
    return y.transpose(1, 0, 2, 3), gi, go, gm


def _ref_conv_for_oracle(inp, masked):
    """the reference the ORACLE is held to: its operator-level input gradient follows L651-653 (pad_h on both axes)"""
    c = inp.case
    ref = K.conv_reference(c.name, inp.tier, masked)
    gim = ref.grad_im
    if masked and c.pad[0] != c.pad[1]:
        gim = RF.mdcn_col2im(inp.gcol, inp.off, inp.mask, inp.im.shape, *K.conv_args(c, pad=(c.pad[0], c.pad[0])))[0]
    return ref, gim


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("name", [c.name for c in K.CONV_CASES] + [K.BORDER.name])
def test_exact_convolution_fixtures_equal_the_fp32_oracle_bit_for_bit(name, masked):
    inp = K.border_inputs() if name == K.BORDER.name else K.conv_inputs(name, "exact")
    ref, gim = _ref_conv_for_oracle(inp, masked)
    col, gi, go, gm = _oracle_conv(inp, masked)
    _eq(col, ref.col, name + " col")
    _eq(gi, gim, name + " grad_im")
    _eq(go, ref.grad_offset, name + " grad_offset")
    if masked:
        _eq(gm, ref.grad_mask, name + " grad_mask")
    assert np.array_equal(inp.off * 4, np.round(inp.off * 4)) and np.array_equal(inp.mask * 8, np.round(inp.mask * 8))
    # any order: quarters x quarters x eighths x integers = multiples of 2^-7; the largest accumulator stays far below 2^24
    gabs = RF.mdcn_col2im(np.abs(inp.gcol), inp.off, np.abs(inp.mask) if masked else None, inp.im.shape, *K.conv_args(inp.case))[0]
    assert gabs.max() * 2.0 ** 7 < 2.0 ** 24


# ------------------------------------------------------------------------------------------- tolerance tier
_MEASURED = {}


def _measure(kind, got, ref, what):
    e = float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, float(np.abs(ref).max())))
    _MEASURED[kind] = max(_MEASURED.get(kind, 0.0), e)
    print("oracle vs float64  %-34s %-12s %.3e" % (what, kind, e))
    assert e <= K.ORACLE_ERR[kind], "%s %s: the oracle is %.3e off the reference, the table states %.3e" % (
        what, kind, e, K.ORACLE_ERR[kind])


@pytest.mark.parametrize("name", [c.name for c in K.POOL_CASES if c.tier == "tolerance"])
def test_tolerance_pooling_decisions_agree_and_oracle_error(name):
    inp = K.pool_inputs(name)
    c = inp.case
    dev = K.pool_device_inputs(name)
    for nt in c.modes:
        ref = K.pool_reference(name, nt)
        assert ref.margins.every().min() >= K.MARGIN, "%s: a decision within %g px of its threshold" % (name, K.MARGIN)
        cfg = K._cfg(c, nt)
        out, cnt = O.deform_psroi_forward(dev.x, dev.rois, dev.trans, *cfg)
        assert np.array_equal(cnt, ref.count), name + ": the oracle counts other samples"
        _measure("out", out, ref.out, "%s no_trans=%d" % (name, nt))
        gi, gt = O.deform_psroi_backward(dev.grad, cnt, dev.x, dev.rois, dev.trans, *cfg)
        _measure("grad_input", gi, ref.grad_input, "%s no_trans=%d" % (name, nt))
        if not nt:
            _measure("grad_trans", gt, ref.grad_trans, "%s no_trans=%d" % (name, nt))


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("name", [c.name for c in K.CONV_CASES])
def test_tolerance_convolution_decisions_agree_and_oracle_error(name, masked):
    inp = K.conv_inputs(name, "tolerance")
    ref, gim = _ref_conv_for_oracle(inp, masked)
    assert min(ref.margins.inside, ref.margins.floor) >= K.MARGIN
    # fp32 positions (one rounding of integer + offset, as the text computes them) decide as float64 does
    off = inp.off.reshape(inp.case.B, inp.case.dg, -1, 2, *inp.off.shape[2:])
    for p64, o32, size in zip(ref.margins.positions, (off[:, :, :, 0], off[:, :, :, 1]), (inp.case.H, inp.case.W)):
        p32 = np.round(p64 - o32).astype(F) + o32
        assert p32.dtype == F and np.array_equal(np.floor(p32), np.floor(p64))
        assert np.array_equal(p32 > -1, p64 > -1) and np.array_equal(p32 < size, p64 < size)
    col, gi, go, gm = _oracle_conv(inp, masked)
    tag = "%s mask=%d" % (name, masked)
    _measure("col", col, ref.col, tag)
    _measure("grad_im", gi, gim, tag)
    _measure("grad_offset", go, ref.grad_offset, tag)
    if masked:
        _measure("grad_mask", gm, ref.grad_mask, tag)


def test_bounds_are_built_from_the_oracle_error_and_the_suite():
    for k, b in K.BOUND.items():
        assert b == max(4 * K.ORACLE_ERR[k], K.SUITE_BOUND[k])
    assert K.SUITE_BOUND["out"] == 2e-6 and K.SUITE_BOUND["grad_input"] == 2e-5 and K.SUITE_BOUND["grad_trans"] == 1e-4
    assert K.SUITE_BOUND["col"] == 2e-5 and {K.SUITE_BOUND[k] for k in ("grad_im", "grad_offset", "grad_mask")} == {1e-4}


# ------------------------------------------------------------------------------------------- closed form
@pytest.mark.parametrize("no_trans", [True, False])
def test_reference_agrees_with_the_closed_form_on_an_affine_map(no_trans):
    """on f_c(x, y) = a_c x + b_c y + d_c a bin whose samples are all inside and unclamped pools f at the mean sample
    position (tests/closed_form.py::psroi_expected); its shift derivative is (a, b) x trans_std x RoI size"""
    rng = np.random.default_rng(3)
    N, H, W, od, G, P, part, spp, scale, tstd = 1, 40, 48, 4, 2, 4, 2, 3, 0.25, 0.1
    C = od * G * G
    a, b, d = rng.standard_normal(C), rng.standard_normal(C), rng.standard_normal(C)
    yy, xx = np.mgrid[0:H, 0:W]
    x = a[:, None, None] * xx + b[:, None, None] * yy + d[:, None, None]
    rois = np.array([[0, 40, 36, 120, 100], [0, 52.2, 41.7, 99.3, 110.1], [0, 64, 48, 127, 95]], F)
    trans = (rng.standard_normal((3, 4, part, part)) * 0.3).astype(F)
    # float64 image: the closed form is then exact up to float64 rounding
    out, cnt, mg = RF.psroi_forward(x[None], rois, trans, no_trans, scale, od, G, P, part, spp, tstd)
    assert (cnt == spp * spp).all() and mg.clamped == 0
    exp, dtr = CF.psroi_expected((a, b, d), rois, None if no_trans else trans, scale, od, G, P, part, spp, float(F(tstd)))
    np.testing.assert_allclose(out, exp, rtol=0, atol=1e-11)
    if not no_trans:
        g = rng.standard_normal(out.shape)
        _, gt, _ = RF.psroi_backward(g, cnt, x[None], rois, trans, no_trans, scale, od, G, P, part, spp, tstd)
        want = np.zeros_like(gt, dtype=np.float64)
        cells = RF._part_cells(P, part)
        cec = od // 2
        for n in range(3):
            for ct in range(od):
                for ph in range(P):
                    for pw in range(P):
                        want[n, 2 * (ct // cec), cells[ph], cells[pw]] += g[n, ct, ph, pw] * dtr[n, ct, ph, pw, 0]
                        want[n, 2 * (ct // cec) + 1, cells[ph], cells[pw]] += g[n, ct, ph, pw] * dtr[n, ct, ph, pw, 1]
        np.testing.assert_allclose(gt, want, rtol=0, atol=1e-10)
