"""GPU: every regime of the DCN v2 kernels -- csrc/deform_psroi_pool.hip (VEC 4 / 1, one and several channel chunks
with full and partial tails, classes, groups, part cells, the second lap of the capped grid, every border rule of the
sample geometry, batch indices outside [0, N)) and the modulated entry points of csrc/deform_nchw.hip with and without
a mask (one to three wo blocks with 1- / 2- / 6-lane tails, 1 to 8 channels per deformable group over the four waves,
1 to 3 groups, four kernel geometries, every border class of the sample position) -- against the float64 references of
tests/dcn_v2_ref.py.  tests/dcn_v2_cases.py is the case table; tests/test_dcn_v2_cases_cpu.py proves, without a GPU,
that the table reaches these regimes and that its EXACT tier is exact.

Every case runs through the Python wrappers (dcn_v2_pooling, dcn_v2_conv; the v1 wrappers for mask == nullptr) AND
through the C ABI called directly, where every output -- out, top_count, grad_input, grad_trans, col, grad_offset,
grad_mask -- holds NaN before the call: a NaN left afterwards is an element nobody wrote.  The ABI's images sit in
NaN-guarded allocations (tests/guarded.py): a corner read outside the map, even times a zero weight, shows as NaN.
Exact tier: array_equal.  Tolerance tier: BOUND[kind] * max(1, |ref|max), BOUND from the cases module (four times the
fp32 oracle's own error against the reference, or the bound tests/test_gpu_dcn_v2.py states where that is larger).
Where oracle/_ref/libjdet_ref_hip.so is present the channel-regime and wo-regime cases are also compared with the
compiled reference kernels, at the tolerances of tests/test_gpu_reference_kernels.py -- never a case with a batch index
outside [0, N): the reference kernels read out of bounds there.

Out of scope: the coordinate-gradient kernel's own grid cap (262144 workgroups x 256 items) is reached only with
hundreds of megabytes of columns; its grid-stride loop takes one lap in every case here."""
import numpy as np
import pytest
import torch

from oracle import ref_hip as RH
from tests import dcn_v2_cases as K
from tests import dcn_v2_ref as RF
from tests import guarded as GD

pytestmark = pytest.mark.gpu
F = np.float32


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F)).to(dev)


def _nan(dev, shape):
    return torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=dev)


def _guarded(dev, a):
    """the array inside NaN guard bands"""
    view, raw = GD.guarded(a.shape, torch.float32, dev, GD.QNAN_WORD)
    view.copy_(_t(dev, a))
    return view, raw


def _compare(got, ref, tier, kind, what, bound=None):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == ref.shape, "%s %s: shape %r, reference %r" % (what, kind, got.shape, ref.shape)
    nan = np.argwhere(np.isnan(got))
    assert nan.shape[0] == 0, "%s %s: %d elements were never written, first at %s" % (
        what, kind, nan.shape[0], tuple(nan[0]) if nan.size else ())
    scale = max(1.0, float(np.abs(ref).max())) if ref.size else 1.0
    err = float(np.abs(got.astype(np.float64) - ref).max()) / scale if ref.size else 0.0
    used = 0.0 if tier == "exact" else (K.BOUND[kind] if bound is None else bound)
    print("dcn_v2_regimes | %s | %s | %s | device err %.3e | bound %.3e" % (what, tier, kind, err, used))
    if tier == "exact":
        ref32 = ref.astype(F)
        bad = np.argwhere(got != ref32)
        assert bad.shape[0] == 0, "%s %s: %d of %d values differ, first at %s: got %r, reference %r" % (
            what, kind, bad.shape[0], ref.size, tuple(bad[0]), got[tuple(bad[0])], ref32[tuple(bad[0])])
        assert np.array_equal(got, ref32)
    else:
        assert err <= used, "%s %s: error %.3e of the scale %.3g, bound %.3e" % (what, kind, err, scale, used)


# ------------------------------------------------------------------------------------------- pooling
def _pool_args(c, x_shape, R, no_trans):
    N, C, H, W = x_shape
    return (N, C, H, W, R, int(no_trans), float(c.scale), int(c.od), int(c.G), int(c.P), int(c.part), int(c.spp),
            float(c.tstd), 2 if no_trans else 2 * c.ncls)


def _pool_abi(dev, inp, no_trans):
    """-> out, count, grad_input (NCHW order), grad_trans; every output NaN before the call, the map NaN-guarded"""
    from jdet_amd import _lib as L
    lib = L.lib()
    c = inp.case
    R = inp.rois.shape[0]
    x, _raw = _guarded(dev, inp.x.transpose(0, 2, 3, 1))                    # channels-last
    rois = _t(dev, inp.rois)
    trans = None if no_trans else _t(dev, inp.trans)
    args = _pool_args(c, inp.x.shape, R, no_trans)
    out, cnt = _nan(dev, (R, c.P, c.P, c.od)), _nan(dev, (R, c.P, c.P, c.od))
    st = L.stream_ptr(x)
    L.check(lib.jdet_deform_psroi_pool_forward(L.ptr(x), L.ptr(rois), L.ptr(trans), *args, L.ptr(out), L.ptr(cnt), st),
            "jdet_deform_psroi_pool_forward")
    g = _t(dev, inp.grad.transpose(0, 2, 3, 1))
    gi = _nan(dev, x.shape)
    gt = None if no_trans else _nan(dev, inp.trans.shape)
    L.check(lib.jdet_deform_psroi_pool_backward(L.ptr(g), L.ptr(cnt), L.ptr(x), L.ptr(rois), L.ptr(trans), *args,
                                                L.ptr(gi), L.ptr(gt), st), "jdet_deform_psroi_pool_backward")
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2), cnt.permute(0, 3, 1, 2), gi.permute(0, 3, 1, 2), gt


def _pool_wrapper(dev, inp, no_trans):
    from jdet_amd.ops import dcn_v2
    c = inp.case
    x = _t(dev, inp.x).requires_grad_(True)
    t = _t(dev, inp.trans).requires_grad_(True)
    y = dcn_v2.dcn_v2_pooling(x, _t(dev, inp.rois), t, c.scale, c.P, c.od, no_trans, c.G, c.part, c.spp, c.tstd)
    y.backward(_t(dev, inp.grad))
    if no_trans:
        assert t.grad is None
    return y.detach(), None, x.grad, (None if no_trans else t.grad)


def _check_pool(dev, name, routes=("abi", "wrapper")):
    inp = K.pool_device_inputs(name)
    c = inp.case
    for no_trans in c.modes:
        ref = K.pool_reference(name, no_trans)
        lab = K.pool_labels(c, no_trans)
        tag = "%s no_trans=%d [VEC %d, %d chunk(s), tail %d lanes, %d class(es), group %d, %d lap(s)]" % (
            name, no_trans, lab.vec, lab.chunks, lab.tail_lanes, lab.ncls, lab.group, lab.laps)
        for route in routes:
            out, cnt, gi, gt = (_pool_abi if route == "abi" else _pool_wrapper)(dev, inp, no_trans)
            what = "%s %s" % (tag, route)
            if cnt is not None:
                _compare(cnt, ref.count, "exact", "out", what + " (count)")
            _compare(out, ref.out, c.tier, "out", what)
            _compare(gi, ref.grad_input, c.tier, "grad_input", what)
            if not no_trans:
                _compare(gt, ref.grad_trans, c.tier, "grad_trans", what)


@pytest.mark.parametrize("name", [c.name for c in K.POOL_CASES if c.kind in ("channel", "part")])
def test_pooling_channel_and_part_regimes(dev, name):
    """VEC 4 / 1, classes, groups, one to three chunks with 2-, 6- and 64-lane tails, part cells that are not the bin"""
    _check_pool(dev, name)


@pytest.mark.parametrize("name", [c.name for c in K.POOL_CASES if c.kind == "geometry"])
def test_pooling_geometry_regimes(dev, name):
    """RoIs outside and half outside the map, samples ON -0.5 / W - 0.5 / integers / W - 1, x.5 corners, shifts across
    the border, the 0.1 width clamp"""
    _check_pool(dev, name)
    if name == "geo/P2":
        inp = K.pool_inputs(name)
        a, b, c = K.GEO_ROUNDING_ROWS
        out = _pool_abi(dev, inp, True)[0].cpu().numpy()
        assert np.array_equal(out[a], out[c]) and not np.array_equal(out[a], out[b]), "x.5 corners round away from zero"
        assert not out[0].any(), "the RoI outside the map pools exact zeros"


def test_pooling_batch_index_outside_the_batch(dev):
    """batch -1, -7, N and N + 3 among valid RoIs: their output and count rows are exact zeros, and both gradients
    equal those of the same call without them.  Float64 reference only"""
    name = "geo/bad-batch"
    _check_pool(dev, name)
    inp = K.pool_inputs(name)
    c = inp.case
    bad = (inp.rois[:, 0] < 0) | (inp.rois[:, 0] >= c.N)
    keep = K.NS(case=c, x=inp.x, rois=inp.rois[~bad], trans=inp.trans[~bad], grad=inp.grad[~bad])
    for no_trans in c.modes:
        out, cnt, gi, gt = _pool_abi(dev, inp, no_trans)
        assert not out[bad].any() and not cnt[bad].any()
        _, _, gi2, gt2 = _pool_abi(dev, keep, no_trans)
        assert torch.equal(gi, gi2), "grad_input changes with the RoIs outside the batch"
        if not no_trans:
            assert torch.equal(gt[~bad], gt2) and not gt[bad].any()


def test_pooling_second_lap_of_the_capped_grid(dev):
    """269500 waves against a grid of 262144: the last 7356 run in the grid-stride loop's second lap"""
    _check_pool(dev, "lap2")
    torch.cuda.empty_cache()


@pytest.mark.skipif(not RH.available(), reason="oracle/_ref/libjdet_ref_hip.so not built")
@pytest.mark.parametrize("name", [c.name for c in K.POOL_CASES if c.refhip])
def test_pooling_channel_regimes_against_the_reference_kernels(dev, name):
    inp = K.pool_inputs(name)
    c = inp.case
    assert ((inp.rois[:, 0] >= 0) & (inp.rois[:, 0] < c.N)).all(), "the reference kernels read out of bounds"
    x, rois, trans, g = (_t(dev, v) for v in (inp.x, inp.rois, inp.trans, inp.grad))
    for no_trans in c.modes:
        cfg = K._cfg(c, no_trans)
        ry, rcnt = RH.psroi_forward(x, rois, trans, *cfg)
        rgi, rgt = RH.psroi_backward(g, rcnt, x, rois, trans, *cfg)
        out, _, gi, gt = _pool_wrapper(dev, inp, no_trans)
        what = "%s no_trans=%d vs reference kernels" % (name, no_trans)
        _compare(out, ry.cpu().numpy().astype(np.float64), "tolerance", "out", what, K.REFHIP_ATOL["out"] / max(1.0, float(ry.abs().max())))
        _compare(gi, rgi.cpu().numpy().astype(np.float64), "tolerance", "grad_input", what,
                 K.REFHIP_ATOL["grad_input"] / max(1.0, float(rgi.abs().max())))
        if not no_trans:
            _compare(gt, rgt.cpu().numpy().astype(np.float64), "tolerance", "grad_trans", what, K.REFHIP_ATOL["grad_trans"])


# ------------------------------------------------------------------------------------------- modulated convolution
def _conv_inputs(name, tier):
    return K.border_inputs() if name == K.BORDER.name else K.conv_inputs(name, tier)


def _conv_abi(dev, inp, masked):
    """-> col, grad_im, grad_offset, grad_mask through the C ABI; outputs NaN before the call, the image NaN-guarded"""
    from jdet_amd import _lib as L
    from jdet_amd.ops.dcn_v1 import _geom_args
    lib = L.lib()
    c = inp.case
    geom = _geom_args(c.B, c.C, c.H, c.W, c.k, c.k, c.pad, c.stride, c.dil, c.dg)
    im, _raw = _guarded(dev, inp.im)
    off, gcol = _t(dev, inp.off), _t(dev, inp.gcol)
    col, gim, goff = _nan(dev, inp.gcol.shape), _nan(dev, inp.im.shape), _nan(dev, inp.off.shape)
    st = L.stream_ptr(im)
    if masked:
        mask, gmask = _t(dev, inp.mask), _nan(dev, inp.mask.shape)
        L.check(lib.jdet_modulated_deform_im2col(L.ptr(im), L.ptr(off), L.ptr(mask), *geom, L.ptr(col), st), "im2col")
        L.check(lib.jdet_modulated_deform_col2im(L.ptr(gcol), L.ptr(off), L.ptr(mask), *geom, L.ptr(gim), st), "col2im")
        L.check(lib.jdet_modulated_deform_col2im_coord(L.ptr(gcol), L.ptr(im), L.ptr(off), L.ptr(mask), *geom,
                                                       L.ptr(goff), L.ptr(gmask), st), "col2im_coord")
    else:
        gmask = None
        L.check(lib.jdet_deform_im2col(L.ptr(im), L.ptr(off), *geom, L.ptr(col), st), "im2col")
        L.check(lib.jdet_deform_col2im(L.ptr(gcol), L.ptr(off), *geom, L.ptr(gim), st), "col2im")
        L.check(lib.jdet_deform_col2im_coord(L.ptr(gcol), L.ptr(im), L.ptr(off), *geom, L.ptr(goff), st), "col2im_coord")
    torch.cuda.synchronize()
    return col, gim, goff, gmask


def _conv_wrapper(dev, inp, masked):
    """masked: dcn_v2_conv with an identity weight (its GEMMs then copy the columns / the column gradient);
    mask == nullptr: the v1 wrappers"""
    from jdet_amd.ops import dcn_v1, dcn_v2
    c = inp.case
    a = K.conv_args(c)
    if not masked:
        im, off, gcol = _t(dev, inp.im), _t(dev, inp.off), _t(dev, inp.gcol)
        return (dcn_v1.deformable_im2col(im, off, *a), dcn_v1.deformable_col2im(gcol, off, im.shape, *a),
                dcn_v1.deformable_col2im_coord(gcol, im, off, *a), None)
    n = c.C * c.k * c.k
    t = [_t(dev, v).requires_grad_(True) for v in (inp.im, inp.off, inp.mask, np.eye(n, dtype=F).reshape(n, c.C, c.k, c.k))]
    y = dcn_v2.dcn_v2_conv(*t, None, c.stride, c.pad, c.dil, c.dg)
    y.backward(_t(dev, inp.gcol.transpose(1, 0, 2, 3)))
    return y.detach().permute(1, 0, 2, 3), t[0].grad, t[1].grad, t[2].grad


def _check_conv(dev, name, tier, masked, routes=("abi", "wrapper")):
    inp = _conv_inputs(name, tier)
    c = inp.case
    ref = K.conv_reference(name, tier, masked)
    lab = K.conv_labels(c)
    tag = "%s mask=%d [Wo %d: %d block(s), tail %d lanes, %d ch / group over 4 waves, dg %d, k %d pad %r stride %d dil %d]" % (
        name, masked, lab.Wo, lab.x_blocks, lab.tail_lanes, lab.cpg, lab.dg, c.k, c.pad, c.stride[0], c.dil[0])
    for route in routes:
        col, gim, goff, gmask = (_conv_abi if route == "abi" else _conv_wrapper)(dev, inp, masked)
        what = "%s %s" % (tag, route)
        ref_gim = ref.grad_im
        if route == "wrapper" and masked and c.pad[0] != c.pad[1]:
            # the operator follows the reference's L651-653: its input gradient samples with pad_h on both axes
            ref_gim = RF.mdcn_col2im(inp.gcol, inp.off, inp.mask, inp.im.shape, *K.conv_args(c, pad=(c.pad[0], c.pad[0])))[0]
        _compare(col, ref.col, tier, "col", what)
        _compare(gim, ref_gim, tier, "grad_im", what)
        _compare(goff, ref.grad_offset, tier, "grad_offset", what)
        if masked:
            _compare(gmask, ref.grad_mask, tier, "grad_mask", what)


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("tier", K.TIERS)
@pytest.mark.parametrize("name", [c.name for c in K.CONV_CASES])
def test_modulated_convolution_regimes(dev, name, tier, masked):
    """wo blocks and tails, channels per group against the four waves, 1 to 3 groups, the four kernel geometries"""
    _check_conv(dev, name, tier, masked)


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
def test_modulated_convolution_border_fixture(dev, masked):
    """5 x 6 map: every (row class, column class) pair of {below -1, -1, (-1, 0), 0, interior integer, interior
    fraction, size - 1, (size - 1, size), size, above size}; the image sits between NaN guards"""
    _check_conv(dev, K.BORDER.name, "exact", masked)


@pytest.mark.skipif(not RH.available(), reason="oracle/_ref/libjdet_ref_hip.so not built")
@pytest.mark.parametrize("tier", K.TIERS)
@pytest.mark.parametrize("name", [c.name for c in K.CONV_CASES if c.refhip])
def test_convolution_wo_regimes_against_the_reference_kernels(dev, name, tier):
    """the reference's three modulated kernels, one image at a time as its backward loop calls them"""
    inp = K.conv_inputs(name, tier)
    c = inp.case
    col, gim, goff, gmask = _conv_abi(dev, inp, True)
    if c.pad[0] != c.pad[1]:
        # the reference's host code hands its col2im kernel pad_h for both axes (L651-653); the operator reproduces
        # that, the entry point samples with the true geometry: the operator's input gradient is the comparable one
        gim = _conv_wrapper(dev, inp, True)[1]
    a = K.conv_args(c)
    for b in range(c.B):
        im, off, mask = _t(dev, inp.im[b]), _t(dev, inp.off[b]), _t(dev, inp.mask[b])
        gcol = _t(dev, inp.gcol[:, b])
        rcol = RH.dcn2_im2col(im, off, mask, *a)
        rgim = RH.dcn2_col2im(gcol, off, mask, (c.C, c.H, c.W), *a)
        rgoff, rgmask = RH.dcn2_col2im_coord(gcol, im, off, mask, *a)
        what = "%s image %d vs reference kernels" % (name, b)
        for kind, got, want in (("col", col[:, b], rcol), ("grad_im", gim[b], rgim), ("grad_offset", goff[b], rgoff),
                                ("grad_mask", gmask[b], rgmask)):
            np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=K.REFHIP_ATOL[kind],
                                       err_msg="%s %s" % (what, kind))


# ------------------------------------------------------------------------------------------- the other four routes
def test_border_fixture_through_the_channels_last_routes(dev):
    """the deformable sampling rule is written five times; the border fixture (3 x 3, stride 1, pad 1, one group, 16
    channels, no mask) through the other four: the channels-last im2col, the taps of the channels-last col2im, the
    gathered A operand of conv_igemm.hip and the gathered B operand of conv_wgrad.hip"""
    from jdet_amd.ops import conv_igemm as CI
    from jdet_amd.ops import dcn_v1 as D
    inp = K.border_inputs()
    c = inp.case
    ref = K.conv_reference(c.name, "exact", False)
    x, _raw = _guarded(dev, inp.im.transpose(0, 2, 3, 1))
    off = _t(dev, inp.off)
    g = ((3, 3), (1, 1), (1, 1), (1, 1))
    cols = D.deformable_im2col_nhwc(x, off, 3, 3, *g[1:])
    ref_cols = K.cols_nhwc(ref.col, c)
    _compare(cols, ref_cols, "exact", "col", "border deformable_im2col_nhwc")
    gx = D.deformable_col2im_nhwc(_t(dev, K.cols_nhwc(inp.gcol, c)), off, x.shape, 3, 3, *g[1:])
    _compare(gx, ref.grad_im.transpose(0, 2, 3, 1), "exact", "grad_im", "border deformable_col2im_nhwc")
    w = inp.weight.astype(np.float64)
    Cout = w.shape[0]
    y = CI.conv3x3_nhwc(x, _t(dev, inp.weight), offset=off)
    ref_y = (ref_cols @ w.reshape(Cout, -1).T).reshape(c.B, c.H, c.W, Cout)
    _compare(y, ref_y, "tolerance", "col", "border conv3x3_nhwc(offset)", K.NHWC_GEMM_BOUND * float(np.abs(ref_y).max())
             / max(1.0, float(np.abs(ref_y).max())))
    gw = CI.conv3x3_wgrad(x.permute(0, 3, 1, 2), _t(dev, inp.gy).permute(0, 3, 1, 2), off)
    ref_gw = (inp.gy.astype(np.float64).reshape(-1, Cout).T @ ref_cols).reshape(Cout, 3, 3, c.C).transpose(0, 3, 1, 2)
    _compare(gw, ref_gw, "tolerance", "grad_im", "border conv3x3_wgrad(offset)", K.NHWC_GEMM_BOUND * float(np.abs(ref_gw).max())
             / max(1.0, float(np.abs(ref_gw).max())))
