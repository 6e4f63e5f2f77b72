"""GPU: every regime of the shared sorted gather (csrc/csr_gather.h) through its three clients -- RoIAlign backward
(patch-keyed: direct rows + overflow CSR), channels-last deformable col2im and feature-refine backward (pixel-keyed)
-- against the CPU oracles' scatters.

The gather writes every destination pixel exactly once and never zero-fills, so a mapping bug is an entry dropped,
doubled or sent to the wrong pixel, or a pixel left stale.  Floating-point tolerances hide that once rows get long;
the EXACT tier (tests/gather_cases.py) therefore uses dyadic weights and integer gradients, for which every summation
order gives the same fp32 value, and compares with array_equal.  tests/test_gather_cases_cpu.py proves from the oracles
alone that those fixtures are exact and that the table reaches every regime.  The TOLERANCE tier (9 samples per bin,
hbb1, non-zero angles) uses the bounds the suite already states for these comparisons: BWD_ATOL * max(1, |ref|max) of
test_gpu_roi_align.py and 3e-5 * max(1, |ref|max) of test_gpu_fr.py.

Every output buffer holds NaN before the call (an unwritten pixel shows; untouched pixels must come back as exact
zeros) and every workspace whose content the entry point does not need clean holds 0xA5 bytes."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import gather_cases as G
from tests.test_gpu_roi_align import BWD_ATOL

pytestmark = pytest.mark.gpu

FR_ATOL = 3e-5       # tests/test_gpu_fr.py


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _poison(dev, nbytes):
    return torch.full((max(int(nbytes), 8),), 0xA5, dtype=torch.uint8, device=dev)


def _nan(dev, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _compare(got_nhwc, ref, case, atol, what):
    """got: (N,H,W,C) device tensor written over NaN; ref (N,C,H,W).  Exact tier: equality, whatever the order."""
    got = got_nhwc.permute(0, 3, 1, 2).cpu().numpy()
    ref = ref.astype(np.float32)
    assert not np.isnan(got).any(), "%s: %d values were never written" % (what, int(np.isnan(got).sum()))
    if case.tier == "exact":
        bad = np.argwhere(got != ref)
        assert bad.shape[0] == 0, "%s: %d of %d values differ, first at %s: got %r, reference %r" % (
            what, bad.shape[0], ref.size, tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])
        assert np.array_equal(got, ref)
    else:
        np.testing.assert_allclose(got, ref, rtol=0, atol=atol * max(1.0, float(np.abs(ref).max())), err_msg=what)


# ------------------------------------------------------------------------------------------- pixel-keyed clients
def _dcn_cols(c, grad):
    """oracle layout (C*kk, B, Ho, Wo) -> the channels-last column matrix [pos][tap][c]"""
    kk = c.k * c.k
    Ho, Wo = grad.shape[2:]
    return grad.reshape(c.C, kk, c.B, Ho, Wo).transpose(2, 3, 4, 1, 0).reshape(c.B * Ho * Wo, kk * c.C)


def _run_pixel(dev, inp, through_wrapper=False):
    from jdet_amd import _lib as L
    from jdet_amd.ops import dcn_v1 as D
    lib = L.lib()
    c = inp.case
    if c.client == "dcn":
        cols, off = _t(dev, _dcn_cols(c, inp.grad)), _t(dev, inp.off)
        if through_wrapper:
            return D.deformable_col2im_nhwc(cols, off, (c.B, c.H, c.W, c.C), c.k, c.k, (c.pad, c.pad), (1, 1), (1, 1))
        geom = D._geom_args(c.B, c.C, c.H, c.W, c.k, c.k, (c.pad, c.pad), (1, 1), (1, 1), 1)[:-1]
        wsb = lib.jdet_deform_col2im_nhwc_workspace(*geom)
        assert wsb > 0
        gin, ws = _nan(dev, (c.B, c.H, c.W, c.C)), _poison(dev, wsb)
        L.check(lib.jdet_deform_col2im_nhwc(L.ptr(cols), L.ptr(off), *geom, L.ptr(gin), L.ptr(ws), wsb,
                                            L.stream_ptr(cols)), "jdet_deform_col2im_nhwc")
        return gin
    g, boxes = _t(dev, inp.grad.transpose(0, 2, 3, 1)), _t(dev, inp.boxes)
    wsb = lib.jdet_feature_refine_backward_workspace(c.B, c.C, c.H, c.W, c.points)
    assert wsb > 0
    gin, ws = _nan(dev, (c.B, c.H, c.W, c.C)), _poison(dev, wsb)
    L.check(lib.jdet_feature_refine_backward(L.ptr(g), L.ptr(boxes), c.B, c.C, c.H, c.W, 0.125, c.points, L.ptr(gin),
                                             L.ptr(ws), wsb, L.stream_ptr(g)), "jdet_feature_refine_backward")
    return gin


@pytest.mark.parametrize("name", [c.name for c in G.PIXEL_CASES if not c.large])
def test_pixel_keyed_gather(dev, name):
    """work mapping (patch column / stripe / lap edges, stacked images), channel chunks, row lengths (empty rows, every
    residue of the unroll, 1296 entries), one and two scan tiles"""
    inp = G.pixel_inputs(name)
    ref = G.pixel_reference(inp)
    _compare(_run_pixel(dev, inp), ref, inp.case, FR_ATOL, name)
    if inp.case.client == "dcn":
        _compare(_run_pixel(dev, inp, through_wrapper=True), ref, inp.case, None, name + " (ops wrapper)")


@pytest.mark.parametrize("name", [c.name for c in G.PIXEL_CASES if c.large])
def test_pixel_keyed_gather_past_256_scan_tiles(dev, name):
    """525625 pixels = 257 scan tiles: the last workgroup scans the tile totals in two rounds with a carry"""
    inp = G.pixel_inputs(name)
    gin = _run_pixel(dev, inp)
    _compare(gin, G.pixel_reference(inp), inp.case, None, name)
    del gin
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- RoIAlign backward
def _second_gradient(grad):
    """the C = 8 gradient of the second gather from one plan: other values in the same range"""
    return np.concatenate([grad[:, ::-1], -grad], 1)


def _run_roi(dev, inp, route):
    """-> [(gin (N,H,W,C) device tensor, gradient (R,C,PH,PW) it belongs to, label)]"""
    from jdet_amd import _lib as L
    lib = L.lib()
    c = inp.case
    v, R, N, C, H, W, PH, PW, s = c.variant, c.R, c.N, c.C, c.H, c.W, c.PH, c.PW, c.s
    rois = _t(dev, inp.rois)
    st = L.stream_ptr(rois)
    if route == "planned":
        pb = lib.jdet_roi_align_backward_plan_bytes(v, R, N, H, W, PH, PW, s)
        assert pb > 0
        plan = _poison(dev, pb)
        L.check(lib.jdet_roi_align_backward_plan(v, L.ptr(rois), R, N, H, W, PH, PW, 1.0, s, L.ptr(plan), pb, st), "plan")
        out = []
        for grad in (inp.grad, _second_gradient(inp.grad)):
            Cg = grad.shape[1]
            g = _t(dev, grad.transpose(0, 2, 3, 1))
            gin = _nan(dev, (N, H, W, Cg))
            L.check(lib.jdet_roi_align_backward_cl_planned(v, L.ptr(g), R, N, Cg, H, W, PH, PW, s, L.ptr(gin), L.ptr(plan),
                                                           pb, st), "planned")
            out.append((gin, grad, "planned C=%d" % Cg))
        return out
    wsb = lib.jdet_roi_align_backward_workspace(v, R, N, C, H, W, PH, PW, s)
    assert wsb > 0, "the shape is not served by the gather"
    ws, gin = _poison(dev, wsb), _nan(dev, (N, H, W, C))
    if route == "nchw":
        g = _t(dev, inp.grad)
        L.check(lib.jdet_roi_align_backward(v, L.ptr(g), L.ptr(rois), R, N, C, H, W, PH, PW, 1.0, s, 1, None, L.ptr(gin),
                                            L.ptr(ws), wsb, st), "jdet_roi_align_backward")
    else:
        g = _t(dev, inp.grad.transpose(0, 2, 3, 1))
        L.check(lib.jdet_roi_align_backward_cl(v, L.ptr(g), L.ptr(rois), R, N, C, H, W, PH, PW, 1.0, s, 1, L.ptr(gin),
                                               L.ptr(ws), wsb, 0, st), "jdet_roi_align_backward_cl")
    return [(gin, inp.grad, route)]


def _check_roi_case(dev, name):
    inp = G.roi_inputs(name)
    ref = {}
    for route in inp.case.routes:
        for gin, grad, label in _run_roi(dev, inp, route):
            Cg = grad.shape[1]
            if Cg not in ref:
                ref[Cg] = G.roi_reference(inp, grad)
            _compare(gin, ref[Cg], inp.case, BWD_ATOL, "%s / %s" % (name, label))


@pytest.mark.parametrize("name", [c.name for c in G.ROI_CASES if not c.large])
def test_patch_keyed_gather(dev, name):
    """work mapping (8x1 / 4x2 XCD blocks, several sub-tiles, patches straddling images), every direct-row cap with and
    without rows past it, the producer's rounds / merge / masks -- through every entry point: the (R,C,PH,PW) one, the
    channels-last one, and a plan gathered from twice (C = 4, then C = 8)"""
    _check_roi_case(dev, name)


def test_patch_keyed_gather_without_direct_rows(dev):
    """(1, 1450, 1450): the direct rows would pass 256 MiB, so cap = 0 -- every entry goes through the overflow CSR --
    and the 525625 patches are 257 scan tiles: the two-round scan of the tile totals in its cap / skip_if_zero form"""
    _check_roi_case(dev, "cap0-257-tiles")
    torch.cuda.empty_cache()


def test_kept_workspace_chain_where_patches_straddle_images(dev):
    """workspace_clean = 1 on ONE kept workspace sized for the largest R, on the (3, 5, 7) map: rows past the cap, then
    none, then again; after every call the first jdet_roi_align_backward_clean_bytes() bytes are zero"""
    from jdet_amd import _lib as L
    lib = L.lib()
    N, H, W = G.CHAIN_SHAPE
    PH, PW, s = G.CHAIN_BINS
    sizes = [lib.jdet_roi_align_backward_workspace(O.V_ROT, R, N, 4, H, W, PH, PW, s) for R in G.CHAIN_R]
    wsb = max(sizes)
    assert min(sizes) > 0
    ws = torch.zeros((wsb,), dtype=torch.uint8, device=dev)
    for step in range(3):
        inp = G.chain_inputs(step)
        R = inp.case.R
        clean = lib.jdet_roi_align_backward_clean_bytes(O.V_ROT, R, N, 4, H, W, PH, PW, s)
        assert 0 < clean < wsb
        g, rois = _t(dev, inp.grad.transpose(0, 2, 3, 1)), _t(dev, inp.rois)
        gin = _nan(dev, (N, H, W, 4))
        L.check(lib.jdet_roi_align_backward_cl(O.V_ROT, L.ptr(g), L.ptr(rois), R, N, 4, H, W, PH, PW, 1.0, s, 1,
                                               L.ptr(gin), L.ptr(ws), wsb, 1, L.stream_ptr(g)), "bwd_cl")
        _compare(gin, G.roi_reference(inp), inp.case, None, "chain step %d" % step)
        assert int(ws[:clean].max()) == 0, "step %d left the counters / ticket / overflow flag dirty" % step
