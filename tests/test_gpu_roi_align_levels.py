"""GPU: the FPN-routed RoIAlign (ops/_roi_common.MultiLevelRoIAlignFunction) and the single-level dialects at config size
against the reference's OWN kernels (oracle/_ref/libjdet_ref_hip.so through oracle/ref_hip.py).

Expected values are the reference extractors' loop with the reference's kernels inside: the level of every RoI is
computed HERE (float64 numpy, tests/roi_cases.py), the reference kernel runs per level on that level's RoI subset and its
rows are scattered back; the backward likewise with the gradient rows of the level.  The product is called only through
its public modules (the three extractors, the four layers).  Every element of every row is compared; the inputs are
conditioned so that this is fair (tests/roi_cases.py: no level ties, no sample within 1e-4 px of a validity line, the
RoI's half-diagonal <= 45 map pixels -- the lever under which the 1e-4 forward bound of
test_gpu_reference_kernels.py::test_roi_align_full_size_against_the_reference_kernel was derived).

Bounds (measured figures: profiles/roi_align_levels_parity.md):
  forward   horizontal dialects: reference order bit-equal to the reference kernel, merged <= 2e-6;
            trig dialects: <= 1e-4 in both arithmetics (cosf against the rounded double cosine, times the lever, times
            the map's slope), merged within 2e-6 of the reference-order result of the same run;
  backward  <= 1e-4 x max(1, max|ref|) on every element of every level's gradient (float atomics in arbitrary order
            there, sorted-gather sums here); a level without a live RoI: exactly zero.

Allocator poisoning.  The routed forward writes all levels into ONE torch.empty output and every level's gradient is a
torch.empty too.  This module runs the same inputs through several paths back to back, so the caching allocator would
hand a path the block the previous path has just freed -- holding the previous, correct answer -- and a row or a level
that no launch wrote would go unnoticed.  Before each product call the cache is emptied and a NaN-filled tensor of the
output's size and of each level map's size is allocated and freed on the same device and stream: the recycled blocks
then hold NaN, and a skipped row fails the finiteness check and the comparison."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import ref_hip as RH
from tests import roi_cases as RCS

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not RH.available(), reason="oracle/_ref/libjdet_ref_hip.so not built")]

FWD_TRIG_ATOL = 1e-4          # test_gpu_reference_kernels.py's full-size bound; holds under RCS.MAX_LEVER
FWD_MERGED_ATOL = 2e-6        # test_gpu_roi_align.py FWD_MERGED_ATOL
ADAPTIVE_MERGED_ATOL = 2e-6   # default entry against the reference-order result under sampling_ratio = 0: measured 0
BWD_RTOL = 1e-4
HW = (7, 7)
N_ORIENT = 8

_BACKWARD_ENTRIES = ("jdet_roi_align_backward_cl_planned", "jdet_roi_align_backward_cl", "jdet_roi_align_backward")
_FORWARD_ENTRIES = ("jdet_roi_align_forward", "jdet_roi_align_forward_reference", "jdet_roi_align_forward_cl",
                    "jdet_roi_align_forward_cl_reference")


@contextlib.contextmanager
def _counted_entries():
    """counting shims around the library's RoIAlign entry points: which kernels a path really ran"""
    from jdet_amd import _lib as L
    lib = L.lib()
    calls = {n: 0 for n in _BACKWARD_ENTRIES + _FORWARD_ENTRIES}
    real = {n: getattr(lib, n) for n in calls}

    def shim(name):
        def call(*a):
            calls[name] += 1
            return real[name](*a)
        return call

    try:
        for n in calls:
            setattr(lib, n, shim(n))
        yield calls
    finally:
        for n, fn in real.items():
            setattr(lib, n, fn)


@contextlib.contextmanager
def _switches(arithmetic="merged", plan=True, path="roi_cl"):
    from jdet_amd.ops import _roi_common as RC
    prev = (RC.set_arithmetic(arithmetic), RC.set_backward_plan(plan), RC.set_forward_path(path))
    try:
        yield
    finally:
        RC.set_arithmetic(prev[0])
        RC.set_backward_plan(prev[1])
        RC.set_forward_path(prev[2])


def _poison(dev, sizes):
    """see the module docstring"""
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    blocks = [torch.full((int(n),), float("nan"), dtype=torch.float32, device=dev) for n in sizes]
    del blocks


def _maps(dev, N, C, sizes, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return [torch.randn((N, C, s, s), generator=g, device=dev, dtype=torch.float32)
            .contiguous(memory_format=torch.channels_last) for s in sizes]


def _grad(dev, R, C, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn((R, C) + HW, generator=g, device=dev, dtype=torch.float32)


def _extractor(case, dev):
    from jdet_amd.models.roi_extractors import OrientedSingleRoIExtractor, RboxSingleRoIExtractor, SingleRoIExtractor
    strides, d = list(RCS.STRIDES), case["dialect"]
    if d == "rot_v1":
        e = OrientedSingleRoIExtractor(dict(type="ROIAlignRotated_v1", output_size=7, sampling_ratio=2), 256, strides,
                                       extend_factor=(1.4, 1.2))
    elif d == "hbb1":
        e = SingleRoIExtractor(dict(type="ROIAlign", output_size=7, sampling_ratio=2, version=1), 256, strides)
    elif d == "rot":
        e = RboxSingleRoIExtractor(dict(type="ROIAlignRotated", output_size=7, sampling_ratio=2), 256, strides)
    else:
        e = RboxSingleRoIExtractor(dict(type="RiRoIAlign", output_size=7, sample_num=2, nOrientation=N_ORIENT), 256, strides)
    return e.to(dev)


def _reference(kind, feats, scales, krois, lvl, grad, sampling=2):
    """the reference extractors' loop: mask, gather, the reference's kernel on the level's map, scatter back"""
    R, C = krois.shape[0], feats[0].shape[1]
    ref_y = torch.zeros((R, C) + HW, dtype=torch.float32, device=krois.device)
    ref_g = []
    for l, (f, sc) in enumerate(zip(feats, scales)):
        idx = torch.nonzero(lvl == l).flatten()
        if idx.numel() == 0:
            ref_g.append(torch.zeros(tuple(f.shape), dtype=torch.float32, device=f.device) if grad is not None else None)
            continue
        ref_y[idx] = RH.roi_align_forward(kind, f, krois[idx], HW, sc, sampling, N_ORIENT)
        ref_g.append(RH.roi_align_backward(kind, grad[idx], krois[idx], tuple(f.shape), sc, sampling, N_ORIENT)
                     if grad is not None else None)
    return ref_y, ref_g


def _run(module, feats, rois, grad):
    """one product step under allocator poisoning -> (result, [gradient per map] | None, entry-point counts)"""
    dev = rois.device
    sizes = [rois.shape[0] * feats[0].shape[1] * HW[0] * HW[1]] + [f.numel() for f in feats]
    xs = [f.detach().requires_grad_(grad is not None) for f in feats]
    with _counted_entries() as calls:
        _poison(dev, sizes)
        y = module(xs, rois) if len(xs) > 1 else module(xs[0], rois)
        if grad is not None:
            _poison(dev, sizes)
            y.backward(grad)
    torch.cuda.synchronize(dev)
    return y.detach(), ([x.grad for x in xs] if grad is not None else None), dict(calls)


def _report(tag, **figs):
    print("LEVELS %s %s" % (tag, " ".join("%s=%s" % (k, ("%.3e" % v) if isinstance(v, float) else v)
                                          for k, v in figs.items())), flush=True)


def _check_forward(tag, y, ref_y, trig, arithmetic, twin=None, merged_atol=FWD_MERGED_ATOL):
    assert y.shape == ref_y.shape
    finite = bool(torch.isfinite(y).all())
    err = float((y - ref_y).abs().nan_to_num(nan=float("inf")).max())
    share = float((y == ref_y).float().mean())
    d_twin = float((y - twin).abs().nan_to_num(nan=float("inf")).max()) if twin is not None else None
    _report(tag + " fwd/" + arithmetic, err=err, bit_equal=round(share, 4),
            **({"vs_reference_order": d_twin} if twin is not None else {}))
    assert finite, tag + ": rows of the result that no launch wrote (NaN from the poisoned block)"
    if trig:
        assert err <= FWD_TRIG_ATOL, (tag, arithmetic, err)
    elif arithmetic == "reference":
        assert torch.equal(y, ref_y), (tag, err)
    else:
        assert err <= FWD_MERGED_ATOL, (tag, err)
    if twin is not None and trig:
        assert d_twin <= merged_atol, (tag, d_twin)


def _check_backward(tag, grads, ref_g, live):
    worst = 0.0
    for l, (g, r) in enumerate(zip(grads, ref_g)):
        assert g is not None and g.shape == r.shape, (tag, l)
        assert bool(torch.isfinite(g).all()), "%s: level %d gradient has elements no launch wrote" % (tag, l)
        if not live[l]:
            assert int(torch.count_nonzero(g)) == 0, "%s: level %d has no live RoI, its gradient must be zero" % (tag, l)
            continue
        scale = max(1.0, float(r.abs().max()))
        err = float((g - r).abs().max()) / scale
        worst = max(worst, err)
        _report(tag + " bwd level %d" % l, err_over_scale=err, ref_max=float(r.abs().max()))
        assert err <= BWD_RTOL, (tag, l, err)
    return worst


def _multi_inputs(name, dev, seed_offset=0):
    case = RCS.multi_case(name, seed_offset)
    t = lambda a: torch.from_numpy(a).to(dev)
    return case, t(case["rois"]), t(case["krois"]), t(case["lvl"])


@pytest.mark.parametrize("name", ["orcnn-train", "roitrans-hbb", "roitrans-rot", "riroi", "empty-level"])
def test_multi_level_extractor_against_the_reference_kernels(dev, name):
    """the table of the module docstring's cases, every product path on the same inputs:
    default (merged taps, channels-last gradient -> the planned gather per level; RiRoIAlign has no plan: the
    self-contained channels-last backward), reference order (forward), plan off (two steps in a row with different RoI
    sets: the second runs on the workspaces the first handed back), and for rot_v1 the "roi" forward path with a
    contiguous gradient (jdet_roi_align_forward over masked RoIs + jdet_roi_align_backward)."""
    case, rois, krois, lvl = _multi_inputs(name, dev)
    kind, trig = case["dialect"], case["dialect"] in RCS.TRIG
    N, R, C = case["N"], case["R"], 256
    sizes = [RCS.TILE // s for s in RCS.STRIDES]
    scales = [1.0 / s for s in RCS.STRIDES]
    feats = _maps(dev, N, C, sizes, 1000 + case["seed"])
    grad = _grad(dev, R, C, 2000 + case["seed"])
    grad_cl = grad.contiguous(memory_format=torch.channels_last)
    live = case["info"]["per_level"]
    _report(name, per_level=live, moved=case["info"]["moved"], ties=case["info"]["ties"], lever=case["info"]["lever"],
            min_line_dist=case["info"]["min_dist"])
    ref_y, ref_g = _reference(kind, feats, scales, krois, lvl, grad)
    ext = _extractor(case, dev)
    n_lvl = len(sizes)

    # reference order, forward only
    with _switches("reference"):
        y_twin, _, calls = _run(ext, feats, rois, None)
    assert calls["jdet_roi_align_forward_cl_reference"] == n_lvl
    _check_forward(name, y_twin, ref_y, trig, "reference")

    # default
    with _switches():
        y, grads, calls = _run(ext, feats, rois, grad_cl)
    assert y.is_contiguous(memory_format=torch.channels_last) and calls["jdet_roi_align_forward_cl"] == n_lvl
    if kind == "riroi":
        assert calls["jdet_roi_align_backward_cl_planned"] == 0
        assert calls["jdet_roi_align_backward_cl"] + calls["jdet_roi_align_backward"] == n_lvl
    else:
        assert calls["jdet_roi_align_backward_cl_planned"] == n_lvl, calls      # the path training takes
        assert calls["jdet_roi_align_backward_cl"] == 0 and calls["jdet_roi_align_backward"] == 0
    _check_forward(name, y, ref_y, trig, "merged", twin=y_twin)
    _check_backward(name + " default", grads, ref_g, live)

    # plan off: the self-contained backward on the kept workspaces, two steps with different RoI sets in a row
    case2, rois2, krois2, lvl2 = _multi_inputs(name, dev, RCS.SECOND_STEP_SEED)
    ref_y2, ref_g2 = _reference(kind, feats, scales, krois2, lvl2, grad)
    with _switches(plan=False):
        y_a, grads_a, calls_a = _run(ext, feats, rois, grad_cl)
        y_b, grads_b, calls_b = _run(ext, feats, rois2, grad_cl)
    for calls in (calls_a, calls_b):
        assert calls["jdet_roi_align_backward_cl_planned"] == 0
        if kind != "riroi":
            assert calls["jdet_roi_align_backward_cl"] == n_lvl, calls
    assert torch.equal(y_a, y)
    _check_backward(name + " plan-off step 1", grads_a, ref_g, live)
    _check_forward(name + " step 2", y_b, ref_y2, trig, "merged")
    _check_backward(name + " plan-off step 2", grads_b, ref_g2, case2["info"]["per_level"])

    # the (R, C, PH, PW)-contiguous forward over masked RoIs with a null order + the atomics backward
    if name == "orcnn-train":
        with _switches(path="roi"):
            y_r, grads_r, calls = _run(ext, feats, rois, grad)
        assert y_r.is_contiguous() and calls["jdet_roi_align_forward"] == n_lvl
        assert calls["jdet_roi_align_backward"] == n_lvl and calls["jdet_roi_align_backward_cl_planned"] == 0
        _check_forward(name + " roi-path", y_r, ref_y, trig, "merged", twin=y_twin)
        _check_backward(name + " roi-path", grads_r, ref_g, live)


def test_multi_level_inference_proposals_against_the_reference_kernels(dev):
    """orcnn-infer: 2000 proposals per tile, two tiles, forward only, both arithmetics"""
    name = "orcnn-infer"
    case, rois, krois, lvl = _multi_inputs(name, dev)
    sizes = [RCS.TILE // s for s in RCS.STRIDES]
    feats = _maps(dev, case["N"], 256, sizes, 1000 + case["seed"])
    _report(name, per_level=case["info"]["per_level"], moved=case["info"]["moved"], ties=case["info"]["ties"],
            lever=case["info"]["lever"], min_line_dist=case["info"]["min_dist"])
    ref_y, _ = _reference("rot_v1", feats, [1.0 / s for s in RCS.STRIDES], krois, lvl, None)
    ext = _extractor(case, dev)
    with _switches("reference"):
        y_twin, _, _ = _run(ext, feats, rois, None)
    _check_forward(name, y_twin, ref_y, True, "reference")
    with _switches():
        y, _, calls = _run(ext, feats, rois, None)
    assert calls["jdet_roi_align_forward_cl"] == len(sizes)
    _check_forward(name, y, ref_y, True, "merged", twin=y_twin)


def _single_layer(dialect, sampling):
    from jdet_amd.ops.riroi_align import RiRoIAlign
    from jdet_amd.ops.roi_align import ROIAlign
    from jdet_amd.ops.roi_align_rotated_v1 import ROIAlignRotated_v1
    if dialect == "rot_v1":
        return ROIAlignRotated_v1(7, 0.25, sampling)
    if dialect == "riroi":
        return RiRoIAlign(7, 0.25, sampling, N_ORIENT)
    return ROIAlign(7, 0.25, sampling, version=1 if dialect == "hbb1" else 0)


SINGLE = [("rot_v1", 2000, 2, 11), ("hbb0", 2000, 2, 12), ("hbb1", 2000, 2, 13), ("riroi", 2000, 2, 14),
          ("rot_v1", 512, 0, 21), ("hbb0", 512, 0, 22)]


@pytest.mark.parametrize("dialect,R,sampling,seed", SINGLE,
                         ids=["%s-%d-s%d" % (d, r, s) for d, r, s, _ in SINGLE])
def test_single_level_dialects_at_full_size_against_the_reference_kernels(dev, dialect, R, sampling, seed):
    """the rows test_roi_align_full_size_against_the_reference_kernel lacks: rot_v1, hbb0, hbb1, riroi (32 x 8 planes) on
    the 1 x 256 x 256 x 256 map with 2000 RoIs at sampling 2, and rot_v1 / hbb0 with sampling_ratio = 0 (the grid follows
    the RoI's size: up to 10 x 10 taps per bin; no plan exists for it: the self-contained channels-last backward).
    Default against reference-order arithmetic under adaptive sampling: measured 0.0 at grids up to 10 x 10 for both
    dialects -- the tap merge exists for sample_num == 2 only, the default entry runs the reference's chain otherwise
    (csrc/roi_align_fwd.h) -- so the 2e-6 of the fixed grids is kept as the bound."""
    case = RCS.single_case(dialect, R, sampling, seed)
    trig = dialect in RCS.TRIG
    rois = torch.from_numpy(case["rois"]).to(dev)
    feats = _maps(dev, 1, 256, [256], 1000 + seed)
    grad = _grad(dev, R, 256, 2000 + seed)
    grad_cl = grad.contiguous(memory_format=torch.channels_last)
    tag = "single-%s-%d-s%d" % (dialect, R, sampling)
    _report(tag, moved=case["info"]["moved"], lever=case["info"]["lever"], grid=case["info"]["grid"],
            min_line_dist=case["info"]["min_dist"])
    ref_y, ref_g = _reference(dialect, feats, [0.25], rois, torch.zeros(R, dtype=torch.int64, device=dev), grad, sampling)
    layer = _single_layer(dialect, sampling)
    with _switches("reference"):
        y_twin, _, _ = _run(layer, feats, rois, None)
    _check_forward(tag, y_twin, ref_y, trig, "reference")
    with _switches():
        y, grads, calls = _run(layer, feats, rois, grad_cl)
    planned = dialect != "riroi" and sampling > 0
    assert calls["jdet_roi_align_backward_cl_planned"] == (1 if planned else 0), calls
    assert calls["jdet_roi_align_backward_cl"] + calls["jdet_roi_align_backward"] == (0 if planned else 1), calls
    d_twin = float((y - y_twin).abs().max())
    _check_forward(tag, y, ref_y, trig, "merged", twin=y_twin,
                   merged_atol=ADAPTIVE_MERGED_ATOL if sampling == 0 else FWD_MERGED_ATOL)
    if sampling == 0:
        assert d_twin <= ADAPTIVE_MERGED_ATOL, d_twin       # horizontal dialect too: same-run twin
    _check_backward(tag, grads, ref_g, [R])
