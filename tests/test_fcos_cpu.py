"""CPU: the rotated FCOS pieces that need no device -- mintheta_obb, distance2obb and the general route of
FCOSHead.get_targets against the float64 restatement (tests/fcos_ref.py); the round trip target -> box; the fixtures'
conditions; the names in SIGNATURES; the argument checks of both entry points; the registry names and
FCOS_CFG; closed forms of the loss restatement."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import fcos_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def _max_coord(gts):
    """largest coordinate magnitude of a target fixture: image extent, box centres and sizes"""
    return max([float(R.IMG)] + [float(np.abs(g[:, :4]).max()) for g in gts if len(g)])


def _head(norm_on_bbox=True, center_sampling=False):
    from jdet_amd.models.roi_heads.fcos_head import FCOSHead
    return FCOSHead(num_classes=R.NUM_CLASSES, in_channels=8, feat_channels=32, stacked_convs=1, strides=list(R.STRIDES),
                    regress_ranges=R.RANGES, norm_on_bbox=norm_on_bbox, center_sampling=center_sampling,
                    center_sample_radius=R.RADIUS)


@pytest.mark.parametrize("name", sorted(R.TARGET_FIXTURES))
def test_target_fixture_holds_the_conditions(name):
    gts, labels = R.target_fixture(name)
    for b, (g, lab) in enumerate(zip(gts, labels)):
        for cs in (False, True):
            ref = R.targets(g, lab, True, cs)
            print("%s image %d K %d center_sampling %d: margin %.2e px, theta gap %.2e, positives %d, levels %s"
                  % (name, b, len(g), cs, ref["margin"], ref["theta_gap"], ref["positives"],
                     np.bincount(R.points_of()[1][ref["inds"] >= 0], minlength=5).tolist()))
            if len(g) == 0:
                assert ref["positives"] == 0 and (ref["labels"] == R.NUM_CLASSES).all()
                continue
            assert ref["margin"] >= 1e-3 and ref["theta_gap"] >= 1e-5
            assert ref["positives"] >= 1
        if len(g) > 1:
            # center sampling decides something here: it removes positives on more than one level, and in the 70-gt image
            # it also hands points to another (larger) gt
            off, on = R.targets(g, lab, True, False), R.targets(g, lab, True, True)
            lvl = R.points_of()[1]
            lost = np.bincount(lvl[off["inds"] >= 0], minlength=5) - np.bincount(lvl[on["inds"] >= 0], minlength=5)
            switched = int(((off["inds"] != on["inds"]) & (on["inds"] >= 0)).sum())
            print("%s image %d: center sampling removes %s positives per level, %d points change winner"
                  % (name, b, lost.tolist(), switched))
            assert (off["labels"] != on["labels"]).any() and (lost >= 0).all() and (lost > 0).sum() > 1
            assert switched >= 1 or name != "k70"
        areas = (g[:, 2] * g[:, 3]) if len(g) else np.zeros(0, np.float32)
        if name == "tie":
            assert np.array_equal(g[2], g[4]) and labels[0][2] != labels[0][4]
            assert len(np.unique(areas)) == len(g) - 1
            ref = R.targets(g, lab, True, False)
            assert (ref["inds"] == 2).sum() > 0 and (ref["inds"] == 4).sum() == 0
        else:
            assert len(np.unique(areas)) == len(g)
    assert R.points_of()[0].shape == (341, 2)
    if name == "k70":
        from jdet_amd import _lib
        chunk = int(re.search(r"#define JDET_FCOS_GT_CHUNK (\d+)", open(os.path.join(ROOT, "include",
                                                                                    "jdet_hip.h")).read()).group(1))
        assert len(gts[0]) > chunk and _lib is not None


def test_loss_fixture_holds_the_conditions():
    prd, tgt, passed = R.loss_fixture()
    ref, e_loss, e_grad = R.loss_reference()
    print("loss fixture: %d rows, %.0f %% of the drawn pairs pass; min IoU %.3f; float32 restatement against float64: "
          "loss %.2e, gradient %.2e of the row's max |g|" % (len(prd), 100 * passed, ref["iou"].min(), e_loss, e_grad))
    assert prd.shape == tgt.shape == (R.LOSS_ROWS, 5) and ref["iou"].min() >= 0.05
    assert 0 < e_loss < 1e-3 and 0 < e_grad < 1e-2
    assert np.isfinite(ref["grad"]).all() and (np.abs(ref["grad"]).max(1) > 0).all()
    hull = (ref["index"] >= 0).sum(1) - 1
    assert hull.min() >= 3 and hull.max() <= 8


def test_mintheta_obb_and_distance2obb_match_the_restatement():
    from jdet_amd.models.boxes.box_ops import distance2obb, mintheta_obb
    g = R.target_fixture("k70")[0][0]
    want, gap = R.mintheta_obb(g)
    got = mintheta_obb(torch.from_numpy(g.copy())).numpy()
    assert got.dtype == np.float32 and np.abs(gap).min() >= 1e-5
    np.testing.assert_array_equal(got[:, :4], want[:, :4].astype(np.float32))
    np.testing.assert_allclose(got[:, 4], want[:, 4], rtol=0, atol=4 * _ulp(math.pi))
    assert (np.abs(got[:, 4]) <= math.pi / 4 + 1e-5).all()
    # distance2obb: centre = point + R^T (r - l, b - t) / 2, size = (l + r, t + b), then regular_obb
    pts = torch.tensor([[10.0, 20.0], [50.0, 60.0]], dtype=torch.float64)
    d = torch.tensor([[3.0, 1.0, 5.0, 2.0, 0.4], [1.0, 6.0, 2.0, 8.0, -0.3]], dtype=torch.float64)
    out = distance2obb(pts, d).numpy()
    for (x, y), (l, t, r, b, th), o in zip(pts.numpy(), d.numpy(), out):
        ox, oy = (r - l) / 2, (b - t) / 2
        cx, cy = x + math.cos(th) * ox + math.sin(th) * oy, y - math.sin(th) * ox + math.cos(th) * oy
        w, h = l + r, t + b
        if w > h:
            exp = [cx, cy, w, h, th]
        else:
            exp = [cx, cy, h, w, (th + math.pi / 2 + math.pi / 2) % math.pi - math.pi / 2]
        np.testing.assert_allclose(o, exp, rtol=0, atol=1e-12)


@pytest.mark.parametrize("norm_on_bbox,center_sampling", [(True, False), (False, True)])
@pytest.mark.parametrize("name", ["k7_k0", "k70", "tie"])
def test_general_route_targets_match_the_restatement_and_round_trip(name, norm_on_bbox, center_sampling):
    from jdet_amd.models.boxes.box_ops import distance2obb, mintheta_obb
    from jdet_amd.ops.bbox_transforms import regular_obb
    gts, labels = R.target_fixture(name)
    head = _head(norm_on_bbox, center_sampling)
    points = head.get_points(list(R.SIZES), torch.float32)
    assert np.array_equal(torch.cat(points).numpy(), R.points_of()[0].astype(np.float32))
    targets = [dict(rboxes=torch.from_numpy(g.copy()), labels=torch.from_numpy(lab.copy())) for g, lab in zip(gts, labels)]
    lab_lv, tgt_lv = head.get_targets(points, targets, dense=False)
    B, n_lv = len(gts), [h * w for h, w in R.SIZES]
    assert [t.shape[0] for t in lab_lv] == [B * n for n in n_lv] and lab_lv[0].dtype == torch.int32
    tol = 8 * _ulp(_max_coord(gts))
    for b, (g, lab) in enumerate(zip(gts, labels)):
        ref = R.targets(g, lab, norm_on_bbox, center_sampling)
        got_lab = torch.cat([t.view(B, -1)[b] for t in lab_lv]).numpy()
        got_tgt = torch.cat([t.view(B, -1, 5)[b] for t in tgt_lv]).numpy()
        assert np.array_equal(got_lab, ref["labels"])
        err = np.abs(got_tgt - ref["bbox_targets"]).max()
        print("%s image %d: max target error %.2e (bound %.2e)" % (name, b, err, tol))
        assert err <= tol
        pos = np.flatnonzero(ref["inds"] >= 0)
        if not len(pos):
            assert (got_tgt == 0).all()
            continue
        # round trip in float64 on the restatement's targets: distance2obb gives back regular_obb(mintheta_obb(gt))
        pts, lvl = R.points_of()
        t = ref["bbox_targets"][pos].copy()
        if norm_on_bbox:
            t[:, :4] *= np.asarray(R.STRIDES, np.float64)[lvl[pos]][:, None]
        back = distance2obb(torch.from_numpy(pts[pos]), torch.from_numpy(t)).numpy()
        want = regular_obb(mintheta_obb(torch.from_numpy(g.astype(np.float64)))).numpy()[ref["inds"][pos]]
        np.testing.assert_allclose(back, want, rtol=0, atol=1e-9)
        assert np.array_equal(head.centerness_target(torch.from_numpy(ref["bbox_targets"][pos])).numpy() > 0,
                              np.ones(len(pos), bool))
        np.testing.assert_allclose(head.centerness_target(torch.from_numpy(ref["bbox_targets"][pos])).numpy(),
                                   ref["centerness"][pos], rtol=1e-12)


@pytest.fixture(scope="module")
def built_lib():
    from jdet_amd import _lib
    _lib.build()
    return _lib


def test_header_signatures_and_exports_agree(built_lib):
    assert {"jdet_fcos_targets", "jdet_poly_iou_loss"} <= set(built_lib.SIGNATURES)


def test_argument_checks_return_before_any_launch(built_lib):
    lib = built_lib.lib()
    N, X = None, 4096                                        # X: a non-null address nobody reads
    lv = (ctypes.c_int32 * 6)(4, 4, 8, 2, 2, 16)
    rr = (ctypes.c_float * 4)(-1, 64, 64, 1e8)

    def tg(levels=lv, ranges=rr, L=2, gt=X, gl=X, gc=X, B=2, K=3, C=15, cs=0, radius=1.5, lab=X, bt=X, ct=X, gi=N):
        return lib.jdet_fcos_targets(levels, ranges, L, gt, gl, gc, B, K, C, 1, cs, radius, lab, bt, ct, gi, N)
    for null in ("levels", "ranges", "gt", "gl", "gc", "lab", "bt", "ct"):
        assert tg(**{null: N}) == -1, null
    assert tg(B=0) == -1 and tg(K=-1) == -1 and tg(L=0) == -1 and tg(C=0) == -1
    assert tg(levels=(ctypes.c_int32 * 6)(4, 0, 8, 2, 2, 16)) == -1          # W = 0
    assert tg(levels=(ctypes.c_int32 * 6)(4, 4, 8, 2, 2, 0)) == -1           # stride = 0
    assert tg(cs=1, radius=0.0) == -1 and tg(cs=1, radius=float("nan")) == -1 and tg(cs=1, radius=float("inf")) == -1
    assert tg(L=9, levels=(ctypes.c_int32 * 27)(*([1, 1, 1] * 9)), ranges=(ctypes.c_float * 18)()) == -2
    assert tg(B=65536) == -2
    assert tg(levels=(ctypes.c_int32 * 6)(40000, 40000, 1, 2, 2, 16)) == -2  # B * N beyond 2^31 - 1

    def pl(pred=X, target=X, w=N, P=5, eps=1e-6, loss=X, grad=X):
        return lib.jdet_poly_iou_loss(pred, target, w, P, 0, eps, loss, grad, N)
    for null in ("pred", "target", "loss", "grad"):
        assert pl(**{null: N}) == -1, null
    assert pl(P=-1) == -1 and pl(eps=0.0) == -1 and pl(eps=-1e-6) == -1 and pl(eps=float("nan")) == -1
    assert pl(P=0, pred=N, target=N, loss=N, grad=N) == 0    # nothing to do, nothing launched


def test_registry_builds_the_loss_the_head_and_the_model():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.config.named import FCOS_CFG
    from jdet_amd.utils import registry as Reg
    loss = Reg.build_from_cfg(dict(type="PolyIoULoss", loss_weight=2.0, linear=True), Reg.LOSSES)
    assert loss.linear is True and loss.eps == 1e-6 and loss.loss_weight == 2.0 and loss.reduction == "mean"
    h = Reg.build_from_cfg(FCOS_CFG["model"]["roi_heads"], Reg.HEADS)
    assert type(h).__name__ == "FCOSHead" and type(h.loss_bbox).__name__ == "PolyIoULoss"
    assert h.norm_on_bbox is True and h.center_sampling is False and h.test_cfg.centerness_factor == 0.5
    names = {n for n, _ in h.named_parameters()}
    # the reference's names (cls_convs.0.conv / .gn, conv_cls, conv_reg, conv_centerness, conv_theta, scales.N.scale)
    for n in ("cls_convs.0.conv.weight", "cls_convs.3.gn.weight", "reg_convs.3.gn.bias", "conv_cls.bias",
              "conv_reg.weight", "conv_centerness.weight", "conv_theta.bias", "scales.4.scale", "scale_t.scale"):
        assert n in names, n
    assert "cls_convs.0.conv.bias" not in names              # conv_bias "auto" under GroupNorm
    assert h.conv_cls.weight.shape == (15, 256, 3, 3) and h.conv_reg.weight.shape == (4, 256, 3, 3)
    assert abs(float(h.conv_cls.bias.detach()[0]) + math.log(99.0)) < 1e-5
    m = Reg.build_from_cfg(FCOS_CFG["model"], Reg.MODELS)
    assert type(m).__name__ == "FCOS" and type(m.bbox_head).__name__ == "FCOSHead" and m.neck is not None
    assert isinstance(m, Reg.MODELS.get("SingleStageDetector"))
    m.eval()
    m.train()
    assert m.training and m.backbone.training and m.bbox_head.training
    assert FCOS_CFG["optimizer"]["lr"] == 0.0025 and FCOS_CFG["optimizer"]["grad_clip"]["max_norm"] == 35


def test_head_and_loss_refuse_host_tensors_on_the_device_only_paths():
    from jdet_amd._lib import JDetHipError
    from jdet_amd.models.losses.poly_iou_loss import poly_iou_loss
    from jdet_amd.models.roi_heads.fcos_head import fcos_targets_device
    prd, tgt, _ = R.loss_fixture()
    with pytest.raises(JDetHipError):                        # the general route's hull step is a device kernel
        poly_iou_loss(torch.from_numpy(prd.copy()), torch.from_numpy(tgt.copy()))
    with pytest.raises(JDetHipError):
        fcos_targets_device(list(R.SIZES), R.STRIDES, R.RANGES, torch.zeros((1, 2, 5)),
                            torch.zeros((1, 2), dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 15)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_closed_forms_of_the_loss_restatement(dtype):
    # float64: exact up to eps / area; float32: a dozen roundings of coordinates ~100 (ulp 7.6e-6) on sizes >= 10
    tol = 1e-7 if dtype == torch.float64 else 1e-5
    for name, (p, t, iou) in R.CLOSED_FORMS.items():
        r = R.poly_iou_loss(np.asarray([p], np.float32), np.asarray([t], np.float32), dtype=dtype)
        print(name, dtype, float(r["iou"][0]), iou)
        assert abs(float(r["iou"][0]) - iou) <= tol, name
        assert abs(float(r["loss"][0]) + math.log(iou)) <= tol / iou + tol, name
        lin = R.poly_iou_loss(np.asarray([p], np.float32), np.asarray([t], np.float32), linear=True, dtype=dtype)
        assert abs(float(lin["loss"][0]) - (1 - iou)) <= tol, name
    r = R.poly_iou_loss(np.asarray([R.DISJOINT[0]], np.float32), np.asarray([R.DISJOINT[1]], np.float32), dtype=dtype)
    assert float(r["iou"][0]) == pytest.approx(1e-6, rel=1e-6) and (r["grad"] == 0).all()
    assert float(r["loss"][0]) == pytest.approx(-math.log(1e-6), rel=1e-6)
    assert not r["masks"].any()
    # the gradient of the contained pair: iou = a1 / a2, so d(-log iou) / d(w, h) = -(1 / w, 1 / h), nothing else moves
    r = R.poly_iou_loss(np.asarray([R.CLOSED_FORMS["contained"][0]], np.float32),
                        np.asarray([R.CLOSED_FORMS["contained"][1]], np.float32), dtype=dtype)
    np.testing.assert_allclose(r["grad"][0], [0, 0, -1 / 20.0, -1 / 10.0, 0], rtol=0, atol=1e-4 if dtype == torch.float32
                               else 1e-8)
