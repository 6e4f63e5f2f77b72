"""CPU: the Gliding Vertex coders (GVDeltaXYWHBBoxCoder, GVFixCoder, GVRatioCoder), the detector's registry names, its
config twin and its parameter names.  The float64 restatement (tests/gliding_ref.py) is pinned by closed forms; the
package's torch composition is held to the restatement in both directions of every coder, clamp rows included.  The
reference's own Jittor programs cannot be run here (Jittor is not importable): restatement and closed forms are the
only pins of the Python tensor programs."""
import math
import os

import numpy as np
import pytest
import torch

from tests import gliding_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEANS, STDS = R.MEANS, R.STDS


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _boxes(rng, n):
    obb = R.random_obbs(rng, n)
    # generic angles: away from the axis-aligned cases, where two vertices share an extreme
    obb[:, 4] = rng.uniform(0.05, math.pi / 2 - 0.05, n) * rng.choice([-1.0, 1.0], n)
    return obb


# ------------------------------------------------------------------------------------------ closed forms
def test_closed_forms_of_the_restatement():
    rng = np.random.default_rng(0)
    obb = _boxes(rng, 4000)
    p = R.rect_poly(obb)
    w, h, t = obb[:, 2], obb[:, 3], obb[:, 4]
    # ratio of a rectangle: its area over the area of its enclosing box
    want = w * h / ((np.abs(w * np.cos(t)) + np.abs(h * np.sin(t))) * (np.abs(w * np.sin(t)) + np.abs(h * np.cos(t))))
    np.testing.assert_allclose(R.ratio_encode(p)[:, 0], want, rtol=0, atol=1e-12)
    # central symmetry: the top and bottom vertex glide by the same fraction, so do right and left
    fix, flat = R.fix_encode(p, with_flags=True)
    assert not flat.any() and not R.has_vertex_tie(p).any()
    np.testing.assert_allclose(fix[:, 0], fix[:, 2], rtol=0, atol=1e-12)
    np.testing.assert_allclose(fix[:, 1], fix[:, 3], rtol=0, atol=1e-12)
    assert np.all((fix > 0) & (fix < 1))
    # decode(enclosing box, encode(p)) = the four vertices of p in top / right / bottom / left order
    back = R.fix_decode(R.poly_hbb(p), fix).reshape(-1, 4, 2)
    pts = p.reshape(-1, 4, 2)
    r = np.arange(len(p))
    order = np.stack(R.extreme_vertices(p), 1)
    np.testing.assert_allclose(back, pts[r[:, None], order], rtol=0, atol=1e-12)


def test_axis_aligned_rectangles_give_fix_one_and_ratio_one():
    rng = np.random.default_rng(1)
    b = np.concatenate([rng.uniform(50, 500, (64, 2)), rng.uniform(510, 950, (64, 2))], 1)
    corners = R.hbb_poly(b).reshape(-1, 4, 2)          # TL, TR, BR, BL
    for shift in range(4):
        p = np.roll(corners, -shift, axis=1).reshape(-1, 8)
        fix, flat = R.fix_encode(p, with_flags=True)
        assert flat.all() and np.all(fix == 1.0), shift
        np.testing.assert_allclose(R.ratio_encode(p), 1.0, rtol=0, atol=1e-12)


def test_delta_codec_round_trip_and_clamps():
    rng = np.random.default_rng(2)
    rois, polys = R.random_rows(rng, 200)
    gts = R.poly_hbb(polys)
    d = R.delta_encode(rois, gts, MEANS, STDS)
    np.testing.assert_allclose(R.delta_decode(rois, d, MEANS, STDS)[:, 0], gts, rtol=0, atol=1e-12)
    big = d.copy()
    big[:, 2] = 1e3                                    # far beyond |log(16/1000)| / std
    w = R.delta_decode(rois, big, MEANS, STDS)[:, 0]
    np.testing.assert_allclose(w[:, 2] - w[:, 0], (rois[:, 2] - rois[:, 0]) * 1000 / 16, rtol=1e-12)
    c = R.delta_decode(rois, big, MEANS, STDS, max_shape=(600, 700))[:, 0]
    assert c[:, [0, 2]].min() >= 0 and c[:, [0, 2]].max() <= 700 and c[:, [1, 3]].max() <= 600


# ------------------------------------------------------------------------------------------ composition = restatement
def _coders():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils.registry import BOXES, build_from_cfg
    return (build_from_cfg(dict(type="GVDeltaXYWHBBoxCoder", target_means=MEANS, target_stds=STDS), BOXES),
            build_from_cfg(dict(type="GVFixCoder"), BOXES), build_from_cfg(dict(type="GVRatioCoder"), BOXES))


def _decode_case(rng, n=96, C=3):
    rois, _ = R.random_rows(rng, n)
    bbox = rng.normal(0, 1.0, (n, 4 * C))
    bbox[0, 2], bbox[1, 3], bbox[2, 6] = 40.0, -40.0, 25.0        # dw / dh on the wh_ratio_clip clamp
    rois[3] = [900.0, 880.0, 1100.0, 1010.0]                      # beyond max_shape: on the border clamp
    rois[4] = [-40.0, -30.0, 60.0, 50.0]
    fix = rng.uniform(0, 1, (n, 4 * C))
    ratio = rng.uniform(0, 1, (n, C))
    ratio[5, :3] = [0.95, 0.2, 0.81][:C]                          # both sides of ratio_thr in one row
    return rois, bbox, fix, ratio


def test_composition_matches_the_restatement_encode():
    delta, fixc, ratioc = _coders()
    rng = np.random.default_rng(3)
    rois, polys = R.random_rows(rng, 400)
    corners = R.hbb_poly(R.poly_hbb(polys[:8]))                   # axis-aligned rows: h_mask and vertex ties
    polys[:8] = corners
    polys[8:12] = np.roll(corners[:4].reshape(-1, 4, 2), -1, axis=1).reshape(-1, 8)
    want_b, want_f, want_r = R.targets(rois, polys, MEANS, STDS)
    np.testing.assert_allclose(delta.encode(_t(rois), _t(R.poly_hbb(polys))).numpy(), want_b, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(fixc.encode(_t(polys)).numpy(), want_f, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ratioc.encode(_t(polys)).numpy(), want_r, rtol=1e-12, atol=1e-12)
    assert np.all(want_f[:12] == 1.0)
    from jdet_amd.models.boxes.coder import gliding_targets
    got = gliding_targets(_t(rois), _t(polys), MEANS, STDS)
    for g, w in zip(got, (want_b, want_f, want_r)):
        assert g.dtype == torch.float64
        np.testing.assert_allclose(g.numpy(), w, rtol=1e-12, atol=1e-12)
    with pytest.raises(NotImplementedError):
        ratioc.decode(None, None)


@pytest.mark.parametrize("max_shape", [None, (1024, 1024)])
def test_composition_matches_the_restatement_decode(max_shape):
    delta, fixc, _ = _coders()
    from jdet_amd.models.boxes.coder import gliding_decode
    rng = np.random.default_rng(4)
    rois, bbox, fix, ratio = _decode_case(rng)
    n, C = ratio.shape
    want_boxes = R.delta_decode(rois, bbox, MEANS, STDS, max_shape)
    got_boxes = delta.decode(_t(rois), _t(bbox), max_shape=max_shape)
    assert tuple(got_boxes.shape) == (n, 4 * C)
    np.testing.assert_allclose(got_boxes.numpy(), want_boxes.reshape(n, -1), rtol=1e-12, atol=1e-12)
    if max_shape is not None:
        assert want_boxes[3, :, 2].max() == 1024 and want_boxes[4, :, 0].min() == 0      # the clamp rows are on it
    if max_shape is None:                                                                 # and the dw clamp row
        assert np.isclose(want_boxes[0, 0, 2] - want_boxes[0, 0, 0], (rois[0, 2] - rois[0, 0]) * 62.5)
    got_polys = fixc.decode(got_boxes, _t(fix))
    np.testing.assert_allclose(got_polys.numpy(), R.fix_decode(want_boxes, fix.reshape(n, C, 4)).reshape(n, -1),
                               rtol=1e-12, atol=1e-12)
    scale = (1.25, 0.8, 1.25, 0.8)
    want = R.decode_polys(rois, bbox, fix, ratio, MEANS, STDS, max_shape, ratio_thr=0.8, scale=scale)
    got = gliding_decode(_t(rois), _t(bbox), _t(fix), _t(ratio), MEANS, STDS, max_shape=max_shape, ratio_thr=0.8,
                         scale=scale)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
    # the ratio_thr rows are the box's own corners
    b = want_boxes[5, 0] / np.asarray(scale)
    np.testing.assert_allclose(want[5, :8], R.hbb_poly(b[None])[0], rtol=1e-12)


def test_composition_is_differentiable_where_the_reference_is():
    delta, fixc, _ = _coders()
    rng = np.random.default_rng(5)
    rois, bbox, fix, _ = _decode_case(rng, n=8, C=2)
    b, f = _t(bbox).requires_grad_(True), _t(fix).requires_grad_(True)
    fixc.decode(delta.decode(_t(rois), b), f).sum().backward()
    assert torch.isfinite(b.grad).all() and torch.isfinite(f.grad).all() and f.grad.abs().sum() > 0


# ------------------------------------------------------------------------------------------ registry, config, names
def test_registry_names():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils import registry as Reg
    for reg, name in ((Reg.MODELS, "GlidingVertex"), (Reg.HEADS, "GlidingRPNHead"), (Reg.HEADS, "GlidingHead"),
                      (Reg.BOXES, "GVDeltaXYWHBBoxCoder"), (Reg.BOXES, "GVFixCoder"), (Reg.BOXES, "GVRatioCoder")):
        assert name in reg, name
    d = Reg.build_from_cfg(dict(type="GVDeltaXYWHBBoxCoder"), Reg.BOXES)
    assert tuple(d.means) == (0., 0., 0., 0.) and tuple(d.stds) == (1., 1., 1., 1.)


@pytest.fixture(scope="module")
def model():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.config import Config
    from jdet_amd.utils import registry as Reg
    c = Config(os.path.join(ROOT, "tests", "golden", "configs", "gliding_r50_fpn_1x_dota_with_flip.yaml"))
    return c, Reg.build_from_cfg(c.model, Reg.MODELS)


def test_config_fixture_equals_the_named_twin(model):
    import jdet_amd.optims  # noqa: F401
    from jdet_amd.config import named
    from tests.golden.gen_configs import plain
    c, m = model
    for sec in ("model", "optimizer", "scheduler"):
        assert plain(c.dump()[sec]) == plain(named.GLIDING_CFG[sec]), sec
    assert type(m).__name__ == "GlidingVertex" and type(m.rpn).__name__ == "GlidingRPNHead"
    assert type(m.bbox_head).__name__ == "GlidingHead"
    assert m.rpn.num_anchors == 3 and m.rpn.rpn_cls.out_channels == 6 and m.rpn.rpn_reg.out_channels == 12
    h = m.bbox_head
    assert h.ratio_thr == 0.8 and h.ratio_loss.loss_weight == 16.0 and abs(h.fix_loss.beta - 1 / 3) < 1e-12
    assert tuple(h.bbox_coder.stds) == (0.1, 0.1, 0.2, 0.2)


def test_parameter_names_match_the_reference(model):
    _, m = model
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes["rpn.rpn_conv.weight"] == (256, 256, 3, 3)
    assert shapes["bbox_head.fc1.weight"] == (1024, 256 * 49)
    assert shapes["bbox_head.fc2.weight"] == (1024, 1024)
    assert shapes["bbox_head.cls_score.weight"] == (16, 1024)
    assert shapes["bbox_head.bbox_pred.weight"] == (60, 1024)
    assert shapes["bbox_head.fix_pred.weight"] == (60, 1024)
    assert shapes["bbox_head.ratio_pred.weight"] == (15, 1024)
    for name in ("rpn.rpn_cls.weight", "rpn.rpn_reg.weight", "bbox_head.fc1.bias", "bbox_head.ratio_pred.bias"):
        assert name in shapes, name


def test_head_refuses_configurations_it_does_not_implement():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils.registry import HEADS, build_from_cfg
    for bad in (dict(start_bbox_type="obb"), dict(end_bbox_type="obb"), dict(with_shared_head=True),
                dict(with_avg_pool=True)):
        with pytest.raises(AssertionError):
            build_from_cfg(dict(type="GlidingHead", **bad), HEADS)
    with pytest.raises(AssertionError):
        build_from_cfg(dict(type="GlidingHead", assigner=dict(
            type="MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, ignore_iof_thr=0.5)), HEADS)


# ------------------------------------------------------------------------------------------ C ABI
def test_gliding_entry_points_validate_before_any_launch():
    from jdet_amd import _lib as L
    import shutil
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        L.build()
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libjdet_hip.so not built")
    lib, N = L.lib(), None
    four = L.vecn([1.0] * 4, 4)
    assert lib.jdet_gliding_targets(N, N, 0, N, N, N, N, N, N) == -1            # means / stds are host arrays
    assert lib.jdet_gliding_targets(N, N, 0, four, four, N, N, N, N) == 0       # n = 0: no-op
    assert lib.jdet_gliding_targets(N, N, 4, four, four, N, N, N, N) == -1      # null pointers
    assert lib.jdet_gliding_targets(N, N, -1, four, four, N, N, N, N) == -1
    assert lib.jdet_gliding_decode(N, N, N, N, 0, 15, four, four, 0.016, 0.0, 0.0, 0.8, four, N, N) == 0
    assert lib.jdet_gliding_decode(N, N, N, N, 4, 15, four, four, 0.016, 0.0, 0.0, 0.8, four, N, N) == -1
    assert lib.jdet_gliding_decode(N, N, N, N, 0, 0, four, four, 0.016, 0.0, 0.0, 0.8, four, N, N) == -1    # ncls < 1
    assert lib.jdet_gliding_decode(N, N, N, N, 0, 15, four, four, 0.016, 0.0, 0.0, 0.8, N, N, N) == -1      # scale
    assert lib.jdet_gliding_decode(N, N, N, N, 0, 15, four, four, 0.0, 0.0, 0.0, 0.8, four, N, N) == -1     # clip
    assert lib.jdet_gv_delta_encode(N, N, 0, four, four, N, N) == 0
    assert lib.jdet_gv_delta_encode(N, N, 3, four, four, N, N) == -1
    assert lib.jdet_gv_delta_decode(N, N, 0, 1, four, four, 0.016, 0.0, 0.0, N, N) == 0
    assert lib.jdet_gv_delta_decode(N, N, 3, 1, four, four, 0.016, 0.0, 0.0, N, N) == -1
    assert lib.jdet_gv_delta_decode(N, N, 0, 0, four, four, 0.016, 0.0, 0.0, N, N) == -1
