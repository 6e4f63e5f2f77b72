"""CPU: the Gaussian box losses (GDLoss, GDLoss_v1, KFLoss), KFIoURRetinaHead, FakeBboxOverlaps2D_rotated and the three
RotatedRetinaNet configs that use them.  The float64 restatement (tests/gaussian_loss_ref.py) is pinned by closed forms;
the package's torch composition is held to the restatement on every kind x fun x tau branch, clamp rows included."""
import math
import os

import numpy as np
import pytest
import torch

from tests import gaussian_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kind, constructor, restatement keywords
BRANCHES = (
    [("gwd", dict(type="GDLoss", loss_type="gwd", fun=f, tau=tau), dict(fun=f, tau=tau))
     for f in ("log1p", "sqrt", "none") for tau in (0.0, 1.0)]
    + [("gwd", dict(type="GDLoss", loss_type="gwd", fun="log1p", alpha=2.0, normalize=False),
        dict(fun="log1p", tau=0.0, alpha=2.0, normalize=False))]
    + [(k, dict(type="GDLoss", loss_type=k, fun=f, tau=tau), dict(fun=f, tau=tau))
       for k in ("kld", "jd", "kld_symmax", "kld_symmin") for f in ("log1p", "none") for tau in (0.0, 1.0)]
    + [(k, dict(type="GDLoss", loss_type=k, fun="sqrt", tau=1.0, sqrt=False), dict(fun="sqrt", tau=1.0, sqrt=False))
       for k in ("kld", "jd", "kld_symmax")]
    + [(k + "_v1", dict(type="GDLoss_v1", loss_type=k, fun=f, tau=tau), dict(fun=f, tau=tau))
       for k in ("gwd", "kld", "bcd") for f in ("log1p", "sqrt", "") for tau in (1.0, 2.0)]
    + [("kfiou", dict(type="KFLoss", fun=f), dict(fun=f)) for f in ("none", "ln", "exp")]
)
# the restatement's keyword for GDLoss_v1's '' function is anything but log1p / sqrt
_REF_FUN = {"": "plain"}


def _build(cfg):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils.registry import LOSSES, build_from_cfg
    return build_from_cfg(dict(cfg), LOSSES)


def _rows(rng, n, decoded_scale=0.4):
    """anchors, delta preds / targets (float64) with a few rows on the clamps: dw / dh beyond |log(16/1000)|, w = h,
    angle wrap"""
    anchors = np.concatenate([rng.uniform(0, 512, (n, 2)), np.exp(rng.uniform(np.log(8), np.log(256), (n, 2))),
                              rng.uniform(-math.pi / 4, 3 * math.pi / 4, (n, 1))], 1)
    deltas = rng.normal(0, decoded_scale, (n, 5))
    target = rng.normal(0, decoded_scale, (n, 5))
    deltas[0, 2], deltas[1, 3], deltas[2, 2] = 6.0, -6.0, -4.5      # dw / dh clamp
    anchors[3, 3] = anchors[3, 2]                                   # square anchor
    deltas[3, 2] = deltas[3, 3] = target[3, 2] = target[3, 3] = 0.0  # w = h on both sides
    deltas[4, 4] = 0.74                                             # angle wraps through norm_angle
    anchors[5, 4] = 3 * math.pi / 4 - 1e-3
    return anchors, deltas, target


def test_closed_forms_of_the_restatement():
    rng = np.random.default_rng(0)
    b = torch.tensor(np.concatenate([rng.uniform(0, 100, (32, 2)), rng.uniform(4, 60, (32, 2)),
                                     rng.uniform(-1.5, 1.5, (32, 1))], 1), dtype=R.D)
    b2 = b.clone()
    b2[:, 2:4] = torch.tensor(rng.uniform(4, 60, (32, 2)), dtype=R.D)      # concentric, same angle, other w / h
    want = ((b[:, 2] - b2[:, 2]) ** 2 + (b[:, 3] - b2[:, 3]) ** 2) / 4
    xy, whr, _ = R.gwd_v0_terms(R.gauss(b), R.gauss(b2))
    torch.testing.assert_close(xy + whr, want, rtol=1e-9, atol=1e-9)
    dis, _ = R.gwd_v1_dis(R.gauss(b), R.gauss(b2))
    torch.testing.assert_close(dis, want, rtol=1e-9, atol=1e-9)
    # GDLoss_v1 kld of identical boxes: 0 before its clamp
    torch.testing.assert_close(R.kld_v1_dis(R.gauss(b), R.gauss(b)), torch.zeros(32, dtype=R.D), rtol=0, atol=1e-9)
    # GDLoss kld of identical boxes: 1/det(Sigma) - 1, det = (wh/4)^2 (inv divided by det twice, as written)
    det = (b[:, 2] * b[:, 3] / 4) ** 2
    torch.testing.assert_close(R.kld_v0_raw(R.gauss(b), R.gauss(b), sqrt=False), 1 / det - 1, rtol=1e-9, atol=1e-12)
    # KFIoU of identical boxes: 1/3 (up to eps); KFLoss(fun='none') = 2/3
    _, kf = R.kfiou_terms(b, b, b, b)
    torch.testing.assert_close(kf, torch.full((32,), 1 / 3, dtype=R.D), rtol=0, atol=1e-6)
    torch.testing.assert_close(R.kfiou(b, b, b, b, "none"), torch.full((32,), 2 / 3, dtype=R.D), rtol=0, atol=1e-6)


@pytest.mark.parametrize("kind,cfg,kw", BRANCHES, ids=[f"{c['type']}-{k}-{i}" for i, (k, c, _) in enumerate(BRANCHES)])
def test_composition_matches_the_restatement(kind, cfg, kw):
    """the package's torch composition (float64 on the host) = the restatement: value and gradient, decoded rows with
    ~30 % positives, rows on the dw / dh clamp, w = h, angle wrap"""
    from jdet_amd.models.boxes.coder import DeltaXYWHABBoxCoder
    loss = _build(cfg)
    rng = np.random.default_rng(1)
    n = 96
    anchors, deltas, target = _rows(rng, n)
    weight = np.zeros((n, 5))
    weight[rng.uniform(size=n) < 0.3] = 1.0
    weight[:6] = 1.0
    coder = DeltaXYWHABBoxCoder()
    ref_kw = dict(kw)
    ref_kw["fun"] = _REF_FUN.get(ref_kw.get("fun"), ref_kw.get("fun"))
    if kind != "kfiou":
        tgt = R.delta2bbox(torch.tensor(anchors), torch.tensor(target)).numpy()    # decoded gt boxes
        want, gwant = R.masked_loss_and_grad(kind, deltas, tgt, weight, 7.0, cfg.get("loss_weight", 1.0),
                                             anchors=anchors, decode_pred=True, **ref_kw)
    else:
        tgt = target
        want, gwant = R.masked_loss_and_grad(kind, deltas, tgt, weight, 7.0, 1.0, anchors=anchors, **ref_kw)
    p = torch.tensor(deltas, dtype=torch.float64, requires_grad=True)
    got = loss.level(p, torch.tensor(anchors), torch.tensor(tgt), torch.tensor(weight), 7.0, coder, kind != "kfiou")
    got.backward()
    assert abs(float(got) - want) <= 1e-9 * max(1.0, abs(want)), (float(got), want)
    np.testing.assert_allclose(p.grad.numpy(), gwant, rtol=1e-7, atol=1e-9 * max(1.0, np.abs(gwant).max()))


def test_no_positive_row_gives_zero_and_zero_gradient():
    for cfg in (dict(type="GDLoss", loss_type="gwd"), dict(type="GDLoss_v1", loss_type="kld", fun="log1p"),
                dict(type="KFLoss")):
        loss = _build(cfg)
        p = torch.randn(10, 5, dtype=torch.float64, requires_grad=True)
        t = torch.randn(10, 5, dtype=torch.float64)
        args = (p, t, p, t) if cfg["type"] == "KFLoss" else (p, t)
        out = loss(*args, weight=torch.zeros(10, 5, dtype=torch.float64), avg_factor=3.0)
        out.backward()
        assert float(out) == 0.0 and torch.all(p.grad == 0)


def test_gradcheck_of_the_composition():
    from jdet_amd.models.losses import gaussian_dist_loss as G
    from jdet_amd.models.losses.kf_iou_loss import kfiou_loss
    rng = np.random.default_rng(2)
    box = lambda n: torch.tensor(np.concatenate([rng.uniform(0, 50, (n, 2)), rng.uniform(5, 30, (n, 2)),  # noqa: E731
                                                 rng.uniform(-1.5, 1.5, (n, 1))], 1), dtype=torch.float64)
    t = box(6)
    for fn in (lambda p: G.gwd_loss(G.xy_wh_r_2_xy_sigma(p), G.xy_wh_r_2_xy_sigma(t), fun="log1p", tau=1.0),
               lambda p: G.kld_loss(G.xy_wh_r_2_xy_sigma(p), G.xy_wh_r_2_xy_sigma(t), fun="none", tau=0, sqrt=False),
               lambda p: G.jd_loss(G.xy_wh_r_2_xy_sigma(p), G.xy_wh_r_2_xy_sigma(t), fun="none", tau=0, sqrt=False),
               lambda p: G.gwd_loss_v1(G.xy_wh_r_2_xy_sigma(p), G.xy_wh_r_2_xy_sigma(t)),
               lambda p: G.kld_loss_v1(G.xy_wh_r_2_xy_sigma(p), G.xy_wh_r_2_xy_sigma(t)),
               lambda p: G.bcd_loss_v1(G.xy_wh_r_2_xy_sigma(p), G.xy_wh_r_2_xy_sigma(t)),
               lambda p: kfiou_loss(p * 0.01, t * 0.01, p, t, fun="ln")):
        assert torch.autograd.gradcheck(fn, (box(6).requires_grad_(True),), eps=1e-6, atol=1e-5)


def test_kfiou_nonpositive_det_gives_zero_gradient_not_nan():
    """the decided rule where rounding makes det(Sigma) <= 0: Vb = 0 as the reference's `where(isnan(Vb), 0, Vb)`, with a
    zero gradient where the plain composition back-propagates NaN (negative) or inf (zero); the kernel applies the same
    rule (csrc/gaussian_loss.hip: kfiou)"""
    from jdet_amd.models.losses.kf_iou_loss import kf_volume
    det = torch.tensor([-1e-12, 0.0, 4.0], dtype=torch.float64, requires_grad=True)
    v = kf_volume(det)
    v.sum().backward()
    assert v.tolist() == [0.0, 0.0, 8.0] and det.grad.tolist() == [0.0, 0.0, 1.0]
    plain = torch.tensor([-1e-12, 0.0], dtype=torch.float64, requires_grad=True)
    vb = 4 * plain.sqrt()
    torch.where(torch.isnan(vb), torch.zeros_like(vb), vb).sum().backward()
    assert not torch.isfinite(plain.grad).any()          # what the rule replaces


def test_fake_overlaps_conversion_matches_the_restatement():
    from jdet_amd.models.boxes.iou_calculator import fake_rotated_boxes
    rng = np.random.default_rng(3)
    b = np.concatenate([rng.uniform(0, 500, (200, 2)), rng.uniform(2, 200, (200, 2)),
                        rng.uniform(-math.pi, math.pi, (200, 1))], 1).astype(np.float32)
    b[:4, 4] = [0.0, math.pi / 2, -math.pi / 2, 0.3]      # w >= h flips; a square: equal extents, flag w >= h
    b[3, 2:4] = 10.0
    got = fake_rotated_boxes(torch.from_numpy(b)).numpy()
    want = R.fake_rotated_boxes(b)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-3)
    assert np.all(got[:, 2] >= got[:, 3]) and set(np.unique(got[:, 4])) <= {0.0, np.float32(-math.pi / 2)}


def test_registry_names_and_config_fixtures():
    import jdet_amd.models  # noqa: F401
    import jdet_amd.optims  # noqa: F401
    from jdet_amd.config import Config, named
    from jdet_amd.utils import registry as Reg
    for reg, name in ((Reg.LOSSES, "GDLoss"), (Reg.LOSSES, "GDLoss_v1"), (Reg.LOSSES, "KFLoss"),
                      (Reg.HEADS, "KFIoURRetinaHead"), (Reg.BOXES, "FakeBboxOverlaps2D_rotated")):
        assert name in reg, name
    from tests.golden.gen_configs import plain
    for stem, twin, head, loss in (
            ("rotated_retinanet_hbb_gwd_r50_fpn_1x_dota", named.GWD_RETINANET_CFG, "RotatedRetinaHead", "GDLoss"),
            ("rotated_retinanet_hbb_kld_r50_fpn_1x_dota", named.KLD_RETINANET_CFG, "RotatedRetinaHead", "GDLoss_v1"),
            ("rotated_retinanet_hbb_kfiou_r50_fpn_1x_dota", named.KFIOU_RETINANET_CFG, "KFIoURRetinaHead", "KFLoss")):
        c = Config(os.path.join(ROOT, "tests", "golden", "configs", stem + ".yaml"))
        for sec in ("model", "optimizer", "scheduler"):
            assert plain(c.dump()[sec]) == plain(twin[sec]), (stem, sec)
        m = Reg.build_from_cfg(c.model, Reg.MODELS)
        assert type(m).__name__ == "RotatedRetinaNet" and type(m.bbox_head).__name__ == head
        assert type(m.bbox_head.loss_bbox).__name__ == loss
        assert m.bbox_head.train_cfg.assigner.iou_calculator.type == "FakeBboxOverlaps2D_rotated"
    assert named.GWD_RETINANET_CFG["model"]["bbox_head"]["train_cfg"]["reg_decoded_bbox"] is True
    assert named.KFIOU_RETINANET_CFG["model"]["bbox_head"]["train_cfg"]["reg_decoded_bbox"] is False
    g = _build(dict(type="GDLoss", loss_type="gwd", loss_weight=5.0))
    assert g.tau == 0.0 and g.fun == "log1p" and g.kwargs.get("normalize", True)      # GDLoss defaults


def test_new_entry_points_validate_before_any_launch():
    from jdet_amd import _lib as L
    import shutil
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        L.build()
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libjdet_hip.so not built")
    lib, N = L.lib(), None
    q = L.GaussianLossParams()
    assert lib.jdet_gaussian_loss_level(N, N, 1, 1, N, 1, 1, N, 0, 0, q, N, 1.0, N, N, N, 0, N) == -1   # rows = 0
    q.kind = 9
    assert lib.jdet_gaussian_loss_level(1, 1, 1, 1, N, 1, 1, N, 0, 4, q, 1, 1.0, 1, 1, 1, 4096, N) == -1  # kind
    q.kind, q.decode_pred = 0, 1
    assert lib.jdet_gaussian_loss_level(1, 1, 1, 1, N, 1, 1, N, 0, 4, q, 1, 1.0, 1, 1, 1, 4096, N) == -1  # anchors
    q.decode_pred = 0
    assert lib.jdet_gaussian_loss_level(1, 1, 1, 1, N, 1, 1, N, 0, 4, q, 1, 1.0, 1, 1, 1, 16, N) == -3   # workspace
    assert lib.jdet_obb2hbb2obb(N, 4, 4, N, N) == -1 and lib.jdet_obb2hbb2obb(N, 0, 5, N, N) == 0
    assert lib.jdet_obb2hbb2obb(N, 0, 0, N, N) == 0            # an empty (0, 0) set, as the calculator accepts
    assert lib.jdet_anchor_targets_rotated_boxes(N, N, N, 0, 0, 1.0, N, N, N, N, N, N) == 0
    assert lib.jdet_anchor_targets_rotated_boxes(N, N, N, 5, 1, 1.0, N, N, N, N, N, N) == -1
