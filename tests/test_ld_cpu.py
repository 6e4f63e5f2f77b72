"""CPU: localization distillation -- the composed routes of box_ops.integral / the distribution loss / the KL loss against
the float64 restatements of tests/ld_ref.py, the registry names, the four named configs against their golden YAMLs, the
names in SIGNATURES, argument validation before any launch, and the
distillation detector's bookkeeping (no teacher in parameters() or state_dict(), teacher in eval, no URL checkpoints).

The product has no CPU assigner (anchor targets need the device), so the detector test hands the head its targets."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import ld_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ composed routes
@pytest.mark.parametrize("n", [1, 8, 31])
def test_integral_matches_the_restatement_and_its_closed_forms(n):
    from jdet_amd.models.boxes import box_ops
    rng = np.random.default_rng(n)
    x = torch.from_numpy(rng.standard_normal((13, 5 * (n + 1))) * 3.0)
    got = torch.cat([box_ops.integral(x[:, :4 * (n + 1)], n), box_ops.integral_angle(x[:, 4 * (n + 1):], n)[:, None]], 1)
    assert got.shape == (13, 5) and torch.equal(got, box_ops.integral_rows(x, n))
    # float64 e_k here (the composed route evaluates them in x's dtype), fp32 e_k in the restatement: R = 31 differs
    assert float((got - R.integral(x.numpy(), n)).abs().max()) <= (0.0 if n in (1, 8) else 4e-7) + 1e-14
    assert np.array_equal(R.bins(8, R.ENDS), np.linspace(-2, 2, 9)) and np.array_equal(R.bins(8, R.ANGLE_ENDS),
                                                                                        np.linspace(-5, 2, 9))


def test_integral_is_exact_on_saturated_and_constant_rows():
    from jdet_amd.models.boxes import box_ops
    k = 9
    for dtype in (torch.float32, torch.float64):
        lo_rows = torch.full((2, 5 * k), -200.0, dtype=dtype)
        hi_rows = lo_rows.clone()
        lo_rows[:, 0::k] = 200.0                              # all mass on the first bin of every side
        hi_rows[:, k - 1::k] = 200.0                          # ... on the last
        const = torch.full((2, 5 * k), 3.25, dtype=dtype)
        assert torch.equal(box_ops.integral_rows(lo_rows, 8), torch.tensor([[-2.0] * 4 + [-5.0]] * 2, dtype=dtype))
        assert torch.equal(box_ops.integral_rows(hi_rows, 8), torch.tensor([[2.0] * 4 + [2.0]] * 2, dtype=dtype))
        assert torch.equal(box_ops.integral_rows(const, 8), torch.tensor([[0.0] * 4 + [-1.5]] * 2, dtype=dtype))
        assert torch.equal(box_ops.integral(lo_rows[:, :4 * k], 8), torch.full((2, 4), -2.0, dtype=dtype))
        assert torch.equal(box_ops.integral_angle(hi_rows[:, 4 * k:], 8), torch.full((2,), 2.0, dtype=dtype))


@pytest.mark.parametrize("beta", [0.0, 1.0 / 9.0])
@pytest.mark.parametrize("wmode", ["ones", "mixed"])
def test_composed_distribution_loss_matches_the_restatement(beta, wmode):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.models.losses.dist_bbox_loss import dist_bbox_loss
    from jdet_amd.utils import registry as Reg
    f = R.bbox_fixture(63, 8, beta, wmode)
    fn = Reg.build_from_cfg(dict(type="SmoothL1Loss", beta=float(np.float32(beta)), loss_weight=R.LOSS_WEIGHT) if beta else
                            dict(type="L1Loss", loss_weight=R.LOSS_WEIGHT), Reg.LOSSES)
    x = torch.from_numpy(f["logits"]).double().requires_grad_(True)
    # the level's windows as the head passes them: (B, n, 5)
    t, w = (torch.from_numpy(f[k]).double().reshape(3, 21, 5) for k in ("target", "weight"))
    loss = dist_bbox_loss(fn, x, t, w, R.AVG, 8)
    loss.backward()
    assert abs(float(loss) - f["ref"][0]) <= 1e-12 * max(1.0, abs(f["ref"][0]))
    assert R.grad_error(x.grad.numpy(), f["ref"][1]) <= 1e-12


@pytest.mark.parametrize("wmode", ["null", "zero", "mixed", "last"])
@pytest.mark.parametrize("K,T", [(9, 10), (15, 2), (2, 1)])
def test_composed_kl_loss_matches_the_restatement(K, T, wmode):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils import registry as Reg
    f = R.kl_fixture(64, K, T, wmode)
    fn = Reg.build_from_cfg(dict(type="KnowledgeDistillationKLDivLoss", loss_weight=R.LOSS_WEIGHT, T=T), Reg.LOSSES)
    x = torch.from_numpy(f["pred"]).double().requires_grad_(True)
    s = torch.from_numpy(f["soft"]).double()
    w = None if f["weight"] is None else torch.from_numpy(f["weight"]).reshape(4, 16)     # a (B, n) window
    loss = fn(x, s, w, avg_factor=123.0)                     # avg_factor is ignored, as in the reference
    loss.backward()
    ref_loss, ref_grad, count = f["ref"]
    assert count == (64 if wmode in ("null", "zero") else int((f["weight"] > 0).sum()))
    assert abs(float(loss) - ref_loss) <= 1e-12 * max(1.0, abs(ref_loss))
    assert R.grad_error(x.grad.numpy(), ref_grad) <= 1e-12
    if wmode == "zero":                                      # the fall-through: every row, exactly as without a weight
        n = R.kl_fixture(64, K, T, "null")
        assert np.array_equal(n["pred"], f["pred"]) and n["ref"][0] == ref_loss and np.array_equal(n["ref"][1], ref_grad)
    if wmode in ("mixed", "last"):
        assert (x.grad.numpy()[f["weight"] <= 0] == 0).all()


def test_kl_weight_views_and_im_loss():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.models.losses.kd_loss import IMLoss, _row_weight
    bw = torch.zeros((2, 40, 5))[:, 7:19]                   # a level's bbox_weights window
    v = _row_weight(bw, 2 * 12 * 5)
    assert v.shape == (2, 60) and v.stride() == (200, 1) and v.data_ptr() == bw.data_ptr()
    a, b = torch.randn(6, 256), torch.randn(6, 256)
    assert torch.allclose(IMLoss(loss_weight=2.0)(a, b), 2.0 * ((a - b) ** 2).mean())
    nan = torch.full((6, 256), float("nan"))
    z = IMLoss(loss_weight=0)(nan, nan)                      # weight 0: the maps are not touched
    assert z.dim() == 0 and float(z) == 0.0


# ---------------------------------------------------------------------------------------------------- registry, configs
def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return [_plain(x) for x in v] if isinstance(v, (list, tuple)) else v


GOLDEN = {"RETINANET_R18_CFG": "rotated_retinanet_obb_r18_fpn_1x_dota",
          "DIST_RETINANET_R18_CFG": "rotated_retinanet_obb_distribution_r18_fpn_1x_dota",
          "DIST_RETINANET_R50_CFG": "rotated_retinanet_obb_distribution_r50_fpn_1x_dota",
          "LD_RETINANET_CFG": "ld_rotated_retinanet_obb_r18_r50_fpn_1x_dota"}


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_named_config_equals_the_reference_file(name):
    from jdet_amd.config import Config, named
    cfg = getattr(named, name)
    c = Config(os.path.join(ROOT, "tests", "golden", "configs", GOLDEN[name] + ".yaml")).dump()
    ours, theirs = _plain(cfg["model"]), _plain(c["model"])
    if name == "LD_RETINANET_CFG":
        # the file names the teacher's config file and an https link; the named config holds the teacher's config and no
        # checkpoint (nothing in this project fetches one)
        assert theirs.pop("teacher_config") == "configs/ld/" + GOLDEN["DIST_RETINANET_R50_CFG"] + ".py"
        assert theirs.pop("teacher_ckpt").startswith("https://")
        assert ours.pop("teacher_ckpt") is None
        assert ours.pop("teacher_config") == _plain(named.DIST_RETINANET_R50_CFG)
    assert ours == theirs
    for k in ("optimizer", "scheduler"):
        assert _plain(c[k]) == _plain(cfg[k]), k


def test_registry_builds_the_losses_the_heads_and_the_detector():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.config.named import DIST_RETINANET_R18_CFG, LD_RETINANET_CFG
    from jdet_amd.utils import registry as Reg
    kd = Reg.build_from_cfg(dict(type="KnowledgeDistillationKLDivLoss", loss_weight=10, T=2), Reg.LOSSES)
    assert kd.T == 2 and kd.loss_weight == 10 and kd.reduction == "mean"
    with pytest.raises(AssertionError):
        Reg.build_from_cfg(dict(type="KnowledgeDistillationKLDivLoss", T=0.5), Reg.LOSSES)
    assert Reg.build_from_cfg(dict(type="IMLoss", loss_weight=0), Reg.LOSSES).loss_weight == 0
    h = Reg.build_from_cfg(DIST_RETINANET_R18_CFG["model"]["bbox_head"], Reg.HEADS)
    assert type(h).__name__ == "RotatedRetinaDistributionHead" and isinstance(h, Reg.HEADS.get("RotatedRetinaHead"))
    assert h.reg_max == 8 and h.retina_reg.out_channels == 9 * 5 * 9 and h.retina_cls.out_channels == 9 * 15
    s = Reg.build_from_cfg(LD_RETINANET_CFG["model"]["bbox_head"], Reg.HEADS)
    assert type(s).__name__ == "RotatedRetinaLocalizationDistillationHead" and isinstance(s, type(h))
    assert s.loss_ld.T == 10 and s.loss_kd.T == 2 and s.loss_im.loss_weight == 0 and s.imitation_method == "finegrained"
    assert callable(s.execute_train) and s.retina_reg.out_channels == 405
    assert Reg.MODELS.get("KnowledgeDistillationSingleStageDetector") is not None


# ---------------------------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def built_lib():
    from jdet_amd import _lib
    _lib.build()
    return _lib


def test_header_signatures_and_exports_agree(built_lib):
    assert {"jdet_dist_integral", "jdet_dist_bbox_loss_level", "jdet_kd_kl_div_level_forward",
            "jdet_kd_kl_div_level_backward"} <= set(built_lib.SIGNATURES)


def test_argument_checks_return_before_any_launch(built_lib):
    lib = built_lib.lib()
    N, X = None, 4096                                        # X: a non-null address nobody reads
    nan, inf = float("nan"), float("inf")
    need = lib.jdet_sigmoid_focal_loss_workspace()

    def integ(x=X, rows=4, R=8, lo=-2.0, hi=2.0, la=-5.0, ha=2.0, out=X):
        return lib.jdet_dist_integral(x, rows, R, lo, hi, la, ha, out, N)
    assert integ(x=N) == -1 and integ(out=N) == -1 and integ(rows=-1) == -1 and integ(R=0) == -1 and integ(R=-3) == -1
    assert integ(lo=nan) == -1 and integ(hi=inf) == -1 and integ(la=nan) == -1 and integ(ha=-inf) == -1
    assert integ(R=32) == -2 and integ(R=1000) == -2
    assert integ(rows=0) == 0 and integ(rows=0, x=N, out=N) == 0

    def bbox(x=X, t=X, tr=4, ts=4, w=X, wr=4, wst=4, rows=4, R=8, lo=-2.0, hi=2.0, la=-5.0, ha=2.0, beta=0.1, avg=X,
             lw=1.0, loss=X, g=X, ws=X, wsb=need):
        return lib.jdet_dist_bbox_loss_level(x, t, tr, ts, w, wr, wst, rows, R, lo, hi, la, ha, beta, avg, lw, loss, g,
                                             ws, wsb, N)
    for null in ("x", "t", "avg", "loss", "g", "ws"):
        assert bbox(**{null: N}) == -1, null
    assert bbox(rows=-1) == -1 and bbox(R=0) == -1 and bbox(beta=-0.1) == -1 and bbox(beta=nan) == -1
    assert bbox(tr=0) == -1 and bbox(ts=-1) == -1 and bbox(wr=0) == -1 and bbox(wst=-1) == -1 and bbox(hi=nan) == -1
    assert bbox(R=32) == -2 and bbox(wsb=need - 1) == -3 and bbox(wsb=0) == -3

    def kf(p=X, s=X, w=X, wr=8, wst=8, M=8, K=9, T=2.0, lw=1.0, loss=X, cnt=X, ws=X, wsb=need):
        return lib.jdet_kd_kl_div_level_forward(p, s, w, wr, wst, M, K, T, lw, loss, cnt, ws, wsb, N)

    def kb(p=X, s=X, w=X, wr=8, wst=8, M=8, K=9, T=2.0, lw=1.0, cnt=X, go=X, g=X):
        return lib.jdet_kd_kl_div_level_backward(p, s, w, wr, wst, M, K, T, lw, cnt, go, g, N)
    for f in (kf, kb):
        assert f(p=N) == -1 and f(s=N) == -1 and f(cnt=N) == -1
        assert f(M=-1) == -1 and f(K=0) == -1 and f(K=-2) == -1 and f(wr=0) == -1 and f(wst=-1) == -1
        assert f(T=0.5) == -1 and f(T=0.0) == -1 and f(T=-1.0) == -1 and f(T=nan) == -1 and f(T=inf) == -1
        assert f(K=33) == -2 and f(M=2 ** 31) == -2
    assert kf(loss=N) == -1 and kf(ws=N) == -1 and kf(wsb=need - 1) == -3
    assert kb(go=N) == -1 and kb(g=N) == -1 and kb(M=0, p=N, s=N, g=N) == 0


# ------------------------------------------------------------------------------------------------------------ detector
def _tiny_ld_cfg():
    from jdet_amd.config.named import LD_RETINANET_CFG
    cfg = copy.deepcopy(LD_RETINANET_CFG)
    cfg["model"]["bbox_head"]["stacked_convs"] = 1
    cfg["model"]["teacher_config"]["model"]["bbox_head"]["stacked_convs"] = 1
    return cfg


def _given_targets(anchor_list, valid_flag_list, gt_bboxes, img_metas, means, stds, cfg, **kw):
    """what anchor_target returns, without the device: three positives per image on the two finest levels, none on the
    others (their KL terms take the fall-through)"""
    n = [a.shape[0] for a in anchor_list[0]]
    B, N = len(anchor_list), sum(n)
    g = torch.Generator().manual_seed(5)
    labels, lw = torch.zeros((B, N), dtype=torch.int64), torch.ones((B, N))
    bt, bw = torch.zeros((B, N, 5)), torch.zeros((B, N, 5))
    pos = torch.tensor([3, 40, n[0] + 5])
    labels[:, pos] = torch.randint(1, 16, (B, 3), generator=g)
    bt[:, pos] = torch.randn((B, 3, 5), generator=g) * 0.3
    bw[:, pos] = 1.0
    starts = np.cumsum([0] + n)
    return tuple([t[:, s:e] for s, e in zip(starts[:-1], starts[1:])] for t in (labels, lw, bt, bw)) + (B * 3, 0)


def test_kd_detector_keeps_the_teacher_out_and_returns_five_finite_losses(monkeypatch):
    import socket
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils import registry as Reg
    from jdet_amd.utils.general import parse_losses

    def no_network(*a, **k):
        raise AssertionError("a network call")
    monkeypatch.setattr(socket, "socket", no_network)
    monkeypatch.setattr(socket, "create_connection", no_network)
    monkeypatch.setattr(socket, "getaddrinfo", no_network)
    cfg = _tiny_ld_cfg()
    for url in ("https://example.invalid/teacher.pkl", "http://example.invalid/t.pkl", "jittorhub://teacher.pkl"):
        with pytest.raises(ValueError, match="URL"):
            Reg.build_from_cfg(dict(cfg["model"], teacher_ckpt=url), Reg.MODELS)
    torch.manual_seed(0)
    m = Reg.build_from_cfg(cfg["model"], Reg.MODELS)
    teacher = m.teacher_model
    assert type(teacher.bbox_head).__name__ == "RotatedRetinaDistributionHead" and teacher.backbone is not m.backbone
    t_ids = {id(p) for p in teacher.parameters()}
    assert t_ids and not t_ids & {id(p) for p in m.parameters()} and not any("teacher" in k for k in m.state_dict())
    assert not any("teacher" in n for n, _ in m.named_modules()) and set(map(id, m.frozen_parameters())) == t_ids
    assert not any(p.requires_grad for p in teacher.parameters())
    m.train()
    assert m.training and m.backbone.training and not teacher.training and not teacher.bbox_head.training
    m.double()                                               # dtype / device moves reach the teacher
    assert all(p.dtype == torch.float64 for p in teacher.parameters())
    m.float()
    m.bbox_head.anchor_target = _given_targets
    before = [p.detach().clone() for p in teacher.parameters()]
    images = torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(1))
    targets = [dict(rboxes=torch.zeros((1, 5)), labels=torch.ones((1,), dtype=torch.int32), rboxes_ignore=torch.zeros((0, 5)),
                    img_size=(64, 64), scale_factor=1.0, pad_shape=(64, 64)) for _ in range(2)]
    out = m(images, targets)
    assert set(out) == {"loss_cls", "loss_bbox", "loss_LD", "loss_KD", "loss_FeatureImitation"}
    assert all(len(v) == 5 and all(torch.isfinite(x) for x in v) for v in out.values())
    assert all(float(x) > 0 for x in out["loss_LD"] + out["loss_KD"]) and all(float(x) == 0 for x in
                                                                              out["loss_FeatureImitation"])
    total, _ = parse_losses(out)
    total.backward()
    assert all(p.grad is None for p in teacher.parameters())
    assert m.bbox_head.retina_reg.weight.grad.abs().max() > 0
    assert all(torch.equal(a, b) for a, b in zip(before, teacher.parameters()))
    no_eval = Reg.build_from_cfg(dict(cfg["model"], eval_teacher=False), Reg.MODELS)
    no_eval.train()
    assert no_eval.teacher_model.training
    no_eval.eval()
    assert not no_eval.teacher_model.training


def test_teacher_checkpoint_loads_from_a_local_file(tmp_path):
    import pickle
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils import registry as Reg
    cfg = _tiny_ld_cfg()
    torch.manual_seed(1)
    donor = Reg.build_from_cfg(cfg["model"]["teacher_config"]["model"], Reg.MODELS)
    state = {k: v.numpy() for k, v in donor.state_dict().items()}
    for layout in ("model", "state_dict", None):
        path = tmp_path / ("teacher_%s.pkl" % layout)
        with open(path, "wb") as f:
            pickle.dump({layout: state, "meta": {}} if layout else state, f)
        torch.manual_seed(2)
        m = Reg.build_from_cfg(dict(cfg["model"], teacher_ckpt=str(path)), Reg.MODELS)
        assert m.teacher_missing == []
        assert torch.equal(m.teacher_model.bbox_head.retina_reg.weight, donor.bbox_head.retina_reg.weight)
