"""GPU: localization distillation -- the kernels of csrc/dist_loss.hip (jdet_dist_integral, jdet_dist_bbox_loss_level,
jdet_kd_kl_div_level_forward / _backward) against the float64 restatements of tests/ld_ref.py in every regime, their
buffer contracts (tests/guarded.py: guard bands, poisoned outputs and workspace, inputs unchanged, run B == run A bit
for bit, a short workspace refused), the autograd nodes against their composed routes on the device, and
DIST_RETINANET_R18_CFG / LD_RETINANET_CFG end to end.

Bounds.  Every bound is 4 x the error of the float32 restatement against the float64 one, computed here from the
restatements, never from the code under test, printed and asserted > 0:
  loss       |loss32 - loss64|, absolute;
  gradient   max |g32 - g64| / max |g64|;
  integral   max |E32 - E64|.
tests/ld_ref.py states the conditions its fixtures meet by construction.  The detector tests, whose batch no fixture
restates, use the largest RELATIVE loss error and the largest gradient error over DETECTOR_FIXTURES, times 2 where two
float32 routes are compared with each other, the loss bound scaled by max(1, |loss|) -- float32 error grows with the
magnitude of the sum.

Regimes: tiles of 48 anchors = 240 softmax rows (rows 1, 63, 257: one ragged tile, two, six), the three register sizes
(reg_max + 1 / K of at most 8, 16, 32), a blocked window with an odd offset over two blocks, the grid cap of 384
workgroups (60 000 anchors = 1250 tiles; 270 001 KL rows = 1126 tiles), the unaligned (scalar-copy) route."""
import math

import numpy as np
import pytest
import torch

from tests import ld_ref as R
from tests.abi_cases import (dist_bbox_case as _bbox_case, kl_backward_case as _kl_backward_case,
                             kl_forward_case as _kl_forward_case)

pytestmark = pytest.mark.gpu

NINTH = 1.0 / 9.0
DETECTOR_FIXTURES = [("bbox", 257, 8, 0.0, "mixed"), ("bbox", 257, 8, NINTH, "mixed"), ("bbox", 63, 8, 0.0, "ones"),
                     ("kl", 1285, 9, 10, "mixed"), ("kl", 1285, 15, 2, "mixed"), ("kl", 1285, 9, 10, "null"),
                     ("kl", 1285, 15, 2, "null")]


def detector_bounds():
    """(relative loss bound, gradient bound): 4 x the largest float32 error over DETECTOR_FIXTURES"""
    fx = [R.bbox_fixture(*f[1:]) if f[0] == "bbox" else R.kl_fixture(*f[1:]) for f in DETECTOR_FIXTURES]
    return 4 * max(f["e_loss"] / abs(f["ref"][0]) for f in fx), 4 * max(f["e_grad"] for f in fx)


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bbox_fn(beta):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils import registry as Reg
    return Reg.build_from_cfg(dict(type="SmoothL1Loss", beta=float(np.float32(beta)), loss_weight=R.LOSS_WEIGHT) if beta else
                              dict(type="L1Loss", loss_weight=R.LOSS_WEIGHT), Reg.LOSSES)


# ------------------------------------------------------------------------------------------------------------ integral
@pytest.mark.parametrize("reg_max", [1, 8, 31])
def test_integral_against_float64(dev, reg_max):
    from jdet_amd.models.boxes.box_ops import integral_rows
    for rows in (1, 63, 257, 60000):
        x = R.bbox_fixture(rows, reg_max, 0.0, "ones")["logits"] if rows < 60000 else \
            (np.random.default_rng(rows).standard_normal((rows, 5 * (reg_max + 1))) * 2).astype(np.float32)
        ref = R.integral(x, reg_max).numpy()
        e32 = float(np.abs(R.integral(x, reg_max, torch.float32).double().numpy() - ref).max())
        xd = _dev(x, dev)
        got = integral_rows(xd, reg_max)
        assert got.shape == (rows, 5) and got.dtype == torch.float32
        err = float(np.abs(got.double().cpu().numpy() - ref).max())
        print("integral rows %d reg_max %d: float32 restatement %.3e, kernel %.3e (bound %.3e)" % (rows, reg_max, e32, err, 4 * e32))
        assert e32 > 0 and err <= 4 * e32
        assert torch.equal(got, integral_rows(xd, reg_max)) and torch.equal(xd.cpu(), torch.from_numpy(x))
        # the composed route on the device, at the sum of both bounds
        with torch.enable_grad():
            comp = integral_rows(xd.clone().requires_grad_(True), reg_max)
        assert float((comp.detach() - got).abs().max()) <= 8 * e32
    if reg_max == 31:                                        # the closed forms need exact bins: reg_max = 1, 8
        return
    k = reg_max + 1
    sat = torch.full((3, 5 * k), -200.0, device=dev)
    sat[:, 0::k] = 200.0
    assert torch.equal(integral_rows(sat, reg_max).cpu(), torch.tensor([[-2.0] * 4 + [-5.0]] * 3))
    assert torch.equal(integral_rows(torch.full((3, 5 * k), 1.5, device=dev), reg_max).cpu(),
                       torch.tensor([[0.0] * 4 + [-1.5]] * 3))


# ------------------------------------------------------------------------------------------------- distribution loss
@pytest.mark.parametrize("reg_max", [1, 8, 31])
@pytest.mark.parametrize("rows", [1, 63, 257, 2 * 1531])
def test_bbox_loss_contract_and_float64(dev, rows, reg_max):
    from tests import guarded
    for beta in (0.0, NINTH):
        for wmode in ("ones", "zeros", "last"):
            c = _bbox_case(rows, reg_max, beta, wmode, windowed=rows == 2 * 1531)
            guarded.run_case(c.entry_points[0], c.label, c.fn, dev)


@pytest.mark.parametrize("case", ["capped grid", "capped grid mixed", "unaligned", "unaligned K32"])
def test_bbox_loss_contract_large_and_unaligned(dev, case):
    from tests import guarded
    c = {"capped grid": lambda: _bbox_case(60000, 8, 0.0, "ones"),
         "capped grid mixed": lambda: _bbox_case(60000, 8, NINTH, "mixed"),
         "unaligned": lambda: _bbox_case(257, 8, NINTH, "mixed", unaligned=True),
         "unaligned K32": lambda: _bbox_case(63, 31, 0.0, "ones", unaligned=True)}[case]()
    assert 60000 * 5 > 1024 * 256
    guarded.run_case(c.entry_points[0], c.label, c.fn, dev)


@pytest.mark.parametrize("beta", [0.0, NINTH])
def test_bbox_node_against_float64_and_the_composed_route(dev, beta, monkeypatch):
    """the autograd node (unit gradient scaled by jdet_loss_grad_scale) against float64; the composed route on the device
    against the node at the sum of both bounds; two runs bit-identical"""
    from jdet_amd.models.losses import _level
    from jdet_amd.models.losses import dist_bbox_loss as D
    fn = _bbox_fn(beta)
    for rows, wmode in ((257, "mixed"), (2 * 1531, "mixed"), (63, "ones")):
        f = R.bbox_fixture(rows, 8, beta, wmode)
        B = 2 if rows % 2 == 0 else 1
        n = rows // B
        t = _dev(R.window(f["target"].reshape(B, n, 5), n + 69, 7), dev)[:, 7:7 + n]
        w = _dev(R.window(f["weight"].reshape(B, n, 5), n + 69, 7), dev)[:, 7:7 + n]
        avg = torch.tensor(R.AVG, device=dev)

        def run(fused):
            monkeypatch.setattr(_level, "LEVEL_NODES", fused)
            x = _dev(f["logits"], dev).requires_grad_(True)
            assert D._level_ok(fn, x, t, w, avg, 8) == fused
            loss = D.dist_bbox_loss(fn, x, t, w, avg, 8)
            (loss * 3.0).backward()
            return float(loss.detach()), x.grad.double().cpu().numpy() / 3.0, x.grad
        l1, g1, raw1 = run(True)
        l2, g2, _ = run(False)
        l3, _, raw3 = run(True)
        e1, e2 = R.grad_error(g1, f["ref"][1]), R.grad_error(g2, f["ref"][1])
        print("node rows %d beta %.3f: loss error fused %.3e composed %.3e (bound %.3e), grad fused %.3e composed %.3e "
              "(bound %.3e)" % (rows, beta, abs(l1 - f["ref"][0]), abs(l2 - f["ref"][0]), 4 * f["e_loss"], e1, e2, 4 * f["e_grad"]))
        assert f["e_loss"] > 0 and f["e_grad"] > 0
        assert abs(l1 - f["ref"][0]) <= 4 * f["e_loss"] and e1 <= 4 * f["e_grad"]
        assert abs(l1 - l2) <= 8 * f["e_loss"] and R.grad_error(g1, g2) <= 8 * f["e_grad"]
        assert l1 == l3 and torch.equal(raw1, raw3)


# -------------------------------------------------------------------------------------------------------- KL divergence
@pytest.mark.parametrize("T", [1, 2, 10])
@pytest.mark.parametrize("K", [2, 9, 15, 32])
def test_kl_contract_and_float64(dev, K, T):
    from tests import guarded
    for M in (1, 64, 5 * 257):
        for wmode in ("null", "zero", "mixed", "last"):
            for make in (_kl_forward_case, _kl_backward_case):
                c = make(M, K, T, wmode, windowed=wmode == "mixed")
                guarded.run_case(c.entry_points[0], c.label, c.fn, dev)


@pytest.mark.parametrize("case", ["capped grid", "unaligned", "unaligned K32"])
def test_kl_contract_large_and_unaligned(dev, case):
    from tests import guarded
    M, K, T, kw = {"capped grid": (270001, 9, 10, dict(windowed=False)), "unaligned": (5 * 257, 9, 2, dict(unaligned=True)),
                   "unaligned K32": (64, 32, 1, dict(unaligned=True))}[case]
    assert 270001 > 262144
    for make in (_kl_forward_case, _kl_backward_case):
        c = make(M, K, T, "mixed", **kw)
        guarded.run_case(c.entry_points[0], c.label, c.fn, dev)


def _kl_node(dev, f, T, weight="fixture", soft=None):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.models.losses.kd_loss import KnowledgeDistillationKLDivLoss
    fn = KnowledgeDistillationKLDivLoss(loss_weight=R.LOSS_WEIGHT, T=T)
    x = _dev(f["pred"], dev).requires_grad_(True)
    s = _dev(f["soft"] if soft is None else soft, dev)
    w = _dev(f["weight"], dev) if isinstance(weight, str) else weight
    loss = fn(x, s, w)
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("K,T", [(9, 10), (15, 2), (32, 1), (2, 10)])
def test_kl_node_zero_weight_equals_null_and_soft_equals_pred(dev, K, T, monkeypatch):
    from jdet_amd.models.losses import _level
    M = 5 * 257
    null, zero, mixed = (R.kl_fixture(M, K, T, m) for m in ("null", "zero", "mixed"))
    assert np.array_equal(null["pred"], zero["pred"]) and np.array_equal(null["soft"], zero["soft"])
    ln, gn = _kl_node(dev, null, T)
    lz, gz = _kl_node(dev, zero, T)
    assert torch.equal(ln, lz) and torch.equal(gn, gz)                      # the fall-through, bit for bit
    lm, gm = _kl_node(dev, mixed, T)
    lm2, gm2 = _kl_node(dev, mixed, T)
    assert torch.equal(lm, lm2) and torch.equal(gm, gm2)                    # two runs
    assert (gm.cpu().numpy()[mixed["weight"] <= 0] == 0).all() and (gm.cpu().numpy()[mixed["weight"] > 0] != 0).any()
    # the composed route on the device against the node, at the sum of both bounds
    monkeypatch.setattr(_level, "LEVEL_NODES", False)
    lc, gc = _kl_node(dev, mixed, T)
    monkeypatch.setattr(_level, "LEVEL_NODES", True)
    print("kl node K %d T %d: fused %.7f composed %.7f (bound %.3e), grad %.3e (bound %.3e)" % (
        K, T, float(lm), float(lc), 8 * mixed["e_loss"], R.grad_error(gm.cpu().numpy(), gc.double().cpu().numpy()), 8 * mixed["e_grad"]))
    assert abs(float(lm) - float(lc)) <= 8 * mixed["e_loss"]
    assert R.grad_error(gm.cpu().numpy(), gc.double().cpu().numpy()) <= 8 * mixed["e_grad"]
    # soft == pred: loss and gradient within the fixture's bounds of 0
    l0, g0 = _kl_node(dev, mixed, T, soft=mixed["pred"])
    assert mixed["e_loss"] > 0 and mixed["e_grad"] > 0
    assert abs(float(l0)) <= 4 * mixed["e_loss"]
    assert float(g0.abs().max()) <= 4 * mixed["e_grad"] * np.abs(mixed["ref"][1]).max()


def test_kl_large_spread_stays_finite(dev):
    for K, T in ((9, 10), (15, 2), (32, 1)):
        f = R.kl_fixture(64, K, T, "mixed", spread=300.0)
        assert np.ptp(f["pred"][-1]) / T == 300.0
        loss, grad = _kl_node(dev, f, T)
        assert torch.isfinite(loss) and torch.isfinite(grad).all() and float(loss) > 0


def test_kl_node_runs_without_a_host_sync(dev):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.models.losses.kd_loss import KnowledgeDistillationKLDivLoss
    f = R.kl_fixture(5 * 257, 9, 10, "mixed")
    fn = KnowledgeDistillationKLDivLoss(loss_weight=10, T=10)
    x, s = _dev(f["pred"], dev).requires_grad_(True), _dev(f["soft"], dev)
    bw = _dev(R.window(f["weight"].reshape(1, 257, 5), 300, 11), dev)[:, 11:268]      # a (B, n, 5) bbox_weights window
    zero = torch.zeros_like(bw)
    fn(x, s, bw).backward()                                                          # warm up: code objects, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = fn(x, s, bw)
        b = fn(x, s, zero)                                                           # count == 0: the fall-through
        (a + b).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(a) and torch.isfinite(b) and torch.isfinite(x.grad).all()
    ref = R.kl_loss(f["pred"], f["soft"], f["weight"], 10, 10, torch.float64)[0]
    assert abs(float(a) - ref) <= 1e-6 * abs(ref)


# ------------------------------------------------------------------------------------------------------------ detectors
def _losses_and_reg_grad(m, images, targets):
    from jdet_amd.utils.general import parse_losses
    m.zero_grad(set_to_none=True)
    out = m(images, targets)
    total, _ = parse_losses(out)
    total.backward()
    return ({k: [float(x) for x in v] for k, v in out.items()},
            m.bbox_head.retina_reg.weight.grad.detach().double().cpu().numpy().copy())


def _fused_against_composed(m, images, targets, keys, monkeypatch):
    from jdet_amd.models.losses import _level
    rel, gb = detector_bounds()
    assert rel > 0 and gb > 0
    fused, gf = _losses_and_reg_grad(m, images, targets)
    monkeypatch.setattr(_level, "LEVEL_NODES", False)
    comp, gc = _losses_and_reg_grad(m, images, targets)
    monkeypatch.setattr(_level, "LEVEL_NODES", True)
    for k in keys:
        for lvl, (a, b) in enumerate(zip(fused[k], comp[k])):
            bound = 2 * rel * max(1.0, abs(b))
            print("%s level %d: fused %.7f composed %.7f (bound %.2e)" % (k, lvl, a, b, bound))
            assert math.isfinite(a) and abs(a - b) <= bound, (k, lvl)
    ge = R.grad_error(gf, gc)
    print("retina_reg.weight.grad: fused against composed %.3e (bound %.3e)" % (ge, 2 * gb))
    assert np.isfinite(gf).all() and np.abs(gf).max() > 0 and ge <= 2 * gb
    return fused


def _keys(d):
    """every string key of a nested dict"""
    return [k for k in d if isinstance(k, str)] + [x for v in d.values() if isinstance(v, dict) for x in _keys(v)]


def _batch(dev):
    from jdet_amd.runner import synthetic_batch
    return synthetic_batch(2, 128, dev, seed=3, num_gts=4)


def test_distribution_detector_trains_fused_equals_composed_and_infers(dev, monkeypatch):
    """DIST_RETINANET_R18_CFG at 2 x 128^2 with 4 boxes per image (levels of 16^2 .. 1^2 positions; the coarsest holds
    no positive): finite losses, fused = composed in loss_bbox and retina_reg.weight.grad, the total falling over 10 SGD
    steps on the batch, inference returning polygons / scores / labels of one length"""
    import copy
    from jdet_amd.config.named import DIST_RETINANET_R18_CFG
    from jdet_amd.runner import Runner
    cfg = copy.deepcopy(DIST_RETINANET_R18_CFG)
    cfg["scheduler"] = None                                  # no warm-up: ten steps at the config's learning rate
    images, targets = _batch(dev)
    torch.manual_seed(0)
    r = Runner(cfg, device=dev, conv_autotune=False, graph=False)
    m = r.model
    m.train()
    fused = _fused_against_composed(m, images, targets, ("loss_bbox",), monkeypatch)
    assert set(fused) == {"loss_cls", "loss_bbox"} and all(math.isfinite(x) for v in fused.values() for x in v)
    assert sum(fused["loss_bbox"]) > 0 and fused["loss_bbox"][-1] == 0.0
    hist = [float(r.train_step(images, targets)[0]) for _ in range(10)]
    print("DIST_RETINANET_R18_CFG total loss", np.round(hist, 4).tolist())
    assert np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    m.eval()
    with torch.no_grad():
        m.bbox_head.retina_cls.bias.fill_(-2.0)
        res = m(images, targets)
    assert len(res) == 2
    for polys, scores, labels in res:
        assert polys.dim() == 2 and polys.shape[1] == 8 and polys.shape[0] == scores.shape[0] == labels.shape[0]
        assert 0 < polys.shape[0] <= cfg["model"]["bbox_head"]["test_cfg"]["max_per_img"]
        assert torch.isfinite(polys).all()


def test_ld_detector_distils_from_a_frozen_teacher(dev, monkeypatch, tmp_path):
    """LD_RETINANET_CFG (R50 teacher, randomly initialised, R18 student) at 2 x 128^2: five loss keys; fused = composed
    in loss_bbox / loss_LD / loss_KD and retina_reg.weight.grad; the teacher has no gradient and does not move in a
    step; a checkpoint holds no teacher tensor and round-trips the student"""
    import copy
    import pickle
    from jdet_amd.config.named import LD_RETINANET_CFG
    from jdet_amd.runner import Runner
    images, targets = _batch(dev)
    torch.manual_seed(0)
    r = Runner(copy.deepcopy(LD_RETINANET_CFG), device=dev, conv_autotune=False, graph=False)
    m = r.model
    teacher = m.teacher_model
    assert all(p.is_cuda for p in teacher.parameters())
    assert any(p.dim() == 4 and p.shape[-1] > 1 and p.is_contiguous(memory_format=torch.channels_last) and
               not p.is_contiguous() for p in teacher.parameters())          # the channels-last conversion reached it
    m.train()
    assert not teacher.training
    fused = _fused_against_composed(m, images, targets, ("loss_bbox", "loss_LD", "loss_KD"), monkeypatch)
    assert set(fused) == {"loss_cls", "loss_bbox", "loss_LD", "loss_KD", "loss_FeatureImitation"}
    assert all(len(v) == 5 and all(math.isfinite(x) for x in v) for v in fused.values())
    assert all(x > 0 for x in fused["loss_LD"] + fused["loss_KD"]) and fused["loss_bbox"][-1] == 0.0
    before = [p.detach().clone() for p in teacher.parameters()]
    student0 = m.bbox_head.retina_reg.weight.detach().clone()
    total = float(r.train_step(images, targets)[0])
    assert math.isfinite(total)
    assert all(p.grad is None for p in teacher.parameters())
    assert all(torch.equal(a, b) for a, b in zip(before, teacher.parameters()))
    assert not torch.equal(student0, m.bbox_head.retina_reg.weight.detach())
    path = r.save(str(tmp_path / "ld.pkl"))
    with open(path, "rb") as f:
        data = pickle.load(f)
    own = {k for k in m.state_dict() if not k.endswith("num_batches_tracked")}
    assert set(data["model"]) == own and not any("teacher" in k for k in data["model"])
    assert not any("teacher" in k for k in _keys(data))
    saved = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        for p in m.parameters():
            p.add_(1.0)
    missing, unexpected, mismatched = r.load(path)
    assert missing == [] and unexpected == [] and mismatched == []
    assert all(torch.equal(saved[k], v) for k, v in m.state_dict().items())
    assert all(torch.equal(a, b) for a, b in zip(before, teacher.parameters()))
