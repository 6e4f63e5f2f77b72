"""CPU: Circular Smooth Label -- the float64 restatements of tests/csl_ref.py against an independent restatement of the
reference's encoder (omega 1, where it is defined), against the circular-distance closed form and against central
differences; the composed routes (CSLCoder, SmoothFocalLoss, csl_angle_loss) against the restatements; the side header
against CSL_SIGNATURES and the exports; argument validation before any launch; the dry run of the smallest case of every
entry point; the named config against its golden YAML and the model it builds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import csl_cases as C
from tests import csl_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_TARGETS = np.concatenate([np.linspace(-0.785, 2.3555, 197).astype(np.float32), C.EXACT_TARGETS])


# ------------------------------------------------------------------------------------------------------- restatements
def _reference_encode(a, omega, window, radius):
    """the reference's CSLCoder.encode, restated on its own: zeros, then ONE scatter of the window's values (float32, as
    its framework holds them) at (offsets + bin) % coding_len.  Defined where no index repeats: omega = 1."""
    L = int(180 // omega)
    a = np.asarray(a, np.float32).reshape(-1, 1)
    deg = ((a * np.float32(180 / np.pi)) + np.float32(45)) / np.float32(omega)
    t = deg.astype(np.int64)                                  # the cast truncates toward zero
    out = np.zeros((a.shape[0], L), np.float32)
    if window == "pulse":
        idx, val = t % L, np.float32(1.0)
    elif window in ("rect", "triangle"):
        base = np.arange(-radius, radius)
        idx = (base[None, :] + t) % L
        val = np.float32(1.0) if window == "rect" else (1.0 - np.abs((1 / radius) * base)).astype(np.float32)[None, :]
    else:
        base = np.arange(-180 // 2, 180 // 2)
        idx = (base[None, :] + t) % L
        val = np.exp(-np.power(base.astype(np.float64), 2) / (2 * radius ** 2)).astype(np.float32)[None, :]
    assert all(len(set(r)) == len(r) for r in idx.tolist())   # no duplicate index: the scatter is defined
    np.put_along_axis(out, idx, np.broadcast_to(val, idx.shape).astype(np.float32), axis=1)
    return out


@pytest.mark.parametrize("window,radius", C.WINDOW_CASES)
def test_restatement_equals_the_reference_encoder_at_omega_1(window, radius):
    ours = R.labels(R.bins(ALL_TARGETS, 1), 180, window, radius)
    assert np.array_equal(ours.astype(np.float32), _reference_encode(ALL_TARGETS, 1, window, radius))
    assert R.bins(np.float32([0.0]), 1)[0] == 45 and R.bins(np.float32([-0.7890625]), 1)[0] == 0      # 45 exactly; trunc
    assert R.bins(np.float32([-1.0]), 1)[0] == 180 - 12 and R.bins(np.float32([2.5]), 1)[0] == 188 - 180


@pytest.mark.parametrize("omega", [1, 2.8, 4, 6, 90])
@pytest.mark.parametrize("radius", [3, 6, 0.7])
def test_largest_duplicate_is_the_circular_distance_label(omega, radius):
    L = R.coding_len(omega)
    assert L == {1: 180, 2.8: 64, 4: 45, 6: 30, 90: 2}[omega]
    t = R.bins(ALL_TARGETS, omega)
    assert t.min() == 0 and t.max() == L - 1
    assert np.array_equal(R.labels(t, L, "gaussian", radius), R.circular_labels(t, L, radius))


def test_restated_gradient_is_the_derivative_of_the_restated_loss():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((6, 45)) * 3.0
    y = R.labels(rng.integers(0, 45, 6), 45, "gaussian", 3)
    h = 1e-6
    for gamma in (0.0, 1.0, 2.0, 2.5):
        _, g = R.elementwise(x, y, gamma, 0.25)
        num = (R.elementwise(x + h, y, gamma, 0.25)[0] - R.elementwise(x - h, y, gamma, 0.25)[0]) / (2 * h)
        assert np.abs(g - num).max() <= 1e-8 * max(1.0, np.abs(g).max())
    # +-80: both tails finite and non-zero where float64 can hold them
    l, g = R.elementwise(np.array([80.0, -80.0, 80.0, -80.0]), np.array([1.0, 0.0, 0.0, 1.0]), 0.0, 0.25)
    assert np.isfinite(l).all() and np.isfinite(g).all() and (g != 0).all()
    assert g[0] == pytest.approx(-0.25 * np.exp(-80.0), rel=1e-12) and g[2] == pytest.approx(0.75, rel=1e-12)


# ----------------------------------------------------------------------------------------------------- composed routes
@pytest.mark.parametrize("L", sorted(C.OMEGA))
@pytest.mark.parametrize("window,radius", C.WINDOW_CASES)
def test_coder_encode_and_decode_match_the_restatement(L, window, radius):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils.registry import BOXES, build_from_cfg
    omega, radius = C.OMEGA[L], C.fit_radius(window, radius, L)
    coder = build_from_cfg(dict(type="CSLCoder", omega=omega, window=window, radius=radius), BOXES)
    assert coder.coding_len == L and coder.angle_range == 180 and coder.angle_offset == 45
    a = np.concatenate([C.targets(np.random.default_rng(L), 50, omega), C.EXACT_TARGETS])
    ref = R.labels(R.bins(a, omega), L, window, radius)
    for dtype in (torch.float32, torch.float64):
        got = coder.encode(torch.from_numpy(a).to(dtype)[:, None])
        assert got.shape == (a.shape[0], L) and got.dtype == dtype
        assert torch.equal(coder.bins(torch.from_numpy(a)[:, None])[:, 0], torch.from_numpy(R.bins(a, omega)))
        assert (np.abs(got.double().numpy() - ref) <= (R.ulp32(ref) if dtype == torch.float32 else 1e-15)).all()
    x = C.decode_logits(np.random.default_rng(L + 1), 23, L)
    idx, ang = R.decode(x, omega)
    got = coder.decode(torch.from_numpy(x))
    assert got.shape == (23,) and (np.abs(got.double().numpy() - ang) <= R.ulp32(ang)).all()
    assert np.array_equal(C.index_of_angle(got.numpy(), omega), idx)
    keep = torch.tensor([5, 0, 22, 7])
    assert torch.equal(coder.decode(torch.from_numpy(x), index=keep), got[keep])


def test_over_wide_windows_and_empty_codes_are_refused():
    from jdet_amd.models.boxes.coder import CSLCoder
    for window in ("rect", "triangle"):
        CSLCoder(omega=4, window=window, radius=22)
        with pytest.raises(ValueError):
            CSLCoder(omega=4, window=window, radius=23)          # 46 > 45 bins
        with pytest.raises(ValueError):
            CSLCoder(omega=90, window=window, radius=2)
    with pytest.raises(ValueError):
        CSLCoder(omega=181)
    with pytest.raises(ValueError):
        CSLCoder(window="gaussian", radius=0)
    CSLCoder(omega=90, window="gaussian", radius=6)             # gaussian offsets may meet: the largest wins


@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0, 2.5])
@pytest.mark.parametrize("sel", ["all", "random", "last"])
def test_composed_loss_matches_the_restatement(gamma, sel):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.models.losses.smooth_focal_loss import csl_angle_loss
    from jdet_amd.utils.registry import BOXES, LOSSES, build_from_cfg
    f = C.loss_fixture(126, 45, "gaussian", 3, gamma if gamma != 2.5 else 2.0, sel)
    ref = R.angle_loss(f["logits"], f["target"], f["weight"], 4, "gaussian", 3, gamma, C.ALPHA, C.AVG, C.LOSS_WEIGHT)
    lw = float(np.float32(C.LOSS_WEIGHT))                     # the restatement takes it as the C ABI does, a float32
    fn = build_from_cfg(dict(type="SmoothFocalLoss", gamma=gamma, alpha=C.ALPHA, loss_weight=lw), LOSSES)
    coder = build_from_cfg(dict(type="CSLCoder", omega=4, window="gaussian", radius=3), BOXES)
    x = torch.from_numpy(f["logits"]).double().requires_grad_(True)
    rng = np.random.default_rng(1)
    # the level's windows as the head passes them: (B, n, 5), column 4 the angle's
    t5, w5 = (torch.from_numpy(C._rows5(f[k], False, rng)).double().reshape(2, 63, 5) for k in ("target", "weight"))
    loss = csl_angle_loss(fn, coder, x, t5, w5, C.AVG)
    loss.backward()
    assert abs(float(loss.detach()) - ref[0]) <= 1e-12 * max(1.0, abs(ref[0]))
    unit = x.grad.numpy() * (C.AVG / lw)
    assert np.abs(unit - ref[1]).max() <= 1e-12 * np.abs(ref[1]).max()
    assert (x.grad.numpy()[f["weight"] <= 0] == 0).all()


def test_no_selected_row_takes_the_early_return():
    from jdet_amd.models.losses.smooth_focal_loss import SmoothFocalLoss
    fn = SmoothFocalLoss(loss_weight=0.8)
    x = torch.full((5, 45), float("nan")).requires_grad_(True)          # nothing selected: nothing may be looked at
    for w in (torch.zeros(5), torch.tensor([0.0, -1.0, 0.0, -2.0, 0.0]), torch.zeros(5, 1)):
        loss = fn(x, torch.zeros(5, 45), weight=w, avg_factor=3.0)
        assert loss.dim() == 0 and float(loss.detach()) == 0.0 and loss.requires_grad       # value 0, graph kept
        (g,) = torch.autograd.grad(loss, x)
        assert torch.equal(g, torch.zeros_like(x))
    # the weight is a mask, not a factor
    y = torch.rand(4, 45)
    z = torch.randn(4, 45)
    a = fn(z, y, weight=torch.tensor([1.0, 0.0, 1.0, 0.0]), avg_factor=2.0)
    b = fn(z, y, weight=torch.tensor([9.0, -3.0, 0.5, 0.0]), avg_factor=2.0)
    assert torch.equal(a, b) and fn(z, y, weight=torch.tensor([1.0, 0, 1, 0]), reduction_override="none").shape == (2, 45)


# ---------------------------------------------------------------------------------------------------------------- ABI
def _declared():
    src = open(os.path.join(ROOT, "include", "jdet_hip_csl.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|size_t)\s+(jdet_\w+)\s*\(([^)]*)\)\s*;", src):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
    return out


@pytest.fixture(scope="module")
def built():
    from jdet_amd import _lib
    _lib.build()
    return _lib


def test_header_table_and_exports_agree(built):
    d = _declared()
    assert set(d) == set(built.CSL_SIGNATURES) == {"jdet_csl_encode", "jdet_csl_decode", "jdet_csl_angle_loss_level"}
    assert not set(d) & set(built.SIGNATURES) and not set(d) & set(built.RETINA_SIGNATURES)
    raw = ctypes.CDLL(built.LIB_PATH)
    lib = built.lib()
    for name, nargs in d.items():
        res, args = built.CSL_SIGNATURES[name]
        assert len(args) == nargs, name
        assert hasattr(raw, name), "missing export " + name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    assert built.CSL_WINDOWS == C.WINDOW_ID


def test_argument_validation_returns_before_any_launch(built):
    """every answer comes from the host-side checks: no device here, and a launch on these addresses would not return"""
    lib = built.lib()
    N, X = None, 4096                                        # X: a non-null address nobody reads
    nan, inf = float("nan"), float("inf")
    need = lib.jdet_sigmoid_focal_loss_workspace()
    G, T, RE, P_ = 3, 2, 1, 0

    def enc(a=X, n=4, L=45, omega=4.0, window=G, radius=3.0, out=X):
        return lib.jdet_csl_encode(a, n, L, omega, window, radius, out, N)

    def dec(x=X, rows=8, index=X, n=4, L=45, omega=4.0, out=X):
        return lib.jdet_csl_decode(x, rows, index, n, L, omega, out, N)

    def loss(x=X, t=X, tr=4, ts=4, w=X, wr=4, wst=4, rows=4, L=45, omega=4.0, window=G, radius=3.0, gamma=2.0, alpha=0.25,
             avg=X, lw=1.0, out=X, g=X, ws=X, wsb=need):
        return lib.jdet_csl_angle_loss_level(x, t, tr, ts, w, wr, wst, rows, L, omega, window, radius, gamma, alpha, avg,
                                             lw, out, g, ws, wsb, N)
    for f in (enc, dec, loss):
        assert f(L=0) == -1 and f(L=-3) == -1 and f(L=181) == -2 and f(L=1000) == -2
        assert f(omega=0.0) == -1 and f(omega=-4.0) == -1 and f(omega=nan) == -1 and f(omega=inf) == -1
    for f in (enc, loss):
        assert f(window=4) == -1 and f(window=-1) == -1
        assert f(radius=0.0) == -1 and f(radius=nan) == -1 and f(radius=-3.0) == -1 and f(radius=inf) == -1
        for window in (RE, T):
            assert f(window=window, radius=23.0) == -1 and f(window=window, radius=2.5) == -1      # 46 > 45; an integer
            assert f(window=window, radius=0.0) == -1
    # pulse has no radius: a NaN radius passes the label check, seen on paths that return before any launch
    assert enc(window=P_, radius=nan, n=0, a=N, out=N) == 0 and enc(window=G, radius=nan, n=0, a=N, out=N) == -1
    assert loss(window=P_, radius=nan, gamma=0.5) == -2 and loss(window=G, radius=nan, gamma=0.5) == -1
    assert enc(a=N) == -1 and enc(out=N) == -1 and enc(n=-1) == -1 and enc(n=0, a=N, out=N) == 0
    assert enc(n=2 ** 31 // 45 + 1) == -2
    assert dec(x=N) == -1 and dec(out=N) == -1 and dec(n=-1) == -1 and dec(rows=-1) == -1 and dec(n=0, x=N, out=N) == 0
    assert dec(index=N, n=9, rows=8) == -1                                                        # row i of 8 rows
    for null in ("x", "t", "w", "avg", "out", "g", "ws"):
        assert loss(**{null: N}) == -1, null
    assert loss(rows=-1) == -1 and loss(tr=0) == -1 and loss(ts=-1) == -1 and loss(wr=0) == -1 and loss(wst=-1) == -1
    assert loss(gamma=-1.0) == -1 and loss(gamma=nan) == -1 and loss(alpha=nan) == -1 and loss(lw=inf) == -1
    assert loss(gamma=0.5) == -2 and loss(gamma=0.999) == -2 and loss(rows=2 ** 40) == -2
    assert loss(wsb=need - 1) == -3 and loss(wsb=0) == -3 and loss(ws=X + 4) == -1                # doubles live there


def test_op_routes_raise_or_compose_on_cpu_tensors():
    """no silent device work on CPU tensors: the coder and the loss compose; the node is not chosen"""
    from jdet_amd.models.boxes.coder import CSLCoder
    from jdet_amd.models.losses import smooth_focal_loss as S
    coder = CSLCoder(omega=4, window="gaussian", radius=3)
    x = torch.zeros(4, 45)
    assert not S._level_ok(S.SmoothFocalLoss(), coder, x, torch.zeros(4, 5), torch.zeros(4, 5), torch.tensor(1.0))


def test_every_entry_point_dry_runs(built, monkeypatch):
    """the protocol of tests/test_guarded_cpu.py's dry run on the smallest cases: argument lists fit the ctypes
    signatures, each row calls exactly what it names, the references evaluate with the outputs' sizes"""
    from tests import abi_cases, guarded as G
    from tests.test_guarded_cpu import _DryLib
    covered = set()
    for case in C.smallest_cases():
        called = set()
        monkeypatch.setattr(abi_cases, "lib", lambda called=called: _DryLib(built.lib(), built.CSL_SIGNATURES, called))
        run = G.Run("cpu", "A")
        res = case.fn(run)
        assert called == set(case.entry_points), (case.id, sorted(called))
        covered |= called
        refs = res.ref()
        assert set(refs) == set(res.outs), case.id
        for k, (ref, bound) in refs.items():
            b = np.asarray(bound, np.float64)
            assert np.isfinite(b).all() and (b > 0).all(), (case.id, k)
            assert np.asarray(ref).size == res.outs[k].numel() and (b.ndim == 0 or b.size == res.outs[k].numel())
            assert np.isfinite(np.asarray(ref, np.float64)).all(), (case.id, k)
    assert covered == set(built.CSL_SIGNATURES)


def test_fixture_conditions():
    for L, omega in C.OMEGA.items():
        a = C.targets(np.random.default_rng(L), 300, omega)       # asserts the distance from the bin edges itself
        t = R.bins(a, omega)
        assert {0, L - 1} <= set(t.tolist())
        y = R.labels(t[:4], L, "gaussian", 3)
        assert (y[0, [0, L - 1]] > 0).all() and (y[3, [0, L - 1]] > 0).all()      # the window wraps past both ends
    f = C.loss_fixture(257, 45, "gaussian", 3, 2.0, "all")
    assert np.array_equal(f["target"][-8:], C.EXACT_TARGETS)
    q = R.quotient64(f["target"][:-8], 4)
    assert (np.abs(q - np.round(q)) >= 1e-3).all()
    r = C.loss_fixture(3062, 45, "gaussian", 3, 2.0, "random")
    assert 10 <= int((r["weight"] > 0).sum()) <= 80 and (r["weight"] < 0).any()


def test_grid_cap_constants_are_the_kernels(built):
    src = open(os.path.join(ROOT, "jdet_amd", "csrc", "csl.hip")).read()
    assert int(re.search(r"constexpr int kTileRows = (\d+);", src).group(1)) == C.TILE_ROWS
    assert "kSumGridCap = (int)(kJdetLossWorkspaceBytes / sizeof(double))" in src
    assert built.lib().jdet_sigmoid_focal_loss_workspace() // 8 == C.SUM_GRID_CAP
    red = open(os.path.join(ROOT, "jdet_amd", "csrc", "reduce.h")).read()
    assert int(re.search(r"constexpr int kJdetLossGridCap = (\d+);", red).group(1)) == C.REDUCE_GRID_CAP


# ---------------------------------------------------------------------------------------------------- registry, config
def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return [_plain(x) for x in v] if isinstance(v, (list, tuple)) else v


def test_named_config_equals_the_reference_file_and_builds():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.config import Config, named
    from jdet_amd.utils import registry as Reg
    cfg = named.CSL_RETINANET_CFG
    c = Config(os.path.join(ROOT, "tests", "golden", "configs",
                            "rotated_retinanet_obb_csl_gaussian_r50_fpn_1x_dota.yaml")).dump()
    for k in ("model", "optimizer", "scheduler"):
        assert _plain(cfg[k]) == _plain(c[k]), k
    assert cfg["optimizer"]["lr"] == 0.0025
    for name, reg in (("CSLRRetinaHead", Reg.HEADS), ("CSLCoder", Reg.BOXES), ("SmoothFocalLoss", Reg.LOSSES)):
        assert reg.get(name) is not None, name
    m = Reg.build_from_cfg(dict(cfg["model"], backbone=dict(cfg["model"]["backbone"], pretrained=False)), Reg.MODELS)
    h = m.bbox_head
    assert type(h).__name__ == "CSLRRetinaHead" and isinstance(h, Reg.HEADS.get("RotatedRetinaHead"))
    assert h.coding_len == 45 and h.angle_coder.window == "gaussian" and h.angle_coder.radius == 3
    assert h.retina_angle_cls.out_channels == 405 and h.retina_angle_cls.kernel_size == (3, 3)
    assert h.retina_angle_cls.padding == (1, 1) and h.retina_angle_cls.in_channels == 256
    assert float(h.retina_angle_cls.bias[0].detach()) == pytest.approx(-np.log(99.0))
    assert h.loss_angle.loss_weight == 0.8 and h.loss_angle.gamma == 2.0 and h.loss_angle.alpha == 0.25


def _given_targets(anchor_list, valid_flag_list, gt_bboxes, img_metas, means, stds, cfg, **kw):
    """what anchor_target returns, without the device (the product has no CPU assigner): three positives per image on
    the two finest levels"""
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


def test_head_returns_three_maps_and_three_finite_losses_on_cpu():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.config.named import CSL_RETINANET_CFG
    from jdet_amd.utils import registry as Reg
    from jdet_amd.utils.general import parse_losses
    torch.manual_seed(0)
    h = Reg.build_from_cfg(dict(CSL_RETINANET_CFG["model"]["bbox_head"], stacked_convs=1), Reg.HEADS)
    h.anchor_target = _given_targets
    feats = [torch.randn(2, 256, s, s) for s in (8, 4, 2, 1, 1)]
    outs = h.forward_single(feats[0])
    assert [tuple(o.shape) for o in outs] == [(2, 135, 8, 8), (2, 45, 8, 8), (2, 405, 8, 8)]
    targets = [dict(rboxes=torch.zeros((1, 5)), labels=torch.ones((1,), dtype=torch.int32), rboxes_ignore=torch.zeros((0, 5)),
                    img_size=(64, 64), scale_factor=1.0, pad_shape=(64, 64)) for _ in range(2)]
    h.train()
    out = h(feats, targets)
    assert set(out) == {"loss_cls", "loss_bbox", "loss_angle"}
    assert all(len(v) == 5 and all(torch.isfinite(x) for x in v) for v in out.values())
    assert float(out["loss_angle"][0].detach()) > 0 and float(out["loss_angle"][1].detach()) > 0
    assert all(float(x.detach()) == 0.0 for x in out["loss_angle"][2:])                          # levels without a positive
    total, _ = parse_losses(out)
    total.backward()
    assert h.retina_angle_cls.weight.grad.abs().max() > 0 and torch.isfinite(h.retina_angle_cls.weight.grad).all()
