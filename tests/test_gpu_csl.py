"""GPU: Circular Smooth Label -- the kernels of csrc/csl.hip (jdet_csl_angle_loss_level, jdet_csl_encode,
jdet_csl_decode) against the float64 restatements of tests/csl_ref.py in every regime, their buffer contracts
(tests/guarded.py: guard bands, poisoned outputs and workspace, inputs unchanged, run B == run A bit for bit, a short
workspace refused), the autograd node against float64 and against the composed route, and CSL_RETINANET_CFG end to end.

Bounds.  The kernels compute in double and round once: the loss, every gradient element, every label and every angle
must lie within ONE float32 spacing of the float64 restatement (csl_ref.ulp32; 1.2e-38 below the normal range).  The
hostile run of every case holds NaN in the logits and targets of the unselected rows and in the columns nobody may read,
and must equal the clean run bit for bit: of an unselected row only the weight is read, its gradient row is exact zeros.

The node's gradient leaves through jdet_loss_grad_scale -- unit * ((grad_out * loss_weight) / avg_factor) in float32:
four roundings of 2^-24 each (the unit gradient, the product, the quotient, the final product), so 4.5 * 2^-24 relative.
Fused against composed: twice the composed route's own error against float64, measured here and printed.

Regimes: tiles of 64 rows (rows 1, 63, 257 and a two-block window of 2 x 1531), L = 2 (a float4 spans two rows), 45
(idle lanes, rows straddle float4s), 64 (a full wave), 180 (three trips); more tiles than the kernel's grid cap of 512 workgroups
(32 769 rows) and than reduce.h's 1024 (65 537 rows); the unaligned (scalar-store) route; gamma 0 / 1 / 2 and the pow() route (2.5)."""
import math

import numpy as np
import pytest
import torch

from tests import csl_cases as C
from tests import csl_ref as R

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------------- the level loss
@pytest.mark.parametrize("L", sorted(C.OMEGA))
@pytest.mark.parametrize("rows", [1, 63, 257, 2 * 1531])
def test_loss_contract_and_float64(dev, rows, L):
    """every selection x every window, the three gammas rotating so that each meets every window and every selection"""
    from tests import guarded
    for si, sel in enumerate(C.SELECTIONS):
        for wi, (window, radius) in enumerate(C.WINDOW_CASES):
            gamma = (0.0, 1.0, 2.0)[(si + wi) % 3]
            c = C.loss_case(rows, L, window, C.fit_radius(window, radius, L), gamma, sel, windowed=rows == 2 * 1531)
            guarded.run_case(c.entry_points[0], c.label, c.fn, dev)


@pytest.mark.parametrize("case", ["capped grid", "capped grid 1024", "unaligned", "unaligned L2", "+-80", "+-80 gamma 0", "pow"])
def test_loss_contract_large_unaligned_and_extreme(dev, case):
    from tests import guarded
    # one tile more than the kernel's grid has workgroups (512: the smallest such row count), and than reduce.h's cap
    c = {"capped grid": lambda: C.loss_case(C.TILE_ROWS * C.SUM_GRID_CAP + 1, 2, "gaussian", 3, 2.0, "random"),
         "capped grid 1024": lambda: C.loss_case(C.TILE_ROWS * C.REDUCE_GRID_CAP + 1, 2, "gaussian", 3, 2.0, "random"),
         "unaligned": lambda: C.loss_case(257, 45, "gaussian", 3, 2.0, "random", unaligned=True),
         "unaligned L2": lambda: C.loss_case(63, 2, "pulse", 1, 1.0, "all", unaligned=True),
         "+-80": lambda: C.loss_case(63, 45, "gaussian", 3, 2.0, "all", extreme=True),
         "+-80 gamma 0": lambda: C.loss_case(63, 180, "pulse", 1, 0.0, "all", extreme=True),
         "pow": lambda: C.loss_case(257, 64, "triangle", 4, 2.5, "random")}[case]()
    guarded.run_case(c.entry_points[0], c.label, c.fn, dev)
    if case.startswith("+-80"):
        f = C.loss_fixture(63, 45 if case == "+-80" else 180, "gaussian" if case == "+-80" else "pulse",
                           3 if case == "+-80" else 1, 2.0 if case == "+-80" else 0.0, "all", True)
        assert np.isfinite(f["ref"][0]) and np.isfinite(f["ref"][1]).all() and (np.abs(f["logits"]) == 80).any()


# ------------------------------------------------------------------------------------------------------ encode / decode
@pytest.mark.parametrize("L", sorted(C.OMEGA))
def test_encode_contract_and_float64(dev, L):
    from tests import guarded
    for window, radius in C.WINDOW_CASES:
        for n in (1, 63, 257):
            c = C.encode_case(n, L, window, C.fit_radius(window, radius, L))
            guarded.run_case(c.entry_points[0], c.label, c.fn, dev)


@pytest.mark.parametrize("L", sorted(C.OMEGA))
def test_decode_contract_index_and_angle(dev, L, monkeypatch):
    """with and without an index list, ties (the first wins), the maximum in the last bin, constant rows: the angle within
    one spacing, and the bin it stands for equal to numpy's first argmax"""
    from tests import guarded
    from jdet_amd.models.boxes import coder as K
    monkeypatch.setattr(K, "CSL_FUSED", True)
    for rows in (1, 5, 63, 257):
        for indexed in (False, True):
            c = C.decode_case(rows, L, indexed)
            guarded.run_case(c.entry_points[0], c.label, c.fn, dev)
    coder = K.CSLCoder(omega=C.OMEGA[L], window="pulse")
    x = C.decode_logits(np.random.default_rng(L), 257, L)
    idx, _ = R.decode(x, C.OMEGA[L])
    assert (idx == L - 1).any() and (idx == 0).any()
    xd = _dev(x, dev)
    keep = torch.from_numpy(np.random.default_rng(1).permutation(257)[:100]).to(dev)
    got, got_kept = coder.decode(xd), coder.decode(xd, index=keep)
    assert np.array_equal(C.index_of_angle(got.cpu().numpy(), C.OMEGA[L]), idx)
    assert torch.equal(got_kept, got[keep]) and torch.equal(xd.cpu(), torch.from_numpy(x))
    # the reference's route -- the argmax of float32 sigmoids -- agrees on these rows (gaps of 1e-2 or ties)
    monkeypatch.setattr(K, "CSL_FUSED", False)
    assert torch.equal(coder.decode(xd.sigmoid()), got) and torch.equal(coder.decode(xd, index=keep), got_kept)


def test_coder_encode_fused_equals_composed_on_the_device(dev, monkeypatch):
    from jdet_amd.models.boxes import coder as K
    for L, omega in C.OMEGA.items():
        for window, radius in C.WINDOW_CASES:
            coder = K.CSLCoder(omega=omega, window=window, radius=C.fit_radius(window, radius, L))
            a = np.concatenate([C.targets(np.random.default_rng(L), 200, omega), C.EXACT_TARGETS])
            ad = _dev(a, dev)[:, None]
            monkeypatch.setattr(K, "CSL_FUSED", True)
            fused = coder.encode(ad)
            monkeypatch.setattr(K, "CSL_FUSED", False)
            comp = coder.encode(ad)
            monkeypatch.setattr(K, "CSL_FUSED", True)
            ref = R.labels(R.bins(a, omega), L, window, coder.radius)
            assert torch.equal(coder.bins(ad)[:, 0].cpu(), torch.from_numpy(R.bins(a, omega)))      # float32 on the device
            for got in (fused, comp):
                assert got.shape == (a.shape[0], L) and got.dtype == torch.float32
                assert (np.abs(got.double().cpu().numpy() - ref) <= R.ulp32(ref)).all()


# ------------------------------------------------------------------------------------------------------------- the node
def _node_inputs(dev, f, rows):
    B = 2 if rows % 2 == 0 else 1
    n = rows // B
    rng = np.random.default_rng(2)
    t5, w5 = (C.window5(C._rows5(f[k], False, rng).reshape(B, n, 5), n + 69, 7) for k in ("target", "weight"))
    return _dev(t5, dev)[:, 7:7 + n], _dev(w5, dev)[:, 7:7 + n], torch.tensor(C.AVG, device=dev)


def _grad_error(g, g64):
    return float(np.abs(np.asarray(g, np.float64) - g64).max() / np.abs(g64).max())


@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0])
def test_node_against_float64_and_the_composed_route(dev, gamma, monkeypatch):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.models.boxes import coder as K
    from jdet_amd.models.losses import smooth_focal_loss as S
    lw = float(np.float32(C.LOSS_WEIGHT))
    fn = S.SmoothFocalLoss(gamma=gamma, alpha=C.ALPHA, loss_weight=lw)
    for rows, L, window, radius, sel in ((257, 45, "gaussian", 3, "all"), (2 * 1531, 45, "gaussian", 3, "random"),
                                         (2 * 1531, 180, "gaussian", 6, "all"), (63, 64, "triangle", 4, "all")):
        f = C.loss_fixture(rows, L, window, radius, gamma, sel)
        coder = K.CSLCoder(omega=C.OMEGA[L], window=window, radius=radius)
        t, w, avg = _node_inputs(dev, f, rows)
        loss64, unit64 = f["ref"]
        g64 = unit64 * (lw / C.AVG)

        def run(fused):
            monkeypatch.setattr(K, "CSL_FUSED", fused)
            x = _dev(f["logits"], dev).requires_grad_(True)
            assert S._level_ok(fn, coder, x, t, w, avg) == fused
            loss = S.csl_angle_loss(fn, coder, x, t, w, avg)
            (loss * 3.0).backward()
            return float(loss.detach()), x.grad.double().cpu().numpy() / 3.0, x.grad
        l1, g1, raw1 = run(True)
        l2, g2, _ = run(False)
        l3, _, raw3 = run(True)
        e_loss, e_grad = abs(l2 - loss64), _grad_error(g2, g64)
        print("node rows %d L %d %s gamma %g %s: loss error fused %.3e composed %.3e, fused - composed %.3e (bound %.3e); "
              "grad error fused %.3e composed %.3e, fused - composed %.3e (bound %.3e)" % (
                  rows, L, window, gamma, sel, abs(l1 - loss64), e_loss, abs(l1 - l2), 2 * e_loss,
                  _grad_error(g1, g64), e_grad, _grad_error(g1, g2), 2 * e_grad))
        assert abs(l1 - loss64) <= float(R.ulp32(loss64))
        assert (np.abs(g1 - g64) <= 4.5 * 2.0 ** -24 * np.abs(g64) + 1.2e-38).all()
        assert (g1[f["weight"] <= 0] == 0).all()
        assert abs(l1 - l2) <= 2 * e_loss and _grad_error(g1, g2) <= 2 * e_grad
        assert l1 == l3 and torch.equal(raw1, raw3)


def test_node_runs_without_a_host_sync(dev, monkeypatch):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.models.boxes import coder as K
    from jdet_amd.models.boxes.coder import CSLCoder
    from jdet_amd.models.losses import smooth_focal_loss as S
    monkeypatch.setattr(K, "CSL_FUSED", True)
    f = C.loss_fixture(257, 45, "gaussian", 3, 2.0, "random")
    fn, coder = S.SmoothFocalLoss(loss_weight=float(np.float32(C.LOSS_WEIGHT))), CSLCoder(omega=4, window="gaussian", radius=3)
    t, w, avg = _node_inputs(dev, f, 257)
    x = _dev(f["logits"], dev).requires_grad_(True)
    zero = torch.zeros_like(w)
    S.csl_angle_loss(fn, coder, x, t, w, avg).backward()                         # warm up: code objects, allocator
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = S.csl_angle_loss(fn, coder, x, t, w, avg)
        b = S.csl_angle_loss(fn, coder, x, t, zero, avg)                         # a level without a selected row
        (a + b).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(b.detach()) == 0.0 and abs(float(a.detach()) - f["ref"][0]) <= float(R.ulp32(f["ref"][0]))
    assert torch.isfinite(x.grad).all() and (x.grad.cpu().numpy()[f["weight"] <= 0] == 0).all()


# ------------------------------------------------------------------------------------------------------------ detector
def _detector(dev):
    """CSL_RETINANET_CFG on an R18 backbone, 2 x 128^2 with 4 boxes per image: levels of 16^2 .. 1^2 positions, the
    coarsest without a positive"""
    import copy
    from jdet_amd.config.named import CSL_RETINANET_CFG, DIST_RETINANET_R18_CFG
    from jdet_amd.runner import Runner, synthetic_batch
    cfg = copy.deepcopy(CSL_RETINANET_CFG)
    for k in ("backbone", "neck"):
        cfg["model"][k] = copy.deepcopy(DIST_RETINANET_R18_CFG["model"][k])
    cfg["scheduler"] = None                                  # no warm-up: ten steps at the config's learning rate
    images, targets = synthetic_batch(2, 128, dev, seed=3, num_gts=4)
    torch.manual_seed(0)
    r = Runner(cfg, device=dev, conv_autotune=False, graph=False)
    return cfg, r, images, targets


def _step(m, images, targets):
    from jdet_amd.utils.general import parse_losses
    m.zero_grad(set_to_none=True)
    out = m(images, targets)
    total, _ = parse_losses(out)
    total.backward()
    return ({k: [float(x.detach()) for x in v] for k, v in out.items()},
            m.bbox_head.retina_angle_cls.weight.grad.detach().double().cpu().numpy().copy())


def _float64_angle_branch(m, images, targets, monkeypatch):
    """what the angle branch computes behind its float32 inputs, in float64: per level the restated loss on the logits and
    the target / weight windows the head hands to csl_angle_loss, and d (sum of the levels) / d retina_angle_cls.weight --
    the restated logit gradients through the prediction layer's float64 backward on the tower output it read"""
    import torch.nn.functional as F
    from jdet_amd.models.roi_heads import csl_rretina_head as H
    from jdet_amd.models.utils.level_pack import LevelPack
    h = m.bbox_head
    seen, feats = [], []
    real_loss, real_towers = H.csl_angle_loss, h._towers

    def spy_loss(fn, coder, logits, t, w, avg):
        seen.append((logits.detach().cpu().numpy(), t.detach().cpu().numpy().reshape(-1, 5)[:, 4],
                     w.detach().cpu().numpy().reshape(-1, 5)[:, 4], float(avg)))
        return real_loss(fn, coder, logits, t, w, avg)

    def spy_towers(x, mask=None):
        out = real_towers(x, mask)
        feats.append(out[1].detach().cpu().double())
        return out
    monkeypatch.setattr(H, "csl_angle_loss", spy_loss)
    monkeypatch.setattr(h, "_towers", spy_towers)
    m(images, targets)
    monkeypatch.setattr(H, "csl_angle_loss", real_loss)
    monkeypatch.setattr(h, "_towers", real_towers)
    assert len(seen) == 5 and len(feats) == 1                # five small levels: one packed pass through the towers
    c, fn = h.angle_coder, h.loss_angle
    w64 = h.retina_angle_cls.weight.detach().cpu().double().requires_grad_(True)
    y = F.conv2d(feats[0], w64, h.retina_angle_cls.bias.detach().cpu().double(), padding=1)
    B = images.shape[0]
    hw = [(s, s) for s in (16, 8, 4, 2, 1)]
    levels = LevelPack.cached(hw, images.device)._slices(y)
    losses, grads = [], []
    for (x, t, w, avg), (hh, ww) in zip(seen, hw):
        l64, unit = R.angle_loss(x, t, w, c.omega, c.window, c.radius, fn.gamma, fn.alpha, avg, fn.loss_weight)
        losses.append(l64)
        g = unit * (float(np.float32(fn.loss_weight)) / float(np.float32(avg)))
        grads.append(torch.from_numpy(g).reshape(B, hh, ww, -1).permute(0, 3, 1, 2))
    (gw,) = torch.autograd.grad(levels, w64, grad_outputs=grads)
    return losses, gw.numpy()


def test_detector_trains_fused_equals_composed(dev, monkeypatch):
    """three finite loss lists; loss_angle > 0 where a level holds positives and exactly 0 on the coarsest; fused = composed
    in loss_angle and retina_angle_cls.weight.grad within twice the composed route's own error against float64; the
    total falling over 10 SGD steps on the batch"""
    from jdet_amd.models.boxes import coder as K
    cfg, r, images, targets = _detector(dev)
    m = r.model
    m.train()
    assert type(m.bbox_head).__name__ == "CSLRRetinaHead" and m.bbox_head.coding_len == 45
    loss64, gw64 = _float64_angle_branch(m, images, targets, monkeypatch)
    monkeypatch.setattr(K, "CSL_FUSED", True)
    fused, gf = _step(m, images, targets)
    monkeypatch.setattr(K, "CSL_FUSED", False)
    comp, gc = _step(m, images, targets)
    monkeypatch.setattr(K, "CSL_FUSED", True)
    assert set(fused) == {"loss_cls", "loss_bbox", "loss_angle"}
    assert all(len(v) == 5 and all(math.isfinite(x) for x in v) for v in fused.values())
    assert fused["loss_angle"][-1] == 0.0 and comp["loss_angle"][-1] == 0.0 and loss64[-1] == 0.0
    assert max(fused["loss_angle"]) > 0 and all((a > 0) == (b > 0) for a, b in zip(fused["loss_angle"], loss64))
    for lvl, (a, b, ref) in enumerate(zip(fused["loss_angle"], comp["loss_angle"], loss64)):
        print("loss_angle level %d: float64 %.9f, fused error %.3e, composed error %.3e, fused - composed %.3e (bound %.3e)"
              % (lvl, ref, abs(a - ref), abs(b - ref), abs(a - b), 2 * abs(b - ref)))
        assert abs(a - ref) <= float(R.ulp32(ref)) if ref else a == 0.0
        assert abs(a - b) <= 2 * abs(b - ref), lvl
    ef, ec, efc = _grad_error(gf, gw64), _grad_error(gc, gw64), _grad_error(gf, gc)
    print("retina_angle_cls.weight.grad: error fused %.3e composed %.3e, fused - composed %.3e (bound %.3e)"
          % (ef, ec, efc, 2 * ec))
    assert np.isfinite(gf).all() and np.abs(gf).max() > 0 and efc <= 2 * ec
    hist = [float(r.train_step(images, targets)[0]) for _ in range(10)]
    print("CSL_RETINANET_CFG (R18) total loss", np.round(hist, 4).tolist())
    assert np.all(np.isfinite(hist)) and hist[-1] < hist[0]


def test_detector_infers_the_same_bins_on_both_routes(dev, monkeypatch):
    """polygons / scores / labels of one length, finite; on the same head outputs, the bins decoded from the logits in
    place equal the bins of the reference's route (float32 sigmoid of the whole map, gather, argmax) on every kept row
    whose float32 sigmoid does not tie two different logits -- such rows are printed --, and the detections are identical
    when there is none.  Both routes cut with the same `topk` on the same scores: the kept rows are the same rows."""
    from jdet_amd.models.boxes import coder as K
    from jdet_amd.models.utils.level_pack import run_levels
    cfg, r, images, targets = _detector(dev)
    m = r.model
    m.eval()
    h = m.bbox_head
    h.test_cfg["nms_pre"] = 300                              # the two finest levels (2304, 576 rows) are cut
    real = h._level_angles
    rows = {}

    def spy(angle_cls, keep):
        out = real(angle_cls, keep)
        x = angle_cls.permute(1, 2, 0).reshape(-1, h.coding_len)
        k = np.arange(x.shape[0]) if keep is None else keep.cpu().numpy()
        rows.setdefault(K.CSL_FUSED, []).append((k, out.cpu().numpy(), x.cpu().numpy()[k]))
        return out
    monkeypatch.setattr(h, "_level_angles", spy)
    res = {}
    with torch.no_grad():
        h.retina_cls.bias.fill_(-2.0)
        outs = tuple(map(list, zip(*run_levels(list(m.neck(m.backbone(images))),
                                               lambda x, mask: h.forward_single(x, mask=mask)))))
        metas = h.parse_targets(targets, is_train=False)
        for fused in (True, False):
            monkeypatch.setattr(K, "CSL_FUSED", fused)
            res[fused] = h.get_bboxes(*outs, metas)
    monkeypatch.setattr(K, "CSL_FUSED", True)
    assert len(res[True]) == 2
    for polys, scores, labels in res[True]:
        assert polys.dim() == 2 and polys.shape[1] == 8 and polys.shape[0] == scores.shape[0] == labels.shape[0]
        assert 0 < polys.shape[0] <= cfg["model"]["bbox_head"]["test_cfg"]["max_per_img"]
        assert torch.isfinite(polys).all() and torch.isfinite(scores).all()
    tied = 0
    assert len(rows[True]) == len(rows[False]) == 10 and rows[True][0][1].shape == (300,)
    for (ka, a, x), (kb, b, x2) in zip(rows[True], rows[False]):
        ia, ib = C.index_of_angle(a, 4), C.index_of_angle(b, 4)
        assert np.array_equal(ia, np.argmax(x, axis=1))                          # exact on the logits
        assert np.array_equal(np.sort(ka), np.sort(kb))                           # the same rows are kept
        _, pa, pb = np.intersect1d(ka, kb, return_indices=True)                  # (matched by anchor index)
        assert len(pa) == len(ka) and np.array_equal(x[pa], x2[pb])
        for k, k2 in zip(pa[ia[pa] != ib[pb]], pb[ia[pa] != ib[pb]]):
            p = torch.from_numpy(x[k]).sigmoid().numpy()
            print("float32 sigmoid tie: logits %.9g (bin %d) and %.9g (bin %d) both give %.9g"
                  % (x[k, ia[k]], ia[k], x[k, ib[k2]], ib[k2], p[ia[k]]))
            assert p[ia[k]] == p[ib[k2]] and x[k, ia[k]] > x[k, ib[k2]] and ib[k2] < ia[k]
            tied += 1
    print("rows whose float32 sigmoid tied: %d" % tied)
    if tied == 0:
        for ra, rb in zip(res[True], res[False]):
            ca, cb = (np.concatenate([t.cpu().numpy().reshape(t.shape[0], -1).astype(np.float64) for t in rr], axis=1)
                      for rr in (ra, rb))
            assert np.array_equal(ca[np.lexsort(ca.T)], cb[np.lexsort(cb.T)])
