"""GPU: the fused Gaussian box-loss node (csrc/gaussian_loss.hip) against the float64 restatement and the package's torch
composition; the dense decoded-box targets; FakeBboxOverlaps2D_rotated; the GWD / KLD / KFIoU RotatedRetinaNet configs
end to end (train, loss falls, no host sync, graph = eager, inference).

Bounds (stated and checked per case below): loss relative error <= 1e-5 and gradient max error <= 1e-4 * max|g_ref|
against float64, except GDLoss's KLD family (1e-4 / 2e-3: a sum of "-1 + small" terms from the twice-divided inverse,
and kld_symmax / kld_symmin pick the other branch on near-ties; 3e-4 on the loss where 1 - 1/(tau + d) meets the
sqrt(1e-7) clamp) and KFIoU's gradient (1e-3: rows whose KF-IoU is near 0 amplify fp32 rounding through -ln / exp).  The
measured error of every case is in profiles/r07_gaussian_losses.txt (section 5)."""
import math

import numpy as np
import pytest
import torch

from tests import gaussian_loss_ref as R

pytestmark = pytest.mark.gpu

# kind, constructor, restatement keywords, decode_pred (GD kinds), loss / gradient bounds
CASES = [
    ("gwd", dict(type="GDLoss", loss_type="gwd", loss_weight=5.0), dict(fun="log1p", tau=0.0), True, 1e-5, 1e-4),
    ("gwd", dict(type="GDLoss", loss_type="gwd", fun="sqrt", tau=1.0), dict(fun="sqrt", tau=1.0), True, 1e-5, 1e-4),
    ("gwd", dict(type="GDLoss", loss_type="gwd", fun="none", tau=2.0, normalize=False),
     dict(fun="none", tau=2.0, normalize=False), True, 1e-5, 1e-4),
    ("kld", dict(type="GDLoss", loss_type="kld", fun="log1p", tau=1.0), dict(fun="log1p", tau=1.0), True, 1e-4, 2e-3),
    ("kld", dict(type="GDLoss", loss_type="kld", fun="none"), dict(fun="none", tau=0.0), True, 1e-4, 2e-3),
    ("jd", dict(type="GDLoss", loss_type="jd", fun="none", sqrt=False), dict(fun="none", tau=0.0, sqrt=False), True,
     1e-4, 2e-3),
    ("kld_symmax", dict(type="GDLoss", loss_type="kld_symmax", fun="none", sqrt=False),
     dict(fun="none", tau=0.0, sqrt=False), True, 1e-4, 2e-3),
    ("kld_symmin", dict(type="GDLoss", loss_type="kld_symmin", fun="sqrt", tau=1.0, sqrt=False),
     dict(fun="sqrt", tau=1.0, sqrt=False), True, 1e-4, 2e-3),
    ("gwd_v1", dict(type="GDLoss_v1", loss_type="gwd", fun="sqrt", tau=2.0), dict(fun="sqrt", tau=2.0), True, 1e-5,
     1e-4),
    ("gwd_v1", dict(type="GDLoss_v1", loss_type="gwd", fun="", tau=1.0), dict(fun="plain", tau=1.0), True, 1e-5, 1e-4),
    ("kld_v1", dict(type="GDLoss_v1", loss_type="kld", fun="log1p", tau=1.0, loss_weight=5.5),
     dict(fun="log1p", tau=1.0), True, 1e-5, 1e-4),
    ("kld_v1", dict(type="GDLoss_v1", loss_type="kld", fun="sqrt", tau=1.0), dict(fun="sqrt", tau=1.0), False, 1e-5,
     1e-4),
    ("bcd_v1", dict(type="GDLoss_v1", loss_type="bcd", fun="log1p", tau=1.0), dict(fun="log1p", tau=1.0), True, 1e-5,
     1e-4),
    ("bcd_v1", dict(type="GDLoss_v1", loss_type="bcd", fun="", tau=2.0), dict(fun="plain", tau=2.0), True, 1e-5, 1e-4),
    # the remaining branches: v1 gwd log1p, bcd sqrt, jd / kld_symmax / kld_symmin with their sqrt
    ("gwd_v1", dict(type="GDLoss_v1", loss_type="gwd", fun="log1p", tau=1.0), dict(fun="log1p", tau=1.0), True, 1e-5,
     1e-4),
    ("bcd_v1", dict(type="GDLoss_v1", loss_type="bcd", fun="sqrt", tau=1.0), dict(fun="sqrt", tau=1.0), True, 1e-5,
     1e-4),
    ("jd", dict(type="GDLoss", loss_type="jd", fun="log1p", tau=1.0), dict(fun="log1p", tau=1.0), True, 1e-4, 2e-3),
    ("kld_symmax", dict(type="GDLoss", loss_type="kld_symmax", fun="none"), dict(fun="none", tau=0.0), True, 1e-4,
     2e-3),
    # (rows clamped at sqrt(1e-7): the loss is a sum of 1 - 1/(1 + log(1 + 3e-4)), four digits lost to fp32 there)
    ("kld_symmin", dict(type="GDLoss", loss_type="kld_symmin", fun="log1p", tau=1.0), dict(fun="log1p", tau=1.0), True,
     3e-4, 2e-3),
    ("kfiou", dict(type="KFLoss", loss_weight=5.0), dict(fun="none"), False, 1e-5, 1e-3),
    ("kfiou", dict(type="KFLoss", fun="ln"), dict(fun="ln"), False, 1e-5, 1e-3),
    ("kfiou", dict(type="KFLoss", fun="exp"), dict(fun="exp"), False, 1e-5, 1e-3),
]


def _build(cfg):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils.registry import LOSSES, build_from_cfg
    return build_from_cfg(dict(cfg), LOSSES)


def _level_inputs(rng, n_img=2, A=10000, pos=0.1):
    """one level: anchors (A, 5), deltas (n_img * A, 5), target / weight as (n_img, A, 5) windows of wider arrays (read
    in place), ~10 % positive rows, hand-built edge rows first (dw / dh clamp, w = h, angle wrap)"""
    anchors = np.concatenate([rng.uniform(0, 1024, (A, 2)), np.exp(rng.uniform(np.log(16), np.log(512), (A, 2))),
                              rng.uniform(-math.pi / 4, 3 * math.pi / 4, (A, 1))], 1).astype(np.float32)
    deltas = rng.normal(0, 0.3, (n_img * A, 5)).astype(np.float32)
    tdel = rng.normal(0, 0.3, (n_img, A, 5)).astype(np.float32)
    deltas[0, 2], deltas[1, 3], deltas[2, 2] = 6.0, -6.0, -4.5
    anchors[3, 3] = anchors[3, 2]
    deltas[3, 2:4] = 0.0
    tdel[0, 3, 2:4] = 0.0
    deltas[4, 4] = 0.74
    anchors[5, 4] = np.float32(3 * math.pi / 4 - 1e-3)
    weight = np.zeros((n_img, A, 5), np.float32)
    weight[rng.uniform(size=(n_img, A)) < pos] = 1.0
    weight[0, :6] = 1.0
    return anchors, deltas, tdel, weight


def _windows(dev, arr, extra=7):
    """(n_img, A, 5) -> a column window of an (n_img, A + extra, 5) device array"""
    n, A, _ = arr.shape
    big = torch.zeros((n, A + extra, 5), dtype=torch.float32, device=dev)
    big[:, 3:3 + A] = torch.from_numpy(arr).to(dev)
    return big[:, 3:3 + A]


@pytest.mark.parametrize("kind,cfg,kw,decoded,ltol,gtol", CASES,
                         ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_kernel_matches_float64_restatement(dev, kind, cfg, kw, decoded, ltol, gtol):
    from jdet_amd.models.boxes.box_ops import delta2bbox_rotated
    from jdet_amd.models.boxes.coder import DeltaXYWHABBoxCoder
    from jdet_amd.models.losses.gaussian_dist_loss import GaussianLevel
    loss = _build(cfg)
    rng = np.random.default_rng(5)
    anchors, deltas, tdel, weight = _level_inputs(rng)
    n_img, A = tdel.shape[:2]
    coder = DeltaXYWHABBoxCoder()
    anc_t = torch.from_numpy(anchors).to(dev)
    all_anc = np.tile(anchors, (n_img, 1))
    if kind == "kfiou":
        target = tdel
    elif decoded:   # the gt boxes (decoded targets, fp32 as the dense targets hold them)
        target = delta2bbox_rotated(torch.from_numpy(all_anc).to(dev), torch.from_numpy(tdel.reshape(-1, 5)).to(dev))
        target = target.cpu().numpy().reshape(n_img, A, 5)
    else:           # undecoded: the boxes are the rows themselves
        target = np.concatenate([anchors[None].repeat(n_img, 0)[..., :2] + tdel[..., :2] * 8,
                                 anchors[None].repeat(n_img, 0)[..., 2:4] * np.exp(tdel[..., 2:4]),
                                 anchors[None].repeat(n_img, 0)[..., 4:] + tdel[..., 4:]], -1).astype(np.float32)
    pred = deltas if (decoded or kind == "kfiou") else delta2bbox_rotated(
        torch.from_numpy(all_anc).to(dev), torch.from_numpy(deltas).to(dev)).cpu().numpy()
    avg = torch.tensor(float((weight.mean(-1) > 0).sum()) + 3.0, device=dev)
    lw = cfg.get("loss_weight", 1.0)
    p = torch.from_numpy(pred).to(dev).requires_grad_(True)
    out = loss.level(p, anc_t[None].expand(n_img, A, 5), _windows(dev, target), _windows(dev, weight), avg, coder,
                     decoded)
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith(GaussianLevel.__name__)
    out.backward()
    ref_kw = dict(kw)
    want, gwant = R.masked_loss_and_grad(kind, pred, target.reshape(-1, 5), weight.reshape(-1, 5), float(avg), lw,
                                         anchors=all_anc, decode_pred=decoded, **ref_kw)
    got, g = float(out.detach()), p.grad.cpu().numpy()
    lerr = abs(got - want) / max(abs(want), 1e-30)
    gerr = np.abs(g - gwant).max() / max(np.abs(gwant).max(), 1e-30)
    print("%s %s: loss %.6g vs %.6g rel %.2e, grad max err %.2e of max|g| %.3g" % (kind, kw, got, want, lerr, gerr,
                                                                                   np.abs(gwant).max()))
    assert np.all(np.isfinite(g))
    assert lerr <= ltol and gerr <= gtol
    assert np.all(g.reshape(n_img, A, 5)[weight.mean(-1) <= 0] == 0)         # the weight is a mask


def test_in_kernel_decode_is_bit_identical_and_empty_mask_is_zero(dev):
    """the loss with decode_pred / decode_target equals, bit for bit, the loss of the undecoded route fed
    jdet_delta2bbox_rotated's boxes (so the decode inside is that kernel's arithmetic); no positive row: exactly 0 and a
    zero gradient (the reference's early return, without its sync)"""
    from jdet_amd.models.boxes.box_ops import delta2bbox_rotated
    from jdet_amd.models.boxes.coder import DeltaXYWHABBoxCoder
    from jdet_amd.models.losses.gaussian_dist_loss import GaussianLevel, level_params
    rng = np.random.default_rng(6)
    anchors, deltas, tdel, weight = _level_inputs(rng, n_img=1, A=20000)
    a = torch.from_numpy(anchors).to(dev)
    d = torch.from_numpy(deltas).to(dev)
    t = torch.from_numpy(tdel.reshape(-1, 5)).to(dev)
    w = torch.from_numpy(weight.reshape(-1, 5)).to(dev)
    avg = torch.tensor(100.0, device=dev)
    coder = DeltaXYWHABBoxCoder()
    db, tb = delta2bbox_rotated(a, d), delta2bbox_rotated(a, t)
    for kind in ("gwd", "kld", "jd", "gwd_v1", "kld_v1", "bcd_v1"):
        fused = GaussianLevel.apply(d, t, w, a, level_params(kind, "log1p", coder, True, True, tau=1.0), avg, 1.0)
        plain = GaussianLevel.apply(db, tb, w, a, level_params(kind, "log1p", coder, False, False, tau=1.0), avg, 1.0)
        assert torch.equal(fused, plain), kind
    zero = torch.zeros_like(w)
    for kind in ("gwd", "kfiou"):
        x = d.clone().requires_grad_(True)
        out = GaussianLevel.apply(x, t, zero, a, level_params(kind, "none", coder, True, kind == "kfiou"), avg, 5.0)
        out.backward()
        assert float(out) == 0.0 and torch.count_nonzero(x.grad) == 0


def test_kfiou_nonpositive_det_rows_get_a_zero_gradient(dev):
    """the kernel's side of the decided rule: where fp32 rounding makes det(Sigma) <= 0 (Sigma = K Sigma_t) the KF-IoU
    term takes Vb = 0 with a ZERO gradient.  Rows: thin boxes (w / h 50..5e4) against a slightly rotated, rescaled copy
    -- about a fifth of them round det(Sigma) to <= 0 while det(Sigma_p), det(Sigma_t) stay positive.  Rows whose own
    det(Sigma_p) or det(Sigma_t) rounds negative give NaN as in the reference (its Vb_p / Vb_t are unguarded); they are
    found in a first pass and left out of the second."""
    from jdet_amd.models.boxes.coder import DeltaXYWHABBoxCoder
    from jdet_amd.models.losses.gaussian_dist_loss import GaussianLevel, level_params
    rng = np.random.default_rng(11)
    n = 512
    anchors = np.concatenate([rng.uniform(0, 1024, (n, 2)), np.exp(rng.uniform(np.log(50), np.log(500), (n, 1))),
                              np.exp(rng.uniform(np.log(1e-2), np.log(1.0), (n, 1))), rng.uniform(0.2, 1.4, (n, 1))],
                             1).astype(np.float32)
    tdel = np.zeros((n, 5), np.float32)
    tdel[:, 2], tdel[:, 3], tdel[:, 4] = math.log(1.01), math.log(0.99), 1e-3 / math.pi
    a, t = torch.from_numpy(anchors).to(dev), torch.from_numpy(tdel).to(dev)
    q = level_params("kfiou", "none", DeltaXYWHABBoxCoder(), True, True)
    avg = torch.tensor(1.0, device=dev)

    def run(weight):
        x = torch.zeros((n, 5), device=dev, requires_grad=True)
        out = GaussianLevel.apply(x, t, weight, a, q, avg, 1.0)
        out.backward()
        return out.detach(), x.grad
    _, g = run(torch.ones((n, 5), device=dev))
    own_nan = ~torch.isfinite(g).all(1)
    w = (~own_nan).float()[:, None].expand(n, 5).contiguous()
    loss, g = run(w)
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    kept = ~own_nan
    zero_rows = int(((g == 0).all(1) & kept).sum())
    print("det(Sigma) <= 0 rows with a zero gradient: %d of %d kept (%d own-NaN rows left out)"
          % (zero_rows, int(kept.sum()), int(own_nan.sum())))
    assert zero_rows > 0 and int(kept.sum()) - zero_rows > 0


@pytest.mark.parametrize("cfg", [dict(type="GDLoss", loss_type="gwd", loss_weight=5.0),
                                 dict(type="GDLoss_v1", loss_type="kld", fun="log1p", tau=1.0, loss_weight=5.5),
                                 dict(type="KFLoss", loss_weight=5.0)], ids=["gwd", "kld_v1", "kfiou"])
def test_level_node_equals_the_torch_composition(dev, cfg):
    """the node on the level's windows = the package's torch composition (torch decode, compaction, 2x2 algebra) on
    the same fp32 device tensors: forward, and the backward through jdet_loss_grad_scale"""
    from jdet_amd.models.boxes.coder import DeltaXYWHABBoxCoder
    loss = _build(cfg)
    kf = cfg["type"] == "KFLoss"
    rng = np.random.default_rng(7)
    anchors, deltas, tdel, weight = _level_inputs(rng, n_img=2, A=6000)
    coder = DeltaXYWHABBoxCoder()
    a = torch.from_numpy(anchors).to(dev)
    tw = _windows(dev, tdel)
    if not kf:
        tw = _windows(dev, coder.decode(a.repeat(2, 1), tw.reshape(-1, 5)).reshape(2, -1, 5).cpu().numpy())
    ww = _windows(dev, weight)
    avg = torch.tensor(321.0, device=dev)
    x1 = torch.from_numpy(deltas).to(dev).requires_grad_(True)
    node = loss.level(x1, a[None].expand(2, -1, 5), tw, ww, avg, coder, not kf)
    x2 = torch.from_numpy(deltas).to(dev).requires_grad_(True)
    comp = loss._composed(x2, a, tw.reshape(-1, 5), ww.reshape(-1, 5), avg, coder, not kf)
    assert type(node.grad_fn).__name__.startswith("GaussianLevel")
    (node * 0.7).backward()
    (comp * 0.7).backward()
    torch.testing.assert_close(node, comp, rtol=1e-4, atol=0)
    # fp32 against fp32 in another operation order: tight on the random rows; the hand-built rows (a w / h 62 times the
    # anchor's, where GWD's trace terms cancel) within 2 % of the gradient scale
    scale = float(x2.grad.abs().max())
    torch.testing.assert_close(x1.grad[6:], x2.grad[6:], rtol=0, atol=3e-4 * scale)
    torch.testing.assert_close(x1.grad[:6], x2.grad[:6], rtol=0, atol=2e-2 * scale)


def test_fake_overlaps_conversion_and_assignment(dev):
    """jdet_obb2hbb2obb = the torch fp32 tensor program on the device (bit for bit here: same operations, same order,
    the same device cosf / sinf); the assigner's gt_inds through it are identical"""
    from jdet_amd.models.boxes.assigner import MaxIoUAssigner
    from jdet_amd.models.boxes.iou_calculator import fake_rotated_boxes
    from jdet_amd.ops import box_iou_rotated
    from jdet_amd.ops.bbox_transforms import hbb2obb, obb2hbb
    from tests import inputs as I
    rng = np.random.default_rng(8)
    anchors = torch.from_numpy(I.random_obbs(rng, 196000, extent=1024.0, wh=(8.0, 512.0))).to(dev)
    got = fake_rotated_boxes(anchors)
    want = hbb2obb(obb2hbb(anchors))
    ulp = (got.view(torch.int32) - want.view(torch.int32)).abs().max()
    assert int(ulp) <= 1 and torch.equal(got[:, 4], want[:, 4]), int(ulp)
    print("obb2hbb2obb: max %d ulp from the torch program on the device" % int(ulp))
    gts = torch.from_numpy(I.random_obbs(rng, 64, extent=1024.0, wh=(16.0, 256.0))).to(dev)
    asg = MaxIoUAssigner(0.5, 0.4, min_pos_iou=0, ignore_iof_thr=-1,
                         iou_calculator=dict(type="FakeBboxOverlaps2D_rotated"))
    res = asg.assign(anchors, gts)
    ref = asg.assign_wrt_overlaps(box_iou_rotated(hbb2obb(obb2hbb(gts)), want))
    assert torch.equal(res.gt_inds, ref.gt_inds) and int((res.gt_inds > 0).sum()) > 0


def test_dense_decoded_targets_are_bit_identical_to_the_per_image_path(dev):
    from jdet_amd.config.named import GWD_RETINANET_CFG
    from jdet_amd.models.boxes.anchor_target import anchor_target
    from jdet_amd.models.roi_heads.s2anet_head import _cfg
    from tests import inputs as I
    cfg = _cfg(GWD_RETINANET_CFG["model"]["bbox_head"]["train_cfg"])
    rng = np.random.default_rng(9)
    A = 49104
    anchors = torch.from_numpy(I.random_obbs(rng, A, extent=1024.0, wh=(16.0, 512.0))).to(dev)
    anchors[:, 4] = 0.0
    gts = [torch.from_numpy(I.random_obbs(rng, 64, extent=1024.0, wh=(16.0, 256.0))).to(dev) for _ in range(2)]
    labels = [torch.from_numpy(rng.integers(1, 16, 64).astype(np.int32)).to(dev) for _ in range(2)]
    metas = [dict(img_shape=(1024, 1024), pad_shape=(1024, 1024), _all_valid=True) for _ in range(2)]
    split = [A // 2, A - A // 2]
    out = {}
    for dense in (True, False):
        al = [[anchors[:split[0]], anchors[split[0]:]] for _ in range(2)]
        vf = [[torch.ones(s, dtype=torch.bool, device=dev) for s in split] for _ in range(2)]
        out[dense] = anchor_target(al, vf, gts, metas, (0.,) * 5, (1.,) * 5, cfg, gt_labels_list=labels,
                                   label_channels=15, sampling=False, dense=dense)
    for a, b in zip(out[True][:4], out[False][:4]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert int(out[True][4]) == out[False][4] and int(out[True][4]) > 2


_DETECTORS = ["GWD_RETINANET_CFG", "KLD_RETINANET_CFG", "KFIOU_RETINANET_CFG"]


@pytest.mark.parametrize("name", _DETECTORS)
def test_detector_trains_syncfree_graph_equals_eager_and_infers(dev, name):
    """2 x 1024^2, 64 gts per image: finite losses falling over 10 Runner steps on a repeated batch; the step has no
    device -> host synchronisation; the HIP-graph step follows the eager one; inference returns polygons / scores /
    labels"""
    from jdet_amd.config import named
    from jdet_amd.runner import Runner, synthetic_batch
    from jdet_amd.utils.general import parse_losses
    cfg = getattr(named, name)
    images, targets = synthetic_batch(2, 1024, dev, seed=3, num_gts=64)
    hist = {}
    for mode in (False, True):
        torch.manual_seed(0)
        r = Runner(cfg, device=dev, conv_autotune=False, graph=mode)
        hist[mode] = [float(r.train_step(images, targets)[0]) for _ in range(10)]
        if not mode:
            m = r.model
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                total, parsed = parse_losses(m(images, targets))
                total.backward()
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert set(parsed) == {"loss_cls", "loss_bbox"} and torch.isfinite(total)
            m.zero_grad(set_to_none=True)
        else:
            assert len(r._graphs) == 1
            m = r.model
            m.eval()
            with torch.no_grad():
                m.bbox_head.retina_cls.bias.fill_(-2.0)
                res = m(images, targets)
            assert len(res) == 2
            polys, scores, labels = res[0]
            assert polys.shape[1] == 8 and polys.shape[0] == scores.shape[0] == labels.shape[0] > 0
    e, g = np.array(hist[False]), np.array(hist[True])
    print(name, "eager", np.round(e, 4).tolist(), "graph", np.round(g, 4).tolist())
    assert np.all(np.isfinite(e)) and e[-1] < e[0]
    np.testing.assert_allclose(g, e, rtol=2e-2)
