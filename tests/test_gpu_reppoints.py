"""GPU: Rotated RepPoints -- jdet_convex_point_assign against the sequential-loop restatement (tests/reppoints_ref.py),
jdet_convex_giou_loss against the general route (torch fp32 division, reppoints_convex_giou, the reference's rule in
torch) bit for bit, both buffer contracts (tests/guarded.py), the head's dense route against its general route, and the
detector built from REPPOINTS_CFG: training steps, no host sync on the dense route, inference.

The GIoU and its raw gradient are pinned against oracle/convex_giou_oracle.py by tests/test_gpu_convex_ops.py; nothing
of that is repeated here."""
import numpy as np
import pytest
import torch

from tests import reppoints_ref as R
from tests.abi_cases import REPPOINTS_CONTRACTS, giou_general_rows as _general_rows, giou_loss_rows as _loss_rows

pytestmark = pytest.mark.gpu


def _assign(dev, points, sizes, level_ids, gt, labels, counts, pos_num, labels_filled=-1, scale=R.SCALE):
    """(gt_inds (B, N), labels (B, N) | None) as numpy, through the Python wrapper of jdet_convex_point_assign"""
    from jdet_amd.models.boxes.assigner import convex_point_assign_device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)  # noqa: E731
    gi, lab = convex_point_assign_device(t(points, torch.float32), sizes, level_ids, t(gt, torch.float32),
                                         t(labels, torch.int32) if labels is not None else None,
                                         t(np.asarray(counts), torch.int32), scale, pos_num, labels_filled)
    torch.cuda.synchronize()
    return gi.cpu().numpy(), (lab.cpu().numpy() if lab is not None else None)


def _one(dev, points, sizes, level_ids, gts, pos_num, labels=None):
    """one image, K gts, no padding"""
    gts = np.asarray(gts, np.float32).reshape(1, -1, 8)
    lab = None if labels is None else np.asarray(labels, np.int32).reshape(1, -1)
    gi, gl = _assign(dev, points, sizes, level_ids, gts, lab, [gts.shape[1]], pos_num)
    return gi[0], (gl[0] if gl is not None else None)


# -------------------------------------------------------------------------------------------------------------- assigner
@pytest.mark.parametrize("pos_num", [1, 3])
@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_assigner_equals_the_sequential_loop(dev, name, pos_num):
    fx = R.fixture(name)
    gi, gl = _assign(dev, fx["points"], fx["sizes"], fx["level_ids"], fx["gt"], fx["labels"], fx["counts"], pos_num)
    gi0, gl0 = _assign(dev, fx["points"], fx["sizes"], fx["level_ids"], fx["gt"], None, fx["counts"], pos_num)
    assert gl0 is None and np.array_equal(gi, gi0)
    for b, k in enumerate(fx["counts"]):
        ref = R.assign_loop(fx["points"], fx["sizes"], fx["level_ids"], fx["gt"][b, :k], fx["labels"][b, :k],
                            pos_num=pos_num, labels_filled=-1)
        print("%s image %d pos_num %d: %d positives, %d rank ties, %d equal claims"
              % (name, b, pos_num, int((ref["gt_inds"] > 0).sum()), ref["rank_ties"], ref["equal_claims"]))
        assert np.array_equal(gi[b], ref["gt_inds"])
        assert np.array_equal(gl[b], ref["labels"])
        if k == 0:
            assert not gi[b].any() and (gl[b] == -1).all()


def test_assigner_gt_count_is_read_on_the_device_and_clamped(dev):
    fx = R.fixture("b2_256")
    full, _ = _assign(dev, fx["points"], fx["sizes"], fx["level_ids"], fx["gt"], fx["labels"], [8, 8], 1)
    part, lab = _assign(dev, fx["points"], fx["sizes"], fx["level_ids"], fx["gt"], fx["labels"], [5, -3], 1)
    over, _ = _assign(dev, fx["points"], fx["sizes"], fx["level_ids"], fx["gt"], fx["labels"], [99, 8], 1)
    ref = R.assign_loop(fx["points"], fx["sizes"], fx["level_ids"], fx["gt"][0, :5], fx["labels"][0, :5], labels_filled=-1)
    assert np.array_equal(part[0], ref["gt_inds"]) and np.array_equal(lab[0], ref["labels"])
    assert not part[1].any() and (lab[1] == -1).all()
    assert np.array_equal(over, full)


def test_assigner_ties_and_exact_levels(dev):
    points, sizes = R.grid(64, 64)
    ids = list(R.LEVEL_IDS)
    # two identical gts: the lower index wins everywhere
    g = np.stack([R.square(20.0, 20.0, 32.0)] * 2)
    gi, gl = _one(dev, points, sizes, ids, g, 3, labels=[3, 9])
    ref = R.assign_loop(points, sizes, ids, g, [3, 9], pos_num=3, labels_filled=-1)
    assert ref["equal_claims"] == 3 and np.array_equal(gi, ref["gt_inds"]) and np.array_equal(gl, ref["labels"])
    assert set(gi.tolist()) == {0, 1} and (gi == 1).sum() == 3
    # a gt centred exactly between two grid points: the lower point index
    g = R.square(12.0, 8.0, 32.0)[None]
    gi, _ = _one(dev, points, sizes, ids, g, 1)
    assert R.assign_loop(points, sizes, ids, g, pos_num=1)["rank_ties"] == 1
    assert np.flatnonzero(gi).tolist() == [1 * 8 + 1]
    # ... and between four (the centre of a cell): rank 1..3 in index order
    g = R.square(12.0, 12.0, 32.0)[None]
    gi, _ = _one(dev, points, sizes, ids, g, 3)
    assert np.flatnonzero(gi).tolist() == [1 * 8 + 1, 1 * 8 + 2, 2 * 8 + 1]
    # w / scale, h / scale in {8, 16, 32} exactly: the mathematically exact level, whatever log2f rounds to
    points, sizes = R.grid(256, 256)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for a in (3, 4, 5):
        for b in (3, 4, 5):
            g = R.rect(128.0, 128.0, R.SCALE * 2 ** a, R.SCALE * 2 ** b)[None]
            gi, _ = _one(dev, points, sizes, ids, g, 1)
            (p,) = np.flatnonzero(gi)
            lvl = int(np.searchsorted(offs, p, side="right")) - 1
            assert ids[lvl] == (a + b) // 2, (a, b, lvl)
            assert np.array_equal(gi, R.assign_loop(points, sizes, ids, g, pos_num=1)["gt_inds"])


def test_assigner_point_stride_and_level_gap(dev):
    fx = R.fixture("b2_256")
    wide = np.full((len(fx["points"]), 4), np.nan, np.float32)
    wide[:, :2] = fx["points"]
    gi, gl = _assign(dev, wide, fx["sizes"], fx["level_ids"], fx["gt"], fx["labels"], fx["counts"], 3)
    for b in range(2):
        ref = R.assign_loop(fx["points"], fx["sizes"], fx["level_ids"], fx["gt"][b], fx["labels"][b], pos_num=3,
                            labels_filled=-1)
        assert np.array_equal(gi[b], ref["gt_inds"]) and np.array_equal(gl[b], ref["labels"])
    # level ids with a gap: the level-5 gts claim nothing, the others as before
    keep = [0, 1, 3, 4]
    offs = np.concatenate([[0], np.cumsum(fx["sizes"])])
    pts = np.concatenate([fx["points"][offs[l]:offs[l + 1]] for l in keep])
    sizes, ids = [fx["sizes"][l] for l in keep], [fx["level_ids"][l] for l in keep]
    lv = R.levels_of(fx["gt"][0])
    assert (lv == 5).any() and (lv != 5).any()
    gi, _ = _assign(dev, pts, sizes, ids, fx["gt"][:1], None, [8], 1)
    ref = R.assign_loop(pts, sizes, ids, fx["gt"][0], pos_num=1)
    assert np.array_equal(gi[0], ref["gt_inds"])
    assert not np.isin(gi[0], np.flatnonzero(lv == 5) + 1).any() and (gi[0] > 0).sum() >= 1


def test_general_assigner_entry_reads_the_stride_column(dev):
    from jdet_amd.models.boxes.assigner import ConvexAssigner
    fx = R.fixture("hw_256x192")
    strides = np.repeat(np.asarray(R.STRIDES, np.float32), fx["sizes"])
    pts = torch.from_numpy(np.concatenate([fx["points"], strides[:, None], strides[:, None]], 1)).to(dev)
    a = ConvexAssigner(scale=4, pos_num=3, assigned_labels_filled=-1)
    res = a.assign(pts, torch.from_numpy(fx["gt"][0]).to(dev), None, torch.from_numpy(fx["labels"][0]).to(dev))
    ref = R.assign_loop(fx["points"], fx["sizes"], fx["level_ids"], fx["gt"][0], fx["labels"][0], pos_num=3,
                        labels_filled=-1)
    assert res.num_gts == 8 and res.max_overlaps is None
    assert np.array_equal(res.gt_inds.cpu().numpy(), ref["gt_inds"]) and np.array_equal(res.labels.cpu().numpy(), ref["labels"])
    empty = a.assign(pts, torch.zeros((0, 8), device=dev), None, torch.zeros((0,), dtype=torch.int32, device=dev))
    assert not empty.gt_inds.any() and (empty.labels == -1).all()


# ------------------------------------------------------------------------------------------------------------------ loss
def _bits(t):
    return t.contiguous().view(torch.int32)


def test_dense_loss_is_bit_equal_to_the_general_route(dev):
    from jdet_amd.models.losses.convex_giou_loss import convex_giou_loss_dense_rows
    pred, target, weight, norm, pos = [torch.from_numpy(a).to(dev) for a in _loss_rows()]
    loss, grad = convex_giou_loss_dense_rows(pred, target, weight, norm)
    ref_loss, ref_grad = _general_rows(pred[pos], target[pos], weight[pos], norm[pos])
    assert torch.isfinite(ref_loss).all() and torch.isfinite(ref_grad).all() and (ref_loss > 0).all()
    assert torch.equal(_bits(loss[pos]), _bits(ref_loss)) and torch.equal(_bits(grad[pos]), _bits(ref_grad))
    zero = torch.ones(300, dtype=torch.bool, device=dev)
    zero[pos] = False
    assert zero.sum() == 200 and (loss[zero] == 0).all() and (grad[zero] == 0).all()
    assert not torch.signbit(loss[zero]).any() and not torch.signbit(grad[zero]).any()
    print("dense loss: %d positive rows, loss in [%.4f, %.4f], max |grad| %.3e"
          % (len(pos), float(loss[pos].min()), float(loss[pos].max()), float(grad.abs().max())))


def _rule_rows():
    """hand-built rows, norm 1: nine points within 0.05 of each other against a unit-size target (inside it, across its
    edge, outside it), small targets under points of their own size (gradients of the order 1 / size), and large
    well-spread sets (gradients well below 1)"""
    rng = np.random.default_rng(9)
    unit = R.rect(0.0, 0.0, 1.0, 1.0)
    pred, target = [], []
    for cx, cy in ((0.1, 0.1), (0.5, 0.2), (1.5, 0.3)):
        pred.append((np.asarray([cx, cy]) + rng.uniform(-0.025, 0.025, (9, 2))).reshape(18))
        target.append(unit)
    for size in (0.05, 0.1, 0.2):
        pred.append((rng.uniform(-0.5, 0.5, (9, 2)) * size + 0.3 * size).reshape(18))
        target.append(R.rect(0.0, 0.0, size, size))
    for size in (20.0, 40.0, 80.0):
        pred.append((rng.uniform(-0.5, 0.5, (9, 2)) * size + 0.2 * size).reshape(18))
        target.append(R.rect(0.0, 0.0, size, size))
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    assert np.ptp(pred[:3].reshape(3, 9, 2), axis=1).max() <= 0.05
    return pred, target


def test_dense_loss_invalid_gradient_rule(dev):
    from jdet_amd.models.losses.convex_giou_loss import convex_giou_loss_dense_rows
    from jdet_amd.ops.reppoints_convex_iou import reppoints_convex_giou
    pred, target = [torch.from_numpy(a).to(dev) for a in _rule_rows()]
    n = pred.shape[0]
    one = torch.ones(n, device=dev)
    _, raw = reppoints_convex_giou(pred, target)
    fired = (raw > 1).any(dim=1)
    print("raw gradient maxima per row", [round(float(v), 4) for v in raw.max(dim=1).values], "rule fires on",
          fired.nonzero().flatten().tolist())
    assert fired.any() and not fired.all()                   # a condition on the input: the rule decides something
    ref_loss, ref_grad = _general_rows(pred, target, one, one)
    assert (ref_grad[fired] == -1e-6).all() and not (ref_grad[~fired] == -1e-6).all(dim=1).any()
    loss, grad = convex_giou_loss_dense_rows(pred, target, one, one)
    assert torch.equal(_bits(loss), _bits(ref_loss)) and torch.equal(_bits(grad), _bits(ref_grad))
    # the weight enters before the rule: a weight of 1/64 takes every row of this set below it
    w = torch.full((n,), 1.0 / 64, device=dev)
    ref_loss, ref_grad = _general_rows(pred, target, w, one)
    loss, grad = convex_giou_loss_dense_rows(pred, target, w, one)
    assert torch.equal(_bits(loss), _bits(ref_loss)) and torch.equal(_bits(grad), _bits(ref_grad))


def test_dense_loss_empty_and_module_entries(dev):
    from jdet_amd import _lib as L
    from jdet_amd.models.losses.convex_giou_loss import ConvexGIoULoss, convex_giou_loss_dense_rows
    e = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    loss, grad = convex_giou_loss_dense_rows(e(0, 18), e(0, 8), e(0), e(0))
    assert loss.shape == (0,) and grad.shape == (0, 18)
    assert L.lib().jdet_convex_giou_loss(None, None, None, None, 0, None, None, None) == 0
    # the module: dense over all rows equals the general route over the gathered positives, value and gradient
    pred, target, weight, norm, pos = [torch.from_numpy(a).to(dev) for a in _loss_rows(seed=6, P=64, n_pos=20)]
    m = ConvexGIoULoss(loss_weight=0.375)
    pd = pred.clone().requires_grad_()
    ld = m.dense(pd, target, weight, norm)
    ld.backward()
    pg = pred[pos].clone().requires_grad_()
    lg = m(pg / norm[pos][:, None], target[pos] / norm[pos][:, None], weight[pos])
    lg.backward()
    # the same 20 non-negative terms summed over two trees of depth <= 7: 7 * 2^-24 relative
    assert abs(float(ld) - float(lg)) <= 1e-5 * float(lg) and float(lg) > 0
    assert torch.allclose(pd.grad[pos], pg.grad, rtol=1e-5, atol=1e-30)
    zero = torch.ones(64, dtype=torch.bool, device=dev)
    zero[pos] = False
    assert (pd.grad[zero] == 0).all()
    # no positive weight: the general route returns early with an exact 0 that still reaches pred
    pz = pred[pos].clone().requires_grad_()
    lz = m(pz, target[pos], torch.zeros(20, device=dev))
    lz.backward()
    assert float(lz) == 0 and (pz.grad == 0).all()
    assert float(m.dense(pred, target, torch.zeros(64, device=dev), norm)) == 0


# ----------------------------------------------------------------------------------------------------- buffer contracts
@pytest.mark.parametrize("case", ["assign b2_256", "assign k70_k0", "loss"])
def test_buffer_contract(dev, case):
    """guard bands, canaries, a 0xFF workspace, one byte short refused, B == A bit for bit with poisoned outputs, NaN
    in the gt rows beyond the count and in the unused point columns (tests/guarded.py)"""
    from tests import guarded
    c = REPPOINTS_CONTRACTS[case]()
    guarded.run_case(c.entry_points[0], c.label, c.fn, dev)


# ------------------------------------------------------------------------------------------------------------------ head
def _small_head(dev):
    from jdet_amd.config.named import REPPOINTS_CFG
    from jdet_amd.models.roi_heads.rotated_reppoints_head import RotatedRepPointsHead
    cfg = dict(REPPOINTS_CFG["model"]["bbox_head"])
    cfg.pop("type")
    cfg.update(in_channels=16, feat_channels=32, point_feat_channels=32, stacked_convs=1)
    torch.manual_seed(0)
    h = RotatedRepPointsHead(**cfg).to(dev)
    # point offsets of the order of a cell or two, so that hulls have an area and some IoUs are positive
    torch.nn.init.normal_(h.reppoints_pts_init_out.weight, std=0.3)
    torch.nn.init.normal_(h.reppoints_pts_refine_out.weight, std=0.3)
    return h.train()


def test_offset_to_pts_and_points2rotrect_by_hand(dev):
    h = _small_head(dev)
    # one 2 x 2 map at stride 8: the prediction of cell (row 1, column 0) is (dy_k, dx_k) = (k, -k) / 8, k = 0..8
    pred = torch.zeros((1, 18, 2, 2), device=dev)
    for k in range(9):
        pred[0, 2 * k, 1, 0] = k / 8.0
        pred[0, 2 * k + 1, 1, 0] = -k / 8.0
    grid = h.prior_generator.grid_priors([(2, 2)] + [(1, 1)] * 4, device=dev, with_stride=True)
    assert grid[0].tolist() == [[0.0, 0.0, 8.0, 8.0], [8.0, 0.0, 8.0, 8.0], [0.0, 8.0, 8.0, 8.0], [8.0, 8.0, 8.0, 8.0]]
    pts = h.offset_to_pts([grid], [pred] + [torch.zeros((1, 18, 1, 1), device=dev)] * 4)
    assert pts[0].shape == (1, 4, 18) and pts[1].shape == (1, 1, 18)
    # xy order, times the stride, plus the cell's point (0, 8)
    assert pts[0][0, 2].tolist() == [v for k in range(9) for v in (0.0 - k, 8.0 + k)]
    assert pts[0][0, 0].tolist() == [0.0, 0.0] * 9 and pts[0][0, 3].tolist() == [8.0, 8.0] * 9
    # points2rotrect: y-first points on the border of the axis-aligned rectangle x in [1, 5], y in [2, 4]
    yx = torch.tensor([[2, 1, 2, 5, 4, 5, 4, 1, 3, 3, 2, 3, 4, 3, 3, 1, 3, 5]], dtype=torch.float32, device=dev)
    rect = h.points2rotrect(yx, y_first=True)
    assert rect.shape == (1, 8)
    corners = sorted(tuple(round(float(v), 4) for v in rect[0, 2 * i:2 * i + 2]) for i in range(4))
    assert corners == [(1.0, 2.0), (1.0, 4.0), (5.0, 2.0), (5.0, 4.0)]
    xy = yx.view(1, 9, 2).flip(-1).reshape(1, 18)
    assert torch.equal(h.points2rotrect(xy, y_first=False), rect)


def test_head_dense_route_equals_general_route(dev):
    from jdet_amd.runner import synthetic_batch
    from jdet_amd.utils.general import multi_apply
    h = _small_head(dev)
    _, targets = synthetic_batch(2, 256, dev, seed=3, num_gts=8)
    torch.manual_seed(1)
    feats = [torch.randn((2, 16, s, s), device=dev) for s in (32, 16, 8, 4, 2)]
    with torch.no_grad():
        outs = multi_apply(h.forward_single, feats)
    sizes = [(s, s) for s in (32, 16, 8, 4, 2)]
    parsed = h.parse_targets(targets)

    def stage_targets(dense):
        h.dense = dense
        metas = [dict(m) for m in parsed["img_metas"]]
        centers, flags = h.get_points(sizes, metas, dev)
        init = h.get_targets(centers, flags, parsed["gt_bboxes"], metas, gt_bboxes_ignore_list=parsed["gt_bboxes_ignore"],
                             gt_labels_list=parsed["gt_labels"], stage="init")
        centers, flags = h.get_points(sizes, metas, dev)
        refine = h.get_targets(h._refine_proposals(centers, outs[1]), flags, parsed["gt_bboxes"], metas,
                               gt_bboxes_ignore_list=parsed["gt_bboxes_ignore"], gt_labels_list=parsed["gt_labels"],
                               stage="refine")
        return init, refine

    dense, general = stage_targets(True), stage_targets(False)
    for stage, d, g in zip(("init", "refine"), dense, general):
        assert torch.is_tensor(d[5]) and d[5].is_cuda and isinstance(g[5], int)      # the dense count stays on the device
        assert int(d[5]) == g[5] and int(d[6]) == g[6], stage
        for what, i in (("labels", 0), ("label_weights", 1), ("bbox_gt", 2), ("pos_proposals", 3), ("proposal_weights", 4)):
            for lvl, (a, b) in enumerate(zip(d[i], g[i])):
                assert a.shape == b.shape and a.dtype == b.dtype, (stage, what, lvl)
                assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b), \
                    (stage, what, lvl)
        npos = int(sum((w > 0).sum() for w in d[4]))
        print("%s stage: %d positives, counted %d, negatives %d" % (stage, npos, int(d[5]), int(d[6])))
        assert npos >= 8 if stage == "init" else npos >= 1
    assert sum((w > 0).sum() for w in dense[0][4]) == 16                          # pos_num 1, 8 gts, 2 images
    # the positives of the refine stage are not one blob from all-zero overlaps: more than one gt owns some
    assert len(torch.unique(torch.cat([t.reshape(-1, 8) for t in dense[1][2]]), dim=0)) > 2

    def losses(dense):
        h.dense = dense
        leaves = [[t.detach().clone().requires_grad_() for t in o] for o in outs]
        out = h.loss(*leaves, **{k: ([dict(m) for m in v] if k == "img_metas" else v) for k, v in parsed.items()})
        total = sum(sum(v) for v in out.values())
        total.backward()
        return out, leaves

    (ld, vd), (lg, vg) = losses(True), losses(False)
    h.dense = True
    for k in ("loss_cls", "loss_pts_init", "loss_pts_refine"):
        for lvl, (a, b) in enumerate(zip(ld[k], lg[k])):
            print("%s level %d dense %.7f general %.7f" % (k, lvl, float(a), float(b)))
            assert torch.isfinite(a) and abs(float(a) - float(b)) <= 1e-5 * abs(float(b)), (k, lvl)
    assert sum(float(v) for v in ld["loss_pts_init"]) > 0 and sum(float(v) for v in ld["loss_pts_refine"]) > 0
    for what, i in (("pts_out_init", 1), ("pts_out_refine", 2)):
        for lvl, (a, b) in enumerate(zip(vd[i], vg[i])):
            assert torch.isfinite(a.grad).all()
            assert torch.allclose(a.grad, b.grad, rtol=1e-5, atol=1e-30), (what, lvl, float((a.grad - b.grad).abs().max()))
        assert sum(float(t.grad.abs().sum()) for t in vd[i]) > 0, what


# -------------------------------------------------------------------------------------------------------------- detector
def test_detector_trains_syncfree_and_infers(dev):
    """REPPOINTS_CFG, 2 x 256^2, 8 gts per image: six Runner steps on a repeated batch with finite losses and a falling
    loss_cls (the point losses are printed, not asserted: at random init the nine points nearly coincide and the 1e-6
    rule governs their gradient); every head parameter gets a gradient; forward + backward of the dense route without
    a device -> host synchronisation; inference returns polygons / scores / labels"""
    from jdet_amd.config.named import REPPOINTS_CFG
    from jdet_amd.runner import Runner, synthetic_batch
    from jdet_amd.utils.general import parse_losses
    images, targets = synthetic_batch(2, 256, dev, seed=3, num_gts=8)
    torch.manual_seed(0)
    r = Runner(REPPOINTS_CFG, device=dev, conv_autotune=False, graph=False)
    hist = {"loss_cls": [], "loss_pts_init": [], "loss_pts_refine": []}
    for step in range(6):
        _, losses = r.train_step(images, targets)
        assert set(losses) == set(hist)
        for k in hist:
            hist[k].append(float(losses[k]))
        if step == 0:
            for n, p in r.model.bbox_head.named_parameters():
                assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, n
    for k, v in hist.items():
        print("REPPOINTS_CFG", k, np.round(v, 5).tolist())
        assert np.all(np.isfinite(v)), k
    assert hist["loss_cls"][-1] < hist["loss_cls"][0]
    m = r.model
    m.train()
    assert m.bbox_head.dense
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, parsed = parse_losses(m(images, targets))
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert set(parsed) == set(hist) and torch.isfinite(total)
    m.zero_grad(set_to_none=True)
    m.eval()
    with torch.no_grad():
        m.bbox_head.reppoints_cls_out.bias.fill_(-2.0)
        res = m(images, targets)
    assert len(res) == 2
    for polys, scores, labels in res:
        assert polys.dim() == 2 and polys.shape[1] == 8 and polys.shape[0] == scores.shape[0] == labels.shape[0]
        assert polys.shape[0] > 0 and torch.isfinite(polys).all()
        assert polys.shape[0] <= REPPOINTS_CFG["model"]["bbox_head"]["test_cfg"]["max_per_img"]
