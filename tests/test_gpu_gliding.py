"""GPU: the fused Gliding Vertex codecs (csrc/box_codec_gliding.hip) against the numpy restatement
(tests/gliding_ref.py), the RPN's proposal table, the head's targets at config size, and the detector's train step and
inference.

Tolerances of the kernel comparisons are not fixed numbers: the restatement runs once in float32 and once in float64
on the same (float32-representable) inputs, and the kernel may be off the float64 values by 4x the largest
float32-vs-float64 difference of that output, with an absolute floor of 1e-6.  The factor covers expf / logf and
division rounding differences between the device and numpy; the float32 shoelace sum over absolute coordinates is what
makes the ratio's spread large (profiles/gliding_codecs.md has the figures of one run)."""
import numpy as np
import pytest
import torch

from tests import gliding_ref as R

pytestmark = pytest.mark.gpu

MEANS, STDS = R.MEANS, R.STDS
F32 = np.float32


def _bound(f32, f64):
    return max(4.0 * float(np.abs(f32.astype(np.float64) - f64).max()), 1e-6)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dev)


@pytest.fixture(scope="module")
def rows():
    """4000 (roi, polygon) rows -- rotated rectangles and general convex quadrilaterals, centres in [50, 950], sides
    8-300 -- with the restatement's targets in float64 and in float32, computed once"""
    rois, polys = R.target_case()
    f64 = R.targets(rois, polys, MEANS, STDS)
    f32 = R.targets(rois.astype(F32), polys.astype(F32), np.asarray(MEANS, F32), np.asarray(STDS, F32))
    return rois, polys, f64, f32


def test_target_kernel_matches_the_restatement(dev, rows):
    from jdet_amd.models.boxes.coder import gliding_targets
    rois, polys, f64, f32 = rows
    for p in (polys, polys.astype(F32)):           # no row on h_mask or on a vertex tie, in either precision
        assert not R.fix_encode(p, with_flags=True)[1].any() and not R.has_vertex_tie(p).any()
    assert all(a.dtype == F32 for a in f32)
    got = gliding_targets(_dev(rois, dev), _dev(polys, dev), MEANS, STDS)
    for name, g, a32, a64 in zip(("bbox", "fix", "ratio"), got, f32, f64):
        g = g.cpu().numpy().astype(np.float64)
        assert g.shape == a64.shape
        err, bound = float(np.abs(g - a64).max()), _bound(a32, a64)
        print("gliding_targets %-5s float32-vs-float64 spread %.3e  bound %.3e  kernel max error %.3e"
              % (name, bound / 4, bound, err))
        assert np.isfinite(g).all() and err <= bound, (name, err, bound)


def test_delta_codec_kernels_match_the_restatement(dev, rows):
    """the RPN's pair: encode against horizontal gts, decode with and without the border clamp"""
    from jdet_amd.models.boxes.coder import GVDeltaXYWHBBoxCoder
    rois, polys, f64, f32 = rows
    coder = GVDeltaXYWHBBoxCoder(MEANS, STDS)
    gts = R.poly_hbb(polys)
    enc = coder.encode(_dev(rois, dev), _dev(gts, dev)).cpu().numpy().astype(np.float64)
    assert np.abs(enc - f64[0]).max() <= _bound(f32[0], f64[0])
    rng = np.random.default_rng(1)
    deltas = rng.normal(0, 1.0, (rois.shape[0], 4)).astype(F32).astype(np.float64)
    deltas[:5, 2] = 40.0                           # on the wh_ratio_clip clamp
    for max_shape in (None, (1000, 900)):
        a64 = R.delta_decode(rois, deltas, MEANS, STDS, max_shape)[:, 0]
        a32 = R.delta_decode(rois.astype(F32), deltas.astype(F32), MEANS, STDS, max_shape)[:, 0]
        got = coder.decode(_dev(rois, dev), _dev(deltas, dev), max_shape=max_shape).cpu().numpy().astype(np.float64)
        assert np.abs(got - a64).max() <= _bound(a32, a64), max_shape
        if max_shape is not None:
            assert got[:, [0, 2]].max() == 900 and got[:, [1, 3]].max() == 1000 and got.min() == 0


def test_float64_device_inputs_take_the_float64_composition(dev, rows):
    """the kernels are fp32: float64 tensors on the device are not cast down, they get the composition in float64"""
    from jdet_amd.models.boxes import coder as Cd
    rois, polys, f64, _ = rows
    r, p = (torch.from_numpy(a[:256]).to(dev) for a in (rois, polys))
    got = Cd.gliding_targets(r, p, MEANS, STDS)
    singles = (Cd.GVDeltaXYWHBBoxCoder(MEANS, STDS).encode(r, torch.from_numpy(R.poly_hbb(polys[:256])).to(dev)),
               Cd.GVFixCoder().encode(p), Cd.GVRatioCoder().encode(p))
    for g, s, want in zip(got, singles, f64):
        assert g.dtype == torch.float64 and s.dtype == torch.float64
        np.testing.assert_allclose(g.cpu().numpy(), want[:256], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(s.cpu().numpy(), want[:256], rtol=1e-12, atol=1e-12)
    args = R.decode_case(n=32, C=3)
    want = R.decode_polys(*args, MEANS, STDS, (1024, 1024))
    out = Cd.gliding_decode(*(torch.from_numpy(a).to(dev) for a in args), MEANS, STDS, max_shape=(1024, 1024))
    assert out.dtype == torch.float64
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-12, atol=1e-12)


def _tied_polys():
    """axis-aligned rectangles in their four vertex orders and quadrilaterals with exactly tied extreme vertices (two
    vertices on the top edge / on the right edge / ...), every cyclic order, integer and fractional coordinates"""
    base = [
        [10, 0, 20, 0, 25, 10, 5, 12],        # top tie, not masked: the LOWEST index decides dt
        [0, 5, 10, 0, 30, 8, 30, 20],         # right tie
        [3, 0, 30, 7, 20, 20, 10, 20],        # bottom tie
        [0, 6, 0, 14, 9, 30, 25, 2],          # left tie
        [10, 0, 20, 0, 30, 10, 0, 10],        # trapezoid: right vertex and bottom vertex share an x -> h_mask
        [5, 8, 30, 0, 25, 20, 0, 15],         # one vertex is the top-most AND the right-most one -> h_mask, no tie
        [0, 0, 16, 0, 16, 9, 0, 9],           # rectangle TL, TR, BR, BL
        [0, 0, 7, 0, 7, 7, 0, 7],
    ]
    out = []
    for q in base:
        pts = np.asarray(q, np.float64).reshape(4, 2)
        for shift in range(4):
            for scale, off in ((1.0, (100.0, 200.0)), (2.5, (33.25, 71.5)), (0.375, (640.0, 12.125))):
                for order in (1, -1):
                    p = np.roll(pts, -shift, axis=0)[::order] * scale + np.asarray(off)
                    out.append(p.reshape(8))
    return np.asarray(out)


def test_tied_and_axis_aligned_inputs_equal_the_composition_bit_for_bit(dev):
    """the lowest-index rule and h_mask: on exactly tied inputs the fused launch and the torch composition (float32, on
    the device) agree in every bit"""
    from jdet_amd.models.boxes.coder import gliding_targets
    polys = _tied_polys()
    assert np.array_equal(polys.astype(F32).astype(np.float64), polys)
    flat = R.fix_encode(polys, with_flags=True)[1]
    assert (R.has_vertex_tie(polys) | flat).all() and flat.any() and not flat.all()
    b = R.poly_hbb(polys)
    rois = b + np.asarray([-1.5, -2.0, 3.25, 0.75])[None]           # wider than the gt on every side: finite deltas
    r, p = _dev(rois, dev), _dev(polys, dev)
    fused = gliding_targets(r, p, MEANS, STDS, fused=True)
    comp = gliding_targets(r, p, MEANS, STDS, fused=False)
    for name, a, c in zip(("bbox", "fix", "ratio"), fused, comp):
        assert bool(torch.isfinite(a).all())
        same = torch.equal(a, c)
        print("tied inputs %-5s bit-for-bit %s  max diff %.3e" % (name, same, float((a - c).abs().max())))
        assert same, name
    want = R.fix_encode(polys)
    np.testing.assert_allclose(fused[1].cpu().numpy(), want, rtol=0, atol=1e-6)
    assert bool((fused[1][torch.from_numpy(flat).to(dev)] == 1).all())


@pytest.mark.parametrize("max_shape", [None, (1024, 1024)])
def test_decode_kernel_matches_the_restatement_and_the_composed_coders(dev, max_shape):
    from jdet_amd.models.boxes.coder import GVDeltaXYWHBBoxCoder, GVFixCoder, gliding_decode
    from jdet_amd.ops.bbox_transforms import hbb2poly
    rois, bbox, fix, ratio = R.decode_case()
    n, C = ratio.shape
    scale = (1.25, 0.8, 1.25, 0.8)
    a64 = R.decode_polys(rois, bbox, fix, ratio, MEANS, STDS, max_shape, ratio_thr=0.8, scale=scale)
    a32 = R.decode_polys(*(a.astype(F32) for a in (rois, bbox, fix, ratio)), MEANS, STDS, max_shape, ratio_thr=0.8,
                         scale=scale)
    assert a32.dtype == F32 and (ratio > 0.8).sum() > 100 and (ratio <= 0.8).sum() > 100
    bound = _bound(a32, a64)
    t = [_dev(a, dev) for a in (rois, bbox, fix, ratio)]
    got = gliding_decode(*t, MEANS, STDS, max_shape=max_shape, ratio_thr=0.8, scale=scale)
    assert tuple(got.shape) == (n, 8 * C)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - a64).max())
    print("gliding_decode max_shape=%s spread %.3e bound %.3e kernel max error %.3e" % (max_shape, bound / 4, bound, err))
    assert err <= bound
    # the composed coders (each its own launch) + the ratio switch + the rescale, as the reference chains them
    boxes = GVDeltaXYWHBBoxCoder(MEANS, STDS).decode(t[0], t[1], max_shape=max_shape)
    polys = GVFixCoder().decode(boxes, t[2]).view(n, C, 8)
    polys = torch.where((t[3] > 0.8)[..., None], hbb2poly(boxes.view(n, C, 4)), polys)
    polys = (polys / torch.tensor(scale + scale, device=dev)).view(n, -1)
    # same device function for the box, the same mul / add / divide afterwards (no contraction on either side): equal to
    # the fused launch up to 2 float32 ulp per element, far inside the spread bound that the float64 comparison gets
    diff = (polys - got).abs().cpu().numpy()
    ulp = np.spacing(np.abs(got.cpu().numpy()).astype(F32))
    print("composed coders vs fused launch: %d of %d elements differ, max %.2f ulp"
          % (int((diff > 0).sum()), diff.size, float((diff / ulp).max())))
    assert np.all(diff <= 2 * ulp)
    comp = gliding_decode(*t, MEANS, STDS, max_shape=max_shape, ratio_thr=0.8, scale=scale, fused=False)
    assert float((comp - got).abs().max()) <= bound
    if max_shape is not None:
        g = got.view(n, C, 8)
        assert float(g[3, :, 0::2].max()) == float(F32(1024) / F32(1.25)) and float(g[4, :, 0::2].min()) == 0.0


@pytest.mark.parametrize("nms_post", [100, 1000])
def test_rpn_proposal_table_contract(dev, nms_post):
    """exactly `nms_post` rows [x1, y1, x2, y2, score], descending score, padding rows -1; the survivors are those of a
    numpy greedy NMS over the candidates of ALL levels sorted by score (one label-free pass, not one per level)"""
    from jdet_amd.models.roi_heads import GlidingRPNHead
    from jdet_amd.models.utils.level_pack import run_levels
    torch.manual_seed(3)
    strides = (4, 8, 16, 32, 64)
    rpn = GlidingRPNHead(in_channels=16, feat_channels=16, nms_pre=300, nms_post=nms_post,
                         anchor_generator=dict(type="AnchorGenerator", scales=[8], ratios=[0.5, 1.0, 2.0],
                                               strides=list(strides))).to(dev).eval()
    feats = [torch.randn(2, 16, 128 // s, 128 // s, device=dev) for s in strides]
    targets = [dict(img_size=(128, 128), pad_shape=(128, 128))] * 2
    with torch.no_grad():
        tables, losses = rpn(feats, targets)
        outs = run_levels(list(feats), rpn.forward_single)
    assert losses == {} and len(tables) == 2
    anchors = rpn.anchor_generator.grid_anchors([tuple(f.shape[-2:]) for f in feats], device=dev)
    for img, tab in enumerate(tables):
        assert tuple(tab.shape) == (nms_post, 5)
        # the candidates, restated: per level the 300 best by softmax(...)[:, 1], decoded and clamped to the image
        scores, boxes = [], []
        for (cls, reg), a in zip(outs, anchors):
            s = cls[img].permute(1, 2, 0).reshape(-1, 2).softmax(dim=1)[:, 1]
            d = reg[img].permute(1, 2, 0).reshape(-1, 4)
            if s.shape[0] > 300:
                s, top = torch.topk(s, 300)
                d, a = d[top], a[top]
            scores.append(s)
            boxes.append(rpn.bbox_coder.decode(a, d, max_shape=(128, 128)))
        scores, boxes = torch.cat(scores).cpu().numpy(), torch.cat(boxes).cpu().numpy()
        assert len(scores) == 300 + 300 + 8 * 8 * 3 + 4 * 4 * 3 + 2 * 2 * 3
        big = (boxes[:, 2] - boxes[:, 0] > 0) & (boxes[:, 3] - boxes[:, 1] > 0)
        idx = np.nonzero(big)[0]
        keep = idx[R.greedy_nms(boxes[idx], scores[idx], 0.7)][:nms_post]
        n = len(keep)
        got = tab.cpu().numpy()
        assert 0 < n and (n == nms_post or nms_post == 1000)
        np.testing.assert_array_equal(got[:n, 4], scores[keep])
        np.testing.assert_array_equal(got[:n, :4], boxes[keep])
        assert np.all(got[n:, 4] == -1.0) and np.all(np.diff(got[:n, 4]) <= 0)
        if nms_post == 1000:
            assert n < nms_post                                    # 852 candidates: there are padding rows
            levels = np.searchsorted(np.cumsum([300, 300, 192, 48, 12]), keep, side="right")
            assert len(set(levels.tolist())) >= 2                  # and the pass really spans levels


# ------------------------------------------------------------------------------------------ head and detector
@pytest.fixture(scope="module")
def runner(dev):
    from jdet_amd.config.named import GLIDING_CFG
    from jdet_amd.runner import Runner
    torch.manual_seed(0)
    return Runner(GLIDING_CFG, device=dev, conv_autotune=False)


@pytest.fixture(scope="module")
def batch(dev):
    from jdet_amd.runner import synthetic_batch
    return synthetic_batch(2, 1024, dev, seed=3, num_gts=64)


def _tables(targets, dev, rows=2000, alive=1500):
    """a proposal table per image: jittered copies of the gts (positives), random boxes, then padding rows"""
    g = torch.Generator(device="cpu").manual_seed(11)
    out = []
    for t in targets:
        gt = t["hboxes"].cpu()
        k = gt.shape[0]
        rep = gt[torch.randint(0, k, (alive // 2,), generator=g)]
        wh = (rep[:, 2:] - rep[:, :2])
        near = rep + torch.cat([wh, wh], 1) * (torch.rand((alive // 2, 4), generator=g) - 0.5) * 0.25
        c = torch.rand((alive - alive // 2, 2), generator=g) * 1024
        s = torch.rand((alive - alive // 2, 2), generator=g) * 150 + 8
        far = torch.cat([c - s / 2, c + s / 2], 1)
        boxes = torch.cat([near, far])
        score = torch.sort(torch.rand((alive,), generator=g), descending=True).values
        tab = torch.cat([boxes, score[:, None]], 1)
        pad = torch.zeros((rows - alive, 5))
        pad[:, 4] = -1.0
        out.append(torch.cat([tab, pad]).to(dev))
    return out


def test_head_targets_at_config_size_match_the_restatement(dev, runner, batch):
    """2 images, 64 gts, 512 rows each: one fused launch for all 1024 rows = the restatement on the same sampled rows"""
    from jdet_amd.ops.bbox_transforms import obb2poly
    head = runner.model.bbox_head
    _, targets = batch
    torch.manual_seed(5)
    per_image = [head.sample(tab, tg) for tab, tg in zip(_tables(targets, dev), targets)]
    labels, label_w, bbox_t, fix_t, ratio_t, pos, valid = head.targets(per_image)
    assert labels.shape == (1024,) and bbox_t.shape == (1024, 4) and ratio_t.shape == (1024, 1)
    assert int(pos.sum()) > 100 and bool(valid.all())
    n64 = lambda t: t.cpu().numpy().astype(np.float64)     # noqa: E731
    boxes = np.concatenate([n64(r.boxes) for r, _ in per_image])
    polys = np.concatenate([n64(obb2poly(tg["rboxes"])[r.matched]) for (r, _), tg in zip(per_image, targets)])
    gt_lab = np.concatenate([(tg["labels"].long() - 1)[r.matched].cpu().numpy() for (r, _), tg in zip(per_image, targets)])
    is_pos, ok = pos.cpu().numpy(), valid.cpu().numpy()
    c = head.bbox_coder
    w64 = R.head_targets(boxes, polys, gt_lab, is_pos, ok, c.means, c.stds, 15)
    w32 = R.head_targets(boxes.astype(F32), polys.astype(F32), gt_lab, is_pos, ok, c.means, c.stds, 15)
    assert np.array_equal(labels.cpu().numpy(), w64[0]) and np.array_equal(n64(label_w), w64[1])
    assert set(np.unique(w64[0][~is_pos])) == {15} and w64[0][is_pos].max() < 15
    for name, g, a32, a64 in zip(("bbox", "fix", "ratio"), (bbox_t, fix_t, ratio_t), w32[2:5], w64[2:5]):
        err, bound = float(np.abs(n64(g) - a64).max()), _bound(np.asarray(a32, F32), a64)
        print("head targets %-5s bound %.3e kernel max error %.3e" % (name, bound, err))
        assert err <= bound, (name, err, bound)
        assert np.all(n64(g)[~is_pos] == 0)


def test_polys_key_and_rboxes_give_identical_targets(dev, runner, batch):
    from jdet_amd.ops.bbox_transforms import obb2poly
    head = runner.model.bbox_head
    _, targets = batch
    tables = _tables(targets, dev)
    with_polys = [dict(t, polys=obb2poly(t["rboxes"])) for t in targets]
    assert "polys" not in targets[0]
    outs = []
    for tgs in (targets, with_polys):
        torch.manual_seed(7)
        outs.append(head.targets([head.sample(tab, tg) for tab, tg in zip(tables, tgs)]))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_train_step_at_config_size(dev, runner, batch):
    """2 x 1024^2, 64 gts: six finite loss keys, a finite gradient on every trainable parameter, non-zero regression
    losses, no host synchronisation, and two optimizer steps that leave nothing NaN"""
    from jdet_amd.utils.general import parse_losses
    images, targets = batch
    images = images.contiguous(memory_format=torch.channels_last)
    m = runner.model
    m.train()
    losses = m(images, targets)                       # also the warm-up: anchor caches, workspaces
    assert set(losses) == {"gliding_cls_loss", "gliding_bbox_loss", "gliding_fix_loss", "gliding_ratio_loss",
                           "loss_rpn_cls", "loss_rpn_bbox"}
    assert len(losses["loss_rpn_cls"]) == 5 and len(losses["loss_rpn_bbox"]) == 5
    total, parsed = parse_losses(losses)
    total.backward()
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, parsed = parse_losses(m(images, targets))
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(v).all()) for v in parsed.values()) and bool(torch.isfinite(total))
    for k in ("gliding_bbox_loss", "gliding_fix_loss", "gliding_ratio_loss", "loss_rpn_bbox"):
        assert float(parsed[k].detach()) > 0, k
    g = {n: p.grad for n, p in m.named_parameters() if p.requires_grad}
    bad = [n for n, v in g.items() if v is None or not bool(torch.isfinite(v).all())]
    assert not bad, bad
    for n in ("bbox_head.fix_pred.weight", "bbox_head.ratio_pred.weight", "bbox_head.bbox_pred.weight",
              "bbox_head.fc1.weight", "rpn.rpn_reg.weight", "neck.fpn_convs.0.conv.weight"):
        assert float(g[n].abs().sum()) > 0, n
    m.zero_grad(set_to_none=True)
    for _ in range(2):
        loss, parts = runner.train_step(images, targets)
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v).all()) for v in parts.values())
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_no_positive_row_gives_zero_loss_and_zero_gradient(dev, runner):
    head = runner.model.bbox_head
    R_, C = 64, 15
    preds = [torch.randn(R_, k, device=dev, requires_grad=True) for k in (C + 1, 4 * C, 4 * C, C)]
    labels = torch.full((R_,), C, dtype=torch.long, device=dev)
    z = lambda k: torch.zeros((R_, k), device=dev)      # noqa: E731
    pos = torch.zeros((R_,), dtype=torch.bool, device=dev)
    losses = head.loss(*preds, labels, torch.ones((R_,), device=dev), z(4), z(4), z(1), pos, ~pos)
    sum(v.sum() for v in losses.values()).backward()
    for k, p in zip(("gliding_bbox_loss", "gliding_fix_loss", "gliding_ratio_loss"), preds[1:]):
        assert float(losses[k].detach()) == 0.0 and bool((p.grad == 0).all()), k
    assert float(losses["gliding_cls_loss"]) > 0


def test_inference_output(dev, runner):
    from jdet_amd.runner import synthetic_batch
    images, targets = synthetic_batch(2, 256, dev, seed=5, num_gts=10)
    m = runner.model
    m.eval()
    with torch.no_grad():
        res = m(images, targets)
    m.train()
    assert len(res) == 2
    for polys, scores, labels in res:
        k = polys.shape[0]
        assert tuple(polys.shape) == (k, 8) and tuple(scores.shape) == (k,) and tuple(labels.shape) == (k,)
        assert k > 0 and int(labels.min()) >= 0 and int(labels.max()) < 15
        assert bool(torch.isfinite(polys).all()) and float(scores.min()) > 0.05
        assert bool((scores[:-1] >= scores[1:]).all())
