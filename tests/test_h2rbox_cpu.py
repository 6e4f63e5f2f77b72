"""CPU: the H2RBox pieces that need no device -- the fixtures' conditions; the names in SIGNATURES; the
argument checks of the three entry points (they return before any launch); the registry names; the general routes of
rotate_crop, H2RBoxLoss and H2RBoxHead.loss against the restatements of tests/h2rbox_ref.py; closed forms of the
consistency loss; rotated_box_to_hbbox_np against hand values; H2RBOX_CFG against the reference's file as `Config`
reads it."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import h2rbox_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = [(rot, win) for rot in R.ROTS for win in (1, 2)]
IDS = ["rot%.2f-branch%d" % f for f in FIXTURES]


# ------------------------------------------------------------------------------------------------------------ fixtures
def test_loss_fixtures_hold_the_conditions():
    seen = dict(left=0, shared=0, agnostic=0)
    for rot, win in FIXTURES:
        ref, e_loss, e_g1, e_g2 = R.loss_reference(rot, win)
        m = ref["margins"]
        print("rot %.4f branch %d: %d positives, %d valid, %d leave their level, %d shared view-2 cells, %d agnostic rows, "
              "%d redrawn; tie margin %.2e, margins %s, min IoU %.3f; S1 %.4f S2 %.4f; float32 against float64: loss %.2e "
              "grad %.2e / %.2e" % (rot, win, ref["positives"], ref["valid"], ref["left"], ref["shared_cells"],
                                    ref["agnostic_rows"], R.loss_fixture(rot, win)[4], ref["tie_margin"],
                                    {k: round(v, 4) for k, v in m.items()}, ref["min_iou"], ref["sums"][1],
                                    ref["sums"][2], e_loss, e_g1, e_g2))
        assert ref["tie_margin"] >= 1e-3
        assert all(v >= 1e-3 for v in m.values()), m
        assert ref["min_iou"] >= 0.05
        assert ref["branch"] == win - 1 and ref["branch_gap"] >= 1e-3       # the scalar minimum is decided
        assert ref["valid"] >= 100 and ref["loss"] > 0
        assert np.abs(ref["grad_pred"]).max() > 0 and np.abs(ref["grad_aug"]).max() > 0   # both views get gradient
        assert 0 <= e_loss < 1e-5 and 0 < e_g1 < 1e-5 and 0 < e_g2 < 1e-5
        seen["left"] += ref["left"]
        seen["shared"] += ref["shared_cells"]
        seen["agnostic"] += ref["agnostic_rows"]
        pred, pred_aug, weight, labels, _ = R.loss_fixture(rot, win)
        assert pred.dtype == pred_aug.dtype == weight.dtype == np.float32 and labels.dtype == np.int32
        assert ((labels == R.NUM_CLASSES) == (weight == 0)).all()
        # the single-cell level maps onto itself whatever the angle
        one = R.level_offsets()[3]
        assert R.SIZES[3] == (1, 1) and all(ref["aug_index"][b, one] in (one, -1) for b in range(R.B))
    assert (1, 1) in R.SIZES and seen["left"] > 0 and seen["shared"] > 0 and seen["agnostic"] > 0
    assert any(h != w for h, w in R.SIZES) and R.N == 120


def test_rotate_crop_fixtures_leave_the_frame_on_all_four_sides():
    """at each non-trivial angle the source positions of the 37 x 37 frame cropped to 32 x 32 and of the 40 x 56 frame
    cropped to 38 x 54 leave the frame on all four sides, by more than half a pixel, so reflection, border and zeros act on
    a square and on a non-square frame (where the reference's map is no isometry).  The 40 x 56 frame cropped to
    24 x 40 keeps a margin of 8 px and stays inside at both angles: it pins the interior of the non-square map."""
    for theta in (0.3, -2.5):
        for (h, w), size in (((37, 37), (32, 32)), ((40, 56), (38, 54)), ((40, 56), (24, 40))):
            ix, iy = R.source_positions(h, w, size, theta)
            beyond = np.array([-ix.min(), ix.max() - (w - 1), -iy.min(), iy.max() - (h - 1)])
            print("frame %dx%d crop %s theta %.1f: ix %.1f .. %.1f, iy %.1f .. %.1f, beyond the frame by %s"
                  % (h, w, size, theta, ix.min(), ix.max(), iy.min(), iy.max(), np.round(beyond, 1).tolist()))
            if size == (24, 40):
                assert (beyond < 0).all()
            else:
                assert (beyond > 0.5).all()
    # the quarter and half turns of the square frame stay inside it (a permutation of the pixels)
    for theta in (math.pi / 2, -math.pi / 2, math.pi):
        ix, iy = R.source_positions(37, 37, (32, 32), theta)
        assert ix.min() > -1e-4 and ix.max() < 36 + 1e-4 and iy.min() > -1e-4 and iy.max() < 36 + 1e-4


# ---------------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def built_lib():
    from jdet_amd import _lib
    _lib.build()
    return _lib


def test_header_signatures_and_exports_agree(built_lib):
    assert {"jdet_rotate_crop", "jdet_h2rbox_aug_loss_forward",
            "jdet_h2rbox_aug_loss_backward"} <= set(built_lib.SIGNATURES)


def test_argument_checks_return_before_any_launch(built_lib):
    lib = built_lib.lib()
    N, X = None, 4096                                        # X: a non-null address nobody reads
    nan, inf = float("nan"), float("inf")

    def rc(img=X, n=2, c=3, h=8, w=8, oh=4, ow=4, cs=0.5, sn=0.5, pad=2, out=X):
        return lib.jdet_rotate_crop(img, n, c, h, w, oh, ow, cs, sn, pad, out, N)
    assert rc(img=N) == -1 and rc(out=N) == -1
    for k in ("n", "c", "oh", "ow"):
        assert rc(**{k: 0}) == -1 and rc(**{k: -1}) == -1, k
    assert rc(h=1, oh=1) == -1 and rc(w=1, ow=1) == -1                    # H < 2, W < 2
    assert rc(oh=9) == -1 and rc(ow=9) == -1                              # the crop exceeds the frame
    assert rc(pad=3) == -1 and rc(pad=-1) == -1
    assert rc(cs=nan) == -1 and rc(sn=inf) == -1
    assert rc(n=65536) == -2 and rc(n=4, c=4, h=20000, w=20000) == -2

    lv = (ctypes.c_int32 * 6)(4, 4, 8, 2, 2, 16)
    ag = (ctypes.c_int32 * 2)(3, 7)

    def args(levels=lv, L=2, pred=X, aug=X, w=X, lab=X, agn=ag, na=2, B=2, rot=0.3, cs=0.9, sn=0.3, ch=32, cw=32, ws=1.0,
             wa=1.0, eps=1e-6):
        return (levels, L, pred, aug, w, lab, agn, na, B, rot, cs, sn, ch, cw, ws, wa, eps)

    def fw(terms=X, idx=X, **kw):
        return lib.jdet_h2rbox_aug_loss_forward(*args(**kw), terms, idx, N)

    def bw(idx=X, br=X, sc=X, sb=X, g1=X, g2=X, scratch=X, **kw):
        return lib.jdet_h2rbox_aug_loss_backward(*args(**kw), idx, br, sc, sb, g1, g2, scratch, N)
    for f in (fw, bw):
        for null in ("levels", "pred", "aug", "w", "lab", "agn"):
            assert f(**{null: N}) == -1, null
        assert f(B=0) == -1 and f(L=0) == -1 and f(ch=0) == -1 and f(cw=-3) == -1 and f(na=-1) == -1
        assert f(levels=(ctypes.c_int32 * 6)(4, 0, 8, 2, 2, 16)) == -1       # W = 0
        assert f(levels=(ctypes.c_int32 * 6)(4, 4, 8, 2, 2, 0)) == -1        # stride = 0
        assert f(eps=0.0) == -1 and f(eps=nan) == -1 and f(rot=nan) == -1 and f(cs=inf) == -1 and f(sn=nan) == -1
        assert f(L=9, levels=(ctypes.c_int32 * 27)(*([1, 1, 1] * 9))) == -2
        assert f(na=17, agn=(ctypes.c_int32 * 17)()) == -2 and f(B=65536) == -2
        assert f(levels=(ctypes.c_int32 * 6)(20000, 20000, 1, 2, 2, 16)) == -2   # B * N * 5 beyond 2^31 - 1
    assert fw(terms=N) == -1 and fw(idx=N) == -1
    for null in ("idx", "br", "sc", "sb", "g1", "g2", "scratch"):
        assert bw(**{null: N}) == -1, null


# -------------------------------------------------------------------------------------------------- registry, config
def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return [_plain(x) for x in v] if isinstance(v, (list, tuple)) else v


def test_named_config_equals_the_reference_file():
    from jdet_amd.config import Config
    from jdet_amd.config.named import H2RBOX_CFG
    c = Config(os.path.join(ROOT, "tests", "golden", "configs", "h2rbox_obb_r50_adamw_fpn_1x_dota.yaml")).dump()
    for k in ("model", "optimizer", "scheduler"):
        assert _plain(c[k]) == _plain(H2RBOX_CFG[k]), k
    assert H2RBOX_CFG["optimizer"]["type"] == "AdamW" and H2RBOX_CFG["optimizer"]["weight_decay"] == 0.05


def test_registry_builds_the_losses_the_head_the_model_the_optimizer_and_the_dataset():
    import jdet_amd.data.datasets  # noqa: F401
    import jdet_amd.models  # noqa: F401
    import jdet_amd.optims  # noqa: F401
    from jdet_amd.config.named import H2RBOX_CFG
    from jdet_amd.utils import registry as Reg
    l1 = Reg.build_from_cfg(dict(type="L1Loss", loss_weight=0.5), Reg.LOSSES)
    iou = Reg.build_from_cfg(dict(type="IoULoss", loss_weight=2.0, reduction="sum"), Reg.LOSSES)
    assert l1.loss_weight == 0.5 and l1.reduction == "mean" and iou.loss_weight == 2.0 and iou.reduction == "sum"
    aug = Reg.build_from_cfg(H2RBOX_CFG["model"]["roi_heads"]["loss_bbox_aug"], Reg.LOSSES)
    assert type(aug).__name__ == "H2RBoxLoss" and aug.loss_weight == 0.4 and aug.center_loss.loss_weight == 0.0
    assert type(aug.shape_loss).__name__ == "IoULoss" and type(aug.angle_loss).__name__ == "L1Loss" and aug.dense_ok()
    m = Reg.build_from_cfg(H2RBOX_CFG["model"], Reg.MODELS)
    h = m.bbox_head
    assert type(m).__name__ == "H2RBox" and type(h).__name__ == "H2RBoxHead" and isinstance(h, Reg.HEADS.get("FCOSHead"))
    assert m.crop_size == (1024, 1024) and m.padding == "reflection" and m.fixed_rot is None
    assert h.crop_size == (1024, 1024) and h.rect_classes == [9, 11] and h.rotation_agnostic_classes is None
    assert type(h.loss_bbox).__name__ == "IoULoss" and type(h.loss_bbox_aug).__name__ == "H2RBoxLoss" and h.dense
    names = {n for n, _ in h.named_parameters()}
    for n in ("reg_convs.3.gn.bias", "conv_reg.weight", "conv_theta.bias", "scales.4.scale", "scale_t.scale"):
        assert n in names, n
    for meth in ("forward_aug", "execute_train", "obb2xyxy"):
        assert callable(getattr(h, meth))
    opt = Reg.build_from_cfg(dict(H2RBOX_CFG["optimizer"], grad_clip=dict(max_norm=35, norm_type=2)), Reg.OPTIMS,
                             params=list(h.parameters()))
    assert type(opt).__name__ == "AdamW" and isinstance(opt, torch.optim.AdamW) and opt.cur_lr() == 0.0001
    assert opt.param_groups[0]["weight_decay"] == 0.05 and opt.param_groups[0]["betas"] == (0.9, 0.999)
    w0 = h.conv_theta.weight.detach().clone()
    opt.step((h.conv_theta.weight ** 2).sum())               # step(loss): backward, clip, update
    assert not torch.equal(w0, h.conv_theta.weight.detach())
    ds = Reg.DATASETS.get("DOTAWSOODDataset")
    assert ds is not None and issubclass(ds, Reg.DATASETS.get("DOTADataset"))


def test_rotated_box_to_hbbox_np_against_hand_values():
    from jdet_amd.data.datasets import DOTAWSOODDataset, rotated_box_to_hbbox_np
    c30, s30 = math.cos(math.pi / 6), math.sin(math.pi / 6)
    boxes = np.array([[50, 40, 20, 10, 0.0],                 # already horizontal
                      [50, 40, 10, 20, 0.0],                 # taller than wide: (w, h) = (20, 10), angle pi / 2
                      [0, 0, 20, 10, math.pi / 2],           # a quarter turn: 10 wide, 20 tall
                      [5, -3, 20, 10, math.pi / 6]], np.float32)
    want = np.array([[50, 40, 20, 10, 0], [50, 40, 20, 10, math.pi / 2], [0, 0, 20, 10, math.pi / 2],
                     [5, -3, 20 * c30 + 10 * s30, 20 * s30 + 10 * c30, 0]])
    got = rotated_box_to_hbbox_np(boxes)
    assert got.shape == (4, 5) and got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-4)
    assert DOTAWSOODDataset.rotated_box_to_hbbox_np(np.zeros((0, 5), np.float32)).shape == (0, 5)


# ------------------------------------------------------------------------------------------------------ general routes
@pytest.mark.parametrize("padding", ["reflection", "border", "zeros"])
def test_general_rotate_crop_matches_the_restatement(padding):
    from jdet_amd.ops.rotate_crop import rotate_crop
    img = R.image_fixture(40, 56)
    for theta in (0.0, 0.3, -2.5):
        want = R.rotate_crop(img, theta, (24, 40), padding, torch.float32)
        got = rotate_crop(torch.from_numpy(img.copy()), theta, (24, 40), padding).numpy()
        assert got.shape == (2, 3, 24, 40) and np.array_equal(got, want)
    assert np.array_equal(R.rotate_crop(img, 0.0, (24, 40), padding, torch.float32), img[..., 8:32, 8:48])


def _head(agnostic=R.AGNOSTIC, weights=R.WEIGHTS):
    from jdet_amd.models.roi_heads.h2rbox_head import H2RBoxHead
    return H2RBoxHead(
        num_classes=R.NUM_CLASSES, in_channels=8, feat_channels=32, stacked_convs=1, strides=list(R.STRIDES),
        regress_ranges=((-1, 16), (16, 32), (32, 64), (64, 128), (128, 1e8)), crop_size=R.CROP,
        rotation_agnostic_classes=agnostic, loss_bbox=dict(type="IoULoss", loss_weight=1.0),
        loss_bbox_aug=dict(type="H2RBoxLoss", loss_weight=weights["loss_weight"],
                           center_loss_cfg=dict(type="L1Loss", loss_weight=weights["centre"]),
                           shape_loss_cfg=dict(type="IoULoss", loss_weight=weights["shape"]),
                           angle_loss_cfg=dict(type="L1Loss", loss_weight=weights["angle"])))


def general_aug_loss(head, pred, pred_aug, weight, labels, rot, dtype=torch.float64):
    """the consistency loss of H2RBoxHead._loss_general on prescribed targets: the head's own targets are replaced by
    (labels, weight), everything after them is the head's code.  -> (loss, grad_pred, grad_aug) in image-major order"""
    off = R.level_offsets()
    p1 = torch.tensor(pred, dtype=dtype, requires_grad=True)
    p2 = torch.tensor(pred_aug, dtype=dtype, requires_grad=True)
    maps = lambda t, l, c: t[:, off[l]:off[l + 1], c].reshape(R.B, R.SIZES[l][0], R.SIZES[l][1], -1).permute(0, 3, 1, 2)  # noqa: E731
    nl = len(R.SIZES)
    cls = [torch.zeros((R.B, R.NUM_CLASSES) + R.SIZES[l], dtype=dtype) for l in range(nl)]
    ctr = [torch.zeros((R.B, 1) + R.SIZES[l], dtype=dtype) for l in range(nl)]
    outs = (cls, [maps(p1, l, slice(0, 4)) for l in range(nl)], [maps(p1, l, slice(4, 5)) for l in range(nl)], ctr)
    outs_aug = ([maps(p2, l, slice(0, 4)) for l in range(nl)], [maps(p2, l, slice(4, 5)) for l in range(nl)])
    lab = torch.from_numpy(labels.astype(np.int32))
    w = torch.tensor(weight, dtype=dtype)
    head.get_targets = lambda points, targets, dense=True, featmap_sizes=None: (
        [lab[:, off[l]:off[l + 1]].reshape(-1) for l in range(nl)],
        [torch.zeros((R.B * (off[l + 1] - off[l]), 5), dtype=dtype) for l in range(nl)])
    lw = torch.cat([w[:, off[l]:off[l + 1]].reshape(-1) for l in range(nl)])
    head.centerness_target = lambda pos_bbox_targets: lw[lw > 0]
    sizes = [tuple(s) for s in R.SIZES]
    losses = head._loss_general(outs, outs_aug, rot, sizes, head.get_points(sizes, dtype), [dict()] * R.B)
    losses["loss_bbox_aug"].backward()
    return float(losses["loss_bbox_aug"].detach()), p1.grad.numpy(), p2.grad.numpy()


@pytest.mark.parametrize("rot,win", FIXTURES, ids=IDS)
def test_general_route_of_the_head_matches_the_restatement(rot, win):
    pred, pred_aug, weight, labels, _ = R.loss_fixture(rot, win)
    ref, e_loss, e_g1, e_g2 = R.loss_reference(rot, win)
    # float64 against float64: two writings of one program (image-major gathers against level-major ones)
    loss, g1, g2 = general_aug_loss(_head(), pred, pred_aug, weight, labels, R.f32(rot))
    k1, k2 = R.grad_errors(g1, g2, ref)
    print("float64 general route against the restatement: loss %.2e grad %.2e / %.2e" % (abs(loss - ref["loss"]), k1, k2))
    assert abs(loss - ref["loss"]) <= 1e-12 and k1 <= 1e-12 and k2 <= 1e-12
    loss, g1, g2 = general_aug_loss(_head(), pred, pred_aug, weight, labels, R.f32(rot), torch.float32)
    k1, k2 = R.grad_errors(g1, g2, ref)
    bound = 4 * e_loss
    print("float32 general route against float64: loss %.2e (bound %.2e) grad %.2e / %.2e (bounds %.2e / %.2e)"
          % (abs(loss - ref["loss"]), bound, k1, k2, 4 * e_g1, 4 * e_g2))
    assert abs(loss - ref["loss"]) <= bound and k1 <= 4 * e_g1 and k2 <= 4 * e_g2


def test_general_route_of_the_loss_module_matches_the_restatement():
    """H2RBoxLoss.forward on gathered rows against the same rows through the restatement's sub-losses"""
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils import registry as Reg
    rng = np.random.default_rng(5)
    n = 40
    prd = torch.tensor(np.concatenate([rng.uniform(0, 60, (n, 2)), rng.uniform(3, 8, (n, 2)), rng.uniform(-1.5, 1.5, (n, 1))], 1))
    tgt = torch.tensor(np.concatenate([rng.uniform(0, 60, (n, 2)), rng.uniform(3, 8, (n, 2)), rng.uniform(-1.5, 1.5, (n, 1))], 1))
    w = torch.tensor(rng.uniform(0.2, 1.0, n))
    loss = Reg.build_from_cfg(dict(type="H2RBoxLoss", loss_weight=0.4, center_loss_cfg=dict(type="L1Loss", loss_weight=0.5),
                                   shape_loss_cfg=dict(type="IoULoss", loss_weight=1.0),
                                   angle_loss_cfg=dict(type="L1Loss", loss_weight=1.0)), Reg.LOSSES)
    got = float(loss(prd, tgt, weight=w, avg_factor=float(w.sum())))
    avg = float(w.sum())
    h1 = torch.cat([-prd[:, 2:4], prd[:, 2:4]], -1)
    ht = torch.cat([-tgt[:, 2:4], tgt[:, 2:4]], -1)
    da = prd[:, 4] - tgt[:, 4]
    c = 0.5 * R._l1_loss(prd[:, :2], tgt[:, :2], w[:, None], avg)
    s1 = R._iou_loss(h1, ht, w, avg)[0] + R._l1_loss(da.sin(), torch.zeros_like(da), w, avg)
    s2 = R._iou_loss(h1[:, [1, 0, 3, 2]], ht, w, avg)[0] + R._l1_loss(da.cos(), torch.zeros_like(da), w, avg)
    assert abs(got - 0.4 * float(c + torch.minimum(s1, s2))) <= 1e-12
    # the minimum is of the SCALARS: a per-row minimum would be smaller here
    rows1 = -R.bbox_overlaps_aligned(h1, ht).log() + da.sin().abs()
    rows2 = -R.bbox_overlaps_aligned(h1[:, [1, 0, 3, 2]], ht).log() + da.cos().abs()
    assert float((torch.minimum(rows1, rows2) * w).sum() / avg) < float(torch.minimum(s1, s2)) - 1e-3


# --------------------------------------------------------------------------------------------------------- closed forms
def _uniform_views(theta2_shift=0.0, swap=False):
    """both views predict the same box at every point; view 2 optionally with (l, t, r, b) -> (t, l, b, r) (w and h
    swapped about the same centre offsets) and its angle shifted"""
    pred = np.tile(np.array([2.0, 1.0, 3.0, 1.5, 0.2]), (R.B, R.N, 1))
    aug = pred.copy()
    if swap:
        aug[..., :4] = pred[..., [1, 0, 3, 2]]
    aug[..., 4] += theta2_shift
    weight = np.full((R.B, R.N), 0.5)
    labels = np.full((R.B, R.N), 4, np.int32)
    return pred, aug, weight, labels


def test_closed_forms_of_the_consistency_loss():
    # identical views at rot = 0: every cell maps to itself, the target is the prediction: -log 1 + |sin 0| = 0
    pred, aug, weight, labels = _uniform_views()
    weights = dict(R.WEIGHTS, centre=0.0)
    r = R.aug_loss(pred, aug, weight, labels, 0.0, weights=weights, agnostic=())
    assert r["valid"] == R.B * R.N and r["left"] == 0 and (r["aug_index"] == np.arange(R.N)[None]).all()
    assert abs(r["loss"]) <= 1e-12 and r["branch"] == 0 and abs(r["sums"][1]) <= 1e-9
    # (w, h) = (5, 2.5): the swapped box overlaps it in 5 x 5 of 50 + 50 - 25, and |cos 0| = 1
    assert abs(r["sums"][2] - 0.5 * R.B * R.N * (math.log(3.0) + 1.0)) <= 1e-9
    loss, _, _ = general_aug_loss(_head(agnostic=None, weights=weights), pred, aug, weight, labels, 0.0)
    assert abs(loss) <= 1e-12
    # view 2 predicts w and h swapped and an angle pi / 2 further: regular_obb writes that box as the SAME (w, h) with
    # the angle turned back by pi, so it is the same box -- the loss is 0 again on branch 1 ...
    pred, aug, weight, labels = _uniform_views(theta2_shift=math.pi / 2, swap=True)
    r = R.aug_loss(pred, aug, weight, labels, 0.0, weights=weights, agnostic=())
    assert r["sums"][1] <= 1e-9 and r["branch"] == 0
    # ... while a view 2 of the same (w, h) with da = pi / 2 is the prediction "w, h swapped, da = pi / 2" of the loss's
    # decoded boxes: |cos da| = 0 and, for a SQUARE box, a swapped IoU of 1: branch 2 wins with loss 0 against |sin| = 1
    sq = np.tile(np.array([2.0, 2.0, 2.0, 2.0 - 1e-9, 0.2]), (R.B, R.N, 1))
    aug = sq.copy()
    aug[..., 4] += math.pi / 2
    r = R.aug_loss(sq, aug, weight, labels, 0.0, weights=weights, agnostic=())
    assert r["branch"] == 1 and abs(r["sums"][2]) <= 1e-6 and abs(r["sums"][1] - 0.5 * R.B * R.N) <= 1e-6
    assert abs(r["loss"]) <= 1e-8
    loss, _, _ = general_aug_loss(_head(agnostic=None, weights=weights), sq, aug, weight, labels, 0.0)
    assert abs(loss - r["loss"]) <= 1e-12
    # a non-square box, w and h swapped in the DECODED view-2 box (8 x 4 against 4 x 8 is impossible after regular_obb,
    # so the rows go to H2RBoxLoss directly): branch 2 = -log 1 + |cos(pi / 2)| = 0, branch 1 = -log(1 / 3) + 1
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils import registry as Reg
    loss_mod = Reg.build_from_cfg(dict(type="H2RBoxLoss", loss_weight=1.0, center_loss_cfg=dict(type="L1Loss", loss_weight=0.0),
                                       shape_loss_cfg=dict(type="IoULoss", loss_weight=1.0),
                                       angle_loss_cfg=dict(type="L1Loss", loss_weight=1.0)), Reg.LOSSES)
    p = torch.tensor([[10.0, 10.0, 4.0, 8.0, 0.3 + math.pi / 2]], dtype=torch.float64)
    t = torch.tensor([[10.0, 10.0, 8.0, 4.0, 0.3]], dtype=torch.float64)
    one = torch.ones(1, dtype=torch.float64)
    assert abs(float(loss_mod(p, t, weight=one, avg_factor=1.0))) <= 1e-12
    same_angle = torch.tensor([[10.0, 10.0, 4.0, 8.0, 0.3]], dtype=torch.float64)
    # da = 0: branch 1 = -log(iou(4x8, 8x4) = 1 / 3) + 0, branch 2 = 0 + |cos 0| = 1 -> min = 1
    assert abs(float(loss_mod(same_angle, t, weight=one, avg_factor=1.0)) - 1.0) <= 1e-12
