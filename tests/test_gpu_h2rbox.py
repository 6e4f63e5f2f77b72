"""GPU: H2RBox -- the fused rotated view (csrc/rotate_crop.hip) against grid_sample in float64, the fused consistency loss
(csrc/h2rbox_aug_loss.hip) forward and both gradients against the float64 restatement of tests/h2rbox_ref.py, the buffer
contracts of the three entry points, and H2RBOX_CFG end to end (train, loss falls, no host sync, dense = general,
inference with rect_classes).

Bounds.  Every bound is 4 x the error of the float32 restatement against the float64 one, computed here from the
restatements, never from the code under test, and printed:
  rotate_crop   per (frame, angle, padding) fixture: max |grid_sample float32 - grid_sample float64|;
  gradients     per loss fixture: max |g32 - g64| / max |g64|, for each view (about 1.1e-7 .. 1.6e-7);
  loss          per loss fixture: |loss32 - loss64| (1.2e-8 .. 1.2e-7 over the six, for some of them well below half an
                ulp of the loss: the float64 value happens to lie that close to a float32).  H2RBoxLoss.dense meets it
                because it sums the kernel's terms and forms the loss in float64 and rounds once: its result is the
                float32 nearest to the sum of the once-rounded terms, which is within a few 1e-9 of the float64 value,
                so it can be further from that value than the restatement's float32 only where the value lies about
                midway between two floats and both errors are about half an ulp.  Only the detector test, where no
                fixture applies, uses the largest of the six.
aug_index is compared exactly.  The losing branch's gradient is absent from the float64 reference (autograd through
torch.minimum of the two scalars), so the gradient comparison is also the test of its absence."""
import math

import numpy as np
import pytest
import torch

from tests import h2rbox_ref as R
from tests.abi_cases import H2RBOX_CONTRACTS as CONTRACTS, H2RBOX_FRAMES as FRAMES

pytestmark = pytest.mark.gpu

FIXTURES = [(rot, win) for rot in R.ROTS for win in (1, 2)]
IDS = ["rot%.2f-branch%d" % f for f in FIXTURES]
ANGLES = (0.0, math.pi / 2, -math.pi / 2, math.pi, 0.3, -2.5)


def detector_loss_bound():
    """for H2RBOX_CFG's own batch, which no fixture restates: 4 x the largest float32 error over the loss fixtures"""
    return 4 * max(R.loss_reference(*f)[1] for f in FIXTURES)


# --------------------------------------------------------------------------------------------------------- rotate_crop
@pytest.mark.parametrize("padding", ["reflection", "border", "zeros"])
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_rotate_crop_against_grid_sample_in_float64(dev, frame, padding):
    from jdet_amd.ops.rotate_crop import rotate_crop_device
    (h, w), size = FRAMES[frame]
    img = R.image_fixture(h, w)
    x = torch.from_numpy(img.copy()).to(dev)
    for theta in ANGLES:
        got = rotate_crop_device(x, theta, size, padding)
        assert got.shape == (2, 3) + size and got.dtype == torch.float32 and got.is_contiguous()
        got = got.cpu().numpy()
        if theta == 0:
            ch, cw = (h - size[0]) // 2, (w - size[1]) // 2
            assert np.array_equal(got, img[..., ch:ch + size[0], cw:cw + size[1]])      # bit for bit
            continue
        ref, e32 = R.rotate_crop_reference(h, w, size, theta, padding)
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print("%s %s theta %+.4f: float32 grid_sample against float64 %.3e, kernel %.3e (bound %.3e)"
              % (frame, padding, theta, e32, err, 4 * e32))
        assert np.isfinite(got).all() and e32 > 0
        assert err <= 4 * e32
    assert torch.equal(x.cpu(), torch.from_numpy(img))                                   # the input is not written


def test_rotate_crop_routes_agree_on_the_device(dev):
    """the general route (grid_sample on the device, float32) against the kernel, at the sum of both float32 bounds"""
    from jdet_amd.ops.rotate_crop import rotate_crop
    (h, w), size = FRAMES["40x56->24x40"]
    x = torch.from_numpy(R.image_fixture(h, w).copy()).to(dev)
    for theta in (0.0, 0.3, -2.5):
        a = rotate_crop(x, theta, size, "reflection", device_route=True)
        b = rotate_crop(x, theta, size, "reflection", device_route=False)
        e32 = R.rotate_crop_reference(h, w, size, theta, "reflection")[1] if theta else 0.0
        d = float((a - b).abs().max())
        print("theta %.1f: kernel against device grid_sample %.3e (bound %.3e)" % (theta, d, 8 * e32))
        assert d <= 8 * e32


# ------------------------------------------------------------------------------------------------------ consistency loss
def _head_loss():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils import registry as Reg
    w = R.WEIGHTS
    return Reg.build_from_cfg(dict(type="H2RBoxLoss", loss_weight=w["loss_weight"],
                                   center_loss_cfg=dict(type="L1Loss", loss_weight=w["centre"]),
                                   shape_loss_cfg=dict(type="IoULoss", loss_weight=w["shape"]),
                                   angle_loss_cfg=dict(type="L1Loss", loss_weight=w["angle"])), Reg.LOSSES)


def _device_aug_loss(dev, pred, pred_aug, weight, labels, rot):
    """H2RBoxLoss.dense -> (loss, aug_index, grad_pred, grad_aug) as python / numpy"""
    p1 = torch.from_numpy(np.array(pred, np.float32)).to(dev).requires_grad_(True)
    p2 = torch.from_numpy(np.array(pred_aug, np.float32)).to(dev).requires_grad_(True)
    w = torch.from_numpy(np.array(weight, np.float32)).to(dev)
    lab = torch.from_numpy(np.array(labels, np.int32)).to(dev)
    loss, idx = _head_loss().dense(list(R.SIZES), R.STRIDES, p1, p2, w, lab, R.AGNOSTIC, R.f32(rot), R.CROP)
    assert loss.dim() == 0 and idx.dtype == torch.int32 and idx.shape == (R.B, R.N)
    loss.backward()
    return float(loss.detach()), idx.cpu().numpy(), p1.grad.cpu().numpy(), p2.grad.cpu().numpy()


@pytest.mark.parametrize("rot,win", FIXTURES, ids=IDS)
def test_aug_loss_forward_and_both_gradients_against_float64(dev, rot, win):
    pred, pred_aug, weight, labels, _ = R.loss_fixture(rot, win)
    ref, e_loss, e_g1, e_g2 = R.loss_reference(rot, win)
    loss, idx, g1, g2 = _device_aug_loss(dev, pred, pred_aug, weight, labels, rot)
    k1, k2 = R.grad_errors(g1, g2, ref)
    print("rot %.4f branch %d: float32 restatement against float64 loss %.3e grad %.3e / %.3e; kernel loss %.3e "
          "(bound %.3e) grad %.3e / %.3e (bounds %.3e / %.3e)"
          % (rot, win, e_loss, e_g1, e_g2, abs(loss - ref["loss"]), 4 * e_loss, k1, k2, 4 * e_g1, 4 * e_g2))
    assert np.array_equal(idx, ref["aug_index"])
    assert np.isfinite(g1).all() and np.isfinite(g2).all()
    assert abs(loss - ref["loss"]) <= 4 * e_loss
    assert k1 <= 4 * e_g1 and k2 <= 4 * e_g2
    # rows that take no part get exactly nothing; view 2 gets gradient only where a valid row lands
    assert (g1[ref["aug_index"] < 0] == 0).all()
    hit = np.zeros((R.B, R.N), bool)
    for b in range(R.B):
        hit[b, ref["aug_index"][b][ref["aug_index"][b] >= 0]] = True
    assert (g2[~hit] == 0).all() and (np.abs(g2[hit]).max(1) > 0).all()


def test_aug_terms_select_the_scalar_minimum(dev):
    """the per-row terms against the float64 sums, and the branch the device picks from them"""
    from jdet_amd.models.losses.h2rbox_loss import h2rbox_aug_terms_device
    for rot, win in ((0.3, 1), (0.3, 2)):
        pred, pred_aug, weight, labels, _ = R.loss_fixture(rot, win)
        ref = R.loss_reference(rot, win)[0]
        rf = R.f32(rot)
        t, idx = h2rbox_aug_terms_device(list(R.SIZES), R.STRIDES, *[torch.from_numpy(a.copy()).to(dev) for a in
                                                                     (pred, pred_aug, weight, labels)], R.AGNOSTIC, rf,
                                         R.CROP, R.WEIGHTS["shape"], R.WEIGHTS["angle"], R.EPS)
        sums = t.double().reshape(-1, 4).sum(0).cpu().numpy()
        print("rot %.1f branch %d: sums %s against float64 %s" % (rot, win, sums.tolist(), ref["sums"].tolist()))
        # 4 columns of <= 240 float32 terms, each rounded once (2^-24 relative): the float64 sum of them is within
        # 2^-23 of the float64 reference's column sum
        assert np.all(np.abs(sums - ref["sums"]) <= 2.0 ** -23 * np.abs(ref["sums"]) + 1e-12)
        assert int(sums[2] < sums[1]) == win - 1
        valid = idx.cpu().numpy() >= 0
        assert (t.cpu().numpy()[~valid] == 0).all() and (t.cpu().numpy()[valid][:, 3] == weight[valid]).all()


def test_zero_weight_rows_read_nothing(dev):
    """NaN in view 1's rows of weight 0 and in the view-2 rows no valid row lands on: zeros and -1 there, and bit for
    bit the clean run's values elsewhere"""
    rot, win = -2.5, 1
    pred, pred_aug, weight, labels, _ = R.loss_fixture(rot, win)
    ref = R.loss_reference(rot, win)[0]
    clean = _device_aug_loss(dev, pred, pred_aug, weight, labels, rot)
    hit = np.zeros((R.B, R.N), bool)
    for b in range(R.B):
        hit[b, ref["aug_index"][b][ref["aug_index"][b] >= 0]] = True
    p1, p2 = pred.copy(), pred_aug.copy()
    p1[weight == 0] = np.nan
    p2[~hit] = np.nan
    assert np.isnan(p1).any() and np.isnan(p2).any() and (weight == 0).sum() > 20 and (~hit).sum() > 20
    loss, idx, g1, g2 = _device_aug_loss(dev, p1, p2, weight, labels, rot)
    assert np.isfinite(loss) and loss == clean[0] and np.array_equal(idx, clean[1])
    assert (idx[weight == 0] == -1).all()
    assert np.isfinite(g1).all() and np.isfinite(g2).all()
    assert np.array_equal(g1, clean[2]) and np.array_equal(g2, clean[3])
    assert (g1[weight == 0] == 0).all() and (g2[~hit] == 0).all()


def test_all_zero_weight_is_loss_zero_and_gradient_zero(dev):
    pred, pred_aug, weight, labels, _ = R.loss_fixture(0.3, 1)
    nan = np.full_like(pred, np.nan)
    loss, idx, g1, g2 = _device_aug_loss(dev, nan, nan, np.zeros_like(weight), np.full_like(labels, R.NUM_CLASSES), 0.3)
    assert loss == 0.0 and (idx == -1).all() and (g1 == 0).all() and (g2 == 0).all()


def test_two_runs_give_bit_identical_view_two_gradients(dev):
    pred, pred_aug, weight, labels, _ = R.loss_fixture(0.3, 1)            # 13 view-2 points shared by several rows
    assert R.loss_reference(0.3, 1)[0]["shared_cells"] > 0
    a = _device_aug_loss(dev, pred, pred_aug, weight, labels, 0.3)
    b = _device_aug_loss(dev, pred, pred_aug, weight, labels, 0.3)
    assert a[0] == b[0] and a[3].tobytes() == b[3].tobytes() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("rot,win", [(0.3, 2), (-2.5, 1)], ids=["rot0.30-branch2", "rot-2.50-branch1"])
def test_dense_route_of_the_loss_against_its_general_route(dev, rot, win):
    """H2RBoxLoss.forward (the general route) on the device in float64, fed the rows the exact map gathers, against the
    float64 restatement (two writings of one program: 1e-12), and H2RBoxLoss.dense against both at the fixture's bound"""
    from jdet_amd.models.boxes.box_ops import distance2obb
    pred, pred_aug, weight, labels, _ = R.loss_fixture(rot, win)
    ref, e_loss, _, _ = R.loss_reference(rot, win)
    dense = _device_aug_loss(dev, pred, pred_aug, weight, labels, rot)[0]
    idx = ref["aug_index"]
    b, p = np.nonzero(idx >= 0)
    q = idx[b, p]
    pts = np.concatenate([t.numpy() for t in R.points_of(torch.float64)])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)  # noqa: E731
    v1 = distance2obb(to(pts[p]), to(pred[b, p]))
    v2 = distance2obb(to(pts[q]), to(pred_aug[b, q]))
    rf = R.f32(rot)
    cs, sn = R.f32(math.cos(rf)), R.f32(math.sin(rf))
    cx, cy = (R.CROP[1] - 1) / 2, (R.CROP[0] - 1) / 2
    dx, dy = v1[:, 0] - cx, v1[:, 1] - cy
    xy = torch.stack([dx * cs - dy * sn + cx, dx * sn + dy * cs + cy], 1)
    agn = torch.from_numpy(np.isin(labels[b, p] + 1, R.AGNOSTIC)).to(dev)
    ang = torch.where(agn[:, None], torch.zeros_like(v1[:, 4:]), v1[:, 4:] + rf)
    w = to(weight[b, p])
    general = float(_head_loss()(v2, torch.cat([xy, v1[:, 2:4], ang], 1), weight=w, avg_factor=w.sum().clamp(min=1.0)))
    print("rot %.1f branch %d: dense %.9f general (float64) %.12f restatement %.12f (bound %.2e)"
          % (rot, win, dense, general, ref["loss"], 4 * e_loss))
    assert abs(general - ref["loss"]) <= 1e-12
    assert abs(dense - ref["loss"]) <= 4 * e_loss and abs(dense - general) <= 4 * e_loss


# ----------------------------------------------------------------------------------------------------- buffer contracts
@pytest.mark.parametrize("case", sorted(CONTRACTS))
def test_buffer_contract(dev, case):
    """guard bands, canaries, B == A bit for bit with poisoned outputs and NaN in the rows nobody may read
    (tests/guarded.py)"""
    from tests import guarded
    c = CONTRACTS[case]()
    guarded.run_case(c.entry_points[0], c.label, c.fn, dev)


# ------------------------------------------------------------------------------------------------------------ detector
def test_detector_trains_syncfree_dense_equals_general_and_infers(dev):
    """H2RBOX_CFG at 2 x 256^2 with crop (256, 256), 8 gts per image, fixed_rot = 0.7: the four losses finite and the
    total falling over 6 Runner steps on a repeated batch; forward + backward of the dense route without a device ->
    host synchronisation; the dense route's four losses against the general route's at the loss bound of this file;
    loss_bbox_aug > 0; inference returns polygons / scores / labels with the rect_classes boxes axis-aligned"""
    import copy
    from jdet_amd.config.named import H2RBOX_CFG
    from jdet_amd.runner import Runner, synthetic_batch
    from jdet_amd.utils.general import parse_losses
    cfg = copy.deepcopy(H2RBOX_CFG)
    cfg["model"]["crop_size"] = (256, 256)
    cfg["model"]["roi_heads"]["crop_size"] = (256, 256)
    images, targets = synthetic_batch(2, 256, dev, seed=3, num_gts=8)
    torch.manual_seed(0)
    r = Runner(cfg, device=dev, conv_autotune=False, graph=False)
    m = r.model
    m.fixed_rot = 0.7
    hist = [float(r.train_step(images, targets)[0]) for _ in range(6)]
    print("H2RBOX_CFG total loss", np.round(hist, 4).tolist())
    assert np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    m.train()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, parsed = parse_losses(m(images, targets))
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert set(parsed) == {"loss_cls", "loss_bbox", "loss_centerness", "loss_bbox_aug"} and torch.isfinite(total)
    assert all(torch.isfinite(v) for v in parsed.values())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.bbox_head.parameters())
    m.zero_grad(set_to_none=True)
    with torch.no_grad():
        dense = {k: float(v) for k, v in m(images, targets).items()}
        m.bbox_head.dense = False
        m.device_rotate = False
        general = {k: float(v) for k, v in m(images, targets).items()}
        m.bbox_head.dense = True
        m.device_rotate = True
    for k in dense:
        print("%s dense %.7f general %.7f (bound %.2e)" % (k, dense[k], general[k], detector_loss_bound()))
    for k in dense:
        assert abs(dense[k] - general[k]) <= detector_loss_bound(), k
    assert dense["loss_bbox_aug"] > 0
    m.eval()
    with torch.no_grad():
        m.bbox_head.conv_cls.bias.fill_(-2.0)
        res = m(images, targets)
    assert len(res) == 2
    rect = cfg["model"]["roi_heads"]["rect_classes"]
    seen_rect = 0
    for polys, scores, labels in res:
        assert polys.dim() == 2 and polys.shape[1] == 8 and polys.shape[0] == scores.shape[0] == labels.shape[0]
        assert polys.shape[0] <= cfg["model"]["roi_heads"]["test_cfg"]["max_per_img"]
        sel = torch.zeros_like(labels, dtype=torch.bool)
        for c in rect:
            sel |= labels == c
        p = polys[sel]
        seen_rect += int(sel.sum())
        # (xmin, ymin, xmin, ymax, xmax, ymax, xmax, ymin)
        assert torch.equal(p[:, 0], p[:, 2]) and torch.equal(p[:, 4], p[:, 6]) and torch.equal(p[:, 1], p[:, 7]) and \
            torch.equal(p[:, 3], p[:, 5])
    assert res[0][0].shape[0] > 0 and seen_rect > 0
