"""GPU: rotated FCOS -- the fused point targets (csrc/fcos_targets.hip) and the fused polygon IoU loss
(csrc/poly_iou_loss.hip) against the restatements of tests/fcos_ref.py, the head's dense route against its general
route, the buffer contracts of both entry points, and FCOS_CFG end to end (train, loss falls, no host sync, dense =
general, inference).

Targets.  128^2 image, strides 8..128 (341 points), the reference's regress ranges scaled to that image and a centre
sampling radius of 0.6, at which the centre test rejects points the other two tests accept (tests/fcos_ref.py).  The fixtures
are the ones tests/test_fcos_cpu.py holds to: every min / max / centre-sampling comparison at least 1e-3 px from its
threshold, |theta1| and |theta2| of mintheta_obb at least 1e-5 apart, areas distinct except in the tie case -- so the
float64 restatement decides what the fp32 kernel decides.  Labels and winner indices are compared exactly; a distance is
a three-term fp32 sum of products with a <= 2 ulp sincosf, bound 8 ulp of the largest coordinate magnitude of the
fixture; the centerness is compared with its closed form on the kernel's own targets (two divisions, a product, a square
root: 4 ulp).

Loss.  257 rows (tests/fcos_ref.py: loss_fixture; 96 % of the drawn pairs pass the generation filter, min IoU 0.052).
The float32 restatement differs from the float64 one on this fixture by 2.10e-05 in the loss and by 1.10e-04 of the
row's max |g| in the gradient; the kernel may differ from float64 by 4 x that (a different, legal, operation order).
Both reference errors are computed here from the restatements, never from the code under test."""
import numpy as np
import pytest
import torch

from tests import fcos_ref as R
from tests.abi_cases import (FCOS_CONTRACTS, fcos_centerness_bound as _centerness_bound, fcos_padded as _padded,
                             fcos_ulp as _ulp)

pytestmark = pytest.mark.gpu


def _check_targets(out, gts, labels, norm_on_bbox, center_sampling):
    lab, tgt, ctr, inds = [t.cpu().numpy() for t in out]
    tol = 8 * _ulp(max([float(R.IMG)] + [float(np.abs(g[:, :4]).max()) for g in gts if len(g)]))
    for b, (g, gl) in enumerate(zip(gts, labels)):
        ref = R.targets(g, gl, norm_on_bbox, center_sampling)
        assert np.array_equal(lab[b], ref["labels"]) and np.array_equal(inds[b], ref["inds"])
        err = float(np.abs(tgt[b] - ref["bbox_targets"]).max())
        t = tgt[b].astype(np.float32)
        pos = ref["inds"] >= 0
        with np.errstate(invalid="ignore", divide="ignore"):
            closed = np.sqrt((np.minimum(t[:, 0], t[:, 2]) / np.maximum(t[:, 0], t[:, 2]))
                             * (np.minimum(t[:, 1], t[:, 3]) / np.maximum(t[:, 1], t[:, 3])))
        c_err = float(np.abs(ctr[b][pos] - closed[pos]).max()) if pos.any() else 0.0
        print("image %d K %d: %d positives, max target error %.2e (bound %.2e), centerness against its closed form %.2e"
              % (b, len(g), int(pos.sum()), err, tol, c_err))
        assert err <= tol
        assert (ctr[b][~pos] == 0).all() and (tgt[b][~pos] == 0).all()
        if pos.any():
            assert (np.abs(ctr[b][pos] - closed[pos]) <= 4 * np.spacing(closed[pos])).all()
            assert (ctr[b][pos] > 0).all() and (ctr[b][pos] <= 1).all()
            assert (np.abs(ctr[b][pos] - ref["centerness"][pos]) <= _centerness_bound(ref, tol, norm_on_bbox)[pos]).all()


@pytest.mark.parametrize("norm_on_bbox,center_sampling", [(True, False), (False, False), (True, True), (False, True)],
                         ids=["norm", "plain", "norm-cs", "plain-cs"])
@pytest.mark.parametrize("name", sorted(R.TARGET_FIXTURES))
def test_targets_equal_the_restatement(dev, name, norm_on_bbox, center_sampling):
    from jdet_amd.models.roi_heads.fcos_head import fcos_targets_device
    gts, labels = R.target_fixture(name)
    g, gl, gc = _padded(gts, labels, dev)
    out = fcos_targets_device(list(R.SIZES), R.STRIDES, R.RANGES, g, gl, gc, R.NUM_CLASSES, norm_on_bbox,
                              center_sampling, R.RADIUS, with_inds=True)
    assert out[0].dtype == torch.int32 and out[0].shape == (len(gts), 341) and out[1].shape == (len(gts), 341, 5)
    _check_targets(out, gts, labels, norm_on_bbox, center_sampling)
    if name == "tie":
        inds = out[3].cpu().numpy()
        assert (inds == 2).sum() > 0 and (inds == 4).sum() == 0
    if name == "k7_k0":
        assert (out[0][1] == R.NUM_CLASSES).all()            # the image without gts: background, not class 0


@pytest.mark.parametrize("norm_on_bbox,center_sampling", [(True, False), (False, True)], ids=["norm", "plain-cs"])
@pytest.mark.parametrize("name", ["k7_k0", "k70", "tie"])
def test_dense_get_targets_equals_the_general_route(dev, name, norm_on_bbox, center_sampling):
    from jdet_amd.models.roi_heads.fcos_head import FCOSHead
    gts, labels = R.target_fixture(name)
    head = FCOSHead(num_classes=R.NUM_CLASSES, in_channels=8, feat_channels=32, stacked_convs=1, strides=list(R.STRIDES),
                    regress_ranges=R.RANGES, norm_on_bbox=norm_on_bbox, center_sampling=center_sampling,
                    center_sample_radius=R.RADIUS)
    points = head.get_points(list(R.SIZES), torch.float32, dev)
    targets = [dict(rboxes=torch.from_numpy(g.copy()).to(dev), labels=torch.from_numpy(lab.copy()).to(dev))
               for g, lab in zip(gts, labels)]
    dense = head.get_targets(points, targets, dense=True, featmap_sizes=list(R.SIZES))
    lattice = head.get_targets(points, targets, dense=True)           # the lattice rebuilt from the point lists
    general = head.get_targets(points, targets, dense=False)
    tol = 8 * _ulp(max([float(R.IMG)] + [float(np.abs(g[:, :4]).max()) for g in gts if len(g)]))
    assert len(dense[0]) == len(general[0]) == len(dense[1]) == len(general[1]) == 5
    for lv in range(5):
        assert dense[0][lv].dtype == general[0][lv].dtype == torch.int32
        assert torch.equal(dense[0][lv], general[0][lv]) and torch.equal(dense[0][lv], lattice[0][lv])
        assert dense[1][lv].shape == general[1][lv].shape and torch.equal(dense[1][lv], lattice[1][lv])
        assert float((dense[1][lv] - general[1][lv]).abs().max()) <= tol
    assert int(sum((t < R.NUM_CLASSES).sum() for t in dense[0])) > 0


# ------------------------------------------------------------------------------------------------- polygon IoU loss
def _device_loss(dev, prd, tgt, weight=None, linear=False, eps=1e-6):
    """jdet_poly_iou_loss through the autograd node: (loss (P,), pred.grad (P, 5)) as numpy"""
    from jdet_amd.models.losses.poly_iou_loss import poly_iou_loss
    p = torch.from_numpy(np.array(prd, np.float32)).to(dev).requires_grad_(True)
    t = torch.from_numpy(np.array(tgt, np.float32)).to(dev)
    w = torch.from_numpy(np.array(weight, np.float32)).to(dev) if weight is not None else None
    loss = poly_iou_loss(p, t, linear=linear, eps=eps, weight=w, reduction="none")
    assert loss.shape == (p.shape[0],) and loss.dtype == torch.float32
    loss.sum().backward()
    return loss.detach().cpu().numpy(), p.grad.cpu().numpy()


@pytest.mark.parametrize("linear,weighted", [(False, False), (True, False), (False, True)],
                         ids=["log", "linear", "log-weighted"])
def test_fused_loss_and_gradient_against_float64(dev, linear, weighted):
    prd, tgt, _ = R.loss_fixture()
    ref, e_loss, e_grad = R.loss_reference(linear, weighted)
    loss, grad = _device_loss(dev, prd, tgt, R.loss_weights() if weighted else None, linear)
    k_loss, k_grad = R.row_errors(loss, grad, ref)
    print("P %d linear %d weighted %d: float32 restatement against float64 loss %.3e grad %.3e; kernel loss %.3e grad %.3e"
          % (len(prd), linear, weighted, e_loss, e_grad, k_loss, k_grad))
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    assert k_loss <= 4 * e_loss
    assert k_grad <= 4 * e_grad


def test_fused_route_against_general_route(dev):
    from jdet_amd.models.losses.poly_iou_loss import poly_iou_loss
    prd, tgt, _ = R.loss_fixture()
    ref, e_loss, e_grad = R.loss_reference(False, True)
    w = torch.from_numpy(R.loss_weights().copy()).to(dev)
    t = torch.from_numpy(tgt.copy()).to(dev)
    out = {}
    for fused in (True, False):
        p = torch.from_numpy(prd.copy()).to(dev).requires_grad_(True)
        loss = poly_iou_loss(p, t, weight=w, reduction="none", fused=fused)
        loss.sum().backward()
        out[fused] = (loss.detach().cpu().numpy(), p.grad.cpu().numpy())
        print("fused %d against float64: loss %.3e grad %.3e" % ((fused,) + R.row_errors(*out[fused], ref)))
    d_loss = float(np.abs(out[True][0].astype(np.float64) - out[False][0]).max())
    d_grad = float((np.abs(out[True][1].astype(np.float64) - out[False][1]).max(1) / np.abs(ref["grad"]).max(1)).max())
    print("fused against general: loss %.3e (bound %.3e) grad %.3e (bound %.3e)" % (d_loss, 4 * e_loss, d_grad, 4 * e_grad))
    assert d_loss <= 4 * e_loss and d_grad <= 4 * e_grad
    # the mean with a device scalar as avg_factor
    p = torch.from_numpy(prd.copy()).to(dev)
    mean = poly_iou_loss(p, t, weight=w, reduction="mean", avg_factor=w.sum())
    assert mean.dim() == 0 and abs(float(mean) - out[True][0].sum() / float(w.sum())) <= 1e-5 * float(mean)


def test_closed_forms_on_the_device(dev):
    # a dozen fp32 roundings of coordinates ~100 (ulp 7.6e-6) on sizes >= 10: 1e-5 (tests/test_fcos_cpu.py)
    for name, (p, t, iou) in R.CLOSED_FORMS.items():
        loss, grad = _device_loss(dev, [p], [t])
        lin, _ = _device_loss(dev, [p], [t], linear=True)
        print(name, float(np.exp(-loss[0])), iou)
        assert abs(float(np.exp(-np.float64(loss[0]))) - iou) <= 1e-5, name
        assert abs(float(lin[0]) - (1 - iou)) <= 1e-5, name
    # iou = a1 / a2 for the contained pair: d(-log iou) / d(w, h) = -(1 / w, 1 / h), nothing else moves
    _, grad = _device_loss(dev, [R.CLOSED_FORMS["contained"][0]], [R.CLOSED_FORMS["contained"][1]])
    np.testing.assert_allclose(grad[0], [0, 0, -1 / 20.0, -1 / 10.0, 0], rtol=0, atol=1e-4)
    loss, grad = _device_loss(dev, [R.DISJOINT[0]], [R.DISJOINT[1]])
    assert float(loss[0]) == pytest.approx(-np.log(1e-6), rel=1e-6) and (grad == 0).all()
    loss, grad = _device_loss(dev, [R.DISJOINT[0]], [R.DISJOINT[1]], linear=True)
    assert float(loss[0]) == pytest.approx(1 - 1e-6, rel=1e-6) and (grad == 0).all()


def test_zero_weight_rows_cost_nothing_and_read_nothing(dev):
    prd, tgt, _ = R.loss_fixture()
    p = np.array(prd)
    p[::3] = np.nan                                          # NaN predictions in rows of weight 0
    t = np.array(tgt)
    t[1::3] = np.inf
    zeros = np.zeros(len(p), np.float32)
    loss, grad = _device_loss(dev, p, t, zeros)
    assert (loss == 0).all() and (grad == 0).all()
    w = np.array(R.loss_weights())
    w[::3] = 0
    w[1::3] = 0
    loss, grad = _device_loss(dev, p, t, w)
    ref = R.poly_iou_loss(prd[2::3], tgt[2::3], w[2::3])
    e = R.row_errors(loss[2::3], grad[2::3], ref)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    assert (loss[::3] == 0).all() and (grad[1::3] == 0).all() and (loss[2::3] > 0).all()
    _, e_loss, e_grad = R.loss_reference(False, True)
    assert e[0] <= 4 * e_loss and e[1] <= 4 * e_grad


# ----------------------------------------------------------------------------------------------------- buffer contracts
@pytest.mark.parametrize("case", ["targets k7_k0", "targets k7_k0 cs", "targets k70 cs", "loss", "loss weighted"])
def test_buffer_contract(dev, case):
    """guard bands, canaries, B == A bit for bit with poisoned outputs and NaN gt rows beyond the count, the restatement
    as the reference (tests/guarded.py)"""
    from tests import guarded
    c = FCOS_CONTRACTS[case]()
    guarded.run_case(c.entry_points[0], c.label, c.fn, dev)


# ------------------------------------------------------------------------------------------------------------ detector
def test_detector_trains_syncfree_dense_equals_general_and_infers(dev):
    """FCOS_CFG, 2 x 256^2, 8 gts per image: finite losses, the total falling over 6 Runner steps on a repeated batch;
    forward + backward of the dense route without a device -> host synchronisation; the dense route's three losses
    against the general route's at the loss tolerance of this file; inference returns polygons / scores / labels"""
    from jdet_amd.config.named import FCOS_CFG
    from jdet_amd.runner import Runner, synthetic_batch
    from jdet_amd.utils.general import parse_losses
    images, targets = synthetic_batch(2, 256, dev, seed=3, num_gts=8)
    torch.manual_seed(0)
    r = Runner(FCOS_CFG, device=dev, conv_autotune=False, graph=False)
    hist = [float(r.train_step(images, targets)[0]) for _ in range(6)]
    print("FCOS_CFG total loss", np.round(hist, 4).tolist())
    assert np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    m = r.model
    m.train()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, parsed = parse_losses(m(images, targets))
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert set(parsed) == {"loss_cls", "loss_bbox", "loss_centerness"} and torch.isfinite(total)
    assert all(torch.isfinite(v) for v in parsed.values())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.bbox_head.parameters())
    m.zero_grad(set_to_none=True)
    _, e_loss, _ = R.loss_reference()
    with torch.no_grad():
        dense = {k: float(v) for k, v in m(images, targets).items()}
        m.bbox_head.dense = False
        general = {k: float(v) for k, v in m(images, targets).items()}
        m.bbox_head.dense = True
    for k in dense:
        print("%s dense %.7f general %.7f (bound %.2e)" % (k, dense[k], general[k], 4 * e_loss))
        assert abs(dense[k] - general[k]) <= 4 * e_loss, k
    assert dense["loss_bbox"] > 0
    m.eval()
    with torch.no_grad():
        m.bbox_head.conv_cls.bias.fill_(-2.0)
        res = m(images, targets)
    assert len(res) == 2
    for polys, scores, labels in res:
        assert polys.dim() == 2 and polys.shape[1] == 8 and polys.shape[0] == scores.shape[0] == labels.shape[0]
        assert polys.shape[0] <= FCOS_CFG["model"]["roi_heads"]["test_cfg"]["max_per_img"]
    assert res[0][0].shape[0] > 0
