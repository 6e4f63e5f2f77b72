"""GPU: the fused ATSS assigner (csrc/atss_assign.hip) against the numpy restatement (tests/atss_ref.py) -- gt_inds and
labels equal, max_overlaps bit-equal -- in both modes (IoU computed in the kernel / read from an (A, K) matrix); the
hand-built tie, clamp and stride cases; the head's dense route against its general route; the buffer contract of
jdet_atss_assign; the ATSS RotatedRetinaNet config end to end (train, loss falls, no host sync, graph = eager,
inference).

The fixtures are the ones tests/test_atss_cpu.py holds to: no candidate within 1e-5 (relative) of a gt's edge, no
distance tie across a rank boundary -- so the restatement's float64 atan2 inside test and stable-sort ranking decide
exactly what the kernel's fp32 algebraic test and packed-key minima decide."""
import numpy as np
import pytest
import torch

from tests import atss_ref as R

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _device_assign(dev, anchors, num_level, gts, topk, labels=None, overlaps=None, filled=0):
    from jdet_amd.models.boxes.assigner import atss_assign_device
    a = torch.from_numpy(np.array(anchors)).to(dev)          # copies: the fixtures are read-only
    g = torch.from_numpy(np.array(gts)).to(dev)
    gl = torch.from_numpy(np.array(labels)).to(dev) if labels is not None else None
    return atss_assign_device(a, num_level, g, topk, gl, filled, overlaps)


def _same_as_ref(got, ref, with_labels):
    gt_inds, max_ov, labels = got
    assert gt_inds.dtype == torch.int32 and np.array_equal(gt_inds.cpu().numpy(), ref["gt_inds"])
    assert np.array_equal(_bits(max_ov), ref["max_overlaps"].view(np.int32))
    if with_labels:
        assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), ref["labels"])
    else:
        assert labels is None


@pytest.mark.parametrize("with_labels", [True, False], ids=["labels", "nolabels"])
@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_fused_mode_equals_the_restatement(dev, name, with_labels):
    anchors, num_level, gts, labels, ref = R.fixture(name)
    got = _device_assign(dev, anchors, num_level, gts, R.TOPK, labels if with_labels else None)
    _same_as_ref(got, ref, with_labels)
    assert int((got[0] > 0).sum()) >= gts.shape[0]


@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_matrix_mode_is_bit_identical_to_fused_mode(dev, name):
    """the matrix of jdet_box_iou_rotated fed back in; and another calculator through the assigner class"""
    from jdet_amd.models.boxes.assigner import ATSSAssignerRbbox
    from jdet_amd.ops import box_iou_rotated
    anchors, num_level, gts, labels, ref = R.fixture(name)
    a, g = torch.from_numpy(anchors.copy()).to(dev), torch.from_numpy(gts.copy()).to(dev)
    fused = _device_assign(dev, anchors, num_level, gts, R.TOPK, labels)
    matrix = _device_assign(dev, anchors, num_level, gts, R.TOPK, labels, overlaps=box_iou_rotated(a, g))
    for x, y in zip(fused, matrix):
        assert np.array_equal(_bits(x), _bits(y))
    _same_as_ref(matrix, ref, True)
    asg = ATSSAssignerRbbox(R.TOPK, iou_calculator=dict(type="FakeBboxOverlaps2D_rotated"), assigned_labels_filled=-1)
    res = asg.assign(a, num_level, g, None, torch.from_numpy(labels.copy()).to(dev))
    want = R.assign(anchors, num_level, gts, R.TOPK, labels, -1, overlaps=asg.iou_calculator(a, g).cpu().numpy())
    _same_as_ref((res.gt_inds, res.max_overlaps, res.labels), want, True)
    assert res.num_gts == gts.shape[0] and int((res.labels == -1).sum()) == int((res.gt_inds == 0).sum()) > 0


def test_two_identical_gts_the_lower_index_wins(dev):
    anchors, num_level, gts, _, _ = R.fixture("256a")
    twice = np.concatenate([gts[3:4], gts[3:4], gts[:2]], 0)
    ref = R.assign(anchors, num_level, twice, R.TOPK)
    got = _device_assign(dev, anchors, num_level, twice, R.TOPK)
    _same_as_ref(got, ref, False)
    inds = got[0].cpu().numpy()
    assert (inds == 1).sum() == ref["positives_per_gt"][0] > 0 and (inds == 2).sum() == 0
    assert ref["positives_per_gt"][1] == ref["positives_per_gt"][0]            # gt 1 claimed the same anchors and lost


def test_distance_tie_across_rank_nine_takes_the_lower_anchor_index(dev):
    """a gt centred on the middle of a cell of the finest level: 4 anchors at distance s / sqrt(2), then 8 at
    s * sqrt(2.5) -- ranks 5..12 tie, topk = 9 keeps five of the eight, the lower indices"""
    anchors, num_level = R.lattice(256)
    gt = np.asarray([[79.5, 79.5, 44.0, 36.0, 0.0]], np.float32)
    ref = R.assign(anchors, num_level, gt, R.TOPK)
    assert ref["boundary_ties"] >= 1 and ref["margin"] >= 1e-5
    d = np.hypot(anchors[:1024, 0] - 79.5, anchors[:1024, 1] - 79.5)
    tied = np.flatnonzero(np.isclose(d, 8 * np.sqrt(2.5)))
    assert tied.size == 8 and sorted(ref["cand"][0, 4:9].tolist()) == tied[:5].tolist()
    got = _device_assign(dev, anchors, num_level, gt, R.TOPK)
    _same_as_ref(got, ref, False)
    assert int((got[0] > 0).sum()) > 0


@pytest.mark.parametrize("topk", [1, 9])
def test_topk_one_and_nine(dev, topk):
    anchors, num_level, gts, labels, _ = R.fixture("256b")
    ref = R.assign(anchors, num_level, gts, topk, labels, 0)
    assert ref["cand"].shape[1] == (5 if topk == 1 else 40) and ref["margin"] >= 1e-5 and ref["boundary_ties"] == 0
    _same_as_ref(_device_assign(dev, anchors, num_level, gts, topk, labels), ref, True)


def test_anchor_stride_seven_with_nan_in_the_unused_columns(dev):
    anchors, num_level, gts, labels, ref = R.fixture("256a")
    wide = np.full((anchors.shape[0], 7), np.nan, np.float32)
    wide[:, :5] = anchors
    _same_as_ref(_device_assign(dev, wide, num_level, gts, R.TOPK, labels), ref, True)


def test_dense_head_route_equals_the_general_route(dev):
    """2 images x 256^2, 8 gts each: labels, label weights, box targets, box weights and the positive count"""
    from jdet_amd.config.named import ATSS_RETINANET_CFG
    from jdet_amd.models.roi_heads.rotated_atss_head import RotatedATSSHead
    head = RotatedATSSHead(**{k: v for k, v in ATSS_RETINANET_CFG["model"]["bbox_head"].items() if k != "type"})
    cfg = head.train_cfg.copy()
    anchors, num_level, _, _, _ = R.fixture("256a")
    levels = list(torch.split(torch.from_numpy(anchors.copy()).to(dev), num_level))
    gts = [torch.from_numpy(R.fixture(n)[2].copy()).to(dev) for n in ("256a", "256b")]
    labels = [torch.from_numpy(R.fixture(n)[3].copy()).to(dev) for n in ("256a", "256b")]
    metas = [dict(img_shape=(256, 256), pad_shape=(256, 256), _all_valid=True) for _ in range(2)]
    out = {}
    for dense in (True, False):
        al = [list(levels) for _ in range(2)]
        vf = [[torch.ones(n, dtype=torch.bool, device=dev) for n in num_level] for _ in range(2)]
        out[dense] = head.anchor_target(al, vf, gts, metas, head.target_means, head.target_stds, cfg,
                                        gt_labels_list=labels, label_channels=15, sampling=False, dense=dense)
    for a, b in zip(out[True][:4], out[False][:4]):
        assert len(a) == len(b) == 5
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y))
    assert isinstance(out[True][4], torch.Tensor) and int(out[True][4]) == out[False][4]
    want = sum(int((R.fixture(n)[4]["gt_inds"] > 0).sum()) for n in ("256a", "256b"))
    assert out[False][4] == want > 16
    lab0 = torch.cat([t[0] for t in out[True][0]]).cpu().numpy()
    assert np.array_equal(lab0, R.fixture("256a")[4]["labels"])


@pytest.mark.parametrize("name,matrix", [("256a", False), ("256a", True), ("512b", False), ("512b", True)])
def test_buffer_contract(dev, name, matrix):
    """guard bands, canaries, 0xFF workspace, B == A bit for bit, the restatement as the reference, and a workspace
    claim one byte short refused (tests/guarded.py)"""
    from tests import guarded
    from tests.abi_cases import atss_case
    case = atss_case(name, matrix)
    guarded.run_case(case.entry_points[0], case.label, case.fn, dev)


def test_detector_trains_syncfree_graph_equals_eager_and_infers(dev):
    """2 x 256^2, 8 gts per image (the last level has 4 anchors: min(topk, n)): finite losses, the total falling over 6
    Runner steps on a repeated batch; forward + backward without a device -> host synchronisation; the HIP-graph step
    follows the eager one within rtol 2e-2 (the bound of tests/test_gpu_gaussian_losses.py for the same comparison);
    inference returns polygons / scores / labels"""
    from jdet_amd.config.named import ATSS_RETINANET_CFG
    from jdet_amd.runner import Runner, synthetic_batch
    from jdet_amd.utils.general import parse_losses
    images, targets = synthetic_batch(2, 256, dev, seed=3, num_gts=8)
    hist = {}
    for mode in (False, True):
        torch.manual_seed(0)
        r = Runner(ATSS_RETINANET_CFG, device=dev, conv_autotune=False, graph=mode)
        hist[mode] = [float(r.train_step(images, targets)[0]) for _ in range(6)]
        m = r.model
        if not mode:
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                total, parsed = parse_losses(m(images, targets))
                total.backward()
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert set(parsed) == {"loss_cls", "loss_bbox"} and torch.isfinite(total)
            assert all(torch.isfinite(v) for v in parsed.values())
            m.zero_grad(set_to_none=True)
        else:
            assert len(r._graphs) == 1
            m.eval()
            with torch.no_grad():
                m.bbox_head.retina_cls.bias.fill_(-2.0)
                res = m(images, targets)
            assert len(res) == 2
            polys, scores, labels = res[0]
            assert polys.shape[1] == 8 and polys.shape[0] == scores.shape[0] == labels.shape[0] > 0
    e, g = np.array(hist[False]), np.array(hist[True])
    print("ATSS_RETINANET_CFG eager", np.round(e, 4).tolist(), "graph", np.round(g, 4).tolist())
    assert np.all(np.isfinite(e)) and e[-1] < e[0]
    np.testing.assert_allclose(g, e, rtol=2e-2)
