"""GPU: every regime of the shared NMS scan (csrc/nms_scan.h) against greedy references, through all three tile
kernels that feed it (nms_mask_kernel<false>, nms_mask_kernel<true>, poly_nms_mask_kernel).

The scan prefetches a 64-row block's words while the block reaches at most 128 column blocks to its right and takes
the fetch-after-resolve path for wider blocks, i.e. for the first col_blocks - 129 row blocks of every unlabelled input
with n > 8256 -- the detectors' own pre-NMS sizes.  Every comparison here is exact equality of keep masks; every
output buffer is filled with 7 first and must come back holding only 0 and 1.  tests/test_nms_ref_cpu.py shows from
the references alone that each n >= 8257 input holds boxes only the second path can suppress."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import nms_ref as R

pytestmark = pytest.mark.gpu

O.set_threads(8)


def _t(dev, a, dtype=None):
    """device copy of a (possibly read-only, shared) host array"""
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(dev)


def _flags(keep):
    k = keep.cpu().numpy()
    assert set(np.unique(k)) <= {0, 1}, "the scan left flags unwritten (7) or wrote something else"
    return k.astype(bool)


def _labeled(dev, dets, order, thr, cmp_ge, horizontal, n_labels):
    """jdet_nms_labeled on a keep buffer filled with 7"""
    from jdet_amd import _lib as L
    lib = L.lib()
    d = _t(dev, dets, np.float32)
    o = _t(dev, order, np.int32)
    n, bl = d.shape
    wsb = lib.jdet_nms_rotated_workspace(n)
    keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    ws = torch.empty((max(wsb, 8),), dtype=torch.uint8, device=dev)
    L.check(lib.jdet_nms_labeled(L.ptr(d), n, bl, L.ptr(o), float(thr), int(cmp_ge), 0, int(horizontal),
                                 int(n_labels), L.ptr(keep), L.ptr(ws), wsb, L.stream_ptr(d)), "jdet_nms_labeled")
    return _flags(keep)


def _poly(dev, polys, order, thr, n_labels):
    """jdet_nms_poly on a keep buffer filled with 7"""
    from jdet_amd import _lib as L
    lib = L.lib()
    p = _t(dev, polys, np.float32)
    o = _t(dev, order, np.int32)
    n, rl = p.shape
    wsb = lib.jdet_nms_rotated_workspace(n)
    keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    ws = torch.empty((max(wsb, 8),), dtype=torch.uint8, device=dev)
    L.check(lib.jdet_nms_poly(L.ptr(p), n, rl, L.ptr(o), float(thr), int(n_labels), L.ptr(keep), L.ptr(ws), wsb,
                              L.stream_ptr(p)), "jdet_nms_poly")
    return _flags(keep)


# --------------------------------------------------------------------------------------------------- rotated boxes
@pytest.mark.parametrize("n,thr,cmp_ge", [
    (1, 0.1, 1), (63, 0.1, 1), (64, 0.1, 1), (65, 0.1, 1),
    (8256, 0.1, 1),      # the last all-prefetch size: 8 words per thread in block 0
    (8257, 0.1, 1),      # block 0 takes the second path, the last block has one row
    (8321, 0.1, 1), (8704, 0.1, 1), (8704, 0.5, 0),
    (8321, 0.0, 1),      # zero_hits: an IoU of exactly 0 passes `>= 0`, the circle pre-filter must be off
    (8321, 0.0, 0),      # `> 0`: the pre-filter stays on
    (8321, -0.5, 0),     # zero_hits under the other rule
    (8321, 1.0, 1), (8321, 1.5, 1),
])
def test_rotated_vs_oracle(dev, n, thr, cmp_ge):
    """nms_mask_kernel<false> + scan == the CPU oracle's greedy loop (bit-exact IoU, so no pair is excluded)"""
    dets, _, order, _ = R.rotated_case(n)
    ref = O.nms_rotated_keep(dets, order, thr, cmp_ge=cmp_ge)
    got = _labeled(dev, dets, order, thr, cmp_ge, 0, 1)
    print("rotated n %d thr %g rule %s: kept %d (oracle %d)"
          % (n, thr, ">=" if cmp_ge else ">", int(got.sum()), int(ref.sum())))
    np.testing.assert_array_equal(got, ref)
    if (thr == 0.0 and cmp_ge) or thr < 0:
        assert got.sum() == 1 and got[order[0]]
    if thr > 1:
        assert got.all()


def test_rotated_15_labels_one_scan(dev):
    """six-column dets, 15 random labels, n = 8704, visited as ml_nms_rotated does, one scan: label-homogeneous tiles
    at full size (tile_jmax is then a few blocks away: all prefetch, unlike the unlabelled input of the same size)"""
    n = 8704
    dets, scores, _, labels = R.rotated_case(n)
    d6 = np.concatenate([dets, labels[:, None]], 1)
    order = R.label_order(scores, labels)
    ref = O.nms_rotated_keep(d6, order, 0.1, cmp_ge=1)
    np.testing.assert_array_equal(_labeled(dev, d6, order, 0.1, 1, 0, 1), ref)
    assert ref.sum() > O.nms_rotated_keep(dets, R.score_order(scores), 0.1, cmp_ge=1).sum()   # the labels matter


def test_rotated_level_layout_per_label_scan(dev):
    """labels [8400, 0, 1, 333] (n = 8734): label 0's first three row blocks take the second path inside a per-label
    scan; one workgroup per label and the single scan both equal the oracle on the six-column dets"""
    n = 8734
    dets, scores, _, _ = R.rotated_case(n)
    labels = R.level_labels()
    d6 = np.concatenate([dets, labels[:, None]], 1)
    order = R.label_order(scores, labels)
    ref = O.nms_rotated_keep(d6, order, 0.1, cmp_ge=1)
    np.testing.assert_array_equal(_labeled(dev, d6, order, 0.1, 1, 0, 4), ref)
    np.testing.assert_array_equal(_labeled(dev, d6, order, 0.1, 1, 0, 1), ref)
    assert 0 < ref.sum() < n


# ------------------------------------------------------------------------------------------------ horizontal boxes
def _hbb_obb(boxes):
    """ops/nms.py's centre / size columns (exact in fp32 under the recipe)"""
    b = boxes.astype(np.float32)
    return np.stack([(b[:, 0] + b[:, 2]) * np.float32(0.5), (b[:, 1] + b[:, 3]) * np.float32(0.5), b[:, 2] - b[:, 0],
                     b[:, 3] - b[:, 1], np.zeros_like(b[:, 0])], 1)


@pytest.mark.parametrize("n", [8256, 8257, 8704])
@pytest.mark.parametrize("thr", [0.6875, 0.125, 0.0])
def test_horizontal_vs_exact_greedy(dev, n, thr):
    """nms_mask_kernel<true> + scan through ops.nms.nms_keep_mask (`>` rule) == greedy over the exact rational
    decisions (integer recipe, dyadic threshold: no pair has to be excluded, see nms_ref.hbb_hits_exact)"""
    from jdet_amd.ops.nms import nms_keep_mask
    boxes, scores, order = R.hbb_case(n)
    hit = R.hbb_hits_exact(boxes[order], thr)
    keep_pos = R.greedy_keep(hit)
    ref = R.to_original(keep_pos, order)
    wit = R.wide_path_witnesses(keep_pos, hit, n)
    print("hbb n %d thr %g: kept %d, witnesses %d" % (n, thr, int(ref.sum()), wit))
    assert (wit >= 1) == (n > 8256)
    got, got_order = nms_keep_mask(_t(dev, boxes), _t(dev, scores), thr)
    np.testing.assert_array_equal(got_order.cpu().numpy(), order)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)
    # the wrapper zero-fills its own buffer: the same launch on a buffer of 7s
    np.testing.assert_array_equal(_labeled(dev, _hbb_obb(boxes), order, thr, 0, 1, 1), ref)


def test_horizontal_level_layout(dev):
    """n = 8734, labels [8400, 0, 1, 333], n_labels = 4: the wrapper's own ordering and the caller's visit_order"""
    from jdet_amd.ops.nms import nms_keep_mask
    n, thr = 8734, 0.5
    boxes, scores, _ = R.hbb_case(n)
    labels = R.level_labels()
    visit = R.label_order(scores, labels)
    hit = R.hbb_hits_exact(boxes[visit], thr) & R.same_label(labels[visit])
    keep_pos = R.greedy_keep(hit)
    ref = R.to_original(keep_pos, visit)
    assert R.wide_path_witnesses(keep_pos, hit, n, R.wide_row_blocks(n, labels[visit], 4)) >= 1
    b, s, l = (_t(dev, a) for a in (boxes, scores, labels))
    got, _ = nms_keep_mask(b, s, thr, labels=l, n_labels=4)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)
    v = _t(dev, visit)
    got, got_order = nms_keep_mask(b, s, thr, labels=l, n_labels=4, visit_order=v)
    assert got_order is v
    np.testing.assert_array_equal(got.cpu().numpy(), ref)
    d6 = np.concatenate([_hbb_obb(boxes), labels[:, None]], 1)
    np.testing.assert_array_equal(_labeled(dev, d6, visit, thr, 0, 1, 4), ref)
    assert 0 < ref.sum() < n


# -------------------------------------------------------------------------------------------------------- polygons
def _polys(n):
    from jdet_amd.data.np_boxes import rotated_box_to_poly_np
    dets, scores, order, _ = R.rotated_case(n)
    polys = rotated_box_to_poly_np(dets)
    polys[::3] = polys[::3].reshape(-1, 4, 2)[:, ::-1].reshape(-1, 8)      # every third polygon clockwise
    return polys, scores, order


def _device_hits(dev, polys_sorted, thr):
    from jdet_amd.ops.nms_poly import poly_iou_matrix
    p = _t(dev, polys_sorted)
    return (poly_iou_matrix(p, p, mode=0) > thr).cpu().numpy()


@pytest.mark.parametrize("n", [8257, 8704])
def test_polygon_vs_greedy_over_device_iou(dev, n):
    """poly_nms_mask_kernel + scan == greedy_keep(M > thr), M = poly_iou_matrix(sorted, sorted, mode=0) from the
    device.  M is the SAME device function as the tile kernel's (contraction off, so the same bits): this pins the
    tile logic (ordering, ballots, word addressing, tile_jmax) and the scan, NOT the polygon arithmetic, which
    test_gpu_poly.py and test_gpu_reference_kernels.py pin."""
    from jdet_amd.ops.nms_poly import poly_nms_keep_mask
    thr = 0.1
    polys, _, order = _polys(n)
    hit = _device_hits(dev, polys[order], thr)
    keep_pos = R.greedy_keep(hit)
    ref = R.to_original(keep_pos, order)
    wit = R.wide_path_witnesses(keep_pos, hit, n)
    print("poly n %d thr %g: kept %d, witnesses %d" % (n, thr, int(ref.sum()), wit))
    assert wit >= 1 and 0 < ref.sum() < n
    got = poly_nms_keep_mask(_t(dev, polys), _t(dev, order), thr)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)
    np.testing.assert_array_equal(_poly(dev, polys, order, thr, 1), ref)


def test_polygon_level_layout(dev):
    """nine-column rows, labels [8400, 0, 1, 333], n_labels 1 and 4; reference as above with the label equality
    AND-ed into the device IoU decisions (same caveat: tile logic and scan, not the polygon arithmetic)"""
    n, thr = 8734, 0.1
    polys, scores, _ = _polys(n)
    labels = R.level_labels()
    visit = R.label_order(scores, labels)
    hit = _device_hits(dev, polys[visit], thr) & R.same_label(labels[visit])
    keep_pos = R.greedy_keep(hit)
    ref = R.to_original(keep_pos, visit)
    assert R.wide_path_witnesses(keep_pos, hit, n, R.wide_row_blocks(n, labels[visit], 4)) >= 1
    p9 = np.concatenate([polys, labels[:, None]], 1)
    for nl in (1, 4):
        np.testing.assert_array_equal(_poly(dev, p9, visit, thr, nl), ref)
    assert 0 < ref.sum() < n
