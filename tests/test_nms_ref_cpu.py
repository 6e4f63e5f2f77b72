"""The references of tests/nms_ref.py checked on the CPU, and the condition the GPU cases of
tests/test_gpu_nms_regimes.py rest on: every input that reaches the scan's fetch-after-resolve path holds boxes that
only that path can suppress (wide_path_witnesses >= 1), worked out from the references alone.  The counts are printed
(pytest -s)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import nms_ref as R

O.set_threads(8)


@pytest.mark.parametrize("thr,ge", [(0.1, 1), (0.5, 0), (0.0, 1), (0.0, 0), (1.0, 1)])
def test_greedy_keep_is_the_oracles_nms(thr, ge):
    """greedy_keep over the oracle's IoU matrix == the oracle's own NMS loop (both rules, thresholds 0 and 1)"""
    n = 2000
    dets, _, order, _ = R.rotated_case(n)
    s = dets[order]
    iou = O.box_iou_rotated(s, s)
    hit = (iou >= np.float32(thr)) if ge else (iou > np.float32(thr))
    keep = R.greedy_keep(hit)
    ref = O.nms_rotated_keep(dets, order, thr, cmp_ge=ge)
    print("n %d thr %g rule %s: kept %d" % (n, thr, ">=" if ge else ">", int(ref.sum())))
    np.testing.assert_array_equal(R.to_original(keep, order), ref)
    assert R.wide_path_witnesses(keep, hit, n) == 0           # 32 column blocks: no wide block


def test_greedy_keep_reads_the_upper_triangle_only():
    hit = np.zeros((5, 5), bool)
    hit[0, 2] = hit[2, 3] = hit[1, 4] = True
    hit[3, 0] = hit[4, 4] = True                              # lower triangle / diagonal: never read
    assert R.greedy_keep(hit).tolist() == [True, True, False, True, False]
    assert R.greedy_keep(np.zeros((0, 0), bool)).shape == (0,)


@pytest.mark.parametrize("thr", [0.6875, 0.5, 0.125, 0.0])
def test_horizontal_fp32_formula_takes_the_exact_decisions(thr):
    """the kernel's fp32 centre / size formula, restated in numpy fp32, decides every pair of the horizontal recipe as
    the exact rational comparison does; and the recipe reaches the wide path (witnesses >= 1)"""
    n = 8704
    boxes, _, order = R.hbb_case(n)
    s = boxes[order]
    exact = R.hbb_hits_exact(s, thr)
    np.testing.assert_array_equal(R.hbb_hits_fp32_kernel_formula(s, thr), exact)
    keep = R.greedy_keep(exact)
    wit = R.wide_path_witnesses(keep, exact, n)
    print("hbb n %d thr %g: kept %d, kept in the 7 wide blocks %d, witnesses %d"
          % (n, thr, int(keep.sum()), int(keep[:7 * 64].sum()), wit))
    assert 0 < keep.sum() < n and wit >= 1


def test_horizontal_recipe_is_asserted():
    boxes, _, _ = R.hbb_case(64)
    with pytest.raises(AssertionError):
        R.hbb_hits_exact(boxes, 0.7)                          # 7/10 is no dyadic threshold
    with pytest.raises(AssertionError):
        R.hbb_hits_exact(boxes + np.float32(0.5), 0.5)        # no integer corners
    odd = boxes.copy()
    odd[0, 2] += 1
    with pytest.raises(AssertionError):
        R.hbb_hits_exact(odd, 0.5)                            # odd width: the centre is no longer what fp32 halves


@pytest.mark.parametrize("n", [8257, 8704])
@pytest.mark.parametrize("thr", [0.6875, 0.125, 0.0])
def test_witnesses_horizontal_gpu_cases(n, thr):
    boxes, _, order = R.hbb_case(n)
    hit = R.hbb_hits_exact(boxes[order], thr)
    keep = R.greedy_keep(hit)
    wit = R.wide_path_witnesses(keep, hit, n)
    print("hbb n %d thr %g: kept %d, witnesses %d" % (n, thr, int(keep.sum()), wit))
    assert wit >= 1
    assert R.wide_path_witnesses(keep[:8256], hit[:8256, :8256], 8256) == 0     # 129 column blocks: all prefetch


ROTATED_WIDE_CASES = [(8257, 0.1, 1), (8321, 0.1, 1), (8704, 0.1, 1), (8704, 0.5, 0), (8321, 0.0, 1), (8321, 0.0, 0),
                      (8321, -0.5, 0)]


@pytest.mark.parametrize("n,thr,ge", ROTATED_WIDE_CASES)
def test_witnesses_rotated_gpu_cases(n, thr, ge):
    """rotated recipe; the same counts serve the polygon cases with the `>` rule (their polygons are these boxes'
    corners; the polygon test asserts its own count from its own hit matrix as well)"""
    dets, _, order, _ = R.rotated_case(n)
    keep = O.nms_rotated_keep(dets, order, thr, cmp_ge=ge)[order]
    hit = R.rotated_hits_of_kept_rows(dets[order], keep, thr, ge)
    np.testing.assert_array_equal(R.greedy_keep(hit), keep)   # the kept rows alone reproduce the greedy pass
    wit = R.wide_path_witnesses(keep, hit, n)
    print("rotated n %d thr %g rule %s: kept %d, witnesses %d" % (n, thr, ">=" if ge else ">", int(keep.sum()), wit))
    assert wit >= 1
    if thr == 0.0 and ge or thr < 0:
        assert keep.sum() == 1 and wit == n - 64              # box 0 removes everything; its own block is diagonal


def test_thresholds_of_one_and_above_keep_every_box():
    """(1.0, >=) and (1.5, >=) at n = 8321: no pair of the recipe has IoU 1, so nothing is suppressed and there is no
    witness to ask for: these cases pin that the wide path ORs nothing it should not"""
    dets, _, order, _ = R.rotated_case(8321)
    for thr in (1.0, 1.5):
        assert O.nms_rotated_keep(dets, order, thr, cmp_ge=1).all()


def test_which_blocks_are_wide():
    for n, wide in [(1, 0), (8256, 0), (8257, 1), (8321, 2), (8704, 7), (8734, 8)]:
        w = R.wide_row_blocks(n)
        assert w.sum() == wide and w[:wide].all()
    # 15 random labels visited label by label: the tiles are label-homogeneous, no row block reaches 129 blocks
    _, scores, _, labels = R.rotated_case(8704)
    assert R.wide_row_blocks(8704, labels[R.label_order(scores, labels)]).sum() == 0
    # the level layout: label 0 fills 131.25 blocks, its first three row blocks are wide in either scan
    lv = np.sort(R.level_labels())
    for nl in (1, 4):
        w = R.wide_row_blocks(8734, lv, nl)
        assert w.sum() == 3 and w[:3].all()


@pytest.mark.parametrize("kind", ["rotated", "horizontal"])
def test_witnesses_level_layout(kind):
    """n = 8734 with labels [8400, 0, 1, 333]: boxes of label 0 that only its three wide row blocks suppress"""
    n = 8734
    labels = R.level_labels()
    if kind == "rotated":
        dets, scores, _, _ = R.rotated_case(n)
        order = R.label_order(scores, labels)
        d6 = np.concatenate([dets, labels[:, None]], 1)
        keep = O.nms_rotated_keep(d6, order, 0.1, cmp_ge=1)[order]
        hit = R.rotated_hits_of_kept_rows(dets[order], keep, 0.1, 1, labels[order])
    else:
        boxes, scores, _ = R.hbb_case(n)
        order = R.label_order(scores, labels)
        hit = R.hbb_hits_exact(boxes[order], 0.5) & R.same_label(labels[order])
        keep = R.greedy_keep(hit)
    np.testing.assert_array_equal(R.greedy_keep(hit), keep)
    wit = R.wide_path_witnesses(keep, hit, n, R.wide_row_blocks(n, labels[order], 4))
    print("%s level layout: kept %d, witnesses %d" % (kind, int(keep.sum()), wit))
    assert wit >= 1
