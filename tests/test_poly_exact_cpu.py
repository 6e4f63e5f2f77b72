"""CPU: the exact polygon overlap (oracle/poly_exact.py, vertical slabs in rational arithmetic) against closed forms,
the conditions the regime table (tests/poly_cases.py) has to meet -- from the reference alone, no kernel --, and the
float64 restatement oracle/poly_oracle.py against the exact evaluation."""
from fractions import Fraction as Fr

import numpy as np
import pytest

from oracle import poly_exact as PX
from oracle import poly_oracle as PO
from tests import poly_cases as PC

SQ = np.array([0, 0, 2, 0, 2, 2, 0, 2], np.float32)
OFF = np.tile([4000.0, 2000.0], 4).astype(np.float32)


@pytest.mark.parametrize("off", [0.0, OFF], ids=["origin", "offset"])
def test_closed_forms_are_exact_fractions(off):
    sq = SQ + off
    assert PX.area(sq) == 4 and PX.intersection(sq, sq) == 4
    assert PX.iou(sq, sq, 0) == 1 and PX.iou(sq, sq, 1) == 1
    assert PX.iou(sq, sq + np.tile([1, 0], 4).astype(np.float32)) == Fr(1, 3)            # shifted by half its width
    assert PX.iou(sq, sq + 5) == 0 and PX.iou(sq, sq + np.tile([2, 0], 4).astype(np.float32)) == 0
    diamond = np.array([1, 0, 2, 1, 1, 2, 0, 1], np.float32) + off
    assert PX.intersection(sq, diamond) == 2 and PX.iou(sq, diamond) == Fr(1, 2)
    inner = np.array([0.5, 0.5, 1.5, 0.5, 1.5, 1.5, 0.5, 1.5], np.float32) + off
    assert PX.iou(sq, inner) == Fr(1, 4) and PX.iou(inner, sq, 0) == PX.area(inner) / PX.area(sq)
    # a chevron (area 4) against the band 0 <= y <= 1: two prongs, by hand 2 * (1/2 * (2 - 2/3) * 1) = 4/3
    chevron = np.array([0, 0, 2, 1, 4, 0, 2, 3], np.float32) + off
    strip = np.array([0, 0, 4, 0, 4, 1, 0, 1], np.float32) + off
    assert PX.area(chevron) == 4 and PX.intersection(chevron, strip) == Fr(4, 3)
    # degenerate rules
    point = np.zeros(8, np.float32) + off
    assert PX.iou(point, point, 0) == 1 and PX.iou(point, point, 1) == 0 and PX.iou(point, sq, 0) == 0
    small = (SQ * np.float32(1.0 / 64)) + off                                             # area 1/1024 < 0.01
    assert PX.iou(small, small, 1) == Fr(1, 1024) / Fr(1, 100) and PX.iou(small, small, 0) == 1
    r2, u = PX.scale(sq, sq + np.tile([2, 0], 4).astype(np.float32))
    assert (r2, u) == (5, 8)


def test_is_simple():
    assert PX.is_simple(SQ) and PX.is_simple(PC.DART.reshape(8))
    assert not PX.is_simple(np.array([0, 0, 2, 2, 2, 0, 0, 2], np.float32))               # bow-tie
    assert PX.is_simple(np.array([0, 0, 2, 0, 2, 0, 1, 2], np.float32))                   # triangle stored as a quad
    assert not PX.is_simple(PC.LINE_D.reshape(8)) and not PX.is_simple(PC.POINT.reshape(8))
    assert not PX.is_simple(np.array([0, 0, 4, 0, 2, 0, 2, 3], np.float32))               # an edge folded back


def test_storage_does_not_change_the_exact_value():
    """what lets the GPU tests hold all 8 x 8 storages of a pair to one reference value"""
    for name in ("darts", "vertex_on_edge", "triangle_as_quad", "random_dart_dart"):
        A, B, _ = PC.pairs(name)
        for k in range(0, len(A), 3):
            want = PX.intersection(A[k], B[k])
            va, vb = PC.variants(A[k]), PC.variants(B[k])
            assert np.array_equal(va[0], A[k]) and np.array_equal(va[4].reshape(4, 2), A[k].reshape(4, 2)[::-1])
            for v in va:
                assert sorted(map(tuple, v.reshape(4, 2))) == sorted(map(tuple, A[k].reshape(4, 2)))
            for i, j in ((1, 6), (5, 2), (7, 7)):
                assert PX.intersection(va[i], vb[j]) == want == PX.intersection(vb[j], va[i])
                assert PX.scale(va[i], vb[j]) == PX.scale(A[k], B[k])


def test_regime_table_conditions():
    total = 0
    for name, reg in PC.REGIMES.items():
        A, B, off = PC.pairs(name)
        assert len(A) > 0 and set(off) == {0, 1}, name
        assert A.dtype == np.float32 and B.dtype == np.float32
        total += len(A)
        if not reg.zero_area:
            assert all(PX.is_simple(p) for p in A) and all(PX.is_simple(p) for p in B), name
        ref = PC.reference(name)
        if reg.quota:
            share = float((ref.iou1 > 0.05).mean())
            print("%-22s pairs %3d, exact IoU > 0.05 in %.0f %%" % (name, len(A), 100 * share))
            assert share >= 0.25, name
    slabs = PC.nms_reference().slabs
    print("regime pairs %d + NMS slab evaluations %d" % (total, slabs))
    assert total + slabs <= PC.MAX_EXACT_PAIRS


def test_regimes_hold_what_their_names_say():
    r = {name: PC.reference(name) for name in PC.REGIMES}
    assert np.all(r["identical"].iou0 == 1) and np.all(r["identical"].iou1 == 1)
    for name in ("shared_edge", "half_shared_edge", "corner_touch"):
        assert np.all(r[name].iou0 < 1e-6), name            # 0 at the origin, float32 rounding of b elsewhere
    assert r["collinear_overlap"].exact[0][0] == 4 and r["collinear_overlap"].iou0[0] == 0.5
    assert np.all(r["zero_area_vs_square"].iou0 == 0)
    assert np.all(r["zero_area_self"].iou0 == 1) and np.all(r["zero_area_self"].iou1 == 0)
    assert np.all(r["tiny"].union < 0.01) and np.all(r["tiny"].iou0 > 10 * r["tiny"].iou1)
    assert np.all(r["near_identical"].iou0 > 0.99) and np.all(r["near_identical"].iou0 < 1)
    assert np.all(r["small_in_big"].iou0 > 0) and np.all(r["small_in_big"].iou0 < 2e-4)
    # fan centre: the mean of the 8 vertices is a vertex of a / lies on an edge of a, exactly
    A, B, _ = PC.pairs("fan_centre")
    for k in (0, 1):
        pts = PX.points(A[k]) + PX.points(B[k])
        mean = (sum(p[0] for p in pts) / 8, sum(p[1] for p in pts) / 8)
        a = PX.points(A[k])
        assert mean in a if k == 0 else (mean not in a and any(
            PX._cross(a[i], a[(i + 1) % 4], mean) == 0 and PX._on_segment(a[i], a[(i + 1) % 4], mean)
            for i in range(4)))


def test_float64_restatement_against_exact():
    """oracle/poly_oracle.py on the simple general-position regimes, both sides on the same float64 numbers.
    Tolerance: the module's rounding count K with float64's unit roundoff 2^-53 -- and, because the restatement's
    convex route clips the coordinates as they are (no centring), with X2 = the largest squared distance of a
    vertex from the coordinate origin in place of R2."""
    worst = 0.0
    for name, reg in PC.REGIMES.items():
        if not reg.general:
            continue
        A, B, _ = PC.pairs(name)
        ref = PC.reference(name)
        for k in range(len(A)):
            a, b = A[k].astype(np.float64), B[k].astype(np.float64)
            x2 = max(float(np.max(np.sum(a.reshape(4, 2) ** 2, 1))), float(np.max(np.sum(b.reshape(4, 2) ** 2, 1))))
            for mode, want in ((0, ref.iou0[k]), (1, ref.iou1[k])):
                tol = PC.K * 2.0 ** -53 * x2 / max(ref.union[k], 0.01) + 2.0 ** -52
                err = abs(PO.poly_iou(a, b, mode) - want)
                worst = max(worst, err / tol)
                assert err <= tol, (name, k, mode, err, tol)
    print("poly_oracle vs exact: worst error / tolerance %.3g" % worst)


def test_nms_set_and_thresholds():
    """from the reference alone: at most 5 % of the polygons have a partner within 2 x tol of a threshold, exact
    duplicates are in the set, and both thresholds leave something to suppress and something to keep"""
    polys, scores, labels = PC.nms_set()
    ref = PC.nms_reference()
    n = len(polys)
    assert 200 <= n <= 300 and len(np.unique(scores)) == n
    area2 = [np.sum(p.reshape(4, 2)[:, 0].astype(np.float64) * np.roll(p.reshape(4, 2)[:, 1], -1)
                    - p.reshape(4, 2)[:, 1].astype(np.float64) * np.roll(p.reshape(4, 2)[:, 0], -1)) for p in polys]
    assert all((a < 0) == (k % 3 == 0) for k, a in enumerate(area2))                     # every third clockwise
    assert all(PX.is_simple(p) for p in polys)
    off_diag = ref.iou[~np.eye(n, dtype=bool)]
    assert (off_diag == 1).sum() >= 20                                                    # exact duplicates
    for thr in PC.NMS_THRESHOLDS:
        near = PC.nms_near(thr)
        print("thr %.2f: %d of %d polygons (%.1f %%) have a partner within 2 x tol" % (thr, near.sum(), n,
                                                                                       100.0 * near.mean()))
        assert near.mean() <= 0.05
        assert thr < 1 - ref.tol[ref.iou == 1].max()        # duplicates at IoU 1 suppress at this threshold
        for lab in (None, labels):
            keep = PC.greedy(ref.iou, scores, thr, lab, alive=~near)
            print("    kept %d of %d%s" % (keep.sum(), (~near).sum(), "" if lab is None else " (label by label)"))
            assert 30 < keep.sum() < (~near).sum() - 30
    k1 = PC.greedy(ref.iou, scores, PC.NMS_THRESHOLDS[0]).sum()
    k2 = PC.greedy(ref.iou, scores, PC.NMS_THRESHOLDS[1]).sum()
    assert k1 < k2                                          # the two thresholds decide differently
