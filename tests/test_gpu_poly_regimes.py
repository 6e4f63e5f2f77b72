"""GPU: every regime of the polygon IoU kernel and the polygon NMS decisions (csrc/poly_iou.hip) against the exact
rational evaluation of the same float32 inputs (oracle/poly_exact.py: vertical slabs, nothing in common with the
kernel's clipping and fans).  Regimes, storages and the exact values come from tests/poly_cases.py.

Tolerance, per pair: K * 2^-24 * R2 / max(U, floor) + 2^-23 with R2 (largest squared distance of the 8 vertices from
their mean) and U (union) from the reference, floor = 0.01 in mode 1 and the regime's smallest positive union in
mode 0.  K = 1471 is a count of roundings in the formulation, not a fit: per fan pair 72 in the clipping (one new
vertex for each of the two clip lines through the apex, two for the third; two signed distances of 3 or 7 roundings,
dc - dn, the quotient, and a difference, a product and a sum per coordinate) and 17 in the shoelace over at most 6
vertices (the two terms with the apex are exact zeros); 16 pairs; 15 additions of the pair areas; 2 x 15 for the two
polygon areas; 2 for the union.  tests/poly_cases.py has the table.  Every test prints the worst observed
error / (2^-24 * R2 / max(U, floor)) before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

from tests import nms_ref as R
from tests import poly_cases as PC

pytestmark = pytest.mark.gpu


def _t(dev, a, dtype=None):
    """device copy of a (possibly read-only, shared) host array"""
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(dev)


def _matrix(dev, a, b, mode):
    from jdet_amd.ops.nms_poly import poly_iou_matrix
    return poly_iou_matrix(_t(dev, a, np.float32), _t(dev, b, np.float32), mode).cpu().numpy().astype(np.float64)


def _raw_matrix(dev, a, b, mode):
    """jdet_poly_iou on rows of any stride, into a buffer filled with -7 that is 64 floats longer than needed"""
    from jdet_amd import _lib as L
    ta, tb = _t(dev, a, np.float32), _t(dev, b, np.float32)
    n1, n2 = ta.shape[0], tb.shape[0]
    out = torch.full((n1 * n2 + 64,), -7.0, dtype=torch.float32, device=dev)
    L.check(L.lib().jdet_poly_iou(L.ptr(ta), n1, ta.shape[1], L.ptr(tb), n2, tb.shape[1], int(mode), L.ptr(out),
                                  L.stream_ptr(ta)), "jdet_poly_iou")
    out = out.cpu().numpy()
    assert np.all(out[n1 * n2:] == -7.0), "the kernel wrote past n1 * n2"
    return out[:n1 * n2].reshape(n1, n2)


def _nms(dev, polys, order, thr, n_labels):
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
    k = keep.cpu().numpy()
    assert set(np.unique(k)) <= {0, 1}, "the scan left flags unwritten (7) or wrote something else"
    return k.astype(bool)


@functools.lru_cache(maxsize=None)
def _device_values(dev, name, mode):
    """(m, 128) device IoU of every base pair of the regime: 8 x 8 storages as (a, b), then the same as (b, a).
    One launch per order over all storages of all pairs; the pair's own 8 x 8 block is cut out of the matrix."""
    A, B, _ = PC.pairs(name)
    m = len(A)
    va = np.concatenate([PC.variants(p) for p in A])
    vb = np.concatenate([PC.variants(q) for q in B])
    k = np.arange(m)
    ab = _matrix(dev, va, vb, mode).reshape(m, 8, m, 8)[k, :, k, :].reshape(m, 64)
    ba = _matrix(dev, vb, va, mode).reshape(m, 8, m, 8)[k, :, k, :].reshape(m, 64)
    out = np.concatenate([ab, ba], 1)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("name", list(PC.REGIMES))
def test_regime_vs_exact(dev, name):
    """both modes, every storage (two windings x four relabelings of each polygon) and both pair orders, at the origin
    and at (4000, 2000), against the exact value of the same float32 numbers"""
    ref = PC.reference(name)
    for mode, want, tol, unit in ((0, ref.iou0, ref.tol0, ref.unit0), (1, ref.iou1, ref.tol1, ref.unit1)):
        got = _device_values(dev, name, mode)
        err = np.abs(got - want[:, None]).max(1)
        err[~np.isfinite(got).all(1)] = np.inf
        units = np.where(unit > 0, err / np.where(unit > 0, unit, 1), 0.0)
        print("%-22s mode %d: %3d pairs, worst error %.3g, worst error / (2^-24 R2 / U) %.3g (K = %d)"
              % (name, mode, len(want), err.max(), units.max(), PC.K))
        bad = np.flatnonzero(~(err <= tol))
        assert bad.size == 0, "pairs %s: errors %s above %s (exact %s)" % (bad[:5], err[bad[:5]], tol[bad[:5]],
                                                                             want[bad[:5]])


@pytest.mark.parametrize("name", list(PC.REGIMES))
def test_regime_invariances(dev, name):
    """iou(a, b) against iou(b, a), either winding, every cyclic relabeling: no two of the 128 device values of a
    pair differ by more than the pair's tolerance"""
    ref = PC.reference(name)
    for mode, tol in ((0, ref.tol0), (1, ref.tol1)):
        got = _device_values(dev, name, mode)
        order = np.abs(got[:, :64].reshape(-1, 8, 8) - got[:, 64:].reshape(-1, 8, 8)).max((1, 2))
        spread = got.max(1) - got.min(1)
        print("%-22s mode %d: worst |iou(a,b) - iou(b,a)| / tol %.3g, worst spread over storages / tol %.3g"
              % (name, mode, (order / tol).max(), (spread / tol).max()))
        assert np.all(order <= tol) and np.all(spread <= tol)


TRANSLATIONS = ((256.0, 0.0), (1024.0, 768.0), (4096.0, 4096.0), (-4096.0, 2048.0), (3840.0, -256.0))


@pytest.mark.parametrize("name", ["integer_snapped", "integer_snapped_dart", "fan_centre", "vertex_on_edge",
                                  "zero_area_self"])
def test_translation_by_exact_vectors(dev, name):
    """multiples of 256 up to 4096 added to integer coordinates: the sums are exact in float32, so the translated pair
    IS the same pair elsewhere and its exact value and tolerance are those of the original"""
    A, B, off = PC.pairs(name)
    sel = np.flatnonzero(off == 0)
    ref = PC.reference(name)
    a0, b0 = A[sel], B[sel]
    assert np.all(a0 == np.round(a0)) and np.all(b0 == np.round(b0))
    k = np.arange(len(sel))
    for mode, want, tol in ((0, ref.iou0[sel], ref.tol0[sel]), (1, ref.iou1[sel], ref.tol1[sel])):
        base = _matrix(dev, a0, b0, mode)[k, k]
        worst = 0.0
        for t in TRANSLATIONS:
            tv = np.tile(np.array(t, np.float32), 4)
            a, b = a0 + tv, b0 + tv
            assert a.dtype == np.float32 and np.all(a - tv == a0) and np.all(b - tv == b0)
            got = _matrix(dev, a, b, mode)[k, k]
            worst = max(worst, float((np.abs(got - want) / tol).max()))
            assert np.all(np.abs(got - want) <= tol) and np.all(np.abs(got - base) <= tol)
        print("%-22s mode %d: worst error / tol over %d translations %.3g" % (name, mode, len(TRANSLATIONS), worst))


@pytest.mark.parametrize("n1,n2", [(1, 1), (1, 255), (255, 1), (3, 85), (16, 16), (1, 257), (257, 1), (257, 259)])
@pytest.mark.parametrize("stride", [8, 9, 11])
def test_launch_geometry(dev, n1, n2, stride):
    """n1 * n2 = 1, 255, 256, 257 and 66563 (above 64 k, no multiple of the block); single rows and columns; n2 = 85
    and 259 for the t / n2, t % n2 split; rows of 8, 9 and 11 floats whose trailing columns are NaN.  Row i is polygon
    a[i % m] and column j polygon b[j % m] of the random convex regime, so every entry has to equal, bit for bit, the
    entry of the m x m launch, whose diagonal test_regime_vs_exact holds to the exact values -- checked here again
    for the entries with i % m == j % m."""
    A, B, _ = PC.pairs("random_convex")
    ref = PC.reference("random_convex")
    m = len(A)
    canon = _device_values_canon(dev)
    i, j = np.arange(n1) % m, np.arange(n2) % m
    rows = np.full((n1, stride), np.nan, np.float32)
    cols = np.full((n2, stride), np.nan, np.float32)
    rows[:, :8], cols[:, :8] = A[i], B[j]
    for mode in (0, 1):
        got = _raw_matrix(dev, rows, cols, mode)
        assert np.array_equal(got, canon[mode][np.ix_(i, j)])
        ii, jj = np.nonzero(i[:, None] == j[None, :])
        want, tol = (ref.iou0, ref.tol0) if mode == 0 else (ref.iou1, ref.tol1)
        assert np.all(np.abs(got[ii, jj].astype(np.float64) - want[i[ii]]) <= tol[i[ii]])


@functools.lru_cache(maxsize=None)
def _device_values_canon(dev):
    A, B, _ = PC.pairs("random_convex")
    return tuple(_raw_matrix(dev, A, B, mode) for mode in (0, 1))


def _orders(scores, labels):
    return R.score_order(scores), R.label_order(scores, labels)


@pytest.mark.parametrize("thr", PC.NMS_THRESHOLDS)
def test_nms_decisions_on_contact_heavy_set(dev, thr):
    """tiling, duplicates, half-overlaps, darts, near-identical copies, random simple quads, every third clockwise:
    jdet_nms_poly keeps exactly what the greedy scan over the EXACT mode-0 IoU keeps -- eight-float rows, nine-float
    rows with one scan, nine-float rows label by label.  Polygons with a partner whose exact IoU is within 2 x tol of
    the threshold are left out (tests/test_poly_exact_cpu.py: at most 5 %)."""
    polys, scores, labels = PC.nms_set()
    ref = PC.nms_reference()
    use = ~PC.nms_near(thr)
    print("thr %.2f: %d of %d polygons left out for a partner within 2 x tol (%.1f %%)"
          % (thr, (~use).sum(), len(use), 100.0 * (~use).mean()))
    assert (~use).mean() <= 0.05
    p, s, l = polys[use], scores[use], labels[use]
    iou = ref.iou[np.ix_(use, use)]
    by_score, by_label = _orders(s, l)
    want = PC.greedy(iou, s, thr)
    want_l = PC.greedy(iou, s, thr, l)
    assert 30 < want.sum() < want_l.sum() < len(p) - 30
    np.testing.assert_array_equal(_nms(dev, p, by_score, thr, 1), want)
    p9 = np.concatenate([p, l[:, None].astype(np.float32)], 1)
    np.testing.assert_array_equal(_nms(dev, p9, by_label, thr, 1), want_l)
    np.testing.assert_array_equal(_nms(dev, p9, by_label, thr, PC.NMS_LABELS), want_l)
    one = np.concatenate([p, np.zeros((len(p), 1), np.float32)], 1)              # nine floats, a single label
    np.testing.assert_array_equal(_nms(dev, one, by_score, thr, 1), want)


def test_nms_duplicates_suppress_below_one_minus_tol(dev):
    """pairs of exact IoU 1: the device value is above 1 - tol, so they suppress at every threshold below that; and
    the scan at 1 - 2 tol keeps one polygon of every set of exact duplicates"""
    polys, scores, _ = PC.nms_set()
    ref = PC.nms_reference()
    dup = (ref.iou == 1) & ~np.eye(len(polys), dtype=bool)
    ii, jj = np.nonzero(dup)
    assert len(ii) >= 20
    got = _matrix(dev, polys, polys, 0)
    assert np.all(got[ii, jj] > 1 - ref.tol[ii, jj])
    sel = np.flatnonzero(dup.any(1))
    thr = float(1 - 2 * ref.tol[ii, jj].max())
    keep = _nms(dev, polys[sel], R.score_order(scores[sel]), thr, 1)
    np.testing.assert_array_equal(keep, PC.greedy(ref.iou[np.ix_(sel, sel)], scores[sel], thr))
    assert keep.sum() <= len(sel) // 2


def test_non_finite_rows(dev):
    """one polygon with a NaN coordinate, one with an Inf coordinate: no fault, the finite polygons' keep decisions and
    the finite pairs' matrix entries are those of the run without the two rows.
    OBSERVED for the two rows themselves (pinned, not required by any reference): their mode-0 IoU with every polygon,
    themselves included, is NaN (the mean of the 8 vertices is not finite, so no area is), which never exceeds a
    threshold -- they are kept and suppress nothing; in mode 1 fmaxf(NaN, 0.01) is 0.01 and the IoU is 0."""
    polys, scores, labels = PC.nms_set()
    thr = PC.NMS_THRESHOLDS[0]
    n = len(polys)
    bad = np.stack([polys[3], polys[40]]).copy()
    bad[0, 5], bad[1, 2] = np.nan, np.inf
    p = np.concatenate([polys[:100], bad[:1], polys[100:], bad[1:]])
    s = np.concatenate([scores[:100], [np.float32(0.5001)], scores[100:], [np.float32(0.9999)]]).astype(np.float32)
    finite = np.ones(n + 2, bool)
    finite[[100, n + 1]] = False
    base = _nms(dev, polys, R.score_order(scores), thr, 1)
    keep = _nms(dev, p, R.score_order(s), thr, 1)
    np.testing.assert_array_equal(keep[finite], base)
    assert keep[100] and keep[n + 1]
    lab = np.concatenate([labels[:100], labels[3:4], labels[100:], labels[40:41]])
    p9 = np.concatenate([p, lab[:, None].astype(np.float32)], 1)
    base9 = _nms(dev, np.concatenate([polys, labels[:, None].astype(np.float32)], 1), R.label_order(scores, labels),
                 thr, PC.NMS_LABELS)
    keep9 = _nms(dev, p9, R.label_order(s, lab), thr, PC.NMS_LABELS)
    np.testing.assert_array_equal(keep9[finite], base9)
    assert keep9[100] and keep9[n + 1]
    for mode in (0, 1):
        m0 = _raw_matrix(dev, polys, polys, mode)
        m1 = _raw_matrix(dev, p, p, mode)
        assert np.array_equal(m1[np.ix_(finite, finite)], m0) and np.all(np.isfinite(m0))
        for what, k in (("NaN", 100), ("Inf", n + 1)):
            rows = np.concatenate([m1[k], m1[:, k]])
            print("mode %d, row and column of the %s polygon: values %s" % (mode, what, np.unique(rows)))
            assert np.all(np.isnan(rows)) if mode == 0 else np.all(rows == 0)
