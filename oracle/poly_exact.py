"""Exact polygon overlap by vertical slabs.  TEST INFRASTRUCTURE ONLY (never imported by jdet_amd).

Area of the intersection of two simple 4-point polygons in exact rational arithmetic (fractions.Fraction; every
binary float converts exactly), by a method that shares nothing with the clipping and fan-triangle formulation of
csrc/poly_iou.hip and oracle/poly_oracle.py:

  * cut the x axis at every vertex abscissa and at the abscissa of every point where an edge of P meets a
    non-parallel edge of Q (parallel edges that overlap begin and end at vertices, which are cuts already);
  * inside a slab no two edges cross, so the order of all edge ordinates is the same on every vertical line of the
    slab; the cross-section of a polygon on the slab's mid line is a set of intervals by the even-odd rule over the
    edges whose open x-range contains the mid abscissa, and the length common to both sets is linear across the slab;
  * the area is therefore sum(slab width x common length on the mid line), exactly.

No orientation, no vertex order beyond "consecutive points are joined", no sign test on a cross product decides what
is inside: the result is the same for either winding and for every cyclic relabeling by construction.

A vertex repeated in consecutive positions (a triangle stored as a quad) is an edge of length zero and is dropped
before `is_simple` looks at the polygon; the slabs never see such an edge (its open x-range is empty).
"""
from fractions import Fraction

import numpy as np

__all__ = ["points", "is_simple", "area", "intersection", "iou", "iou_matrix", "scale"]

_ZERO = Fraction(0)


def points(p):
    """8 numbers (any float type) -> four exact (x, y)"""
    v = np.asarray(p).reshape(8)
    return [(Fraction(float(v[2 * i])), Fraction(float(v[2 * i + 1]))) for i in range(4)]


def _edges(pts):
    n = len(pts)
    return [(pts[i], pts[(i + 1) % n]) for i in range(n)]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _on_segment(a, b, c):
    """c on the closed segment a-b, given the three are collinear"""
    return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])


def _segments_meet(a, b, c, d):
    """closed segments a-b and c-d share at least one point"""
    d1, d2, d3, d4 = _cross(c, d, a), _cross(c, d, b), _cross(a, b, c), _cross(a, b, d)
    if ((d1 > 0 and d2 < 0) or (d1 < 0 and d2 > 0)) and ((d3 > 0 and d4 < 0) or (d3 < 0 and d4 > 0)):
        return True
    return ((d1 == 0 and _on_segment(c, d, a)) or (d2 == 0 and _on_segment(c, d, b))
            or (d3 == 0 and _on_segment(a, b, c)) or (d4 == 0 and _on_segment(a, b, d)))


def is_simple(p):
    """no two non-adjacent edges meet, adjacent edges meet in their common vertex only, and the area is not zero.
    Consecutive repeated vertices are merged first, so a triangle stored as a quad is simple."""
    pts = points(p)
    red = [v for i, v in enumerate(pts) if v != pts[i - 1]]
    if len(red) < 3 or area(p) == 0:
        return False
    e = _edges(red)
    n = len(e)
    for i in range(n):
        a, b = e[i]
        c, d = e[(i + 1) % n]                       # adjacent: b == c; they may not fold back onto each other
        if _cross(a, b, d) == 0 and (d[0] - b[0]) * (a[0] - b[0]) + (d[1] - b[1]) * (a[1] - b[1]) > 0:
            return False
        for j in range(i + 2, n):
            if (j + 1) % n == i:
                continue
            if _segments_meet(a, b, *e[j]):
                return False
    return True


def area(p):
    """|shoelace| / 2: the area of a simple polygon (0 for four collinear points)"""
    pts = points(p)
    s = sum(pts[i][0] * pts[(i + 1) % 4][1] - pts[i][1] * pts[(i + 1) % 4][0] for i in range(4))
    return abs(s) / 2


def _meeting_abscissa(a, b, c, d):
    """x of the point where segment a-b meets the non-parallel segment c-d, or None"""
    rx, ry = b[0] - a[0], b[1] - a[1]
    sx, sy = d[0] - c[0], d[1] - c[1]
    den = rx * sy - ry * sx
    if den == 0:
        return None
    qx, qy = c[0] - a[0], c[1] - a[1]
    t = (qx * sy - qy * sx) / den
    u = (qx * ry - qy * rx) / den
    if 0 <= t <= 1 and 0 <= u <= 1:
        return a[0] + t * rx
    return None


def _section(edges, xm):
    """sorted ordinates at which the vertical line x = xm crosses the edges whose open x-range contains xm;
    consecutive pairs are the inside intervals (even-odd rule)"""
    ys = []
    for a, b in edges:
        if min(a[0], b[0]) < xm < max(a[0], b[0]):
            ys.append(a[1] + (b[1] - a[1]) * (xm - a[0]) / (b[0] - a[0]))
    ys.sort()
    assert len(ys) % 2 == 0                        # a closed curve crosses a line that avoids its vertices evenly
    return ys


def _common(ys1, ys2):
    tot = _ZERO
    for i in range(0, len(ys1), 2):
        for j in range(0, len(ys2), 2):
            lo, hi = max(ys1[i], ys2[j]), min(ys1[i + 1], ys2[j + 1])
            if hi > lo:
                tot += hi - lo
    return tot


def intersection(p, q):
    """exact area of the intersection of two simple 4-point polygons"""
    P, Q = points(p), points(q)
    if (max(v[0] for v in P) <= min(v[0] for v in Q) or max(v[0] for v in Q) <= min(v[0] for v in P)
            or max(v[1] for v in P) <= min(v[1] for v in Q) or max(v[1] for v in Q) <= min(v[1] for v in P)):
        return _ZERO                               # the bounding boxes share no interior point
    ep, eq = _edges(P), _edges(Q)
    cuts = {v[0] for v in P} | {v[0] for v in Q}
    for a, b in ep:
        for c, d in eq:
            x = _meeting_abscissa(a, b, c, d)
            if x is not None:
                cuts.add(x)
    cuts = sorted(cuts)
    tot = _ZERO
    for x0, x1 in zip(cuts[:-1], cuts[1:]):
        xm = (x0 + x1) / 2
        ys1 = _section(ep, xm)
        if not ys1:
            continue
        ys2 = _section(eq, xm)
        if ys2:
            tot += (x1 - x0) * _common(ys1, ys2)
    return tot


def _union(p, q, inter=None):
    return area(p) + area(q) - (intersection(p, q) if inter is None else inter)


def iou(p, q, mode=1):
    """the two degenerate rules of the kernel: mode 0 gives 1 when the union is exactly 0, else inter / union;
    mode 1 gives inter / max(union, 0.01)"""
    inter = intersection(p, q)
    union = _union(p, q, inter)
    if mode == 1:
        return inter / max(union, Fraction(1, 100))
    return Fraction(1) if union == 0 else inter / union


def iou_matrix(ps, qs, mode=1):
    """(n1, 8) x (n2, 8) -> (n1, n2) object array of Fractions"""
    ps, qs = np.asarray(ps).reshape(-1, 8), np.asarray(qs).reshape(-1, 8)
    out = np.empty((len(ps), len(qs)), object)
    for i, p in enumerate(ps):
        for j, q in enumerate(qs):
            out[i, j] = iou(p, q, mode)
    return out


def scale_r2(p, q):
    """the largest squared distance of the 8 vertices from their mean"""
    v = points(p) + points(q)
    mx, my = sum(a[0] for a in v) / 8, sum(a[1] for a in v) / 8
    return max((a[0] - mx) ** 2 + (a[1] - my) ** 2 for a in v)


def scale(p, q):
    """(R2, U): the largest squared distance of the 8 vertices from their mean, and the exact union"""
    return scale_r2(p, q), _union(p, q)
