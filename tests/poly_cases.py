"""Regime table of the polygon IoU / polygon NMS tests (csrc/poly_iou.hip).  No kernel calls; importable without a GPU.

Every regime is a named generator of float32 pairs (a, b), produced at the offsets OFFSETS.  `variants` gives the 8
storages of one polygon (two windings x four cyclic relabelings); the exact area does not depend on the storage (the
slab method never reads it, tests/test_poly_exact_cpu.py checks it), so `reference(name)` evaluates every base pair
once and the GPU tests hold all 8 x 8 storages and both pair orders to that one value.

TOLERANCE.  tol = K * 2^-24 * R2 / max(U, floor) + 2^-23 per pair, R2 = largest squared distance of the 8 vertices
from their mean, U = exact union, floor = 0.01 in mode 1 and the smallest positive union of the regime in mode 0.
The kernel subtracts the mean of the 8 vertices first (for coordinates up to a few thousand the subtraction itself is
exact), so every coordinate it then works on is at most R = sqrt(R2) and every product or cross product at most R2.
First-order model: a rounding of a quantity bounded by R2, or of a vertex coordinate (bounded by R, and a vertex
moved by d changes an area by at most R * d), moves the intersection area by at most one unit 2^-24 * R2.  K is the
number of such roundings in the formulation, counted from the source, not fitted to any run:

  per fan pair (0, a, b) x (0, c, d)
    clipping: the apex 0 lies on the first and third clip lines, so each of those creates at most one vertex; the
    line c -> d at most two.  A new vertex costs the two signed distances (3 roundings each for a line through the
    apex -- the subtractions of 0 are exact --, 7 each otherwise), dc - dn, the quotient, and a difference, a product
    and a sum per coordinate:           (2*3 + 8) + 2 * (2*7 + 8) + (2*3 + 8)                            =   72
    shoelace over at most 6 vertices: the two terms that contain the apex are exact zeros; 4 terms of two products
    and a difference, and 5 additions                                              4*3 + 5                 =   17
                                                                                                  per pair:  89
  16 fan pairs                                                                                   16 * 89   = 1424
  adding the 16 pair areas                                                                                 =   15
  the two polygon areas: 4 terms of 3 roundings and 3 additions, each                            2 * 15    =   30
  union = a1 + a2 - inter                                                                                  =    2
                                                                                                        K  = 1471

The final quotient is one rounding of a value at most 1 (2^-24) and the reference's own conversion to float64 is
far below that; 2^-23 covers both.  K is a worst-case count: independent roundings do not all push the same way, and
an observed error far below K units is what a correct kernel is expected to show.
"""
import functools
import math
from fractions import Fraction
from types import SimpleNamespace as NS

import numpy as np

from oracle import poly_exact as PX

F = np.float32
OFFSETS = ((0.0, 0.0), (4000.0, 2000.0))
K = 16 * (72 + 17) + 15 + 2 * 15 + 2            # 1471, see the module docstring
U24 = 2.0 ** -24
MAX_EXACT_PAIRS = 3000                          # slab evaluations of the whole GPU module (regimes + NMS set)


def tolerance(r2, union, floor):
    """per-pair bound on |device IoU - exact IoU|, arrays or scalars (float64)"""
    return K * U24 * np.asarray(r2, np.float64) / np.maximum(np.asarray(union, np.float64), floor) + 2.0 ** -23


def unit(r2, union, floor):
    """2^-24 * R2 / max(U, floor): the unit the observed errors are reported in"""
    return U24 * np.asarray(r2, np.float64) / np.maximum(np.asarray(union, np.float64), floor)


# ---------------------------------------------------------------------------------------------- building blocks
def variants(p):
    """(8,) -> (8, 8): rows 0-3 the four cyclic relabelings, rows 4-7 the same of the reversed winding"""
    q = np.asarray(p).reshape(4, 2)
    out = [np.roll(w, -s, axis=0).reshape(8) for w in (q, q[::-1]) for s in range(4)]
    return np.stack(out).astype(np.asarray(p).dtype)


def _place(poly, off):
    """float64 (4, 2) or (8,) at the origin -> float32 (8,) at the offset (one rounding per coordinate)"""
    return (np.asarray(poly, np.float64).reshape(4, 2) + np.asarray(off, np.float64)).astype(F).reshape(8)


def _rot(poly, ang, about=(0.0, 0.0)):
    p = np.asarray(poly, np.float64).reshape(4, 2) - about
    c, s = math.cos(ang), math.sin(ang)
    return p @ np.array([[c, s], [-s, c]]) + about


def _rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)


def _box(cx, cy, w, h, ang):
    return _rot(_rect(-w / 2, -h / 2, w / 2, h / 2), ang) + (cx, cy)


def _convex(p):
    p = np.asarray(p, np.float64).reshape(4, 2)
    s = [(p[(i + 1) % 4, 0] - p[i, 0]) * (p[(i + 2) % 4, 1] - p[(i + 1) % 4, 1])
         - (p[(i + 1) % 4, 1] - p[i, 1]) * (p[(i + 2) % 4, 0] - p[(i + 1) % 4, 0]) for i in range(4)]
    return all(v >= 0 for v in s) or all(v <= 0 for v in s)


def _usable(p32):
    """simple with an area above 1 as float32 numbers"""
    return PX.is_simple(p32) and PX.area(p32) > 1


def random_quad(rng, centre, dart, off, snap=False, rmin=4.0, rmax=30.0):
    """vertices at sorted random angles about the centre; dart: one of them pulled to 0.3 of its radius and the
    result kept only when it is not convex.  Always filtered to simple float32 polygons: a self-intersecting
    quadrilateral has no area to compare against."""
    while True:
        ang = np.sort(rng.uniform(0, 2 * math.pi, 4))
        r = rng.uniform(rmin, rmax, 4)
        if dart:
            r[2] *= 0.3
        q = np.asarray(centre) + np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
        if snap:
            q = np.round(q)
        if _convex(q) == dart:
            continue
        p = _place(q, off)
        if _usable(p):
            return p


# ------------------------------------------------------------------------------------------------------ regimes
SHAPES = (0.0, 0.3, math.pi / 4)
DART = np.array([[0, 0], [10, 4], [20, 0], [10, 20]], np.float64)          # reflex vertex (10, 4), area 160
LINE_D = np.array([[0, 0], [4, 4], [8, 8], [12, 12]], np.float64)
LINE_H = np.array([[0, 5], [4, 5], [8, 5], [12, 5]], np.float64)
POINT = np.array([[5, 5]] * 4, np.float64)


def _identical(off):
    out = [_place(_rot(_rect(0, 0, 30, 12), t, (15, 6)), off) for t in SHAPES]
    out += [_place(DART, off), _place([[0, 0], [25, 3], [31, 22], [-4, 17]], off)]
    return [(p, p.copy()) for p in out]


def _parallelograms(off):
    out = [_place(_rot(_rect(0, 0, 30, 12), t, (15, 6)), off) for t in SHAPES]
    return out + [_place([[0, 0], [30, 5], [37, 19], [7, 14]], off)]


def _shared_edge(off):
    """b = a + (a's own edge vector), all in float32: the neighbour across an edge"""
    out = []
    for a in _parallelograms(off):
        v = a.reshape(4, 2)
        for k in (0, 1):
            e = v[k + 1] - v[k]
            out.append((a, (v + e).astype(F).reshape(8)))
    return out


def _half_shared_edge(off):
    out = []
    for a in _parallelograms(off):
        v = a.reshape(4, 2)
        e = (v[1] - v[0]) + F(0.5) * (v[3] - v[0])
        out.append((a, (v + e).astype(F).reshape(8)))
    return out


def _corner_touch(off):
    out = []
    for a in _parallelograms(off):
        v = a.reshape(4, 2)
        out.append((a, (v + ((v[1] - v[0]) + (v[3] - v[0]))).astype(F).reshape(8)))
    return out


def _collinear_overlap(off):
    out = [(_place(_rect(0, 0, 4, 2), off), _place(_rect(1, 0, 3, 2), off))]
    for t in SHAPES:
        out.append((_place(_rot(_rect(0, 0, 32, 16), t), off), _place(_rot(_rect(8, 0, 24, 16), t), off)))
    out.append((_place(_rect(0, 0, 32, 16), off), _place(_rect(8, 0, 40, 16), off)))     # one edge line, partly
    return out


def _concentric(off):
    big = _rect(0, 0, 40, 40)
    out = [(_place(big, off), _place(_rect(10, 10, 30, 30), off)),
           (_place(big, off), _place(_rect(15, 15, 25, 25), off)),
           (_place(big, off), _place(_rot(_rect(10, 10, 30, 30), math.pi / 4, (20, 20)), off)),
           (_place(big, off), _place(_rect(12, 16, 28, 24), off))]
    out.append((_place(_rot(big, 0.3, (20, 20)), off), _place(_rot(_rect(10, 10, 30, 30), 0.3, (20, 20)), off)))
    return out


def _corner_containment(off):
    out = []
    for t in SHAPES:
        out.append((_place(_rot(_rect(0, 0, 40, 40), t), off), _place(_rot(_rect(0, 0, 10, 10), t), off)))
    out.append((_place(_rect(0, 0, 40, 40), off), _place(_rect(30, 0, 40, 25), off)))
    return out


def _vertex_on_edge(off):
    a = _place(_rect(0, 0, 20, 20), off)
    return [(a, _place([[10, 0], [15, 5], [10, 10], [5, 5]], off)),          # inside, one vertex on a's edge
            (a, _place([[10, 0], [15, -5], [10, -10], [5, -5]], off)),       # outside, touching: area 0
            (a, _place([[10, 0], [16, 8], [8, 12], [4, -6]], off)),          # straddling
            (a, _place([[20, 20], [30, 25], [35, 35], [25, 30]], off)),      # vertex on vertex, outside
            (a, _place([[20, 20], [10, 15], [5, 5], [15, 10]], off))]        # vertex on vertex, inside


def _vertex_inside(off):
    a = _rect(0, 0, 20, 20)
    return [(_place(a, off), _place(_rot(a, 0.5, (18, 18)) + (9, 7), off)),
            (_place(a, off), _place([[15, 14], [40, 10], [44, 31], [21, 36]], off)),
            (_place(_rot(a, 0.3), off), _place(_rot(a, 1.0) + (14, 3), off))]


def _triangle_as_quad(off):
    tri = _place([[0, 0], [20, 0], [20, 0], [10, 15]], off)
    tri2 = _place([[4, 3], [4, 3], [26, 6], [12, 20]], off)
    return [(tri, tri.copy()), (tri, _place(_rect(5, -5, 25, 10), off)), (tri, tri2),
            (tri2, _place(DART, off))]


def _zero_area_vs_square(off):
    sq = _place(_rect(2, 2, 10, 10), off)
    return [(_place(z, off), sq) for z in (LINE_D, LINE_H, POINT)]


def _zero_area_self(off):
    """union exactly 0: a zero-area quad against itself, and against another one that it crosses (there the fan
    centre is on neither line, the fan triangles have area, and the interpolated crossings have to cancel)"""
    z =[_place(v, off) for v in (LINE_D, LINE_H, POINT)]
    return [(v, v.copy()) for v in z] + [(z[0], z[1]), (z[0], z[2])]


def _fan_centre(off):
    """the mean of the 8 vertices is a vertex of a / the midpoint of an edge of a (small integers: the kernel's own
    float32 mean is that point exactly, so a fan triangle of a degenerates: wa == 0)"""
    a = _rect(0, 0, 16, 16)
    return [(_place(a, off), _place([[4, 4], [-12, -4], [-20, -20], [-4, -12]], off)),      # mean (0, 0): a's vertex
            (_place(a, off), _place(_rect(-4, -20, 20, 4), off)),                           # mean (8, 0): on a's edge
            (_place(a, off), _place(_rect(-8, -8, 8, 8), off)),                             # mean (4, 4): inside both
            (_place(DART + (-10, -4), off), _place([[10, 4], [2, 12], [-10, -4], [-2, -12]], off))]   # the reflex vertex


def _darts(off):
    sq_in, sq_out = _rect(6, 1, 14, 9), _rect(1, -6, 19, 2)
    mirrored = np.array([[0, 20], [10, 16], [20, 20], [10, 0]], np.float64)
    out = []
    for t in (0.0, 0.3):
        d = _rot(DART, t, (10, 8))
        out += [(_place(d, off), _place(_rot(sq_in, t, (10, 8)), off)),          # reflex vertex inside the square
                (_place(d, off), _place(_rot(sq_out, t, (10, 8)), off)),         # outside: the square cuts both prongs
                (_place(d, off), _place(_rot(mirrored, t, (10, 8)), off)),
                (_place(d, off), _place(d + (3, 2), off)),
                (_place(d, off), _place(_rot(DART, t + 1.1, (10, 8)), off))]
    return out


def _near_identical(off):
    rng = np.random.default_rng(101)
    out = []
    while len(out) < 30:
        a64 = random_quad(rng, rng.uniform(0, 60, 2), len(out) % 3 == 2, (0, 0)).astype(np.float64)
        a, b = _place(a64, off), _place(a64 + rng.normal(0, 1e-3, 8), off)
        if _usable(a) and _usable(b):
            out.append((a, b))
    return out


def _slivers(off):
    """two long thin boxes about ONE centre (itself within 40 px of the offset), angles 1e-3 .. 0.3 apart"""
    rng = np.random.default_rng(102)
    out = []
    for _ in range(40):
        c = rng.uniform(-40, 40, 2)
        t = rng.uniform(0, math.pi)
        d = math.exp(rng.uniform(math.log(1e-3), math.log(0.3)))
        w, h = rng.uniform(300, 1200, 2), rng.uniform(2, 8, 2)
        out.append((_place(_box(c[0], c[1], w[0], h[0], t), off), _place(_box(c[0], c[1], w[1], h[1], t + d), off)))
    return out


def _small_in_big(off):
    rng = np.random.default_rng(103)
    big = _place(_rect(0, 0, 1000, 800), off)
    out = [(big, _place(_rect(0, 0, 5, 5), off)), (big, _place(_rect(995, 795, 1000, 800), off))]
    while len(out) < 20:
        c = np.array([rng.uniform(20, 980), rng.uniform(20, 780)])
        if abs(c[0] - 500) < 200 and abs(c[1] - 400) < 150:
            continue                                                    # away from the big box's centre
        w, h = rng.uniform(3, 12, 2)
        out.append((big, _place(_box(c[0], c[1], w, h, rng.uniform(0, math.pi)), off)))
    return out


def _tiny(off):
    """1e-2 px polygons: the unions are ~1e-4, so mode 1's 0.01 floor decides"""
    rng = np.random.default_rng(104)
    out = []
    while len(out) < 20:
        c = rng.uniform(0, 1, 2)
        a = _place(_box(c[0], c[1], 0.01, 0.008, rng.uniform(0, math.pi)), off)
        b = _place(_box(c[0] + rng.uniform(-4e-3, 4e-3), c[1] + rng.uniform(-4e-3, 4e-3), 0.012, 0.01,
                        rng.uniform(0, math.pi)), off)
        if PX.is_simple(a) and PX.is_simple(b):
            out.append((a, b))
    return out


def _random_pairs(seed, n, dart_a, dart_b, snap):
    def gen(off):
        rng = np.random.default_rng(seed)
        out = []
        for _ in range(n):
            c = rng.uniform(0, 60, 2)
            out.append((random_quad(rng, c, dart_a, off, snap),
                        random_quad(rng, c + rng.uniform(-14, 14, 2), dart_b, off, snap)))
        return out
    return gen


def _regime(gen, quota=False, zero_area=False, general=False):
    """quota: a random regime, at least 25 % of its pairs must have exact IoU > 0.05; zero_area: declared degenerate
    input (not simple); general: simple polygons in general position, fit to cross-check oracle/poly_oracle.py"""
    return NS(gen=gen, quota=quota, zero_area=zero_area, general=general)


REGIMES = {
    "identical": _regime(_identical),
    "shared_edge": _regime(_shared_edge),
    "half_shared_edge": _regime(_half_shared_edge),
    "corner_touch": _regime(_corner_touch),
    "collinear_overlap": _regime(_collinear_overlap),
    "concentric": _regime(_concentric),
    "corner_containment": _regime(_corner_containment),
    "vertex_on_edge": _regime(_vertex_on_edge),
    "vertex_inside": _regime(_vertex_inside, general=True),
    "triangle_as_quad": _regime(_triangle_as_quad),
    "zero_area_vs_square": _regime(_zero_area_vs_square, zero_area=True),
    "zero_area_self": _regime(_zero_area_self, zero_area=True),
    "fan_centre": _regime(_fan_centre),
    "darts": _regime(_darts),
    "near_identical": _regime(_near_identical, quota=True),
    "slivers": _regime(_slivers, quota=True),
    "small_in_big": _regime(_small_in_big),
    "tiny": _regime(_tiny),
    "random_convex": _regime(_random_pairs(105, 70, False, False, False), quota=True, general=True),
    "random_dart": _regime(_random_pairs(106, 50, True, False, False), quota=True, general=True),
    "random_dart_dart": _regime(_random_pairs(107, 30, True, True, False), quota=True, general=True),
    "integer_snapped": _regime(_random_pairs(108, 60, False, False, True), quota=True),
    "integer_snapped_dart": _regime(_random_pairs(109, 30, True, False, True), quota=True),
}


@functools.lru_cache(maxsize=None)
def pairs(name):
    """(A, B, off_index): float32 (m, 8) each, the base pairs of the regime at every offset; read-only"""
    a, b, o = [], [], []
    for k, off in enumerate(OFFSETS):
        for p, q in REGIMES[name].gen(off):
            a.append(p), b.append(q), o.append(k)
    out = np.stack(a).astype(F), np.stack(b).astype(F), np.array(o)
    for v in out:
        v.setflags(write=False)
    return out


def measure(p, q):
    """exact (intersection, union, R2) of one pair"""
    inter = PX.intersection(p, q)
    return inter, PX.area(p) + PX.area(q) - inter, PX.scale_r2(p, q)


def ious_of(inter, union):
    """exact (mode 0, mode 1) IoU from an exact intersection and union"""
    return (Fraction(1) if union == 0 else inter / union), inter / max(union, Fraction(1, 100))


@functools.lru_cache(maxsize=None)
def reference(name):
    """exact values of the regime's base pairs, computed once per process: NS of float64 (m,) arrays iou0, iou1, r2,
    union, tol0, tol1 (the per-pair tolerances of the two modes) and the exact Fractions in `exact`"""
    A, B, _ = pairs(name)
    ex = [measure(p, q) for p, q in zip(A, B)]
    iou = [ious_of(i, u) for i, u, _ in ex]
    r2 = np.array([float(r) for _, _, r in ex])
    union = np.array([float(u) for _, u, _ in ex])
    pos = union[union > 0]
    floor0 = pos.min() if len(pos) else np.inf         # nothing but zero unions: only the 2^-23 term is left
    out = NS(iou0=np.array([float(v[0]) for v in iou]), iou1=np.array([float(v[1]) for v in iou]), r2=r2, union=union,
             floor0=floor0, tol0=tolerance(r2, union, floor0), tol1=tolerance(r2, union, 0.01),
             unit0=unit(r2, union, floor0), unit1=unit(r2, union, 0.01), exact=ex)
    for v in (out.iou0, out.iou1, out.r2, out.union, out.tol0, out.tol1, out.unit0, out.unit1):
        v.setflags(write=False)
    return out


def total_pairs():
    return sum(len(pairs(name)[0]) for name in REGIMES)


# ------------------------------------------------------------------------------------------- the NMS input set
NMS_THRESHOLDS = (0.23, 0.61)           # away from what the tiling produces: 0, 1/3, 1/2, 1
NMS_LABELS = 3


@functools.lru_cache(maxsize=None)
def nms_set():
    """contact-heavy polygons for the NMS decisions: (polys (n, 8) float32, scores (n,) float32 without ties,
    labels (n,) int).  Every third polygon is stored clockwise, the others counter-clockwise."""
    rng = np.random.default_rng(110)
    off = (0.0, 0.0)
    polys = []
    tiles = [_place(_rect(30 * i, 12 * j, 30 * i + 30, 12 * j + 12), off) for j in range(5) for i in range(6)]
    polys += tiles                                                                      # 30 rectangles sharing edges
    src = {}                                                                            # copy -> the polygon it copies
    for k in rng.choice(30, 10, replace=False):                                         # exact duplicates
        src[len(polys)] = k
        polys.append(tiles[k].copy())
    polys += [_place(_rect(30 * i + 15, 12 * j, 30 * i + 45, 12 * j + 12), off)         # half over two tiles each
              for i, j in zip(rng.integers(0, 5, 10), rng.integers(0, 5, 10))]
    polys += [_place(_rect(30 * i, 12 * j + 6, 30 * i + 30, 12 * j + 18), off)
              for i, j in zip(rng.integers(0, 6, 10), rng.integers(0, 4, 10))]
    free = []
    for k in range(130):
        c = np.array([rng.uniform(230, 700), rng.uniform(0, 260)])
        free.append(random_quad(rng, c, k % 4 == 3, off))                               # random simple quads, darts
    first = len(polys)
    polys += free
    for k in rng.choice(130, 10, replace=False):                                        # exact duplicates of those
        src[len(polys)] = first + k
        polys.append(free[k].copy())
    for k in rng.choice(130, 30, replace=False):                                        # near-identical copies
        while True:
            p = (free[k].astype(np.float64) + rng.normal(0, 1e-3, 8)).astype(F)
            if _usable(p):
                src[len(polys)] = first + k
                polys.append(p)
                break
    for t in (0.0, 0.3):                                                                # the hand-made darts
        d = _rot(DART, t, (10, 8)) + (100, 120)
        polys += [_place(d, off), _place(d + (3, 2), off),
                  _place(_rot(_rect(6, 1, 14, 9), t, (10, 8)) + (100, 120), off)]
    polys = np.stack(polys).astype(F)
    for k in range(len(polys)):
        v = polys[k].reshape(4, 2).astype(np.float64)
        ccw = float(np.sum(v[:, 0] * np.roll(v[:, 1], -1) - v[:, 1] * np.roll(v[:, 0], -1))) > 0
        if ccw == (k % 3 == 0):
            polys[k] = v[::-1].astype(F).reshape(8)
    n = len(polys)
    scores = (rng.permutation(n) + 1).astype(F) / F(n + 1)          # no ties
    labels = rng.integers(0, NMS_LABELS, n)
    for k, j in src.items():
        labels[k] = labels[j]                                       # a copy competes with what it copies
    for v in (polys, scores, labels):
        v.setflags(write=False)
    return polys, scores, labels


@functools.lru_cache(maxsize=None)
def nms_reference():
    """exact mode-0 IoU of every pair of nms_set() whose bounding boxes share an interior point (all others are 0
    without a slab evaluation): NS of float64 (n, n) iou and tol (mode 0, floor = the smallest positive union of the
    set) and the number of slab evaluations"""
    polys, _, _ = nms_set()
    n = len(polys)
    lo, hi = polys.reshape(n, 4, 2).min(1), polys.reshape(n, 4, 2).max(1)
    v = polys.reshape(n, 1, 4, 2).astype(np.float64)
    both = np.concatenate([np.broadcast_to(v, (n, n, 4, 2)), np.broadcast_to(v.transpose(1, 0, 2, 3), (n, n, 4, 2))], 2)
    r2 = ((both - both.mean(2, keepdims=True)) ** 2).sum(3).max(2)       # float64 is plenty for a tolerance's scale
    areas = [PX.area(p) for p in polys]
    iou = np.zeros((n, n))
    union = np.add.outer(np.array(areas, np.float64), np.array(areas, np.float64))
    slabs = 0
    for i in range(n):
        for j in range(i, n):
            if np.any(hi[i] <= lo[j]) or np.any(hi[j] <= lo[i]):
                continue                                                 # no common interior point: IoU 0
            inter = PX.intersection(polys[i], polys[j])
            u = areas[i] + areas[j] - inter
            iou[i, j] = iou[j, i] = float(ious_of(inter, u)[0])
            union[i, j] = union[j, i] = float(u)
            slabs += 1
    floor0 = union[union > 0].min()
    out = NS(iou=iou, tol=tolerance(r2, union, floor0), slabs=slabs)
    out.iou.setflags(write=False), out.tol.setflags(write=False)
    return out


def nms_near(thr):
    """bool (n,): polygons with a partner (other than themselves) whose exact IoU is within 2 x that pair's tolerance
    of the threshold -- a correct kernel may decide those either way, so they are left out of the comparison"""
    ref = nms_reference()
    near = np.abs(ref.iou - thr) <= 2 * ref.tol
    np.fill_diagonal(near, False)
    return near.any(1)


def greedy(iou, scores, thr, labels=None, alive=None):
    """keep flags of the greedy scan in descending score order, suppressing at IoU > thr (same label only)"""
    n = len(scores)
    order = np.argsort(-np.asarray(scores, np.float64), kind="stable")
    gone = np.zeros(n, bool) if alive is None else ~np.asarray(alive)
    keep = np.zeros(n, bool)
    for i in order:
        if gone[i]:
            continue
        keep[i] = True
        hit = iou[i] > thr
        if labels is not None:
            hit &= labels == labels[i]
        gone |= hit
    return keep
