"""numpy restatement and fixtures of the Rotated RepPoints init-stage assignment (include/jdet_hip.h:
jdet_convex_point_assign).

`assign_loop` is ConvexAssigner.assign of the reference (models/boxes/assigner.py:L433-548) as its LITERAL sequential
loop over the gts -- a mask of the gt's level, the distances, a stable argsort standing for the topk (equal distances:
lower point index first; clamped to the level's size), the strict `<` against the distance recorded so far -- with the
fp32 operations taken in the order the header states.  The kernel resolves the same conflicts by an order-independent
64-bit atomicMin; the tests compare the two forms.

Fixtures come from fixed seeds.  Apart from the hand-built cases every gt keeps (log2(w / scale) + log2(h / scale)) / 2 at
least 1e-3 away from an integer, so a one-ulp difference between two log2f implementations cannot move its level."""
import math

import numpy as np

F = np.float32
STRIDES = (8, 16, 32, 64, 128)
LEVEL_IDS = (3, 4, 5, 6, 7)
SCALE = 4.0
MARGIN = 1e-3


def grid(h, w, strides=STRIDES):
    """(points (N, 2) fp32 [x, y], per-level sizes) of an h x w image: MlvlPointGenerator with offset 0, row-major"""
    pts, sizes = [], []
    for s in strides:
        fh, fw = int(math.ceil(h / s)), int(math.ceil(w / s))
        yy, xx = np.meshgrid(np.arange(fh, dtype=F) * F(s), np.arange(fw, dtype=F) * F(s), indexing="ij")
        pts.append(np.stack([xx.reshape(-1), yy.reshape(-1)], 1))
        sizes.append(fh * fw)
    return np.concatenate(pts).astype(F), sizes


def lg(x):
    """log2 in fp32, exact on exact powers of two (the header's lg)"""
    x = np.asarray(x, F)
    m, e = np.frexp(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m == F(0.5), (e - 1).astype(F), np.log2(x).astype(F)).astype(F)


def boxes_of(gt):
    """horizontal boxes of (K, 8) polygons: (cx, cy, w, h), fp32"""
    gt = np.asarray(gt, F).reshape(-1, 8)
    xs, ys = gt[:, 0::2], gt[:, 1::2]
    xmin, xmax, ymin, ymax = xs.min(1), xs.max(1), ys.min(1), ys.max(1)
    cx, cy = (xmin + xmax) / F(2), (ymin + ymax) / F(2)
    w, h = np.maximum(xmax - xmin, F(1e-6)), np.maximum(ymax - ymin, F(1e-6))
    return cx.astype(F), cy.astype(F), w.astype(F), h.astype(F)


def level_value(gt, scale=SCALE):
    """(lg(w / scale) + lg(h / scale)) / 2 in fp32, before truncation"""
    _, _, w, h = boxes_of(gt)
    return ((lg(w / F(scale)) + lg(h / F(scale))) / F(2)).astype(F)


def levels_of(gt, level_ids=LEVEL_IDS, scale=SCALE):
    v = level_value(gt, scale)
    return np.clip(np.trunc(v).astype(np.int64), min(level_ids), max(level_ids))


def level_margin(gt, scale=SCALE):
    """distance of every gt's level value from the nearest integer (float64 of the fp32 value)"""
    v = level_value(gt, scale).astype(np.float64)
    return np.abs(v - np.rint(v))


def assign_loop(points, sizes, level_ids, gt, gt_labels=None, scale=SCALE, pos_num=1, labels_filled=0):
    """the reference's sequential loop.  Returns dict(gt_inds int32 (N), labels int32 (N) | None, rank_ties,
    equal_claims): rank_ties counts the gts whose candidate list is cut between two equal distances, equal_claims the
    claims that met a recorded distance equal to their own (the strict < keeps the earlier gt)."""
    points = np.asarray(points, F)[:, :2]
    gt = np.asarray(gt, F).reshape(-1, 8)
    N, K = len(points), len(gt)
    points_lvl = np.repeat(np.asarray(level_ids, np.int64), sizes)
    assert len(points_lvl) == N
    assigned = np.zeros(N, np.int32)
    dist = np.full(N, np.inf, F)
    rank_ties = equal_claims = 0
    if K:
        cx, cy, w, h = boxes_of(gt)
        lvl = levels_of(gt, level_ids, scale)
    rng = np.arange(N)
    for idx in range(K):
        mask = points_lvl == lvl[idx]
        index = rng[mask]
        if len(index) == 0:
            continue
        lp = points[mask]
        dx = ((lp[:, 0] - cx[idx]) / w[idx]).astype(F)
        dy = ((lp[:, 1] - cy[idx]) / h[idx]).astype(F)
        d = np.sqrt((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)
        k = min(pos_num, len(index))
        order = np.argsort(d, kind="stable")
        if k < len(index) and d[order[k - 1]] == d[order[k]]:
            rank_ties += 1
        order = order[:k]
        min_dist, pidx = d[order], index[order]
        equal_claims += int((min_dist == dist[pidx]).sum())
        less = min_dist < dist[pidx]
        assigned[pidx[less]] = idx + 1
        dist[pidx[less]] = min_dist[less]
    labels = None
    if gt_labels is not None:
        labels = np.full(N, labels_filled, np.int32)
        pos = assigned > 0
        labels[pos] = np.asarray(gt_labels, np.int32)[assigned[pos] - 1]
    return dict(gt_inds=assigned, labels=labels, rank_ties=rank_ties, equal_claims=equal_claims)


def obb_poly(c, wh, th):
    """corners of rotated boxes (K, 8), fp32"""
    c, wh, th = np.asarray(c, np.float64), np.asarray(wh, np.float64), np.asarray(th, np.float64).reshape(-1)
    cs, sn = np.cos(th), np.sin(th)
    out = []
    for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        dx, dy = sx * wh[:, 0] / 2, sy * wh[:, 1] / 2
        out += [c[:, 0] + dx * cs - dy * sn, c[:, 1] + dx * sn + dy * cs]
    return np.stack(out, 1).astype(F)


def random_gts(rng, K, h, w, lo=8.0, hi=None):
    """K rotated boxes centred inside an h x w image, sides in [lo, hi] (hi: the image's longer side), whose level value
    keeps MARGIN from every integer (rejection sampling)"""
    out = []
    while len(out) < K:
        c = rng.uniform(0, [w, h], (1, 2))
        wh = np.exp(rng.uniform(np.log(lo), np.log(hi or max(h, w)), (1, 2)))
        th = rng.uniform(-np.pi / 2, np.pi / 2, 1)
        p = obb_poly(c, wh, th)
        if level_margin(p)[0] >= MARGIN:
            out.append(p[0])
    return np.stack(out).astype(F)


# name -> (image (h, w), gt counts per image, seed, longest side of a gt).  s64: the gts reach past the image, so the
# one-point levels 6 and 7 get gts and pos_num = 3 meets the clamp.
FIXTURES = {
    "b2_256": ((256, 256), (8, 8), 11, None),
    "hw_256x192": ((192, 256), (8,), 12, None),
    "s64": ((64, 64), (8,), 13, 1024.0),
    "k70_k0": ((256, 256), (70, 0), 14, None),
}


def fixture(name):
    """dict(points, sizes, level_ids, gt (B, Kmax, 8) zero-padded, labels (B, Kmax) int32 1-based, counts)"""
    (h, w), counts, seed, hi = FIXTURES[name]
    rng = np.random.default_rng(seed)
    points, sizes = grid(h, w)
    Kmax = max(max(counts), 1)
    gt = np.zeros((len(counts), Kmax, 8), F)
    labels = np.zeros((len(counts), Kmax), np.int32)
    for b, k in enumerate(counts):
        if k:
            gt[b, :k] = random_gts(rng, k, h, w, hi=hi)
            labels[b, :k] = rng.integers(1, 16, k)
    return dict(points=points, sizes=sizes, level_ids=list(LEVEL_IDS), gt=gt, labels=labels, counts=list(counts),
                hw=(h, w))


def square(cx, cy, side):
    """axis-aligned square polygon (8,)"""
    a = side / 2.0
    return np.asarray([cx - a, cy - a, cx + a, cy - a, cx + a, cy + a, cx - a, cy + a], F)


def rect(cx, cy, w, h):
    return np.asarray([cx - w / 2, cy - h / 2, cx + w / 2, cy - h / 2, cx + w / 2, cy + h / 2, cx - w / 2, cy + h / 2], F)
