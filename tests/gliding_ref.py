"""Restatement of the Gliding Vertex box algebra in numpy (test infrastructure; nothing in jdet_amd imports it).

What it restates, from the formulas of the paper (https://arxiv.org/pdf/1911.09358.pdf, section 3.1-3.3) and the
contract the package documents: the horizontal delta codec, the gliding offsets of a quadrilateral's four extreme
vertices along the sides of its enclosing box, the obliquity ratio, the head's target assembly for a given set of
sampled rows, and the decode -> polygon path.  Every function computes in the dtype of its first array argument, so
the same text gives the float64 reference and the float32 twin the GPU tests use to size their tolerances.  Where the
order of floating-point operations matters (the shoelace sum over absolute coordinates) the order is the documented
one: terms i = 0..3 of 0.5 * (x_i y_{i+1} - x_{i+1} y_i), added to 0 in that order.

Ties between extreme vertices go to the lowest vertex index (numpy's argmax / argmin return the first extreme)."""
import math

import numpy as np

# the head's codec constants in GLIDING_CFG, shared by the tests and by scripts/gliding_timing.py
MEANS, STDS = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)


def _c(v, like):
    return np.asarray(v, dtype=like.dtype)


def rect_poly(obb):
    """(n,5) [x, y, w, h, theta] -> (n,8): centre +- (w/2)(cos, -sin) +- (h/2)(-sin, -cos), the package's obb2poly"""
    obb = np.asarray(obb)
    x, y, w, h, t = (obb[:, k] for k in range(5))
    c, s = np.cos(t), np.sin(t)
    ax, ay = w / 2 * c, -w / 2 * s
    bx, by = -h / 2 * s, -h / 2 * c
    return np.stack([x + ax + bx, y + ay + by, x + ax - bx, y + ay - by, x - ax - bx, y - ay - by,
                     x - ax + bx, y - ay + by], 1)


def poly_hbb(polys):
    xs, ys = polys[:, 0::2], polys[:, 1::2]
    return np.stack([xs.min(1), ys.min(1), xs.max(1), ys.max(1)], 1)


def hbb_poly(b):
    return np.stack([b[..., 0], b[..., 1], b[..., 2], b[..., 1], b[..., 2], b[..., 3], b[..., 0], b[..., 3]], -1)


def delta_encode(rois, gts, means=(0, 0, 0, 0), stds=(1, 1, 1, 1)):
    half = _c(0.5, rois)
    px, py = (rois[:, 0] + rois[:, 2]) * half, (rois[:, 1] + rois[:, 3]) * half
    pw, ph = rois[:, 2] - rois[:, 0], rois[:, 3] - rois[:, 1]
    gx, gy = (gts[:, 0] + gts[:, 2]) * half, (gts[:, 1] + gts[:, 3]) * half
    gw, gh = gts[:, 2] - gts[:, 0], gts[:, 3] - gts[:, 1]
    d = np.stack([(gx - px) / pw, (gy - py) / ph, np.log(gw / pw), np.log(gh / ph)], 1)
    return (d - _c(means, rois)[None]) / _c(stds, rois)[None]


def delta_decode(rois, deltas, means=(0, 0, 0, 0), stds=(1, 1, 1, 1), max_shape=None, wh_ratio_clip=16 / 1000):
    """rois (n,4), deltas (n,4C) -> boxes (n,C,4); max_shape = (h, w) clamps x to [0, w] and y to [0, h]"""
    n = rois.shape[0]
    half = _c(0.5, rois)
    d = deltas.reshape(n, -1, 4) * _c(stds, rois)[None, None] + _c(means, rois)[None, None]
    lim = _c(abs(math.log(wh_ratio_clip)), rois)
    dw, dh = np.clip(d[..., 2], -lim, lim), np.clip(d[..., 3], -lim, lim)
    px, py = ((rois[:, 0] + rois[:, 2]) * half)[:, None], ((rois[:, 1] + rois[:, 3]) * half)[:, None]
    pw, ph = (rois[:, 2] - rois[:, 0])[:, None], (rois[:, 3] - rois[:, 1])[:, None]
    gw, gh = pw * np.exp(dw), ph * np.exp(dh)
    gx, gy = px + pw * d[..., 0], py + ph * d[..., 1]
    x1, y1, x2, y2 = gx - gw * half, gy - gh * half, gx + gw * half, gy + gh * half
    if max_shape is not None:
        h, w = _c(max_shape[0], rois), _c(max_shape[1], rois)
        zero = _c(0, rois)
        x1, x2 = np.clip(x1, zero, w), np.clip(x2, zero, w)
        y1, y2 = np.clip(y1, zero, h), np.clip(y2, zero, h)
    return np.stack([x1, y1, x2, y2], -1)


def extreme_vertices(polys):
    """indices (n,) of the top (min y), right (max x), bottom (max y), left (min x) vertex; first extreme on a tie"""
    xs, ys = polys[:, 0::2], polys[:, 1::2]
    return ys.argmin(1), xs.argmax(1), ys.argmax(1), xs.argmin(1)


def fix_encode(polys, with_flags=False):
    """(n,8) -> (n,4) gliding offsets (dt, dr, dd, dl); rows whose top and right vertex share a y, or whose right and
    bottom vertex share an x, are all 1.  with_flags: also that row mask"""
    xs, ys = polys[:, 0::2], polys[:, 1::2]
    r = np.arange(polys.shape[0])
    top, right, bottom, left = extreme_vertices(polys)
    b = poly_hbb(polys)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    fix = np.stack([(xs[r, top] - b[:, 0]) / w, (ys[r, right] - b[:, 1]) / h, (b[:, 2] - xs[r, bottom]) / w,
                    (b[:, 3] - ys[r, left]) / h], 1)
    flat = (ys[r, top] - ys[r, right] == 0) | (xs[r, right] - xs[r, bottom] == 0)
    fix[flat] = 1
    return (fix, flat) if with_flags else fix


def has_vertex_tie(polys):
    """rows where an extreme of x or of y is reached by more than one vertex"""
    xs, ys = polys[:, 0::2], polys[:, 1::2]
    cnt = lambda v, e: (v == e[:, None]).sum(1)   # noqa: E731
    return (cnt(xs, xs.max(1)) > 1) | (cnt(xs, xs.min(1)) > 1) | (cnt(ys, ys.max(1)) > 1) | (cnt(ys, ys.min(1)) > 1)


def fix_decode(boxes, fix):
    """boxes (..., 4), fix (..., 4) -> (..., 8): top, right, bottom, left vertex"""
    x1, y1, x2, y2 = (boxes[..., k] for k in range(4))
    w, h = x2 - x1, y2 - y1
    return np.stack([x1 + w * fix[..., 0], y1, x2, y1 + h * fix[..., 1], x2 - w * fix[..., 2], y2, x1,
                     y2 - h * fix[..., 3]], -1)


def ratio_encode(polys):
    xs, ys = polys[:, 0::2], polys[:, 1::2]
    b = poly_hbb(polys)
    h_area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    area = np.zeros(polys.shape[0], dtype=polys.dtype)
    half = _c(0.5, polys)
    for i in range(4):
        j = (i + 1) % 4
        area = area + half * (xs[:, i] * ys[:, j] - xs[:, j] * ys[:, i])
    return (np.abs(area) / h_area)[:, None]


def targets(rois, polys, means, stds):
    """bbox (n,4), fix (n,4), ratio (n,1) targets of matched (roi, polygon) rows"""
    return delta_encode(rois, poly_hbb(polys), means, stds), fix_encode(polys), ratio_encode(polys)


def head_targets(boxes, polys, labels, is_pos, valid, means, stds, num_classes, pos_weight=-1):
    """the head's target assembly for GIVEN sampled rows: boxes (R,4), their matched polygons (R,8), the matched gt's
    0-based label (R,), is_pos / valid (R,) -> labels [background = num_classes off the positives], label_weights,
    bbox / fix / ratio targets (zero off the positives), regression weight (1 on the positives)"""
    pw = 1.0 if pos_weight <= 0 else pos_weight
    out_labels = np.where(is_pos, labels, num_classes)
    label_weights = valid * np.where(is_pos, pw, 1.0)
    bt, ft, rt = targets(boxes, polys, means, stds)
    m = is_pos[:, None]
    return out_labels, label_weights, np.where(m, bt, 0), np.where(m, ft, 0), np.where(m, rt, 0), is_pos.astype(float)


def decode_polys(rois, bbox_pred, fix_pred, ratio_pred, means, stds, max_shape=None, wh_ratio_clip=16 / 1000,
                 ratio_thr=0.8, scale=(1, 1, 1, 1)):
    """rois (n,4), bbox_pred / fix_pred (n,4C), ratio_pred (n,C) -> polygons (n, 8C): decoded box, vertices glided
    along its sides, the box's own corners where ratio > ratio_thr, (x, y) / (scale_x, scale_y)"""
    n, C = ratio_pred.shape
    boxes = delta_decode(rois, bbox_pred, means, stds, max_shape, wh_ratio_clip)
    polys = fix_decode(boxes, fix_pred.reshape(n, C, 4))
    polys = np.where((ratio_pred > _c(ratio_thr, rois))[..., None], hbb_poly(boxes), polys)
    s = _c(scale, rois)
    return (polys / np.concatenate([s, s])[None, None]).reshape(n, -1)


def greedy_nms(boxes, scores, thresh):
    """kept indices in descending score (stable); suppress when IoU > thresh, no +1 pixel convention"""
    order = np.argsort(-scores, kind="stable")
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    dead = np.zeros(len(boxes), bool)
    keep = []
    for i in order:
        if dead[i]:
            continue
        keep.append(i)
        iw = np.clip(np.minimum(boxes[i, 2], boxes[:, 2]) - np.maximum(boxes[i, 0], boxes[:, 0]), 0, None)
        ih = np.clip(np.minimum(boxes[i, 3], boxes[:, 3]) - np.maximum(boxes[i, 1], boxes[:, 1]), 0, None)
        inter = iw * ih
        iou = inter / np.maximum(area[i] + area - inter, 1e-12)
        dead |= iou > thresh
    return np.asarray(keep, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ inputs
def random_obbs(rng, n, lo=50.0, hi=950.0, side=(8.0, 300.0)):
    return np.concatenate([rng.uniform(lo, hi, (n, 2)), rng.uniform(side[0], side[1], (n, 2)),
                           rng.uniform(-math.pi / 2, math.pi / 2, (n, 1))], 1)


def random_convex_quads(rng, n, lo=50.0, hi=950.0, side=(8.0, 300.0)):
    """general convex quadrilaterals: one vertex on each side of a random box (top, right, bottom, left, away from the
    corners -- such a quadrilateral is convex and its four extreme vertices are four different vertices), listed from
    a random starting vertex in a random direction"""
    c = rng.uniform(lo, hi, (n, 2))
    wh = rng.uniform(2 * side[0], side[1], (n, 2))
    b = np.concatenate([c - wh / 2, c + wh / 2], 1)
    q = fix_decode(b, rng.uniform(0.05, 0.95, (n, 4))).reshape(n, 4, 2)
    start, flip = rng.integers(0, 4, n), rng.integers(0, 2, n).astype(bool)
    idx = (start[:, None] + np.arange(4)[None]) % 4
    idx = np.where(flip[:, None], idx[:, ::-1], idx)
    return q[np.arange(n)[:, None], idx].reshape(n, 8)


def random_rows(rng, n):
    """n (roi, polygon) rows: half rotated rectangles, half general convex quadrilaterals; the roi is the polygon's
    enclosing box jittered as a positive proposal would be.  float32-representable float64 arrays."""
    k = n // 2
    polys = np.concatenate([rect_poly(random_obbs(rng, k)), random_convex_quads(rng, n - k)])
    b = poly_hbb(polys)
    wh = np.stack([b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)
    ctr = (b[:, :2] + b[:, 2:]) / 2 + rng.uniform(-0.15, 0.15, (n, 2)) * wh
    half = wh / 2 * np.exp(rng.uniform(-0.3, 0.3, (n, 2)))
    rois = np.concatenate([ctr - half, ctr + half], 1)
    return rois.astype(np.float32).astype(np.float64), polys.astype(np.float32).astype(np.float64)


def target_case(n=4000, seed=0):
    """the rows of the GPU target comparison (tests/test_gpu_gliding.py; scripts/gliding_timing.py reports the same)"""
    return random_rows(np.random.default_rng(seed), n)


def decode_case(n=300, C=15, seed=2):
    """inputs of the GPU decode comparison: rois (n,4), bbox_pred / fix_pred (n,4C), ratio_pred (n,C) with rows on the
    wh_ratio_clip clamp, beyond a 1024^2 image on both sides, and on both sides of ratio_thr = 0.8;
    float32-representable float64 arrays"""
    rng = np.random.default_rng(seed)
    rois, _ = random_rows(rng, n)
    bbox = rng.normal(0, 1.0, (n, 4 * C))
    bbox[0, 2::4], bbox[1, 3::4], bbox[2, 6] = 40.0, -40.0, 25.0  # dw / dh on the wh_ratio_clip clamp
    rois[3] = [900.0, 880.0, 1100.0, 1010.0]                      # beyond max_shape: on the border clamp
    rois[4] = [-40.0, -30.0, 60.0, 50.0]
    fix = rng.uniform(0, 1, (n, 4 * C))
    ratio = rng.uniform(0, 1, (n, C))
    ratio[5, :3] = [0.95, 0.2, 0.81]                              # both sides of ratio_thr in one row
    f = lambda a: a.astype(np.float32).astype(np.float64)         # noqa: E731
    return f(rois), f(bbox), f(fix), f(ratio)
