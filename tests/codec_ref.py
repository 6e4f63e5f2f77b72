"""Restatements of the seven elementwise rotated-box codecs, their decision margins and the fixtures of the codec tests
(test infrastructure; nothing in jdet_amd imports it, and it does not import oracle/box_oracle.py, the float32 twin).

  bbox2delta_rotated / delta2bbox_rotated   models/boxes/box_ops.py:L176-285 of the reference
  midpoint_encode / midpoint_decode         models/boxes/coder.py:L332-437, ops/bbox_transforms.py:L499-517, L575-646
  oriented_encode / oriented_decode         models/boxes/coder.py:L449-518
  obb2hbb2obb                               ops/bbox_transforms.py:L639-646, L653-665

Written from the reference's text in plain numpy, in its order of operations.  Every function computes in `dt` (float64
by default) from the float32 VALUES of its inputs, so the same text is the float64 reference and, with dt = float32, the
twin whose distance from float64 (`e32`) sizes every bound of the GPU tests.  `%` is floor-mod.  Each function returns

  (output, margins, flags)

margins: name -> the distance of every comparison of that kind to its threshold, one value per output box (the minimum
over the comparisons of that kind in the box); flags: name -> which way the box's discrete decisions went.

  clamp      dw, dh against +-max_ratio (delta units)          dab       da, db against +-0.5
  safe_log   the size ratios against log's clamp (in log units)
  wrap       every floor-mod argument against its wrap point, in radians
  wh         w > h of regular_obb, |w - h| / max(w, h)         wwhh      ww >= hh of hbb2obb, relative
  tie        | |dtheta1| - |dtheta2| | of the oriented encode, in radians
  mask       the eight |delta| > 0.1 comparisons of the midpoint encode, in px
  sep        midpoint decode: distance of the top and the right vertex / the longest half-diagonal (atan2 of a
             vanishing difference is not a comparison any precision settles)
  diag       midpoint decode: (longest - second longest half-diagonal group) / longest, top/bottom against right/left

`mut` switches ONE deliberately wrong variant on (tests/test_codec_cpu.py: the bounds must tell each from the right
one); no test compares a kernel with a mutated restatement.

Fixtures are functions of a seed, with no files: `fixture(name)`.  A fixture is drawn with a surplus and cut to N_ROWS
rows that meet the CONSTRUCTION limits (every decoded side in [8, 1024] px, centres within [0, 1024]; these are part
of what the fixture is, a 0.13 px box at x = 900 has an inherent fp32 angle error of 2.7e-3 rad).  RETENTION is
separate and is what the 1 % cap of the tests is about: a box is retained when each margin exceeds RETAIN[name].

Means, stds and the deltas' scale are exactly representable in float32 (dyadic), so the float64 restatement, the torch
composition in float64 and the kernel are handed the same numbers."""
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
PI = math.pi

# pairwise distinct in every slot, dyadic
M5 = (0.03125, -0.0625, 0.09375, -0.015625, 0.046875)
S5 = (0.125, 0.15625, 0.1875, 0.25, 0.109375)
M6 = M5 + (-0.0234375,)
S6 = (0.125, 0.15625, 0.1875, 0.25, 0.5, 0.375)
CLIP_HI, CLIP_LO = 16 / 1000, 0.25          # max_ratio 4.135 (the default) and 1.386
N_ROWS = 4096
SIDE_MIN, COORD_MAX = 8.0, 1024.0

# retention thresholds.  The issue's starting values, kept; the three it leaves open:
#   dab 1e-5 like the other clamps; sep 1e-2: the top-right distance is a side of the decoded rectangle, >= 8 px by
#   construction, and the half-diagonal is <= 724 px, so 1e-2 only restates the side limit in the margin's unit;
#   diag 1e-6: the stretch factor max / len is continuous where two lengths cross, so the tie is no branch -- the
#   margin is reported, and only an exact tie is kept out
RETAIN = dict(wrap=1e-4, tie=1e-4, clamp=1e-5, dab=1e-5, safe_log=1e-5, wh=1e-4, wwhh=1e-4, mask=1e-3, sep=1e-2,
              diag=1e-6)


# ------------------------------------------------------------------------------------------------------ pieces
def _slots(means, stds, mut):
    means, stds = list(means), list(stds)
    for name, (a, b) in (("swap01", (0, 1)), ("swap23", (2, 3))):
        if mut == name:
            means[a], means[b] = means[b], means[a]
            stds[a], stds[b] = stds[b], stds[a]
    return means, stds


def _floor_mod(x, start, cycle, dt):
    """x folded into [start, start + cycle) -> (value, distance of x to the nearest wrap point)"""
    s, c = dt(start), dt(cycle)
    m = np.mod(x - s, c)
    return m + s, np.minimum(m, c - m).astype(F64)


def _regular_theta(theta, dt, mut):
    return _floor_mod(theta, 0.0 if mut == "wrap0pi" else -PI / 2, PI, dt)


def _norm_angle(a, dt, mut):
    return _floor_mod(a, -PI / 2 if mut == "norm_start" else -PI / 4, PI, dt)


def _regular_obb(w, h, theta, dt, mut):
    """-> w, h, theta, margins(wh, wrap), swapped"""
    keep = w > h
    m_wh = (np.abs(w - h) / np.maximum(w, h)).astype(F64)
    turned = theta if mut == "no_half_pi" else theta + dt(PI / 2)
    t, m_wrap = _regular_theta(np.where(keep, theta, turned), dt, mut)
    return np.where(keep, w, h), np.where(keep, h, w), t, m_wh, m_wrap, ~keep


def _denorm(deltas, means, stds, k, dt, mut):
    """(n, C * k) -> (n, C, k) denormalised"""
    means, stds = _slots(means, stds, mut)
    d = np.asarray(deltas, dt)
    return d.reshape(d.shape[0], -1, k) * np.asarray(stds, dt) + np.asarray(means, dt)


def _roi_rows(rois, C, dt, mut):
    """the roi of every (row, class) element: (n, C, cols).  Element idx = row * C + class reads roi idx / C"""
    r = np.asarray(rois, dt)
    idx = np.arange(r.shape[0] * C)
    rows = idx % C if mut == "mod_ncls" else idx // C
    return r[rows].reshape(r.shape[0], C, r.shape[1])


def _size_clamp(dw, dh, clip, dt, mut):
    mr = dt(abs(math.log(clip)))
    margin = np.minimum(np.minimum(np.abs(dw - mr), np.abs(dw + mr)), np.minimum(np.abs(dh - mr), np.abs(dh + mr)))
    flags = dict(lower=(dw < -mr) | (dh < -mr), upper=(dw > mr) | (dh > mr))
    flags["clamped"] = flags["lower"] | flags["upper"]
    if mut == "upper_only":
        dw, dh = np.minimum(dw, mr), np.minimum(dh, mr)
    elif mut != "no_clamp":
        dw, dh = np.clip(dw, -mr, mr), np.clip(dh, -mr, mr)
    return dw, dh, margin.astype(F64), flags


def _safe_log(x, dt):
    lo, hi = dt(1e-30), dt(1e30)
    with np.errstate(divide="ignore"):
        lx = np.log(x.astype(F64))
    return np.log(np.clip(x, lo, hi)), np.minimum(lx - math.log(1e-30), math.log(1e30) - lx)


# ------------------------------------------------------------------------------------------------------ codecs
def bbox2delta_rotated(proposals, gt, means, stds, dt=F64, mut=None):
    """(n, 5), (n, 5) -> (n, 5)"""
    p, g = np.asarray(proposals, dt), np.asarray(gt, dt)
    means, stds = _slots(means, stds, mut)
    c, s = np.cos(p[:, 4]), np.sin(p[:, 4])
    cx, cy = g[:, 0] - p[:, 0], g[:, 1] - p[:, 1]
    dx = (c * cx + s * cy) / p[:, 2]
    dy = (-s * cx + c * cy) / p[:, 3]
    dw, m1 = _safe_log(g[:, 2] / p[:, 2], dt)
    dh, m2 = _safe_log(g[:, 3] / p[:, 3], dt)
    a, m_wrap = _norm_angle(g[:, 4] - p[:, 4], dt, mut)
    d = np.stack([dx, dy, dw, dh, a / dt(PI)], 1)
    out = (d - np.asarray(means, dt)[None]) / np.asarray(stds, dt)[None]
    return out, dict(safe_log=np.minimum(m1, m2), wrap=m_wrap), {}


def delta2bbox_rotated(rois, deltas, means, stds, wh_ratio_clip=CLIP_HI, dt=F64, mut=None):
    """(n, 5), (n, 5C) -> (n, 5C)"""
    d = _denorm(deltas, means, stds, 5, dt, mut)
    r = _roi_rows(rois, d.shape[1], dt, mut)
    dw, dh, m_clamp, flags = _size_clamp(d[..., 2], d[..., 3], wh_ratio_clip, dt, mut)
    c, s = np.cos(r[..., 4]), np.sin(r[..., 4])
    gx = d[..., 0] * r[..., 2] * c - d[..., 1] * r[..., 3] * s + r[..., 0]
    gy = d[..., 0] * r[..., 2] * s + d[..., 1] * r[..., 3] * c + r[..., 1]
    gw, gh = r[..., 2] * np.exp(dw), r[..., 3] * np.exp(dh)
    ga, m_wrap = _norm_angle(dt(PI) * d[..., 4] + r[..., 4], dt, mut)
    out = np.stack([gx, gy, gw, gh, ga], -1).reshape(d.shape[0], -1)
    return out, dict(clamp=m_clamp, wrap=m_wrap), flags


def obb2hbb2obb(boxes, dt=F64, mut=None):
    """hbb2obb(obb2hbb(b)): (n, 5+) -> (n, 5)"""
    b = np.asarray(boxes, dt)
    x, y, w, h, t = (b[:, k] for k in range(5))
    c, s = np.cos(t), np.sin(t)
    xb = np.abs(w / dt(2) * c) + np.abs(h / dt(2) * s)
    yb = np.abs(w / dt(2) * s) + np.abs(h / dt(2) * c)
    x1, y1, x2, y2 = x - xb, y - yb, x + xb, y + yb
    cx, cy, ww, hh = (x1 + x2) * dt(0.5), (y1 + y2) * dt(0.5), x2 - x1, y2 - y1
    flag = ww >= hh
    out = np.stack([cx, cy, np.where(flag, ww, hh), np.where(flag, hh, ww), np.where(flag, dt(0), dt(0) - dt(PI / 2))], 1)
    return out, dict(wwhh=(np.abs(ww - hh) / np.maximum(ww, hh)).astype(F64)), dict(wide=flag)


def midpoint_encode(anchors, gt, means, stds, dt=F64, mut=None):
    """hbb anchors (n, 4), obb gts (n, 5) -> (n, 6)"""
    a, g = np.asarray(anchors, dt), np.asarray(gt, dt)
    means, stds = _slots(means, stds, mut)
    thr = dt({"mask005": 0.05, "mask02": 0.2}.get(mut, 0.1))
    px, py = (a[:, 0] + a[:, 2]) * dt(0.5), (a[:, 1] + a[:, 3]) * dt(0.5)
    pw, ph = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    c, s = np.cos(g[:, 4]), np.sin(g[:, 4])
    w2, h2 = g[:, 2] / dt(2), g[:, 3] / dt(2)
    xb, yb = np.abs(w2 * c) + np.abs(h2 * s), np.abs(w2 * s) + np.abs(h2 * c)
    hx0, hy0, hx1, hy1 = g[:, 0] - xb, g[:, 1] - yb, g[:, 0] + xb, g[:, 1] + yb
    gx, gy, gw, gh = (hx0 + hx1) * dt(0.5), (hy0 + hy1) * dt(0.5), hx1 - hx0, hy1 - hy0
    v1x, v1y, v2x, v2y = w2 * c, -w2 * s, -h2 * s, -h2 * c
    qx = np.stack([g[:, 0] + v1x + v2x, g[:, 0] + v1x - v2x, g[:, 0] - v1x - v2x, g[:, 0] - v1x + v2x], 1)
    qy = np.stack([g[:, 1] + v1y + v2y, g[:, 1] + v1y - v2y, g[:, 1] - v1y - v2y, g[:, 1] - v1y + v2y], 1)
    ay, ax = np.abs(qy - qy.min(1, keepdims=True)), np.abs(qx - qx.max(1, keepdims=True))
    ga = np.where(ay > thr, dt(-1000), qx).max(1)
    gb = np.where(ax > thr, dt(-1000), qy).max(1)
    m_mask = np.minimum(np.abs(ay - dt(0.1)).min(1), np.abs(ax - dt(0.1)).min(1)).astype(F64)
    d = np.stack([(gx - px) / pw, (gy - py) / ph, np.log(gw / pw), np.log(gh / ph), (ga - gx) / gw, (gb - gy) / gh], 1)
    out = (d - np.asarray(means, dt)[None]) / np.asarray(stds, dt)[None]
    return out, dict(mask=m_mask), dict(two_top=(ay <= dt(0.1)).sum(1) > 1, two_right=(ax <= dt(0.1)).sum(1) > 1)


def midpoint_decode(anchors, deltas, means, stds, wh_ratio_clip=CLIP_HI, dt=F64, mut=None):
    """hbb anchors (n, 4), deltas (n, 6) -> (n, 5)"""
    a = np.asarray(anchors, dt)
    d = _denorm(deltas, means, stds, 6, dt, mut)[:, 0]
    dw, dh, m_clamp, flags = _size_clamp(d[:, 2], d[:, 3], wh_ratio_clip, dt, mut)
    px, py = (a[:, 0] + a[:, 2]) * dt(0.5), (a[:, 1] + a[:, 3]) * dt(0.5)
    pw, ph = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    gw, gh = pw * np.exp(dw), ph * np.exp(dh)
    gx, gy = px + pw * d[:, 0], py + ph * d[:, 1]
    half = dt(0.5)
    x1, y1, x2, y2 = gx - gw * half, gy - gh * half, gx + gw * half, gy + gh * half
    da, db = d[:, 4], d[:, 5]
    m_dab = np.minimum(np.minimum(np.abs(da - half), np.abs(da + half)),
                       np.minimum(np.abs(db - half), np.abs(db + half))).astype(F64)
    flags["dab"] = (np.abs(da) > half) | (np.abs(db) > half)
    flags["dab_both"] = (np.abs(da) > half) & (np.abs(db) > half)
    if mut != "no_dab_clamp":
        da, db = np.clip(da, -half, half), np.clip(db, -half, half)
    # top, right, bottom, left vertex of the parallelogram, centred, stretched to equal half-diagonals
    cx = np.stack([gx + da * gw - gx, x2 - gx, gx - da * gw - gx, x1 - gx], 1)
    cy = np.stack([y1 - gy, gy + db * gh - gy, y2 - gy, gy - db * gh - gy], 1)
    ln = np.sqrt(cx * cx + cy * cy)
    mx = ln.max(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = mx / ln
        rx, ry = cx * sc + gx[:, None], cy * sc + gy[:, None]
        la, lb = np.maximum(ln[:, 0], ln[:, 2]), np.maximum(ln[:, 1], ln[:, 3])
        m_diag = (np.abs(la - lb) / mx[:, 0]).astype(F64)
        m_sep = (np.hypot(rx[:, 1] - rx[:, 0], ry[:, 1] - ry[:, 0]) / mx[:, 0]).astype(F64)
    # rectpoly2obb
    theta = np.arctan2(-(ry[:, 1] - ry[:, 0]), rx[:, 1] - rx[:, 0])
    c, s = np.cos(theta), np.sin(theta)
    x = (rx[:, 0] + rx[:, 1] + rx[:, 2] + rx[:, 3]) / dt(4)
    y = (ry[:, 0] + ry[:, 1] + ry[:, 2] + ry[:, 3]) / dt(4)
    ux, uy = rx - x[:, None], ry - y[:, None]
    vx, vy = ux * c[:, None] + uy * (-s[:, None]), ux * s[:, None] + uy * c[:, None]
    w, h = vx.max(1) - vx.min(1), vy.max(1) - vy.min(1)
    w, h, t, m_wh, m_wrap, swapped = _regular_obb(w, h, theta, dt, mut)
    flags["swapped"] = swapped
    nan_to = lambda m: np.where(np.isfinite(m), m, 0.0)     # noqa: E731  a degenerate row clears no margin
    return (np.stack([x, y, w, h, t], 1),
            dict(clamp=m_clamp, dab=m_dab, sep=nan_to(m_sep), diag=nan_to(m_diag), wh=nan_to(m_wh), wrap=nan_to(m_wrap)),
            flags)


def oriented_encode(rois, gt, means, stds, dt=F64, mut=None):
    """(n, 5), (n, 5) -> (n, 5)"""
    p, g = np.asarray(rois, dt), np.asarray(gt, dt)
    means, stds = _slots(means, stds, mut)
    px, py, pw, ph, pt = (p[:, k] for k in range(5))
    d1, m1 = _regular_theta(g[:, 4] - pt, dt, mut)
    d2, m2 = _regular_theta(g[:, 4] - pt + dt(PI / 2), dt, mut)
    first = np.abs(d1) < np.abs(d2)
    gw, gh, dth = np.where(first, g[:, 2], g[:, 3]), np.where(first, g[:, 3], g[:, 2]), np.where(first, d1, d2)
    ang = pt if mut == "cos_pt" else -pt
    c, s = np.cos(ang), np.sin(ang)
    ex, ey = g[:, 0] - px, g[:, 1] - py
    d = np.stack([(c * ex + s * ey) / pw, (-s * ex + c * ey) / ph, np.log(gw / pw), np.log(gh / ph), dth], 1)
    out = (d - np.asarray(means, dt)[None]) / np.asarray(stds, dt)[None]
    return out, dict(wrap=np.minimum(m1, m2), tie=np.abs(np.abs(d1) - np.abs(d2)).astype(F64)), dict(second=~first)


def oriented_decode(rois, deltas, means, stds, wh_ratio_clip=CLIP_HI, dt=F64, mut=None):
    """(n, 5), (n, 5C) -> (n, 5C)"""
    d = _denorm(deltas, means, stds, 5, dt, mut)
    r = _roi_rows(rois, d.shape[1], dt, mut)
    dw, dh, m_clamp, flags = _size_clamp(d[..., 2], d[..., 3], wh_ratio_clip, dt, mut)
    px, py, pw, ph, pt = (r[..., k] for k in range(5))
    ang = pt if mut == "cos_pt" else -pt
    c, s = np.cos(ang), np.sin(ang)
    gx = d[..., 0] * pw * c - d[..., 1] * ph * s + px
    gy = d[..., 0] * pw * s + d[..., 1] * ph * c + py
    gw, gh = pw * np.exp(dw), ph * np.exp(dh)
    t1, m1 = _regular_theta(d[..., 4] + pt, dt, mut)
    w, h, t, m_wh, m2, swapped = _regular_obb(gw, gh, t1, dt, mut)
    flags["swapped"] = swapped
    out = np.stack([gx, gy, w, h, t], -1).reshape(d.shape[0], -1)
    return out, dict(clamp=m_clamp, wh=m_wh, wrap=np.minimum(m1, m2)), flags


CODECS = dict(b2d=bbox2delta_rotated, d2b=delta2bbox_rotated, hbb=obb2hbb2obb, mid_enc=midpoint_encode,
              mid_dec=midpoint_decode, ori_enc=oriented_encode, ori_dec=oriented_decode)
DECODES = ("d2b", "hbb", "mid_dec", "ori_dec")


def retained(margins):
    """boxes whose every margin clears its threshold"""
    keep = None
    for name, m in margins.items():
        k = np.asarray(m) > RETAIN[name]
        keep = k if keep is None else keep & k
    return keep


# ------------------------------------------------------------------------------------------------------ error measures
def errors(codec, got, ref):
    """name of the column group -> error per box, the measures of the GPU tests:
    encodes: |err| / max(1, |ref|), one group per column; decodes: 'xywh' = the largest position / size error of the box
    relative to its largest |x|, |y|, w, h, and 'angle' = the angle error in radians, compared directly"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if codec in DECODES:
        g, r = got.reshape(-1, 5), ref.reshape(-1, 5)
        shape = (ref.shape[0], -1)
        scale = np.abs(r[:, :4]).max(1)
        return dict(xywh=(np.abs(g[:, :4] - r[:, :4]).max(1) / scale).reshape(shape),
                    angle=np.abs(g[:, 4] - r[:, 4]).reshape(shape))
    e = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    return {"col%d" % k: e[:, k:k + 1] for k in range(ref.shape[1])}


def worst(err, keep):
    """name -> max of the error over the retained boxes"""
    return {k: float(v[keep].max()) if keep.any() else 0.0 for k, v in err.items()}


BOUND_FACTOR = 4.0       # a different legal operation order plus a device libm within 2 ulp (tests/test_gpu_fcos.py)


# ------------------------------------------------------------------------------------------------------ fixtures
def _f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def _log_uniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), shape))


def _obbs(rng, n, side, angle=(-4.0, 4.0), centre=(100.0, 900.0)):
    return np.concatenate([rng.uniform(centre[0], centre[1], (n, 2)), _log_uniform(rng, side[0], side[1], (n, 2)),
                           rng.uniform(angle[0], angle[1], (n, 1))], 1)


def _normalise(target, means, stds):
    """the float32 network output whose denormalised value is `target` (up to its rounding)"""
    return _f32((target - np.asarray(means)) / np.asarray(stds))


def _size_targets(rng, shape, variant, small):
    """denormalised (dw, dh) targets.  'hi' (default clip, max_ratio 4.135): the rows of `small` (8-16 px) anchors reach
    the UPPER clamp with 60 % of their elements, up to 120 beyond it (an untrained head), and never shrink; every other
    anchor stays within +-0.6.  'lo' (clip 0.25, max_ratio 1.386, anchors >= 32 px): 6 % of the elements beyond each side"""
    if variant == "hi":
        mr = abs(math.log(CLIP_HI))
        calm = rng.uniform(-0.6, 0.6, shape)
        wild = np.where(rng.random(shape) < 0.6, mr + rng.uniform(0.01, 120.0, shape), rng.uniform(0.0, 1.0, shape))
        return np.where(small.reshape((-1,) + (1,) * (len(shape) - 1)), wild, calm)
    mr = abs(math.log(CLIP_LO))
    u = rng.random(shape)
    beyond = mr + rng.uniform(0.01, 120.0, shape)
    return np.where(u < 0.06, -beyond, np.where(u < 0.12, beyond, rng.uniform(-1.3, 1.3, shape)))


def _anchor_sides(rng, n, variant, small_share):
    small = rng.random(n) < small_share if variant == "hi" else np.zeros(n, bool)
    if variant == "hi":
        sides = np.where(small[:, None], rng.uniform(8.0, 16.0, (n, 2)), _log_uniform(rng, 40.0, 200.0, (n, 2)))
    else:
        sides = _log_uniform(rng, 32.0, 128.0, (n, 2))
    return sides, small


def _draw_rotated_decode(rng, n, variant, C, angle_span):
    sides, small = _anchor_sides(rng, n, variant, 0.15)
    rois = np.concatenate([rng.uniform(250, 750, (n, 2)), sides, rng.uniform(-4, 4, (n, 1))], 1)
    t = np.empty((n, C, 5))
    t[..., :2] = rng.uniform(-0.8, 0.8, (n, C, 2))
    t[..., 2:4] = _size_targets(rng, (n, C, 2), variant, small)
    t[..., 4] = rng.uniform(-angle_span, angle_span, (n, C))
    return _f32(rois), _normalise(t, M5, S5).reshape(n, C * 5)


def _draw_mid_decode(rng, n, variant):
    sides, small = _anchor_sides(rng, n, variant, 0.3)
    ctr = rng.uniform(250, 750, (n, 2))
    anchors = np.concatenate([ctr - sides / 2, ctr + sides / 2], 1)
    t = np.empty((n, 6))
    t[:, :2] = rng.uniform(-0.5, 0.5, (n, 2))
    t[:, 2:4] = _size_targets(rng, (n, 2), variant, small)
    t[:, 4:] = rng.uniform(-0.45, 0.45, (n, 2))
    u = rng.random(n)
    beyond = (0.5 + rng.uniform(0.01, 15.0, n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    # da alone or db alone.  Both at once leaves a corner pair: (+, -) and (-, +) make two vertices coincide (a segment,
    # no box), (+, +) and (-, -) give the axis-aligned box with its angle ON a wrap point, which float64 cannot referee:
    # those two are rows 14-17 of the edge case `mid_dec_edges`, compared with the float32 composition
    t[:, 4] = np.where(u < 0.12, beyond, t[:, 4])
    t[:, 5] = np.where((u >= 0.12) & (u < 0.24), beyond, t[:, 5])
    return _f32(anchors), _normalise(t, M6, S6)


def _draw_mid_encode(rng, n):
    """gts 8-300 px, angle in [-pi/2, pi/2); every 8th row nearly axis-aligned (about 0 or about -pi/2), its second
    top-most vertex 0.05-0.2 px from the extreme: the rows on which the 0.1 masks decide"""
    g = _obbs(rng, n, (8.0, 300.0), (-PI / 2, PI / 2), (330.0, 690.0))     # the jittered anchors stay within 1024
    near = np.arange(n) % 8 == 3
    base = np.where(rng.random(n) < 0.5, 0.0, -PI / 2)
    side = np.where(base == 0.0, g[:, 2], g[:, 3])
    tilt = np.arcsin(_log_uniform(rng, 0.05, 0.2, n) / side) * np.where((rng.random(n) < 0.5) & (base == 0.0), -1.0, 1.0)
    g[:, 4] = np.where(near, base + tilt, g[:, 4])
    g = _f32(g).astype(F64)
    c, s = np.cos(g[:, 4]), np.sin(g[:, 4])
    xb = np.abs(g[:, 2] / 2 * c) + np.abs(g[:, 3] / 2 * s)
    yb = np.abs(g[:, 2] / 2 * s) + np.abs(g[:, 3] / 2 * c)
    wh = np.stack([xb, yb], 1) * 2
    ctr = g[:, :2] + rng.uniform(-0.1, 0.1, (n, 2)) * wh
    half = wh / 2 * np.exp(rng.uniform(-0.3, 0.3, (n, 2)))
    return _f32(np.concatenate([ctr - half, ctr + half], 1)), _f32(g), near


def _draw_pairs(rng, n):
    """(proposal, gt) rows of the two 5-parameter encodes: both angles in [-4, 4]"""
    p = _obbs(rng, n, (8.0, 300.0), centre=(160.0, 860.0))
    g = p.copy()
    g[:, :2] += rng.uniform(-0.5, 0.5, (n, 2)) * p[:, 2:4]
    g[:, 2:4] = np.clip(p[:, 2:4] * np.exp(rng.uniform(-1.0, 1.0, (n, 2))), 8.0, 600.0)
    g[:, 4] = rng.uniform(-4, 4, n)
    return _f32(p), _f32(g)


# name -> (codec, seed, variant, ncls).  n = N_ROWS is no multiple of 3 or 15
FIXTURES = {
    "b2d": ("b2d", 11, None, 1), "ori_enc": ("ori_enc", 12, None, 1), "mid_enc": ("mid_enc", 13, None, 1),
    "hbb": ("hbb", 14, None, 1),
    "d2b_hi3": ("d2b", 21, "hi", 3), "d2b_lo15": ("d2b", 22, "lo", 15), "d2b_lo1": ("d2b", 23, "lo", 1),
    "ori_dec_hi3": ("ori_dec", 31, "hi", 3), "ori_dec_lo15": ("ori_dec", 32, "lo", 15), "ori_dec_lo1": ("ori_dec", 33, "lo", 1),
    "mid_dec_hi": ("mid_dec", 41, "hi", 1), "mid_dec_lo": ("mid_dec", 42, "lo", 1),
}
ENTRY_POINT = dict(b2d="jdet_bbox2delta_rotated", d2b="jdet_delta2bbox_rotated", hbb="jdet_obb2hbb2obb",
                   mid_enc="jdet_midpoint_offset_encode", mid_dec="jdet_midpoint_offset_decode",
                   ori_enc="jdet_oriented_delta_encode", ori_dec="jdet_oriented_delta_decode")


class Fixture:
    """args: the float32 input arrays; kw: means / stds / wh_ratio_clip; ref, margins, flags: the float64 restatement;
    twin: the float32 one; keep: the retained boxes, (n, C); e32: column group -> the twin's worst error on them;
    drawn_ok: the share of the drawn rows that met the construction limits"""

    def run(self, dt=F64, mut=None, args=None):
        return CODECS[self.codec](*(self.args if args is None else args), dt=dt, mut=mut, **self.kw)

    def bound(self):
        return {k: BOUND_FACTOR * v for k, v in self.e32.items()}

    def broken_share(self, out, rows=None):
        """the share of the retained boxes (of `rows`) on which `out` breaks the GPU tests' bound"""
        err, b = errors(self.codec, out, self.ref), self.bound()
        bad = np.zeros_like(self.keep)
        for k, v in err.items():
            bad |= ~(v <= b[k])                         # NaN breaks it
        sel = self.keep if rows is None else self.keep & rows[:, None]
        return float(bad[sel].mean())


def _construction_ok(codec, out):
    """rows whose every decoded box has its sides in [SIDE_MIN, COORD_MAX] and its centre in [0, COORD_MAX]"""
    if codec not in DECODES:
        return np.ones(out.shape[0], bool)
    b = out.reshape(out.shape[0], -1, 5)
    with np.errstate(invalid="ignore"):
        ok = (b[..., 2:4] >= SIDE_MIN).all(-1) & (b[..., 2:4] <= COORD_MAX).all(-1) & \
             (b[..., :2] >= 0).all(-1) & (b[..., :2] <= COORD_MAX).all(-1)
    return ok.all(1)


@functools.lru_cache(maxsize=None)
def fixture(name, n=N_ROWS):
    codec, seed, variant, C = FIXTURES[name]
    rng = np.random.default_rng(seed)
    f = Fixture()
    f.name, f.codec, f.ncls, f.variant, f.slice = name, codec, C, variant, None
    clip = CLIP_LO if variant == "lo" else CLIP_HI
    draw = 2 * n
    if codec in ("b2d", "ori_enc"):
        args, f.kw = _draw_pairs(rng, draw), dict(means=M5, stds=S5)
    elif codec == "hbb":
        args, f.kw = (_f32(_obbs(rng, draw, (8.0, 512.0))),), {}
    elif codec == "mid_enc":
        a, g, near = _draw_mid_encode(rng, draw)
        args, f.kw, f.slice = (a, g), dict(means=M6, stds=S6), near
    elif codec == "mid_dec":
        draw = 4 * n
        args, f.kw = _draw_mid_decode(rng, draw, variant), dict(means=M6, stds=S6, wh_ratio_clip=clip)
    else:
        args = _draw_rotated_decode(rng, draw, variant, C, 1.5 if codec == "d2b" else 2.5)
        f.kw = dict(means=M5, stds=S5, wh_ratio_clip=clip)
    ok = _construction_ok(codec, CODECS[codec](*args, **f.kw)[0])
    f.drawn_ok = float(ok.mean())
    rows = np.flatnonzero(ok)[:n]
    assert rows.size == n, "%s: only %d of %d drawn rows meet the construction limits" % (name, rows.size, draw)
    f.args = tuple(np.ascontiguousarray(a[rows]) for a in args)
    if f.slice is not None:
        f.slice = f.slice[rows]
    f.ref, f.margins, f.flags = f.run()
    f.twin = f.run(F32)[0]
    assert f.twin.dtype == F32
    f.keep = retained(f.margins).reshape(n, -1)
    f.flags = {k: np.asarray(v).reshape(n, -1) for k, v in f.flags.items()}
    f.e32 = worst(errors(codec, f.twin, f.ref), f.keep)
    for a in f.args + (f.ref, f.twin, f.keep):
        a.setflags(write=False)
    return f


# ------------------------------------------------------------------------------------------------------ edge fixture
# The exact cases.  In float64 these fp32 ties are no ties, so the reference of the edge rows is the float32 composition
# (the torch general routes, same IEEE operations in the same order as the kernels): identical branch, values within 2 ulp.
EDGE_M5, EDGE_S5 = (0.0,) * 5, (1.0, 1.0, 1.0, 1.0, 1.0)
EDGE_M6, EDGE_S6 = (0.0,) * 6, (1.0,) * 6
HALF_PI32, QUARTER_PI32 = float(F32(PI / 2)), float(F32(PI / 4))


def edge_cases():
    """name -> (codec, args, kw): some hundred hand-built rows.  Means 0 and stds 1, so that a delta IS its denormalised value
    and `exactly on the clamp` can be written down"""
    mr = float(F32(abs(math.log(CLIP_HI))))
    k5, k6 = dict(means=EDGE_M5, stds=EDGE_S5), dict(means=EDGE_M6, stds=EDGE_S6)
    out = {}
    # axis-aligned gts at theta = 0: two vertices on the top edge and two on the right edge, da = db = +0.5
    g = [[100, 200, 40, 20, 0], [33.25, 71.5, 17.5, 60.25, 0], [640, 12.125, 300, 9, 0], [512, 512, 64, 64, 0],
         [100, 200, 40, 20, -HALF_PI32], [77.5, 90, 8, 8, 0], [300, 300, 128, 32, 0], [10, 900, 12, 250, 0]]
    g = np.asarray(g, F64)
    hbb = np.stack([g[:, 0] - 40, g[:, 1] - 30, g[:, 0] + 50, g[:, 1] + 45], 1)
    out["mid_enc_axis"] = ("mid_enc", (_f32(hbb), _f32(g)), k6)
    # oriented decode: square boxes (pw = ph, dw = dh = 0: the tie of regular_obb, swap and + pi/2), dw exactly on
    # +-max_ratio and one ulp beyond, angles exactly on a wrap point (sum -pi/2, +pi/2, and 0 with the quarter turn)
    r = [[100, 100, 32, 32, 0.25], [200, 150, 64, 64, -HALF_PI32], [300, 300, 16, 16, HALF_PI32], [50, 60, 24, 24, 0],
         [400, 400, 12, 10, 0.5], [400, 400, 12, 10, 0.5], [400, 400, 10, 12, 0.5], [400, 400, 10, 12, 0.5],
         [500, 500, 40, 20, -HALF_PI32], [500, 500, 40, 20, HALF_PI32], [500, 500, 20, 40, 0], [500, 500, 20, 40, -1.0],
         [600, 600, 48, 48, 1.0]]
    up, dn = float(np.nextafter(F32(mr), F32(10))), float(np.nextafter(F32(mr), F32(0)))
    d = [[0, 0, 0, 0, 0], [0.5, -0.25, 0, 0, 0], [0, 0, 0, 0, 0], [0.125, 0.25, 0, 0, 0],
         [0, 0, mr, 0, 0.25], [0, 0, up, dn, 0.25], [0, 0, 0, mr, 0.25], [0, 0, dn, up, 0.25],
         [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 1.0],
         [0, 0, 0, 0, -1.0]]
    out["ori_dec_edges"] = ("ori_dec", (_f32(r), _f32(d)), dict(k5, wh_ratio_clip=CLIP_HI))
    # delta2bbox_rotated folds into [-pi/4, 3pi/4): the same rows, and angle sums exactly on its wrap points (-pi/4 twice, fp32 pi - pi/4)
    r2 = r + [[700, 700, 30, 20, -QUARTER_PI32], [700, 700, 30, 20, QUARTER_PI32], [700, 700, 30, 20, 3 * QUARTER_PI32]]
    d2 = d + [[0, 0, 0, 0, 0], [0, 0, 0, 0, -0.5], [0.25, 0.5, 0.125, -0.125, 0]]
    # ... and its own lower clamp: dw exactly -max_ratio, one ulp beyond and one ulp short of it (a 160 x 192 roi)
    r2 = r2 + [[800, 800, 160, 192, 0.5]] * 2
    d2 = d2 + [[0, 0, -mr, 0, 0.25], [0, 0, -up, -dn, 0.25]]
    out["d2b_edges"] = ("d2b", (_f32(r2), _f32(d2)), dict(k5, wh_ratio_clip=CLIP_HI))
    out["d2b_n1"] = ("d2b", (_f32(r[4:5]), _f32([d[4] + d[5] + d[1]])), dict(k5, wh_ratio_clip=CLIP_HI))      # 3 classes
    dl = np.asarray(d, F64)
    dl[:, 2:4] *= -1                                       # the lower clamp: exactly on it, one ulp on either side
    big = np.asarray(r, F64)
    big[:, 2:4] *= 16                                      # sides stay >= 2 px at exp(-4.135)
    out["ori_dec_lower"] = ("ori_dec", (_f32(big), _f32(dl)), dict(k5, wh_ratio_clip=CLIP_HI))
    # n = 1; n = 0 (one and fifteen classes wide)
    out["ori_dec_n1"] = ("ori_dec", (_f32(r[:1]), _f32(d[1:2])), dict(k5, wh_ratio_clip=CLIP_HI))
    out["ori_dec_n0"] = ("ori_dec", (_f32(r[:0]).reshape(0, 5), _f32(d[:0]).reshape(0, 5)), dict(k5, wh_ratio_clip=CLIP_HI))
    out["d2b_n0"] = ("d2b", (_f32(r[:0]).reshape(0, 5), np.zeros((0, 15), F32)), dict(k5, wh_ratio_clip=CLIP_HI))
    # oriented encode at the fp32 +-pi/4 tie: gt angle - roi angle = +-pi/4 (fp32) exactly, and its neighbours
    p = [[100, 100, 30, 20, 0], [100, 100, 30, 20, 0], [100, 100, 30, 20, 0], [100, 100, 30, 20, 0],
         [100, 100, 30, 20, 0], [100, 100, 30, 20, 0], [200, 200, 16, 48, 0.5], [200, 200, 16, 48, HALF_PI32]]
    q = QUARTER_PI32
    gg = [[110, 95, 40, 25, q], [110, 95, 40, 25, -q], [110, 95, 40, 25, float(np.nextafter(F32(q), F32(0)))],
          [110, 95, 40, 25, float(np.nextafter(F32(q), F32(1)))], [110, 95, 40, 25, HALF_PI32], [110, 95, 40, 25, -HALF_PI32],
          [190, 210, 20, 40, 0.5], [190, 210, 20, 40, 0.0]]
    out["ori_enc_ties"] = ("ori_enc", (_f32(p), _f32(gg)), k5)
    out["ori_enc_n1"] = ("ori_enc", (_f32(p[6:7]), _f32(gg[6:7])), k5)
    out["ori_enc_n0"] = ("ori_enc", (np.zeros((0, 5), F32), np.zeros((0, 5), F32)), k5)
    out["b2d_edges"] = ("b2d", (_f32(p), _f32(gg)), k5)
    out["b2d_n1"] = ("b2d", (_f32(p[1:2]), _f32(gg[1:2])), k5)
    out["b2d_n0"] = ("b2d", (np.zeros((0, 5), F32), np.zeros((0, 5), F32)), k5)
    # midpoint decode: da / db exactly +-0.5 and one ulp beyond, alone and together (da = db = +0.5 is the axis-aligned
    # box: the top vertex is the top-right corner), dw on the clamp, square anchors with dw = dh = 0.  Rows 14-17: BOTH
    # da and db strictly beyond the clamp -- (+, +) puts the top vertex on the top-right corner, theta = atan2f(-gh, 0) =
    # -pi/2 exactly; (-, -) gives the axis-aligned box at theta = 0 -- each on a wide and on a tall anchor (with and
    # without the swap; both tall rows end ON the fold of regular_theta, at -pi/2).  Rows 18-19: the lower size clamp
    a = [[100, 100, 164, 132]] * 8 + [[200, 200, 232, 232]] * 4 + [[300, 300, 310, 312]] * 2
    a = a + [[100, 100, 164, 132], [100, 100, 132, 164]] * 2 + [[400, 400, 656, 592]] * 2
    hp, hm = float(np.nextafter(F32(0.5), F32(1))), float(np.nextafter(F32(0.5), F32(0)))
    d6 = [[0, 0, 0, 0, 0.5, 0.25], [0, 0, 0, 0, 0.25, 0.5], [0, 0, 0, 0, -0.5, 0.25], [0, 0, 0, 0, 0.25, -0.5],
          [0, 0, 0, 0, hp, 0.125], [0, 0, 0, 0, hm, 0.125], [0.125, -0.25, 0.5, -0.5, 3.0, 0.125], [0, 0, 0, 0, -0.5, -0.5],
          [0, 0, 0, 0, 0.25, 0.25], [0, 0, 0, 0, 0.0, 0.0], [0, 0, 0, 0, -0.25, 0.375], [0, 0, 0, 0, 0.5, 0.0],
          [0, 0, mr, mr, 0.25, 0.125], [0, 0, up, dn, -0.125, 0.25],
          [0, 0, 0, 0, 0.75, 2.0], [0, 0, 0, 0, 0.75, 2.0], [0, 0, 0, 0, -3.0, -0.625], [0, 0, 0, 0, -3.0, -0.625],
          [0, 0, -mr, -mr, 0.25, 0.125], [0, 0, -up, -dn, -0.125, 0.25]]
    out["mid_dec_edges"] = ("mid_dec", (_f32(a), _f32(d6)), dict(k6, wh_ratio_clip=CLIP_HI))
    out["mid_dec_n1"] = ("mid_dec", (_f32(a[:1]), _f32(d6[:1])), dict(k6, wh_ratio_clip=CLIP_HI))
    out["mid_dec_n0"] = ("mid_dec", (np.zeros((0, 4), F32), np.zeros((0, 6), F32)), dict(k6, wh_ratio_clip=CLIP_HI))
    out["mid_enc_n1"] = ("mid_enc", (_f32(hbb[1:2]), _f32(g[1:2])), k6)
    out["mid_enc_n0"] = ("mid_enc", (np.zeros((0, 4), F32), np.zeros((0, 5), F32)), k6)
    # obb2hbb2obb: ww == hh (squares at 0, at pi/4 where w = h, swapped sides at pi/2), n = 1, n = 0
    s = [[100, 100, 32, 32, 0], [100, 100, 32, 32, q], [200, 100, 48, 16, q], [200, 100, 16, 48, -q], [50, 50, 8, 8, HALF_PI32],
         [300, 300, 40, 20, 0], [300, 300, 20, 40, 0], [300, 300, 40, 20, HALF_PI32]]
    out["hbb_squares"] = ("hbb", (_f32(s),), {})
    out["hbb_n1"] = ("hbb", (_f32(s[1:2]),), {})
    out["hbb_n0"] = ("hbb", (np.zeros((0, 5), F32),), {})
    return out
