"""Restatements of the rotated FCOS pieces, written from the reference's text, and the fixtures of the FCOS tests.

  targets(...)        FCOSHead._get_target_single (python/jdet/models/roi_heads/fcos_head.py:L599-670) + mintheta_obb
                      (models/boxes/box_ops.py:L679-692) in numpy float64, with the rules include/jdet_hip.h fixes:
                      equal areas to the lower gt index, background rows zero, an image without gts all background.
                      It also returns the margins by which every decision clears its threshold.
  poly_iou_loss(...)  poly_iou_loss (models/losses/poly_iou_loss.py:L39-123) in torch, in float64 or float32: the tensor
                      program as written, differentiated by torch autograd; the Graham scan (ops/convex_sort.py) is the
                      python loop `graham_scan` below, every operation rounded in the working precision.

Pinned by restatement only: Jittor is not importable here.  The fixtures are drawn and FILTERED here, at generation,
so the tests drop no row: target fixtures keep every comparison at least 1e-3 px from its threshold, loss fixtures keep
the float64 IoU at or above 0.05 and the float64 and float32 restatements on identical mask and hull decisions."""
import functools
import math

import numpy as np
import torch

F32 = np.float32
INF = 1e8
STRIDES = (8, 16, 32, 64, 128)
IMG = 128
SIZES = tuple((IMG // s, IMG // s) for s in STRIDES)         # 16, 8, 4, 2, 1 -> 341 points
# the reference's ranges scaled to the 128 px image (/ 4), so that every level but the last can win a point
RANGES = ((-1, 16), (16, 32), (32, 64), (64, 128), (128, INF))
# below 1 on purpose: with hi = 2 x stride the inside and range tests already force |rx|, |ry| < stride, so the
# reference's 1.5 could never reject a point here; 0.6 x stride does (the fixtures assert it)
RADIUS = 0.6
NUM_CLASSES = 15


def points_of(sizes=SIZES, strides=STRIDES):
    """(N, 2) float64 points, (N,) level index -- fcos_head.py:L521-533"""
    pts, lvl = [], []
    for l, ((h, w), s) in enumerate(zip(sizes, strides)):
        y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        pts.append(np.stack([x.ravel() * s, y.ravel() * s], -1) + s // 2)
        lvl.append(np.full(h * w, l))
    return np.concatenate(pts).astype(np.float64), np.concatenate(lvl)


def regular_theta(theta, dt=np.float64):
    start, cycle = dt(-math.pi / 2), dt(math.pi)
    return np.mod(theta - start, cycle) + start             # floor-mod, as torch.remainder


def mintheta_obb(obbs, dt=np.float64):
    """-> (boxes, |theta1| - |theta2|)"""
    o = np.asarray(obbs, dt)
    pi = 3.141592
    t1 = regular_theta(o[:, 4], dt)
    t2 = regular_theta(o[:, 4] + dt(pi / 2), dt)
    first = np.abs(t1) < np.abs(t2)
    out = np.stack([o[:, 0], o[:, 1], np.where(first, o[:, 2], o[:, 3]), np.where(first, o[:, 3], o[:, 2]),
                    np.where(first, t1, t2)], -1)
    return out, np.abs(t1) - np.abs(t2)


def targets(gts, gt_labels, norm_on_bbox, center_sampling, sizes=SIZES, strides=STRIDES, ranges=RANGES, radius=RADIUS,
            num_classes=NUM_CLASSES):
    """one image.  gts (K, 5) fp32 values, gt_labels (K,) 1-based -> dict(labels, inds, bbox_targets, centerness, margin,
    theta_gap, positives)"""
    pts, lvl = points_of(sizes, strides)
    N, K = pts.shape[0], len(gts)
    out = dict(labels=np.full(N, num_classes, np.int32), inds=np.full(N, -1, np.int32),
               bbox_targets=np.zeros((N, 5)), centerness=np.zeros(N), margin=np.inf, theta_gap=np.inf, positives=0)
    if K == 0:
        return out
    g = np.asarray(gts, np.float64)
    areas = (np.asarray(gts, F32)[:, 2] * np.asarray(gts, F32)[:, 3]).astype(np.float64)    # fp32 product, as compared
    m, gap = mintheta_obb(g)
    m32, _ = mintheta_obb(gts, F32)
    assert np.array_equal(m[:, 2], m32[:, 2].astype(np.float64)), "float32 and float64 mintheta_obb swap differently"
    cos, sin = np.cos(m[:, 4]), np.sin(m[:, 4])
    off = pts[:, None, :] - m[None, :, :2]
    rx = cos[None] * off[..., 0] - sin[None] * off[..., 1]
    ry = sin[None] * off[..., 0] + cos[None] * off[..., 1]
    l, r = m[None, :, 2] / 2 + rx, m[None, :, 2] / 2 - rx
    t, b = m[None, :, 3] / 2 + ry, m[None, :, 3] / 2 - ry
    d = np.stack([l, t, r, b], -1)
    dmin, dmax = d.min(-1), d.max(-1)
    lo = np.asarray([ranges[i][0] for i in lvl], np.float64)[:, None]
    hi = np.asarray([ranges[i][1] for i in lvl], np.float64)[:, None]
    rad = np.asarray([strides[i] * radius for i in lvl], np.float64)[:, None]
    inside = dmin > 0
    margins = [np.abs(dmin), np.abs(dmax - lo), np.abs(dmax - hi)]
    # center sampling is part of every fixture's conditions, whichever way a test sets the flag
    margins += [np.abs(np.abs(rx) - rad), np.abs(np.abs(ry) - rad)]
    if center_sampling:
        inside = inside & (np.abs(rx) < rad) & (np.abs(ry) < rad)
    ok = inside & (dmax >= lo) & (dmax <= hi)
    a = np.where(ok, areas[None], np.inf)
    inds = np.argmin(a, 1)                                   # first minimum: the lower index on equal areas
    pos = ok.any(1)
    rows = np.flatnonzero(pos)
    bt = np.concatenate([d[rows, inds[rows]], m[inds[rows], 4:5]], 1)
    if norm_on_bbox:
        bt[:, :4] /= np.asarray(strides, np.float64)[lvl[rows]][:, None]
    out["labels"][rows] = np.asarray(gt_labels)[inds[rows]] - 1
    out["inds"][rows] = inds[rows]
    out["bbox_targets"][rows] = bt
    out["centerness"][rows] = np.sqrt(np.minimum(bt[:, 0], bt[:, 2]) / np.maximum(bt[:, 0], bt[:, 2])
                                      * (np.minimum(bt[:, 1], bt[:, 3]) / np.maximum(bt[:, 1], bt[:, 3])))
    out.update(margin=float(min(x.min() for x in margins)), theta_gap=float(np.abs(gap).min()), positives=int(pos.sum()))
    return out


def _draw_gts(rng, K):
    """K gts drawn one by one; a gt is kept when each of its comparisons clears its threshold by 1e-3 px, its angle
    choice by 1e-5 and its fp32 area differs from those kept before"""
    keep = []
    while len(keep) < K:
        c = rng.uniform(8, IMG - 8, 2)
        wh = np.exp(rng.uniform(np.log(6.0), np.log(150.0), 2))
        g = np.concatenate([c, wh, rng.uniform(-np.pi / 2, np.pi / 2, 1)]).astype(F32)[None]
        try:
            r = targets(g, np.ones(1, np.int32), False, False)
        except AssertionError:
            continue
        if r["margin"] < 1e-3 or r["theta_gap"] < 1e-5 or abs(float(g[0, 4])) < 1e-3 or \
                abs(abs(float(g[0, 4])) - math.pi / 2) < 1e-3:
            continue
        if any(F32(k[0, 2]) * F32(k[0, 3]) == F32(g[0, 2]) * F32(g[0, 3]) for k in keep):
            continue
        keep.append(g)
    return np.concatenate(keep, 0)


# name -> (seed, gt count per image); "tie" repeats its gt 2 as gt 4 (same area, same box: the lower index wins)
TARGET_FIXTURES = {"k7_k0": (24, (7, 0)), "k70": (12, (70,)), "k1": (13, (1,)), "tie": (27, (8,))}


@functools.lru_cache(maxsize=None)
def target_fixture(name):
    """-> (list of (K_b, 5) fp32 gts, list of (K_b,) int32 labels), read-only"""
    seed, counts = TARGET_FIXTURES[name]
    rng = np.random.default_rng(seed)
    gts, labels = [], []
    for K in counts:
        if name == "tie":
            g = _draw_gts(rng, 7)
            g = np.concatenate([g[:4], g[2:3], g[4:]], 0)    # gt 4 == gt 2
        else:
            g = _draw_gts(rng, K) if K else np.zeros((0, 5), F32)
        lab = rng.integers(1, NUM_CLASSES + 1, len(g)).astype(np.int32)
        if name == "tie":
            lab[4] = lab[2] % NUM_CLASSES + 1                # a different class, so the label tells who won
        g.setflags(write=False)
        lab.setflags(write=False)
        gts.append(g)
        labels.append(lab)
    return gts, labels


# ------------------------------------------------------------------------------------------------- polygon IoU loss
def graham_scan(pts, masks, dt):
    """the scan of csrc/graham_scan.h (ops/convex_sort.py:L4-65, L159-194) on one point set, every operation in `dt`:
    (n + 1,) indices, circular, -1 padded"""
    p, n = np.asarray(pts, dt), len(pts)
    m = np.asarray(masks, dt)
    v = m * p[:, 1] + (dt(1) - m) * dt(10000000.0)
    start = int(np.argmin(v))
    d = p - p[start]
    c = d[:, 0] / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + dt(0.000001))
    order = np.argsort(-c, kind="stable")
    idx = [start]
    for j in order:
        j = int(j)
        if j == start or m[j] < 0.5:
            continue
        x0, y0 = p[j]
        x1, y1 = p[idx[-1]]
        if float((x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0)) < 0.000001:
            continue
        if len(idx) < 3:
            idx.append(j)
            continue
        while True:
            x1, y1 = p[idx[-1]]
            x2, y2 = p[idx[-2]]
            if (x1 - x2) * (y0 - y2) - (y1 - y2) * (x0 - x2) >= 0:
                idx.append(j)
                break
            if len(idx) <= 2:
                idx[-1] = j
                break
            idx.pop()
    idx.append(idx[0])
    return np.asarray(idx + [-1] * (n + 1 - len(idx)), np.int64)


def obb2poly(b):
    c, w, h, th = torch.split(b, [2, 1, 1, 1], dim=-1)
    Cos, Sin = torch.cos(th), torch.sin(th)
    v1 = torch.cat([w / 2 * Cos, -w / 2 * Sin], dim=-1)
    v2 = torch.cat([-h / 2 * Sin, -h / 2 * Cos], dim=-1)
    return torch.cat([c + v1 + v2, c + v1 - v2, c - v1 - v2, c - v1 + v2], dim=-1)


def poly_iou_loss(pred, target, weight=None, linear=False, eps=1e-6, dtype=torch.float64):
    """-> dict(loss (P,), grad (P, 5), iou (P,), masks (P, 24) bool, index (P, 25)) as numpy, computed in `dtype` from
    the given (fp32) values"""
    p = torch.from_numpy(np.array(pred)).to(dtype).clone().requires_grad_(True)
    t = torch.from_numpy(np.array(target)).to(dtype)
    a1, a2 = p[:, 2] * p[:, 3], t[:, 2] * t[:, 3]
    pts1, pts2 = obb2poly(p).view(-1, 4, 2), obb2poly(t).view(-1, 4, 2)
    l1 = torch.cat([pts1, torch.roll(pts1, -1, dims=1)], dim=2).unsqueeze(2)
    l2 = torch.cat([pts2, torch.roll(pts2, -1, dims=1)], dim=2).unsqueeze(1)
    x1, y1, x2, y2 = l1.unbind(dim=-1)
    x3, y3, x4, y4 = l2.unbind(dim=-1)
    num = (x1 - x2) * (y3 - y4) - (y1 - y2) * (x3 - x4)
    den_t = (x1 - x3) * (y3 - y4) - (y1 - y3) * (x3 - x4)
    with torch.no_grad():
        den_u = (x2 - x1) * (y1 - y3) - (y2 - y1) * (x1 - x3)
        tt, uu = den_t / num, den_u / num
        mask_inter = (tt > 0) & (tt < 1) & (uu > 0) & (uu < 1)
        tri1 = 0.5 * torch.abs((x3 - x1) * (y4 - y1) - (y3 - y1) * (x4 - x1))
        inside1 = torch.abs(tri1.sum(dim=-1) - a2[:, None]) < 1e-3 * a2[:, None]
        tri2 = 0.5 * torch.abs((x1 - x3) * (y2 - y3) - (x2 - x3) * (y1 - y3))
        inside2 = torch.abs(tri2.sum(dim=-2) - a1[:, None]) < 1e-3 * a1[:, None]
    te = den_t / (num + eps)
    inter = torch.stack([x1 + te * (x2 - x1), y1 + te * (y2 - y1)], dim=-1).view(-1, 16, 2)
    P = p.shape[0]
    all_pts = torch.cat([inter, pts1, pts2], dim=1)
    masks = torch.cat([mask_inter.reshape(P, 16), inside1, inside2], dim=1)
    dt = np.float64 if dtype == torch.float64 else np.float32
    pn, mn = all_pts.detach().numpy(), masks.numpy()
    index = np.stack([graham_scan(pn[i], mn[i], dt) for i in range(P)]) if P else np.zeros((0, 25), np.int64)
    gidx = torch.from_numpy(np.where(index < 0, 24, index))[..., None].repeat(1, 1, 2)
    polys = torch.gather(torch.cat([all_pts, all_pts.new_zeros((P, 1, 2))], dim=1), 1, gidx)
    xyxy = polys[:, :-1, 0] * polys[:, 1:, 1] - polys[:, :-1, 1] * polys[:, 1:, 0]
    overlap = 0.5 * torch.abs(xyxy.sum(dim=-1))
    iou = (overlap / (a1 + a2 - overlap + eps)).clamp(min=eps)
    loss = 1 - iou if linear else -iou.log()
    if weight is not None:
        loss = loss * torch.from_numpy(np.array(weight)).to(dtype)
    loss.sum().backward()
    return dict(loss=loss.detach().numpy(), grad=p.grad.numpy(), iou=iou.detach().numpy(), masks=mn, index=index)


LOSS_ROWS = 257


@functools.lru_cache(maxsize=None)
def loss_fixture(rows=LOSS_ROWS, seed=5):
    """(pred, target) fp32 (rows, 5), read-only, and the float64 / float32 restatements of the plain (-log, unweighted)
    loss on them.  Pairs as in the experiment the tolerance comes from: centres jittered +-15 px, sizes 8-68 px, angle
    difference +-0.4 rad; kept when the float64 IoU >= 0.05 and both precisions decide every mask and hull index alike"""
    rng = np.random.default_rng(seed)
    n = rows * 2
    tgt = np.concatenate([rng.uniform(60, 200, (n, 2)), rng.uniform(8, 68, (n, 2)),
                          rng.uniform(-np.pi / 2, np.pi / 2, (n, 1))], 1).astype(F32)
    prd = np.concatenate([tgt[:, :2] + rng.uniform(-15, 15, (n, 2)), rng.uniform(8, 68, (n, 2)),
                          tgt[:, 4:] + rng.uniform(-0.4, 0.4, (n, 1))], 1).astype(F32)
    r64, r32 = poly_iou_loss(prd, tgt), poly_iou_loss(prd, tgt, dtype=torch.float32)
    ok = (r64["iou"] >= 0.05) & (r64["masks"] == r32["masks"]).all(1) & (r64["index"] == r32["index"]).all(1)
    sel = np.flatnonzero(ok)[:rows]
    assert sel.size == rows, "only %d of %d drawn pairs pass the filter" % (sel.size, n)
    prd, tgt = prd[sel].copy(), tgt[sel].copy()
    prd.setflags(write=False)
    tgt.setflags(write=False)
    return prd, tgt, float(ok.mean())


def row_errors(got_loss, got_grad, ref):
    """(max |loss - ref|, max over rows of max|grad - ref| / max|ref grad of the row|)"""
    e_loss = float(np.abs(np.asarray(got_loss, np.float64) - ref["loss"]).max())
    gmax = np.abs(ref["grad"]).max(1)
    e_grad = float((np.abs(np.asarray(got_grad, np.float64) - ref["grad"]).max(1) / gmax).max())
    return e_loss, e_grad


@functools.lru_cache(maxsize=None)
def loss_reference(linear=False, weighted=False):
    """the float64 restatement on the fixture and the float32 restatement's own error against it: (ref64, E_loss, E_grad)"""
    prd, tgt, _ = loss_fixture()
    w = loss_weights() if weighted else None
    r64 = poly_iou_loss(prd, tgt, w, linear)
    r32 = poly_iou_loss(prd, tgt, w, linear, dtype=torch.float32)
    assert np.array_equal(r64["index"], r32["index"]) and np.array_equal(r64["masks"], r32["masks"])
    return (r64,) + row_errors(r32["loss"], r32["grad"], r64)


def loss_weights():
    w = np.random.default_rng(6).uniform(0.05, 1.0, LOSS_ROWS).astype(F32)
    w.setflags(write=False)
    return w


# closed forms: (pred, target, iou)
CLOSED_FORMS = {
    "identical": ([100, 100, 40, 20, 0.3], [100, 100, 40, 20, 0.3], 1.0),
    "contained": ([102, 101, 20, 10, 0.9], [100, 100, 60, 40, 0.3], 200.0 / 2400.0),
    "parallel": ([100, 100, 40, 20, 0], [105, 103, 30, 24, 0], 0.6),
}
DISJOINT = ([40, 40, 20, 10, 0.2], [140, 150, 30, 12, -0.5])
