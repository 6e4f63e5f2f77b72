"""Restatements of the H2RBox pieces, written from the reference's text, and the fixtures of the H2RBox tests.

  rotate_crop(...)   H2RBox.rotate_crop for the image tensor (python/jdet/models/networks/h2rbox.py:L35-75): the grid as
                     L45-49 build it, torch.nn.functional.grid_sample on the CPU, the slice; float64 or float32.  This one
                     is pinned by EXECUTION (grid_sample is the same function the reference calls).
  aug_loss(...)      the consistency branch of H2RBoxHead.loss (models/roi_heads/h2rbox_head.py:L399-506) with
                     H2RBoxLoss.execute (models/losses/h2rbox_loss.py:L42-66), distance2obb (models/boxes/box_ops.py:
                     L694-707), bbox_overlaps(is_aligned=True) (models/boxes/iou_calculator.py:L302-342), iou_loss and
                     l1_loss, in torch, float64 or float32, LEVEL-major as the reference flattens, differentiated by
                     autograd into BOTH views.  The rounding of the cell map is half-to-even (include/jdet_hip.h).

Pinned by restatement only: Jittor is not importable here.  The loss fixtures are drawn and FILTERED here, at
generation, so the tests drop no row: a cell whose rotated position is within 1e-3 of a rounding tie gets weight 0, and a
row whose float64 quantities come within 1e-3 of a kink (|w_p - w_t|, |h_p - h_t|, the swapped pairs, |sin da|,
|cos da|, |dx|, |dy|, and w - h of either decoded box, where regular_obb swaps) or whose IoUs fall below 0.05 is redrawn.
The angle of view 2 and its cos / sin enter as the float32 values the kernel receives."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
SIZES = ((8, 8), (4, 4), (2, 2), (1, 1), (5, 7))            # 64 + 16 + 4 + 1 + 35 = 120 points; (5, 7): h = 5, w = 7
STRIDES = (8, 16, 32, 64, 8)
CROP = (64, 64)
N = sum(h * w for h, w in SIZES)
B = 2
NUM_CLASSES = 15
AGNOSTIC = (3, 7)                                           # 1-based class ids
ROTS = (0.3, -2.5, math.pi / 2)
WEIGHTS = dict(loss_weight=0.4, centre=0.5, shape=1.0, angle=1.0)   # the config's, but a centre weight that is not 0
EPS = 1e-6
MARGIN = 1e-3


def level_offsets(sizes=SIZES):
    off = [0]
    for h, w in sizes:
        off.append(off[-1] + h * w)
    return off


def f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------------- rotate_crop
def rotate_crop(img, theta, size, padding="reflection", dtype=torch.float64):
    """img (n, c, h, w) numpy -> (n, c, size_h, size_w) numpy in `dtype`"""
    img = torch.from_numpy(np.asarray(img)).to(dtype)
    n, c, h, w = img.shape
    size_h, size_w = size
    crop_h = (h - size_h) // 2
    crop_w = (w - size_w) // 2
    if theta != 0:
        cosa, sina = math.cos(theta), math.sin(theta)
        tf = torch.tensor([[cosa, -sina], [sina, cosa]], dtype=torch.float32).to(dtype)    # a float tensor, L43
        x_range = torch.linspace(-1, 1, w, dtype=dtype)
        y_range = torch.linspace(-1, 1, h, dtype=dtype)
        y, x = torch.meshgrid(y_range, x_range, indexing="ij")
        grid = torch.stack([x, y], -1).unsqueeze(0).expand(n, -1, -1, -1)
        grid = grid.reshape(-1, 2).matmul(tf).view(n, h, w, 2)
        img = F.grid_sample(img, grid, "bilinear", padding, align_corners=True)
    return img[..., crop_h:crop_h + size_h, crop_w:crop_w + size_w].numpy()


def source_positions(h, w, size, theta):
    """(ix, iy) float64 source positions (in pixels, before padding) of the cropped window's pixels"""
    size_h, size_w = size
    crop_h, crop_w = (h - size_h) // 2, (w - size_w) // 2
    Y, X = np.meshgrid(np.arange(crop_h, crop_h + size_h), np.arange(crop_w, crop_w + size_w), indexing="ij")
    gx, gy = -1 + 2 * X / (w - 1), -1 + 2 * Y / (h - 1)
    cs, sn = f32(math.cos(theta)), f32(math.sin(theta))
    sx, sy = gx * cs + gy * sn, -gx * sn + gy * cs
    return (sx + 1) / 2 * (w - 1), (sy + 1) / 2 * (h - 1)


@functools.lru_cache(maxsize=None)
def image_fixture(h, w):
    rng = np.random.default_rng(1000 * h + w)
    return rng.standard_normal((2, 3, h, w)).astype(F32)


@functools.lru_cache(maxsize=None)
def rotate_crop_reference(h, w, size, theta, padding):
    """(float64 result, max |float32 restatement - float64|) on image_fixture(h, w)"""
    img = image_fixture(h, w)
    r64 = rotate_crop(img, theta, size, padding, torch.float64)
    r32 = rotate_crop(img, theta, size, padding, torch.float32)
    return r64, float(np.abs(r32.astype(np.float64) - r64).max())


# ---------------------------------------------------------------------------------------------------------- aug loss
def regular_obb(obboxes):
    x, y, w, h, theta = obboxes.unbind(dim=-1)
    m = (w > h).to(w.dtype)
    w_regular = w * m + h * (1 - m)
    h_regular = h * m + w * (1 - m)
    theta_regular = theta * m + (theta + math.pi / 2) * (1 - m)
    theta_regular = torch.remainder(theta_regular - (-math.pi / 2), math.pi) + (-math.pi / 2)
    return torch.stack([x, y, w_regular, h_regular, theta_regular], dim=-1)


def distance2obb(points, distance):
    distance, theta = distance.split([4, 1], dim=1)
    Cos, Sin = torch.cos(theta), torch.sin(theta)
    Matrix = torch.cat([Cos, Sin, -Sin, Cos], dim=1).reshape(-1, 2, 2)
    wh = distance[:, :2] + distance[:, 2:]
    offset_t = ((distance[:, 2:] - distance[:, :2]) / 2).unsqueeze(2)
    offset = torch.bmm(Matrix, offset_t).squeeze(2)
    ctr = points + offset
    return regular_obb(torch.cat([ctr, wh, theta], dim=1))


def bbox_overlaps_aligned(b1, b2, eps=EPS):
    area1 = (b1[..., 2] - b1[..., 0]) * (b1[..., 3] - b1[..., 1])
    area2 = (b2[..., 2] - b2[..., 0]) * (b2[..., 3] - b2[..., 1])
    lt = torch.maximum(b1[..., :2], b2[..., :2])
    rb = torch.minimum(b1[..., 2:], b2[..., 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = torch.clamp(area1 + area2 - overlap, min=eps)
    return overlap / union


def _iou_loss(pred, target, weight, avg_factor, eps=EPS):
    ious = bbox_overlaps_aligned(pred, target).clamp(min=eps)
    return ((-ious.log()) * weight).sum() / avg_factor, ious


def _l1_loss(pred, target, weight, avg_factor):
    return ((pred - target).abs() * weight).sum() / avg_factor


def points_of(dtype, sizes=SIZES, strides=STRIDES):
    out = []
    for (h, w), s in zip(sizes, strides):
        y, x = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
        out.append(torch.stack((x.flatten() * s, y.flatten() * s), dim=-1) + s // 2)
    return out


def aug_loss(pred, pred_aug, weight, labels, rot, dtype=torch.float64, sizes=SIZES, strides=STRIDES, crop=CROP,
             agnostic=AGNOSTIC, weights=WEIGHTS, with_grad=True):
    """pred, pred_aug (B, N, 5), weight (B, N), labels (B, N) 0-based (numpy, image-major) -> dict(loss, sums
    (centre, branch 1, branch 2, weight), branch, aug_index (B, N), grad_pred, grad_aug, margins, ...)"""
    nb = pred.shape[0]
    off = level_offsets(sizes)
    n_pts = off[-1]
    p1 = torch.tensor(np.asarray(pred), dtype=dtype, requires_grad=with_grad)
    p2 = torch.tensor(np.asarray(pred_aug), dtype=dtype, requires_grad=with_grad)
    wgt = torch.tensor(np.asarray(weight), dtype=dtype)
    lab = torch.from_numpy(np.asarray(labels).astype(np.int64))
    # the reference's LEVEL-major flattening: per level (num_imgs * h * w) rows, levels concatenated
    lvl = lambda t: torch.cat([t[:, off[l]:off[l + 1]].reshape((-1,) + tuple(t.shape[2:]))  # noqa: E731
                               for l in range(len(sizes))])
    flat1, flat2, flat_w, flat_lab = lvl(p1), lvl(p2), lvl(wgt), lvl(lab) + 1               # labels 1-based, L387
    pts = points_of(dtype, sizes, strides)
    flat_points = torch.cat([p.repeat(nb, 1) for p in pts])
    # image-major index of every level-major row, to hand the map back in the kernel's layout
    image_major = torch.cat([(torch.arange(nb)[:, None] * n_pts + torch.arange(off[l], off[l + 1])[None]).reshape(-1)
                             for l in range(len(sizes))])
    pos_inds = (flat_w > 0).nonzero().reshape(-1)
    out = dict(aug_index=np.full((nb, n_pts), -1, np.int32), positives=int(len(pos_inds)))
    zero = dict(loss=0.0, sums=np.zeros(4), branch=0, grad_pred=np.zeros((nb, n_pts, 5)),
                grad_aug=np.zeros((nb, n_pts, 5)), valid=0, margins={})
    if len(pos_inds) == 0:
        return dict(out, **zero)
    rot_f = f32(rot)                                        # the angle is rounded to float once, then its cos / sin
    cosa, sina = f32(math.cos(rot_f)), f32(math.sin(rot_f))
    tf_T = torch.tensor([[cosa, sina], [-sina, cosa]], dtype=dtype)
    pos_inds_aug, valid_mask, tie = [], torch.zeros(len(pos_inds), dtype=torch.bool), []
    offset = 0
    for h, w in sizes:
        level_mask = (offset <= pos_inds) & (pos_inds < offset + nb * h * w)
        pos_ind = pos_inds[level_mask] - offset
        xy = torch.stack((pos_ind % w, (pos_ind // w) % h), dim=-1).to(dtype)
        b = pos_ind // (w * h)
        ctr = torch.tensor([[(w - 1) / 2, (h - 1) / 2]], dtype=dtype)
        real = (xy - ctr).matmul(tf_T) + ctr
        xy_aug = real.round().long()                                       # half to even
        tie.append((real - real.floor() - 0.5).abs().reshape(-1))
        x_aug, y_aug = xy_aug[..., 0], xy_aug[..., 1]
        ok = (x_aug >= 0) & (x_aug < w) & (y_aug >= 0) & (y_aug < h)
        pos_ind_aug = (b * h + y_aug) * w + x_aug
        valid_mask[level_mask] = ok
        pos_inds_aug.append(pos_ind_aug[ok] + offset)
        offset += nb * h * w
    pos_inds_aug = torch.cat(pos_inds_aug)
    tie = torch.cat(tie)
    out["tie_margin"] = float(tie.min())
    out["valid"] = int(valid_mask.sum())
    out["left"] = int((~valid_mask).sum())
    src = image_major[pos_inds[valid_mask]]
    dst = image_major[pos_inds_aug]
    out["aug_index"].reshape(-1)[src.numpy()] = (dst % n_pts).numpy().astype(np.int32)
    out["shared_cells"] = int((np.bincount(dst.numpy(), minlength=nb * n_pts) >= 2).sum())
    if not valid_mask.any():
        return dict(out, **zero)
    pos_bbox_preds = flat1[pos_inds]
    pos_points = flat_points[pos_inds]
    pos_labels = flat_lab[pos_inds]
    pos_centerness_targets = flat_w[pos_inds]
    pos_bbox_preds_aug = flat2[pos_inds_aug]
    pos_points_aug = flat_points[pos_inds_aug]
    pos_decoded_bbox_preds = distance2obb(pos_points, pos_bbox_preds)
    pos_decoded_bbox_preds_aug = distance2obb(pos_points_aug, pos_bbox_preds_aug)
    _h, _w = crop
    _ctr = torch.tensor([[(_w - 1) / 2, (_h - 1) / 2]], dtype=dtype)
    _xy = pos_decoded_bbox_preds[valid_mask, :2]
    _wh = pos_decoded_bbox_preds[valid_mask, 2:4]
    angle_t = pos_decoded_bbox_preds[valid_mask, 4:] + rot_f
    _xy = (_xy - _ctr).matmul(tf_T) + _ctr
    lab_aug = pos_labels[valid_mask]
    mask = torch.ones_like(angle_t)
    for c in agnostic or ():
        mask[lab_aug == c] = 0
    angle_t = angle_t * mask
    out["agnostic_rows"] = int((mask == 0).sum())
    target = torch.cat([_xy, _wh, angle_t], dim=-1)
    w_aug = pos_centerness_targets[valid_mask]
    avg = max(float(w_aug.sum()), 1.0)
    # H2RBoxLoss.execute
    prd = pos_decoded_bbox_preds_aug
    hbb_pred1 = torch.cat([-prd[..., 2:4], prd[..., 2:4]], dim=-1)
    hbb_pred2 = hbb_pred1[..., [1, 0, 3, 2]]
    hbb_target = torch.cat([-target[..., 2:4], target[..., 2:4]], dim=-1)
    d_a = prd[..., 4] - target[..., 4]
    center = weights["centre"] * _l1_loss(prd[..., :2], target[..., :2], w_aug[:, None], avg)
    s1, iou1 = _iou_loss(hbb_pred1, hbb_target, w_aug, avg)
    s2, iou2 = _iou_loss(hbb_pred2, hbb_target, w_aug, avg)
    shape1 = weights["shape"] * s1 + weights["angle"] * _l1_loss(d_a.sin(), torch.zeros_like(d_a), w_aug, avg)
    shape2 = weights["shape"] * s2 + weights["angle"] * _l1_loss(d_a.cos(), torch.zeros_like(d_a), w_aug, avg)
    loss = weights["loss_weight"] * (center + torch.minimum(shape1, shape2))
    out.update(loss=float(loss.detach()), branch=int(float(shape2.detach()) < float(shape1.detach())), avg=avg,
               sums=np.array([float(center.detach()) * avg / weights["centre"] if weights["centre"] else 0.0,
                              float(shape1.detach()) * avg, float(shape2.detach()) * avg, float(w_aug.sum())]),
               branch_gap=abs(float(shape1.detach()) - float(shape2.detach())))
    raw1 = flat1[pos_inds][valid_mask]
    raw2 = pos_bbox_preds_aug
    d = lambda a, b_: float((a - b_).abs().min())  # noqa: E731
    out["margins"] = dict(
        w=d(prd[:, 2], target[:, 2]), h=d(prd[:, 3], target[:, 3]), w_swapped=d(prd[:, 3], target[:, 2]),
        h_swapped=d(prd[:, 2], target[:, 3]), sin=float(d_a.sin().abs().min()), cos=float(d_a.cos().abs().min()),
        dx=d(prd[:, 0], target[:, 0]), dy=d(prd[:, 1], target[:, 1]),
        swap1=float(((raw1[:, 0] + raw1[:, 2]) - (raw1[:, 1] + raw1[:, 3])).abs().min()),
        swap2=float(((raw2[:, 0] + raw2[:, 2]) - (raw2[:, 1] + raw2[:, 3])).abs().min()))
    out["min_iou"] = float(torch.minimum(iou1, iou2).min())
    # per valid row, for the generation filter: the smallest margin and the smallest IoU
    with torch.no_grad():
        row = torch.stack([(prd[:, 2] - target[:, 2]).abs(), (prd[:, 3] - target[:, 3]).abs(),
                           (prd[:, 3] - target[:, 2]).abs(), (prd[:, 2] - target[:, 3]).abs(), d_a.sin().abs(),
                           d_a.cos().abs(), (prd[:, 0] - target[:, 0]).abs(), (prd[:, 1] - target[:, 1]).abs(),
                           ((raw1[:, 0] + raw1[:, 2]) - (raw1[:, 1] + raw1[:, 3])).abs(),
                           ((raw2[:, 0] + raw2[:, 2]) - (raw2[:, 1] + raw2[:, 3])).abs()], 1).min(1).values
        out["row_src"] = src.numpy()
        out["row_margin"] = row.numpy()
        out["row_iou"] = torch.minimum(iou1, iou2).numpy()
    if with_grad:
        loss.backward()
        out["grad_pred"] = p1.grad.numpy().astype(np.float64)
        out["grad_aug"] = p2.grad.numpy().astype(np.float64)
    return out


def _draw_rows(rng, n, square):
    """n rows [l, t, r, b, theta]: sizes 3 .. 8; `square`: w / h in 1.05 .. 1.3, else anything"""
    ltrb = rng.uniform(1.5, 4.0, (n, 4))
    if square:
        h = rng.uniform(3.0, 6.0, n)
        w = h * rng.uniform(1.05, 1.3, n)
        fl, ft = rng.uniform(0.3, 0.7, n), rng.uniform(0.3, 0.7, n)
        ltrb = np.stack([w * fl, h * ft, w * (1 - fl), h * (1 - ft)], 1)
    return np.concatenate([ltrb, rng.uniform(-1.0, 1.0, (n, 1))], 1)


@functools.lru_cache(maxsize=None)
def loss_fixture(rot, winner=1, seed=0):
    """(pred, pred_aug (B, N, 5) fp32, weight (B, N) fp32, labels (B, N) int32 0-based, redrawn rows) with the branch
    `winner` (1 or 2) the smaller scalar: for 1 view 2 repeats view 1's angle turned by rot (|sin da| small), for 2 the
    boxes are near-square and view 2's angle is a quarter turn further (|cos da| small, the swapped shapes match)"""
    rng = np.random.default_rng(seed + 17 * int(round(rot * 1000)) + 1000003 * winner)
    square = winner == 2
    pred = _draw_rows(rng, B * N, square).reshape(B, N, 5)
    pred_aug = _draw_rows(rng, B * N, square).reshape(B, N, 5)
    weight = np.where(rng.uniform(size=(B, N)) < 0.75, rng.uniform(0.2, 1.0, (B, N)), 0.0)
    labels = rng.integers(0, NUM_CLASSES, (B, N))
    labels[:, ::5] = AGNOSTIC[0] - 1                       # every fifth point rotation-agnostic (where positive)
    labels = np.where(weight > 0, labels, NUM_CLASSES).astype(np.int32)
    # cells within MARGIN of a rounding tie get weight 0 (the map depends on the cell and rot alone)
    off = level_offsets()
    cs, sn = f32(math.cos(f32(rot))), f32(math.sin(f32(rot)))
    for l, (h, w) in enumerate(SIZES):
        y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        dx, dy = x.ravel() - (w - 1) / 2, y.ravel() - (h - 1) / 2
        real = np.stack([dx * cs - dy * sn + (w - 1) / 2, dx * sn + dy * cs + (h - 1) / 2], 1)
        near = (np.abs(real - np.floor(real) - 0.5) < MARGIN).any(1)
        weight[:, off[l]:off[l + 1]][:, near] = 0.0
    labels = np.where(weight > 0, labels, NUM_CLASSES).astype(np.int32)
    # view 2 follows the LAST view-1 row that lands on each of its points
    r = aug_loss(pred.astype(F32), pred_aug.astype(F32), weight.astype(F32), labels, rot, with_grad=False)
    idx = r["aug_index"]
    for b in range(B):
        for p in np.flatnonzero(idx[b] >= 0):
            q = idx[b, p]
            agn = (labels[b, p] + 1) in AGNOSTIC
            turn = (0.0 if agn else rot) + (math.pi / 2 if square else 0.0)
            common = rng.uniform(0.85, 0.95) if rng.uniform() < 0.5 else rng.uniform(1.05, 1.2)
            pred_aug[b, q, :4] = pred[b, p, :4] * common * rng.uniform(0.97, 1.03, 4)
            pred_aug[b, q, 4] = pred[b, p, 4] + turn + rng.uniform(0.05, 0.3) * rng.choice([-1, 1])
    redrawn = 0
    for _ in range(200):
        r = aug_loss(pred.astype(F32), pred_aug.astype(F32), weight.astype(F32), labels, rot, with_grad=False)
        bad = r["row_src"][(r["row_margin"] < 2 * MARGIN) | (r["row_iou"] < 0.06)]
        if len(bad) == 0:
            break
        redrawn += len(bad)
        pred.reshape(-1, 5)[bad] = _draw_rows(rng, len(bad), square)
        # (a kink of the view-2 row alone -- its own w - h, the angle against a rotation-agnostic target -- needs a new
        # view-2 row as well)
        dst = (bad // N) * N + r["aug_index"].reshape(-1)[bad]
        pred_aug.reshape(-1, 5)[dst] = _draw_rows(rng, len(dst), square)
    else:
        raise AssertionError("the loss fixture did not settle")
    return pred.astype(F32), pred_aug.astype(F32), weight.astype(F32), labels, redrawn


@functools.lru_cache(maxsize=None)
def loss_reference(rot, winner=1):
    """(float64 result, |loss32 - loss64|, max |grad32 - grad64| / max |grad64| per view) on loss_fixture(rot, winner)"""
    pred, pred_aug, weight, labels, _ = loss_fixture(rot, winner)
    r64 = aug_loss(pred, pred_aug, weight, labels, rot, torch.float64)
    r32 = aug_loss(pred, pred_aug, weight, labels, rot, torch.float32)
    assert np.array_equal(r64["aug_index"], r32["aug_index"]) and r64["branch"] == r32["branch"]
    e_loss = abs(r32["loss"] - r64["loss"])
    e_g1 = float(np.abs(r32["grad_pred"] - r64["grad_pred"]).max() / np.abs(r64["grad_pred"]).max())
    e_g2 = float(np.abs(r32["grad_aug"] - r64["grad_aug"]).max() / np.abs(r64["grad_aug"]).max())
    return r64, e_loss, e_g1, e_g2


def grad_errors(grad_pred, grad_aug, ref):
    """the two gradient errors in the measure of loss_reference"""
    return (float(np.abs(np.asarray(grad_pred, np.float64) - ref["grad_pred"]).max() / np.abs(ref["grad_pred"]).max()),
            float(np.abs(np.asarray(grad_aug, np.float64) - ref["grad_aug"]).max() / np.abs(ref["grad_aug"]).max()))
