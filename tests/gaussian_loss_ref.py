"""float64 restatement of the reference's Gaussian box losses, written from its text (torch float64 on the host,
torch.linalg for det / inv as the reference's jt.linalg): models/losses/gaussian_dist_loss.py:L48-276,
gaussian_dist_loss_v1.py:L48-156, kf_iou_loss.py:L48-99, the decode of models/boxes/box_ops.py:L229-285 and the
obb -> hbb -> obb conversion of ops/bbox_transforms.py:L639-665.  Independent of jdet_amd (imports nothing from it).

`row_losses` returns the per-row loss (no reduction, no mask); the tests mask, sum and differentiate it."""
import math

import numpy as np
import torch

D = torch.float64


def norm_angle(a):
    return torch.remainder(a + math.pi / 4, math.pi) - math.pi / 4


def delta2bbox(anchors, deltas, means=(0.,) * 5, stds=(1.,) * 5, wh_ratio_clip=16 / 1000):
    d = deltas * torch.tensor(stds, dtype=D) + torch.tensor(means, dtype=D)
    dx, dy, dw, dh, da = d.unbind(-1)
    m = abs(math.log(wh_ratio_clip))
    dw, dh = dw.clamp(-m, m), dh.clamp(-m, m)
    ax, ay, aw, ah, aa = anchors.unbind(-1)
    gx = dx * aw * torch.cos(aa) - dy * ah * torch.sin(aa) + ax
    gy = dx * aw * torch.sin(aa) + dy * ah * torch.cos(aa) + ay
    return torch.stack([gx, gy, aw * dw.exp(), ah * dh.exp(), norm_angle(math.pi * da + aa)], -1)


def gauss(b):
    wh = b[:, 2:4].clamp(1e-7, 1e7)
    c, s = torch.cos(b[:, 4]), torch.sin(b[:, 4])
    R = torch.stack((c, -s, s, c), -1).reshape(-1, 2, 2)
    S = torch.diag_embed(0.5 * wh)
    return b[:, :2], R @ S @ S @ R.transpose(1, 2)


def _tr(m):
    return m.diagonal(dim1=-2, dim2=-1).sum(-1)


def post_v0(d, fun, tau):
    if fun == "log1p":
        d = torch.log(1 + d)
    elif fun == "sqrt":
        d = torch.sqrt(d.clamp(min=1e-7))
    return 1 - 1 / (tau + d) if tau >= 1.0 else d


def gwd_v0_terms(p, t):
    """(xy_distance, whr_distance, _t_det_sqrt) of GDLoss's gwd_loss"""
    (xp, Sp), (xt, St) = p, t
    xy = ((xp - xt) ** 2).sum(-1)
    whr = _tr(Sp) + _tr(St)
    t_tr = _tr(Sp @ St)
    t_det_sqrt = (torch.linalg.det(Sp) * torch.linalg.det(St)).clamp(min=0).sqrt()
    whr = whr - 2 * (t_tr + 2 * t_det_sqrt).clamp(min=1e-7).sqrt()
    return xy, whr, t_det_sqrt


def gwd_v0(p, t, fun, tau, alpha=1.0, normalize=True):
    xy, whr, t_det_sqrt = gwd_v0_terms(p, t)
    dist = (xy + alpha * alpha * whr).clamp(min=1e-7).sqrt()
    if normalize:
        dist = dist / (2 * t_det_sqrt.clamp(min=1e-7).sqrt().clamp(min=1e-7).sqrt().clamp(min=1e-7))
    return post_v0(dist, fun, tau)


def kld_v0_raw(p, t, alpha=1.0, sqrt=True):
    (xp, Sp), (xt, St) = p, t
    inv = torch.linalg.inv(Sp) / torch.linalg.det(Sp)[:, None, None]
    d = (xp - xt)[:, :, None]
    xy = 0.5 * (d.transpose(1, 2) @ inv @ d).reshape(-1)
    whr = 0.5 * _tr(inv @ St) + 0.5 * (torch.log(torch.linalg.det(Sp)) - torch.log(torch.linalg.det(St))) - 1
    dist = xy / (alpha * alpha) + whr
    return dist.clamp(min=1e-7).sqrt() if sqrt else dist


def gwd_v1_dis(p, t):
    (xp, Sp), (xt, St) = p, t
    xy = ((xp - xt) ** 2).sum(-1)
    t_det_sqrt = (torch.linalg.det(Sp) * torch.linalg.det(St)).clamp(min=0).sqrt()
    whr = _tr(Sp) + _tr(St) - 2 * (_tr(Sp @ St) + 2 * t_det_sqrt).clamp(min=0).sqrt()
    return xy + whr, t_det_sqrt


def gwd_v1(p, t, fun, tau):
    dis, t_det_sqrt = gwd_v1_dis(p, t)
    g = dis.clamp(min=1e-6)
    if fun == "sqrt":
        return 1 - 1 / (tau + g.sqrt())
    if fun == "log1p":
        return 1 - 1 / (tau + torch.log(1 + g))
    return torch.log(1 + g.sqrt() / (2 * t_det_sqrt.sqrt().sqrt().clamp(min=1e-7)))


def bcd_v1(p, t, fun, tau):
    (xp, Sp), (xt, St) = p, t
    S = 0.5 * (Sp + St)
    d = (xp - xt)[:, :, None]
    term1 = torch.log(torch.linalg.det(S) / torch.sqrt(torch.linalg.det(St @ Sp)))
    term2 = (d.transpose(1, 2) @ torch.linalg.inv(S) @ d).reshape(-1)
    b = (0.5 * term1 + 0.125 * term2).clamp(min=1e-6)
    if fun == "sqrt":
        return 1 - 1 / (tau + b.sqrt())
    if fun == "log1p":
        return 1 - 1 / (tau + torch.log(1 + b))
    return 1 - 1 / (tau + b)


def kld_v1_dis(p, t):
    (xp, Sp), (xt, St) = p, t
    inv = torch.linalg.inv(St)
    d = (xp - xt)[:, :, None]
    term1 = (d.transpose(1, 2) @ inv @ d).reshape(-1)
    term2 = _tr(inv @ Sp) + torch.log(torch.linalg.det(St) / torch.linalg.det(Sp))
    return term1 + term2 - 2


def kld_v1(p, t, fun, tau):
    kl = kld_v1_dis(p, t).clamp(min=1e-6)
    if fun == "sqrt":
        return 1 - 1 / (tau + kl.sqrt())
    return 1 - 1 / (tau + torch.log(1 + kl))


def kfiou_terms(pred, target, pred_decode, target_decode, beta=1.0 / 9.0, eps=1e-6):
    """(xy_loss, KFIoU) of kfiou_loss"""
    _, Sp = gauss(pred_decode)
    _, St = gauss(target_decode)
    diff = (pred[:, :2] - target[:, :2]).abs()
    xy_loss = torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta).sum(-1)
    Vb_p = 4 * torch.linalg.det(Sp).sqrt()
    Vb_t = 4 * torch.linalg.det(St).sqrt()
    K = Sp @ torch.linalg.inv(Sp + St)
    Vb = 4 * torch.linalg.det(Sp - K @ Sp).sqrt()
    Vb = torch.where(torch.isnan(Vb), torch.zeros_like(Vb), Vb)
    return xy_loss, Vb / (Vb_p + Vb_t - Vb + eps)


def kfiou(pred, target, pred_decode, target_decode, fun="none", beta=1.0 / 9.0, eps=1e-6):
    xy_loss, kf = kfiou_terms(pred, target, pred_decode, target_decode, beta, eps)
    if fun == "ln":
        kl = -torch.log(kf + eps)
    elif fun == "exp":
        kl = torch.exp(1 - kf) - 1
    else:
        kl = 1 - kf
    return (xy_loss + kl).clamp(min=0)


def row_losses(kind, pred, target, anchors=None, fun="log1p", tau=0.0, alpha=1.0, normalize=True, sqrt=True,
               decode_pred=False, decode_target=False):
    """per-row loss of `kind` (gwd kld jd kld_symmax kld_symmin | gwd_v1 kld_v1 bcd_v1 | kfiou); pred / target rows of
    deltas when decoded (anchors (rows, 5)), else boxes"""
    pb = delta2bbox(anchors, pred) if decode_pred or kind == "kfiou" else pred
    tb = delta2bbox(anchors, target) if decode_target or kind == "kfiou" else target
    if kind == "kfiou":
        return kfiou(pred, target, pb, tb, fun=fun)
    p, t = gauss(pb), gauss(tb)
    if kind == "gwd":
        return gwd_v0(p, t, fun, tau, alpha, normalize)
    if kind == "kld":
        return post_v0(kld_v0_raw(p, t, alpha, sqrt), fun, tau)
    if kind == "jd":
        j = 0.5 * (kld_v0_raw(p, t, alpha, False) + kld_v0_raw(t, p, alpha, False))
        return post_v0(j.clamp(min=1e-7).sqrt() if sqrt else j, fun, tau)
    if kind in ("kld_symmax", "kld_symmin"):
        a, b = kld_v0_raw(p, t, alpha, sqrt), kld_v0_raw(t, p, alpha, sqrt)
        return post_v0(torch.maximum(a, b) if kind == "kld_symmax" else torch.minimum(a, b), fun, tau)
    return {"gwd_v1": gwd_v1, "kld_v1": kld_v1, "bcd_v1": bcd_v1}[kind](p, t, fun, tau)


def masked_loss_and_grad(kind, pred, target, weight, avg_factor, loss_weight, **kw):
    """(loss, d loss / d pred) in float64: sum over rows with weight.mean(-1) > 0, / avg_factor, * loss_weight"""
    p = torch.as_tensor(np.asarray(pred), dtype=D).clone().requires_grad_(True)
    t = torch.as_tensor(np.asarray(target), dtype=D)
    a = kw.pop("anchors", None)
    a = torch.as_tensor(np.asarray(a), dtype=D) if a is not None else None
    mask = torch.as_tensor(np.asarray(weight), dtype=D).mean(-1) > 0
    rows = row_losses(kind, p[mask], t[mask], a[mask] if a is not None else None, **kw)
    loss = rows.sum() / avg_factor * loss_weight
    loss.backward()
    return float(loss.detach()), p.grad.numpy()


def fake_rotated_boxes(boxes):
    """hbb2obb(obb2hbb(boxes)), float64 numpy"""
    b = np.asarray(boxes, dtype=np.float64)
    x, y, w, h, t = b[:, 0], b[:, 1], b[:, 2], b[:, 3], b[:, 4]
    xb = np.abs(w / 2 * np.cos(t)) + np.abs(h / 2 * np.sin(t))
    yb = np.abs(w / 2 * np.sin(t)) + np.abs(h / 2 * np.cos(t))
    ww, hh = 2 * xb, 2 * yb
    flag = ww >= hh
    return np.stack([x, y, np.where(flag, ww, hh), np.where(flag, hh, ww), np.where(flag, 0.0, -np.pi / 2)], 1)
