"""BBox coders of the named configs.  Mirrors python/jdet/models/boxes/coder.py:
`DeltaXYWHABBoxCoder` L76-141."""
import math
import os

import torch

from jdet_amd import _lib as L
from jdet_amd.ops.bbox_transforms import (hbb2poly, obb2hbb, obb2poly, poly2hbb, rectpoly2obb, regular_obb,
                                          regular_theta)
from jdet_amd.utils.general import const_like
from jdet_amd.utils.registry import BOXES

from .box_ops import bbox2delta_rotated, delta2bbox_rotated


def _fused_ok(*ts):
    """the fused HIP codecs produce values, not graphs: used whenever no gradient is asked for"""
    return all(t.is_cuda and t.dim() == 2 for t in ts) and not (torch.is_grad_enabled() and
                                                                  any(t.requires_grad for t in ts))


def _fused32_ok(*ts):
    """`_fused_ok` for float32 inputs only: the kernels are fp32, and a float64 caller is promised the float64
    composition, not a silent down-cast"""
    return _fused_ok(*ts) and all(t.dtype == torch.float32 for t in ts)


def _fused_no64_ok(*ts):
    """`_fused_ok` unless an input is float64 (the Oriented R-CNN coders): the kernels are fp32, and a float64 caller is
    promised the float64 composition, not a silent down-cast.  Half and bfloat16 inputs (a head under autocast) are
    up-cast to the one fp32 launch, as before"""
    return _fused_ok(*ts) and not any(t.dtype == torch.float64 for t in ts)


def _floating(t):
    """the reference's `.float()`, except that float64 stays float64"""
    return t if t.dtype == torch.float64 else t.float()


@BOXES.register_module()
class DeltaXYWHABBoxCoder:
    """encodes (x,y,w,h,a) into (dx,dy,dw,dh,da) relative to a base box and back."""

    def __init__(self, target_means=(0., 0., 0., 0., 0.), target_stds=(1., 1., 1., 1., 1.), clip_border=True):
        self.means = target_means
        self.stds = target_stds
        self.clip_border = clip_border

    def encode(self, bboxes, gt_bboxes):
        assert bboxes.size(0) == gt_bboxes.size(0)
        assert bboxes.size(-1) == gt_bboxes.size(-1) == 5
        return bbox2delta_rotated(bboxes, gt_bboxes, self.means, self.stds)

    def decode(self, bboxes, pred_bboxes, max_shape=None, wh_ratio_clip=16 / 1000):
        assert pred_bboxes.size(0) == bboxes.size(0)
        return delta2bbox_rotated(bboxes, pred_bboxes, self.means, self.stds, max_shape, wh_ratio_clip,
                                  self.clip_border)


@BOXES.register_module()
class MidpointOffsetCoder:
    """Oriented RPN 6-parameter codec (coder.py:L322-437): hbb anchor -> (dx,dy,dw,dh,da,db) where a/b are
    the offsets of the top-most / right-most vertex from the mid-points of the enclosing box."""

    def __init__(self, target_means=(0., 0., 0., 0., 0., 0.), target_stds=(1., 1., 1., 1., 1., 1.)):
        self.means = target_means
        self.stds = target_stds

    def encode(self, bboxes, gt_bboxes):
        assert bboxes.size(0) == gt_bboxes.size(0)
        if _fused_no64_ok(bboxes, gt_bboxes) and bboxes.shape[1] == 4 and gt_bboxes.shape[1] == 5:
            a, g = L.f32c(bboxes), L.f32c(gt_bboxes)
            out = torch.empty((a.shape[0], 6), dtype=torch.float32, device=a.device)
            L.check(L.lib().jdet_midpoint_offset_encode(L.ptr(a), L.ptr(g), a.shape[0], L.vecn(self.means, 6),
                                                        L.vecn(self.stds, 6), L.ptr(out), L.stream_ptr(a)),
                    "jdet_midpoint_offset_encode")
            return out
        pred_bboxes, gt = _floating(bboxes), _floating(gt_bboxes)
        px = (pred_bboxes[..., 0] + pred_bboxes[..., 2]) * 0.5
        py = (pred_bboxes[..., 1] + pred_bboxes[..., 3]) * 0.5
        pw = pred_bboxes[..., 2] - pred_bboxes[..., 0]
        ph = pred_bboxes[..., 3] - pred_bboxes[..., 1]
        hbb, poly = obb2hbb(gt), obb2poly(gt)
        gx = (hbb[..., 0] + hbb[..., 2]) * 0.5
        gy = (hbb[..., 1] + hbb[..., 3]) * 0.5
        gw = hbb[..., 2] - hbb[..., 0]
        gh = hbb[..., 3] - hbb[..., 1]
        x_coor, y_coor = poly[:, 0::2], poly[:, 1::2]
        y_min = y_coor.min(dim=1, keepdim=True).values
        x_max = x_coor.max(dim=1, keepdim=True).values
        _x_coor = x_coor.clone()
        _x_coor[torch.abs(y_coor - y_min) > 0.1] = -1000
        ga = _x_coor.max(dim=1).values
        _y_coor = y_coor.clone()
        _y_coor[torch.abs(x_coor - x_max) > 0.1] = -1000
        gb = _y_coor.max(dim=1).values
        dx = (gx - px) / pw
        dy = (gy - py) / ph
        dw = torch.log(gw / pw)
        dh = torch.log(gh / ph)
        da = (ga - gx) / gw
        db = (gb - gy) / gh
        deltas = torch.stack([dx, dy, dw, dh, da, db], dim=-1)
        means = deltas.new_tensor(self.means).unsqueeze(0)
        stds = deltas.new_tensor(self.stds).unsqueeze(0)
        return (deltas - means) / stds

    def decode(self, bboxes, pred_bboxes, max_shape=None, wh_ratio_clip=16 / 1000):
        assert pred_bboxes.size(0) == bboxes.size(0)
        if _fused_no64_ok(bboxes, pred_bboxes) and bboxes.shape[1] == 4 and pred_bboxes.shape[1] == 6:
            a, d = L.f32c(bboxes), L.f32c(pred_bboxes)
            out = torch.empty((a.shape[0], 5), dtype=torch.float32, device=a.device)
            L.check(L.lib().jdet_midpoint_offset_decode(L.ptr(a), L.ptr(d), a.shape[0], L.vecn(self.means, 6),
                                                        L.vecn(self.stds, 6), float(wh_ratio_clip), L.ptr(out),
                                                        L.stream_ptr(a)), "jdet_midpoint_offset_decode")
            return out
        means = pred_bboxes.new_tensor(self.means).repeat(1, pred_bboxes.size(1) // 6)
        stds = pred_bboxes.new_tensor(self.stds).repeat(1, pred_bboxes.size(1) // 6)
        d = pred_bboxes * stds + means
        dx, dy, dw, dh, da, db = d[:, 0::6], d[:, 1::6], d[:, 2::6], d[:, 3::6], d[:, 4::6], d[:, 5::6]
        max_ratio = abs(math.log(wh_ratio_clip))
        dw = dw.clamp(min=-max_ratio, max=max_ratio)
        dh = dh.clamp(min=-max_ratio, max=max_ratio)
        px = ((bboxes[:, 0] + bboxes[:, 2]) * 0.5).unsqueeze(1)
        py = ((bboxes[:, 1] + bboxes[:, 3]) * 0.5).unsqueeze(1)
        pw = (bboxes[:, 2] - bboxes[:, 0]).unsqueeze(1)
        ph = (bboxes[:, 3] - bboxes[:, 1]).unsqueeze(1)
        gw, gh = pw * dw.exp(), ph * dh.exp()
        gx, gy = px + pw * dx, py + ph * dy
        x1, y1, x2, y2 = gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5
        da = da.clamp(min=-0.5, max=0.5)
        db = db.clamp(min=-0.5, max=0.5)
        ga, _ga = gx + da * gw, gx - da * gw
        gb, _gb = gy + db * gh, gy - db * gh
        polys = torch.stack([ga, y1, x2, gb, _ga, y2, x1, _gb], dim=-1)
        center = torch.stack([gx, gy, gx, gy, gx, gy, gx, gy], dim=-1)
        center_polys = polys - center
        diag_len = torch.sqrt(center_polys[..., 0::2] ** 2 + center_polys[..., 1::2] ** 2)
        max_diag_len = diag_len.max(dim=-1, keepdim=True).values
        diag_scale_factor = max_diag_len / diag_len
        center_polys = center_polys * diag_scale_factor.repeat_interleave(2, dim=-1)
        rectpolys = center_polys + center
        return rectpoly2obb(rectpolys).flatten(-2)


@BOXES.register_module()
class OrientedDeltaXYWHTCoder:
    """Oriented R-CNN 5-parameter codec (coder.py:L439-518): picks between dtheta and dtheta + pi/2 (with a
    w/h swap) by smaller magnitude, using arithmetic masks."""

    def __init__(self, target_means=(0., 0., 0., 0., 0.), target_stds=(1., 1., 1., 1., 1.)):
        self.means = target_means
        self.stds = target_stds

    def encode(self, bboxes, gt_bboxes):
        assert bboxes.size(0) == gt_bboxes.size(0)
        assert bboxes.size(-1) == gt_bboxes.size(-1) == 5
        if _fused_no64_ok(bboxes, gt_bboxes):
            p, g = L.f32c(bboxes), L.f32c(gt_bboxes)
            out = torch.empty_like(p)
            L.check(L.lib().jdet_oriented_delta_encode(L.ptr(p), L.ptr(g), p.shape[0], L.vecn(self.means, 5),
                                                       L.vecn(self.stds, 5), L.ptr(out), L.stream_ptr(p)),
                    "jdet_oriented_delta_encode")
            return out
        px, py, pw, ph, ptheta = _floating(bboxes).unbind(dim=-1)
        gx, gy, gw, gh, gtheta = _floating(gt_bboxes).unbind(dim=-1)
        dtheta1 = regular_theta(gtheta - ptheta)
        dtheta2 = regular_theta(gtheta - ptheta + math.pi / 2)
        m = (torch.abs(dtheta1) < torch.abs(dtheta2)).to(px.dtype)
        gw_regular = gw * m + gh * (1 - m)
        gh_regular = gh * m + gw * (1 - m)
        dtheta = dtheta1 * m + dtheta2 * (1 - m)
        dx = (torch.cos(-ptheta) * (gx - px) + torch.sin(-ptheta) * (gy - py)) / pw
        dy = (-torch.sin(-ptheta) * (gx - px) + torch.cos(-ptheta) * (gy - py)) / ph
        dw = torch.log(gw_regular / pw)
        dh = torch.log(gh_regular / ph)
        deltas = torch.stack([dx, dy, dw, dh, dtheta], dim=-1)
        means = deltas.new_tensor(self.means).unsqueeze(0)
        stds = deltas.new_tensor(self.stds).unsqueeze(0)
        return (deltas - means) / stds

    def decode(self, bboxes, pred_bboxes, max_shape=None, wh_ratio_clip=16 / 1000):
        assert pred_bboxes.size(0) == bboxes.size(0)
        if _fused_no64_ok(bboxes, pred_bboxes) and bboxes.shape[1] == 5 and pred_bboxes.shape[1] % 5 == 0:
            r, d = L.f32c(bboxes), L.f32c(pred_bboxes)
            out = torch.empty_like(d)
            L.check(L.lib().jdet_oriented_delta_decode(L.ptr(r), L.ptr(d), d.shape[0], d.shape[1] // 5,
                                                       L.vecn(self.means, 5), L.vecn(self.stds, 5),
                                                       float(wh_ratio_clip), L.ptr(out), L.stream_ptr(d)),
                    "jdet_oriented_delta_decode")
            return out
        means = pred_bboxes.new_tensor(self.means).repeat(1, pred_bboxes.size(1) // 5)
        stds = pred_bboxes.new_tensor(self.stds).repeat(1, pred_bboxes.size(1) // 5)
        d = pred_bboxes * stds + means
        dx, dy, dw, dh, dtheta = d[:, 0::5], d[:, 1::5], d[:, 2::5], d[:, 3::5], d[:, 4::5]
        max_ratio = abs(math.log(wh_ratio_clip))
        dw = dw.clamp(min=-max_ratio, max=max_ratio)
        dh = dh.clamp(min=-max_ratio, max=max_ratio)
        px, py, pw, ph, ptheta = bboxes.unbind(dim=-1)
        px, py = px.unsqueeze(1).expand_as(dx), py.unsqueeze(1).expand_as(dy)
        pw, ph = pw.unsqueeze(1).expand_as(dw), ph.unsqueeze(1).expand_as(dh)
        ptheta = ptheta.unsqueeze(1).expand_as(dtheta)
        gx = dx * pw * torch.cos(-ptheta) - dy * ph * torch.sin(-ptheta) + px
        gy = dx * pw * torch.sin(-ptheta) + dy * ph * torch.cos(-ptheta) + py
        gw, gh = pw * dw.exp(), ph * dh.exp()
        gtheta = regular_theta(dtheta + ptheta)
        new_bboxes = regular_obb(torch.stack([gx, gy, gw, gh, gtheta], dim=-1))
        return new_bboxes.view_as(pred_bboxes)


# ----------------------------------------------------------------------------------------------------------------
# Gliding Vertex coders (coder.py:L143-320 of the reference).  The fused launches live in csrc/box_codec_gliding.hip;
# the torch compositions below are what runs on the host, in float64 and wherever a gradient is asked for.  The Jittor
# programs themselves cannot be run here (Jittor is not importable): the compositions are pinned by the restatement in
# tests/gliding_ref.py and its closed forms only.

def _max_hw(max_shape):
    """(h, w) of a `max_shape` argument as floats; (0, 0) = no clamp"""
    if max_shape is None:
        return 0.0, 0.0
    return float(max_shape[0]), float(max_shape[1])


def gv_delta_encode(bboxes, gt_bboxes, means, stds):
    """GVDeltaXYWHBBoxCoder.encode as a torch composition (coder.py:L248-268)"""
    px = (bboxes[..., 0] + bboxes[..., 2]) * 0.5
    py = (bboxes[..., 1] + bboxes[..., 3]) * 0.5
    pw = bboxes[..., 2] - bboxes[..., 0]
    ph = bboxes[..., 3] - bboxes[..., 1]
    gx = (gt_bboxes[..., 0] + gt_bboxes[..., 2]) * 0.5
    gy = (gt_bboxes[..., 1] + gt_bboxes[..., 3]) * 0.5
    gw = gt_bboxes[..., 2] - gt_bboxes[..., 0]
    gh = gt_bboxes[..., 3] - gt_bboxes[..., 1]
    deltas = torch.stack([(gx - px) / pw, (gy - py) / ph, torch.log(gw / pw), torch.log(gh / ph)], dim=-1)
    return (deltas - deltas.new_tensor(means).unsqueeze(0)) / deltas.new_tensor(stds).unsqueeze(0)


def gv_delta_decode(bboxes, pred_bboxes, means, stds, max_shape=None, wh_ratio_clip=16 / 1000):
    """GVDeltaXYWHBBoxCoder.decode as a torch composition (coder.py:L280-318)"""
    reps = pred_bboxes.size(1) // 4
    d = pred_bboxes * pred_bboxes.new_tensor(stds).repeat(1, reps) + pred_bboxes.new_tensor(means).repeat(1, reps)
    dx, dy, dw, dh = d[:, 0::4], d[:, 1::4], d[:, 2::4], d[:, 3::4]
    max_ratio = abs(math.log(wh_ratio_clip))
    dw = dw.clamp(min=-max_ratio, max=max_ratio)
    dh = dh.clamp(min=-max_ratio, max=max_ratio)
    px = ((bboxes[:, 0] + bboxes[:, 2]) * 0.5).unsqueeze(1)
    py = ((bboxes[:, 1] + bboxes[:, 3]) * 0.5).unsqueeze(1)
    pw = (bboxes[:, 2] - bboxes[:, 0]).unsqueeze(1)
    ph = (bboxes[:, 3] - bboxes[:, 1]).unsqueeze(1)
    gw, gh = pw * dw.exp(), ph * dh.exp()
    gx, gy = px + pw * dx, py + ph * dy
    x1, y1, x2, y2 = gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5
    max_h, max_w = _max_hw(max_shape)
    if max_h > 0 and max_w > 0:
        x1, x2 = x1.clamp(min=0, max=max_w), x2.clamp(min=0, max=max_w)
        y1, y2 = y1.clamp(min=0, max=max_h), y2.clamp(min=0, max=max_h)
    return torch.stack([x1, y1, x2, y2], dim=-1).view_as(pred_bboxes)


def gv_fix_encode(polys):
    """GVFixCoder.encode as a torch composition (coder.py:L152-185).  torch.argmax / argmin return the FIRST extreme:
    the lowest-vertex-index tie rule of the fused kernel."""
    xs, ys = polys[:, 0::2], polys[:, 1::2]
    max_x, max_x_idx = xs.max(dim=1).values, xs.argmax(dim=1)
    min_x, min_x_idx = xs.min(dim=1).values, xs.argmin(dim=1)
    max_y, max_y_idx = ys.max(dim=1).values, ys.argmax(dim=1)
    min_y, min_y_idx = ys.min(dim=1).values, ys.argmin(dim=1)
    pick = lambda v, idx: v.gather(1, idx[:, None])[:, 0]   # noqa: E731
    t_x, t_y = pick(xs, min_y_idx), pick(ys, min_y_idx)
    r_x, r_y = pick(xs, max_x_idx), pick(ys, max_x_idx)
    d_x = pick(xs, max_y_idx)
    l_y = pick(ys, min_x_idx)
    dt = (t_x - min_x) / (max_x - min_x)
    dr = (r_y - min_y) / (max_y - min_y)
    dd = (max_x - d_x) / (max_x - min_x)
    dl = (max_y - l_y) / (max_y - min_y)
    h_mask = (t_y - r_y == 0) | (r_x - d_x == 0)
    fix = torch.stack([dt, dr, dd, dl], dim=1)
    return torch.where(h_mask[:, None], torch.ones_like(fix), fix)


def gv_fix_decode(hbboxes, fix_deltas):
    """GVFixCoder.decode as a torch composition (coder.py:L188-205): (n, 4C), (n, 4C) -> (n, 8C)"""
    x1, y1, x2, y2 = hbboxes[:, 0::4], hbboxes[:, 1::4], hbboxes[:, 2::4], hbboxes[:, 3::4]
    w, h = x2 - x1, y2 - y1
    pred_t_x = x1 + w * fix_deltas[:, 0::4]
    pred_r_y = y1 + h * fix_deltas[:, 1::4]
    pred_d_x = x2 - w * fix_deltas[:, 2::4]
    pred_l_y = y2 - h * fix_deltas[:, 3::4]
    return torch.stack([pred_t_x, y1, x2, pred_r_y, pred_d_x, y2, x1, pred_l_y], dim=-1).flatten(1)


def gv_ratio_encode(polys):
    """GVRatioCoder.encode as a torch composition (coder.py:L215-228)"""
    xs, ys = polys[:, 0::2], polys[:, 1::2]
    h_areas = (xs.max(dim=1).values - xs.min(dim=1).values) * (ys.max(dim=1).values - ys.min(dim=1).values)
    areas = torch.zeros_like(h_areas)
    for i in range(4):
        j = (i + 1) % 4
        areas = areas + 0.5 * (xs[:, i] * ys[:, j] - xs[:, j] * ys[:, i])
    return (torch.abs(areas) / h_areas)[:, None]


def gliding_targets(rois, polys, means, stds, fused=None):
    """the target pass of GlidingHead for matched (roi, gt polygon) rows (gliding_head.py:L309-321): bbox_targets (n,4),
    fix_targets (n,4), ratio_targets (n,1) -- one launch (jdet_gliding_targets) on a device, the three compositions
    elsewhere.  `fused`: None = decide by `_fused32_ok`, False = the composition."""
    if (fused is None and _fused32_ok(rois, polys) and rois.shape[1] == 4 and polys.shape[1] == 8) or fused:
        r, p = L.f32c(rois), L.f32c(polys)
        n = r.shape[0]
        assert tuple(r.shape) == (n, 4) and tuple(p.shape) == (n, 8)
        bbox_t = torch.empty((n, 4), dtype=torch.float32, device=r.device)
        fix_t = torch.empty((n, 4), dtype=torch.float32, device=r.device)
        ratio_t = torch.empty((n, 1), dtype=torch.float32, device=r.device)
        L.check(L.lib().jdet_gliding_targets(L.ptr(r), L.ptr(p), n, L.vecn(means, 4), L.vecn(stds, 4), L.ptr(bbox_t),
                                             L.ptr(fix_t), L.ptr(ratio_t), L.stream_ptr(r)), "jdet_gliding_targets")
        return bbox_t, fix_t, ratio_t
    return gv_delta_encode(rois, poly2hbb(polys), means, stds), gv_fix_encode(polys), gv_ratio_encode(polys)


def gliding_decode(rois, bbox_pred, fix_pred, ratio_pred, means, stds, max_shape=None, wh_ratio_clip=16 / 1000,
                   ratio_thr=0.8, scale=(1., 1., 1., 1.), fused=None):
    """the decode pass of GlidingHead (gliding_head.py:L362-374): rois (n,4), bbox_pred / fix_pred (n,4C), ratio_pred
    (n,C) -> polygons (n, 8C), divided by scale.repeat(2).  One launch (jdet_gliding_decode) on a device."""
    if (fused is None and _fused32_ok(rois, bbox_pred, fix_pred, ratio_pred) and rois.shape[1] == 4) or fused:
        r, b, f, q = L.f32c(rois), L.f32c(bbox_pred), L.f32c(fix_pred), L.f32c(ratio_pred)
        n, ncls = q.shape
        assert b.shape == (n, 4 * ncls) and f.shape == (n, 4 * ncls) and tuple(r.shape) == (n, 4)
        out = torch.empty((n, 8 * ncls), dtype=torch.float32, device=r.device)
        max_h, max_w = _max_hw(max_shape)
        L.check(L.lib().jdet_gliding_decode(L.ptr(r), L.ptr(b), L.ptr(f), L.ptr(q), n, ncls, L.vecn(means, 4),
                                            L.vecn(stds, 4), float(wh_ratio_clip), max_h, max_w, float(ratio_thr),
                                            L.vecn(scale, 4), L.ptr(out), L.stream_ptr(r)), "jdet_gliding_decode")
        return out
    boxes = gv_delta_decode(rois, bbox_pred, means, stds, max_shape, wh_ratio_clip)
    polys = gv_fix_decode(boxes, fix_pred)
    boxes = boxes.view(*ratio_pred.shape, 4)
    polys = polys.view(*ratio_pred.shape, 8)
    polys = torch.where((ratio_pred > ratio_thr)[..., None], hbb2poly(boxes), polys)
    polys = polys / polys.new_tensor(scale).repeat(2)
    return polys.view(polys.size(0), -1)


@BOXES.register_module()
class GVFixCoder:
    """Gliding offsets (coder.py:L143-205): the positions of the top / right / bottom / left vertex of a quadrilateral
    along the sides of its enclosing box, as fractions (dt, dr, dd, dl); rows the reference's `h_mask` marks (the top
    and right vertex share a y, or the right and bottom vertex an x: a horizontal rectangle) are all 1."""

    def __init__(self):
        pass

    def encode(self, polys):
        assert polys.size(1) == 8
        if _fused32_ok(polys):
            # the fused launch computes the three target groups together; a dummy unit roi keeps its delta encode
            # finite.
            # Not the hot path: the head takes all three from ONE `gliding_targets` call; a standalone coder call pays a
            # launch of its own and drops the two outputs it does not return
            rois = const_like((0., 0., 1., 1.), polys).expand(polys.shape[0], 4)
            return gliding_targets(rois, polys, (0.,) * 4, (1.,) * 4, fused=True)[1]
        return gv_fix_encode(polys)

    def decode(self, hbboxes, fix_deltas):
        return gv_fix_decode(hbboxes, fix_deltas)


@BOXES.register_module()
class GVRatioCoder:
    """Obliquity ratio (coder.py:L208-231): |polygon area| / area of its enclosing box."""

    def __init__(self):
        pass

    def encode(self, polys):
        assert polys.size(1) == 8
        if _fused32_ok(polys):       # a launch of its own, as in GVFixCoder.encode: the head uses `gliding_targets`
            rois = const_like((0., 0., 1., 1.), polys).expand(polys.shape[0], 4)
            return gliding_targets(rois, polys, (0.,) * 4, (1.,) * 4, fused=True)[2]
        return gv_ratio_encode(polys)

    def decode(self, bboxes, bboxes_pred):
        raise NotImplementedError


@BOXES.register_module()
class GVDeltaXYWHBBoxCoder:
    """Horizontal (dx, dy, dw, dh) codec of the Gliding Vertex RPN and head (coder.py:L233-320); decode is class-wise
    and clamps to `max_shape` = (h, w)."""

    def __init__(self, target_means=(0., 0., 0., 0.), target_stds=(1., 1., 1., 1.)):
        self.means = target_means
        self.stds = target_stds

    def encode(self, bboxes, gt_bboxes):
        assert bboxes.size(0) == gt_bboxes.size(0)
        assert bboxes.size(-1) == gt_bboxes.size(-1) == 4
        assert bboxes.size() == gt_bboxes.size()
        if _fused32_ok(bboxes, gt_bboxes):
            a, g = L.f32c(bboxes), L.f32c(gt_bboxes)
            out = torch.empty_like(a)
            L.check(L.lib().jdet_gv_delta_encode(L.ptr(a), L.ptr(g), a.shape[0], L.vecn(self.means, 4),
                                                 L.vecn(self.stds, 4), L.ptr(out), L.stream_ptr(a)),
                    "jdet_gv_delta_encode")
            return out
        return gv_delta_encode(bboxes.float() if bboxes.dtype != torch.float64 else bboxes,
                               gt_bboxes.float() if gt_bboxes.dtype != torch.float64 else gt_bboxes,
                               self.means, self.stds)

    def decode(self, bboxes, pred_bboxes, max_shape=None, wh_ratio_clip=16 / 1000):
        assert pred_bboxes.size(0) == bboxes.size(0)
        if _fused32_ok(bboxes, pred_bboxes) and bboxes.shape[1] == 4 and pred_bboxes.shape[1] % 4 == 0:
            a, d = L.f32c(bboxes), L.f32c(pred_bboxes)
            out = torch.empty_like(d)
            max_h, max_w = _max_hw(max_shape)
            L.check(L.lib().jdet_gv_delta_decode(L.ptr(a), L.ptr(d), d.shape[0], d.shape[1] // 4,
                                                 L.vecn(self.means, 4), L.vecn(self.stds, 4), float(wh_ratio_clip),
                                                 max_h, max_w, L.ptr(out), L.stream_ptr(d)), "jdet_gv_delta_decode")
            return out
        return gv_delta_decode(bboxes, pred_bboxes, self.means, self.stds, max_shape, wh_ratio_clip)


# the fused routes of Circular Smooth Label: CSLCoder's kernels, the angle-loss node and the head's in-place decode
# (A/B switch; profiles/csl.md).  Read at call time.
CSL_FUSED = os.environ.get("JDET_CSL_FUSED", "1") != "0"


@BOXES.register_module()
class CSLCoder:
    """Circular Smooth Label coder (coder.py:L521-605 of the reference): an angle delta becomes a smooth label over
    `coding_len = int(180 // omega)` bins, a row of bin scores becomes the angle of its best bin.  include/jdet_hip_csl.h
    states the rules; two of them are this project's:

      * the bin of a target is evaluated in float32 in the reference's operation order, whatever the input's dtype;
      * where the reference scatters several values into one bin (gaussian window, coding_len < 180: the winner of its
        duplicate indices is undefined) the LARGEST wins, i.e. the label is exp(-d^2 / (2 radius^2)) of the circular bin
        distance d.  rect / triangle windows wider than the code (2 radius > coding_len) are refused.

    omega: degrees per bin, int or float; radius: int for 'triangle' / 'rect', any positive number for 'gaussian'."""

    def __init__(self, omega=1, window="gaussian", radius=6):
        assert window in ["gaussian", "triangle", "rect", "pulse"]
        self.angle_range = 180
        self.angle_offset = 45
        self.omega = omega
        self.window = window
        self.radius = radius
        self.coding_len = int(self.angle_range // omega)
        if self.coding_len < 1:
            raise ValueError("omega=%r leaves no bin" % (omega,))
        if window in ("rect", "triangle") and (radius != int(radius) or radius < 1 or 2 * radius > self.coding_len):
            raise ValueError("a '%s' window of radius %r does not fit %d bins (an integer radius, 2 * radius <= coding_len)"
                             % (window, radius, self.coding_len))
        if window == "gaussian" and not radius > 0:
            raise ValueError("a gaussian window needs radius > 0, got %r" % (radius,))

    def bins(self, angle_targets):
        """(n, 1) angle deltas -> (n, 1) int64 bins in [0, coding_len): float32, the reference's operation order, truncated
        toward zero, floor-mod.  The divisor is a tensor: the framework divides by a host scalar through its reciprocal."""
        a = angle_targets.float()
        deg = (a * (180 / math.pi) + self.angle_offset) / a.new_full((), self.omega)
        return deg.long() % self.coding_len

    def encode(self, angle_targets):
        """(n, 1) -> (n, coding_len) labels of angle_targets' dtype"""
        assert angle_targets.dim() == 2 and angle_targets.shape[1] == 1
        n, Lc = angle_targets.shape[0], self.coding_len
        if CSL_FUSED and Lc <= 180 and _fused32_ok(angle_targets) and n > 0:
            a = L.f32c(angle_targets)
            out = torch.empty((n, Lc), dtype=torch.float32, device=a.device)
            L.check(L.lib().jdet_csl_encode(L.ptr(a), n, Lc, float(self.omega), L.CSL_WINDOWS[self.window],
                                            float(self.radius), L.ptr(out), L.stream_ptr(a)), "jdet_csl_encode")
            return out
        dtype = angle_targets.dtype if angle_targets.is_floating_point() else torch.float32
        d = (torch.arange(Lc, device=angle_targets.device)[None, :] - self.bins(angle_targets)) % Lc
        r = self.radius
        if self.window == "pulse":
            y = (d == 0).double()
        elif self.window == "rect":
            y = ((d < r) | (d >= Lc - r)).double()
        elif self.window == "triangle":
            b = torch.where(d < r, d, Lc - d)
            y = torch.where(b <= r, 1.0 - b.double() / r, torch.zeros((), dtype=torch.float64, device=d.device))
        else:
            cd = torch.minimum(d, Lc - d).double()
            y = torch.exp(-(cd * cd) / (2 * r ** 2))
        return y.to(dtype)

    def decode(self, angle_preds, index=None):
        """(rows, coding_len) bin scores -> the angle of the first best bin of every row, or of the rows `index` (int64)
        names: (n,) of angle_preds' dtype.  On the fused route the rows are read in place (jdet_csl_decode)."""
        assert angle_preds.dim() == 2 and angle_preds.shape[1] == self.coding_len
        n = angle_preds.shape[0] if index is None else index.shape[0]
        if (CSL_FUSED and self.coding_len <= 180 and _fused32_ok(angle_preds) and angle_preds.is_contiguous() and n > 0 and
                (index is None or (index.is_cuda and index.dtype == torch.int64 and index.dim() == 1))):
            out = torch.empty((n,), dtype=torch.float32, device=angle_preds.device)
            idx = index.contiguous() if index is not None else None
            L.check(L.lib().jdet_csl_decode(L.ptr(angle_preds), angle_preds.shape[0], L.ptr(idx), n, self.coding_len,
                                            float(self.omega), L.ptr(out), L.stream_ptr(angle_preds)), "jdet_csl_decode")
            return out
        if index is not None:
            angle_preds = angle_preds[index]
        idx = angle_preds.argmax(dim=1)
        angle = ((idx.double() + 0.5) * self.omega) % self.angle_range - self.angle_offset
        return (angle * (math.pi / 180)).to(angle_preds.dtype)
