"""Rotated box algebra used by the named configs.  Mirrors python/jdet/models/boxes/box_ops.py:
norm_angle L176-178, bbox2delta_rotated L180-226, delta2bbox_rotated L229-285,
rotated_box_to_poly L592-613, points_in_rotated_boxes L725-741.

On a HIP device and outside autograd the two coders run as ONE fused fp32 kernel each
(csrc/box_codec_assign.hip; half inputs are up-cast); the torch expressions below are the differentiable form
(needed when a loss is applied to decoded boxes), define the same arithmetic and serve float64 inputs in float64.
"""
import math

import torch

from jdet_amd import _lib as L


def norm_angle(angle, range=(float(-math.pi / 4), float(math.pi))):
    # Python-style floor mod (Jittor's float % is unpinned; floor-mod is what makes the
    # documented [-pi/4, 3pi/4) range come out)
    return torch.remainder(angle - range[0], range[1]) + range[0]


def _fused_ok(*ts):
    return all(t.is_cuda for t in ts) and not (torch.is_grad_enabled() and any(t.requires_grad for t in ts))


def _fused_no64_ok(*ts):
    """`_fused_ok` unless an input is float64: the kernels are fp32, and a float64 caller is promised the float64
    composition below, not a silent down-cast.  Half and bfloat16 inputs (a head under autocast) are up-cast to the
    one fp32 launch, as before"""
    return _fused_ok(*ts) and not any(t.dtype == torch.float64 for t in ts)


def _vec5(v):
    import ctypes
    return (ctypes.c_float * 5)(*[float(x) for x in v])


def bbox2delta_rotated(proposals, gt, means=(0., 0., 0., 0., 0.), stds=(1., 1., 1., 1., 1.)):
    assert proposals.size() == gt.size()
    if _fused_no64_ok(proposals, gt) and proposals.dim() == 2:
        p, g = L.f32c(proposals), L.f32c(gt)
        out = torch.empty_like(p)
        L.check(L.lib().jdet_bbox2delta_rotated(L.ptr(p), L.ptr(g), p.shape[0], _vec5(means), _vec5(stds),
                                                L.ptr(out), L.stream_ptr(p)), "jdet_bbox2delta_rotated")
        return out
    gt_widths, gt_heights, gt_angle = gt[..., 2], gt[..., 3], gt[..., 4]
    pw, ph, pa = proposals[..., 2], proposals[..., 3], proposals[..., 4]
    cosa, sina = torch.cos(pa), torch.sin(pa)
    coord = gt[..., 0:2] - proposals[..., 0:2]
    dx = (cosa * coord[..., 0] + sina * coord[..., 1]) / pw
    dy = (-sina * coord[..., 0] + cosa * coord[..., 1]) / ph
    dw = torch.log(torch.clamp(gt_widths / pw, 1e-30, 1e30))   # jt.safe_log
    dh = torch.log(torch.clamp(gt_heights / ph, 1e-30, 1e30))
    da = norm_angle(gt_angle - pa) / math.pi
    deltas = torch.stack((dx, dy, dw, dh, da), -1)
    means = deltas.new_tensor(means).unsqueeze(0)
    stds = deltas.new_tensor(stds).unsqueeze(0)
    return (deltas - means) / stds


def delta2bbox_rotated(rois, deltas, means=(0., 0., 0., 0., 0.), stds=(1., 1., 1., 1., 1.), max_shape=None,
                       wh_ratio_clip=16 / 1000, clip_border=True):
    """rois (N,5), deltas (N, 5*num_classes) -> (N, 5*num_classes).  `max_shape` / `clip_border` are
    accepted but never applied, exactly as in the reference (box_ops.py:L229-285)."""
    if _fused_no64_ok(rois, deltas) and deltas.dim() == 2 and deltas.shape[1] % 5 == 0:
        r, d = L.f32c(rois), L.f32c(deltas)
        out = torch.empty_like(d)
        L.check(L.lib().jdet_delta2bbox_rotated(L.ptr(r), L.ptr(d), d.shape[0], d.shape[1] // 5, _vec5(means),
                                                _vec5(stds), float(wh_ratio_clip), L.ptr(out),
                                                L.stream_ptr(d)), "jdet_delta2bbox_rotated")
        return out
    means = deltas.new_tensor(means).repeat(1, deltas.size(1) // 5)
    stds = deltas.new_tensor(stds).repeat(1, deltas.size(1) // 5)
    denorm = deltas * stds + means
    dx, dy, dw, dh, dangle = denorm[:, 0::5], denorm[:, 1::5], denorm[:, 2::5], denorm[:, 3::5], denorm[:, 4::5]
    max_ratio = abs(math.log(wh_ratio_clip))
    dw = dw.clamp(min=-max_ratio, max=max_ratio)
    dh = dh.clamp(min=-max_ratio, max=max_ratio)
    roi_x = rois[:, 0].unsqueeze(1).expand_as(dx)
    roi_y = rois[:, 1].unsqueeze(1).expand_as(dy)
    roi_w = rois[:, 2].unsqueeze(1).expand_as(dw)
    roi_h = rois[:, 3].unsqueeze(1).expand_as(dh)
    roi_angle = rois[:, 4].unsqueeze(1).expand_as(dangle)
    gx = dx * roi_w * torch.cos(roi_angle) - dy * roi_h * torch.sin(roi_angle) + roi_x
    gy = dx * roi_w * torch.sin(roi_angle) + dy * roi_h * torch.cos(roi_angle) + roi_y
    gw = roi_w * dw.exp()
    gh = roi_h * dh.exp()
    ga = norm_angle(math.pi * dangle + roi_angle)
    return torch.stack([gx, gy, gw, gh, ga], dim=-1).view_as(deltas)


def rotated_box_to_poly(rrects):
    """(n,5) [xc,yc,w,h,theta] -> (n,8) [x0,y0,...,x3,y3], corners tl, tr, br, bl of the unrotated
    box rotated by theta: x' = c*x - s*y + xc, y' = s*x + c*y + yc (box_ops.py:L592-613)."""
    n = rrects.shape[0]
    if n == 0:
        return rrects.new_zeros((0, 8))
    x_ctr, y_ctr, width, height, angle = rrects[:, 0], rrects[:, 1], rrects[:, 2], rrects[:, 3], rrects[:, 4]
    tl_x, tl_y, br_x, br_y = -width / 2, -height / 2, width / 2, height / 2
    xs = torch.stack([tl_x, br_x, br_x, tl_x], 1)
    ys = torch.stack([tl_y, tl_y, br_y, br_y], 1)
    c, s_ = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
    px = c * xs - s_ * ys + x_ctr[:, None]
    py = s_ * xs + c * ys + y_ctr[:, None]
    return torch.stack([px, py], dim=2).reshape(n, 8)


def points_in_rotated_boxes(points, rrects):
    """(n, 2+) points x (m, 5) boxes -> (n, m) bool, True where the point lies inside the box.  The tensor program of
    box_ops.py:L725-741 as written (atan2 of the offset, cos / sin of the angle difference), kept for API parity: the
    fused assigner (csrc/atss_assign.hip) tests only its candidates, in the algebraic form stated in
    include/jdet_hip.h."""
    offsets = points[:, None, :2] - rrects[None, :, :2]
    offset_angles = torch.atan2(offsets[..., 1], offsets[..., 0])
    offset_distances = offsets.square().sum(-1).sqrt()
    delta_angles = offset_angles - rrects[None, :, 4]
    delta_w = torch.abs(offset_distances * torch.cos(delta_angles))
    delta_h = torch.abs(offset_distances * torch.sin(delta_angles))
    return (delta_w < rrects[None, :, 2] / 2) & (delta_h < rrects[None, :, 3] / 2)


def mintheta_obb(obboxes):
    """(…, 5) boxes with the side order swapped where that brings the angle nearer 0: of theta and theta + pi/2, both
    folded into [-pi/2, pi/2), the one of smaller magnitude (box_ops.py:L679-692; `pi = 3.141592` is the reference's)."""
    from jdet_amd.ops.bbox_transforms import regular_theta
    pi = 3.141592
    x, y, w, h, theta = obboxes.unbind(dim=-1)
    theta1 = regular_theta(theta)
    theta2 = regular_theta(theta + pi / 2)
    first = torch.abs(theta1) < torch.abs(theta2)
    w_regular = torch.where(first, w, h)
    h_regular = torch.where(first, h, w)
    theta_regular = torch.where(first, theta1, theta2)
    return torch.stack([x, y, w_regular, h_regular, theta_regular], dim=-1)


def distance2obb(points, distance, max_shape=None):
    """(n, 2) points + (n, 5) [l, t, r, b, theta] -> (n, 5) regular_obb boxes (box_ops.py:L694-707; `max_shape` is
    accepted and unused, as there).  The inverse of the FCOS point targets: centre = point + R(theta)^T-rotated half
    difference of the distances, size = their sums."""
    from jdet_amd.ops.bbox_transforms import regular_obb
    distance, theta = distance.split([4, 1], dim=1)
    Cos, Sin = torch.cos(theta), torch.sin(theta)
    Matrix = torch.cat([Cos, Sin, -Sin, Cos], dim=1).reshape(-1, 2, 2)
    wh = distance[:, :2] + distance[:, 2:]
    offset_t = ((distance[:, 2:] - distance[:, :2]) / 2).unsqueeze(2)
    offset = torch.bmm(Matrix, offset_t).squeeze(2)
    ctr = points + offset
    return regular_obb(torch.cat([ctr, wh, theta], dim=1))


# ---- the discretised regression distributions of the localization-distillation heads (box_ops.py:L709-723) ------------
DIST_ENDS = (-2.0, 2.0)            # the bins of the four box sides span [-2, 2]
DIST_ANGLE_ENDS = (-5.0, 2.0)      # those of the angle [-5, 2]


def _dist_bins(n, ends, like):
    """e_k = lo + k * ((hi - lo) / n), k = 0 .. n, evaluated in x's dtype (exact in fp32 at n = 8)"""
    lo, hi = ends
    step = torch.tensor((hi - lo), dtype=like.dtype, device=like.device) / n
    return lo + torch.arange(n + 1, dtype=like.dtype, device=like.device) * step


def _integral(x, n, ends):
    # softmax(x) . e as (exp(x - max) . e) / sum exp(x - max): one division per row, so a constant row gives exactly the
    # bins' mean and a saturated one exactly its bin (the kernel's form, csrc/dist_loss.hip)
    y = x.reshape(-1, n + 1)
    y = torch.exp(y - y.max(dim=1, keepdim=True).values.detach())
    return (y * _dist_bins(n, ends, y)).sum(dim=1) / y.sum(dim=1)


def integral(x, n):
    """(rows, 4 * (n + 1)) logits -> (rows, 4): the expectation of each side's distribution over bins on [-2, 2]"""
    return _integral(x, n, DIST_ENDS).reshape(-1, 4)


def integral_angle(x, n):
    """(rows, n + 1) logits -> (rows,): the same for the angle, bins on [-5, 2]"""
    return _integral(x, n, DIST_ANGLE_ENDS).reshape(-1)


def integral_rows(x, n):
    """(rows, 5 * (n + 1)) logits of a distribution head -> (rows, 5) deltas [integral of the four sides, integral_angle].
    fp32 on the device without a gradient: one launch (jdet_dist_integral); otherwise composed from the two above."""
    k = n + 1
    if (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 5 * k and k <= 32 and
            not (torch.is_grad_enabled() and x.requires_grad) and not torch.is_autocast_enabled()):
        x = x.contiguous()
        out = torch.empty((x.shape[0], 5), dtype=torch.float32, device=x.device)
        L.check(L.lib().jdet_dist_integral(L.ptr(x), x.shape[0], n, *DIST_ENDS, *DIST_ANGLE_ENDS, L.ptr(out),
                                           L.stream_ptr(x)), "jdet_dist_integral")
        return out
    return torch.cat([integral(x[:, :4 * k], n), integral_angle(x[:, 4 * k:], n)[:, None]], dim=1)


# ---- the horizontal-anchor algebra of RetinaHead (box_ops.py:L36-86, L117-129, L650-675 of the reference) ----------------
def loc2bbox_r(src_bbox, loc, mean=(0., 0., 0., 0., 0.), std=(1., 1., 1., 1., 1.)):
    """(n, 5) [x, y, w, h, a] sources + (n, 5) offsets -> (n, 5) boxes, with the reference's (x1 + x2) / 2, x2 - x1
    round trip through the corners"""
    if src_bbox.shape[0] == 0:
        return loc.new_zeros((0, 4))
    loc = loc * loc.new_tensor(std) + loc.new_tensor(mean)
    sx, sy, sw, sh = src_bbox[:, 0:1], src_bbox[:, 1:2], src_bbox[:, 2:3], src_bbox[:, 3:4]
    cx = loc[:, 0:1] * sw + sx
    cy = loc[:, 1:2] * sh + sy
    w = torch.exp(loc[:, 2:3]) * sw
    h = torch.exp(loc[:, 3:4]) * sh
    x1, y1, x2, y2 = cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h
    theta = loc[:, 4:5] + src_bbox[:, 4:5]
    return torch.cat([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, theta], dim=1)


def bbox2loc_r(src_bbox, dst_bbox, mean=(0., 0., 0., 0., 0.), std=(1., 1., 1., 1., 1.)):
    """offsets that take (n, 5) sources to (n, 5) targets: the +1 on the source sides and eps = 1e-5 inside the logs are
    the reference's"""
    x, y, w, h = src_bbox[:, 0:1], src_bbox[:, 1:2], src_bbox[:, 2:3], src_bbox[:, 3:4]
    bx, by, bw, bh = dst_bbox[:, 0:1], dst_bbox[:, 1:2], dst_bbox[:, 2:3], dst_bbox[:, 3:4]
    eps = 1e-5
    dx = (bx - x) / (w + 1)
    dy = (by - y) / (h + 1)
    dw = torch.log(bw / (w + 1) + eps)
    dh = torch.log(bh / (h + 1) + eps)
    da = dst_bbox[:, 4:5] - src_bbox[:, 4:5]
    loc = torch.cat([dx, dy, dw, dh, da], dim=1)
    return (loc - loc.new_tensor(mean)) / loc.new_tensor(std)


def bbox_iou(bbox_a, bbox_b):
    """(A, 4) x (K, 4) corner boxes -> (A, K) IoU: area_i = (br.x - tl.x) * (br.y - tl.y) * [tl < br in both],
    area_i / (area_a + area_b - area_i).  csrc/retina.hip evaluates the same operations in the same order."""
    assert bbox_a.shape[1] == 4 and bbox_b.shape[1] == 4
    if bbox_a.numel() == 0 or bbox_b.numel() == 0:
        return bbox_a.new_zeros((bbox_a.shape[0], bbox_b.shape[0]))
    tl = torch.maximum(bbox_a[:, None, :2], bbox_b[:, :2])
    br = torch.minimum(bbox_a[:, None, 2:], bbox_b[:, 2:])
    d = br - tl
    area_i = (d[..., 0] * d[..., 1]) * (tl < br).all(dim=2).to(d.dtype)
    da, db = bbox_a[:, 2:] - bbox_a[:, :2], bbox_b[:, 2:] - bbox_b[:, :2]
    area_a, area_b = da[:, 0] * da[:, 1], db[:, 0] * db[:, 1]
    return area_i / (area_a[:, None] + area_b - area_i)


def rotated_box_to_bbox(rotated_boxes):
    """(n, 5) -> (n, 4) [x0, y0, x1, y1]: the enclosing horizontal box of the four corners"""
    polys = rotated_box_to_poly(rotated_boxes)
    xs, ys = polys[:, 0::2], polys[:, 1::2]
    return torch.stack([xs.min(1).values, ys.min(1).values, xs.max(1).values, ys.max(1).values], dim=1)


def boxes_xywh_to_x0y0x1y1(boxes):
    assert boxes.shape[1] >= 4
    x, y, w, h = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    return torch.cat([torch.stack([x - 0.5 * w, y - 0.5 * h, x + 0.5 * w, y + 0.5 * h], dim=1), boxes[:, 4:]], dim=1)


def boxes_x0y0x1y1_to_xywh(boxes):
    assert boxes.shape[1] >= 4
    x0, y0, x1, y1 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    return torch.cat([torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], dim=1), boxes[:, 4:]], dim=1)


def loc2bbox(src_bbox, loc, mean=(0., 0., 0., 0.), std=(1., 1., 1., 1.)):
    """(n, 4) corner sources + (n, 4) offsets -> (n, 4) corner boxes (box_ops.py:L5-34)"""
    if src_bbox.shape[0] == 0:
        return loc.new_zeros((0, 4))
    loc = loc * loc.new_tensor(std) + loc.new_tensor(mean)
    sw, sh = src_bbox[:, 2:3] - src_bbox[:, 0:1], src_bbox[:, 3:4] - src_bbox[:, 1:2]
    cx = loc[:, 0:1] * sw + (src_bbox[:, 0:1] + 0.5 * sw)
    cy = loc[:, 1:2] * sh + (src_bbox[:, 1:2] + 0.5 * sh)
    w, h = torch.exp(loc[:, 2:3]) * sw, torch.exp(loc[:, 3:4]) * sh
    return torch.cat([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=1)


def bbox2loc(src_bbox, dst_bbox, mean=(0., 0., 0., 0.), std=(1., 1., 1., 1.)):
    """offsets that take (n, 4) corner sources to (n, 4) corner targets (box_ops.py:L88-115)"""
    w, h = src_bbox[:, 2:3] - src_bbox[:, 0:1], src_bbox[:, 3:4] - src_bbox[:, 1:2]
    x, y = src_bbox[:, 0:1] + 0.5 * w, src_bbox[:, 1:2] + 0.5 * h
    bw, bh = dst_bbox[:, 2:3] - dst_bbox[:, 0:1], dst_bbox[:, 3:4] - dst_bbox[:, 1:2]
    bx, by = dst_bbox[:, 0:1] + 0.5 * bw, dst_bbox[:, 1:2] + 0.5 * bh
    eps = 1e-5
    w, h = torch.clamp(w, min=eps), torch.clamp(h, min=eps)
    loc = torch.cat([(bx - x) / w, (by - y) / h, torch.log(torch.clamp(bw / w, 1e-30, 1e30)),
                     torch.log(torch.clamp(bh / h, 1e-30, 1e30))], dim=1)      # jt.safe_log
    return (loc - loc.new_tensor(mean)) / loc.new_tensor(std)
