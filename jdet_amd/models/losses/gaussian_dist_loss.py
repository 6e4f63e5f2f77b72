"""Gaussian distribution box losses.  Mirrors python/jdet/models/losses/gaussian_dist_loss.py:L48-276 (GDLoss:
xy_wh_r_2_xy_sigma, postprocess, gwd_loss, kld_loss, jd_loss, kld_symmax_loss, kld_symmin_loss) and
gaussian_dist_loss_v1.py:L48-156 (GDLoss_v1: gwd_loss, bcd_loss, kld_loss).

The torch functions below are the reference's composition (rows compacted by `weight.mean(-1) > 0`, 2x2 det / inv
written out); they run for CPU tensors and `reduction='none'`.  On a HIP device with reduction mean / sum the head
hands each pyramid level to ONE autograd node (`GaussianLevel`: csrc/gaussian_loss.hip decodes, evaluates the loss
and its gradient in one pass over the level's windows, masked sum, no host sync) -- `GaussianBoxLoss.level`."""
from copy import deepcopy

import torch
from torch import nn

from jdet_amd.utils.registry import LOSSES

from ._level import blocked_rows, loss_workspace, scale_unit_grad


def reduce_loss(loss, reduction="mean", avg_factor=None):
    if avg_factor is None:
        avg_factor = max(loss.shape[0], 1)
    if reduction == "mean":
        loss = loss.sum() / avg_factor
    elif reduction == "sum":
        loss = loss.sum()
    return loss


def xy_wh_r_2_xy_sigma(xywhr):
    """(N, 5) rotated boxes -> centres (N, 2), covariances (N, 2, 2) = R diag(wh / 2)^2 R^T"""
    _shape = xywhr.shape
    assert _shape[-1] == 5
    xy = xywhr[..., :2]
    wh = xywhr[..., 2:4].clamp(1e-7, 1e7).reshape(-1, 2)
    r = xywhr[..., 4]
    cos_r, sin_r = torch.cos(r), torch.sin(r)
    R = torch.stack((cos_r, -sin_r, sin_r, cos_r), dim=-1).reshape(-1, 2, 2)
    S = 0.5 * torch.diag_embed(wh)
    sigma = R.bmm(S.square()).bmm(R.permute(0, 2, 1)).reshape(_shape[:-1] + (2, 2))
    return xy, sigma


def det2(m):
    return m[..., 0, 0] * m[..., 1, 1] - m[..., 0, 1] * m[..., 1, 0]


def inv2(m):
    adj = torch.stack((m[..., 1, 1], -m[..., 0, 1], -m[..., 1, 0], m[..., 0, 0]), -1).reshape(m.shape)
    return adj / det2(m)[..., None, None]


def _trace(m):
    return m[..., 0, 0] + m[..., 1, 1]


def postprocess(distance, fun="log1p", tau=1.0):
    if fun == "log1p":
        distance = torch.log(1 + distance)
    elif fun == "sqrt":
        distance = torch.sqrt(distance.clamp(1e-7))
    elif fun == "none":
        pass
    else:
        raise ValueError(f"Invalid non-linear function {fun}")
    if tau >= 1.0:
        return 1 - 1 / (tau + distance)
    return distance


def gwd_loss(pred, target, fun="log1p", tau=1.0, alpha=1.0, normalize=True, reduction="mean", avg_factor=None):
    xy_p, Sigma_p = pred
    xy_t, Sigma_t = target
    xy_distance = (xy_p - xy_t).square().sum(dim=-1)
    whr_distance = _trace(Sigma_p) + _trace(Sigma_t)
    _t_tr = _trace(Sigma_p.bmm(Sigma_t))
    _t_det_sqrt = (det2(Sigma_p) * det2(Sigma_t)).clamp(0).sqrt()
    whr_distance = whr_distance + (-2) * ((_t_tr + 2 * _t_det_sqrt).clamp(1e-7).sqrt())
    distance = (xy_distance + alpha * alpha * whr_distance).clamp(1e-7).sqrt()
    if normalize:
        scale = 2 * (_t_det_sqrt.clamp(1e-7).sqrt().clamp(1e-7).sqrt()).clamp(1e-7)
        distance = distance / scale
    return reduce_loss(postprocess(distance, fun=fun, tau=tau), reduction, avg_factor)


def kld_loss(pred, target, fun="log1p", tau=1.0, alpha=1.0, sqrt=True, reduction="mean", avg_factor=None):
    """as written in the reference: inv(Sigma_p) divided by det(Sigma_p) once more (identical boxes: 1/det - 1)"""
    xy_p, Sigma_p = pred
    xy_t, Sigma_t = target
    _shape = xy_p.shape
    xy_p, xy_t = xy_p.reshape(-1, 2), xy_t.reshape(-1, 2)
    Sigma_p, Sigma_t = Sigma_p.reshape(-1, 2, 2), Sigma_t.reshape(-1, 2, 2)
    Sigma_p_inv = inv2(Sigma_p) / det2(Sigma_p)[..., None, None]
    dxy = (xy_p - xy_t).unsqueeze(-1)
    xy_distance = 0.5 * dxy.permute(0, 2, 1).bmm(Sigma_p_inv).bmm(dxy).view(-1)
    whr_distance = 0.5 * _trace(Sigma_p_inv.bmm(Sigma_t))
    whr_distance = whr_distance + 0.5 * (torch.log(det2(Sigma_p)) - torch.log(det2(Sigma_t)))
    whr_distance = whr_distance - 1
    distance = xy_distance / (alpha * alpha) + whr_distance
    if sqrt:
        distance = distance.clamp(1e-7).sqrt()
    distance = distance.reshape(_shape[:-1])
    return reduce_loss(postprocess(distance, fun=fun, tau=tau), reduction, avg_factor)


def jd_loss(pred, target, fun="log1p", tau=1.0, alpha=1.0, sqrt=True, reduction="mean", avg_factor=None):
    jd = kld_loss(pred, target, fun="none", tau=0, alpha=alpha, sqrt=False, reduction="none")
    jd = jd + kld_loss(target, pred, fun="none", tau=0, alpha=alpha, sqrt=False, reduction="none")
    jd = jd * 0.5
    if sqrt:
        jd = jd.clamp(1e-7).sqrt()
    return reduce_loss(postprocess(jd, fun=fun, tau=tau), reduction, avg_factor)


def _kld_sym(pick, pred, target, fun, tau, alpha, sqrt, reduction, avg_factor):
    kld_pt = kld_loss(pred, target, fun="none", tau=0, alpha=alpha, sqrt=sqrt, reduction="none")
    kld_tp = kld_loss(target, pred, fun="none", tau=0, alpha=alpha, sqrt=sqrt, reduction="none")
    return reduce_loss(postprocess(pick(kld_pt, kld_tp), fun=fun, tau=tau), reduction, avg_factor)


def kld_symmax_loss(pred, target, fun="log1p", tau=1.0, alpha=1.0, sqrt=True, reduction="mean", avg_factor=None):
    return _kld_sym(torch.maximum, pred, target, fun, tau, alpha, sqrt, reduction, avg_factor)


def kld_symmin_loss(pred, target, fun="log1p", tau=1.0, alpha=1.0, sqrt=True, reduction="mean", avg_factor=None):
    return _kld_sym(torch.minimum, pred, target, fun, tau, alpha, sqrt, reduction, avg_factor)


# ---- gaussian_dist_loss_v1.py ----------------------------------------------------------------------------------------
def gwd_loss_v1(pred, target, fun="sqrt", tau=2.0, reduction="mean", avg_factor=None):
    mu_p, sigma_p = pred
    mu_t, sigma_t = target
    xy_distance = (mu_p - mu_t).square().sum(dim=-1)
    whr_distance = _trace(sigma_p) + _trace(sigma_t)
    _t_tr = _trace(sigma_p.bmm(sigma_t))
    _t_det_sqrt = (det2(sigma_p) * det2(sigma_t)).clamp(0).sqrt()
    whr_distance = whr_distance + (-2) * (_t_tr + 2 * _t_det_sqrt).clamp(0).sqrt()
    gwd_dis = (xy_distance + whr_distance).clamp(min=1e-6)
    if fun == "sqrt":
        loss = 1 - 1 / (tau + torch.sqrt(gwd_dis))
    elif fun == "log1p":
        loss = 1 - 1 / (tau + torch.log(1 + gwd_dis))
    else:
        scale = 2 * (_t_det_sqrt.sqrt().sqrt()).clamp(1e-7)
        loss = torch.log(1 + torch.sqrt(gwd_dis) / scale)
    return reduce_loss(loss, reduction, avg_factor)


def bcd_loss_v1(pred, target, fun="log1p", tau=1.0, reduction="mean", avg_factor=None):
    mu_p, sigma_p = pred
    mu_t, sigma_t = target
    mu_p, mu_t = mu_p.reshape(-1, 2), mu_t.reshape(-1, 2)
    sigma_p, sigma_t = sigma_p.reshape(-1, 2, 2), sigma_t.reshape(-1, 2, 2)
    delta = (mu_p - mu_t).unsqueeze(-1)
    sigma = 0.5 * (sigma_p + sigma_t)
    sigma_inv = inv2(sigma)
    term1 = torch.log(det2(sigma) / torch.sqrt(det2(sigma_t.matmul(sigma_p)))).reshape(-1, 1)
    term2 = delta.transpose(-1, -2).matmul(sigma_inv).matmul(delta).squeeze(-1)
    bcd_dis = (0.5 * term1 + 0.125 * term2).clamp(min=1e-6)
    if fun == "sqrt":
        loss = 1 - 1 / (tau + torch.sqrt(bcd_dis))
    elif fun == "log1p":
        loss = 1 - 1 / (tau + torch.log(1 + bcd_dis))
    else:
        loss = 1 - 1 / (tau + bcd_dis)
    return reduce_loss(loss, reduction, avg_factor)


def kld_loss_v1(pred, target, fun="log1p", tau=1.0, reduction="mean", avg_factor=None):
    """GDLoss_v1's KLD: inverts Sigma_t (GDLoss's inverts Sigma_p), no 0.5 factors, clamp at 1e-6"""
    mu_p, sigma_p = pred
    mu_t, sigma_t = target
    mu_p, mu_t = mu_p.reshape(-1, 2), mu_t.reshape(-1, 2)
    sigma_p, sigma_t = sigma_p.reshape(-1, 2, 2), sigma_t.reshape(-1, 2, 2)
    delta = (mu_p - mu_t).unsqueeze(-1)
    sigma_t_inv = inv2(sigma_t)
    term1 = delta.transpose(-1, -2).matmul(sigma_t_inv).matmul(delta).squeeze(-1)
    term2 = _trace(sigma_t_inv.matmul(sigma_p)).reshape(-1, 1) + \
        torch.log(det2(sigma_t) / det2(sigma_p)).reshape(-1, 1)
    kl_dis = (term1 + term2 - 2).clamp(min=1e-6)
    if fun == "sqrt":
        kl_loss = 1 - 1 / (tau + torch.sqrt(kl_dis))
    else:
        kl_loss = 1 - 1 / (tau + torch.log(1 + kl_dis))
    return reduce_loss(kl_loss, reduction, avg_factor)


def positive_rows(weight, *tensors):
    """the rows the reference keeps: weight.mean(-1) > 0 (the weight is a mask only); no weight: every row"""
    if weight is None:
        return tensors
    if weight.dim() > 1:
        assert weight.shape == tensors[0].shape
        weight = weight.mean(-1)
    mask = (weight > 0).detach()
    return tuple(t[mask] for t in tensors)


# ---- the level node --------------------------------------------------------------------------------------------------
class GaussianLevel(torch.autograd.Function):
    """(sum of the row losses over the counted rows / avg_factor) * loss_weight of one pyramid level as ONE node
    (csrc/gaussian_loss.hip: jdet_gaussian_loss_level; backward: jdet_loss_grad_scale).  deltas (rows, 5) contiguous;
    target / weight (rows, 5) or (blocks, rows_per_block, 5) windows read in place; anchors (A_l, 5), row r -> r % A_l."""

    @staticmethod
    def forward(ctx, deltas, target, weight, anchors, params, avg_factor, loss_weight):
        from jdet_amd import _lib as L
        p = deltas.contiguous()
        rows = p.shape[0]
        tb = blocked_rows(target, 5)
        wb = blocked_rows(weight, 5) if weight is not None else (1, 0)
        anc = anchors.contiguous() if anchors is not None else None
        out = torch.empty((), dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p)
        ws, wsb = loss_workspace(p.device)
        L.check(L.lib().jdet_gaussian_loss_level(
            L.ptr(p), L.ptr(target), tb[0], tb[1], L.ptr(weight) if weight is not None else None, wb[0], wb[1],
            L.ptr(anc), anc.shape[0] if anc is not None else 0, rows, params, L.ptr(avg_factor), float(loss_weight),
            out.data_ptr(), L.ptr(grad), L.ptr(ws), wsb, L.stream_ptr(p)), "jdet_gaussian_loss_level")
        ctx.save_for_backward(grad, avg_factor)
        ctx.loss_weight = float(loss_weight)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        grad, avg = ctx.saved_tensors
        return (scale_unit_grad(grad, grad_out, avg, ctx.loss_weight),) + (None,) * 6


def level_params(kind, fun, coder=None, decode_pred=False, decode_target=False, tau=0.0, alpha=1.0, normalize=True,
                 sqrt=True, beta=1.0 / 9.0, eps=1e-6, wh_ratio_clip=16 / 1000):
    """jdet_gaussian_loss_params_t of one loss configuration"""
    from jdet_amd import _lib as L
    q = L.GaussianLossParams()
    q.kind, q.fun = L.GD_KINDS[kind], L.GD_FUNS[fun]
    q.tau, q.alpha, q.normalize, q.sqrt_dist = float(tau), float(alpha), int(bool(normalize)), int(bool(sqrt))
    q.beta, q.eps = float(beta), float(eps)
    q.decode_pred, q.decode_target = int(bool(decode_pred)), int(bool(decode_target))
    means = coder.means if coder is not None else (0., 0., 0., 0., 0.)
    stds = coder.stds if coder is not None else (1., 1., 1., 1., 1.)
    for k in range(5):
        q.means[k], q.stds[k] = float(means[k]), float(stds[k])
    q.wh_ratio_clip = float(wh_ratio_clip)
    return q


def _node_ok(deltas, target, weight, anchors, avg_factor, reduction, coder, decoding):
    from jdet_amd.models.boxes.coder import DeltaXYWHABBoxCoder
    if reduction not in ("mean", "sum") or (reduction == "mean" and avg_factor is None):
        return False
    if not (deltas.is_cuda and deltas.dtype == torch.float32 and deltas.dim() == 2 and deltas.shape[1] == 5 and
            deltas.shape[0] > 0 and not torch.is_autocast_enabled() and not target.requires_grad):
        return False
    if torch.is_tensor(avg_factor) and not (avg_factor.is_cuda and avg_factor.numel() == 1 and
                                            not avg_factor.requires_grad):
        return False
    if decoding and not isinstance(coder, DeltaXYWHABBoxCoder):
        return False
    for t in (target, weight):
        if t is not None and (t.dtype != torch.float32 or t.numel() != deltas.numel() or blocked_rows(t, 5) is None):
            return False
    return anchors is None or (anchors.dtype == torch.float32 and deltas.shape[0] % anchors.shape[-2] == 0)


class GaussianBoxLoss(nn.Module):
    """what GDLoss, GDLoss_v1 and KFLoss share: the per-level entry point of the anchor heads"""
    decodes_target = False

    def _params(self, coder, decode_pred, decode_target):
        raise NotImplementedError

    def _composed(self, deltas, anchors, target, weight, avg_factor, coder, decode_pred):
        raise NotImplementedError

    def level(self, deltas, anchors, target, weight, avg_factor, coder, decode_pred):
        """one pyramid level of a dense head: deltas (rows, 5) in (image, location, anchor) order, anchors (N, A_l, 5)
        (every image has the same grid anchors), target / weight (N, A_l, 5) windows of the per-image arrays"""
        decode_target = self.decodes_target
        decode_pred = decode_pred or self.decodes_target
        anc = anchors[0] if anchors.dim() == 3 else anchors
        if _node_ok(deltas, target, weight, anc, avg_factor, self.reduction, coder, decode_pred or decode_target):
            avg = avg_factor
            if self.reduction == "sum":
                avg = torch.ones((), dtype=torch.float32, device=deltas.device)
            elif not torch.is_tensor(avg):
                avg = torch.full((), float(avg), dtype=torch.float32, device=deltas.device)
            avg = avg.reshape(()).to(torch.float32)
            return GaussianLevel.apply(deltas, target, weight, anc,
                                       self._params(coder, decode_pred, decode_target), avg, self.loss_weight)
        return self._composed(deltas, anchors.reshape(-1, 5), target.reshape(-1, 5),
                              weight.reshape(-1, 5) if weight is not None else None, avg_factor, coder, decode_pred)


@LOSSES.register_module()
class GDLoss(GaussianBoxLoss):
    BAG_GD_LOSS = {"gwd": gwd_loss, "kld": kld_loss, "jd": jd_loss, "kld_symmax": kld_symmax_loss,
                   "kld_symmin": kld_symmin_loss}
    BAG_PREP = {"xy_wh_r": xy_wh_r_2_xy_sigma}

    def __init__(self, loss_type, representation="xy_wh_r", fun="log1p", tau=0.0, alpha=1.0, reduction="mean",
                 loss_weight=1.0, **kwargs):
        super().__init__()
        assert reduction in ["none", "sum", "mean"]
        assert fun in ["log1p", "none", "sqrt"]
        assert loss_type in self.BAG_GD_LOSS
        self.loss_type = loss_type
        self.loss = self.BAG_GD_LOSS[loss_type]
        self.preprocess = self.BAG_PREP[representation]
        self.fun = fun
        self.tau = tau
        self.alpha = alpha
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.kwargs = kwargs

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        _kwargs = deepcopy(self.kwargs)
        _kwargs.update(kwargs)
        pred, target = positive_rows(weight, pred, target)
        return self.loss(self.preprocess(pred), self.preprocess(target), fun=self.fun, tau=self.tau, alpha=self.alpha,
                         avg_factor=avg_factor, reduction=reduction, **_kwargs) * self.loss_weight

    execute = forward

    def _params(self, coder, decode_pred, decode_target):
        kw = self.kwargs
        return level_params(self.loss_type, self.fun, coder, decode_pred, decode_target, tau=self.tau,
                            alpha=self.alpha, normalize=kw.get("normalize", True), sqrt=kw.get("sqrt", True))

    def _composed(self, deltas, anchors, target, weight, avg_factor, coder, decode_pred):
        n = deltas.shape[0]
        pred = coder.decode(anchors.repeat(n // anchors.shape[0], 1) if anchors.shape[0] != n else anchors, deltas) \
            if decode_pred else deltas
        return self.forward(pred, target, weight, avg_factor=avg_factor)


@LOSSES.register_module()
class GDLoss_v1(GaussianBoxLoss):
    BAG_GD_LOSS = {"kld": kld_loss_v1, "bcd": bcd_loss_v1, "gwd": gwd_loss_v1}

    def __init__(self, loss_type, fun="sqrt", tau=1.0, reduction="mean", loss_weight=1.0, **kwargs):
        super().__init__()
        assert reduction in ["none", "sum", "mean"]
        assert fun in ["log1p", "sqrt", ""]
        assert loss_type in self.BAG_GD_LOSS
        self.loss_type = loss_type
        self.loss = self.BAG_GD_LOSS[loss_type]
        self.preprocess = xy_wh_r_2_xy_sigma
        self.fun = fun
        self.tau = tau
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.kwargs = kwargs

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        _kwargs = deepcopy(self.kwargs)
        _kwargs.update(kwargs)
        pred, target = positive_rows(weight, pred, target)
        return self.loss(self.preprocess(pred), self.preprocess(target), fun=self.fun, tau=self.tau,
                         reduction=reduction, avg_factor=avg_factor, **_kwargs) * self.loss_weight

    execute = forward

    def _params(self, coder, decode_pred, decode_target):
        return level_params(self.loss_type + "_v1", self.fun, coder, decode_pred, decode_target, tau=self.tau)

    _composed = GDLoss._composed
