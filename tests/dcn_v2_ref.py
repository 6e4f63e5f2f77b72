"""Float64 statements of the DCN v2 operators, written from the reference text (ops/dcn_v2.py), not from the kernels:
deformable position-sensitive RoI pooling (L832-932 forward, L1007-1116 backward) and the three modulated sampling
kernels (L60-149 im2col, L380-440 + L506-558 col2im, L560-627 the offset / mask gradient).  numpy only: importable
without a GPU and without the C oracle.

All arithmetic is float64 on the float32 inputs; every DECISION follows the text's rule:
  pooling      round() half away from zero; a sample outside [-0.5, W - 0.5] x [-0.5, H - 0.5] is skipped, one ON a
               threshold is kept; kept samples are clamped to [0, W - 1], then read between floor and CEIL (an integer
               coordinate reads one pixel); max(width, 0.1); part / group cell = floor of the text's own float
               expression (float(ph) / P * part is evaluated in float32 as the text writes it: it is an integer
               decision, 3.f / 7 * 7 is not 3 in every precision)
  convolution  a sample counts on the OPEN interval -1 < h < H; corners floor / floor + 1, each zero outside the map;
               the coordinate weights of dmcn_get_coordinate_weight hold at integer positions as written (one-sided)
Two rules are the project's own (stated in csrc/deform_psroi_pool.hip and oracle/jdet_oracle.cpp): a batch index
outside [0, N) pools nothing and receives no gradient (the text reads out of bounds), and count 0 gives output 0.

Every function also returns the MARGINS by which its decisions clear their thresholds, in pixels, so that fixtures
can be filtered where they are generated (as tests/fcos_ref.py does) and the tests then drop nothing."""
import numpy as np

F64 = np.float64


def round_half_away(v):
    """C round(): halves go away from zero (numpy's round sends them to even)"""
    v = np.asarray(v, F64)
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def _dist_to_integer(v):
    return np.abs(v - np.round(v))


class PsMargins:
    """per-RoI margins (R,) of the pooling decisions, +inf where a RoI takes no such decision, and counters of the
    samples that sit exactly on a rule's edge (the exact tier places them there on purpose)"""

    def __init__(self, R):
        self.skip = np.full(R, np.inf)       # |sample - (-0.5)|, |sample - (W - 0.5)| (and H), every sample
        self.clamp = np.full(R, np.inf)      # kept samples: distance of the raw position to 0 and to W - 1 (H - 1)
        self.floor = np.full(R, np.inf)      # kept, unclamped samples: distance to the nearest integer
        self.width = np.full(R, np.inf)      # |end - start - 0.1|, both axes
        self.round = np.full(R, np.inf)      # distance of the four corners to the nearest x.5
        self.on_low = self.on_high = self.on_integer = self.on_last = 0
        self.clamped = self.skipped = self.kept = 0
        self.crossed = 0                     # bins with kept samples that would have none (or the reverse) without trans
        self.width_clamped = 0

    def every(self):
        return np.minimum.reduce([self.skip, self.clamp, self.floor, self.width, self.round])


def _part_cells(P, part):
    """floor(static_cast<float>(ph) / pooled * part_size), in the text's float32"""
    ph = np.arange(P, dtype=np.float32)
    return np.floor(ph / np.float32(P) * np.float32(part)).astype(np.int64)


def _group_cells(P, G):
    pw = np.arange(P, dtype=np.float32)
    g = np.floor(pw * np.float32(G) / np.float32(P)).astype(np.int64)
    return np.minimum(np.maximum(g, 0), G - 1)


def _psroi_roi(n, roi, trans, no_trans, shape, scale, od, G, P, part, spp, tstd, mg):
    """geometry of one RoI -> None (bad batch) or a dict of index / weight arrays over (od, P, P, spp, spp)"""
    N, C, H, W = shape
    ncls = 1 if no_trans else trans.shape[1] // 2
    cec = od if no_trans else od // ncls
    batch = int(roi[0])
    scale, tstd = F64(np.float32(scale)), F64(np.float32(tstd))
    c = np.asarray(roi[1:5], F64)
    mg.round[n] = np.min(np.abs(np.abs(c - np.floor(c)) - 0.5))
    x1, y1, x2, y2 = round_half_away(c)
    sw, sh = x1 * scale - 0.5, y1 * scale - 0.5
    ew, eh = (x2 + 1.0) * scale - 0.5, (y2 + 1.0) * scale - 0.5
    mg.width[n] = min(abs(ew - sw - 0.1), abs(eh - sh - 0.1))
    mg.width_clamped += int(ew - sw < 0.1) + int(eh - sh < 0.1)
    rw, rh = max(ew - sw, 0.1), max(eh - sh, 0.1)
    if batch < 0 or batch >= N:
        return None
    part_c = _part_cells(P, part)
    if no_trans:
        tx = ty = np.zeros((ncls, P, P))
    else:
        t = np.asarray(trans[n], F64).reshape(ncls, 2, part, part) * tstd
        tx = t[:, 0][:, part_c][:, :, part_c]                  # (cls, ph, pw)
        ty = t[:, 1][:, part_c][:, :, part_c]
    # wstart = pw * bin_w + roi_start_w + trans_x * roi_width: depends on (cls, ph, pw); samples add iw * sub_w
    bw, bh = rw / P, rh / P
    ar = np.arange(P, dtype=F64)
    wraw = (ar[None, None, :] * bw + sw + tx * rw)[..., None] + np.arange(spp, dtype=F64) * (bw / spp)   # (cls,ph,pw,iw)
    hraw = (ar[None, :, None] * bh + sh + ty * rh)[..., None] + np.arange(spp, dtype=F64) * (bh / spp)   # (cls,ph,pw,ih)
    okw = ~((wraw < -0.5) | (wraw > W - 0.5))
    okh = ~((hraw < -0.5) | (hraw > H - 0.5))
    keep = okh[..., :, None] & okw[..., None, :]               # (cls, ph, pw, ih, iw)
    wpos = np.minimum(np.maximum(wraw, 0.0), W - 1.0)
    hpos = np.minimum(np.maximum(hraw, 0.0), H - 1.0)
    # ---- margins and edge counters
    mg.skip[n] = min(np.abs(wraw + 0.5).min(), np.abs(wraw - (W - 0.5)).min(), np.abs(hraw + 0.5).min(),
                     np.abs(hraw - (H - 0.5)).min())
    kw_any, kh_any = okw & okh.any(-1, keepdims=True), okh & okw.any(-1, keepdims=True)   # coordinates of kept samples
    for raw, kept, lim in ((wraw, kw_any, W), (hraw, kh_any, H)):
        if kept.any():
            r = raw[kept]
            mg.clamp[n] = min(mg.clamp[n], np.abs(r).min(), np.abs(r - (lim - 1.0)).min())
            free = r[(r > 0.0) & (r < lim - 1.0)]
            if free.size:
                mg.floor[n] = min(mg.floor[n], _dist_to_integer(free).min())
            mg.on_low += int((r == -0.5).sum())
            mg.on_high += int((r == lim - 0.5).sum())
            mg.on_integer += int(((r == np.round(r)) & (r >= 0.0) & (r <= lim - 1.0)).sum())
            mg.on_last += int((r == lim - 1.0).sum())
            mg.clamped += int(((r < 0.0) | (r > lim - 1.0)).sum())
    mg.kept += int(keep.sum())
    mg.skipped += int((~keep).sum())
    if not no_trans:
        w0 = wraw - (tx * rw)[..., None]
        h0 = hraw - (ty * rh)[..., None]
        k0 = (~((h0 < -0.5) | (h0 > H - 0.5)))[..., :, None] & (~((w0 < -0.5) | (w0 > W - 0.5)))[..., None, :]
        mg.crossed += int((keep.any((-1, -2)) != k0.any((-1, -2))).sum())
    # ---- per output channel
    gcell = _group_cells(P, G)
    ctop = np.arange(od)
    cls = ctop // cec
    chan = (ctop[:, None, None] * G + gcell[None, :, None]) * G + gcell[None, None, :]          # (od, ph, pw)
    x0, xc = np.floor(wpos).astype(np.int64), np.ceil(wpos).astype(np.int64)
    y0, yc = np.floor(hpos).astype(np.int64), np.ceil(hpos).astype(np.int64)
    dx, dy = wpos - x0, hpos - y0
    e = lambda a, ax: (a[cls][..., None, :] if ax == "w" else a[cls][..., :, None])               # -> (od,ph,pw,ih,iw)
    full = (od, P, P, spp, spp)
    bc = lambda a: np.broadcast_to(a, full)
    return dict(batch=batch, cls=cls, part=part_c, rw=rw, rh=rh, tstd=tstd, ncls=ncls,
                keep=bc(keep[cls]), chan=bc(chan[..., None, None]),
                x0=bc(e(x0, "w")), x1=bc(e(xc, "w")), y0=bc(e(y0, "h")), y1=bc(e(yc, "h")),
                dx=bc(e(dx, "w")), dy=bc(e(dy, "h")))


def psroi_forward(x, rois, trans, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size, spp,
                  trans_std):
    """x (N, C, H, W), rois (R, 5), trans (R, 2 * classes, part, part) -> out, count (R, od, P, P) float64, PsMargins"""
    x = np.asarray(x, F64)
    R = rois.shape[0]
    od, P = output_dim, pooled_size
    out, cnt = np.zeros((R, od, P, P)), np.zeros((R, od, P, P))
    mg = PsMargins(R)
    for n in range(R):
        q = _psroi_roi(n, rois[n], trans, no_trans, x.shape, spatial_scale, od, group_size, P, part_size, spp,
                       trans_std, mg)
        if q is None:
            continue
        im = x[q["batch"]]
        dx, dy = q["dx"], q["dy"]
        v11, v12 = im[q["chan"], q["y0"], q["x0"]], im[q["chan"], q["y1"], q["x0"]]
        v21, v22 = im[q["chan"], q["y0"], q["x1"]], im[q["chan"], q["y1"], q["x1"]]
        val = (1 - dx) * (1 - dy) * v11 + (1 - dx) * dy * v12 + dx * (1 - dy) * v21 + dx * dy * v22
        c = q["keep"].sum((-1, -2))
        s = np.where(q["keep"], val, 0.0).sum((-1, -2))
        cnt[n] = c
        out[n] = np.where(c > 0, s / np.maximum(c, 1), 0.0)
    return out, cnt, mg


def psroi_backward(grad_out, top_count, x, rois, trans, no_trans, spatial_scale, output_dim, group_size, pooled_size,
                   part_size, spp, trans_std, with_abs=False):
    """-> grad_input (N, C, H, W), grad_trans (like trans, None with no_trans), PsMargins.  with_abs: also the sums of
    the ABSOLUTE values of the terms each accumulator receives (the bound under which any fp32 order is exact)"""
    x, g, top_count = np.asarray(x, F64), np.asarray(grad_out, F64), np.asarray(top_count, F64)
    R = rois.shape[0]
    od, P = output_dim, pooled_size
    gi = np.zeros(x.shape)
    gt = None if no_trans else np.zeros(trans.shape)
    gi_abs, gt_abs = np.zeros(x.shape), (None if no_trans else np.zeros(trans.shape))
    terms = []
    mg = PsMargins(R)
    for n in range(R):
        q = _psroi_roi(n, rois[n], trans, no_trans, x.shape, spatial_scale, od, group_size, P, part_size, spp,
                       trans_std, mg)
        if q is None:
            continue
        live = q["keep"] & (top_count[n] > 0)[..., None, None]
        if not live.any():
            continue
        diff = (g[n] / np.maximum(top_count[n], 1))[..., None, None]
        dx, dy = q["dx"], q["dy"]
        b = q["batch"]
        for ys, xs, wgt in ((q["y0"], q["x0"], (1 - dx) * (1 - dy)), (q["y1"], q["x0"], (1 - dx) * dy),
                            (q["y0"], q["x1"], dx * (1 - dy)), (q["y1"], q["x1"], dx * dy)):
            t = (wgt * diff)[live]
            np.add.at(gi[b], (q["chan"][live], ys[live], xs[live]), t)
            if with_abs:
                np.add.at(gi_abs[b], (q["chan"][live], ys[live], xs[live]), np.abs(t))
                terms.append(t)
        if no_trans:
            continue
        im = x[b]
        U00, U01 = im[q["chan"], q["y0"], q["x0"]], im[q["chan"], q["y1"], q["x0"]]
        U10, U11 = im[q["chan"], q["y0"], q["x1"]], im[q["chan"], q["y1"], q["x1"]]
        tx = (U11 * dy + U10 * (1 - dy) - U01 * dy - U00 * (1 - dy)) * q["tstd"] * diff * q["rw"]
        ty = (U11 * dx + U01 * (1 - dx) - U10 * dx - U00 * (1 - dx)) * q["tstd"] * diff * q["rh"]
        full = live.shape
        ci = np.broadcast_to(q["cls"][:, None, None, None, None], full)[live]
        ph = np.broadcast_to(q["part"][None, :, None, None, None], full)[live]
        pw = np.broadcast_to(q["part"][None, None, :, None, None], full)[live]
        np.add.at(gt[n], (2 * ci, ph, pw), tx[live])
        np.add.at(gt[n], (2 * ci + 1, ph, pw), ty[live])
        if with_abs:
            np.add.at(gt_abs[n], (2 * ci, ph, pw), np.abs(tx[live]))
            np.add.at(gt_abs[n], (2 * ci + 1, ph, pw), np.abs(ty[live]))
            terms += [tx[live], ty[live]]
    if with_abs:
        return gi, gt, mg, dict(gi_abs=gi_abs, gt_abs=gt_abs, terms=np.concatenate(terms) if terms else np.zeros(0))
    return gi, gt, mg


# ------------------------------------------------------------------------------------------- modulated convolution
class ConvMargins:
    def __init__(self):
        self.inside = np.inf      # |h + 1|, |h - H|, |w + 1|, |w - W|: every sample
        self.floor = np.inf       # inside samples: distance to the nearest integer
        self.positions = None     # (h, w) of every sample, for the regime assertions


def _conv_geometry(offset, im_hw, kh, kw, pad, stride, dil, dg):
    """offset (B, dg * 2 * kk, Ho, Wo) -> h, w (B, dg, kk, Ho, Wo) float64 and the margins.  Ho / Wo are the offset's
    own (the reference hands its col2im kernel another padding than the one Wo came from, L651-653)"""
    H, W = im_hw
    off = np.asarray(offset, F64)
    B, _, Ho, Wo = off.shape
    kk = kh * kw
    off = off.reshape(B, dg, kk, 2, Ho, Wo)
    i, j = np.divmod(np.arange(kk), kw)
    h = (np.arange(Ho)[:, None] * stride[0] - pad[0])[None, None, None] + (i * dil[0])[None, None, :, None, None] + off[:, :, :, 0]
    w = (np.arange(Wo)[None, :] * stride[1] - pad[1])[None, None, None] + (j * dil[1])[None, None, :, None, None] + off[:, :, :, 1]
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    m = ConvMargins()
    m.inside = min(np.abs(h + 1).min(), np.abs(h - H).min(), np.abs(w + 1).min(), np.abs(w - W).min())
    if inside.any():
        m.floor = min(_dist_to_integer(h[inside]).min(), _dist_to_integer(w[inside]).min())
    m.positions = (h, w)
    return h, w, inside, m


def _corners(h, w, H, W):
    hl, wl = np.floor(h).astype(np.int64), np.floor(w).astype(np.int64)
    hh, wh = hl + 1, wl + 1
    ok = ((hl >= 0) & (wl >= 0), (hl >= 0) & (wh <= W - 1), (hh <= H - 1) & (wl >= 0), (hh <= H - 1) & (wh <= W - 1))
    ys, xs = (hl, hl, hh, hh), (wl, wh, wl, wh)
    return hl, wl, ok, ys, xs


def _gather(im, b_idx, c_idx, ys, xs, ok, H, W):
    """im[b, c, y, x] where ok, else 0 (the indices are clipped only to make the masked-out reads legal)"""
    v = im[b_idx, c_idx, np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)]
    return np.where(ok, v, 0.0)


def _expand(a, cpg):
    """(B, dg, kk, Ho, Wo) -> (B, dg, cpg, kk, Ho, Wo) view"""
    return np.broadcast_to(a[:, :, None], a.shape[:2] + (cpg,) + a.shape[2:])


def _idx(B, dg, cpg, kk, Ho, Wo):
    shape = (B, dg, cpg, kk, Ho, Wo)
    b = np.broadcast_to(np.arange(B)[:, None, None, None, None, None], shape)
    c = np.broadcast_to((np.arange(dg)[:, None] * cpg + np.arange(cpg)[None, :])[None, :, :, None, None, None], shape)
    return b, c


def _cols_view(col, B, C, dg, kk, Ho, Wo):
    """(C * kk, B, Ho, Wo) -> (B, dg, cpg, kk, Ho, Wo)"""
    return np.asarray(col, F64).reshape(dg, C // dg, kk, B, Ho, Wo).transpose(3, 0, 1, 2, 4, 5)


def _mask_view(mask, B, dg, kk, Ho, Wo):
    return 1.0 if mask is None else np.asarray(mask, F64).reshape(B, dg, 1, kk, Ho, Wo)


def mdcn_im2col(im, offset, mask, kh, kw, pad, stride, dil, dg):
    """im (B, C, H, W), offset (B, dg*2*kk, Ho, Wo), mask (B, dg*kk, Ho, Wo) or None -> col (C*kk, B, Ho, Wo), margins"""
    im = np.asarray(im, F64)
    B, C, H, W = im.shape
    kk, cpg = kh * kw, C // dg
    h, w, inside, m = _conv_geometry(offset, (H, W), kh, kw, pad, stride, dil, dg)
    Ho, Wo = h.shape[-2:]
    hl, wl, ok, ys, xs = _corners(h, w, H, W)
    lh, lw = h - hl, w - wl
    wts = ((1 - lh) * (1 - lw), (1 - lh) * lw, lh * (1 - lw), lh * lw)
    bi, ci = _idx(B, dg, cpg, kk, Ho, Wo)
    val = np.zeros((B, dg, cpg, kk, Ho, Wo))
    for k in range(4):
        val += _expand(wts[k], cpg) * _gather(im, bi, ci, _expand(ys[k], cpg), _expand(xs[k], cpg), _expand(ok[k], cpg), H, W)
    val = np.where(_expand(inside, cpg), val, 0.0) * _mask_view(mask, B, dg, kk, Ho, Wo)
    return val.transpose(1, 2, 3, 0, 4, 5).reshape(C * kk, B, Ho, Wo), m


def mdcn_col2im(col, offset, mask, im_shape, kh, kw, pad, stride, dil, dg):
    """-> grad_im (B, C, H, W), margins.  dmcn_get_gradient_weight gives floor / floor + 1 the bilinear weights and
    every other pixel of the 5 x 5 search zero; a corner outside the map receives nothing"""
    B, C, H, W = im_shape
    kk, cpg = kh * kw, C // dg
    h, w, inside, m = _conv_geometry(offset, (H, W), kh, kw, pad, stride, dil, dg)
    Ho, Wo = h.shape[-2:]
    hl, wl, ok, ys, xs = _corners(h, w, H, W)
    wts = ((hl + 1 - h) * (wl + 1 - w), (hl + 1 - h) * (w - wl), (h - hl) * (wl + 1 - w), (h - hl) * (w - wl))
    top = _cols_view(col, B, C, dg, kk, Ho, Wo) * _mask_view(mask, B, dg, kk, Ho, Wo)
    bi, ci = _idx(B, dg, cpg, kk, Ho, Wo)
    gim = np.zeros((B, C, H, W))
    for k in range(4):
        sel = _expand(ok[k] & inside, cpg)
        np.add.at(gim, (bi[sel], ci[sel], _expand(ys[k], cpg)[sel], _expand(xs[k], cpg)[sel]), (_expand(wts[k], cpg) * top)[sel])
    return gim, m


def mdcn_col2im_coord(col, im, offset, mask, kh, kw, pad, stride, dil, dg):
    """-> grad_offset (like offset), grad_mask (B, dg*kk, Ho, Wo; None without a mask), margins"""
    im = np.asarray(im, F64)
    B, C, H, W = im.shape
    kk, cpg = kh * kw, C // dg
    h, w, inside, m = _conv_geometry(offset, (H, W), kh, kw, pad, stride, dil, dg)
    Ho, Wo = h.shape[-2:]
    hl, wl, ok, ys, xs = _corners(h, w, H, W)
    bi, ci = _idx(B, dg, cpg, kk, Ho, Wo)
    v = [_gather(im, bi, ci, _expand(ys[k], cpg), _expand(xs[k], cpg), _expand(ok[k], cpg), H, W) for k in range(4)]
    E = lambda a: _expand(a, cpg)
    # dmcn_get_coordinate_weight, bp_dir 0 (d/dh) and 1 (d/dw): corners outside the map contribute nothing
    wh = -(E(wl + 1 - w)) * v[0] - E(w - wl) * v[1] + E(wl + 1 - w) * v[2] + E(w - wl) * v[3]
    ww = -(E(hl + 1 - h)) * v[0] + E(hl + 1 - h) * v[1] - E(h - hl) * v[2] + E(h - hl) * v[3]
    top = _cols_view(col, B, C, dg, kk, Ho, Wo)
    mk = _mask_view(mask, B, dg, kk, Ho, Wo)
    ins = E(inside)
    gh = np.where(ins, wh * top * mk, 0.0).sum(2)              # (B, dg, kk, Ho, Wo)
    gw = np.where(ins, ww * top * mk, 0.0).sum(2)
    goff = np.stack([gh, gw], 3).reshape(B, dg * 2 * kk, Ho, Wo)
    gmask = None
    if mask is not None:
        lh, lw = h - hl, w - wl
        bil = E((1 - lh) * (1 - lw)) * v[0] + E((1 - lh) * lw) * v[1] + E(lh * (1 - lw)) * v[2] + E(lh * lw) * v[3]
        gmask = np.where(ins, top * bil, 0.0).sum(2).reshape(B, dg * kk, Ho, Wo)
    return goff, gmask, m
