"""Case table of the sorted-gather regime tests (csrc/csr_gather.h and its three clients: RoIAlign backward,
channels-last deformable col2im, feature-refine backward).  No kernel calls; importable without a GPU.

EXACT tier: every bilinear weight and every gradient value of a fixture is a small dyadic rational, so every partial
sum -- in any order -- is a multiple of 1/unit below 2^24 / unit and therefore exact in fp32: the device result has to
EQUAL the oracle's.  tests/test_gather_cases_cpu.py proves both conditions from the oracles alone.
TOLERANCE tier: what cannot be dyadic (9 samples per bin, hbb1 extents, non-zero angles), random inputs, short rows.

cap_of / tile_count / patch_grid / row-length helpers restate the host-side choices of the kernels; they LABEL the
regime a case is in (and let the CPU test prove the table reaches every regime) and never produce expected values.
"""
import functools
from types import SimpleNamespace as NS

import numpy as np

from oracle import fr_oracle as FO
from oracle import oracle as O
from tests import closed_form as CF

F = np.float32
SCAN_TILE = 2048


# ------------------------------------------------------------------------------------------- regime labels
def tile_count(nkeys):
    return -(-nkeys // SCAN_TILE)


def cap_of(nkeys, max_recs):
    """patch_direct_cap: power of two >= 2.5 x the expected row length in 32..256, halved while the direct rows
    (32-byte entries) would pass 256 MiB; below 16 -> 0"""
    expect = 0.5 * float(max_recs) / float(max(nkeys, 1))
    cap = 32
    while cap < 256 and float(cap) < 2.5 * expect:
        cap *= 2
    while cap >= 16 and nkeys * cap * 32 > (256 << 20):
        cap //= 2
    return cap if cap >= 16 else 0


def patch_grid(N, H, W):
    """work mapping of the patch-keyed gather: patches per image, workgroups per patch row, XCD block size"""
    php, pwp = (H + 1) // 2, (W + 1) // 2
    bw = (pwp + 1) // 2
    gr = (N * php + 1) // 2
    nbc = 2 if bw >= 2 else 1
    nbr = 8 // nbc
    return NS(php=php, pwp=pwp, bw=bw, nkeys=N * php * pwp, BR=-(-gr // nbr), BC=-(-bw // nbc))


def pixel_grid(B, H, W):
    """work mapping of the pixel-keyed gather: stripes of 8 stacked pixel rows, round-robin over 8 XCDs"""
    n_rows = B * H
    stripes = -(-n_rows // 8)
    return NS(n_rows=n_rows, stripes=stripes, laps=-(-stripes // 8), nkeys=B * H * W)


# ------------------------------------------------------------------------------------------- tap rules (numpy)
def bilinear_taps(h, w, H, W):
    """deformable rule (dcn_v1.py get_gradient_weight): the sample counts only inside the open interval
    -1 < h < H, -1 < w < W; four corners; corners off the map and zero-weight corners are dropped.
    -> ys, xs (int), ws (float64), keep (bool), each (4,) + h.shape"""
    h, w = np.asarray(h, np.float64), np.asarray(w, np.float64)
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    hl, wl = np.floor(h).astype(np.int64), np.floor(w).astype(np.int64)
    ys = np.stack([hl, hl, hl + 1, hl + 1])
    xs = np.stack([wl, wl + 1, wl, wl + 1])
    ws = np.stack([(hl + 1 - h) * (wl + 1 - w), (hl + 1 - h) * (w - wl), (h - hl) * (wl + 1 - w), (h - hl) * (w - wl)])
    keep = inside[None] & (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W) & (ws != 0)
    return ys, xs, ws, keep


def dcn_row_lengths(off, B, H, W, k, pad):
    """entries per pixel of the deformable col2im gather (stride 1, dilation 1), (B*H*W,)"""
    Ho, Wo = off.shape[2:]
    ho, wo = np.mgrid[0:Ho, 0:Wo]
    cnt = np.zeros(B * H * W, np.int64)
    for b in range(B):
        for t in range(k * k):
            ys, xs, _, keep = bilinear_taps(ho - pad + t // k + off[b, 2 * t], wo - pad + t % k + off[b, 2 * t + 1], H, W)
            cnt += np.bincount(((b * H + ys) * W + xs)[keep], minlength=B * H * W)
    return cnt


def fr_row_lengths(boxes, scale, points):
    """entries per pixel of the feature-refine gather: the kept corner taps + the identity tap, (N*H*W,)"""
    N, H, W = boxes.shape[:3]
    py, px = FO.sample_points(boxes, scale, points)
    cnt = np.ones(N * H * W, np.int64)
    base = (np.arange(N) * H)[:, None, None]
    for i in range(points):
        yl, xl, yh, xh, ws, valid = FO._taps(py[i].copy(), px[i].copy(), H, W)
        for yy, xx, w in ((yl, xl, ws[0]), (yl, xh, ws[1]), (yh, xl, ws[2]), (yh, xh, ws[3])):
            keep = valid & (w != 0)
            cnt += np.bincount(((base + yy) * W + xx)[keep], minlength=N * H * W)
    return cnt


def patch_row_lengths(variant, rois, N, H, W, PH, PW, s, scale=1.0):
    """entries per 2x2 patch of the RoIAlign backward: the taps of one (RoI, bin) that fall into one patch are one
    entry when the bin's samples are merged (4 samples per bin), one entry per (RoI, bin, sample) otherwise.
    Sample grid of tests/closed_form.py, clamping rule of the RoI kernels (= fr_oracle._taps).  (N*php*pwp,)"""
    g = patch_grid(N, H, W)
    cnt = np.zeros(g.nkeys, np.int64)
    for r in range(rois.shape[0]):
        b = int(rois[r, 0])
        if b < 0:
            continue
        X, Y, _ = CF.sample_positions(variant, rois[r], scale, PH, PW, s)
        yl, xl, yh, xh, ws, valid = FO._taps(Y.astype(F), X.astype(F), H, W)
        row = np.broadcast_to(np.arange(PH * PW * s * s).reshape(PH, PW, s, s), X.shape)
        if s == 2:
            row = row // 4
        pairs = []
        for yy, xx, w in ((yl, xl, ws[0]), (yl, xh, ws[1]), (yh, xl, ws[2]), (yh, xh, ws[3])):
            keep = valid & (w != 0)
            pairs.append(np.stack([row[keep], ((b * g.php + (yy >> 1)) * g.pwp + (xx >> 1))[keep]], 1))
        pairs = np.unique(np.concatenate(pairs), axis=0)
        cnt += np.bincount(pairs[:, 1], minlength=g.nkeys)
    return cnt


# ------------------------------------------------------------------------------------------- pixel-keyed cases
def _pix(name, client, shape, C=4, *, k=3, points=1, mode="dyadic", claims=None, large=False):
    B, H, W = shape
    return NS(name=name, client=client, B=B, H=H, W=W, C=C, k=k, pad=(k - 1) // 2, points=points, mode=mode,
              claims=claims or {}, large=large, tier="tol" if mode == "generic" else "exact")


_GEOMETRY = [((1, 1, 1), {}), ((1, 1, 2), {}), ((1, 2, 1), {}), ((1, 1, 67), {"odd_w": True}),
             ((1, 67, 1), {"stripes": 9, "laps": 2}), ((3, 5, 7), {"odd_w": True, "straddles_images": True}),
             ((1, 16, 16), {"stripes": 2}), ((2, 33, 9), {"n_rows": 66, "stripes": 9, "laps": 2}),
             ((1, 9, 130), {"stripes": 2}), ((1, 48, 48), {"tiles": 2})]

PIXEL_CASES = []
for _shape, _claims in _GEOMETRY:
    _tag = "x".join(map(str, _shape))
    PIXEL_CASES.append(_pix("dcn-" + _tag, "dcn", _shape, claims=_claims))
    PIXEL_CASES.append(_pix("fr1-" + _tag, "fr", _shape, points=1, claims=_claims))
    PIXEL_CASES.append(_pix("fr5-" + _tag, "fr", _shape, points=5, claims=_claims))
for _C in (4, 252, 260, 512):
    PIXEL_CASES.append(_pix("dcn-chunks-C%d" % _C, "dcn", (1, 9, 11), _C, claims={"chunks": -(-_C // 256)}))
    PIXEL_CASES.append(_pix("fr5-chunks-C%d" % _C, "fr", (1, 9, 11), _C, points=5, claims={"chunks": -(-_C // 256)}))
PIXEL_CASES += [
    _pix("dcn-converged", "dcn", (1, 12, 12), mode="converged", claims={"max_row": 1296, "empty_rows": 140}),
    _pix("dcn-all-dropped", "dcn", (1, 12, 12), mode="dropped", claims={"max_row": 0, "empty_rows": 144}),
    _pix("dcn-257-tiles", "dcn", (1, 725, 725), k=1, claims={"tiles": 257}, large=True),
    _pix("fr1-257-tiles", "fr", (1, 725, 725), points=1, claims={"tiles": 257}, large=True),
    # tolerance tier: boxes at non-zero angles (cosf / sinf), generic sizes, normal gradients
    _pix("fr5-generic-3x5x7", "fr", (3, 5, 7), points=5, mode="generic"),
    _pix("fr5-generic-2x33x9", "fr", (2, 33, 9), points=5, mode="generic"),
]
CONVERGED_POINT = (5.25, 6.75)     # a quarter-pixel point: its four corner weights are 9/16, 3/16, 3/16 and 1/16


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 32)


@functools.lru_cache(maxsize=None)
def pixel_inputs(name):
    """-> NS(case, off | boxes, grad (oracle layout), unit).  Gradients are integers; long rows get {-2..2}."""
    c = {x.name: x for x in PIXEL_CASES}[name]
    rng = np.random.default_rng(_seed(name))
    B, H, W, C = c.B, c.H, c.W, c.C
    if c.client == "dcn":
        kk = c.k * c.k
        Ho, Wo = O._dcn_out(H, W, c.k, c.k, (c.pad, c.pad), (1, 1), (1, 1))
        if c.mode == "converged":
            ho, wo = np.mgrid[0:Ho, 0:Wo]
            off = np.zeros((B, 2 * kk, Ho, Wo), F)
            for t in range(kk):
                off[:, 2 * t] = CONVERGED_POINT[0] - (ho - c.pad + t // c.k)
                off[:, 2 * t + 1] = CONVERGED_POINT[1] - (wo - c.pad + t % c.k)
        elif c.mode == "dropped":
            off = np.full((B, 2 * kk, Ho, Wo), 1000.0, F)
        else:
            off = (rng.integers(-12, 13, size=(B, 2 * kk, Ho, Wo)) / 4.0).astype(F)      # multiples of 0.25
        lim = 2 if c.mode == "converged" else 3
        grad = rng.integers(-lim, lim + 1, size=(C * kk, B, Ho, Wo)).astype(F)
        return NS(case=c, off=off, grad=grad, unit=16.0)
    ys, xs = np.mgrid[0:H, 0:W]
    if c.mode == "generic":
        boxes = np.stack([ys * 8 + rng.normal(0, 16.0, (B, H, W)), xs * 8 + rng.normal(0, 16.0, (B, H, W)),
                          np.exp(rng.normal(np.log(32.0), 0.6, (B, H, W))), np.exp(rng.normal(np.log(32.0), 0.6, (B, H, W))),
                          rng.uniform(-1.6, 1.6, (B, H, W))], -1).astype(F)
        return NS(case=c, boxes=boxes, grad=rng.standard_normal((B, C, H, W)).astype(F), unit=None)
    boxes = np.zeros((B, H, W, 5), F)
    boxes[..., 0] = ys * 8 + 2 * rng.integers(-12, 13, size=(B, H, W))       # even integers: x 0.125 -> quarters
    boxes[..., 1] = xs * 8 + 2 * rng.integers(-12, 13, size=(B, H, W))
    boxes[..., 2:4] = 4 * rng.integers(1, 9, size=(B, H, W, 2))             # multiples of 4: half extents in quarters
    far = rng.random((B, H, W)) < 0.05
    boxes[far, 0] = -1000.0                                                # every sample of the location dropped
    grad = rng.integers(-3, 4, size=(B, C, H, W)).astype(F)
    return NS(case=c, boxes=boxes, grad=grad, unit=16.0)


def pixel_reference(inp, grad=None):
    """(B, C, H, W) result of the CPU oracle (float32 for deformable col2im, float64-accumulated for feature refine)"""
    c = inp.case
    g = inp.grad if grad is None else grad
    if c.client == "dcn":
        return O.deform_col2im(g, inp.off, (c.B, c.C, c.H, c.W), c.k, c.k, (c.pad, c.pad), (1, 1), (1, 1), 1)
    return FO.feature_refine_backward(g, inp.boxes, 0.125, c.points)


def pixel_row_lengths(inp):
    c = inp.case
    if c.client == "dcn":
        return dcn_row_lengths(inp.off, c.B, c.H, c.W, c.k, c.pad)
    return fr_row_lengths(inp.boxes, 0.125, c.points)


def pixel_regime(inp):
    c = inp.case
    g = pixel_grid(c.B, c.H, c.W)
    rows = pixel_row_lengths(inp)
    return {"tiles": tile_count(g.nkeys), "n_rows": g.n_rows, "stripes": g.stripes, "laps": g.laps,
            "odd_w": c.W % 2 == 1, "straddles_images": c.B > 1 and c.H % 2 == 1, "chunks": -(-c.C // 256),
            "max_row": int(rows.max()), "empty_rows": int((rows == 0).sum())}


# ------------------------------------------------------------------------------------------- patch-keyed cases
V_NAMES = {O.V_ROT: "rot", O.V_ROT_V1: "rot_v1", O.V_HBB0: "hbb0", O.V_HBB1: "hbb1"}
UNIT = {1: 2.0 ** 2, 2: 2.0 ** 6, 4: 2.0 ** 10}     # 1 / (weight granularity x samples per bin), bin size >= 1 pixel


def dyadic_rois(rng, R, N, H, W, PH, PW, variant, overhang=True):
    """RoIs at spatial_scale 1, angle 0: integer corners (so odd sizes have half-integer centres), width PW*k, height
    PH*k, k in {1, 2}.  overhang: corners up to a full RoI size off the map (clamped and dropped samples)."""
    out = np.zeros((R, 5 if variant in (O.V_HBB0, O.V_HBB1) else 6), F)
    for r in range(R):
        k = int(rng.integers(1, 3))
        w, h = PW * k, PH * k
        if overhang:
            x1, y1 = int(rng.integers(-w, W + 1)), int(rng.integers(-h, H + 1))
        else:
            x1, y1 = int(rng.integers(0, max(W - w, 0) + 1)), int(rng.integers(0, max(H - h, 0) + 1))
        out[r, 0] = int(rng.integers(0, N))
        out[r, 1:5] = (x1, y1, x1 + w, y1 + h) if out.shape[1] == 5 else (x1 + w / 2.0, y1 + h / 2.0, w, h)
    return out


def point_rois(R, x, y, PH, PW, variant):
    """R identical 1x1-pixel RoIs with corner (x, y): every bin of every one of them lands in the patch of pixel (x, y)
    (bins of 1/PH x 1/PW pixel: dyadic for power-of-two bin grids only)"""
    row = [0, x, y, x + 1, y + 1] if variant in (O.V_HBB0, O.V_HBB1) else [0, x + 0.5, y + 0.5, 1, 1, 0]
    return np.tile(np.array([row], F), (R, 1))


def random_rois(rng, R, N, H, W, variant):
    """tolerance tier: generic sizes, angles spread over (-2 pi, 2 pi), centres up to 3 pixels off the map"""
    xc, yc = rng.uniform(-3, W + 3, R), rng.uniform(-3, H + 3, R)
    w, h = rng.uniform(0.5, 0.8 * W, R), rng.uniform(0.5, 0.8 * H, R)
    b = rng.integers(0, N, R)
    if variant in (O.V_HBB0, O.V_HBB1):
        return np.stack([b, xc - w / 2, yc - h / 2, xc + w / 2, yc + h / 2], 1).astype(F)
    return np.stack([b, xc, yc, w, h, np.linspace(-6.2, 6.2, R)], 1).astype(F)


ROUTES = ("nchw", "cl", "planned")


def _roi(name, variant, shape, bins, *, R=30, C=4, kind="dyadic", tier="exact", routes=ROUTES, claims=None,
         large=False, lim=3):
    N, H, W = shape
    PH, PW, s = bins
    return NS(name=name, variant=variant, N=N, H=H, W=W, C=C, PH=PH, PW=PW, s=s, R=R, kind=kind, tier=tier,
              routes=routes, claims=claims or {}, large=large, lim=lim)


ROI_CASES = []
_PATCH_GEOMETRY = [((1, 1, 1), {"bw": 1}), ((1, 1, 2), {"bw": 1}), ((1, 2, 1), {"bw": 1}), ((1, 3, 4), {"bw": 1}),
                   ((1, 4, 5), {"bw": 2}), ((1, 1, 70), {"BC": 9}), ((1, 70, 1), {"bw": 1, "BR": 3}),
                   ((3, 5, 7), {"php": 3, "straddles_images": True}), ((1, 140, 6), {"BR": 9}), ((1, 6, 140), {"BC": 18})]
for _shape, _claims in _PATCH_GEOMETRY:
    for _v in (O.V_ROT, O.V_ROT_V1, O.V_HBB0):
        ROI_CASES.append(_roi("geo-%s-%s" % ("x".join(map(str, _shape)), V_NAMES[_v]), _v, _shape, (7, 7, 2),
                              claims=_claims))

# producer: bin grids and samplings on a (2, 20, 24) map; every third RoI masked, one RoI entirely off the map
_PRODUCER = [((7, 7, 2), {"S": 196, "spb": 4}), ((14, 14, 2), {"S": 784, "spb": 4, "rounds": 4, "partial_round": True}),
             ((7, 7, 1), {"S": 49, "spb": 1}), ((3, 5, 4), {"S": 240, "spb": 16}), ((1, 1, 2), {"S": 4, "spb": 4}),
             ((16, 16, 1), {"S": 256, "spb": 1, "rounds": 1})]
for _bins, _claims in _PRODUCER:
    for _v in (O.V_ROT, O.V_HBB0):
        ROI_CASES.append(_roi("prod-%dx%dx%d-%s" % (_bins + (V_NAMES[_v],)), _v, (2, 20, 24), _bins, R=24,
                              kind="dyadic+masked+off", claims=_claims))
ROI_CASES.append(_roi("prod-7x7x3-rot", O.V_ROT, (2, 20, 24), (7, 7, 3), R=24, kind="dyadic+masked+off", tier="tol",
                      claims={"S": 441, "spb": 9, "rounds": 2, "partial_round": True}))
for _bins in ((7, 7, 2), (14, 14, 2)):
    for _v in (O.V_HBB1, O.V_ROT, O.V_ROT_V1):
        ROI_CASES.append(_roi("prod-%dx%dx%d-%s-generic" % (_bins + (V_NAMES[_v],)), _v, (2, 20, 24), _bins, R=24,
                              kind="random+masked+off", tier="tol"))
ROI_CASES += [
    _roi("prod-R1", O.V_ROT, (2, 20, 24), (7, 7, 2), R=1, kind="dyadic"),
    _roi("prod-all-masked", O.V_ROT, (2, 20, 24), (7, 7, 2), R=9, kind="dyadic+allmasked", claims={"entries": 0}),
]

# direct-row caps on a (1, 20, 24) map (120 patches), 8x8 bins at sampling 2: a 1x1-pixel RoI has bins of 1/8 pixel
# (weights in 1/1024 x 1/4: dyadic) and puts all of its 64 (RoI, bin) rows into ONE patch
CAP_BINS = (8, 8, 2)
UNIT_POINT = 2.0 ** 12
for _cap, _R in ((32, 3), (64, 5), (128, 10), (256, 16)):
    ROI_CASES.append(_roi("cap%d-overflow" % _cap, O.V_ROT, (1, 20, 24), CAP_BINS, R=_R, kind="clustered", lim=2,
                          claims={"cap": _cap, "overflow": True}))
    ROI_CASES.append(_roi("cap%d-direct" % _cap, O.V_ROT, (1, 20, 24), CAP_BINS, R=_R, kind="spread", lim=2,
                          claims={"cap": _cap, "overflow": False}))
# two scan tiles of patches with rows past the cap in BOTH (a row's place = tile-local offset + tile base)
ROI_CASES.append(_roi("cap32-2-tiles-overflow", O.V_ROT, (1, 100, 100), CAP_BINS, R=12, kind="clustered2", lim=2,
                      claims={"cap": 32, "tiles": 2, "overflow": True, "overflow_tiles": [0, 1]}))
ROI_CASES.append(_roi("cap0-257-tiles", O.V_ROT, (1, 1450, 1450), (7, 7, 2), R=64, kind="dyadic-inside+clustered",
                      claims={"cap": 0, "tiles": 257, "overflow": True}, routes=("cl", "planned"), large=True))


@functools.lru_cache(maxsize=None)
def roi_inputs(name):
    """-> NS(case, rois (masked rows have batch -1), grad (R, C, PH, PW) integers, unit)"""
    c = {x.name: x for x in ROI_CASES}[name]
    rng = np.random.default_rng(_seed(name))
    N, H, W, PH, PW, R = c.N, c.H, c.W, c.PH, c.PW, c.R
    unit = UNIT.get(c.s)
    if c.kind.startswith("random"):
        rois = random_rois(rng, R, N, H, W, c.variant)
    elif c.kind == "clustered":          # two thirds of the RoIs (at least two) on one pixel, the rest spread over the map
        n = max(2, R - R // 3)
        rois = np.concatenate([point_rois(n, 6, 10, PH, PW, c.variant),
                               dyadic_rois(rng, R - n, N, H, W, PH, PW, c.variant, overhang=False)])
        unit = UNIT_POINT
    elif c.kind == "clustered2":         # one cluster in the first scan tile of patches, one in the second
        rois = np.concatenate([point_rois(4, 6, 10, PH, PW, c.variant), point_rois(5, 90, 96, PH, PW, c.variant),
                               dyadic_rois(rng, R - 9, N, H, W, PH, PW, c.variant, overhang=False)])
        unit = UNIT_POINT
    elif c.kind == "spread":
        rois = dyadic_rois(rng, R, N, H, W, PH, PW, c.variant, overhang=False)
    elif c.kind == "dyadic-inside+clustered":      # cap 0: a cluster of identical RoIs makes rows of dozens of entries
        rois = dyadic_rois(rng, R, N, H, W, PH, PW, c.variant, overhang=False)
        rois[:24] = rois[0]
        rois[24:32, 1:3] = (W - 3.5, H - 3.5)       # the last patch row / column of the map, overhanging
    else:
        rois = dyadic_rois(rng, R, N, H, W, PH, PW, c.variant)
    if "+masked" in c.kind:
        rois[2::3, 0] = -1
    if "+off" in c.kind:
        rois[1, 1:3] = (-40.0, -40.0) if rois.shape[1] == 6 else (-60.0, -60.0)
        if rois.shape[1] == 5:
            rois[1, 3:5] = (-46.0, -46.0)
    if "+allmasked" in c.kind:
        rois[:, 0] = -1
    grad = rng.integers(-c.lim, c.lim + 1, size=(R, c.C, PH, PW)).astype(F)
    return NS(case=c, rois=rois.astype(F), grad=grad, unit=unit)


def roi_reference(inp, grad=None):
    """(N, C, H, W) float32 result of the CPU oracle over the live RoIs"""
    c = inp.case
    g = inp.grad if grad is None else grad
    live = inp.rois[:, 0] >= 0
    if not live.any():
        return np.zeros((c.N, g.shape[1], c.H, c.W), F)
    return O.roi_align_backward(c.variant, g[live], inp.rois[live], (c.N, g.shape[1], c.H, c.W), 1.0, c.s)


def roi_regime(inp):
    c = inp.case
    g = patch_grid(c.N, c.H, c.W)
    S = c.PH * c.PW * c.s * c.s
    cap = cap_of(g.nkeys, c.R * S * 4)
    out = {"cap": cap, "tiles": tile_count(g.nkeys), "bw": g.bw, "BR": g.BR, "BC": g.BC, "php": g.php,
           "straddles_images": c.N > 1 and g.php % 2 == 1, "S": S, "spb": c.s * c.s, "rounds": -(-S // 256),
           "partial_round": S > 256 and S % 256 != 0}
    if c.tier == "exact":            # row lengths restate exact geometry only
        rows = patch_row_lengths(c.variant, inp.rois, c.N, c.H, c.W, c.PH, c.PW, c.s)
        out.update(overflow=bool((rows > cap).any()), entries=int(rows.sum()), max_row=int(rows.max()),
                   overflow_tiles=sorted({int(k) // SCAN_TILE for k in np.nonzero(rows > cap)[0]}))
    return out


# the kept-workspace chain on the map whose workgroups straddle images: overflow, none, overflow again
CHAIN_SHAPE = (3, 5, 7)
CHAIN_BINS = CAP_BINS
CHAIN_R = (12, 6, 12)


@functools.lru_cache(maxsize=None)
def chain_inputs(step):
    N, H, W = CHAIN_SHAPE
    R = CHAIN_R[step]
    rng = np.random.default_rng(900 + step)
    if step == 1:
        rois = dyadic_rois(rng, R, N, H, W, 8, 8, O.V_ROT, overhang=False)
    else:
        rois = np.concatenate([point_rois(R - 4, 2 + step, 3, 8, 8, O.V_ROT), dyadic_rois(rng, 4, N, H, W, 8, 8, O.V_ROT)])
        rois[:R - 4, 0] = 1
    grad = rng.integers(-2, 3, size=(R, 4, 8, 8)).astype(F)
    c = NS(name="chain%d" % step, variant=O.V_ROT, N=N, H=H, W=W, C=4, PH=8, PW=8, s=2, R=R, tier="exact", claims={})
    return NS(case=c, rois=rois.astype(F), grad=grad, unit=UNIT_POINT)
