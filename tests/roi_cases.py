"""Conditioned RoI sets for the multi-level RoIAlign pins (tests/test_gpu_roi_align_levels.py; checked on the CPU by
tests/test_roi_cases_cpu.py).

The product and the reference's kernels are compared on EVERY element, so the inputs must stay clear of the two places
where a last-bit difference in a float32 intermediate legitimately changes the result by O(0.1):

* level ties -- the FPN level is floor(log2(scale / 56 + 1e-6)); the product takes it in float32 on the device, the test
  in float64.  A RoI whose log2 lies within TIE_EPS of an integer gets its width multiplied by 1.01 until it does not.
* validity lines -- the dialects drop a sample at x < -1, x > W, y < -1, y > H and clamp it onto the map otherwise: the
  pooled value jumps there.  The reference kernel rotates by the device's cosf, the product by the rounded
  double-precision cosine, so a sample within ~1e-5 px of a line can be valid in one and dropped in the other.  A RoI
  with a sample within LINE_EPS map pixels of a line has its centre moved by MOVE image pixels, until none is left.

No RoI is left out and no element is excluded from a comparison.  Everything here is float64 numpy on the float32 RoI
values the kernels read; the sampling grid of `sampling_ratio = 0` is taken as the kernels take it (ceilf of the float32
quotient, csrc/roi_geom.h)."""
import math

import numpy as np

from tests import inputs as I

FINEST_SCALE = 56
STRIDES = (4, 8, 16, 32)
TILE = 1024
OUT_HW = (7, 7)
TIE_EPS = 1e-4
LINE_EPS = 1e-4
MOVE = (0.37, 0.23)
MAX_ROUNDS = 3
MAX_MOVED_SHARE = 0.01
MAX_LEVER = 45.0
TRIG = ("rot", "rot_v1", "riroi")


def spread_obbs(rng, R, N):
    """(R, 6) float32 [batch, xc, yc, w, h, theta]: sizes log-uniform over 8..900 px so that all four levels of a
    1024-pixel tile are populated (about 50 / 14 / 14 / 20 % under the (1.2, 1.4) enlargement), aspect up to 5."""
    c = rng.uniform(0, TILE, size=(R, 2))
    s = np.exp(rng.uniform(math.log(8.0), math.log(900.0), size=R))
    a = np.exp(rng.uniform(-math.log(5.0), math.log(5.0), size=R))
    th = rng.uniform(-math.pi / 2, math.pi / 2, size=R)
    b = rng.integers(0, N, size=R)
    return np.stack([b, c[:, 0], c[:, 1], s * np.sqrt(a), s / np.sqrt(a), th], 1).astype(np.float32)


def enlarge(rois, factors):
    """(w * fw, h * fh) in float32, as the extractor (OrientedSingleRoIExtractor.roi_rescale) or its caller does"""
    r = rois.copy()
    r[:, 3] = r[:, 3] * np.float32(factors[0])
    r[:, 4] = r[:, 4] * np.float32(factors[1])
    return r


def obb_scale(rois6):
    r = rois6.astype(np.float64)
    return np.sqrt(r[:, 3] * r[:, 4])


def hbb_scale(rois5):
    r = rois5.astype(np.float64)
    return np.sqrt((r[:, 3] - r[:, 1] + 1) * (r[:, 4] - r[:, 2] + 1))


def level_log2(scale):
    return np.log2(scale / FINEST_SCALE + 1e-6)


def levels_of(scale, num_levels):
    """the reference's rule (single_level.py map_roi_levels), float64"""
    return np.clip(np.floor(level_log2(scale)), 0, num_levels - 1).astype(np.int64)


def fix_level_ties(rois6, scale_of):
    """widen (w *= 1.01) every RoI whose level logarithm lies within TIE_EPS of an integer; scale_of(rois6) -> float64
    scale of the RoI as the extractor sees it.  -> (rois, number of RoIs touched)"""
    rois = rois6.copy()
    touched = np.zeros(rois.shape[0], bool)
    for _ in range(64):
        t = level_log2(scale_of(rois))
        bad = np.abs(t - np.round(t)) < TIE_EPS
        if not bad.any():
            return rois, int(touched.sum())
        touched |= bad
        rois[bad, 3] = rois[bad, 3] * np.float32(1.01)
    raise AssertionError("level ties did not clear")


def kernel_grids(krois, scale, sampling, out_hw=OUT_HW):
    """sampling grid (gh, gw) per RoI as the kernels take it: float32 arithmetic of csrc/roi_geom.h"""
    R = krois.shape[0]
    if sampling > 0:
        return np.full(R, sampling, np.int64), np.full(R, sampling, np.int64)
    sc = np.asarray(scale, np.float32)
    w = np.maximum(krois[:, 3] * sc, np.float32(1.0))
    h = np.maximum(krois[:, 4] * sc, np.float32(1.0))
    assert w.dtype == np.float32 and h.dtype == np.float32
    gh = np.ceil(h / np.float32(out_hw[0])).astype(np.int64)
    gw = np.ceil(w / np.float32(out_hw[1])).astype(np.int64)
    return gh, gw


def line_distance(krois, lvl, dialect, sampling, strides=STRIDES, tile=TILE, out_hw=OUT_HW):
    """-> (distance of each RoI's nearest sample to a validity line of its level's map [map pixels, float64],
    half-diagonal of each RoI in map pixels, largest sampling grid)"""
    assert dialect in TRIG
    PH, PW = out_hw
    r = krois.astype(np.float64)
    stride = np.asarray(strides, np.float64)[lvl]
    scale = 1.0 / stride
    size = tile / stride                                  # H = W of the RoI's own level
    gh, gw = kernel_grids(krois, (1.0 / np.asarray(strides, np.float64))[lvl].astype(np.float32), sampling, out_hw)
    off = 0.5 if dialect == "rot_v1" else 0.0
    cx, cy = r[:, 1] * scale - off, r[:, 2] * scale - off
    w, h = np.maximum(r[:, 3] * scale, 1.0), np.maximum(r[:, 4] * scale, 1.0)
    cos, sin = np.cos(r[:, 5]), np.sin(r[:, 5])
    dist = np.full(r.shape[0], np.inf)
    for g_h, g_w in sorted(set(zip(gh.tolist(), gw.tolist()))):
        m = (gh == g_h) & (gw == g_w)
        fy = (np.arange(PH)[:, None] + (np.arange(g_h)[None, :] + 0.5) / g_h).reshape(-1)      # bin + in-bin fraction
        fx = (np.arange(PW)[:, None] + (np.arange(g_w)[None, :] + 0.5) / g_w).reshape(-1)
        yy = (-h[m] / 2)[:, None] + fy[None, :] * (h[m] / PH)[:, None]                          # (r, PH * gh)
        xx = (-w[m] / 2)[:, None] + fx[None, :] * (w[m] / PW)[:, None]                          # (r, PW * gw)
        c, s = cos[m][:, None, None], sin[m][:, None, None]
        X, Y = xx[:, None, :], yy[:, :, None]
        if dialect == "rot_v1":
            x, y = X * c + Y * s, Y * c - X * s
        else:
            x, y = X * c - Y * s, X * s + Y * c
        x, y = x + cx[m][:, None, None], y + cy[m][:, None, None]
        S = size[m][:, None, None]
        d = np.minimum(np.minimum(np.abs(x + 1), np.abs(x - S)), np.minimum(np.abs(y + 1), np.abs(y - S)))
        dist[m] = d.reshape(d.shape[0], -1).min(1)
    lever = 0.5 * np.sqrt(w * w + h * h)
    return dist, lever, int(max(gh.max(), gw.max()))


def keep_off_validity_lines(rois, lvl, dialect, sampling, factors=(1.0, 1.0), strides=STRIDES, tile=TILE, out_hw=OUT_HW):
    """Move the centre of every RoI that has a sample within LINE_EPS map pixels of a validity line of its level by
    MOVE image pixels, until none is left.  `rois` are the RoIs handed to the product, `factors` the (w, h) enlargement
    between them and what the kernel reads.  -> (rois, dict(moved, rounds, lever, grid)); asserts its own conditions."""
    rois = rois.copy()
    moved = np.zeros(rois.shape[0], bool)
    rounds = 0
    while True:
        dist, lever, grid = line_distance(enlarge(rois, factors), lvl, dialect, sampling, strides, tile, out_hw)
        near = dist < LINE_EPS
        if not near.any():
            break
        rounds += 1
        assert rounds <= MAX_ROUNDS, "validity-line conditioning did not settle in %d rounds" % MAX_ROUNDS
        moved |= near
        rois[near, 1] = rois[near, 1] + np.float32(MOVE[0])
        rois[near, 2] = rois[near, 2] + np.float32(MOVE[1])
    assert moved.mean() <= MAX_MOVED_SHARE, "%d of %d RoIs moved" % (moved.sum(), moved.size)
    return rois, dict(moved=int(moved.sum()), rounds=rounds, lever=float(lever.max()), grid=grid,
                      min_dist=float(dist.min()))


# ---- the committed cases ------------------------------------------------------------------------------------------------
# id -> dialect, images, RoIs, seed, generator, (w, h) enlargement and who applies it ("extractor" | "caller" | None)
MULTI = {
    "orcnn-train": dict(dialect="rot_v1", N=2, R=1024, seed=0, gen="spread", factors=(1.2, 1.4), by="extractor"),
    "orcnn-infer": dict(dialect="rot_v1", N=2, R=4000, seed=1, gen="spread", factors=(1.2, 1.4), by="extractor"),
    "roitrans-hbb": dict(dialect="hbb1", N=4, R=2048, seed=2, gen="spread", factors=(1.0, 1.0), by=None),
    "roitrans-rot": dict(dialect="rot", N=4, R=2048, seed=2, gen="spread", factors=(1.2, 1.4), by="caller"),
    "riroi": dict(dialect="riroi", N=2, R=1024, seed=3, gen="spread", factors=(1.2, 1.4), by="caller"),
    "empty-level": dict(dialect="rot_v1", N=2, R=1024, seed=4, gen="random", factors=(1.2, 1.4), by="extractor"),
}
SECOND_STEP_SEED = 100      # the plan-off path's second step: the same case with seed + SECOND_STEP_SEED


def multi_case(name, seed_offset=0):
    """-> dict(rois: what the extractor is given, krois: what the kernel of the RoI's level reads, lvl, info)"""
    c = MULTI[name]
    rng = np.random.default_rng(c["seed"] + seed_offset)
    if c["gen"] == "spread":
        base = spread_obbs(rng, c["R"], c["N"])
    else:
        base = I.rois_from_obbs(I.random_obbs(rng, c["R"]), rng.integers(0, c["N"], c["R"]))
    n_lvl = len(STRIDES)
    if c["dialect"] in ("hbb0", "hbb1"):
        base, ties = fix_level_ties(base, lambda r: hbb_scale(I.obb_to_hbb_rois(r)))
        rois = I.obb_to_hbb_rois(base)
        lvl = levels_of(hbb_scale(rois), n_lvl)
        info = dict(moved=0, rounds=0, lever=0.0, grid=2, min_dist=float("inf"))
        krois = rois
    else:
        base, ties = fix_level_ties(base, lambda r: obb_scale(enlarge(r, c["factors"])))
        given = enlarge(base, c["factors"]) if c["by"] == "caller" else base
        between = c["factors"] if c["by"] == "extractor" else (1.0, 1.0)
        lvl = levels_of(obb_scale(enlarge(given, between)), n_lvl)
        rois, info = keep_off_validity_lines(given, lvl, c["dialect"], 2, between)
        krois = enlarge(rois, between)
        assert info["lever"] <= MAX_LEVER, info
    info["ties"] = ties
    info["per_level"] = np.bincount(lvl, minlength=n_lvl).tolist()
    return dict(rois=rois, krois=krois, lvl=lvl, info=info, **c)


def single_case(dialect, R, sampling, seed):
    """one 1 x C x 256 x 256 map at stride 4, I.random_obbs sizes (what the existing full-size pin of `rot` uses)"""
    rng = np.random.default_rng(seed)
    rois = I.rois_from_obbs(I.random_obbs(rng, R), np.zeros(R))
    lvl = np.zeros(R, np.int64)
    if dialect in ("hbb0", "hbb1"):
        h = I.obb_to_hbb_rois(rois)
        sc = np.float32(0.25)
        ext = np.maximum(np.stack([h[:, 3] * sc - h[:, 1] * sc, h[:, 4] * sc - h[:, 2] * sc]), np.float32(1.0))
        grid = int(np.ceil(ext / np.float32(OUT_HW[0])).max()) if sampling <= 0 else sampling
        return dict(rois=h, info=dict(moved=0, rounds=0, lever=0.0, min_dist=float("inf"), grid=grid))
    rois, info = keep_off_validity_lines(rois, lvl, dialect, sampling, strides=(4,))
    assert info["lever"] <= MAX_LEVER, info
    return dict(rois=rois, info=info)
