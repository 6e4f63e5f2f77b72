"""Case table of the DCN v2 regime tests: csrc/deform_psroi_pool.hip and the modulated entry points of
csrc/deform_nchw.hip (plus the border fixture the channels-last deformable routes share).  No kernel calls; importable
without a GPU.  Expected values come from tests/dcn_v2_ref.py (float64, written from the reference text).

EXACT tier: every quantity is a small dyadic rational -- spatial_scale 1 or 0.25, integer RoI corners, P in {2, 4},
1 or 2 samples per bin (counts 0, 1, 2, 4), trans in eighths with trans_std 0.25, offsets in quarters, masks in
eighths, integer features / images / gradients in [-8, 8] -- so every product and every partial sum, in any order, is
exact in fp32 and the device has to EQUAL the rounded float64 reference.  tests/test_dcn_v2_cases_cpu.py proves it from
the fp32 oracle (bit-equal to the reference) and from the sums of absolute terms (below 2^24 units).
TOLERANCE tier: what cannot be dyadic (P = 3, 6, 7; 3 or 4 samples per bin; the 0.1 width clamp; general offsets).
Rows are drawn and FILTERED here: a RoI / an offset is redrawn until every decision (skip, clamp, floor, inside)
clears its threshold by MARGIN pixels in float64 and the fp32 oracle counts the same samples; the tests drop nothing.

vec_of / chunks_of / waves_of / laps_of / x_blocks_of restate the host-side choices of the kernels.  They LABEL the
regime a case is in and never produce expected values."""
import functools
from types import SimpleNamespace as NS

import numpy as np

from oracle import oracle as O
from tests import dcn_v2_ref as RF

F = np.float32
MARGIN = 1e-4
WAVE_CAP = 65536 * 4                  # deform_psroi_pool.hip: 65536 workgroups of four waves


# ------------------------------------------------------------------------------------------- regime labels
def vec_of(G, cec, C):
    return 4 if (G == 1 and cec % 4 == 0 and C % 4 == 0) else 1


def chunks_of(cec, vec):
    return -(-cec // (64 * vec))


def waves_of(R, P, ncls, chunks):
    return R * P * P * ncls * chunks


def laps_of(waves):
    return -(-waves // WAVE_CAP)


def x_blocks_of(Wo):
    """(blocks along wo, lanes of the last one that own a column)"""
    return -(-Wo // 64), (Wo - 1) % 64 + 1


def pool_labels(c, no_trans):
    ncls = 1 if no_trans else c.ncls
    cec = c.od // ncls
    C = c.od * c.G * c.G
    vec = vec_of(c.G, cec, C)
    chunks = chunks_of(cec, vec)
    tail = -(-(cec - (chunks - 1) * 64 * vec) // vec)          # lanes of the last chunk that own channels
    waves = waves_of(c.R, c.P, ncls, chunks)
    return NS(ncls=ncls, cec=cec, C=C, vec=vec, chunks=chunks, tail_lanes=tail, waves=waves, laps=laps_of(waves),
              group=c.G, identity_parts=c.part == c.P)


def conv_labels(c):
    Ho, Wo = conv_out_hw(c)
    blocks, tail = x_blocks_of(Wo)
    return NS(Ho=Ho, Wo=Wo, x_blocks=blocks, tail_lanes=tail, cpg=c.C // c.dg, dg=c.dg)


# ------------------------------------------------------------------------------------------- bounds
# The fp32 oracle's own largest error against the float64 reference over the tolerance tier, divided by
# max(1, |ref|max), as tests/test_dcn_v2_cases_cpu.py measures it (it asserts these figures are not exceeded; the
# per-case figures are in profiles/dcn_v2_regimes.md).  Most of it is the text's fp32 SAMPLE POSITION: integer + offset
# near 128 carries half an ulp = 7.6e-6 px, which the interpolation turns into a value error of that size.
ORACLE_ERR = {"out": 1.6e-6, "grad_input": 4.9e-6, "grad_trans": 3.0e-6,
              "col": 7.8e-6, "grad_im": 5.5e-6, "grad_offset": 6.4e-6, "grad_mask": 6.0e-6}
# what tests/test_gpu_dcn_v2.py already states for the same comparisons
SUITE_BOUND = {"out": 2e-6, "grad_input": 2e-5, "grad_trans": 1e-4,
               "col": 2e-5, "grad_im": 1e-4, "grad_offset": 1e-4, "grad_mask": 1e-4}
# the device sums in another order (lanes, atomics, the wave reduction): four times the oracle's own error, or the
# suite's bound where that is larger; times max(1, |ref|max)
BOUND = {k: max(4.0 * ORACLE_ERR[k], SUITE_BOUND[k]) for k in SUITE_BOUND}
# tests/test_gpu_reference_kernels.py, against the compiled reference kernels (absolute; grad_trans x max(1, |ref|max))
REFHIP_ATOL = {"out": 2e-6, "grad_input": 2e-5, "grad_trans": 1e-4, "col": 1e-6, "grad_im": 2e-5, "grad_offset": 2e-5,
               "grad_mask": 2e-5}
NHWC_GEMM_BOUND = 2e-5                # tests/test_gpu_conv_igemm.py / test_gpu_conv_wgrad.py: of the output scale


# ------------------------------------------------------------------------------------------- pooling table
def _pc(name, tier, kind, R, od, G, P, part, ncls, spp, scale, modes=(False, True), N=2, H=9, W=11, refhip=False,
        tstd=None):
    """modes: the no_trans values the case runs with"""
    return NS(name=name, tier=tier, kind=kind, N=N, H=H, W=W, R=R, od=od, G=G, P=P, part=part, ncls=ncls, spp=spp,
              scale=scale, tstd=(0.25 if tier == "exact" else 0.1) if tstd is None else tstd, modes=tuple(modes),
              refhip=refhip)


_CHANNEL = [
    # name, od, G, classes, P (exact), spp (exact), scale, modes
    ("baseline", 8, 1, 1, 2, 2, 0.25, (False, True)),
    ("classes3-vec4", 24, 1, 3, 2, 2, 1.0, (False, True)),
    ("chunks3-tail2", 520, 1, 1, 2, 1, 0.25, (True,)),
    ("chunks2-full", 1024, 1, 2, 2, 1, 1.0, (False, True)),
    ("group1-scalar", 6, 1, 2, 4, 2, 0.25, (False, True)),
    ("c-not-mult-4", 10, 1, 1, 2, 2, 1.0, (False, True)),
    ("group2-chunks2-tail6", 70, 2, 1, 4, 1, 0.25, (False, True)),
    ("group3-cec4", 8, 3, 2, 4, 2, 1.0, (False, True)),
    ("group2-cec1", 4, 2, 4, 2, 2, 0.25, (False, True)),
]
_TOL_BINS = [(3, 3), (6, 4), (7, 4), (3, 4), (7, 3), (6, 3)]

POOL_CASES = []
for _k, (_n, _od, _G, _cl, _P, _spp, _sc, _modes) in enumerate(_CHANNEL):
    POOL_CASES.append(_pc("ch/" + _n, "exact", "channel", 6, _od, _G, _P, _P, _cl, _spp, _sc, _modes, refhip=True))
    _tp, _ts = _TOL_BINS[_k % len(_TOL_BINS)]
    POOL_CASES.append(_pc("ch/" + _n + "/tol", "tolerance", "channel", 6, _od, _G, _tp, _tp, _cl, _ts, 0.25, _modes,
                          refhip=True))
POOL_CASES += [
    _pc("part/P4-part2", "exact", "part", 6, 8, 1, 4, 2, 2, 2, 1.0),
    _pc("part/P2-part1", "exact", "part", 6, 8, 2, 2, 1, 1, 2, 0.25),
    _pc("part/P6-part4", "tolerance", "part", 6, 8, 2, 6, 4, 2, 3, 0.25),
    _pc("part/P7-part1", "tolerance", "part", 6, 4, 1, 7, 1, 1, 4, 0.25),
    _pc("geo/P2", "exact", "geometry", 11, 8, 1, 2, 2, 1, 2, 1.0),
    _pc("geo/P4", "exact", "geometry", 6, 8, 2, 4, 4, 2, 2, 1.0),
    _pc("geo/width-clamp", "tolerance", "geometry", 8, 8, 1, 3, 3, 2, 3, 0.25),
    _pc("geo/bad-batch", "exact", "badbatch", 10, 8, 2, 2, 2, 2, 2, 0.25),
    _pc("lap2", "tolerance", "lap", 5500, 4, 1, 7, 7, 1, 2, 0.25, N=4, H=16, W=16),
]
LAP_DISTINCT = 250                    # lap2: 250 distinct RoIs x 22 repeats = 5500
POOL_BY_NAME = {c.name: c for c in POOL_CASES}


def _ints(rng, shape, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, size=shape).astype(F)


def _exact_roi(rng, c):
    """integer corners; the scaled extent is a multiple of P * spp (bins and sample steps are integers)"""
    unit = c.P * c.spp
    r = [float(rng.integers(0, c.N))]
    for lim in (c.W, c.H):
        ext = unit * int(rng.integers(1, max(2, 16 // unit + 1)))
        ext_img = int(round(ext / c.scale))
        lo = int(rng.integers(-ext_img // 2, int(lim / c.scale) - ext_img // 2 + 1))
        r += [lo, lo + ext_img - 1]
    return np.array([r[0], r[1], r[3], r[2], r[4]], F)


def _tol_roi(rng, c):
    x1, y1 = rng.uniform(-12, c.W / c.scale), rng.uniform(-12, c.H / c.scale)
    return np.array([rng.integers(0, c.N), x1, y1, x1 + rng.uniform(0, c.W / c.scale / 1.5),
                     y1 + rng.uniform(0, c.H / c.scale / 1.5)], F)


def _trans_of(rng, c, R):
    shape = (R, 2 * c.ncls, c.part, c.part)
    if c.tier == "exact":
        return (rng.integers(-8, 9, size=shape) / 8.0).astype(F)
    return rng.standard_normal(shape).astype(F)


def _cfg(c, no_trans):
    return (bool(no_trans), c.scale, c.od, c.G, c.P, c.part, c.spp, c.tstd)


def _row_clears(c, x_shape, roi, trans):
    """tolerance tier: every decision of this RoI clears MARGIN with and without trans, and the fp32 oracle counts the
    samples the float64 rule counts"""
    dummy = np.zeros(x_shape, F)
    for no_trans in (False, True):
        _, cnt, mg = RF.psroi_forward(dummy, roi[None], trans[None], *_cfg(c, no_trans))
        if not mg.every()[0] >= MARGIN:
            return False
        if not np.array_equal(O.deform_psroi_forward(dummy, roi[None], trans[None], *_cfg(c, no_trans))[1], cnt):
            return False
    return True


_GEO_P2 = [  # batch, x1, y1, x2, y2, trans value (None: random eighths)
    (0, 20, 20, 27, 27, None),          # wholly outside the 9 x 11 map
    (1, -2, -2, 5, 5, 0.0),             # half outside: 1, 2 and 4 samples per bin
    (0, 5, 3, 12, 10, 0.0),             # samples at 10.5 = W - 0.5 and 8.5 = H - 0.5: kept, clamped to W - 1, H - 1
    (0, 0, 0, 7, 7, 0.0),               # samples at -0.5: kept, clamped to 0
    (1, 4, 2, 11, 9, 0.25),             # shifted by 0.5: integer coordinates 4, 6, 8, 10 = W - 1 and 2, 4, 6, 8 = H - 1
    (0, 2.5, -2.5, 9.5, 4.5, None),     # round(): 3, -3, 10, 5 (to even would give 2, -2, 10, 4)
    (0, 2.49, -2.49, 9.49, 4.49, None),
    (0, 2.51, -2.51, 9.51, 4.51, None),
    (1, 3.5, 3.5, 6.5, 6.5, None),      # 4, 4, 7, 7
    (0, 6, 4, 13, 11, 1.0),             # + 2 px: the last bin leaves the map
    (1, -1, -1, 6, 6, -1.0),            # - 2 px: the first bin leaves the map
]
_GEO_P4 = [
    (0, -5, -5, 2, 2, 0.0),             # per axis 0, 0, 1, 2 kept samples: counts 0, 1, 2 and 4 in one RoI
    (1, 9, 7, 16, 14, 0.0),             # the same at the far border
    (0, 30, -30, 37, -23, None),        # wholly outside
    (1, 1, 0, 8, 7, None),
    (0, 3, 1, 10, 8, 0.5),
    (1, -6, 2, 9, 9, None),
]
GEO_ROUNDING_ROWS = (5, 6, 7)           # geo/P2: row 5 (x.5) has to equal row 7 (x.51) and differ from row 6 (x.49)


@functools.lru_cache(maxsize=None)
def pool_inputs(name):
    c = POOL_BY_NAME[name]
    rng = np.random.default_rng(abs(hash_name(name)))
    C = c.od * c.G * c.G
    shape = (c.N, C, c.H, c.W)
    R = LAP_DISTINCT if c.kind == "lap" else c.R
    fixed = {"geo/P2": _GEO_P2, "geo/P4": _GEO_P4}.get(name)
    if c.tier == "exact":
        x, g = _ints(rng, shape), _ints(rng, (R, c.od, c.P, c.P))
        trans = _trans_of(rng, c, R)
        if fixed:
            rois = np.array([r[:5] for r in fixed], F)
            for n, r in enumerate(fixed):
                if r[5] is not None:
                    trans[n] = r[5]
        else:
            rois = np.stack([_exact_roi(rng, c) for _ in range(R)])
        if c.kind == "badbatch":
            rois[:, 0] = [-1, 0, c.N, 1, -1, 0, c.N + 3, 1, 0, -7]
    else:
        x, g = rng.standard_normal(shape).astype(F), rng.standard_normal((R, c.od, c.P, c.P)).astype(F)
        rois, trans = np.zeros((R, 5), F), np.zeros((R, 2 * c.ncls, c.part, c.part), F)
        for n in range(R):
            for _ in range(200):
                roi, t = _tol_roi(rng, c), _trans_of(rng, c, 1)[0]
                if name == "geo/width-clamp" and n < 5:          # x2 < x1 - 1 and / or y2 < y1 - 1: width 0.1
                    roi[1], roi[2] = rng.uniform(8, c.W / c.scale - 8), rng.uniform(8, c.H / c.scale - 8)   # on the map
                    roi[3] = roi[1] + (rng.uniform(4, 12) if n == 1 else -rng.uniform(1.6, 9.0))
                    roi[4] = roi[2] + (rng.uniform(4, 12) if n == 0 else -rng.uniform(1.6, 9.0))
                if _row_clears(c, shape, roi, t):
                    break
            else:
                raise AssertionError("%s: no RoI clears the margins" % name)
            rois[n], trans[n] = roi, t
    return NS(case=c, x=x, rois=rois, trans=trans, grad=g)


def hash_name(name):
    """a seed that does not depend on the interpreter's string hashing"""
    return int.from_bytes(name.encode()[:8].ljust(8, b"\0"), "little") % (2 ** 31) + len(name)


def pool_device_inputs(name):
    """what the kernels see: the lap case repeats its distinct RoIs (with their trans and gradient rows)"""
    inp = pool_inputs(name)
    if inp.case.kind != "lap":
        return inp
    k = inp.case.R // LAP_DISTINCT
    return NS(case=inp.case, x=inp.x, rois=np.tile(inp.rois, (k, 1)), trans=np.tile(inp.trans, (k, 1, 1, 1)),
              grad=np.tile(inp.grad, (k, 1, 1, 1)))


@functools.lru_cache(maxsize=None)
def pool_reference(name, no_trans):
    """float64: out, count, grad_input, grad_trans (None with no_trans) for the DEVICE inputs, the margins, and the
    absolute-term sums of the backward.  The lap case: output rows repeat, grad_input is the distinct RoIs' times the
    number of repeats, grad_trans rows repeat"""
    inp = pool_inputs(name)
    c = inp.case
    out, cnt, mg = RF.psroi_forward(inp.x, inp.rois, inp.trans, *_cfg(c, no_trans))
    gi, gt, _, ab = RF.psroi_backward(inp.grad, cnt, inp.x, inp.rois, inp.trans, *_cfg(c, no_trans), with_abs=True)
    k = 1
    if c.kind == "lap":
        k = c.R // LAP_DISTINCT
        out, cnt, gi = np.tile(out, (k, 1, 1, 1)), np.tile(cnt, (k, 1, 1, 1)), gi * k
        gt = None if gt is None else np.tile(gt, (k, 1, 1, 1))
    return NS(out=out, count=cnt, grad_input=gi, grad_trans=gt, margins=mg, abs=ab, repeats=k)


# ------------------------------------------------------------------------------------------- convolution table
def _cc(name, B, C, H, W, k, pad, stride, dil, dg, refhip=True):
    return NS(name=name, B=B, C=C, H=H, W=W, k=k, pad=pad, stride=(stride, stride), dil=(dil, dil), dg=dg, refhip=refhip)


CONV_CASES = [
    _cc("wo64-cpg8", 2, 8, 3, 64, 3, (1, 1), 1, 1, 1),             # full blocks; two channels per wave
    _cc("wo65-cpg1-dg2", 1, 2, 3, 65, 3, (1, 1), 1, 1, 2),         # a 1-lane tail; three waves idle
    _cc("wo70-cpg5-dg3", 2, 15, 3, 70, 3, (1, 1), 1, 1, 3),        # a 6-lane tail; 5 channels over 4 waves
    _cc("wo130-cpg3", 1, 3, 3, 130, 3, (1, 1), 1, 1, 1),           # two blocks and a 2-lane tail
    _cc("wo65-s2-d2-cpg2-dg2", 2, 4, 5, 129, 3, (2, 2), 2, 2, 2),
    _cc("wo70-1x1-cpg2-dg3", 1, 6, 3, 70, 1, (0, 0), 1, 1, 3),
    _cc("wo66-pad21-cpg2", 2, 2, 4, 66, 3, (2, 1), 1, 1, 1),       # the asymmetric padding
]
CONV_BY_NAME = {c.name: c for c in CONV_CASES}
TIERS = ("exact", "tolerance")


def conv_out_hw(c):
    return O._dcn_out(c.H, c.W, c.k, c.k, c.pad, c.stride, c.dil)


def conv_args(c, pad=None):
    return (c.k, c.k, pad or c.pad, c.stride, c.dil, c.dg)


def _redraw_offsets(rng, c, off, draw):
    """tolerance tier: redraw the offsets whose sample is within MARGIN of -1, H / W or an integer"""
    Ho, Wo = off.shape[2:]
    for _ in range(50):
        h, w, inside, _ = RF._conv_geometry(off, (c.H, c.W), c.k, c.k, c.pad, c.stride, c.dil, c.dg)
        bad_h = (np.minimum(np.abs(h + 1), np.abs(h - c.H)) < MARGIN) | (RF._dist_to_integer(h) < MARGIN)
        bad_w = (np.minimum(np.abs(w + 1), np.abs(w - c.W)) < MARGIN) | (RF._dist_to_integer(w) < MARGIN)
        bad = np.stack([bad_h, bad_w], 3).reshape(off.shape)
        if not bad.any():
            return off
        off[bad] = draw(int(bad.sum()))
    raise AssertionError("%s: offsets do not clear the margins" % c.name)


@functools.lru_cache(maxsize=None)
def conv_inputs(name, tier):
    c = CONV_BY_NAME[name]
    rng = np.random.default_rng(hash_name(name + tier))
    Ho, Wo = conv_out_hw(c)
    kk = c.k * c.k
    s_off, s_mask, s_col = (c.B, c.dg * 2 * kk, Ho, Wo), (c.B, c.dg * kk, Ho, Wo), (c.C * kk, c.B, Ho, Wo)
    if tier == "exact":
        im, gcol = _ints(rng, (c.B, c.C, c.H, c.W)), _ints(rng, s_col)
        off = (rng.integers(-12, 13, size=s_off) / 4.0).astype(F)
        mask = (rng.integers(0, 9, size=s_mask) / 8.0).astype(F)
    else:
        im, gcol = rng.standard_normal((c.B, c.C, c.H, c.W)).astype(F), rng.standard_normal(s_col).astype(F)
        draw = lambda n: (rng.standard_normal(n) * 2.5).astype(F)
        off = _redraw_offsets(rng, c, draw(int(np.prod(s_off))).reshape(s_off), draw)
        mask = rng.uniform(0, 1, size=s_mask).astype(F)
    return NS(case=c, tier=tier, im=im, off=off, mask=mask, gcol=gcol)


@functools.lru_cache(maxsize=None)
def conv_reference(name, tier, masked):
    inp = conv_inputs(name, tier) if name != BORDER.name else border_inputs()
    c = inp.case
    m = inp.mask if masked else None
    col, mg = RF.mdcn_im2col(inp.im, inp.off, m, *conv_args(c))
    gim, _ = RF.mdcn_col2im(inp.gcol, inp.off, m, inp.im.shape, *conv_args(c))
    goff, gmask, _ = RF.mdcn_col2im_coord(inp.gcol, inp.im, inp.off, m, *conv_args(c))
    return NS(col=col, grad_im=gim, grad_offset=goff, grad_mask=gmask, margins=mg)


# ------------------------------------------------------------------------------------------- the border fixture
BORDER = _cc("border-5x6", 2, 16, 5, 6, 3, (1, 1), 1, 1, 1, refhip=False)
BORDER_CLASSES = ("below -1", "at -1", "in (-1, 0)", "at 0", "interior integer", "interior fraction", "at size - 1",
                  "in (size - 1, size)", "at size", "above size")


def border_positions(size):
    """one position per class of BORDER_CLASSES on an axis of `size` pixels (quarters: exact tier)"""
    return np.array([-1.5, -1.0, -0.25, 0.0, 2.0, 1.25, size - 1.0, size - 0.75, float(size), size + 0.5])


def border_class(v, size):
    v = np.asarray(v, np.float64)
    conds = [v < -1, v == -1, (v > -1) & (v < 0), v == 0, (v > 0) & (v < size - 1) & (v == np.round(v)),
             (v > 0) & (v < size - 1) & (v != np.round(v)), v == size - 1, (v > size - 1) & (v < size), v == size, v > size]
    return np.select(conds, np.arange(10), -1)


@functools.lru_cache(maxsize=None)
def border_inputs():
    """5 x 6 map, 3 x 3, stride 1, pad 1, one deformable group, 16 channels (what every channels-last route accepts):
    sample s of image b sits at class pair (s + 37 b) mod 100 -- all 10 x 10 (row class, column class) pairs occur"""
    c = BORDER
    rng = np.random.default_rng(56)
    Ho, Wo = conv_out_hw(c)
    kk = 9
    off = np.zeros((c.B, 1, kk, 2, Ho, Wo), np.float64)
    ph, pw = border_positions(c.H), border_positions(c.W)
    s = 0
    for b in range(c.B):
        for t in range(kk):
            for ho in range(Ho):
                for wo in range(Wo):
                    pair = (s + 37 * b) % 100
                    off[b, 0, t, 0, ho, wo] = ph[pair // 10] - (ho - 1 + t // 3)
                    off[b, 0, t, 1, ho, wo] = pw[pair % 10] - (wo - 1 + t % 3)
                    s += 1
    return NS(case=c, tier="exact", im=_ints(rng, (c.B, c.C, c.H, c.W)), off=off.reshape(c.B, 2 * kk, Ho, Wo).astype(F),
              mask=(rng.integers(0, 9, size=(c.B, kk, Ho, Wo)) / 8.0).astype(F), gcol=_ints(rng, (c.C * kk, c.B, Ho, Wo)),
              weight=_ints(rng, (8, 3, 3, c.C), -4, 4), gy=_ints(rng, (c.B, Ho, Wo, 8), -4, 4))


def cols_nhwc(col, c):
    """(C * kk, B, Ho, Wo) -> the channels-last column matrix [pos][tap][c]"""
    kk = c.k * c.k
    Ho, Wo = col.shape[2:]
    return col.reshape(c.C, kk, c.B, Ho, Wo).transpose(2, 3, 4, 1, 0).reshape(c.B * Ho * Wo, kk * c.C)
