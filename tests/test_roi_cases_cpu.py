"""CPU: the conditions tests/roi_cases.py promises to the multi-level RoIAlign pins (tests/test_gpu_roi_align_levels.py),
recomputed here without its vectorised helpers: one RoI at a time, from the kernels' formulas (csrc/roi_geom.h)."""
import math

import numpy as np
import pytest

from tests import inputs as I
from tests import roi_cases as RCS


def _nearest_line_one_roi(kroi, stride, dialect, gh, gw, tile=RCS.TILE, PH=7, PW=7):
    """distance (map pixels) of the nearest sample of ONE RoI to x = -1, x = W, y = -1, y = H"""
    _, x0, y0, w, h, th = (float(v) for v in kroi)
    size = tile / stride
    off = 0.5 if dialect == "rot_v1" else 0.0
    cx, cy = x0 / stride - off, y0 / stride - off
    w, h = max(w / stride, 1.0), max(h / stride, 1.0)
    c, s = math.cos(th), math.sin(th)
    best = float("inf")
    for ph in range(PH):
        for iy in range(gh):
            yy = -h / 2 + ph * (h / PH) + (iy + 0.5) * (h / PH) / gh
            for pw in range(PW):
                for ix in range(gw):
                    xx = -w / 2 + pw * (w / PW) + (ix + 0.5) * (w / PW) / gw
                    if dialect == "rot_v1":
                        x, y = xx * c + yy * s + cx, yy * c - xx * s + cy
                    else:
                        x, y = xx * c - yy * s + cx, xx * s + yy * c + cy
                    best = min(best, abs(x + 1), abs(x - size), abs(y + 1), abs(y - size))
    return best


def _check_lines(krois, lvl, dialect, sampling, strides, step=1):
    worst = float("inf")
    for r in range(0, krois.shape[0], step):
        stride = strides[int(lvl[r])]
        if sampling > 0:
            gh = gw = sampling
        else:
            gh = int(math.ceil(np.float32(max(np.float32(krois[r, 4]) * np.float32(1.0 / stride), np.float32(1))) / np.float32(7)))
            gw = int(math.ceil(np.float32(max(np.float32(krois[r, 3]) * np.float32(1.0 / stride), np.float32(1))) / np.float32(7)))
        worst = min(worst, _nearest_line_one_roi(krois[r], stride, dialect, gh, gw))
    return worst


# orcnn-infer is forward only: it has no second step
@pytest.mark.parametrize("name,step", [(n, 0) for n in sorted(RCS.MULTI)]
                         + [(n, RCS.SECOND_STEP_SEED) for n in sorted(RCS.MULTI) if n != "orcnn-infer"])
def test_multi_level_cases_meet_their_conditions(name, step):
    c = RCS.multi_case(name, step)
    info, lvl, R = c["info"], c["lvl"], c["R"]
    assert c["rois"].dtype == np.float32 and c["rois"].shape == (R, 5 if c["dialect"] == "hbb1" else 6)
    assert lvl.shape == (R,) and lvl.min() >= 0 and lvl.max() <= 3
    # populations
    if name == "empty-level":
        # no RoI on the coarsest level and only a few (3 % of them) on the one before
        assert info["per_level"][3] == 0 and 1 <= info["per_level"][2] <= 0.05 * R, info
    else:
        assert min(info["per_level"]) >= 110, info
    # no level tie: recomputed from what the extractor sees
    if c["dialect"] == "hbb1":
        r = c["rois"].astype(np.float64)
        scale = np.sqrt((r[:, 3] - r[:, 1] + 1) * (r[:, 4] - r[:, 2] + 1))
    else:
        r = c["krois"].astype(np.float64)
        scale = np.sqrt(r[:, 3] * r[:, 4])
    t = np.log2(scale / 56 + 1e-6)
    assert np.abs(t - np.round(t)).min() >= RCS.TIE_EPS
    np.testing.assert_array_equal(np.clip(np.floor(t), 0, 3).astype(np.int64), lvl)
    assert info["ties"] <= 0.01 * R
    if c["dialect"] in RCS.TRIG:
        assert info["moved"] <= RCS.MAX_MOVED_SHARE * R and info["rounds"] <= RCS.MAX_ROUNDS
        assert info["lever"] <= RCS.MAX_LEVER
        assert _check_lines(c["krois"], lvl, c["dialect"], 2, RCS.STRIDES) >= RCS.LINE_EPS
        # the kernel-side RoIs are the given ones under the extractor's float32 enlargement
        if c["by"] == "extractor":
            np.testing.assert_array_equal(c["krois"][:, 3], c["rois"][:, 3] * np.float32(1.2))
            np.testing.assert_array_equal(c["krois"][:, 4], c["rois"][:, 4] * np.float32(1.4))
        else:
            np.testing.assert_array_equal(c["krois"], c["rois"])


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("R", [1024, 2048, 4000])
def test_spread_obbs_populate_every_level(seed, R):
    rois = RCS.spread_obbs(np.random.default_rng(seed), R, 2)
    lvl = RCS.levels_of(RCS.obb_scale(RCS.enlarge(rois, (1.2, 1.4))), 4)
    assert np.bincount(lvl, minlength=4).min() >= 110
    assert set(np.unique(rois[:, 0]).tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("dialect,R,sampling,seed", [("rot_v1", 2000, 2, 11), ("riroi", 2000, 2, 14),
                                                     ("rot_v1", 512, 0, 21)])
def test_single_level_cases_meet_their_conditions(dialect, R, sampling, seed):
    c = RCS.single_case(dialect, R, sampling, seed)
    info = c["info"]
    assert info["moved"] <= RCS.MAX_MOVED_SHARE * R and info["rounds"] <= RCS.MAX_ROUNDS and info["lever"] <= RCS.MAX_LEVER
    assert _check_lines(c["rois"], np.zeros(R, int), dialect, sampling, (4,)) >= RCS.LINE_EPS
    if sampling == 0:
        assert 8 <= info["grid"] <= 10          # I.random_obbs: up to 256 px = 64 map pixels over 7 bins


def test_a_roi_on_a_validity_line_is_moved():
    # rot, theta = 0, level 0 (stride 4): sample x of bin 0, grid point 0 = cx - w/2 + w/28 lands on x = -1 exactly
    w = 56.0
    cx_map = -1.0 + w / 4 / 2 - w / 4 / 28
    rois = np.array([[0, cx_map * 4, 300.0, w, 40.0, 0.0],
                     [0, 500.0, 500.0, 60.0, 30.0, 0.3]], np.float32)
    lvl = np.zeros(2, np.int64)
    dist, _, _ = RCS.line_distance(rois, lvl, "rot", 2)
    assert dist[0] < RCS.LINE_EPS <= dist[1]
    assert _check_lines(rois[:1], lvl, "rot", 2, RCS.STRIDES) < RCS.LINE_EPS
    out, info = RCS.keep_off_validity_lines(rois[[0] + [1] * 199], np.zeros(200, np.int64), "rot", 2)
    assert info["moved"] == 1 and info["rounds"] == 1
    np.testing.assert_array_equal(out[0, 1:3], rois[0, 1:3] + np.float32(RCS.MOVE))
    np.testing.assert_array_equal(out[1:], rois[[1] * 199])
    assert _check_lines(out[:2], lvl, "rot", 2, RCS.STRIDES) >= RCS.LINE_EPS
    # more than 1 % of the RoIs near a line: the helper refuses the set
    with pytest.raises(AssertionError):
        RCS.keep_off_validity_lines(rois[[0, 0, 1]], np.zeros(3, np.int64), "rot", 2)


def test_a_roi_on_a_level_tie_is_widened():
    # enlarged scale = 56 * 2 exactly: w * h * 1.2 * 1.4 = 112^2
    rois = np.array([[0, 100.0, 100.0, 112.0 / 1.2, 112.0 / 1.4, 0.1],
                     [0, 100.0, 100.0, 30.0, 50.0, 0.1]], np.float32)
    scale_of = lambda r: RCS.obb_scale(RCS.enlarge(r, (1.2, 1.4)))
    t = RCS.level_log2(scale_of(rois))
    assert abs(t[0] - 1.0) < RCS.TIE_EPS
    out, n = RCS.fix_level_ties(rois, scale_of)
    assert n == 1
    assert out[0, 3] == rois[0, 3] * np.float32(1.01) and np.array_equal(out[1], rois[1])
    t2 = RCS.level_log2(scale_of(out))
    assert np.abs(t2 - np.round(t2)).min() >= RCS.TIE_EPS and RCS.levels_of(scale_of(out), 4).tolist() == [1, 0]
    # the horizontal rule: (x2 - x1 + 1) * (y2 - y1 + 1) = 224^2
    hb = np.array([[0, 500.0, 500.0, 223.0, 223.0, 0.0]], np.float32)
    hs = lambda r: RCS.hbb_scale(I.obb_to_hbb_rois(r))
    assert abs(RCS.level_log2(hs(hb))[0] - 2.0) < RCS.TIE_EPS
    out, n = RCS.fix_level_ties(hb, hs)
    assert n == 1 and RCS.levels_of(hs(out), 4).tolist() == [2]
