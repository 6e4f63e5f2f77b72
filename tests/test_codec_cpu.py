"""No GPU: the float64 restatements of the rotated box codecs (tests/codec_ref.py) and their fixtures.

  * the fixtures hold their contract: at most 1 % of the boxes fall to the retention margins, every branch is taken by
    5-95 % of the boxes, sides and coordinates stay within their limits, means and stds are pairwise distinct, and on the
    retained boxes the float32 twin decides every branch as float64 does;
  * the restatements agree with the package's torch compositions run in float64 on the host (1e-12) and with the
    float32 twin of oracle/box_oracle.py (within e32, the float32 restatement's own error);
  * closed forms: decode(encode(g)) = g with the angle compared directly, da = db = 0.5 for an axis-aligned gt, the
    enclosing box of a square at pi/4;
  * mutation sensitivity: each wrong variant of a restatement breaks the GPU tests' bound on at least 1 % of the
    retained boxes of the fixture meant for it -- the bounds can tell right from wrong."""
import math

import numpy as np
import pytest
import torch

from tests import codec_ref as R

F64 = np.float64


def _t64(a):
    return torch.from_numpy(np.asarray(a, F64))


def _torch_route(codec, args, kw):
    """the package's general (torch) route of a codec, on the host in float64"""
    from jdet_amd.models.boxes import box_ops, coder
    from jdet_amd.models.boxes.iou_calculator import fake_rotated_boxes
    t = [_t64(a) for a in args]
    if codec == "b2d":
        out = box_ops.bbox2delta_rotated(*t, kw["means"], kw["stds"])
    elif codec == "d2b":
        out = box_ops.delta2bbox_rotated(*t, kw["means"], kw["stds"], None, kw["wh_ratio_clip"])
    elif codec == "hbb":
        out = fake_rotated_boxes(t[0])
    else:
        c = (coder.MidpointOffsetCoder if codec.startswith("mid") else coder.OrientedDeltaXYWHTCoder)(kw["means"], kw["stds"])
        out = c.encode(*t) if codec.endswith("enc") else c.decode(*t, wh_ratio_clip=kw["wh_ratio_clip"])
    assert out.dtype == torch.float64
    return out.numpy()


def _oracle_route(codec, args, kw):
    from oracle import box_oracle as B
    fn = dict(b2d=B.bbox2delta_rotated, d2b=B.delta2bbox_rotated, mid_enc=B.midpoint_offset_encode,
              mid_dec=B.midpoint_offset_decode, ori_enc=B.oriented_delta_encode, ori_dec=B.oriented_delta_decode)[codec]
    return fn(*args, **kw)


# which branch shares a fixture must hold within 5-95 %
SHARES = dict(d2b=("clamped",), ori_dec=("clamped", "swapped"), mid_dec=("clamped", "dab", "swapped"), ori_enc=("second",),
              hbb=("wide",), b2d=(), mid_enc=())


@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_fixture_holds_its_contract(name):
    f = R.fixture(name)
    n = R.N_ROWS
    dropped = 1.0 - float(f.keep.mean())
    shares = {k: float(f.flags[k].mean()) for k in SHARES[f.codec]}
    if f.variant == "lo":
        shares.update(lower=float(f.flags["lower"].mean()), upper=float(f.flags["upper"].mean()))
    if f.variant == "hi":
        shares.update(upper=float(f.flags["upper"].mean()))
    if f.codec == "mid_enc":        # the rows the masks decide on: both ways inside the near-axis slice
        shares.update(slice_two_top=float(f.flags["two_top"][f.slice].mean()),
                      slice_two_right=float(f.flags["two_right"][f.slice].mean()))
    print("%-13s dropped %.4f %%  construction kept %.3f of the drawn rows  shares %s  e32 %s"
          % (name, 100 * dropped, f.drawn_ok, {k: round(v, 3) for k, v in shares.items()},
             {k: "%.2e" % v for k, v in f.e32.items()}))
    assert dropped <= 0.01
    for k, v in shares.items():
        assert 0.05 <= v <= 0.95, (k, v)
    assert all(a.shape[0] == n and a.dtype == np.float32 for a in f.args)
    assert f.ncls == 1 or n % f.ncls
    for vals in (f.kw.get("means"), f.kw.get("stds")):
        if vals is not None:
            assert len(set(vals)) == len(vals)
            assert all(float(np.float32(v)) == v for v in vals)
    # limits: input coordinates and sizes, decoded sides and centres
    assert all(float(np.abs(a[:, :4]).max()) <= R.COORD_MAX for a in f.args if a.shape[1] in (4, 5))
    if f.codec in R.DECODES:
        b = f.ref.reshape(-1, 5)
        assert b[:, 2:4].min() >= R.SIDE_MIN and b[:, :4].max() <= R.COORD_MAX and b[:, :2].min() >= 0
    else:
        assert min(float(a[:, 2:4].min()) for a in f.args if a.shape[1] == 5) >= R.SIDE_MIN
    if f.codec in ("b2d", "d2b", "ori_enc", "ori_dec", "hbb"):
        ang = f.args[0][:, 4]
        assert ang.min() < -3.9 and ang.max() > 3.9 and np.abs(ang).max() <= 4
    # the float32 twin takes every branch as float64 does wherever the margins are cleared
    flags32 = f.run(np.float32)[2]
    for k, v in flags32.items():
        assert np.array_equal(np.asarray(v).reshape(n, -1)[f.keep], f.flags[k][f.keep]), k
    assert np.isfinite(f.ref).all() and np.isfinite(f.twin).all()


@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_restatement_equals_the_torch_composition_in_float64(name):
    f = R.fixture(name)
    got = _torch_route(f.codec, f.args, f.kw).reshape(f.ref.shape)
    cols = f.ref.shape[1] // f.keep.shape[1]
    keep = np.repeat(f.keep, cols, axis=1)
    np.testing.assert_allclose(got[keep], f.ref[keep], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", sorted(k for k, v in R.FIXTURES.items() if v[0] != "hbb"))
def test_float32_oracle_within_the_yardstick(name):
    f = R.fixture(name)
    got = _oracle_route(f.codec, f.args, f.kw)
    assert got.dtype == np.float32
    err = R.worst(R.errors(f.codec, got.reshape(f.ref.shape), f.ref), f.keep)
    print("%-13s oracle/box_oracle.py against float64 %s   e32 %s"
          % (name, {k: "%.2e" % v for k, v in err.items()}, {k: "%.2e" % v for k, v in f.e32.items()}))
    for k, e in f.e32.items():              # a host numpy twin: no device libm, no other order -- e32 itself, 1 % slack
        assert err[k] <= 1.01 * e, (k, err[k], e)


def _regular_gts(n, seed):
    rng = np.random.default_rng(seed)
    g = R._obbs(rng, n, (8.0, 300.0), (-math.pi / 2, math.pi / 2))
    g[:, 2:4] = np.stack([g[:, 2:4].max(1) * 1.01, g[:, 2:4].min(1)], 1)        # w > h
    return R._f32(g)


def test_round_trips_return_the_gt_with_its_angle():
    """decode(encode(g)) = g in float64 (1e-9, far inside every new bound), the angle compared directly: the gt's angle
    lies in the decoder's range.  wh_ratio_clip 1e-6 keeps the clamp out"""
    n = 1024
    g = _regular_gts(n, 5)
    p, _ = R._draw_pairs(np.random.default_rng(6), n)
    p[:, :2] = g[:, :2] + (p[:, :2] - p[:, :2].mean(0)) * 0.05
    for enc, dec in ((R.bbox2delta_rotated, R.delta2bbox_rotated), (R.oriented_encode, R.oriented_decode)):
        gg = g.copy()
        if enc is R.bbox2delta_rotated:             # norm_angle folds into [-pi/4, 3pi/4)
            gg[:, 4] = np.where(gg[:, 4] < -math.pi / 4, gg[:, 4] + np.float32(math.pi), gg[:, 4])
            gg = gg[np.abs(gg[:, 4].astype(F64) - 3 * math.pi / 4) > 1e-3]
        d = enc(p[:len(gg)], gg, R.M5, R.S5)[0]
        back = dec(p[:len(gg)], d, R.M5, R.S5, 1e-6)[0]
        e = R.errors("d2b", back, gg.astype(F64))
        assert e["xywh"].max() < 1e-9 and e["angle"].max() < 1e-9, (enc.__name__, e["xywh"].max(), e["angle"].max())
    # midpoint offsets describe a rectangle exactly when each extreme is reached by ONE vertex (no mask ambiguity)
    gm = _regular_gts(n, 8)
    c, s = np.cos(gm[:, 4].astype(F64)), np.sin(gm[:, 4].astype(F64))
    xb = np.abs(gm[:, 2] / 2 * c) + np.abs(gm[:, 3] / 2 * s)
    yb = np.abs(gm[:, 2] / 2 * s) + np.abs(gm[:, 3] / 2 * c)
    a = R._f32(np.stack([gm[:, 0] - xb * 1.1, gm[:, 1] - yb * 0.9, gm[:, 0] + xb * 1.2, gm[:, 1] + yb], 1))
    d, _, fl = R.midpoint_encode(a, gm, R.M6, R.S6)
    one = ~fl["two_top"] & ~fl["two_right"]
    assert one.mean() > 0.9
    back = R.midpoint_decode(a[one], d[one], R.M6, R.S6, 1e-6)[0]
    e = R.errors("mid_dec", back, gm[one].astype(F64))
    assert e["xywh"].max() < 1e-9 and e["angle"].max() < 1e-8, (e["xywh"].max(), e["angle"].max())


def test_closed_forms():
    codec, (a, g), kw = R.edge_cases()["mid_enc_axis"]
    out = R.midpoint_encode(a, g, **kw)[0]
    axis = g[:, 4] == 0
    assert axis.sum() >= 7
    assert np.array_equal(out[axis, 4:], np.full((int(axis.sum()), 2), 0.5))          # da = db = +0.5, means 0, stds 1
    out32 = R.midpoint_encode(a, g, dt=np.float32, **kw)[0]
    assert np.array_equal(out32[axis, 4:], np.full((int(axis.sum()), 2), 0.5, np.float32))
    # a square at pi/4: the enclosing box is the square of side w * sqrt(2); with x = y the two extents are the same
    # operations on the same numbers, so ww == hh in every precision: the >= side of the tie, angle 0
    q = float(np.float32(math.pi / 4))
    for dt in (np.float64, np.float32):
        o, m, fl = R.obb2hbb2obb(np.asarray([[128, 128, 32, 32, q]], np.float32), dt=dt)
        assert m["wwhh"][0] == 0 and fl["wide"][0] and o[0, 4] == 0 and o[0, 2] == o[0, 3]
        assert abs(o[0, 2] - 32 * math.sqrt(2)) < 1e-5 and o[0, 0] == 128 and o[0, 1] == 128
    # a decoded square takes regular_obb's tie branch: sides swapped (equal), angle + pi/2, folded
    o, m, fl = R.oriented_decode(np.asarray([[100, 100, 32, 32, 0.25]], np.float32), np.zeros((1, 5), np.float32),
                                 R.EDGE_M5, R.EDGE_S5)
    assert fl["swapped"][0, 0] and m["wh"][0, 0] == 0 and abs(o[0, 4] - (0.25 + math.pi / 2 - math.pi)) < 1e-15


def test_edge_cases_are_the_edges_they_claim():
    """some hundred rows, and each family sits ON its threshold: zero margin in the float32 twin"""
    cases = R.edge_cases()
    rows = sum(c[1][0].shape[0] for c in cases.values())
    assert 64 <= rows <= 128, rows
    assert {c[1][0].shape[0] for c in cases.values()} >= {0, 1}
    run = lambda name: R.CODECS[cases[name][0]](*cases[name][1], dt=np.float32, **cases[name][2])      # noqa: E731
    _, m, fl = run("ori_dec_edges")
    assert (m["wh"][:4, 0] == 0).all() and fl["swapped"][:4, 0].all()               # squares
    assert m["clamp"][4, 0] == 0 and m["clamp"][6, 0] == 0                          # dw / dh exactly max_ratio
    assert (m["wrap"][[1, 8, 9], 0] == 0).all()                                     # angle sums on a wrap point
    _, m, fl = run("ori_enc_ties")
    assert m["tie"][0] < 1e-7 and m["tie"][1] < 1e-7 and m["wrap"][4] == 0
    _, m, fl = run("mid_dec_edges")
    assert (m["dab"][[0, 1, 2, 3, 7, 11]] == 0).all() and fl["dab"][[4, 6]].all() and not fl["dab"][5]
    assert m["clamp"][12] == 0 and fl["upper"][13]
    assert fl["dab_both"][14:18].all() and not fl["dab_both"][:14].any()            # both beyond the clamp: (+, +), (-, -)
    assert (m["wrap"][[15, 17]] == 0).all()            # the tall anchor: -pi/2 unswapped, 0 + pi/2 swapped -- on the fold
    assert m["clamp"][18] == 0 and not fl["lower"][18] and fl["lower"][19]          # exactly -max_ratio; one ulp beyond
    _, m, fl = run("d2b_edges")
    assert m["clamp"][4, 0] == 0 and m["clamp"][16, 0] == 0 and not fl["lower"][16, 0] and fl["lower"][17, 0] and fl["upper"][5, 0]
    assert (m["wrap"][13:16, 0] == 0).all()
    _, m, fl = run("hbb_squares")
    assert (m["wwhh"][[0, 1, 4]] == 0).all()
    _, m, fl = run("mid_enc_axis")
    assert fl["two_top"].all() and fl["two_right"].all()


# mutation -> the fixtures meant for it (a third element: judged on the fixture's near-axis slice)
MUTATIONS = [
    ("no_clamp", "d2b_hi3"), ("no_clamp", "d2b_lo15"), ("no_clamp", "ori_dec_hi3"), ("no_clamp", "ori_dec_lo1"),
    ("no_clamp", "mid_dec_hi"), ("no_clamp", "mid_dec_lo"),
    ("upper_only", "d2b_lo15"), ("upper_only", "d2b_lo1"), ("upper_only", "ori_dec_lo15"), ("upper_only", "mid_dec_lo"),
    ("no_dab_clamp", "mid_dec_hi"), ("no_dab_clamp", "mid_dec_lo"),
    ("wrap0pi", "ori_dec_hi3"), ("wrap0pi", "ori_dec_lo15"), ("wrap0pi", "mid_dec_lo"), ("wrap0pi", "ori_enc"),
    ("norm_start", "d2b_hi3"), ("norm_start", "d2b_lo1"), ("norm_start", "b2d"),
    ("no_half_pi", "ori_dec_hi3"), ("no_half_pi", "ori_dec_lo1"), ("no_half_pi", "mid_dec_hi"),
    ("mask005", "mid_enc", "slice"), ("mask02", "mid_enc", "slice"),
    ("swap23", "b2d"), ("swap23", "d2b_lo15"), ("swap23", "ori_enc"), ("swap23", "ori_dec_hi3"), ("swap23", "mid_enc"),
    ("swap23", "mid_dec_lo"),
    ("swap01", "b2d"), ("swap01", "d2b_lo15"), ("swap01", "ori_enc"), ("swap01", "ori_dec_hi3"), ("swap01", "mid_enc"),
    ("swap01", "mid_dec_lo"),
    ("mod_ncls", "d2b_hi3"), ("mod_ncls", "d2b_lo15"), ("mod_ncls", "ori_dec_hi3"), ("mod_ncls", "ori_dec_lo15"),
    ("cos_pt", "ori_enc"), ("cos_pt", "ori_dec_lo15"),
]


@pytest.mark.parametrize("case", MUTATIONS, ids=["-".join(c) for c in MUTATIONS])
def test_bound_tells_the_mutation_from_the_restatement(case):
    mut, name = case[:2]
    f = R.fixture(name)
    rows = f.slice if len(case) > 2 else None
    assert f.broken_share(f.ref, rows) == 0 and f.broken_share(f.twin, rows) == 0
    with np.errstate(over="ignore", invalid="ignore"):
        wrong = f.run(mut=mut)[0]
    share = f.broken_share(wrong, rows)
    print("%-13s %-12s breaks the bound on %.1f %% of the retained boxes" % (name, mut, 100 * share))
    assert share >= 0.01
