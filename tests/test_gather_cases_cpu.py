"""The case table of tests/test_gpu_gather_regimes.py, checked on the CPU from the oracles alone: every exact-tier
fixture is exact (no rounding in any summation order), every case is in the regime it claims, and the table as a whole
reaches every regime of csrc/csr_gather.h and of the RoIAlign producer."""
import numpy as np
import pytest

from tests import gather_cases as G

PIXEL = [c.name for c in G.PIXEL_CASES]
ROI = [c.name for c in G.ROI_CASES]


def _assert_exact(ref, ref_abs, unit, what):
    """1. the reference is a multiple of 1/unit; 2. per pixel, sum |contribution| * unit < 2^24 (the weights are
    non-negative, so the oracle applied to |grad| is that sum): every partial sum is an fp32 integer / unit"""
    scaled = ref.astype(np.float64) * unit
    assert np.array_equal(scaled, np.round(scaled)), what + ": the reference is not a multiple of 1/%g" % unit
    peak = float(ref_abs.astype(np.float64).max()) * unit
    assert peak < 2.0 ** 24, what + ": sum |contribution| * unit = %g >= 2^24" % peak


def _assert_claims(regime, claims, what):
    for key, want in claims.items():
        assert regime[key] == want, "%s: claims %s = %r, is in %r" % (what, key, want, regime[key])


@pytest.mark.parametrize("name", PIXEL)
def test_pixel_case_is_exact_and_in_its_regime(name):
    inp = G.pixel_inputs(name)
    if inp.case.tier == "exact":
        _assert_exact(G.pixel_reference(inp), G.pixel_reference(inp, np.abs(inp.grad)), inp.unit, name)
    _assert_claims(G.pixel_regime(inp), inp.case.claims, name)


@pytest.mark.parametrize("name", ROI)
def test_roi_case_is_exact_and_in_its_regime(name):
    inp = G.roi_inputs(name)
    if inp.case.tier == "exact":
        _assert_exact(G.roi_reference(inp), G.roi_reference(inp, np.abs(inp.grad)), inp.unit, name)
    _assert_claims(G.roi_regime(inp), inp.case.claims, name)


def test_kept_workspace_chain_is_exact_and_alternates_overflow():
    flags = []
    for step in range(3):
        inp = G.chain_inputs(step)
        _assert_exact(G.roi_reference(inp), G.roi_reference(inp, np.abs(inp.grad)), inp.unit, inp.case.name)
        flags.append(G.roi_regime(inp)["overflow"])
    assert flags == [True, False, True]
    assert G.patch_grid(*G.CHAIN_SHAPE).php % 2 == 1       # a workgroup's 2x2 patches straddle two images


def test_restated_cap_formula():
    """spot values worked out by hand from patch_direct_cap's definition"""
    assert G.cap_of(120, 3 * 1024) == 32 and G.cap_of(120, 5 * 1024) == 64
    assert G.cap_of(120, 10 * 1024) == 128 and G.cap_of(120, 16 * 1024) == 256
    assert G.cap_of(16384, 2000 * 784) == 128        # 256x256 map, 2000 RoIs of 7x7 bins at sampling 2
    assert G.cap_of(262144, 64 * 784) == 32          # 262144 * 32 * 32 B = 256 MiB: not past the limit
    assert G.cap_of(262145, 64 * 784) == 16 and G.cap_of(525625, 64 * 784) == 0
    assert G.tile_count(2048) == 1 and G.tile_count(2049) == 2 and G.tile_count(525625) == 257


def test_bilinear_taps_rule():
    ys, xs, ws, keep = G.bilinear_taps(np.array([0.25, -0.5, -1.0, 2.0, 3.0]), np.array([0.5, 0.0, 0.0, 1.0, 0.0]), 3, 2)
    assert keep[:, 0].all() and np.allclose(ws[:, 0], [0.375, 0.375, 0.125, 0.125])
    assert keep[:, 1].tolist() == [False, False, True, False] and ws[2, 1] == 0.5     # row -1 off the map, lw = 0
    assert not keep[:, 2].any() and not keep[:, 4].any()                            # h = -1 and h = H: outside
    assert keep[:, 3].tolist() == [True, False, False, False] and (ys[0, 3], xs[0, 3], ws[0, 3]) == (2, 1, 1.0)


def test_the_table_reaches_every_regime():
    roi = {n: G.roi_regime(G.roi_inputs(n)) for n in ROI}
    pix = {n: G.pixel_regime(G.pixel_inputs(n)) for n in PIXEL}
    # direct-row caps, each non-zero one with and without a row past it
    assert {r["cap"] for r in roi.values()} >= {0, 32, 64, 128, 256}
    for cap in (32, 64, 128, 256):
        assert {r["overflow"] for r in roi.values() if r["cap"] == cap and "overflow" in r} == {True, False}, cap
    assert any(r["cap"] == 0 and r["overflow"] and r["tiles"] > 256 for r in roi.values())
    # scan: one tile, several, more than 256 (both key kinds)
    for regimes in (roi, pix):
        tiles = {r["tiles"] for r in regimes.values()}
        assert 1 in tiles and any(t > 256 for t in tiles)
    assert any(2 <= r["tiles"] <= 256 for r in pix.values())
    assert any(2 <= r["tiles"] <= 256 and len(r.get("overflow_tiles", ())) > 1 for r in roi.values())
    # pixel-keyed rows
    rows = np.concatenate([G.pixel_row_lengths(G.pixel_inputs(n)) for n in PIXEL if not G.pixel_inputs(n).case.large])
    assert (rows == 0).any() and rows.max() >= 1000
    assert {int(v) for v in np.unique(rows[rows > 0] % 4)} == {0, 1, 2, 3}
    # pixel-keyed work mapping
    assert any(r["laps"] >= 2 for r in pix.values()) and any(r["straddles_images"] for r in pix.values())
    assert any(r["odd_w"] for r in pix.values()) and {r["chunks"] for r in pix.values()} >= {1, 2}
    # patch rows
    prow = np.concatenate([G.patch_row_lengths(c.variant, G.roi_inputs(c.name).rois, c.N, c.H, c.W, c.PH, c.PW, c.s)
                           for c in G.ROI_CASES if c.tier == "exact" and not c.large])
    assert (prow == 0).any() and prow.max() > 64
    assert {int(v) for v in np.unique(prow[prow > 0] % 8)} == set(range(8))
    assert any(n > 64 and n % 64 for n in prow)                       # a partial batch after a full one
    # patch-keyed work mapping
    assert {r["bw"] for r in roi.values()} >= {1, 2}
    assert any(r["BR"] > 8 for r in roi.values()) and any(r["BC"] > 8 for r in roi.values())
    assert any(r["straddles_images"] for r in roi.values())
    # producer
    S = {r["S"] for r in roi.values()}
    assert any(s < 256 for s in S) and 256 in S and any(r["partial_round"] for r in roi.values())
    assert {r["spb"] for r in roi.values()} >= {1, 4, 9, 16}
    assert any(r["spb"] == 4 and r["rounds"] > 1 for r in roi.values())       # a later round with the merge on
    assert any((G.roi_inputs(n).rois[:, 0] < 0).all() for n in ROI)          # all RoIs masked
    assert any(r.get("entries") == 0 for r in roi.values())
