"""Fixtures and buffer-contract cases (tests/guarded.py) of the Circular Smooth Label entry points of
include/jdet_hip_csl.h.  Importable without a GPU; tests/test_csl_cpu.py dry-runs the smallest instances,
tests/test_gpu_csl.py runs every regime.

Conditions the fixtures meet, asserted where they are built:
  * every random target has (a * 180 / pi + 45) / omega at least 1e-3 from an integer in float64 (they are drawn a
    tenth of a bin or more inside their bin), so no float32 evaluation can put it into another bin;
  * EXACT_TARGETS are apart: a = 0 (the quotient 45 / omega, an integer at omega 1), float32-exact values, values whose
    quotient is negative (truncation toward zero, not floor) or beyond the code (the wrap);
  * the forced bins 0, 1, L - 2, L - 1 make every window wrap past both ends of the code;
  * decode rows: the two largest logits of a row are 1e-2 or more apart, or exactly equal (ties, the first wins).

Bound of every output: arithmetic is double and rounded once, so one float32 spacing at the float64 value
(csl_ref.ulp32); no bound comes from the code under test."""
import functools

import numpy as np

from tests import csl_ref as R
from tests import abi_cases
from tests.abi_cases import Case, P, Res, ST

AVG, LOSS_WEIGHT, ALPHA = 7.0, 0.8, 0.25
OMEGA = {2: 90, 45: 4, 64: 2.8, 180: 1}                  # coding_len -> omega
WINDOW_CASES = (("gaussian", 3), ("gaussian", 6), ("triangle", 4), ("rect", 3), ("pulse", 1))
SELECTIONS = ("none", "all", "first", "last", "random")
EXACT_TARGETS = np.array([0.0, 0.25, 0.5, -0.25, -0.75, -0.7890625, -1.0, 2.5], np.float32)
# csrc/csl.hip: kTileRows; its grid cap kSumGridCap = the 4 KiB loss workspace / 8 (double partials); reduce.h's
# kJdetLossGridCap (float partials).  tests/test_csl_cpu.py ties the first two to the source and the workspace query.
TILE_ROWS, SUM_GRID_CAP, REDUCE_GRID_CAP = 64, 512, 1024
WINDOW_ID = {"pulse": 0, "rect": 1, "triangle": 2, "gaussian": 3}


def lib():
    return abi_cases.lib()


def fit_radius(window, radius, L):
    """rect / triangle radii cut to the code (L = 2: radius 1)"""
    return min(radius, L // 2) if window in ("rect", "triangle") else radius


def targets(rng, n, omega):
    """n float32 targets inside their bins, the first ones on the forced bins"""
    L = R.coding_len(omega)
    k = rng.integers(0, L, n)
    forced = np.array([0, 1, L - 2, L - 1]) % L
    k[:min(n, 4)] = forced[:min(n, 4)]
    frac = rng.uniform(0.1, 0.9, n)
    a = (((k + frac) * float(omega) - R.OFFSET) * np.pi / 180.0).astype(np.float32)
    q = R.quotient64(a, omega)
    assert (np.abs(q - np.round(q)) >= 1e-3).all() and np.array_equal(R.bins(a, omega), k)
    return a


def selection(rng, n, mode):
    w = np.zeros(n, np.float32)
    if mode == "all":
        w[:] = rng.uniform(0.5, 2.0, n)                     # a mask, never a factor: any positive value
    elif mode == "first":
        w[0] = 1.0
    elif mode == "last":
        w[-1] = 1.0
    elif mode == "random":
        w[rng.random(n) < 0.01] = 1.0
        w[rng.integers(0, n)] = 1.0
    else:
        assert mode == "none"
    w[(w == 0) & (rng.random(n) < 0.3)] = -1.0               # negative weights are unselected too
    return w


@functools.lru_cache(maxsize=None)
def loss_fixture(rows, L, window, radius, gamma, sel, extreme=False):
    """-> dict(logits (rows, L), target, weight (rows,), ref = (loss64, unit grad64)); shared, never written"""
    omega = OMEGA[L]
    assert R.coding_len(omega) == L
    rng = np.random.default_rng([rows, L, WINDOW_ID[window], int(radius), int(gamma * 2), SELECTIONS.index(sel)])
    x = (rng.standard_normal((rows, L)) * 2.0).astype(np.float32)
    if extreme:
        x[rng.random((rows, L)) < 0.3] = 80.0
        x[rng.random((rows, L)) < 0.3] = -80.0
    a = targets(rng, rows, omega)
    n_exact = min(rows, len(EXACT_TARGETS)) if sel == "all" else 0
    a[rows - n_exact:] = EXACT_TARGETS[:n_exact]
    w = selection(rng, rows, sel)
    ref = R.angle_loss(x, a, w, omega, window, radius, gamma, ALPHA, AVG, LOSS_WEIGHT)
    return dict(logits=x, target=a, weight=w, ref=ref, omega=omega)


def _rows5(col4, hostile, rng):
    """(rows,) -> (rows, 5) with the values in column 4; the other columns are nobody's: NaN in the hostile runs"""
    out = np.full((col4.shape[0], 5), np.nan, np.float32) if hostile else \
        rng.standard_normal((col4.shape[0], 5)).astype(np.float32)
    out[:, 4] = col4
    return out


def window5(arr, total, start):
    """(B, n, 5) placed as the window [:, start:start + n] of a (B, total, 5) array of NaN"""
    full = np.full((arr.shape[0], total, 5), np.nan, np.float32)
    full[:, start:start + arr.shape[1]] = arr
    return full


def loss_case(rows, L, window, radius, gamma, sel, windowed=False, unaligned=False, extreme=False):
    """contract row of jdet_csl_angle_loss_level.  windowed: rows = 2 n, target / weight the windows [:, 7:7 + n] of
    (2, n + 69, 5) arrays whose other rows are NaN; unaligned: logits and gradient one float into their allocations.
    Hostile runs: NaN in the logits and targets of unselected rows and in columns 0..3 of targets and weights."""
    f = loss_fixture(rows, L, window, radius, gamma, sel, extreme)

    def fn(run):
        x, a, w = f["logits"].copy(), f["target"].copy(), f["weight"]
        if run.hostile:
            x[w <= 0] = np.nan
            a[w <= 0] = np.nan
        rng = np.random.default_rng(rows)
        t5, w5 = _rows5(a, run.hostile, rng), _rows5(w, run.hostile, rng)
        n, total, start = rows, rows, 0
        if windowed:
            n = rows // 2
            total, start = n + 69, 7
            t5, w5 = (window5(v.reshape(2, n, 5), total, start) for v in (t5, w5))
        pad = 1 if unaligned else 0
        xin = run.inp("logits", np.concatenate([np.zeros(pad, np.float32), x.reshape(-1)]))
        tin, win = run.inp("target", t5), run.inp("weight", w5)
        avg = run.inp("avg_factor", np.array([AVG], np.float32))
        loss, grad = run.out("loss", (1,)), run.out("grad_logits", (rows * L + pad,))
        ws, wsb = run.ws("workspace", lib().jdet_sigmoid_focal_loss_workspace())
        off = start * 5 * 4
        run.ok(lib().jdet_csl_angle_loss_level(
            P(xin) + 4 * pad, P(tin) + off, n, total, P(win) + off, n, total, rows, L, float(f["omega"]),
            WINDOW_ID[window], float(radius), float(gamma), ALPHA, P(avg), LOSS_WEIGHT, P(loss), P(grad) + 4 * pad, P(ws),
            wsb, ST(xin)), "jdet_csl_angle_loss_level")
        if pad:                                              # the word in front of the unaligned gradient is nobody's
            grad[:1].zero_()
        unit = np.concatenate([np.zeros(pad), f["ref"][1].reshape(-1)])
        return Res({"loss": loss, "grad_logits": grad},
                   lambda: {"loss": (np.array([f["ref"][0]]), R.ulp32(f["ref"][0])), "grad_logits": (unit, R.ulp32(unit))})
    return Case(("jdet_csl_angle_loss_level",), "rows %d L %d %s r %s gamma %g %s%s%s%s" % (
        rows, L, window, radius, gamma, sel, " window" if windowed else "", " unaligned" if unaligned else "",
        " +-80" if extreme else ""), fn)


def encode_case(n, L, window, radius):
    omega = OMEGA[L]
    rng = np.random.default_rng([n, L, WINDOW_ID[window]])
    a = targets(rng, n, omega)
    a[n - min(n, len(EXACT_TARGETS)):] = EXACT_TARGETS[:min(n, len(EXACT_TARGETS))]
    ref = R.labels(R.bins(a, omega), L, window, radius)

    def fn(run):
        ain = run.inp("angle", a)
        out = run.out("labels", (n, L))
        run.ok(lib().jdet_csl_encode(P(ain), n, L, float(omega), WINDOW_ID[window], float(radius), P(out), ST(ain)),
               "jdet_csl_encode")
        return Res({"labels": out}, lambda: {"labels": (ref, R.ulp32(ref))})
    return Case(("jdet_csl_encode",), "n %d L %d %s r %s" % (n, L, window, radius), fn)


def decode_logits(rng, rows, L):
    """(rows, L) logits whose two largest entries per row are >= 1e-2 apart or equal: rows 0.. hold in turn a plain
    maximum, the maximum in the last bin, a tie of two bins, a tie of the first and the last bin, a constant row"""
    x = np.round(rng.standard_normal((rows, L)) * 3.0, 1).astype(np.float32)      # a grid of 0.1: apart or equal
    for r in range(rows):
        kind = r % 5
        top = np.float32(x[r].max() + 1.0)
        if kind == 1:
            x[r, L - 1] = top
        elif kind == 2:
            x[r, rng.choice(L, size=min(2, L), replace=False)] = top
        elif kind == 3:
            x[r, 0] = x[r, L - 1] = top
        elif kind == 4:
            x[r, :] = np.float32(-4.5)
    s = np.sort(x, axis=1)
    gap = s[:, -1] - s[:, -2] if L > 1 else np.ones(rows)
    assert ((gap >= 1e-2) | (gap == 0)).all()
    return x


def decode_case(rows, L, indexed):
    omega = OMEGA[L]
    rng = np.random.default_rng([rows, L, int(indexed)])
    x = decode_logits(rng, rows, L)
    index = rng.permutation(rows)[:max(1, (rows * 2) // 3)].astype(np.int64) if indexed else None
    n = rows if index is None else index.shape[0]
    idx, ang = R.decode(x if index is None else x[index], omega)

    def fn(run):
        xin = run.inp("logits", x)
        iin = run.inp("index", index) if indexed else None
        out = run.out("angle", (n,))
        run.ok(lib().jdet_csl_decode(P(xin), rows, P(iin), n, L, float(omega), P(out), ST(xin)), "jdet_csl_decode")
        return Res({"angle": out}, lambda: {"angle": (ang, R.ulp32(ang))})
    c = Case(("jdet_csl_decode",), "rows %d L %d%s" % (rows, L, " indexed" if indexed else ""), fn)
    c.expected_index, c.omega = idx, omega
    return c


def index_of_angle(angle, omega):
    """the bin an angle of decode's form stands for"""
    return np.rint((np.asarray(angle, np.float64) * 180.0 / np.pi + R.OFFSET) % R.RANGE / float(omega) - 0.5).astype(np.int64)


def smallest_cases():
    """one instance per entry point, for the CPU dry run"""
    return [loss_case(63, 45, "gaussian", 3, 2.0, "random"), loss_case(2 * 37, 2, "rect", 1, 0.0, "all", windowed=True),
            encode_case(9, 45, "triangle", 4), decode_case(7, 64, True), decode_case(7, 2, False)]
