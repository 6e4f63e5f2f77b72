"""Float64 restatements of Circular Smooth Label for tests/test_csl_cpu.py and tests/test_gpu_csl.py: the rules of
include/jdet_hip_csl.h written a second time, with numpy, from the rule text and not from the kernels' closed forms.

  bins      float32, the reference's operation order, truncation toward zero, floor-mod;
  labels    the window's offset table scattered bin by bin, THE LARGEST VALUE kept where offsets meet (np.maximum), in
            double -- no circular-distance formula here; tests/test_csl_cpu.py checks that formula against this;
  loss      per selected row and bin, in double; sigmoid and 1 - sigmoid both from exp(-|x|) so that neither cancels;
  gradient  the analytic derivative;
  decode    first index of the row maximum of the logits.

gamma, alpha, avg_factor and loss_weight enter as the float32 nearest to what the caller passes (the C ABI takes floats);
omega and radius as doubles, omega rounded to float32 where the rule says float32 (the bin)."""
import numpy as np

RANGE, OFFSET = 180, 45
DEG32 = np.float32(180.0 / np.pi)
WINDOWS = ("pulse", "rect", "triangle", "gaussian")
TINY = 1.1754944e-38            # the smallest normal float32


def coding_len(omega):
    return int(RANGE // omega)


def quotient64(a, omega):
    """(a * 180 / pi + 45) / omega in float64: how far a target is from a bin edge"""
    return (np.asarray(a, np.float64) * (180.0 / np.pi) + OFFSET) / float(omega)


def bins(a, omega):
    """targets (n,) -> int64 bins in [0, L)"""
    a = np.asarray(a, np.float32)
    v = ((a * DEG32).astype(np.float32) + np.float32(OFFSET)).astype(np.float32) / np.float32(omega)
    assert v.dtype == np.float32
    return np.trunc(v).astype(np.int64) % coding_len(omega)


def window_table(window, radius):
    """(offsets b, values) of the rule's table, values in double"""
    if window == "pulse":
        return np.array([0]), np.array([1.0])
    if window in ("rect", "triangle"):
        b = np.arange(-int(radius), int(radius))
        return b, np.ones(b.shape) if window == "rect" else 1.0 - np.abs(b) / float(radius)
    assert window == "gaussian"
    b = np.arange(-RANGE // 2, RANGE // 2)
    return b, np.exp(-(b.astype(np.float64) ** 2) / (2.0 * float(radius) ** 2))


def labels(t, L, window, radius):
    """target bins (n,) -> (n, L) double labels: the table written offset by offset, the largest value winning"""
    t = np.asarray(t, np.int64)
    y = np.zeros((t.shape[0], L))
    rows = np.arange(t.shape[0])
    for b, v in zip(*window_table(window, radius)):
        j = (t + b) % L
        y[rows, j] = np.maximum(y[rows, j], v)
    return y


def circular_labels(t, L, radius):
    """the closed form of the gaussian window: exp(-d^2 / (2 r^2)) of the circular bin distance"""
    d = (np.arange(L)[None, :] - np.asarray(t, np.int64)[:, None]) % L
    d = np.minimum(d, L - d).astype(np.float64)
    return np.exp(-(d * d) / (2.0 * float(radius) ** 2))


def elementwise(x, y, gamma, alpha):
    """(loss, d loss / d x) per element in double"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    gamma, alpha = float(np.float32(gamma)), float(np.float32(alpha))
    e = np.exp(-np.abs(x))
    p = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    q = np.where(x >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    bce = np.maximum(x, 0.0) - x * y + np.log1p(e)
    pt = q * y + p * (1.0 - y)
    aw = alpha * y + (1.0 - alpha) * (1.0 - y)
    if gamma == 0.0:
        ptg, first = np.ones_like(pt), np.zeros_like(pt)
    else:
        ptg = pt ** gamma
        first = gamma * pt ** (gamma - 1.0) * p * q * (1.0 - 2.0 * y) * bce
    return bce * aw * ptg, aw * (first + ptg * (p * (1.0 - y) - q * y))


def angle_loss(x, target, weight, omega, window, radius, gamma, alpha, avg_factor, loss_weight):
    """logits (rows, L), target / weight (rows,) = column 4 of the level's windows -> (loss, unit gradient (rows, L)):
    loss = loss_weight * sum / avg_factor, unit gradient = d sum / d logits.  Unselected rows are not looked at."""
    L = coding_len(omega)
    sel = np.asarray(weight) > 0
    grad = np.zeros(np.asarray(x).shape)
    if not sel.any():
        return 0.0, grad
    y = labels(bins(np.asarray(target)[sel], omega), L, window, radius)
    l, g = elementwise(np.asarray(x)[sel], y, gamma, alpha)
    grad[sel] = g
    return float(l.sum() / float(np.float32(avg_factor)) * float(np.float32(loss_weight))), grad


def decode(logits, omega):
    """-> (first argmax (n,), angle (n,) in double)"""
    idx = np.argmax(np.asarray(logits), axis=1)
    return idx, (((idx + 0.5) * float(omega)) % RANGE - OFFSET) * np.pi / 180.0


def ulp32(ref):
    """the bound of 'double arithmetic rounded once': one float32 spacing at |ref|, 1.2e-38 below the normal range"""
    r = np.abs(np.asarray(ref, np.float64))
    with np.errstate(over="ignore"):
        s = np.spacing(r.astype(np.float32)).astype(np.float64)
    return np.where(r < TINY, 1.2e-38, s)
