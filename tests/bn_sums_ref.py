"""Float64 restatements of the frozen-BatchNorm / bias / per-channel-sum entries of include/jdet_hip.h, written from the
header's contract and the module semantics (F.batch_norm in eval mode, + residual, ReLU), and the two input families
the GPU tests (tests/test_gpu_bn_sums.py) run them on.  tests/test_bn_sums_cpu.py holds them to float64 autograd.

Conventions
  * tensors are channels-last rows [P][C]; parameters are the float32 arrays the kernel receives, promoted to float64
    before any arithmetic (so the reference sees the very numbers the kernel sees);
  * the ReLU mask of every backward is `y > 0` of the y ARRAY HANDED IN (an input of the ABI), never of a recomputed
    activation: reference and kernel cannot disagree on a near-zero activation.  `subnormal_positive` says what
    `y > 0` answers for a positive subnormal (True in IEEE arithmetic; a device that flushes float32 denormals in
    comparisons answers False) -- the GPU test measures it on the device and passes it in.

Error bounds (u = 2^-24, one float32 rounding).  The device's sqrtf and division are allowed 2 ulp = 4 u each.
  a      = weight * (1 / sqrt(var + eps))            1 (var + eps) + 4 (sqrt) + 4 (1 / .) + 1 (weight * .)   = 10 u
  forward  (x - mean) * rsqrt * weight + bias (+ res)  the header's formula:
           1 (var + eps) + 4 + 4 (rsqrt) + 1 (x - mean) + 1 (* rsqrt) + 1 (* weight) + 1 (+ bias) + 1 (+ res) = 14 u
           of |x a| + |mean a| + |bias| + |res|
  dx     = g * a                                      10 (a) + 1 (g * a)                                     = 11 u
  g * xhat, xhat = (x - mean) * rsqrt                 1 (x - mean) + 9 (rsqrt) + 1 (* rsqrt) + 1 (g * .)     = 12 u
           of |g| (|x| + |mean|) rsqrt
  g * t,   t = y - beta | (y - identity) - beta | own - beta    2 subtractions + 1 product                   =  3 u
           of |g| (|y| + |identity| + |beta|)
  / gamma  in jdet_bn_sums_finish                     4 u of the quotient
A per-channel sum over a chain of at most L additions adds L u sum|terms| (chain_length below)."""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
K_A, K_FWD, K_DX, K_GXHAT, K_GT, K_DIV = 10, 14, 11, 12, 3, 4
SUBNORMAL = np.float32(2.0 ** -149)          # the smallest positive float32
MIN_NORMAL = np.float32(2.0 ** -126)
LATTICE_LIMIT = 2 ** 24


# ---- the operations ------------------------------------------------------------------------------------------------------
def constants(C, weight, bias, mean, var, eps):
    """(w, b, mean, invstd, a, sh) in float64 from the float32 parameters; weight / bias None = 1 / 0"""
    for p in (weight, bias, mean, var):
        assert p is None or (p.dtype == F32 and p.shape == (C,))
    w = np.ones(C, F64) if weight is None else weight.astype(F64)
    b = np.zeros(C, F64) if bias is None else bias.astype(F64)
    m = mean.astype(F64)
    invstd = 1.0 / np.sqrt(var.astype(F64) + F64(F32(eps)))
    a = w * invstd
    return w, b, m, invstd, a, b - m * a


def relu_mask(y, subnormal_positive=True):
    """[y > 0] of the float32 array handed to the kernel"""
    assert y.dtype == F32
    return y > 0 if subnormal_positive else y >= MIN_NORMAL


def forward(x, residual, weight, bias, mean, var, eps, relu):
    """y and the sum of the magnitudes of its terms (for the bound K_FWD * U * mag)"""
    _, b, m, _, a, _ = constants(x.shape[1], weight, bias, mean, var, eps)
    x64 = x.astype(F64)
    y = (x64 - m) * a + b
    mag = (np.abs(x64) + np.abs(m)) * np.abs(a) + np.abs(b)
    if residual is not None:
        y = y + residual.astype(F64)
        mag = mag + np.abs(residual.astype(F64))
    if relu:
        y = np.maximum(y, 0.0)
    return y, mag


def backward_from_x(dy, y, x, weight, bias, mean, var, eps, relu, subnormal_positive=True):
    """dict: dx, dres (= the masked gradient), dgamma, dbeta and the magnitude sums dx_mag (elements), dbeta_mag,
    dgamma_mag (channels)"""
    _, _, m, invstd, a, _ = constants(dy.shape[1], weight, bias, mean, var, eps)
    g = dy.astype(F64)
    if relu:
        g = g * relu_mask(y, subnormal_positive)
    out = {"dx": g * a, "dres": g, "dbeta": g.sum(0), "dbeta_mag": np.abs(g).sum(0)}
    out["dx_mag"] = np.abs(out["dx"])
    if x is not None:
        x64 = x.astype(F64)
        out["dgamma"] = (g * ((x64 - m) * invstd)).sum(0)
        out["dgamma_mag"] = (np.abs(g) * ((np.abs(x64) + np.abs(m)) * invstd)).sum(0)
    return out


def backward_from_output(dy, y, identity, own_output, weight, bias, mean, var, eps, subnormal_positive=True):
    """the three forms of jdet_bn_act_backward_from_output: dc, the two sums S0 = sum g, S1 = sum g t and what
    jdet_bn_sums_finish makes of them: dbeta = S0, dgamma = S1 / gamma"""
    assert identity is None or own_output is None
    w, b, _, _, a, _ = constants(dy.shape[1], weight, bias, mean, var, eps)
    g = dy.astype(F64) * relu_mask(y, subnormal_positive)
    y64 = y.astype(F64)
    if own_output is not None:
        t, tmag = own_output.astype(F64) - b, np.abs(own_output.astype(F64)) + np.abs(b)
    elif identity is not None:
        t, tmag = y64 - identity.astype(F64) - b, np.abs(y64) + np.abs(identity.astype(F64)) + np.abs(b)
    else:
        t, tmag = y64 - b, np.abs(y64) + np.abs(b)
    s1 = (g * t).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        dgamma = s1 / w
    return {"dc": g * a, "dc_mag": np.abs(g * a), "s0": g.sum(0), "s1": s1, "dbeta": g.sum(0), "dgamma": dgamma,
            "s0_mag": np.abs(g).sum(0), "s1_mag": (np.abs(g) * tmag).sum(0), "gamma": w}


def bias_act_backward(dy, y, relu, subnormal_positive=True):
    g = dy.astype(F64)
    if relu:
        g = g * relu_mask(y, subnormal_positive)
    return {"grad_pre": g, "grad_bias": g.sum(0), "grad_bias_mag": np.abs(g).sum(0)}


def column_sums(partial, gamma=None):
    """jdet_bn_sums_finish of a [rows][2][C] float32 array: (grad_beta, grad_gamma, |.| sums of both halves)"""
    assert partial.ndim == 3 and partial.shape[1] == 2
    p = partial.astype(F64)
    s0, s1 = p[:, 0].sum(0), p[:, 1].sum(0)
    m0, m1 = np.abs(p[:, 0]).sum(0), np.abs(p[:, 1]).sum(0)
    if gamma is None:
        return s0, s1, m0, m1
    with np.errstate(divide="ignore", invalid="ignore"):
        return s0, s1 / gamma.astype(F64), m0, m1 / np.abs(gamma.astype(F64))


def chain_length(P, rows):
    """upper bound on the number of additions any addend of a channel passes through in a two-stage per-channel sum that
    wrote `rows` partial rows for P tensor rows.  First stage: the workgroups share the P rows evenly to within one pass
    of a workgroup, and a workgroup has at most 1024 threads, so a partial row holds at most ceil(P / rows) + 1024
    addends of a channel, summed in some order.  Second stage: 32 row groups, each a serial sum of ceil(rows / 32)
    partial rows, then the 32 group sums."""
    rows = max(int(rows), 1)
    return -(-int(P) // rows) + 1024 + finish_chain_length(rows)


def finish_chain_length(rows):
    return -(-int(rows) // 32) + 32


# ---- inputs --------------------------------------------------------------------------------------------------------------
def channel_pattern(C):
    """a non-zero integer in {-3..3} per channel that depends on c % 7 and on c // 4: neighbouring channels, channels a
    quad apart and channels 7 apart all differ, so the sums of two channels a thread could confuse differ too"""
    c = np.arange(C)
    mag = (c % 7 + 2 * (c // 4)) % 3 + 1
    sign = np.where((c % 7 + c // 4) % 2 == 0, 1, -1)
    return (mag * sign).astype(F64)


def lattice_params(C):
    """gamma in {+-0.5, +-1, +-2}, beta in {+-1, +-2} (never 0: y - beta then absorbs a subnormal y in float32 and in
    float64 alike), mean an integer in [-2, 2], var = 0.25 with eps = 0: 1 / sqrt is exactly 2"""
    c = np.arange(C)
    gamma = np.array([0.5, -1.0, 2.0, -0.5, 1.0, -2.0])[(c % 7 + c // 4) % 6]
    beta = np.array([1.0, -2.0, 2.0, -1.0])[(c % 7 + 3 * (c // 4)) % 4]
    mean = ((c % 7 + c // 4) % 5 - 2).astype(F64)
    return gamma.astype(F32), beta.astype(F32), mean.astype(F32), np.full(C, 0.25, F32), 0.0


def plant(y, dy, P, C):
    """exact 0.0, -0.0 and the smallest positive subnormal in y at known positions spread over the first, a middle and
    the last rows (the last row lies in the scalar tail of a grid-stride loop), with a non-zero gradient above each.
    Returns {kind: (rows, cols)}."""
    rows = np.array(sorted({0, P // 3, P - 1}))
    where = {}
    for k, (kind, val) in enumerate((("zero", F32(0.0)), ("negzero", F32(-0.0)), ("subnormal", SUBNORMAL))):
        cols = (np.array([1, 2, 3]) * (k + 2) + rows) % C
        y[rows, cols] = val
        dy[rows, cols] = np.where(dy[rows, cols] == 0, F32(1.0), dy[rows, cols])
        where[kind] = (rows, cols)
    return where


def lattice_inputs(P, C, seed=0):
    """dy, x, y, residual, identity, own_output: small integers (|v| <= 3); dy = a value of {-1, 0, 1} times the channel
    pattern.  y (an input of the backward entries) carries the planted zeros / subnormal; elsewhere it is an integer,
    negative or zero on about 40 % of the elements."""
    rng = np.random.default_rng(1000 + seed)
    pat = channel_pattern(C)
    dy = (rng.integers(-1, 2, (P, C)) * pat).astype(F32)
    x = rng.integers(-3, 4, (P, C)).astype(F32)
    y = rng.integers(-2, 4, (P, C)).astype(F32)
    res = rng.integers(-3, 4, (P, C)).astype(F32)
    idn = rng.integers(-3, 4, (P, C)).astype(F32)
    own = rng.integers(-3, 4, (P, C)).astype(F32)
    planted = plant(y, dy, P, C)
    return {"dy": dy, "x": x, "y": y, "residual": res, "identity": idn, "own_output": own, "planted": planted,
            "params": lattice_params(C)}


def normal_params(C, seed=0):
    rng = np.random.default_rng(2000 + seed)
    gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(F32)
    return gamma, rng.normal(size=C).astype(F32), rng.normal(size=C).astype(F32), rng.uniform(0.5, 2.0, C).astype(F32), 1e-5


def normal_inputs(P, C, seed=0):
    rng = np.random.default_rng(3000 + seed)
    t = {k: rng.standard_normal((P, C), dtype=F32) for k in ("dy", "x", "y", "residual", "identity", "own_output")}
    t["planted"] = plant(t["y"], t["dy"], P, C)
    t["params"] = normal_params(C, seed)
    return t


def lattice_sum_magnitudes(t):
    """the largest sum of |terms| of any per-channel sum the entries form on lattice inputs `t`, the ReLU mask taken as
    all ones (an upper bound of every masked sum): below 2^24 every partial sum, in any order, is an exactly
    representable integer"""
    _, b, m, invstd, _, _ = constants(t["dy"].shape[1], *t["params"])
    g = np.abs(t["dy"].astype(F64))
    ab = lambda k: np.abs(t[k].astype(F64))
    sums = [g.sum(0), (g * ((ab("x") + np.abs(m)) * invstd)).sum(0),
            (g * (ab("y") + ab("identity") + np.abs(b))).sum(0), (g * (ab("own_output") + np.abs(b))).sum(0)]
    return float(max(s.max() for s in sums))


# the (C, P) of every per-channel sum the GPU tests run; the CPU test asserts the lattice limit for each
SUM_SHAPES = ((64, 83333), (2048, 2605), (1536, 2605), (256, 20011))
