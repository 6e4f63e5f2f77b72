"""Restatements of the localization-distillation terms for tests/test_ld_cpu.py and tests/test_gpu_ld.py: `integral`,
the weighted L1 / smooth-L1 on it and the knowledge-distillation KL divergence, each with torch on the CPU at float64
(the reference) and at float32 (the yardstick of the bounds: every bound of the GPU tests is 4 x the float32
restatement's error against the float64 one).

What the float64 side shares with every float32 implementation, because the C ABI takes them as floats: the bin values
e_k = lo + k * ((hi - lo) / R) EVALUATED IN FP32 (include/jdet_hip.h; exact at R = 8), beta, avg_factor, loss_weight
and T as the float32 nearest to what the caller passes.

Fixtures are seeded and cached; the arrays they return are shared and must not be written.  Conditions they meet by
construction, so that no bound is vacuous or unreachable:
  L1 sign     target = E64 +- U(0.05, 1.5) (and | |E64 - t| - beta | >= 1e-3): sign(E - t) and the smooth-L1 branch
              cannot differ between precisions;
  KL range    max - min of a row's logits / T is at most 60: no float32 softmax term underflows, t log t stays finite;
  reachable   a float32 result cannot be expected closer to the float64 value than the spacing of float32 there, and
              the gradients leave the level nodes through float32 steps (the unit gradient's rounding, then
              jdet_loss_grad_scale's (grad_out * loss_weight) / avg_factor and its product: 2^-24 each).  A seed whose
              4 x float32 error is below ONE float32 spacing of the loss, or below 4 * 2^-24 of the largest gradient,
              is skipped for the next seed (+ 1000): such a bound would measure the luck of one summation order, not
              an implementation.  The rule looks at the two restatements only."""
import functools

import numpy as np
import torch

ENDS, ANGLE_ENDS = (-2.0, 2.0), (-5.0, 2.0)


def bins(R, ends):
    """e_k, k = 0 .. R, evaluated in fp32 -> float32 array"""
    lo, hi = np.float32(ends[0]), np.float32(ends[1])
    step = np.float32((hi - lo) / np.float32(R))
    return (lo + np.arange(R + 1, dtype=np.float32) * step).astype(np.float32)


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def integral(logits, R, dtype=torch.float64):
    """(rows, 5 * (R + 1)) -> (rows, 5) torch tensor of `dtype`; differentiable when logits is a tensor"""
    x = logits if torch.is_tensor(logits) else _t(logits, dtype)
    y = torch.softmax(x.reshape(-1, 5, R + 1), dim=2)
    e = torch.stack([_t(bins(R, ENDS), x.dtype)] * 4 + [_t(bins(R, ANGLE_ENDS), x.dtype)])
    return (y * e).sum(dim=2)


def bbox_loss(logits, target, weight, R, beta, avg_factor, loss_weight, dtype):
    """(loss, d loss / d logits) as python float / numpy float64, computed at `dtype`"""
    x = _t(logits, dtype).requires_grad_(True)
    t, w = _t(target, dtype).reshape(-1, 5), _t(weight, dtype).reshape(-1, 5)
    b = float(np.float32(beta))
    d = torch.abs(integral(x, R) - t)
    l = torch.where(d < b, 0.5 * d * d / b, d - 0.5 * b) if b != 0 else d
    loss = (l * w).sum() / float(np.float32(avg_factor)) * float(np.float32(loss_weight))
    loss.backward()
    return float(loss.detach().double()), x.grad.double().numpy()


def kl_loss(pred, soft, weight, T, loss_weight, dtype):
    """knowledge_distillation_kl_div_loss (models/losses/kd_loss.py:L7-39 of the reference) * loss_weight, as written
    there -- boolean compaction, softmax(.).log(), KLDivLoss's mean over all elements -- at `dtype`.
    -> (loss, d loss / d pred (zero rows where unselected), count)"""
    x = _t(pred, dtype).requires_grad_(True)
    s = _t(soft, dtype)
    T = float(np.float32(T))
    p, q = x, s
    count = x.shape[0]
    if weight is not None:
        pos = torch.from_numpy(np.asarray(weight).reshape(-1) > 0)
        if int(pos.sum()) > 0:
            p, q = x[pos], s[pos]
            count = int(pos.sum())
    target = torch.softmax(q / T, dim=1)
    logp = torch.softmax(p / T, dim=1).log()
    loss = (target * (target.log() - logp)).mean() * (T * T) * float(np.float32(loss_weight))
    loss.backward()
    return float(loss.detach().double()), x.grad.double().numpy(), count


def errors(r32, r64):
    """(|loss32 - loss64|, max |g32 - g64| / max |g64|)"""
    return abs(r32[0] - r64[0]), float(np.abs(r32[1] - r64[1]).max() / np.abs(r64[1]).max())


def grad_error(g, g64):
    return float(np.abs(np.asarray(g, np.float64) - g64).max() / np.abs(g64).max())


def _reachable(e_loss, e_grad, loss64):
    return 4 * e_loss >= float(np.spacing(np.float32(abs(loss64)))) and 4 * e_grad >= 4 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ fixtures
AVG, LOSS_WEIGHT = 7.0, 1.5


@functools.lru_cache(maxsize=None)
def bbox_fixture(rows, R, beta, wmode, seed=0):
    """-> dict(logits (rows, 5 (R + 1)), target, weight (rows, 5), ref = (loss64, grad64), e_loss, e_grad).
    wmode: 'ones' | 'mixed' (about a fifth of the rows positive, some sides of them zero) | 'last' (the last row only)"""
    while True:
        rng = np.random.default_rng([rows, R, int(beta * 1e6), seed])
        logits = (rng.standard_normal((rows, 5 * (R + 1))) * 2.0).astype(np.float32)
        E = integral(logits, R).numpy()
        off = rng.uniform(0.05, 1.5, (rows, 5))
        off = np.where(np.abs(off - beta) < 1e-3, off + 2e-3, off)
        target = (E + off * rng.choice([-1.0, 1.0], (rows, 5))).astype(np.float32)
        if wmode == "ones":
            weight = np.ones((rows, 5), np.float32)
        elif wmode == "last":
            weight = np.zeros((rows, 5), np.float32)
            weight[-1] = 1.0
        else:
            weight = (rng.random((rows, 1)) < 0.2).astype(np.float32) * (rng.random((rows, 5)) < 0.8)
            weight[-1] = 1.0
            weight = weight.astype(np.float32)
        r64 = bbox_loss(logits, target, weight, R, beta, AVG, LOSS_WEIGHT, torch.float64)
        r32 = bbox_loss(logits, target, weight, R, beta, AVG, LOSS_WEIGHT, torch.float32)
        e_loss, e_grad = errors(r32, r64)
        if _reachable(e_loss, e_grad, r64[0]):
            return dict(logits=logits, target=target, weight=weight, ref=r64, e_loss=e_loss, e_grad=e_grad, seed=seed)
        seed += 1000


def kl_weight(M, wmode, rng):
    if wmode == "null":
        return None
    if wmode == "zero":
        return np.zeros((M,), np.float32)
    if wmode == "last":
        w = np.zeros((M,), np.float32)
        w[-1] = 1.0
        return w
    w = np.where(rng.random(M) < 0.3, rng.uniform(0.5, 2.0, M), 0.0).astype(np.float32)   # 'mixed'
    w[0] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def kl_fixture(M, K, T, wmode, seed=0, spread=None):
    """-> dict(pred, soft (M, K), weight (M,) | None, ref = (loss64, grad64, count), e_loss, e_grad).  The logits are
    normal with deviation 2 T, clipped so that max - min of z / T stays below 60; `spread`: one row pair spans it."""
    while True:
        rng = np.random.default_rng([M, K, int(T), seed])
        pred = np.clip(rng.standard_normal((M, K)) * 2.0 * T, -29.0 * T, 29.0 * T).astype(np.float32)
        soft = np.clip(rng.standard_normal((M, K)) * 2.0 * T, -29.0 * T, 29.0 * T).astype(np.float32)
        weight = kl_weight(M, wmode, rng)
        if spread is not None:
            pred[-1, 0], pred[-1, -1] = spread * T / 2, -spread * T / 2
            soft[-1, 0], soft[-1, -1] = -spread * T / 2, spread * T / 2
            if weight is not None:
                weight[-1] = 1.0
            return dict(pred=pred, soft=soft, weight=weight)
        assert max(np.ptp(pred, axis=1).max(), np.ptp(soft, axis=1).max()) / T <= 60
        r64 = kl_loss(pred, soft, weight, T, LOSS_WEIGHT, torch.float64)
        r32 = kl_loss(pred, soft, weight, T, LOSS_WEIGHT, torch.float32)
        e_loss, e_grad = errors(r32, r64)
        if _reachable(e_loss, e_grad, r64[0]):
            return dict(pred=pred, soft=soft, weight=weight, ref=r64, e_loss=e_loss, e_grad=e_grad, seed=seed)
        seed += 1000


def window(arr, total, start):
    """`arr` (B, n, ...) placed as the window [:, start:start + n] of a (B, total, ...) array of NaN"""
    full = np.full((arr.shape[0], total) + arr.shape[2:], np.nan, np.float32)
    full[:, start:start + arr.shape[1]] = arr
    return full
