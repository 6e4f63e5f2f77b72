"""The float32 order emulation of tests/sum_order_ref.py, on the host: every emulated sum lies within the bound that
tests/dense_loss_ref.py / tests/bn_sums_ref.py state for the kernel it mirrors (so it is a sum of the right addends),
and on the inputs the GPU pins use it DIFFERS in bits from numpy's float32 sum (so those inputs exercise the order: a
kernel that added in another order would not match it)."""
import numpy as np
import pytest

from tests import bn_sums_ref as B
from tests import dense_loss_ref as D
from tests import sum_order_ref as S

F32, F64 = np.float32, np.float64


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def _differs(emulated, addends, axis=None):
    return (_bits(emulated) != _bits(np.sum(addends, axis=axis, dtype=F32))).any()


def test_butterfly_and_block_sum_are_plain_sums_on_integers():
    rng = np.random.default_rng(1)
    acc = rng.integers(-1000, 1001, (3, 256)).astype(F32)
    assert (S.block_sum4(acc) == acc.astype(F64).sum(1)).all()
    assert S.loss_grid(1) == 1 and S.loss_grid(1024) == 1 and S.loss_grid(1025) == 2 and S.loss_grid(1 << 30) == 1024
    v = rng.integers(-1000, 1001, 700000).astype(F32)
    total, partial = S.loss_tree(v)
    assert total == v.astype(F64).sum() and partial.size == 684


@pytest.mark.parametrize("n", S.L1_SIZES + S.L1_LEVEL_SIZES)
def test_loss_tree(n):
    pred, target, weight, total, partial = S.l1_case(n)
    terms, _, tb, _ = D.smooth_l1_terms(pred, target, weight, 0.0)
    assert partial.size == S.loss_grid(n)
    bound = tb.sum() + D.sum_chain_length(n, partial.size) * D.U * np.abs(terms).sum()
    assert abs(float(total) - terms.sum()) <= bound
    if n > 1:
        assert _differs(total, S.l1_terms(pred, target, weight))
    scaled = S.level_scale(total, S.AVG, S.LOSS_WEIGHT)
    ref = D.level_loss(float(total), S.AVG, S.LOSS_WEIGHT)
    assert abs(float(scaled) - ref) <= D.K_LEVEL * D.U * abs(ref)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("C,P", S.BIAS_SHAPES)
def test_bias_tree(C, P, relu):
    dy, y, grad_bias, part = S.bias_case(C, P, relu)
    ref = B.bias_act_backward(dy, y, relu)
    assert part.shape == (256, C)
    assert (np.abs(grad_bias - ref["grad_bias"]) <= B.chain_length(P, part.shape[0]) * B.U * ref["grad_bias_mag"]).all()
    assert _differs(grad_bias, S.masked(dy, y) if relu else dy, axis=0)


@pytest.mark.parametrize("C,P", S.CHANNEL_SUM_SHAPES)
def test_channel_sum_tree(C, P):
    x, sums, part = S.channel_sum_case(C, P)
    assert part.shape[0] == {333: 1 if C == 5 else 21, 70001: 256}[P]
    x64 = x.astype(F64)
    assert (np.abs(sums - x64.sum(0)) <= B.chain_length(P, part.shape[0]) * B.U * np.abs(x64).sum(0)).all()
    assert _differs(sums, x, axis=0)


@pytest.mark.parametrize("C,P", S.BN_SHAPES)
def test_frozen_bn_tree(C, P):
    dy, y, x, grad_bias, grad_weight, rows = S.frozen_bn_case(C, P)
    assert rows == (256 if C == 64 else 512)
    one, zero = np.ones(C, F32), np.zeros(C, F32)
    ref = B.backward_from_x(dy, y, x, one, zero, zero, one, 0.0, 1)
    chain = B.chain_length(P, rows)
    assert (np.abs(grad_bias - ref["dbeta"]) <= chain * B.U * ref["dbeta_mag"]).all()
    assert (np.abs(grad_weight - ref["dgamma"]) <= (chain + B.K_GXHAT) * B.U * ref["dgamma_mag"]).all()
    g = S.masked(dy, y)
    assert _differs(grad_bias, g, axis=0) and _differs(grad_weight, g * x, axis=0)


@pytest.mark.parametrize("C", S.FINISH_CS)
@pytest.mark.parametrize("rows", S.FINISH_ROWS)
def test_bn_sums_finish_tree(rows, C):
    part, gamma, grad_beta, grad_gamma, grad_gamma_plain = S.finish_case(rows, C)
    chain = B.finish_chain_length(rows)
    s0, s1, m0, m1 = B.column_sums(part, gamma)
    assert (np.abs(grad_beta - s0) <= chain * B.U * m0).all()
    assert (np.abs(grad_gamma - s1) <= chain * B.U * m1 + B.K_DIV * B.U * np.abs(s1)).all()
    _, s1p, _, m1p = B.column_sums(part)
    assert (np.abs(grad_gamma_plain - s1p) <= chain * B.U * m1p).all()
    if rows == 0:
        assert not grad_beta.any() and not grad_gamma.any()
    if rows >= 97:              # up to 32 rows every row group holds one row and the sum is the plain serial one
        assert _differs(grad_beta, part[:, 0], axis=0) and _differs(grad_gamma_plain, part[:, 1], axis=0)
    # the two second stages add in different orders once a row group holds more than five rows: the eight-in-flight
    # tree of sums_finish_kernel is another sum
    if rows == 512:
        assert (_bits(S.sums_finish(part[:, 0])) != _bits(grad_beta)).any()
