"""No GPU: the float64 restatements of tests/dense_loss_ref.py.

  * focal terms and gradient agree with torch float64 autograd of the package's tensor chain
    (models/losses/focal_loss.py: sigmoid_focal_loss), alpha on and off, weight on and off, gamma 2 and 1.5, and stay
    finite and right at logits of +-40 / +-100 where the chain's 1 - p_t cancels;
  * smooth-L1 / L1 terms and gradient agree with float64 autograd of models/losses/smooth_l1_loss.py away from the kink,
    and take the branches the header states at differences of exactly 0, +-beta and one float32 step to either side;
  * the level scaling and jdet_loss_grad_scale are the autograd of (sum / avg_factor) * loss_weight;
  * the blocked row index is the window [:, s:e] of an (N, A) array;
  * the focal yardstick: the float32 tensor chain's normalised error on the inputs of the GPU test, printed here and
    held inside a sanity band (a float32 chain cannot be better than half an ulp nor worse than a few hundred)."""
import numpy as np
import pytest
import torch

from tests import dense_loss_ref as R

F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("alpha", [0.25, -1.0])
@pytest.mark.parametrize("gamma", [2.0, 1.5])
@pytest.mark.parametrize("with_weight", [True, False])
@pytest.mark.parametrize("M,C", [(37, 15), (37, 1), (2000, 15)])
def test_focal_reference_equals_float64_autograd(M, C, with_weight, gamma, alpha):
    from jdet_amd.models.losses.focal_loss import sigmoid_focal_loss
    logits, labels, weight = R.focal_case(M, C, seed=M + C, with_weight=with_weight)
    assert set(R.EXTREME_LOGITS) <= set(np.unique(logits).tolist()) and labels[0] == 0 and labels[1] == C
    x = torch.from_numpy(logits.astype(F64)).requires_grad_(True)
    w = None if weight is None else torch.from_numpy(weight.astype(F64))
    loss = sigmoid_focal_loss(x, torch.from_numpy(labels), w, alpha=alpha, gamma=gamma, reduction="none")
    loss.sum().backward()
    terms, grad, aw = R.focal_terms(logits, labels, weight, alpha, gamma)
    assert np.isfinite(terms).all() and np.isfinite(grad).all() and (terms >= 0).all()
    # the float64 chain itself loses q = 1 - p_t below 1e-16 (|x| >= 40): absolute agreement there, relative elsewhere
    assert np.abs(loss.detach().numpy() - terms).max() <= 1e-12
    assert np.abs(x.grad.numpy() - grad).max() <= 1e-12
    mild = np.abs(logits) < 20
    assert np.allclose(loss.detach().numpy()[mild], terms[mild], rtol=1e-9, atol=1e-300)
    assert np.allclose(x.grad.numpy()[mild], grad[mild], rtol=1e-9, atol=1e-300)
    if weight is not None:
        assert (terms[weight == 0] == 0).all() and (grad[weight == 0] == 0).all()


def test_focal_reference_at_extreme_logits():
    x = np.array([[100.0, -100.0, 40.0, -40.0]], F32).T.copy()          # C = 1
    for label, want_loss, want_grad in ((1, [0.0, 100.0, 0.0, 40.0], [0.0, -1.0, 0.0, -1.0]),
                                        (0, [100.0, 0.0, 40.0, 0.0], [1.0, 0.0, 1.0, 0.0])):
        terms, grad, _ = R.focal_terms(x, np.full(4, label, np.int32), None, -1.0, 2.0)
        # the gradient of ce q^2 at |x| = 40 and 100 with q -> 1 is -+(1 + 2 p_t ce) = -+1 to 1e-15
        assert np.allclose(terms[:, 0], want_loss, rtol=0, atol=1e-15) and np.allclose(grad[:, 0], want_grad, rtol=0, atol=1e-14)


@pytest.mark.parametrize("beta", [0.0, 1.0 / 9.0, 1.0])
def test_smooth_l1_reference(beta):
    from jdet_amd.models.losses.smooth_l1_loss import l1_loss, smooth_l1_loss
    pred, target, weight = R.smooth_l1_case(3001, beta, seed=3)
    b32 = float(F32(beta))
    terms, grad, tb, gb = R.smooth_l1_terms(pred, target, weight, beta)
    p = torch.from_numpy(pred.astype(F64)).requires_grad_(True)
    t, w = torch.from_numpy(target.astype(F64))[:, None], torch.from_numpy(weight.astype(F64))[:, None]
    loss = smooth_l1_loss(p[:, None], t, w, beta=b32, reduction="sum") if beta else l1_loss(p[:, None], t, w, reduction="sum")
    loss.backward()
    assert abs(float(loss.detach()) - terms.sum()) <= 1e-12 * terms.sum()
    away = np.abs(np.abs(pred.astype(F64) - target) - b32) > 1e-6          # autograd of the flag form at the kink is its own matter
    away &= (pred != target)
    assert np.abs(p.grad.numpy() - grad)[away].max() <= 1e-12
    assert (tb >= 0).all() and (gb >= 0).all()
    d = pred[:7].astype(F64)                                               # the planted differences (target 0, weight 1)
    assert d[0] == 0 and terms[0] == 0 and grad[0] == 0
    if beta:
        up, dn = float(np.nextafter(F32(beta), F32(np.inf))), float(np.nextafter(F32(beta), F32(0)))
        assert d[1:4].tolist() == [b32, up, dn] and d[4:7].tolist() == [-b32, -up, -dn]
        assert terms[1] == 0.5 * b32 and grad[1] == 1.0 and grad[4] == -1.0          # |d| == beta: the linear branch
        assert terms[2] == up - 0.5 * b32 and grad[2] == 1.0
        assert terms[3] == 0.5 * dn * dn / b32 and grad[3] == dn / b32 and grad[6] == -dn / b32


def test_l1_lattice_sum_is_exact():
    for n in (1, 1050005):
        pred, target, weight = R.smooth_l1_case(n, 0.0, seed=1, lattice=True)
        terms, grad, tb, gb = R.smooth_l1_terms(pred, target, weight, 0.0)
        assert (terms == np.round(terms)).all() and terms.sum() < 2 ** 24 and 9 * n < 2 ** 24 + 9 * 2 ** 20
        assert float(np.add.reduce((np.abs(pred - target) * weight), dtype=F32)) == terms.sum()


def test_level_scaling_and_grad_scale_are_the_autograd_of_the_node():
    rng = np.random.default_rng(0)
    unit = rng.standard_normal(50).astype(F32)
    x = torch.from_numpy(unit.astype(F64)).requires_grad_(True)
    avg, lw, go = 37.5, 0.75, 1.25
    node = ((x * x).sum() * 0.5 / avg) * lw              # a loss whose unit gradient is x
    node.backward(torch.tensor(go, dtype=torch.float64))
    assert np.allclose(x.grad.numpy(), R.grad_scale(unit, go, avg, lw), rtol=1e-14, atol=0)
    assert abs(R.level_loss(float((x * x).sum().detach() * 0.5), avg, lw) - float(node.detach())) <= 1e-14 * float(node.detach())


def test_blocked_rows_is_a_column_window():
    N, A, s, e = 3, 50, 7, 19
    a = np.arange(N * A).reshape(N, A)
    idx = R.blocked_rows(N * (e - s), e - s, A)
    assert (a.reshape(-1)[s:][idx] == a[:, s:e].reshape(-1)).all()
    assert (R.blocked_rows(10, 10, 10) == np.arange(10)).all()


def test_chain_length():
    assert R.sum_chain_length(1050015, 1024) == 5 + 256 + 1024 and R.sum_chain_length(1, 1) == 258


def test_focal_yardstick_on_the_gpu_tests_inputs():
    """the number the GPU test multiplies by FOCAL_FACTOR; printed for the record"""
    logits, labels, weight = R.focal_case(70001, 15, seed=0)
    assert logits.size > R.FOCAL_CAP
    y_loss, y_grad = R.focal_yardstick(logits, labels, weight, 0.25, 2.0)
    print("focal yardstick, M 70001 C 15 alpha 0.25 gamma 2: loss %.3e  gradient %.3e (u = %.3e)" % (y_loss, y_grad, R.U))
    assert 0.5 * R.U <= y_loss <= 200 * R.U and 0.5 * R.U <= y_grad <= 200 * R.U
