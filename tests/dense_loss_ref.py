"""Float64 restatements of the dense-head loss sums of include/jdet_hip.h (sigmoid focal loss, weighted smooth-L1 / L1,
the level variants' (sum / avg_factor) * loss_weight, jdet_loss_grad_scale), the inputs the GPU tests
(tests/test_gpu_dense_losses.py) run them on, and the float32 yardstick of the focal bound.
tests/test_dense_loss_cpu.py holds them to torch float64 autograd.

Focal loss (the reference project's models/losses/focal_loss.py: BCE with logits, one-hot by class index + 1 == label,
per-row weight, (1 - p_t)^gamma, alpha_t; alpha < 0: no alpha term) with z = +x for the true class, -x otherwise:
    p_t = sigmoid(z),  q = 1 - p_t = sigmoid(-z),  ce = -log p_t = softplus(-z)
    term = alpha_t w ce q^gamma
    d term / dx = alpha_t w s (-q^(gamma + 1) - gamma q^gamma p_t ce),  s = dz/dx = +-1
written with sigmoid(-z) and softplus so that float64 keeps q and ce where 1 - p_t cancels (|x| = 40, 100); the
reference's log floor of 1e-10 never acts (its argument is >= 1).

Bounds.  u = 2^-24.  Smooth-L1, counted from d = pred - target (1 rounding, of |d|):
    |d| < beta:  0.5 d d / beta w   2 (d twice) + 1 (d d) + 4 (division, 2 ulp) + 1 (w)            = 8 u of the term
                 gradient d / beta w   1 + 4 + 1                                                  = 6 u
    otherwise:   (|d| - 0.5 beta) w    1 (d) + 1 (-) + 1 (w)  <= 8 u of (|d| + 0.5 beta) w;   gradient +-w exact
  An element whose |d| lies within 4 u beta of beta may take the other branch in float32; both branches agree there to
  first order, and it gets the linear branch's magnitude for the term and 6 u w for the gradient.
Focal: expf / logf / powf differ between libms, so no operation count: the error of the float32 torch tensor chain
(models/losses/focal_loss.py: sigmoid_focal_loss, the composition the kernel replaces) against float64, on the host, on
the same inputs, normalised by alpha_t w (1 + |x|) (gradient: times max(1, gamma)), is the yardstick; the kernel is
given FOUR times its maximum (device transcendentals are specified a few ulp looser than the host's and the kernel's
gradient formula has two more products).  Loss totals: the sum of the per-term bounds + L u sum|terms|."""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
K_SL1_TERM, K_SL1_GRAD, K_SCALE = 8, 6, 6
FOCAL_FACTOR = 4.0
FOCAL_CAP = 1024 * 256 * 4            # elements one pass of 1024 workgroups x 256 threads x 4 covers: the grid caps here


def focal_terms(logits, labels, weight, alpha, gamma):
    """(terms, d sum / d logits, alpha_t w) of shape (M, C), float64, from float32 logits / weights"""
    x = logits.astype(F64)
    M, C = x.shape
    t = labels.reshape(M, 1).astype(np.int64) == np.arange(1, C + 1)[None, :]
    s = np.where(t, 1.0, -1.0)
    z = s * x
    ce = np.logaddexp(0.0, -z)
    q = np.exp(-np.logaddexp(0.0, z))               # sigmoid(-z)
    pt = np.exp(-np.logaddexp(0.0, -z))             # sigmoid(z)
    at = np.where(t, alpha, 1.0 - alpha) if alpha >= 0 else np.ones_like(x)
    w = np.ones((M, 1)) if weight is None else weight.reshape(M, 1).astype(F64)
    aw = at * w
    qg = q ** gamma
    return aw * ce * qg, aw * s * (-(qg * q) - gamma * qg * pt * ce), aw


def smooth_l1_terms(pred, target, weight, beta):
    """(terms, d sum / d pred, term bound, gradient bound), float64; beta the float32 value the kernel receives"""
    beta = float(F32(beta))
    d = pred.astype(F64) - target.astype(F64)
    w = np.ones_like(d) if weight is None else weight.astype(F64)
    ad = np.abs(d)
    if beta == 0.0:
        return ad * w, np.sign(d) * w, 2 * U * ad * np.abs(w), np.zeros_like(d)       # L1: d and the product
    quad = ad < beta
    lin_mag = (ad + 0.5 * beta) * np.abs(w)
    terms = np.where(quad, 0.5 * d * d / beta, ad - 0.5 * beta) * w
    grad = np.where(quad, d / beta, np.sign(d)) * w
    near = np.abs(ad - beta) <= 4 * U * beta
    tb = K_SL1_TERM * U * np.where(quad & ~near, np.abs(terms), lin_mag)
    gb = K_SL1_GRAD * U * np.where(quad | near, np.maximum(np.abs(grad), np.abs(w) * near), 0.0)
    return terms, grad, tb, gb


def level_loss(total, avg_factor, loss_weight):
    """(sum / avg_factor) * loss_weight with the float32 scalars the kernel receives; K_LEVEL u of it on top of the sum's bound"""
    return total / float(F32(avg_factor)) * float(F32(loss_weight))


K_LEVEL = 5        # division (2 ulp = 4 u) + product


def grad_scale(unit, grad_out, avg_factor, loss_weight):
    """jdet_loss_grad_scale: unit * ((grad_out * loss_weight) / avg_factor); K_SCALE = 1 + 4 + 1 u of the result"""
    return unit.astype(F64) * ((float(F32(grad_out)) * float(F32(loss_weight))) / float(F32(avg_factor)))


def blocked_rows(rows, rows_per_block, block_stride):
    """the header's blocked row index: logical row r -> (r / rows_per_block) * block_stride + r % rows_per_block"""
    r = np.arange(rows)
    return (r // rows_per_block) * block_stride + r % rows_per_block


def sum_chain_length(n, rows_written):
    """additions any term passes through in a two-stage sum of n terms whose first stage wrote `rows_written` partial sums
    from 256-thread workgroups into the 1024-row workspace: its thread's share, the 256 threads of its workgroup, the
    partial sums"""
    rows_written = max(int(rows_written), 1)
    return -(-int(n) // (256 * rows_written)) + 256 + rows_written


# ---- inputs --------------------------------------------------------------------------------------------------------------
EXTREME_LOGITS = (40.0, -40.0, 100.0, -100.0)


def focal_case(M, C, seed=0, with_weight=True):
    """logits N(0, 3) with +-40 / +-100 planted on true and on false classes, labels 0 (background, about half) .. C,
    weights 0 (a quarter of the rows) or in [0.5, 2]"""
    rng = np.random.default_rng(4000 + seed)
    logits = (3.0 * rng.standard_normal((M, C))).astype(F32)
    labels = np.where(rng.random(M) < 0.5, 0, rng.integers(1, C + 1, M)).astype(np.int32)
    labels[:min(M, 4)] = [0, C, 1, 0][:min(M, 4)]
    for r in range(min(M, 16)):                     # extremes under the true class and under a false one
        v = EXTREME_LOGITS[r % 4]
        if labels[r] > 0:
            logits[r, labels[r] - 1] = v
        if C > 1 or labels[r] == 0:
            logits[r, labels[r] % C] = -v if r % 8 < 4 else v      # column labels[r] is class labels[r] + 1: never the true one
    k = min(64, M // 8)                             # and on a few random elements further down
    if k:
        rows = rng.integers(min(16, M - 1), M, k)
        logits[rows, rng.integers(0, C, k)] = np.array(EXTREME_LOGITS, F32)[rng.integers(0, 4, k)]
    weight = None
    if with_weight:
        weight = np.where(rng.random(M) < 0.25, 0.0, rng.uniform(0.5, 2.0, M)).astype(F32)
        weight[:min(M, 16)] = 1.0
    return logits, labels, weight


def focal_yardstick(logits, labels, weight, alpha, gamma):
    """largest normalised error of the float32 torch tensor chain against float64, on the host: (loss terms, gradient)"""
    import torch
    from jdet_amd.models.losses.focal_loss import sigmoid_focal_loss
    x = torch.from_numpy(logits).clone().requires_grad_(True)
    w = None if weight is None else torch.from_numpy(weight)
    loss = sigmoid_focal_loss(x, torch.from_numpy(labels), w, alpha=alpha, gamma=gamma, reduction="none")
    loss.sum().backward()
    terms, grad, aw = focal_terms(logits, labels, weight, alpha, gamma)
    norm = aw * (1.0 + np.abs(logits.astype(F64)))
    on = norm > 0
    e_loss = np.abs(loss.detach().numpy().astype(F64) - terms)[on] / norm[on]
    e_grad = np.abs(x.grad.numpy().astype(F64) - grad)[on] / (norm[on] * max(1.0, gamma))
    return float(e_loss.max()), float(e_grad.max())


def focal_bounds(logits, labels, weight, alpha, gamma):
    """(terms, grad, term bound, gradient bound, (yardstick loss, yardstick gradient)): FOCAL_FACTOR times the yardstick,
    de-normalised per element"""
    terms, grad, aw = focal_terms(logits, labels, weight, alpha, gamma)
    y_loss, y_grad = focal_yardstick(logits, labels, weight, alpha, gamma)
    norm = aw * (1.0 + np.abs(logits.astype(F64)))
    return terms, grad, FOCAL_FACTOR * y_loss * norm, FOCAL_FACTOR * y_grad * max(1.0, gamma) * norm, (y_loss, y_grad)


def smooth_l1_case(n, beta, seed=0, lattice=False):
    """pred, target, weight (n,), float32.  With beta > 0 (and n >= 7) the first elements carry differences of exactly 0, +-beta and
    one float32 step to either side of +-beta (target 0 there, so pred - target is exact).  lattice: integers with
    |pred| <= 2, |target| <= 1, weight in {0, 1, 2}: the L1 sum is an integer below 2^24 for n <= 2 700 000."""
    rng = np.random.default_rng(5000 + seed)
    if lattice:
        return (rng.integers(-2, 3, n).astype(F32), rng.integers(-1, 2, n).astype(F32), rng.integers(0, 3, n).astype(F32))
    pred = rng.standard_normal(n).astype(F32)
    target = rng.standard_normal(n).astype(F32)
    weight = np.where(rng.random(n) < 0.25, 0.0, rng.uniform(0.5, 2.0, n)).astype(F32)
    b = F32(beta)
    planted = [F32(0.0)]
    if b > 0:
        for s in (F32(1), F32(-1)):
            planted += [s * b, s * np.nextafter(b, F32(np.inf)), s * np.nextafter(b, F32(0))]
    if n >= len(planted):
        k = len(planted)
        pred[:k], target[:k], weight[:k] = planted, 0.0, 1.0
    return pred, target, weight
