"""GPU: the dense-head loss sums of csrc/loss_offset.hip PAST THE CAP of their grid (1024 workgroups x 256 threads: the
grid-stride loop runs from 1 048 576 elements on) against the float64 restatements of tests/dense_loss_ref.py (held to
float64 autograd by tests/test_dense_loss_cpu.py), through the C ABI.

  * gradient buffers element by element (a dropped element shows there);
  * loss totals within the sum of the per-term bounds + L u sum|terms|, L = sum_chain_length(n, partial sums written),
    the partial sums counted in the canary-filled workspace (allocated at the size of the query between guard bands);
  * probe runs: the weight is zero except on one row / element of the LAST grid-stride iteration, then one of the
    first: the loss must be that row's terms -- a term lost from, or counted twice in, the total shows at full size;
  * L1 (beta = 0) on lattice inputs: the sum is an integer below 2^24 and must EQUAL the reference;
  * level variants: labels / targets / weights are windows [:, s:e] of per-image arrays addressed through
    rows_per_block / block_stride; everything outside the window is NaN or a wrong label;
  * every call runs twice and must give the same bits.

Smooth-L1 bounds are counted from the header's formula (tests/dense_loss_ref.py).  The focal bound is measured, not
counted: FOUR times the largest normalised error of the float32 torch tensor chain (the composition the kernel
replaces) against float64, on the host, on the same inputs; neither number comes from the kernel.  On the main case
(M 70 001, C 15, alpha 0.25, gamma 2, weighted; normalised by alpha_t w (1 + |x|), the gradient also by gamma):

    yardstick  loss 2.824e-07  gradient 7.175e-08      bound (x 4)  loss 1.130e-06  gradient 2.870e-07

Measured on an MI355X (this module's printout): on that case the kernel's largest normalised gradient error is 7.018e-08
(0.245 of its bound; 0.23 - 0.26 of it at C = 15, up to 0.57 at M 37, C 1, whose yardstick rests on 37 elements), its loss total 802181.25 against 802181.268 (bound 64: the
chain term L u sum|terms| with L = 5 + 256 + 1024 dominates, which is why the probe runs exist).  Smooth-L1 gradients
reach 0.41 of their bound.  Partial sums written: 1024 of the 1024-row workspace at every size past the cap, 440 for
450 000 elements, 1 for the small cases."""
import functools

import numpy as np
import pytest
import torch

from tests import dense_loss_ref as R
from tests import guarded as G

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
CANARY_I32 = G.CANARY_WORD - (1 << 32) if G.CANARY_WORD >= (1 << 31) else G.CANARY_WORD
STRIDE = 1024 * 256                      # elements one grid-stride iteration covers at the cap


def _out(name, shape, dev):
    return G.Buf(name, "out", shape, torch.float32, dev, G.CANARY_WORD, payload_word=G.CANARY_WORD)


def _workspace(L, dev):
    nbytes = L.lib().jdet_sigmoid_focal_loss_workspace()
    assert nbytes == 4 * 1024                     # the 1024-row workspace the header documents
    return _out("ws", (nbytes // 4,), dev), nbytes


def _partials_written(ws):
    touched = (ws.t.view(torch.int32) != CANARY_I32).cpu().numpy()
    n = int(touched.sum())
    assert touched[:n].all(), "the written partial sums are not the leading ones"
    return n


def _done(bufs, written):
    torch.cuda.synchronize()
    for b in bufs:
        b.check_guards()
    for b in written:
        b.check_written()


def _np(t):
    return t.detach().cpu().numpy()


def _d(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_elements(got, ref, bound, what):
    g = _np(got).astype(F64).reshape(ref.shape)
    err = np.abs(g - ref)
    bad = ~(err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, 0.0)
    print("  %-10s max |err| %.3e, %.3g of its bound at most" % (what, float(err.max()) if err.size else 0.0,
                                                               float(frac.max()) if err.size else 0.0))
    if bad.any():
        k = np.unravel_index(int(np.flatnonzero(bad.reshape(-1))[0]), ref.shape)
        raise AssertionError("%s: %d of %d elements beyond their bound, first at %r: got %r, reference %r, bound %.3e"
                             % (what, int(bad.sum()), ref.size, k, float(g[k]), float(ref[k]), float(bound[k])))


def _check_total(got, terms, term_bound, chain, what, scale=1.0, extra_u=0):
    ref = float(terms.sum()) * scale
    bound = (float(term_bound.sum()) + chain * R.U * float(np.abs(terms).sum())) * abs(scale) + extra_u * R.U * abs(ref)
    err = abs(float(got) - ref)
    print("  %-10s %.9g, reference %.9g, |err| %.3e, bound %.3e (chain %d)" % (what, float(got), ref, err, bound, chain))
    assert err <= bound, "%s: %r against %r: error %.3e beyond %.3e" % (what, float(got), ref, err, bound)


# ---- focal loss -------------------------------------------------------------------------------------------------------
VARIANTS = {"weighted": (0.25, 2.0, True), "no_weight": (0.25, 2.0, False), "no_alpha": (-1.0, 2.0, True)}


@functools.lru_cache(maxsize=4)
def _focal_reference(M, C, variant):
    alpha, gamma, with_weight = VARIANTS[variant]
    logits, labels, weight = R.focal_case(M, C, seed=0, with_weight=with_weight)
    return (logits, labels, weight) + R.focal_bounds(logits, labels, weight, alpha, gamma)


def _focal_call(L, dev, d_logits, d_labels, d_weight, M, C, alpha, gamma):
    loss, grad = _out("loss", (1,), dev), _out("grad", (M, C), dev)
    ws, wsb = _workspace(L, dev)
    L.check(L.lib().jdet_sigmoid_focal_loss(L.ptr(d_logits), L.ptr(d_labels), L.ptr(d_weight) if d_weight is not None else None,
                                            M, C, alpha, gamma, L.ptr(loss.t), L.ptr(grad.t), L.ptr(ws.t), wsb,
                                            L.stream_ptr(d_logits)), "jdet_sigmoid_focal_loss")
    _done([loss, grad, ws], [loss, grad])
    return loss, grad, ws


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("M,C", [(70001, 15), (37, 15), (37, 1)])
def test_sigmoid_focal_loss(dev, M, C, variant):
    """70 001 x 15 = 1 050 015 elements: 1024 workgroups and a fifth, ragged grid-stride iteration.  Logits of +-40 and
    +-100 under true and false classes, labels 0 (background) and C, weight NULL / given, alpha < 0"""
    from jdet_amd import _lib as L
    alpha, gamma, _ = VARIANTS[variant]
    logits, labels, weight, terms, grad, tb, gb, yard = _focal_reference(M, C, variant)
    dl, dlab, dw = _d(logits, dev), _d(labels, dev), _d(weight, dev)
    a, b = _focal_call(L, dev, dl, dlab, dw, M, C, alpha, gamma), _focal_call(L, dev, dl, dlab, dw, M, C, alpha, gamma)
    assert G.same_bits(a[0].t, b[0].t) and G.same_bits(a[1].t, b[1].t)
    written = _partials_written(a[2])
    chain = R.sum_chain_length(M * C, written)
    print("focal M %d C %d %s: yardstick loss %.3e gradient %.3e -> bound %.3e / %.3e; %d partial sums"
          % (M, C, variant, yard[0], yard[1], R.FOCAL_FACTOR * yard[0], R.FOCAL_FACTOR * yard[1], written))
    assert 1 <= written <= 1024 and (M * C <= R.FOCAL_CAP or written == 1024)
    _check_elements(a[1].t, grad, gb, "gradient")
    g = _np(a[1].t)
    if weight is not None:
        assert (g[weight == 0] == 0).all()                               # a zero weight is a zero gradient, also at |x| = 100
    norm = gb / (R.FOCAL_FACTOR * yard[1] * max(1.0, gamma))
    on = norm > 0
    print("  kernel's largest normalised gradient error %.3e" % float((np.abs(g.astype(F64) - grad)[on] / (norm[on] * max(1.0, gamma))).max()))
    _check_total(a[0].t[0], terms, tb, chain, "loss sum")


@pytest.mark.parametrize("row", ["last_iteration", "first_iteration"])
def test_sigmoid_focal_loss_probe_rows(dev, row):
    """weight zero except on one row: the total is that row's terms.  Row 69 990 lies in the last, ragged grid-stride
    iteration (elements from 4 x 262 144 on), row 5 in the first (and carries +-40 logits)."""
    from jdet_amd import _lib as L
    M, C = 70001, 15
    alpha, gamma, _ = VARIANTS["weighted"]
    logits, labels, _, _, _, _, _, yard = _focal_reference(M, C, "weighted")
    r = 69990 if row == "last_iteration" else 5
    assert (r * C >= 4 * STRIDE) == (row == "last_iteration") and M * C > 4 * STRIDE
    weight = np.zeros(M, F32)
    weight[r] = 1.5
    terms, grad, aw = R.focal_terms(logits, labels, weight, alpha, gamma)
    norm = aw * (1.0 + np.abs(logits.astype(F64)))
    tb, gb = R.FOCAL_FACTOR * yard[0] * norm, R.FOCAL_FACTOR * yard[1] * max(1.0, gamma) * norm
    loss, g, ws = _focal_call(L, dev, _d(logits, dev), _d(labels, dev), _d(weight, dev), M, C, alpha, gamma)
    print("focal probe row %d" % r)
    assert not np.delete(terms, r, 0).any() and terms[r].sum() > 0
    _check_elements(g.t, grad, gb, "gradient")
    _check_total(loss.t[0], terms[r], tb[r], C, "loss sum")


# ---- smooth-L1 / L1 ----------------------------------------------------------------------------------------------------
def _smooth_l1_call(L, dev, dp, dt, dw, n, beta):
    loss = _out("loss", (1,), dev)
    grad = _out("grad", (n,), dev)
    ws, wsb = _workspace(L, dev)
    L.check(L.lib().jdet_smooth_l1_loss(L.ptr(dp), L.ptr(dt), L.ptr(dw) if dw is not None else None, n, beta, L.ptr(loss.t),
                                        L.ptr(grad.t), L.ptr(ws.t), wsb, L.stream_ptr(loss.t)), "jdet_smooth_l1_loss")
    _done([loss, grad, ws], [loss] + ([grad] if n else []))
    return loss, grad, ws


@pytest.mark.parametrize("beta", [0.0, 1.0 / 9.0, 1.0])
@pytest.mark.parametrize("n", [1050005, 1, 0])
def test_smooth_l1_loss(dev, n, beta):
    """1 050 005 elements: past the cap, ragged fifth iteration; differences of exactly 0, +-beta and one float32 step to
    either side of +-beta; n = 0 gives a zero loss"""
    from jdet_amd import _lib as L
    pred, target, weight = R.smooth_l1_case(n, beta, seed=int(beta * 9))
    terms, grad, tb, gb = R.smooth_l1_terms(pred, target, weight, beta)
    dp, dt, dw = _d(pred, dev), _d(target, dev), _d(weight, dev)
    a, b = _smooth_l1_call(L, dev, dp, dt, dw, n, beta), _smooth_l1_call(L, dev, dp, dt, dw, n, beta)
    assert G.same_bits(a[0].t, b[0].t) and G.same_bits(a[1].t, b[1].t)
    print("smooth_l1 n %d beta %g" % (n, beta))
    if n == 0:
        assert float(a[0].t[0]) == 0.0
        return
    written = _partials_written(a[2])
    assert 1 <= written <= 1024 and (n <= R.FOCAL_CAP or written == 1024)
    _check_elements(a[1].t, grad, gb, "gradient")
    if n >= 7:                                     # the planted differences: d is exact there, so is the branch
        k = 7 if beta else 1
        assert (pred[:k] - target[:k] == pred[:k]).all() and (_np(a[1].t)[:k] == grad[:k].astype(F32)).all()
    _check_total(a[0].t[0], terms, tb, R.sum_chain_length(n, written), "loss sum")


@pytest.mark.parametrize("beta", [0.0, 1.0 / 9.0])
@pytest.mark.parametrize("where", ["last_iteration", "first_iteration"])
def test_smooth_l1_loss_probe_elements(dev, where, beta):
    """weight zero except on one element: the total is that element's term"""
    from jdet_amd import _lib as L
    n = 1050005
    i = 1050000 if where == "last_iteration" else 3
    assert (i >= 4 * STRIDE) == (where == "last_iteration")
    pred, target, _ = R.smooth_l1_case(n, beta, seed=7)
    weight = np.zeros(n, F32)
    weight[i] = 1.5
    terms, grad, tb, gb = R.smooth_l1_terms(pred, target, weight, beta)
    loss, g, _ = _smooth_l1_call(L, dev, _d(pred, dev), _d(target, dev), _d(weight, dev), n, beta)
    print("smooth_l1 probe element %d beta %g" % (i, beta))
    assert terms[i] > 0 and not np.delete(terms, i).any()
    _check_elements(g.t, grad, gb, "gradient")
    _check_total(loss.t[0], terms[i:i + 1], tb[i:i + 1], 0, "loss sum")


def test_l1_loss_on_lattice_inputs_is_exact(dev):
    """integers: every partial sum in any order is an integer below 2^24, the total must EQUAL the float64 sum"""
    from jdet_amd import _lib as L
    n = 1050005
    pred, target, weight = R.smooth_l1_case(n, 0.0, seed=1, lattice=True)
    terms, grad, _, _ = R.smooth_l1_terms(pred, target, weight, 0.0)
    assert terms.sum() < 2 ** 24
    loss, g, _ = _smooth_l1_call(L, dev, _d(pred, dev), _d(target, dev), _d(weight, dev), n, 0.0)
    assert float(loss.t[0]) == float(terms.sum())
    assert (_np(g.t).astype(F64) == grad).all()
    loss, g, _ = _smooth_l1_call(L, dev, _d(pred, dev), _d(target, dev), None, n, 0.0)          # weight NULL = 1
    terms, grad, _, _ = R.smooth_l1_terms(pred, target, None, 0.0)
    assert float(loss.t[0]) == float(terms.sum()) and (_np(g.t).astype(F64) == grad).all()


# ---- level variants ----------------------------------------------------------------------------------------------------
N_IMG, ANCHORS = 3, 30000
AVG, LOSS_WEIGHT, GRAD_OUT = 123.5, 0.75, 1.25
WINDOWS = [(3300, 26700), (77, 78), (0, ANCHORS)]


def _grad_scale(L, dev, unit, n):
    out = _out("scaled", unit.t.shape, dev)
    go, avg = _d(np.array([GRAD_OUT], F32), dev), _d(np.array([AVG], F32), dev)
    L.check(L.lib().jdet_loss_grad_scale(L.ptr(unit.t), n, L.ptr(go), L.ptr(avg), LOSS_WEIGHT, L.ptr(out.t),
                                         L.stream_ptr(unit.t)), "jdet_loss_grad_scale")
    _done([out, unit], [out])
    ref = R.grad_scale(_np(unit.t), GRAD_OUT, AVG, LOSS_WEIGHT)          # the unit gradient is an input of this entry
    _check_elements(out.t, ref, R.K_SCALE * R.U * np.abs(ref), "scaled")


@pytest.mark.parametrize("s,e", WINDOWS)
def test_sigmoid_focal_loss_level(dev, s, e):
    """3 images, the column window [s:e] of (3, 30 000) label / weight arrays: 70 200 rows x 15 classes past the cap, a
    window of one column, the whole array.  Outside the window: labels of a wrong class or far out of range, NaN weights"""
    from jdet_amd import _lib as L
    C, alpha, gamma = 15, 0.25, 2.0
    M = N_IMG * (e - s)
    logits, lab, w = R.focal_case(M, C, seed=s + 1)
    c = np.arange(N_IMG * ANCHORS)
    labels = np.where(c % 2 == 0, 1 + c % C, 2 ** 30).astype(np.int32).reshape(N_IMG, ANCHORS)
    weights = np.full((N_IMG, ANCHORS), np.nan, F32)
    labels[:, s:e], weights[:, s:e] = lab.reshape(N_IMG, -1), w.reshape(N_IMG, -1)
    idx = s + R.blocked_rows(M, e - s, ANCHORS)
    assert (labels.reshape(-1)[idx] == lab).all() and (weights.reshape(-1)[idx] == w).all()
    terms, grad, tb, gb, yard = R.focal_bounds(logits, lab, w, alpha, gamma)
    dl, dlab, dw, davg = _d(logits, dev), _d(labels, dev), _d(weights, dev), _d(np.array([AVG], F32), dev)

    def call():
        loss, g = _out("loss", (1,), dev), _out("grad", (M, C), dev)
        ws, wsb = _workspace(L, dev)
        L.check(L.lib().jdet_sigmoid_focal_loss_level(
            L.ptr(dl), dlab.data_ptr() + 4 * s, e - s, ANCHORS, dw.data_ptr() + 4 * s, e - s, ANCHORS, M, C, alpha, gamma,
            L.ptr(davg), LOSS_WEIGHT, L.ptr(loss.t), L.ptr(g.t), L.ptr(ws.t), wsb, L.stream_ptr(dl)),
            "jdet_sigmoid_focal_loss_level")
        _done([loss, g, ws], [loss, g])
        return loss, g, ws

    a, b = call(), call()
    assert G.same_bits(a[0].t, b[0].t) and G.same_bits(a[1].t, b[1].t)
    written = _partials_written(a[2])
    print("focal level window [%d:%d] M %d: yardstick loss %.3e gradient %.3e; %d partial sums" % (s, e, M, yard[0], yard[1], written))
    assert 1 <= written <= 1024 and (M * C <= R.FOCAL_CAP or written == 1024)
    _check_elements(a[1].t, grad, gb, "gradient")
    _check_total(a[0].t[0], terms, tb, R.sum_chain_length(M * C, written), "loss", scale=LOSS_WEIGHT / AVG, extra_u=R.K_LEVEL)
    _grad_scale(L, dev, a[1], M * C)


@pytest.mark.parametrize("s,e,E", [(3300, 26700, 15), (77, 78, 5), (0, ANCHORS, 5)])
def test_smooth_l1_loss_level(dev, s, e, E):
    """targets / weights are windows [:, s:e, :] of (3, 30 000, E) arrays, NaN outside; 70 200 rows x 15 values past the
    cap (the box heads use E = 5: the one-column window and the whole array)"""
    from jdet_amd import _lib as L
    beta = 1.0 / 9.0
    rows = N_IMG * (e - s)
    n = rows * E
    pred, tgt, w = R.smooth_l1_case(n, beta, seed=s + 2)
    targets = np.full((N_IMG, ANCHORS, E), np.nan, F32)
    weights = np.full((N_IMG, ANCHORS, E), np.nan, F32)
    targets[:, s:e], weights[:, s:e] = tgt.reshape(N_IMG, -1, E), w.reshape(N_IMG, -1, E)
    idx = s + R.blocked_rows(rows, e - s, ANCHORS)
    assert (targets.reshape(-1, E)[idx].reshape(-1) == tgt).all()
    terms, grad, tb, gb = R.smooth_l1_terms(pred, tgt, w, beta)
    dp, dt, dw, davg = _d(pred, dev), _d(targets, dev), _d(weights, dev), _d(np.array([AVG], F32), dev)

    def call():
        loss, g = _out("loss", (1,), dev), _out("grad", (rows, E), dev)
        ws, wsb = _workspace(L, dev)
        L.check(L.lib().jdet_smooth_l1_loss_level(
            L.ptr(dp), dt.data_ptr() + 4 * s * E, e - s, ANCHORS, dw.data_ptr() + 4 * s * E, e - s, ANCHORS, rows, E, beta,
            L.ptr(davg), LOSS_WEIGHT, L.ptr(loss.t), L.ptr(g.t), L.ptr(ws.t), wsb, L.stream_ptr(dp)),
            "jdet_smooth_l1_loss_level")
        _done([loss, g, ws], [loss, g])
        return loss, g, ws

    a, b = call(), call()
    assert G.same_bits(a[0].t, b[0].t) and G.same_bits(a[1].t, b[1].t)
    written = _partials_written(a[2])
    print("smooth_l1 level window [%d:%d] rows %d E %d: %d partial sums" % (s, e, rows, E, written))
    assert 1 <= written <= 1024 and (n <= R.FOCAL_CAP or written == 1024)
    _check_elements(a[1].t, grad.reshape(rows, E), gb.reshape(rows, E), "gradient")
    _check_total(a[0].t[0], terms, tb, R.sum_chain_length(n, written), "loss", scale=LOSS_WEIGHT / AVG, extra_u=R.K_LEVEL)
    _grad_scale(L, dev, a[1], n)
