"""Buffer-contract cases (tests/guarded.py protocol, `tests.abi_cases.Case` objects) for the entry points of
include/jdet_hip_retina.h, with the float64 restatements of tests/retina_ref.py as references.  Importable without a GPU:
tests/test_retinanet_cpu.py dry-runs every case, tests/test_gpu_retinanet.py runs them on the device.  The builders reach
the library through `abi_cases.lib()`, so the dry run's replacement applies; nothing is appended to abi_cases.CASES.

Bounds: gt preparation, encode and decode are float64 arithmetic rounded once, so one fp32 spacing of the float64
value; labels, weights, counts and the selection order are exact; the bilinear bounds are derived in `bilinear_k`."""
import numpy as np
import torch

from tests import abi_cases as AC
from tests import retina_ref as R
from tests.abi_cases import Case, P, Res, ST, exact

I32 = torch.int32
U24 = 2.0 ** -24


def one_spacing(ref):
    return np.asarray(ref, np.float64), R.spacing(ref)


def gt_prepare_case(K, seed=0):
    """random gts over the documented angle range and beyond: every branch (a >= 0, a < -pi/2, w > h) occurs"""
    rng = np.random.default_rng(seed)
    g0 = np.concatenate([rng.uniform(20, 600, (K, 2)), np.exp(rng.uniform(np.log(8), np.log(300), (K, 2))),
                         rng.uniform(-np.pi, np.pi, (K, 1))], 1).astype(np.float32)

    def fn(run):
        g = run.inp("gts", g0)
        rb, rh = run.out("rboxes", (K, 5)), run.out("rboxes_h", (K, 4))
        run.ok(AC.lib().jdet_retina_gt_prepare(P(g), K, P(rb), P(rh), ST(g)), "jdet_retina_gt_prepare")

        def ref():
            b, h = R.gt_prepare(g0)
            return {"rboxes": one_spacing(b), "rboxes_h": one_spacing(h)}
        return Res({"rboxes": rb, "rboxes_h": rh}, ref)
    return Case(("jdet_retina_gt_prepare",), "K %d" % K, fn)


def targets_case(tie=False):
    """the batch fixture: images of 0, 1, 70 [+ a duplicate] and GT_CHUNK + 1 gts on the 1113 anchors"""
    f = R.batch(tie)
    a0 = R.anchors()
    N, A = len(f["raws"]), len(a0)

    def fn(run):
        a, rb, rh = run.inp("anchors", a0), run.inp("rboxes", f["rboxes"]), run.inp("rboxes_h", f["rboxes_h"])
        gl, off = run.inp("gt_labels", f["gt_labels"]), run.inp("gt_offsets", f["offsets"])
        outs = dict(labels=run.out("labels", (N, A), I32), label_weights=run.out("label_weights", (N, A)),
                    loc_targets=run.out("loc_targets", (N, A, 5)), loc_weights=run.out("loc_weights", (N, A, 5)),
                    raw_labels=run.out("raw_labels", (N, A), I32), normalizer=run.out("normalizer", (N,)))
        ws, wsb = run.ws("workspace", AC.lib().jdet_retina_targets_workspace(N, A))
        run.ok(AC.lib().jdet_retina_targets(
            P(a), A, P(rb), P(rh), P(gl), P(off), N, len(f["rboxes"]), R.POS, R.NEG_HI, R.NEG_LO, P(outs["labels"]),
            P(outs["label_weights"]), P(outs["loc_targets"]), P(outs["loc_weights"]), P(outs["raw_labels"]),
            P(outs["normalizer"]), P(ws), wsb, ST(a)), "jdet_retina_targets")

        def ref():
            raw = f["raw_labels"]
            return {"labels": exact(np.maximum(raw, 0)), "label_weights": exact((raw >= 0).astype(np.float32)),
                    "loc_targets": one_spacing(f["loc"]),
                    "loc_weights": exact(np.repeat((raw > 0).astype(np.float32)[..., None], 5, -1)),
                    "raw_labels": exact(raw), "normalizer": exact(f["normalizer"])}
        return Res(outs, ref)
    return Case(("jdet_retina_targets",), "K (0, 1, 70%s, %d) x 1113 anchors, dirty workspace"
                % ("+1 tied" if tie else "", R.GT_CHUNK + 1), fn)


def detect_case(sx=2.0, sy=0.5):
    """count + fill on the detect fixture; the size ratios are powers of two, so the fp32 scaling after the rounding is
    exact and the one-spacing bound holds for the scaled columns too"""
    f = R.detect_fixture()
    a0 = R.anchors()
    A, C = f["logits"].shape
    d = R.detect(a0, f["loc"], f["logits"], f["thr"], sx, sy)
    M = len(d["labels"])

    def fn(run):
        a, loc, x = run.inp("anchors", a0), run.inp("loc", f["loc"]), run.inp("logits", f["logits"])
        counts = run.out("counts", (C,), I32)
        boxes, scores, labels = run.out("boxes", (M, 5)), run.out("scores", (M,)), run.out("labels", (M,), I32)
        ws, wsb = run.ws("workspace", AC.lib().jdet_retina_detect_workspace(A, C))
        run.ok(AC.lib().jdet_retina_detect_count(P(a), P(loc), P(x), A, C, f["thr"], P(counts), P(ws), wsb, ST(a)),
               "jdet_retina_detect_count")
        run.ok(AC.lib().jdet_retina_detect_fill(P(a), P(loc), P(x), A, C, f["thr"], sx, sy, P(ws), wsb, M, P(boxes),
                                                P(scores), P(labels), ST(a)), "jdet_retina_detect_fill")
        return Res(dict(counts=counts, boxes=boxes, scores=scores, labels=labels),
                   lambda: {"counts": exact(d["counts"].astype(np.int32)), "boxes": one_spacing(d["boxes"]),
                            "scores": one_spacing(d["scores"]), "labels": exact(d["labels"])})
    return Case(("jdet_retina_detect_count", "jdet_retina_detect_fill"),
                "1113 anchors x %d classes, %d selected, dirty workspace" % (C, M), fn)


BILINEAR_SHAPES = [(2, 8, 10, 6, 5, 3, 2.0), (1, 4, 25, 25, 13, 13, 2.0), (2, 12, 17, 9, 5, 4, 1.0),
                   (1, 4, 5, 3, 5, 3, 2.0)]          # N, C, H, W, Ht, Wt, div


def bilinear_k(shape, backward):
    """the multiple k of 2^-24 * max|input| that bounds the kernel against float64 (u = 2^-24, inputs within m):
    forward: a lerp d*b + (1-d)*a costs u for 1-d, 2u*m for the products, u*m for the sum = 4u*m; the second level
    passes the 4u*m on and adds 4u*m of its own; the add to the lateral (|sum| <= 2m) 2u*m and the division 2u*m more:
    k = 12 (div >= 1).
    backward, n = the largest pre-image: a weight (two selected terms and their sum) 2u, the product of two weights 5u,
    times g 6u*m per addend; every partial sum is within n*m, so n additions n*n*u*m; the division u*n*m:
    k = n * (n + 7)."""
    N, C, H, W, Ht, Wt, div = shape
    if not backward:
        return 12.0
    n = R.preimage_addends(H, W, Ht, Wt)
    return float(n * (n + 7))


def _bilinear_inputs(shape):
    N, C, H, W, Ht, Wt, div = shape
    rng = np.random.default_rng(H * 1000 + W)
    return (rng.standard_normal((N, H, W, C)).astype(np.float32), rng.standard_normal((N, Ht, Wt, C)).astype(np.float32),
            rng.standard_normal((N, H, W, C)).astype(np.float32))


def bilinear_forward_case(shape):
    N, C, H, W, Ht, Wt, div = shape
    lat0, top0, _ = _bilinear_inputs(shape)

    def fn(run):
        lat, top, out = run.inp("lateral", lat0), run.inp("top", top0), run.out("out", (N, H, W, C))
        run.ok(AC.lib().jdet_upsample_add_bilinear_nhwc_forward(P(lat), P(top), N, C, H, W, Ht, Wt, div, P(out), ST(lat)),
               "jdet_upsample_add_bilinear_nhwc_forward")
        m = max(float(np.abs(lat0).max()), float(np.abs(top0).max()))
        return Res({"out": out}, lambda: {"out": ((lat0.astype(np.float64) + R.resize(top0, H, W)) / div,
                                                  bilinear_k(shape, False) * U24 * m)})
    return Case(("jdet_upsample_add_bilinear_nhwc_forward",), "%d x %d from %d x %d, N %d C %d div %g"
                % (H, W, Ht, Wt, N, C, div), fn)


def bilinear_backward_case(shape):
    N, C, H, W, Ht, Wt, div = shape
    g0 = _bilinear_inputs(shape)[2]

    def fn(run):
        g, gt = run.inp("grad_out", g0), run.out("grad_top", (N, Ht, Wt, C))
        run.ok(AC.lib().jdet_upsample_add_bilinear_nhwc_backward(P(g), N, C, H, W, Ht, Wt, div, P(gt), ST(g)),
               "jdet_upsample_add_bilinear_nhwc_backward")
        return Res({"grad_top": gt}, lambda: {"grad_top": (R.resize_t(g0, Ht, Wt) / div,
                                                          bilinear_k(shape, True) * U24 * float(np.abs(g0).max()))})
    return Case(("jdet_upsample_add_bilinear_nhwc_backward",), "%d x %d onto %d x %d, N %d C %d div %g"
                % (H, W, Ht, Wt, N, C, div), fn)


def all_cases():
    cases = [gt_prepare_case(1), gt_prepare_case(300, 1), targets_case(False), targets_case(True), detect_case()]
    for s in BILINEAR_SHAPES:
        cases += [bilinear_forward_case(s), bilinear_backward_case(s)]
    return cases
