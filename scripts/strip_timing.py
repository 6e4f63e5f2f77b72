#!/usr/bin/env python3
"""StripNet_S at config size (2 x 1024^2): the rolling-window strip kernel (csrc/strip_conv.hip) against the generic
depthwise kernel (csrc/dwconv.hip) and against the library, at the four stage shapes, and one STRIP_RCNN_S_CFG train
step with the strip kernel on and off -- one process, the routes alternating; every figure is the median of 5
repetitions after 3 untimed windows of the same length per route, with their spread (max - min):
  1x19 / 19x1   the two strip layers of the stage's width, forward and forward + backward, three routes on the same
                channels-last tensors: (a) strip = ops.strip_conv._StripConv, (b) generic = ops.dwconv._DWConv,
                (c) library = torch.nn.functional.conv2d(groups=C); device events around 10 calls per repetition;
  step          one eager train step (batch 2, 1024^2, 64 boxes per image), host clock around a synchronise, 2 steps per
                repetition; "strip" sends every strip layer to the strip kernel whatever `preferred` says, "generic"
                is JDET_STRIP_CONV=0: the same layers on the generic kernel.
Needs a HIP device.

    python scripts/strip_timing.py [out.txt] [--no-step]

The numbers of profiles/strip.md come from this script."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jdet_amd.models  # noqa: E402,F401
from jdet_amd.config.named import STRIP_RCNN_S_CFG  # noqa: E402
from jdet_amd.ops import dwconv as D  # noqa: E402
from jdet_amd.ops import strip_conv as S  # noqa: E402

REPS, WARMUP = 5, 3          # timed repetitions; untimed windows of the same length before them, per route
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def host_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def device_ms(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def compare(label, fn, routes, clock, n, unit):
    """fn(route) timed REPS times per route, the routes alternating -> {route: (median, spread)}"""
    ms = {r: [] for r in routes}
    for _ in range(WARMUP):
        for r in routes:
            clock(lambda: fn(r), n)
    for _ in range(REPS):
        for r in routes:
            ms[r].append(clock(lambda: fn(r), n))
    res = {}
    for r in routes:
        res[r] = (statistics.median(ms[r]), max(ms[r]) - min(ms[r]))
        say("%-22s %-8s median %.4f ms, spread %.4f ms over %d repetitions of %d %s: %s"
            % (label, r, res[r][0], res[r][1], REPS, n, unit, " ".join("%.4f" % v for v in ms[r])))
    a, b = res[routes[0]], res[routes[1]]
    d = b[0] - a[0]
    verdict = "faster" if d > 0 else "SLOWER"
    say("%-22s %s is %.4f ms %s than %s (%.2fx); the two spreads add to %.4f ms: %s"
        % (label, routes[0], abs(d), verdict, routes[1], b[0] / a[0], a[1] + b[1],
           "resolved" if abs(d) > a[1] + b[1] else "NOT resolved"))
    return res


dev = torch.device("cuda:0")
torch.manual_seed(0)
STAGES = [(64, 256), (128, 128), (320, 64), (512, 32)]     # width, map side
ROUTES = ("strip", "generic", "library")


def cl(*shape):
    return torch.randn(shape, device=dev).contiguous(memory_format=torch.channels_last)


def conv(route, x, w, b, pad):
    if route == "strip":
        return S._StripConv.apply(x, w, b)
    if route == "generic":
        return D._DWConv.apply(x, w, b, pad, 1, 0)
    return D.dwconv_composed(x, w, b, pad, 1)


for stage, (C, side) in enumerate(STAGES, 1):
    for label, kshape, pad in (("1x19", (1, 19), (0, 9)), ("19x1", (19, 1), (9, 0))):
        x = cl(2, C, side, side).requires_grad_(True)
        g = cl(2, C, side, side)
        w = (torch.randn((C, 1) + kshape, device=dev) * 0.2).requires_grad_(True)
        b = torch.zeros(C, device=dev).requires_grad_(True)
        assert S.fusable(x, w, b, pad) and D.fusable(x, w, b, pad, 1)
        with torch.no_grad():
            assert torch.equal(conv("strip", x, w, b, pad), conv("generic", x, w, b, pad))

        def run(route, x=x, g=g, w=w, b=b, pad=pad):
            x.grad = w.grad = b.grad = None
            conv(route, x, w, b, pad).backward(g)

        def fwd(route, x=x, w=w, b=b, pad=pad):
            with torch.no_grad():
                conv(route, x, w, b, pad)
        say("stage %d %s: (2, %d, %d, %d), %.1f MB per map" % (stage, label, C, side, side, x.numel() * 4 / 1e6))
        compare("stage %d %s fwd" % (stage, label), fwd, ROUTES, device_ms, 10, "forward")
        compare("stage %d %s" % (stage, label), run, ROUTES, device_ms, 10, "forward + backward")
        del x, g, w, b
    torch.cuda.empty_cache()

if "--no-step" not in sys.argv:
    from jdet_amd.runner import Runner, synthetic_batch
    images, targets = synthetic_batch(2, 1024, dev, seed=0, num_gts=64)
    torch.manual_seed(0)
    r = Runner(STRIP_RCNN_S_CFG, device=dev, graph=False, conv_autotune=False)     # the heuristic solver pick on both routes
    shipped = S.preferred

    def step(route):
        S.ENABLED = route == "strip"
        S.preferred = (lambda x, w: True) if route == "strip" else shipped
        return r.train_step(images, targets)
    for route in ("strip", "generic"):
        say("warm-up %s: mean of 2 steps %.1f ms" % (route, host_ms(lambda: step(route), 2)))
    compare("step", step, ("strip", "generic"), host_ms, 2, "eager train steps")
    S.preferred = shipped
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    open(args[0], "w").write("\n".join(out) + "\n")
