#!/usr/bin/env python3
"""LSKNet_s at config size (2 x 1024^2): every HIP route of csrc/dwconv.hip and csrc/lsk_select.hip against the library
form it replaces, at the four stage shapes, and one LSKNET_S_ORCNN_CFG train step with the routes on and off -- one
process, the routes alternating; every figure is the median of 5 repetitions after warm-up, with their spread (max - min):
  dw5 / dw7d3   the 5x5 and the 7x7 dilation-3 depthwise convolutions of the stage's width, forward + backward, against
                torch.nn.functional.conv2d(groups=C) on the same channels-last tensors;
  mlp3          the 3x3 + bias + GELU over the MLP's hidden map (8x / 8x / 4x / 4x the stage), forward + backward,
                against conv2d(groups=C) followed by F.gelu;
  select        lsk_squeeze -> (a stand-in sigmoid map) -> lsk_select, forward + backward, against the composed mean /
                max / cat / mul chain;
  device events around 10 calls per repetition;
  step          one eager train step (batch 2, 1024^2, 64 boxes per image), host clock around a synchronise, 2 steps per
                repetition.
Needs a HIP device.

    python scripts/lsk_timing.py [out.txt] [--no-step]

The numbers of profiles/lsk.md come from this script."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jdet_amd.models  # noqa: E402,F401
from jdet_amd.config.named import LSKNET_S_ORCNN_CFG  # noqa: E402
from jdet_amd.ops import dwconv as D  # noqa: E402
from jdet_amd.ops import lsk_select as S  # noqa: E402

REPS = 5
OPS, LARGE_DEFAULT = True, D.LARGE_TAPS_MIN_POSITIONS
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def name(hip):
    return "hip" if hip else "library"


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


def compare(label, fn, clock, n, unit):
    """fn(hip) timed REPS times per route, the routes alternating -> {hip: (median, spread)}"""
    ms = {True: [], False: []}
    for hip in (True, False):
        clock(lambda: fn(hip), 2)
    for _ in range(REPS):
        for hip in (True, False):
            ms[hip].append(clock(lambda: fn(hip), n))
    res = {}
    for hip in (True, False):
        res[hip] = (statistics.median(ms[hip]), max(ms[hip]) - min(ms[hip]))
        say("%-22s %-8s median %.3f ms, spread %.3f ms over %d repetitions of %d %s: %s"
            % (label, name(hip), res[hip][0], res[hip][1], REPS, n, unit, " ".join("%.3f" % v for v in ms[hip])))
    d = res[False][0] - res[True][0]
    say("%-22s hip is %.3f ms %s (%.2fx)" % (label, abs(d), "faster" if d > 0 else "SLOWER", res[False][0] / res[True][0]))
    return res


def routes(hip):
    D.ENABLED = hip
    D.LARGE_TAPS_MIN_POSITIONS = 0 if OPS else LARGE_DEFAULT      # per op: the kernel itself at every stage
    S.ENABLED = hip


dev = torch.device("cuda:0")
torch.manual_seed(0)
STAGES = [(64, 256, 8), (128, 128, 8), (320, 64, 4), (512, 32, 4)]     # width, map side, MLP ratio


def cl(*shape):
    return torch.randn(shape, device=dev).contiguous(memory_format=torch.channels_last)


for stage, (C, side, ratio) in enumerate(STAGES, 1):
    for label, ch, k, pad, dil, act in (("dw5", C, 5, 2, 1, None), ("dw7d3", C, 7, 9, 3, None),
                                        ("mlp3", C * ratio, 3, 1, 1, "gelu")):
        x = cl(2, ch, side, side).requires_grad_(True)
        g = cl(2, ch, side, side)
        w = (torch.randn(ch, 1, k, k, device=dev) * 0.2).requires_grad_(True)
        b = torch.zeros(ch, device=dev).requires_grad_(True)

        def run(hip, x=x, g=g, w=w, b=b, pad=pad, dil=dil, act=act):
            routes(hip)
            x.grad = w.grad = b.grad = None
            D.dwconv(x, w, b, pad, dil, act).backward(g)
        mb = x.numel() * 4 / 1e6
        say("stage %d %s: (2, %d, %d, %d), %.1f MB per map" % (stage, label, ch, side, side, mb))
        compare("stage %d %s" % (stage, label), run, device_ms, 10, "forward + backward")

        def fwd(hip, x=x, w=w, b=b, pad=pad, dil=dil, act=act):
            routes(hip)
            with torch.no_grad():
                D.dwconv(x, w, b, pad, dil, act)
        compare("stage %d %s fwd" % (stage, label), fwd, device_ms, 10, "forward")
        del x, g, w, b
    a1, a2 = cl(2, C // 2, side, side).requires_grad_(True), cl(2, C // 2, side, side).requires_grad_(True)
    g = cl(2, C // 2, side, side)
    mix = torch.randn(2, 2, 1, 1, device=dev)

    def sel(hip, a1=a1, a2=a2, g=g):
        routes(hip)
        a1.grad = a2.grad = None
        agg = S.lsk_squeeze(a1, a2)
        sig = (agg * mix).sigmoid().contiguous(memory_format=torch.channels_last)   # stands in for conv_squeeze + sigmoid
        S.lsk_select(a1, a2, sig).backward(g)
    say("stage %d select: two branches of (2, %d, %d, %d)" % (stage, C // 2, side, side))
    compare("stage %d select" % stage, sel, device_ms, 10, "forward + backward")
    del a1, a2, g
    torch.cuda.empty_cache()

OPS = False                                                    # the step: the default routing
if "--no-step" not in sys.argv:
    from jdet_amd.runner import Runner, synthetic_batch
    images, targets = synthetic_batch(2, 1024, dev, seed=0, num_gts=64)
    torch.manual_seed(0)
    r = Runner(LSKNET_S_ORCNN_CFG, device=dev, graph=False, conv_autotune=False)     # the heuristic solver pick on both routes

    def step(hip):
        routes(hip)
        return r.train_step(images, targets)
    for hip in (True, False):
        say("warm-up %s: mean of 2 steps %.1f ms" % (name(hip), host_ms(lambda: step(hip), 2)))
    compare("step", step, host_ms, 2, "eager train steps")
routes(True)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    open(args[0], "w").write("\n".join(out) + "\n")
