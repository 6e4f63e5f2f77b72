#!/usr/bin/env python3
"""Rotated RepPoints at config size: one eager REPPOINTS_CFG train step at 2 x 1024^2 with 64 gts per image, the head's
dense route against its general route in one process, alternating -- step time (host clock around a synchronise, three
rounds of eight steps after warm-up), the refine stage's jdet_convex_iou matrix (device events around the calculator),
and the launches of one step (torch.profiler, in a step of its own).  Needs a HIP device.

    python scripts/reppoints_timing.py [out.txt]

The numbers of profiles/reppoints.md come from this script."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jdet_amd.config.named import REPPOINTS_CFG  # noqa: E402
from jdet_amd.runner import Runner, synthetic_batch  # noqa: E402

out = []


def say(s):
    print(s, flush=True)
    out.append(s)


dev = torch.device("cuda:0")
images, targets = synthetic_batch(2, 1024, dev, seed=0, num_gts=64)
torch.manual_seed(0)
r = Runner(REPPOINTS_CFG, device=dev, graph=False)
head = r.model.bbox_head


class TimedIoU:
    def __init__(self, inner):
        self.inner, self.events = inner, []

    def __call__(self, *a, **k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        y = self.inner(*a, **k)
        e.record()
        self.events.append((s, e))
        return y


def steps(n, dense):
    head.dense = dense
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        loss, parts = r.train_step(images, targets)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, {k: float(v) for k, v in parts.items()}


for dense in (True, False):
    ms, parts = steps(4, dense)
    say("warm-up %s: %.1f ms/step %s" % ("dense" if dense else "general", ms, parts))
for rnd in range(3):
    for dense in (True, False):
        ms, _ = steps(8, dense)
        say("round %d %-7s %.2f ms/step (8 steps, host clock around a synchronise)" % (rnd, "dense" if dense else "general", ms))

timed = TimedIoU(head.refine_assigner.iou_calculator)
head.refine_assigner.iou_calculator = timed
for dense in (True, False):
    timed.events.clear()
    ms, _ = steps(4, dense)
    torch.cuda.synchronize()
    el = [s.elapsed_time(e) for s, e in timed.events]
    say("%-7s refine-stage jdet_convex_iou matrix (21824 point sets x 64 gts): %d calls in 4 steps, mean %.3f ms, max %.3f ms "
        "per call; %.3f ms of a %.2f ms step" % ("dense" if dense else "general", len(el), sum(el) / len(el), max(el),
                                                  sum(el) / 4, ms))
head.refine_assigner.iou_calculator = timed.inner

try:
    from torch.profiler import ProfilerActivity, profile
    for dense in (True, False):
        head.dense = dense
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            r.train_step(images, targets)
            torch.cuda.synchronize()
        ev = prof.events()
        kernels = [e for e in ev if str(e.device_type).endswith("CUDA") and not e.name.lower().startswith("memcpy")
                   and not e.name.lower().startswith("memset")]
        copies = [e for e in ev if str(e.device_type).endswith("CUDA") and e.name.lower().startswith("memcpy")]
        d2h = [e for e in copies if "dtoh" in e.name.lower() or "device -> host" in e.name.lower()]
        say("%-7s one eager step: %d kernel launches, %d memcpy (%d device -> host), %d memset"
            % ("dense" if dense else "general", len(kernels), len(copies), len(d2h),
               len([e for e in ev if str(e.device_type).endswith("CUDA") and e.name.lower().startswith("memset")])))
except Exception as ex:  # noqa: BLE001
    say("launch count: torch.profiler failed: %r" % (ex,))
head.dense = True
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
