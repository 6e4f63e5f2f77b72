#!/usr/bin/env python3
"""H2RBox at config size: one eager H2RBOX_CFG train step at 2 x 1024^2 (crop 1024^2) with 64 gts per image and a fixed
angle of 0.7, the dense route (jdet_rotate_crop + the fused consistency loss) against the general route (grid_sample +
the reference's tensor program) in one process, alternating -- step time (host clock around a synchronise, three rounds
of eight steps after warm-up), jdet_rotate_crop against the grid_sample program on the same 2 x 3 x 1024^2 input (device
events around 5000 calls of the kernel and 2000 of the program -- windows of 0.2 to 0.5 s -- three alternating rounds), and the launches of one step (torch.profiler, in a step of its own).
Needs a HIP device.

    python scripts/h2rbox_timing.py [out.txt]

The numbers of profiles/h2rbox.md come from this script."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jdet_amd.config.named import H2RBOX_CFG  # noqa: E402
from jdet_amd.ops.rotate_crop import rotate_crop  # noqa: E402
from jdet_amd.runner import Runner, synthetic_batch  # noqa: E402

out = []


def say(s):
    print(s, flush=True)
    out.append(s)


dev = torch.device("cuda:0")
images, targets = synthetic_batch(2, 1024, dev, seed=0, num_gts=64)
torch.manual_seed(0)
r = Runner(H2RBOX_CFG, device=dev, graph=False)
model, head = r.model, r.model.bbox_head
model.fixed_rot = 0.7


def route(dense):
    head.dense = dense
    model.device_rotate = dense


def steps(n, dense):
    route(dense)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        loss, parts = r.train_step(images, targets)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, {k: round(float(v), 5) for k, v in parts.items()}


for dense in (True, False):
    ms, parts = steps(4, dense)
    say("warm-up %s: mean of 4 steps %.1f ms %s" % ("dense" if dense else "general", ms, parts))
for rnd in range(3):
    for dense in (True, False):
        ms, _ = steps(8, dense)
        say("round %d %-7s %.2f ms/step (8 steps, host clock around a synchronise)" % (rnd, "dense" if dense else "general", ms))


def view(device_route, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        y = rotate_crop(images, 0.7, (1024, 1024), "reflection", device_route=device_route)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n, y


a, b = view(True, 5)[1], view(False, 5)[1]
say("rotate_crop 2 x 3 x 1024^2, theta 0.7, reflection: kernel against grid_sample max |difference| %.3e" % float((a - b).abs().max()))
for rnd in range(3):
    for device_route, n in ((True, 5000), (False, 2000)):
        ms, _ = view(device_route, n)
        say("round %d rotate_crop %-22s %.4f ms/call (%d calls between device events, window %.0f ms)"
            % (rnd, "jdet_rotate_crop" if device_route else "grid_sample program", ms, n, ms * n))

try:
    from torch.profiler import ProfilerActivity, profile

    def count(fn, label):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        copies = [e for e in ev if e.name.lower().startswith("memcpy")]
        sets = [e for e in ev if e.name.lower().startswith("memset")]
        d2h = [e for e in copies if "dtoh" in e.name.lower() or "device -> host" in e.name.lower()]
        say("%-28s %d kernel launches, %d memcpy (%d device -> host), %d memset"
            % (label, len(ev) - len(copies) - len(sets), len(copies), len(d2h), len(sets)))
    for dense in (True, False):
        route(dense)
        count(lambda: r.train_step(images, targets), "%-7s one eager step:" % ("dense" if dense else "general"))
    for device_route in (True, False):
        count(lambda: rotate_crop(images, 0.7, (1024, 1024), "reflection", device_route=device_route),
              "jdet_rotate_crop:" if device_route else "grid_sample program:")
except Exception as ex:  # noqa: BLE001
    say("launch count: torch.profiler failed: %r" % (ex,))
route(True)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
