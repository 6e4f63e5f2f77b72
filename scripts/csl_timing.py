#!/usr/bin/env python3
"""Circular Smooth Label at config size: CSL_RETINANET_CFG (R50) at 2 x 1024^2 with 100 gts per image, the fused routes
(csrc/csl.hip: the angle-loss node, the in-place decode) against the composed ones (JDET_CSL_FUSED=0) in one process,
alternating; every figure is the median of 5 repetitions after warm-up, with their spread (max - min) --
  nodes   loss_angle of all five levels, forward and backward, on synthetic maps of the config's sizes (392 832 anchors x
          45 bins, about 1 % positive anchors), device events around 20 calls per repetition;
  step    one eager train step, host clock around a synchronise, 4 steps per repetition;
  infer   bbox_head.get_bboxes on the head outputs of one eval forward, host clock around a synchronise, 4 calls per
          repetition;
  launches of one pass over the nodes, one step and one get_bboxes (torch.profiler, in passes of their own).
Needs a HIP device.

    python scripts/csl_timing.py [out.txt]

The numbers of profiles/csl.md come from this script."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jdet_amd.models  # noqa: E402,F401
from jdet_amd.config.named import CSL_RETINANET_CFG  # noqa: E402
from jdet_amd.models.boxes import coder as K  # noqa: E402
from jdet_amd.models.losses.smooth_focal_loss import csl_angle_loss  # noqa: E402
from jdet_amd.runner import Runner, synthetic_batch  # noqa: E402

REPS = 5
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def name(fused):
    return "fused" if fused else "composed"


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
    """fn(fused) timed REPS times per route, the routes alternating -> {fused: (median, spread)}"""
    ms = {True: [], False: []}
    for fused in (True, False):
        clock(lambda: fn(fused), 2)                          # warm up every shape of the window
    for _ in range(REPS):
        for fused in (True, False):
            ms[fused].append(clock(lambda: fn(fused), n))
    res = {}
    for fused in (True, False):
        res[fused] = (statistics.median(ms[fused]), max(ms[fused]) - min(ms[fused]))
        say("%-6s %-8s median %.3f ms, spread %.3f ms over %d repetitions of %d %s: %s"
            % (label, name(fused), res[fused][0], res[fused][1], REPS, n, unit, " ".join("%.3f" % v for v in ms[fused])))
    return res


dev = torch.device("cuda:0")
images, targets = synthetic_batch(2, 1024, dev, seed=0, num_gts=100)
torch.manual_seed(0)
r = Runner(CSL_RETINANET_CFG, device=dev, graph=False)
head = r.model.bbox_head

# ---- the angle loss alone, on maps of the config's sizes
B, A, BINS = 2, 9, head.coding_len
sizes = [128, 64, 32, 16, 8]
n_level = [A * s * s for s in sizes]
total = sum(n_level)
g = torch.Generator(device="cpu").manual_seed(1)
pos = (torch.rand((B, total), generator=g) < 0.01).float()
bbox_weights = (pos[:, :, None] * torch.ones(5)).to(dev)
bbox_targets = (torch.rand((B, total, 5), generator=g) - 0.25).to(dev) * bbox_weights      # the delta's range: [-0.25, 0.75)
avg = pos.sum().clamp(min=1).to(dev)
levels, start = [], 0
for n in n_level:
    levels.append(dict(x=(torch.randn((B * n, BINS), generator=g) - 4.6).to(dev).requires_grad_(True),
                       bt=bbox_targets[:, start:start + n], bw=bbox_weights[:, start:start + n]))
    start += n
say("nodes: %d anchors x %d bins, %.1f MB of angle logits, %d positive anchors"
    % (B * total, BINS, B * total * BINS * 4 / 1e6, int(pos.sum())))


def nodes(fused):
    K.CSL_FUSED = fused
    losses = [csl_angle_loss(head.loss_angle, head.angle_coder, lv["x"], lv["bt"], lv["bw"], avg) for lv in levels]
    total_loss = torch.stack(losses).sum()
    for lv in levels:
        lv["x"].grad = None
    total_loss.backward()
    return total_loss.detach(), [lv["x"].grad for lv in levels]


(lf, gf), (lc, gc) = nodes(True), nodes(False)
say("nodes: total loss fused %.7f composed %.7f; largest gradient difference over the largest gradient %.3e"
    % (float(lf), float(lc), max(float((a - b).abs().max()) for a, b in zip(gf, gc)) / max(float(a.abs().max()) for a in gf)))
t_nodes = compare("nodes", nodes, device_ms, 20, "forward + backward passes over the five levels")


# ---- the train step
def step(fused):
    K.CSL_FUSED = fused
    return r.train_step(images, targets)


for fused in (True, False):
    ms = host_ms(lambda: step(fused), 3)
    say("warm-up %s: mean of 3 steps %.1f ms" % (name(fused), ms))
t_step = compare("step", step, host_ms, 4, "eager train steps")

# ---- get_bboxes on the outputs of one eval forward
r.model.eval()
with torch.no_grad():
    head.retina_cls.bias.fill_(-2.0)                          # scores above the threshold: the NMS has work
    feats = r.model.neck(r.model.backbone(images))
    from jdet_amd.models.utils.level_pack import run_levels
    outs = tuple(map(list, zip(*run_levels(list(feats), lambda x, mask: head.forward_single(x, mask=mask)))))
    metas = head.parse_targets(targets, is_train=False)


def infer(fused):
    K.CSL_FUSED = fused
    with torch.no_grad():
        return head.get_bboxes(*outs, metas)


ra, rb = infer(True), infer(False)
say("infer: %s detections per image; identical between the routes: %s"
    % ([int(p.shape[0]) for p, _, _ in ra], all(torch.equal(x, y) for a, b in zip(ra, rb) for x, y in zip(a, b))))
t_infer = compare("infer", infer, host_ms, 4, "get_bboxes calls")

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
        say("%-34s %d kernel launches, %d memcpy (%d device -> host), %d memset"
            % (label, len(ev) - len(copies) - len(sets), len(copies), len(d2h), len(sets)))
    r.model.train()
    for what, fn in (("loss_angle, five levels:", nodes), ("one eager step:", step), ("get_bboxes:", infer)):
        for fused in (True, False):
            count(lambda: fn(fused), "%-8s %s" % (name(fused), what))
except Exception as ex:  # noqa: BLE001
    say("launch count: torch.profiler failed: %r" % (ex,))
K.CSL_FUSED = True
d = t_step[False][0] - t_step[True][0]
say("decision: the fused step is %.2f ms %s than the composed one; spread of the repetitions %.2f ms (fused) / %.2f ms "
    "(composed): %s" % (abs(d), "faster" if d > 0 else "slower", t_step[True][1], t_step[False][1],
                        "a win beyond the spread" if d > max(t_step[True][1], t_step[False][1]) else "no win beyond the spread"))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
