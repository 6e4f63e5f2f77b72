#!/usr/bin/env python3
"""Localization distillation at config size: LD_RETINANET_CFG (R50 teacher, R18 student) at 2 x 1024^2 with 64 gts per
image, the fused level nodes (csrc/dist_loss.hip) against the composed routes (JDET_LOSS_LEVEL_NODES=0) in one process,
alternating --
  step    one eager train step, host clock around a synchronise, three rounds of six steps after warm-up;
  nodes   loss_bbox + loss_LD + loss_KD of all five levels, forward and backward, on synthetic maps of the config's
          sizes (392 832 anchors x 45 regression / 15 class logits, about 1 % positive anchors, every label weight 1),
          device events around 40 calls, three alternating rounds;
  launches of one step and of one pass over the nodes (torch.profiler, in a pass of their own).
Needs a HIP device.

    python scripts/ld_timing.py [out.txt]

The numbers of profiles/ld.md come from this script."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jdet_amd.models  # noqa: E402,F401
from jdet_amd.config.named import LD_RETINANET_CFG  # noqa: E402
from jdet_amd.models.losses import _level  # noqa: E402
from jdet_amd.models.losses.dist_bbox_loss import dist_bbox_loss  # noqa: E402
from jdet_amd.runner import Runner, synthetic_batch  # noqa: E402

out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def name(fused):
    return "fused" if fused else "composed"


dev = torch.device("cuda:0")
images, targets = synthetic_batch(2, 1024, dev, seed=0, num_gts=64)
torch.manual_seed(0)
r = Runner(LD_RETINANET_CFG, device=dev, graph=False)
head = r.model.bbox_head


def steps(n, fused):
    _level.LEVEL_NODES = fused
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        loss, parts = r.train_step(images, targets)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, {k: round(float(v), 5) for k, v in parts.items()}


for fused in (True, False):
    ms, parts = steps(3, fused)
    say("warm-up %s: mean of 3 steps %.1f ms %s" % (name(fused), ms, parts))
for rnd in range(3):
    for fused in (True, False):
        ms, _ = steps(6, fused)
        say("round %d step %-8s %.2f ms/step (6 steps, host clock around a synchronise)" % (rnd, name(fused), ms))

# ---- the three loss nodes alone, on maps of the config's sizes
B, A, BINS, C = 2, 9, 9, 15
sizes = [128, 64, 32, 16, 8]
n_level = [A * s * s for s in sizes]
total = sum(n_level)
g = torch.Generator(device="cpu").manual_seed(1)
pos = (torch.rand((B, total), generator=g) < 0.01).float()
bbox_weights = (pos[:, :, None] * torch.ones(5)).to(dev)
bbox_targets = (torch.randn((B, total, 5), generator=g) * 0.5).to(dev) * bbox_weights
label_weights = torch.ones((B, total), device=dev)
avg = pos.sum().clamp(min=1).to(dev)
levels, start = [], 0
for n in n_level:
    mk = lambda k, scale: (torch.randn((B * n, k), generator=g) * scale).to(dev)  # noqa: E731
    levels.append(dict(reg=mk(5 * BINS, 1.0).requires_grad_(True), reg_t=mk(5 * BINS, 1.0),
                       cls=mk(C, 1.0).requires_grad_(True), cls_t=mk(C, 1.0),
                       bt=bbox_targets[:, start:start + n], bw=bbox_weights[:, start:start + n],
                       lw=label_weights[:, start:start + n]))
    start += n
say("nodes: %d anchors, %.1f MB of regression logits, %.1f MB of class logits, %d positive anchors"
    % (B * total, B * total * 45 * 4 / 1e6, B * total * C * 4 / 1e6, int(pos.sum())))


def nodes(fused):
    _level.LEVEL_NODES = fused
    losses = []
    for lv in levels:
        losses.append(dist_bbox_loss(head.loss_bbox, lv["reg"], lv["bt"], lv["bw"], avg, BINS - 1))
        losses.append(head.loss_ld(lv["reg"].reshape(-1, BINS), lv["reg_t"].reshape(-1, BINS), lv["bw"], avg_factor=avg))
        losses.append(head.loss_kd(lv["cls"], lv["cls_t"], lv["lw"], avg_factor=avg))
    total_loss = torch.stack(losses).sum()
    for lv in levels:
        lv["reg"].grad = lv["cls"].grad = None
    total_loss.backward()
    return total_loss.detach(), [lv["reg"].grad for lv in levels]


def timed(fused, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        nodes(fused)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


(lf, gf), (lc, gc) = nodes(True), nodes(False)
say("nodes: total loss fused %.6f composed %.6f; largest gradient difference over the largest gradient %.3e"
    % (float(lf), float(lc), max(float((a - b).abs().max()) for a, b in zip(gf, gc)) / max(float(a.abs().max()) for a in gf)))
for fused in (True, False):
    timed(fused, 5)
for rnd in range(3):
    for fused in (True, False):
        ms = timed(fused, 40)
        say("round %d nodes %-8s %.3f ms per forward + backward of the 15 loss terms (40 calls between device events, "
            "window %.0f ms)" % (rnd, name(fused), ms, ms * 40))

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
        say("%-30s %d kernel launches, %d memcpy (%d device -> host), %d memset"
            % (label, len(ev) - len(copies) - len(sets), len(copies), len(d2h), len(sets)))
    for fused in (True, False):
        count(lambda: nodes(fused), "%-8s 15 loss terms:" % name(fused))
    for fused in (True, False):
        _level.LEVEL_NODES = fused
        count(lambda: r.train_step(images, targets), "%-8s one eager step:" % name(fused))
except Exception as ex:  # noqa: BLE001
    say("launch count: torch.profiler failed: %r" % (ex,))
_level.LEVEL_NODES = True
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
