#!/usr/bin/env python3
"""RetinaNet-v1d at config size: RETINANET_V1D_DOTA_CFG (Resnet50_v1d, bilinear FPN, RetinaHead on 280 203 anchors) at
3 x 800^2 with 64 gts per image, each fused route (csrc/retina.hip, csrc/upsample_add_bilinear.hip) against its composed
route in one process, alternating, after a warm-up of every shape --
  targets   assignment + encoded targets + focal / smooth-L1 of the three images, forward and backward, on synthetic head
            outputs of the config's sizes; device events around 100 calls, three alternating rounds;
  merges    the top-down merges of the config's neck (start_level 1: two merges, 25^2 -> 50^2 -> 100^2, 256 channels),
            forward and backward; device events around 200 calls;
  detect    get_bboxes of one image, (a) logits at the head's bias prior (nothing passes the score threshold), (b) logits
            shifted until about 1 % of the 4.2 M scores pass; host clock around a synchronise (the routes synchronise
            themselves), 50 calls;
  step      one eager train step, host clock around a synchronise, three rounds of 4 steps;
  launches  of each of the above (torch.profiler, in passes of their own).
Needs a HIP device.

    python scripts/retinanet_timing.py [output directory, default profiles/]

Writes retinanet_timing.txt (the raw lines) and retinanet.md (the tables and the decision) there."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jdet_amd.models  # noqa: E402,F401
from jdet_amd.config.named import RETINANET_V1D_DOTA_CFG  # noqa: E402
from jdet_amd.ops import upsample_add as UA  # noqa: E402
from jdet_amd.runner import Runner, synthetic_batch  # noqa: E402

OUT_DIR = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
out, table = [], {}


def say(s):
    print(s, flush=True)
    out.append(s)


def name(fused):
    return "fused" if fused else "composed"


def route(fused):
    os.environ["JDET_RETINA_FUSED"] = "1" if fused else "0"


def events(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def host(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
    copies = [e for e in ev if e.name.lower().startswith("memcpy")]
    sets = [e for e in ev if e.name.lower().startswith("memset")]
    return len(ev) - len(copies) - len(sets), len(copies), len(sets)


def compare(key, what, run, timer, n, rounds=3):
    """run(fused) alternating; table[key] = {route: [ms per round]}"""
    table[key] = {True: [], False: [], "what": what}
    for fused in (True, False):
        timer(lambda: run(fused), 2)
    for rnd in range(rounds):
        for fused in (True, False):
            ms = timer(lambda: run(fused), n)
            table[key][fused].append(ms)
            say("round %d %-26s %-8s %.3f ms (%d calls, window %.1f ms)" % (rnd, what, name(fused), ms, n, ms * n))
    try:
        table[key]["launches"] = {f: launches(lambda: run(f)) for f in (True, False)}
        for f in (True, False):
            say("%-26s %-8s %d kernel launches, %d memcpy, %d memset" % ((what, name(f)) + table[key]["launches"][f]))
    except Exception as ex:  # noqa: BLE001
        say("launch count of %s: torch.profiler failed: %r" % (what, ex))


dev = torch.device("cuda:0")
B, SIZE, GTS = 3, 800, 64
images, targets = synthetic_batch(B, SIZE, dev, seed=0, num_gts=GTS)
torch.manual_seed(0)
r = Runner(RETINANET_V1D_DOTA_CFG, device=dev, graph=False, conv_autotune=False)
head, neck = r.model.rpn_net, r.model.neck
sizes = [(100, 100), (50, 50), (25, 25), (13, 13), (7, 7)]
anchors = head.anchors_of(sizes, dev)
A, C = anchors.shape[0], head.n_class
say("config size: batch %d x %d^2, %d gts per image, %d anchors per image, %d classes" % (B, SIZE, GTS, A, C))

# ---- targets + losses
g = torch.Generator(device="cpu").manual_seed(1)
bbox_pred = (torch.randn((B, A, 5), generator=g) * 0.1).to(dev).requires_grad_(True)
cls_score = (torch.randn((B, A, C), generator=g) * 0.05 - 4.595).to(dev).requires_grad_(True)


def loss_pass(fused):
    bbox_pred.grad = cls_score.grad = None
    if fused:
        losses = head.loss_fused(bbox_pred, cls_score, anchors, targets)
    else:
        t = head.composed_targets(anchors, targets)
        losses = head.losses(list(bbox_pred), list(cls_score), [x[0] for x in t], [x[1] for x in t])
    (losses["roi_cls_loss"] + losses["roi_loc_loss"]).backward()
    return {k: float(v) for k, v in losses.items()}


say("targets + losses: fused %s composed %s" % (loss_pass(True), loss_pass(False)))
compare("targets", "targets + losses fwd+bwd", loss_pass, events, 100)

# ---- the top-down merges
cl = torch.channels_last
laterals = [torch.randn((B, 256, h, w), generator=g).to(dev).contiguous(memory_format=cl).requires_grad_(True)
            for h, w in sizes[:3]]
keep_fusable = UA.fusable


def merges(fused):
    UA.fusable = keep_fusable if fused else (lambda a, b: False)
    try:
        for t in laterals:
            t.grad = None
        merged = neck._top_down(laterals)
        torch.autograd.backward([merged[0]], [torch.ones_like(merged[0])])
    finally:
        UA.fusable = keep_fusable


compare("merges", "2 FPN merges fwd+bwd", merges, events, 200)

# ---- get_bboxes of one image
meta = [dict(img_size=(SIZE, SIZE), ori_img_size=(SIZE, SIZE))]
loc1 = (torch.randn((1, A, 5), generator=g) * 0.1).to(dev)
prior = (torch.randn((1, A, C), generator=g) * 0.05 - 4.595).to(dev)
shifted = (torch.randn((1, A, C), generator=g) - 5.27).to(dev)
head.eval()
for label, logits in (("prior", prior), ("shifted", shifted)):
    passed = float((logits.sigmoid() > head.score_thresh).float().mean())

    def detect(fused, logits=logits):
        route(fused)
        with torch.no_grad():
            return head.get_bboxes(anchors, loc1, logits, meta)[0]
    kept = [detect(f)[0].shape[0] for f in (True, False)]
    say("get_bboxes %s: %.3f %% of the scores pass; detections kept fused %d composed %d" % (label, 100 * passed, *kept))
    compare("detect_" + label, "get_bboxes (%s logits)" % label, detect, host, 50)
head.train()

# ---- the train step
def step(fused):
    route(fused)
    return r.train_step(images, targets)


for fused in (True, False):
    ms = host(lambda: step(fused), 3)
    say("warm-up %s: mean of 3 steps %.1f ms" % (name(fused), ms))
compare("step", "train step", step, host, 4)
route(True)

# ---- the files
os.makedirs(OUT_DIR, exist_ok=True)
open(os.path.join(OUT_DIR, "retinanet_timing.txt"), "w").write("\n".join(out) + "\n")
md = ["# RetinaNet-v1d (`RETINANET_V1D_DOTA_CFG`): the fused routes against their composed routes", "",
      "Measured on one MI355X with `python scripts/retinanet_timing.py` (raw lines: `retinanet_timing.txt`): one process, the",
      "two routes alternating, every shape warmed up first.  Batch %d x 3 x %d², %d gts per image (`synthetic_batch`)," % (B, SIZE, GTS),
      "Resnet50_v1d, %d anchors per image, eager steps, MIOpen's heuristic solver pick (`conv_autotune=False`)." % A,
      "Ranges are the three rounds' values; kernel times were not traced, so no share of peak is claimed.  The windows of the",
      "head-only measurements are short (see the raw lines): they resolve the factors between the routes, not the third digit.",
      "Findings that are not timings are in `retinanet_notes.md`.", "",
      "| measurement | route | round 0 | round 1 | round 2 | kernel launches | memcpy | memset |", "|---|---|---|---|---|---|---|---|"]
decisions = []
for key in ("targets", "merges", "detect_prior", "detect_shifted", "step"):
    t = table.get(key)
    if not t:
        continue
    for f in (True, False):
        ln = t.get("launches", {}).get(f, ("not measured",) * 3)
        md.append("| %s | %s | %s | %s | %s | %s |" % (t["what"], name(f), " | ".join("%.3f ms" % v for v in t[f]), *ln))
    slower = min(t[True]) > max(t[False])
    decisions.append("- %s: fused %.3f - %.3f ms, composed %.3f - %.3f ms: the fused route is %s." % (
        t["what"], min(t[True]), max(t[True]), min(t[False]), max(t[False]),
        "SLOWER beyond the run-to-run range" if slower else "not slower beyond the run-to-run range"))
md += ["", "## Decision", "", "A fused route is the default when it is not slower than the composed one beyond the run-to-run range:", ""]
md += decisions
open(os.path.join(OUT_DIR, "retinanet.md"), "w").write("\n".join(md) + "\n")
