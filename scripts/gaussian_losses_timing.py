#!/usr/bin/env python3
"""Timing and accuracy of the Gaussian box losses (round 7): writes profiles/r07_gaussian_losses.txt.

    python scripts/gaussian_losses_timing.py time --commit <sha> [--out profiles/r07_gaussian_losses.txt]
        1. per level (P3 of 2 x 1024^2: 294912 rows, ~10 % positive): forward + backward of the fused node against the
           package's torch composition on the same inputs (device events; launches counted by the framework profiler)
        2. the same two, kernel by kernel, from `rocprofv3 --kernel-trace --stats` runs of their own (child processes
           running the `level-node` / `level-comp` modes below), summarised into the file
        3. train step (eager, ms and img/s) of GWD / KLD / KFIoU RetinaNet against RETINANET_CFG at 2 x 1024^2
        4. launches per GWD step with the dense decoded-target route against the per-image route
        5. the kernel against the float64 restatement, every case of tests/test_gpu_gaussian_losses.py: measured loss
           relative error and gradient max error / max|g_ref| next to the bounds the test holds it to
    python scripts/gaussian_losses_timing.py level-node | level-comp
        ten forward + backward passes of one level per loss, node or composition only (what the trace runs execute)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def level_inputs(dev, n_img=2, A=128 * 128 * 9, seed=0):
    rng = np.random.default_rng(seed)
    anchors = np.concatenate([rng.uniform(0, 1024, (A, 2)), np.exp(rng.uniform(np.log(16), np.log(256), (A, 2))),
                              np.zeros((A, 1))], 1).astype(np.float32)
    deltas = rng.normal(0, 0.3, (n_img * A, 5)).astype(np.float32)
    tdel = rng.normal(0, 0.3, (n_img, A, 5)).astype(np.float32)
    weight = np.zeros((n_img, A, 5), np.float32)
    weight[rng.uniform(size=(n_img, A)) < 0.1] = 1.0
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    return t(anchors), t(deltas), t(tdel), t(weight)


def level_cases(dev):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.models.boxes.coder import DeltaXYWHABBoxCoder
    from jdet_amd.utils.registry import LOSSES, build_from_cfg
    a, d, tdel, w = level_inputs(dev)
    coder = DeltaXYWHABBoxCoder()
    gt = coder.decode(a.repeat(2, 1), tdel.reshape(-1, 5)).reshape(tdel.shape)
    avg = torch.tensor(float((w.mean(-1) > 0).sum()), device=dev)
    out = []
    for name, cfg, decoded in (("GDLoss gwd", dict(type="GDLoss", loss_type="gwd", loss_weight=5.0), True),
                               ("GDLoss_v1 kld", dict(type="GDLoss_v1", loss_type="kld", fun="log1p", tau=1.0,
                                                      loss_weight=5.5), True),
                               ("KFLoss", dict(type="KFLoss", loss_weight=5.0), False)):
        loss = build_from_cfg(cfg, LOSSES)
        tgt = gt if decoded else tdel
        x = d.clone().requires_grad_(True)

        def node(loss=loss, tgt=tgt, x=x, decoded=decoded):
            loss.level(x, a[None].expand(2, -1, 5), tgt, w, avg, coder, decoded).backward()

        def comp(loss=loss, tgt=tgt, x=x, decoded=decoded):
            loss._composed(x, a, tgt.reshape(-1, 5), w.reshape(-1, 5), avg, coder, decoded).backward()
        out.append((name, node, comp))
    return out


def rocprof_summary(dev_mode, tmp):
    """kernel launches and summed kernel time of one `level-*` run under rocprofv3 (its own process), per pass"""
    import csv
    import glob
    d = os.path.join(tmp, dev_mode)
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "r07", "--",
                        sys.executable, os.path.abspath(__file__), dev_mode], capture_output=True, text=True,
                       timeout=240)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return ["   %s: rocprofv3 failed (rc %d)" % (dev_mode, r.returncode)]
    rows = list(csv.DictReader(open(files[0])))
    passes = 3 * 10      # three losses x ten forward + backward passes
    calls = sum(int(x["Calls"]) for x in rows)
    total_ns = sum(float(x["TotalDurationNs"]) for x in rows)
    out = ["   %s: %d kernel launches, %.1f us kernel time per forward + backward (%d kernel names); top 5:"
           % (dev_mode, round(calls / passes), total_ns / passes / 1e3, len(rows))]
    for x in sorted(rows, key=lambda x: -float(x["TotalDurationNs"]))[:5]:
        out.append("      %6d calls %9.1f us  %s" % (int(x["Calls"]), float(x["TotalDurationNs"]) / 1e3, x["Name"][:90]))
    return out


def accuracy(dev):
    """the kernel against the float64 restatement, case by case (tests/test_gpu_gaussian_losses.py: CASES)"""
    from jdet_amd.models.boxes.box_ops import delta2bbox_rotated
    from jdet_amd.models.boxes.coder import DeltaXYWHABBoxCoder
    from tests import gaussian_loss_ref as R
    from tests import test_gpu_gaussian_losses as T
    out = []
    for kind, cfg, kw, decoded, ltol, gtol in T.CASES:
        loss = T._build(cfg)
        anchors, deltas, tdel, weight = T._level_inputs(np.random.default_rng(5))
        n_img, A = tdel.shape[:2]
        all_anc = np.tile(anchors, (n_img, 1))
        if kind == "kfiou":
            target = tdel
        elif decoded:
            target = delta2bbox_rotated(torch.from_numpy(all_anc).to(dev),
                                        torch.from_numpy(tdel.reshape(-1, 5)).to(dev)).cpu().numpy().reshape(n_img, A, 5)
        else:
            rep = anchors[None].repeat(n_img, 0)
            target = np.concatenate([rep[..., :2] + tdel[..., :2] * 8, rep[..., 2:4] * np.exp(tdel[..., 2:4]),
                                     rep[..., 4:] + tdel[..., 4:]], -1).astype(np.float32)
        pred = deltas if (decoded or kind == "kfiou") else delta2bbox_rotated(
            torch.from_numpy(all_anc).to(dev), torch.from_numpy(deltas).to(dev)).cpu().numpy()
        avg = torch.tensor(float((weight.mean(-1) > 0).sum()) + 3.0, device=dev)
        p = torch.from_numpy(pred).to(dev).requires_grad_(True)
        o = loss.level(p, torch.from_numpy(anchors).to(dev)[None].expand(n_img, A, 5), T._windows(dev, target),
                       T._windows(dev, weight), avg, DeltaXYWHABBoxCoder(), decoded)
        o.backward()
        want, gwant = R.masked_loss_and_grad(kind, pred, target.reshape(-1, 5), weight.reshape(-1, 5), float(avg),
                                             cfg.get("loss_weight", 1.0), anchors=all_anc, decode_pred=decoded, **kw)
        lerr = abs(float(o.detach()) - want) / max(abs(want), 1e-30)
        gerr = float(np.abs(p.grad.cpu().numpy() - gwant).max() / max(np.abs(gwant).max(), 1e-30))
        args = ", ".join("%s=%r" % kv for kv in cfg.items() if kv[0] not in ("type", "loss_weight"))
        out.append("   %-9s %-42s %-7s %9.2e (<= %.0e)  %9.2e (<= %.0e)"
                   % (cfg["type"], args[:42], "decoded" if decoded or kind == "kfiou" else "boxes", lerr, ltol, gerr,
                      gtol))
    return out


def timed(fn, n=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def step_fn(cfg, dev, images, targets):
    from jdet_amd.runner import Runner
    torch.manual_seed(0)
    r = Runner(cfg, device=dev, conv_autotune=False)
    return lambda: r.train_step(images, targets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "level-node", "level-comp"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_gaussian_losses.txt"))
    ap.add_argument("--commit", default="unknown", help="the tree's commit (the GPU box has no repository)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.mode.startswith("level"):
        for name, node, comp in level_cases(dev):
            for _ in range(10):
                (node if args.mode == "level-node" else comp)()
        torch.cuda.synchronize()
        return
    from jdet_amd.config import named
    from jdet_amd.models.boxes import anchor_target as AT
    from jdet_amd.runner import synthetic_batch
    lines = ["Gaussian box losses (round 7) -- MI355X, torch %s, tree: %s" % (torch.__version__, args.commit),
             "written by scripts/gaussian_losses_timing.py time", ""]
    lines.append("1. one pyramid level (P3 of 2 x 1024^2: 294912 rows, ~10 % positive), forward + backward")
    lines.append("   %-14s %22s %22s" % ("loss", "fused node", "torch composition"))
    for name, node, comp in level_cases(dev):
        tn, tc = timed(node), timed(comp, n=10)
        ln, lc = launches(node), launches(comp)
        lines.append("   %-14s %9.3f ms %4d launches %9.3f ms %4d launches" % (name, tn, ln, tc, lc))
    import tempfile
    lines += ["", "2. the same level work under rocprofv3 --kernel-trace --stats (runs of their own, 3 losses x 10 passes)"]
    with tempfile.TemporaryDirectory() as tmp:
        for mode in ("level-node", "level-comp"):
            lines += rocprof_summary(mode, tmp)
    images, targets = synthetic_batch(2, 1024, dev, seed=3, num_gts=64)
    lines += ["", "3. train step, eager, 2 x 1024^2, 64 gts per image (Runner.train_step, 20 steps after 5)"]
    for name in ("RETINANET_CFG", "GWD_RETINANET_CFG", "KLD_RETINANET_CFG", "KFIOU_RETINANET_CFG"):
        fn = step_fn(getattr(named, name), dev, images, targets)
        ms = timed(fn, n=20, warm=5)
        lines.append("   %-20s %8.2f ms  %6.1f img/s  %5d launches" % (name, ms, 2e3 / ms, launches(fn)))
    lines += ["", "4. GWD step launches: dense decoded targets vs the per-image route they replace"]
    fn = step_fn(named.GWD_RETINANET_CFG, dev, images, targets)
    dense_n, dense_ms = launches(fn), timed(fn, n=20, warm=5)
    orig = AT._dense_ok
    AT._dense_ok = lambda cfg, *a: (not cfg.get("reg_decoded_bbox", False)) and orig(cfg, *a)
    try:
        per_n, per_ms = launches(fn), timed(fn, n=20, warm=5)
    finally:
        AT._dense_ok = orig
    lines.append("   dense decoded targets : %5d launches  %8.2f ms" % (dense_n, dense_ms))
    lines.append("   per-image targets     : %5d launches  %8.2f ms (nonzero + index scatters + host syncs)"
                 % (per_n, per_ms))
    lines += ["", "5. kernel vs float64 restatement (tests/test_gpu_gaussian_losses.py CASES: 2 x 10000 rows, ~10 % positive,",
              "   hand-built clamp / w = h / angle-wrap rows); loss relative error, gradient max error / max|g_ref|",
              "   %-9s %-42s %-7s %22s %22s" % ("loss", "arguments", "pred", "loss rel. err (bound)", "grad err (bound)")]
    lines += accuracy(dev)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("done in %.0f s" % (time.time() - t0))
