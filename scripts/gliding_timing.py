#!/usr/bin/env python3
"""Gliding Vertex: train-step time and launch count beside Oriented R-CNN, launch count of the head's target pass
(fused kernel vs torch composition), and the error figures of the fused codecs against the numpy restatement.

    python scripts/gliding_timing.py [--out-dir profiles]

writes <out-dir>/gliding_step.md and <out-dir>/gliding_codecs.md from one run.  The driver itself never opens the GPU:
every measurement is a child process of its own under its own `timeout`, one at a time, and the first child that
fails (non-zero status, time limit included) ends the run -- nothing more is started on the device after a fault.
Times are device-event means over eager steps at 2 x 1024^2 with 64 gts per image (`synthetic_batch`); launches are
the device kernels the framework profiler records for one step (copy and fill records left out).  The fused codecs
are launch-latency bound (<= 1024 rows in training, <= 2000 x 15 (row, class) pairs at inference): their figure of
merit is the launch count, no roofline fraction is claimed."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("codecs", 120), ("targets", 120), ("gliding", 420), ("orcnn", 420))      # name, time limit in seconds


def timed(fn, n, warm):
    import torch
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
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    # kernels only: the profiler also records copies and fills as device events
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and
               not e.name.lower().startswith(("memcpy", "memset")))


def step_codecs(dev):
    import numpy as np
    import torch
    from jdet_amd.models.boxes.coder import gliding_decode, gliding_targets
    from tests import gliding_ref as R      # the inputs of tests/test_gpu_gliding.py come from the same helpers
    f32 = np.float32
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dev)     # noqa: E731
    rois, polys = R.target_case()
    a64 = R.targets(rois, polys, R.MEANS, R.STDS)
    a32 = R.targets(rois.astype(f32), polys.astype(f32), R.MEANS, R.STDS)
    got = gliding_targets(to(rois), to(polys), R.MEANS, R.STDS)
    out = []
    for name, g, x32, x64 in zip(("bbox_targets", "fix_targets", "ratio_targets"), got, a32, a64):
        out.append(dict(output="jdet_gliding_targets " + name, rows=4000,
                        spread=float(np.abs(x32.astype(np.float64) - x64).max()),
                        kernel_error=float(np.abs(g.cpu().numpy().astype(np.float64) - x64).max())))
    scale = (1.25, 0.8, 1.25, 0.8)
    for max_shape in (None, (1024, 1024)):
        args = R.decode_case()
        x64 = R.decode_polys(*args, R.MEANS, R.STDS, max_shape, ratio_thr=0.8, scale=scale)
        x32 = R.decode_polys(*(a.astype(f32) for a in args), R.MEANS, R.STDS, max_shape, ratio_thr=0.8, scale=scale)
        g = gliding_decode(*(to(a) for a in args), R.MEANS, R.STDS, max_shape=max_shape, ratio_thr=0.8, scale=scale)
        out.append(dict(output="jdet_gliding_decode polys (C = 15, max_shape %s)" % (max_shape,), rows=300,
                        spread=float(np.abs(x32.astype(np.float64) - x64).max()),
                        kernel_error=float(np.abs(g.cpu().numpy().astype(np.float64) - x64).max())))
    return out


def step_targets(dev):
    """the head's target pass at config size (2 images x 512 rows)"""
    import numpy as np
    import torch
    from jdet_amd.models.boxes.coder import gliding_targets
    from tests import gliding_ref as R
    rois, polys = R.target_case(1024, seed=1)
    r, p = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in (rois, polys))
    means, stds = R.MEANS, R.STDS
    out = {}
    for name, fused in (("fused", True), ("composition", False)):
        fn = lambda: gliding_targets(r, p, means, stds, fused=fused)     # noqa: E731
        out[name] = dict(launches=launches(fn), ms=timed(fn, 200, 20))
    return out


def step_train(dev, cfg_name):
    import torch
    from jdet_amd.config import named
    from jdet_amd.runner import Runner, synthetic_batch
    torch.manual_seed(0)
    r = Runner(getattr(named, cfg_name), device=dev, conv_autotune=False)
    images, targets = synthetic_batch(2, 1024, dev)
    images = images.contiguous(memory_format=torch.channels_last)
    fn = lambda: r.train_step(images, targets)     # noqa: E731
    ms = timed(fn, 20, 5)
    return dict(config=cfg_name, ms=ms, launches=launches(fn), loss=float(fn()[0]))


def child(step, path):
    import torch
    dev = torch.device("cuda:0")
    res = {"codecs": lambda: step_codecs(dev), "targets": lambda: step_targets(dev),
           "gliding": lambda: step_train(dev, "GLIDING_CFG"), "orcnn": lambda: step_train(dev, "ORCNN_CFG")}[step]()
    with open(path, "w") as f:
        json.dump(dict(result=res, torch=torch.__version__, device=torch.cuda.get_device_name(0)), f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="(internal) run one measurement in this process")
    ap.add_argument("--json", help="(internal) where the child writes its result")
    args = ap.parse_args()
    if args.step:
        return child(args.step, args.json)
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in STEPS:
            path = os.path.join(tmp, step + ".json")
            rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
                                  "--step", step, "--json", path])
            if rc != 0:
                print("step %s ended with status %d: nothing more is started on the device" % (step, rc))
                return rc
            with open(path) as f:
                res[step] = json.load(f)
            print(step, json.dumps(res[step]["result"]), flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    env = "%s, torch %s" % (res["gliding"]["device"], res["gliding"]["torch"])
    g, o, t = res["gliding"]["result"], res["orcnn"]["result"], res["targets"]["result"]
    with open(os.path.join(args.out_dir, "gliding_step.md"), "w") as f:
        f.write("# Gliding Vertex train step\n\nWritten by `scripts/gliding_timing.py` (%s).  Eager steps, 2 x 1024^2 "
                "images, 64 gts per image (`synthetic_batch`),\nmean of 20 steps after 5 warm-up steps (device events); "
                "launches = device kernels of one step (framework profiler, copies and fills not counted).\n"
                "One run, one process per row.\n\n" % env)
        f.write("| config | step time (ms) | launches per step | loss of the last step |\n|---|---|---|---|\n")
        for r in (g, o):
            f.write("| `%s` | %.1f | %d | %.3f |\n" % (r["config"], r["ms"], r["launches"], r["loss"]))
        f.write("\n## Target pass of the head (1024 rows: 2 images x 512)\n\n"
                "| path | launches | time per call (ms) |\n|---|---|---|\n")
        f.write("| `jdet_gliding_targets` (fused) | %d | %.4f |\n" % (t["fused"]["launches"], t["fused"]["ms"]))
        f.write("| torch composition (`fused=False`) | %d | %.4f |\n" % (t["composition"]["launches"],
                                                                        t["composition"]["ms"]))
        f.write("\nThe fused codecs are launch-latency bound at these sizes; no roofline fraction is claimed.\n")
    with open(os.path.join(args.out_dir, "gliding_codecs.md"), "w") as f:
        f.write("# Fused Gliding Vertex codecs against the restatement\n\nWritten by `scripts/gliding_timing.py` (%s).  "
                "Inputs and bounds are those of\n`tests/test_gpu_gliding.py`: the restatement (`tests/gliding_ref.py`) "
                "runs in float32 and in float64 on the same inputs;\n`spread` is the largest difference between the "
                "two, the kernel is allowed max(4 x spread, 1e-6) against the float64 values.\n\n" % env)
        f.write("| output | rows | float32-vs-float64 spread | bound | kernel max error |\n|---|---|---|---|---|\n")
        for r in res["codecs"]["result"]:
            f.write("| %s | %d | %.3e | %.3e | %.3e |\n" % (r["output"], r["rows"], r["spread"],
                                                          max(4 * r["spread"], 1e-6), r["kernel_error"]))
    print("wrote", os.path.join(args.out_dir, "gliding_step.md"), os.path.join(args.out_dir, "gliding_codecs.md"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
