#!/usr/bin/env python3
"""ATSS assignment at config size: time per image and launches per image of

  (a) jdet_atss_assign, fused mode (the IoU of the K x C candidate pairs computed in the kernel);
  (b) jdet_atss_assign, matrix mode, including the jdet_box_iou_rotated launch that fills its (A, K) matrix;
  (c) a literal torch port of the reference's tensor program (models/boxes/assigner.py:L314-391 and
      points_in_rotated_boxes, boxes/box_ops.py:L725-741), held below, on the same IoU op -- the baseline.

    python scripts/atss_timing.py [--out-dir profiles]

writes <out-dir>/atss_assign.txt.  A = 21 824 anchors (1024^2, one anchor per location, the config's generator),
K = 64 gts (the recipe of tests/atss_ref.py, seed 0), topk = 9.  The driver never opens the GPU: the measurement is one
child process under its own `timeout`; a child that fails ends the run.  Times are device-event means of 200 calls
after 20 warm-up calls, taken in 5 rounds that alternate the three paths (the min .. max over the rounds is the
run-to-run spread); launches are the device kernels the framework profiler records for one call (copies and fills
left out; (c)'s host synchronisations are part of its time).  The three paths must agree on gt_inds before anything is
timed.  Launch-latency bound: no roofline fraction is claimed."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT = 420
ROUNDS, CALLS, WARM = 5, 200, 20


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
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and
               not e.name.lower().startswith(("memcpy", "memset")))


def torch_port(bboxes, num_level_bboxes, gt_bboxes, topk, iou):
    """assigner.py:L314-391 line by line (jt -> torch); returns (assigned_gt_inds, max_overlaps)"""
    import torch
    from jdet_amd.models.boxes.box_ops import points_in_rotated_boxes
    num_gt, num_bboxes = gt_bboxes.shape[0], bboxes.shape[0]
    overlaps = iou(bboxes, gt_bboxes)
    assigned_gt_inds = torch.zeros((num_bboxes,), dtype=torch.int32, device=bboxes.device)
    gt_points, bboxes_points = gt_bboxes[:, :2], bboxes[:, :2]
    offsets = bboxes_points[:, None, :] - gt_points[None, :, :]
    distances = offsets.square().sum(-1).sqrt()
    candidate_idxs, start_idx = [], 0
    for bboxes_per_level in num_level_bboxes:
        end_idx = start_idx + bboxes_per_level
        _, topk_idxs_per_level = distances[start_idx:end_idx, :].topk(min(topk, bboxes_per_level), dim=0, largest=False)
        candidate_idxs.append(topk_idxs_per_level + start_idx)
        start_idx = end_idx
    candidate_idxs = torch.cat(candidate_idxs, dim=0)
    ar = torch.arange(num_gt, device=bboxes.device)
    candidate_overlaps = overlaps[candidate_idxs, ar]
    overlaps_mean_per_gt = candidate_overlaps.mean(0)
    std = (candidate_overlaps - overlaps_mean_per_gt[None]).square().sum(0) / (candidate_overlaps.shape[0] - 1)
    overlaps_thr_per_gt = overlaps_mean_per_gt + std.clamp(min=1e-6).sqrt()
    is_pos = candidate_overlaps >= overlaps_thr_per_gt[None, :]
    inside_flag = points_in_rotated_boxes(bboxes_points, gt_bboxes)
    is_pos = is_pos & inside_flag[candidate_idxs, ar]
    for gt_idx in range(num_gt):
        candidate_idxs[:, gt_idx] += gt_idx * num_bboxes
    candidate_idxs = candidate_idxs.view(-1)
    INF = 100000000
    overlaps_inf = torch.full_like(overlaps, -INF).t().contiguous().view(-1)
    index = candidate_idxs.view(-1)[is_pos.view(-1)]
    overlaps_inf[index] = overlaps.t().contiguous().view(-1)[index]
    overlaps_inf = overlaps_inf.view(num_gt, -1).t()
    max_overlaps, argmax_overlaps = overlaps_inf.max(dim=1)
    hit = max_overlaps != -INF
    assigned_gt_inds[hit] = argmax_overlaps[hit].int() + 1
    return assigned_gt_inds, max_overlaps


def child(path):
    import numpy as np
    import torch
    from jdet_amd.models.boxes.assigner import atss_assign_device
    from jdet_amd.ops import box_iou_rotated
    from tests import atss_ref as R
    dev = torch.device("cuda:0")
    anchors, num_level = R.lattice(1024)
    gts = R.random_gts(np.random.default_rng(0), 1024, 64)
    a, g = torch.from_numpy(anchors).to(dev), torch.from_numpy(gts).to(dev)
    paths = {
        "fused": lambda: atss_assign_device(a, num_level, g, R.TOPK),
        "matrix": lambda: atss_assign_device(a, num_level, g, R.TOPK, overlaps=box_iou_rotated(a, g)),
        "torch_port": lambda: torch_port(a, num_level, g, R.TOPK, box_iou_rotated),
    }
    got = {k: fn() for k, fn in paths.items()}
    torch.cuda.synchronize()
    assert torch.equal(got["fused"][0], got["matrix"][0]) and torch.equal(got["fused"][1], got["matrix"][1])
    differ = int((got["fused"][0] != got["torch_port"][0]).sum())
    res = dict(A=int(a.shape[0]), K=int(g.shape[0]), levels=num_level, topk=R.TOPK,
               positives=int((got["fused"][0] > 0).sum()), port_differs=differ,
               launches={k: launches(fn) for k, fn in paths.items()}, ms={k: [] for k in paths})
    for _ in range(ROUNDS):
        for k, fn in paths.items():
            res["ms"][k].append(timed(fn, CALLS, WARM))
    with open(path, "w") as f:
        json.dump(dict(result=res, torch=torch.__version__, device=torch.cuda.get_device_name(0)), f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", help="(internal) measure in this process and write the result here")
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "atss.json")
        rc = subprocess.call(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__),
                              "--child", path])
        if rc != 0:
            print("the measurement ended with status %d: nothing more is started on the device" % rc)
            return rc
        with open(path) as f:
            res = json.load(f)
    r = res["result"]
    os.makedirs(args.out_dir, exist_ok=True)
    out = os.path.join(args.out_dir, "atss_assign.txt")
    names = (("fused", "(a) jdet_atss_assign, fused mode"),
             ("matrix", "(b) jdet_atss_assign, matrix mode + jdet_box_iou_rotated"),
             ("torch_port", "(c) torch port of assigner.py:L314-391 + the IoU op"))
    with open(out, "w") as f:
        f.write("ATSS assignment, per image, steady state.  Written by scripts/atss_timing.py (%s, torch %s).\n"
                % (res["device"], res["torch"]))
        f.write("A = %d anchors (levels %s), K = %d gts, topk = %d, %d positives.\n"
                % (r["A"], r["levels"], r["K"], r["topk"], r["positives"]))
        f.write("Device-event mean of %d calls after %d warm-up calls, %d alternating rounds: mean (min .. max) over the "
                "rounds.\nLaunches: device kernels of one call (framework profiler; copies and fills not counted).\n\n"
                % (CALLS, WARM, ROUNDS))
        f.write("%-62s %9s   %-21s %s\n" % ("path", "ms/image", "(min .. max)", "launches/image"))
        for key, label in names:
            ms = r["ms"][key]
            f.write("%-62s %9.4f   (%.4f .. %.4f)    %d\n" % (label, sum(ms) / len(ms), min(ms), max(ms),
                                                             r["launches"][key]))
        f.write("\n(a) and (b) agree bit for bit on gt_inds and max_overlaps; (c) differs from them on %d of %d anchors "
                "(its topk / argmax tie orders and fp32 atan2 inside test are the framework's).\n"
                "Launch-latency bound at this size; no roofline fraction is claimed.\n" % (r["port_differs"], r["A"]))
    print(open(out).read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
