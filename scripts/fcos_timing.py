#!/usr/bin/env python3
"""Rotated FCOS at config size: time and launches of the head's dense route against its own general route

  targets   FCOSHead.get_targets, B = 2 images of 1024^2 (21 824 points each), K = 100 gts per image:
            (a) dense: jdet_fcos_targets, one launch;  (b) general: the reference's tensor program per image
  loss      the polygon IoU loss over the 43 648 points of that batch (the positives of (a)), forward + backward to
            the predictions:
            (a) dense: jdet_poly_iou_loss over ALL points, weight = centerness target;
            (b) general: nonzero() + gather of the positives + the tensor program on ops.convex_sort

    python scripts/fcos_timing.py [--out-dir profiles]

writes <out-dir>/fcos_timing.txt.  The driver never opens the GPU: the measurement is one child process under its own
`timeout`; a child that fails ends the run.  Times are device-event means of 100 calls after 10 warm-up calls, taken in
5 rounds that alternate the paths (min .. max over the rounds is the run-to-run spread); launches are the device kernels
the framework profiler records for one call (copies and fills left out; (b)'s host synchronisations are part of its
time).  Latency-bound at these sizes: no roofline fraction is claimed."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LIMIT = 420
ROUNDS, CALLS, WARM = 5, 100, 10


def child(path):
    import numpy as np
    import torch
    from atss_timing import launches, timed
    from jdet_amd.config.named import FCOS_CFG
    from jdet_amd.models.boxes.box_ops import distance2obb
    from jdet_amd.models.losses.poly_iou_loss import poly_iou_loss
    from jdet_amd.models.roi_heads.fcos_head import FCOSHead
    from jdet_amd.runner import synthetic_batch
    dev = torch.device("cuda:0")
    head = FCOSHead(**{k: v for k, v in FCOS_CFG["model"]["roi_heads"].items() if k != "type"})
    sizes = [(1024 // s, 1024 // s) for s in head.strides]
    points = head.get_points(sizes, torch.float32, dev)
    _, targets = synthetic_batch(2, 1024, dev, seed=0, num_gts=100)
    t_paths = {"dense": lambda: head.get_targets(points, targets, dense=True, featmap_sizes=sizes),
               "general": lambda: head.get_targets(points, targets, dense=False)}
    d, g = t_paths["dense"](), t_paths["general"]()
    torch.cuda.synchronize()
    label_differs = int(sum((x != y).sum() for x, y in zip(d[0], g[0])))
    labels, bbox_targets, ctr = head._dense_targets(sizes, [t["rboxes"] for t in targets], [t["labels"] for t in targets])
    labels, bbox_targets, ctr = labels.reshape(-1), bbox_targets.reshape(-1, 5), ctr.reshape(-1)
    pts = torch.cat(points).repeat(2, 1)
    rng = np.random.default_rng(1)
    noise = torch.from_numpy(rng.uniform(0.7, 1.3, (pts.shape[0], 4)).astype(np.float32)).to(dev)
    # predictions: the targets' distances off by up to 30 %, angle off by up to 0.2 rad; background rows get a box too
    pred = torch.cat([bbox_targets[:, :4].clamp(min=0.5) * noise,
                      bbox_targets[:, 4:] + torch.from_numpy(rng.uniform(-0.2, 0.2, (pts.shape[0], 1)).astype(
                          np.float32)).to(dev)], dim=1).requires_grad_(True)

    def dense_loss():
        pred.grad = None
        loss = poly_iou_loss(distance2obb(pts, pred), distance2obb(pts, bbox_targets), weight=ctr, reduction="mean",
                             avg_factor=ctr.sum())
        loss.backward()
        return loss

    def general_loss():
        pred.grad = None
        pos = (labels < head.num_classes).nonzero().reshape(-1)
        w = ctr[pos]
        loss = poly_iou_loss(distance2obb(pts[pos], pred[pos]), distance2obb(pts[pos], bbox_targets[pos]), weight=w,
                             reduction="mean", avg_factor=w.sum(), fused=False)
        loss.backward()
        return loss

    l_paths = {"dense": dense_loss, "general": general_loss}
    vals = {k: float(fn()) for k, fn in l_paths.items()}
    res = dict(points=int(pts.shape[0]), K=100, positives=int((labels < head.num_classes).sum()),
               label_differs=label_differs, loss=vals,
               launches=dict(targets={k: launches(fn) for k, fn in t_paths.items()},
                             loss={k: launches(fn) for k, fn in l_paths.items()}),
               ms=dict(targets={k: [] for k in t_paths}, loss={k: [] for k in l_paths}))
    for _ in range(ROUNDS):
        for k, fn in t_paths.items():
            res["ms"]["targets"][k].append(timed(fn, CALLS, WARM))
        for k, fn in l_paths.items():
            res["ms"]["loss"][k].append(timed(fn, CALLS, WARM))
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
        path = os.path.join(tmp, "fcos.json")
        rc = subprocess.call(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__),
                              "--child", path])
        if rc != 0:
            print("the measurement ended with status %d: nothing more is started on the device" % rc)
            return rc
        with open(path) as f:
            res = json.load(f)
    r = res["result"]
    os.makedirs(args.out_dir, exist_ok=True)
    out = os.path.join(args.out_dir, "fcos_timing.txt")
    with open(out, "w") as f:
        f.write("Rotated FCOS head, steady state.  Written by scripts/fcos_timing.py (%s, torch %s).\n"
                % (res["device"], res["torch"]))
        f.write("B = 2 images of 1024^2: %d points, K = %d gts per image, %d positives (%.1f %%).\n"
                % (r["points"], r["K"], r["positives"], 100.0 * r["positives"] / r["points"]))
        f.write("Device-event mean of %d calls after %d warm-up calls, %d alternating rounds: mean (min .. max) over the "
                "rounds.\nLaunches: device kernels of one call (framework profiler; copies and fills not counted).\n\n"
                % (CALLS, WARM, ROUNDS))
        f.write("%-66s %9s   %-21s %s\n" % ("path", "ms/batch", "(min .. max)", "launches"))
        rows = (("targets", "dense", "get_targets (a) dense: jdet_fcos_targets"),
                ("targets", "general", "get_targets (b) general: tensor program per image"),
                ("loss", "dense", "IoU loss fwd+bwd (a) dense: jdet_poly_iou_loss, all points"),
                ("loss", "general", "IoU loss fwd+bwd (b) general: nonzero + gather + tensor program"))
        for what, key, label in rows:
            ms = r["ms"][what][key]
            f.write("%-66s %9.4f   (%.4f .. %.4f)    %d\n" % (label, sum(ms) / len(ms), min(ms), max(ms),
                                                             r["launches"][what][key]))
        f.write("\nThe two target routes differ on %d of %d labels; the two losses are %.6f (dense) and %.6f (general).\n"
                "Both loss rows include distance2obb of predictions and targets and the backward pass to the predictions.\n"
                % (r["label_differs"], r["points"], r["loss"]["dense"], r["loss"]["general"]))
    print(open(out).read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
