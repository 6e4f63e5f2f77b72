"""The dense side of RetinaHead on the device (csrc/retina.hip, include/jdet_hip_retina.h): ground-truth preparation,
one-pass assignment + encoded targets for the whole batch, and the decode / threshold / compaction in front of the
per-class NMS.  Device tensors only, as every op here; models/roi_heads/retina_head.py holds the composed tensor program
of the same rules."""
import torch

from .. import _lib as L


def gt_prepare(gts):
    """raw gts (K, 5) [x, y, w, h, a] -> (rboxes (K, 5), rboxes_h (K, 4)) as RetinaNet.execute makes them"""
    L.need_device(gts)
    g = L.f32c(gts)
    K = g.shape[0]
    rboxes = torch.empty((K, 5), dtype=torch.float32, device=g.device)
    rboxes_h = torch.empty((K, 4), dtype=torch.float32, device=g.device)
    L.check(L.lib().jdet_retina_gt_prepare(L.ptr(g), K, L.ptr(rboxes), L.ptr(rboxes_h), L.stream_ptr(g)),
            "jdet_retina_gt_prepare")
    return rboxes, rboxes_h


def targets(anchors, rboxes, rboxes_h, gt_labels, gt_offsets, pos_iou_thresh, neg_iou_thresh_hi, neg_iou_thresh_lo):
    """anchors (A, 4); the prepared gts of all images packed (sum K, 5 | 4 | ) with gt_offsets (N + 1) int32 on the device
    -> dict(labels, label_weights, loc_targets, loc_weights, raw_labels, normalizer) in the layouts of the header"""
    L.need_device(anchors, rboxes, rboxes_h, gt_labels, gt_offsets)
    a, rb, rh = L.f32c(anchors), L.f32c(rboxes), L.f32c(rboxes_h)
    lab = gt_labels.to(torch.int32).contiguous()
    off = gt_offsets.to(torch.int32).contiguous()
    A, N, total = a.shape[0], off.numel() - 1, rb.shape[0]
    dev = a.device
    out = dict(labels=torch.empty((N, A), dtype=torch.int32, device=dev),
               label_weights=torch.empty((N, A), dtype=torch.float32, device=dev),
               loc_targets=torch.empty((N, A, 5), dtype=torch.float32, device=dev),
               loc_weights=torch.empty((N, A, 5), dtype=torch.float32, device=dev),
               raw_labels=torch.empty((N, A), dtype=torch.int32, device=dev),
               normalizer=torch.empty((N,), dtype=torch.float32, device=dev))
    wsb = L.lib().jdet_retina_targets_workspace(N, A)
    ws = torch.empty((max(wsb, 4),), dtype=torch.uint8, device=dev)
    L.check(L.lib().jdet_retina_targets(
        L.ptr(a), A, L.ptr(rb), L.ptr(rh), L.ptr(lab), L.ptr(off), N, total, float(pos_iou_thresh),
        float(neg_iou_thresh_hi), float(neg_iou_thresh_lo), L.ptr(out["labels"]), L.ptr(out["label_weights"]),
        L.ptr(out["loc_targets"]), L.ptr(out["loc_weights"]), L.ptr(out["raw_labels"]), L.ptr(out["normalizer"]),
        L.ptr(ws), wsb, L.stream_ptr(a)), "jdet_retina_targets")
    return out


def detect(anchors, loc, logits, score_thresh, scale_x=1.0, scale_y=1.0):
    """anchors (A, 4), loc (A, 5), logits (A, C) of one image -> (boxes (M, 5), scores (M), labels (M) int32, counts: a
    host list of C ints), class-major and anchor-ascending.  One host synchronisation: reading the counts."""
    L.need_device(anchors, loc, logits)
    a, l, x = L.f32c(anchors), L.f32c(loc), L.f32c(logits)
    A, C = x.shape
    dev = a.device
    wsb = L.lib().jdet_retina_detect_workspace(A, C)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    counts = torch.empty((C,), dtype=torch.int32, device=dev)
    L.check(L.lib().jdet_retina_detect_count(L.ptr(a), L.ptr(l), L.ptr(x), A, C, float(score_thresh), L.ptr(counts),
                                             L.ptr(ws), wsb, L.stream_ptr(a)), "jdet_retina_detect_count")
    counts = counts.cpu().tolist()
    M = sum(counts)
    boxes = torch.empty((M, 5), dtype=torch.float32, device=dev)
    scores = torch.empty((M,), dtype=torch.float32, device=dev)
    labels = torch.empty((M,), dtype=torch.int32, device=dev)
    L.check(L.lib().jdet_retina_detect_fill(L.ptr(a), L.ptr(l), L.ptr(x), A, C, float(score_thresh), float(scale_x),
                                            float(scale_y), L.ptr(ws), wsb, M, L.ptr(boxes), L.ptr(scores),
                                            L.ptr(labels), L.stream_ptr(a)), "jdet_retina_detect_fill")
    return boxes, scores, labels, counts
