"""Pieces shared by every single-stage head, anchor-based (S2ANet, RetinaNet, ATSS: through RotatedAnchorHeadMixin in
_anchor_head_common.py) and anchor-free (FCOS, H2RBox, RepPoints): the default train/test cfg wrapper, the target-dict
parsing, the padded (B, Kmax, D) ground truth of the dense routes and the per-image post-processing -- per-level cut to
the `nms_pre` best rows, concatenation, rescale, background column, multiclass rotated NMS, polygons.  What differs per
head (score transform, ranking score, decode) stays in the head."""
import torch

from jdet_amd.models.boxes.box_ops import rotated_box_to_poly
from jdet_amd.ops.nms_rotated import multiclass_nms_rotated


class _AttrDict(dict):
    """dict with Config-like attribute access (missing -> None), for the default train/test cfgs"""

    def __getattr__(self, name):
        return self.get(name)

    def copy(self):
        return _AttrDict(self)


def _cfg(d):
    if type(d) is dict:  # plain dicts (the signature defaults); Config objects already have attribute access
        return _AttrDict({k: _cfg(v) if isinstance(v, dict) else v for k, v in d.items()})
    return d


_DEFAULT_ASSIGN = dict(
    assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1,
                  iou_calculator=dict(type="BboxOverlaps2D_rotated")),
    bbox_coder=dict(type="DeltaXYWHABBoxCoder", target_means=(0., 0., 0., 0., 0.), target_stds=(1., 1., 1., 1., 1.),
                    clip_border=True),
    allowed_border=-1, pos_weight=-1, debug=False)


def device_counts(counts, device):
    """(B,) int32 device tensor of the images' gt counts: a pinned host tensor copied asynchronously (no host sync)"""
    return torch.tensor(counts, dtype=torch.int32).pin_memory().to(device, non_blocking=True)


def parse_targets(targets, is_train):
    """target dicts -> (gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore); the gt lists stay empty at inference"""
    img_metas, gt_bboxes, gt_bboxes_ignore, gt_labels = [], [], [], []
    for target in targets:
        if is_train:
            gt_bboxes.append(target["rboxes"])
            gt_labels.append(target["labels"])
            gt_bboxes_ignore.append(target["rboxes_ignore"])
        img_metas.append(dict(img_shape=target["img_size"][::-1], scale_factor=target["scale_factor"],
                              pad_shape=target["pad_shape"]))
    return gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore


def pad_gts(gt_list, labels_list, width):
    """(gt (B, Kmax, width) fp32, labels (B, Kmax) int32, counts: host list); Kmax >= 1, the rows beyond an image's
    count 0"""
    B = len(gt_list)
    counts = [int(g.shape[0]) for g in gt_list]
    Kmax = max(max(counts), 1)
    if all(c == Kmax for c in counts):
        return torch.stack(gt_list), torch.stack([t.to(torch.int32) for t in labels_list]), counts
    dev = gt_list[0].device
    gt = torch.zeros((B, Kmax, width), dtype=torch.float32, device=dev)
    gl = torch.zeros((B, Kmax), dtype=torch.int32, device=dev)
    for b, (g, t) in enumerate(zip(gt_list, labels_list)):
        if counts[b]:
            gt[b, :counts[b]] = g
            gl[b, :counts[b]] = t.to(torch.int32)
    return gt, gl, counts


# ------------------------------------------------------------------------------------------------------ post-processing
def topk_rows(rank, nms_pre):
    """indices of the `nms_pre` largest entries of rank (n,), in `topk` order; None where nothing is cut"""
    if nms_pre <= 0 or rank.shape[0] <= nms_pre:
        return None
    return rank.topk(nms_pre).indices


def cut_level(nms_pre, rank, *rows):
    """a level's per-position tensors cut to its `nms_pre` best rows.  `rank()` returns the (n,) ranking score: a
    function, so that a level below the cut launches nothing for it"""
    if nms_pre <= 0 or rows[0].shape[0] <= nms_pre:
        return rows
    keep = topk_rows(rank(), nms_pre)
    return tuple(t[keep] for t in rows)


def merge_levels(bboxes_per_level, scores_per_level, scale_factor, rescale, pad_background,
                 score_factors_per_level=None):
    """the levels of one image -> (bboxes (n, 5), scores (n, C [+ 1]), score_factors (n,) | None), what
    multiclass_nms_rotated takes: columns :4 back to the original image's scale, a zero background column 0 for
    sigmoid scores"""
    bboxes = torch.cat(bboxes_per_level)
    if rescale:
        bboxes = torch.cat([bboxes[..., :4] / scale_factor, bboxes[..., 4:]], dim=-1)
    scores = torch.cat(scores_per_level)
    if pad_background:
        scores = torch.cat([scores.new_zeros((scores.shape[0], 1)), scores], dim=1)
    score_factors = torch.cat(score_factors_per_level) if score_factors_per_level is not None else None
    return bboxes, scores, score_factors


def nms_polys(bboxes, scores, score_factors, cfg):
    """multiclass rotated NMS of `merge_levels`' result -> (polys (k, 8), scores (k,), labels (k,) 0-based)"""
    det_bboxes, det_labels = multiclass_nms_rotated(bboxes, scores, cfg.score_thr, cfg.nms, cfg.max_per_img,
                                                    score_factors=score_factors)
    return rotated_box_to_poly(det_bboxes[:, :5]), det_bboxes[:, 5], det_labels


def per_image(single, num_imgs, *outs):
    """[single(b, *levels of image b)]: of every head output in `outs` (a list over levels of (B, ...) maps) level i of
    image b, detached"""
    return [single(b, *([level[b].detach() for level in out] for out in outs)) for b in range(num_imgs)]
