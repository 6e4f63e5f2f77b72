"""Pieces shared by the RPN heads of the two-stage detectors (FasterrcnnHead, OrientedRPNHead, GlidingRPNHead): the
3x3 + two 1x1 convolutions, the dense loss over all anchors and the per-image candidate gathering in front of
`proposal_table`.  All of it is fixed-shape and never waits for the device (models/boxes/fixed_shape.py).  A head keeps
what is its own: anchors and valid flags, which gts go to the assigner and the coder, the objectness function, the
decode, the min-size predicate and the keywords of `proposal_table`."""
import torch

from jdet_amd.models.utils.level_pack import run_levels
from jdet_amd.ops.conv_igemm import conv_module

INVALID_SCORE = -1.0   # score of a padding row in a proposal table


def forward_single(head, x, mask=None):
    """`rpn_conv` (3x3, relu) -> (`rpn_cls`, `rpn_reg`); bound as a method by the three-conv heads.  `mask` is part of
    `run_levels`' callback signature (the gap mask of a packed input): the 1x1 layers read no neighbours, so a packed
    input needs none here"""
    x = conv_module(head.rpn_conv, x, relu=True)
    return conv_module(head.rpn_cls, x), conv_module(head.rpn_reg, x)


def level_outputs(head, feats):
    """(cls_scores, bbox_preds), one entry per level; small levels run as one packed tensor"""
    outs = run_levels(list(feats), head.forward_single)
    return [o[0] for o in outs], [o[1] for o in outs]


def per_anchor(t, width):
    """(N, A*width, H, W) -> (N, H*W*A, width): the anchor order of grid_anchors (location-major, A fastest)"""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, width)


def dense_loss(head, cls_scores, bbox_preds, level_anchors, per_image, cls_width, reg_dim):
    """per_image: the `dense_anchor_targets` tuple of every image -> (losses_cls, losses_bbox), one entry per level"""
    labels, label_w, box_t, box_w = (torch.stack([p[k] for p in per_image]) for k in range(4))
    # sum over images of max(#pos, 1) + max(#neg, 1) (anchor_target.py:L77-78), kept on the device
    n_samples = sum(torch.clamp(p[4], min=1) + torch.clamp(p[5], min=1) for p in per_image).float()
    losses_cls, losses_bbox, start = [], [], 0
    for cls, reg, lvl in zip(cls_scores, bbox_preds, level_anchors):
        sl = slice(start, start + lvl.shape[0])
        start += lvl.shape[0]
        losses_cls.append(head.loss_cls(per_anchor(cls, cls_width).reshape(-1, cls_width), labels[:, sl].reshape(-1),
                                        label_w[:, sl].reshape(-1), avg_factor=n_samples))
        losses_bbox.append(head.loss_bbox(per_anchor(reg, reg_dim).reshape(-1, reg_dim),
                                          box_t[:, sl].reshape(-1, reg_dim), box_w[:, sl].reshape(-1, reg_dim),
                                          avg_factor=n_samples))
    return losses_cls, losses_bbox


def image_candidates(cls_scores, bbox_preds, level_anchors, cls_width, reg_dim, objectness, nms_pre, sort_levels):
    """Yields, image by image, the candidates of all levels: (scores (M,), deltas (M, reg_dim), anchors (M, 4),
    level ids (M,) long, level sizes).  `objectness`: (n, cls_width) logits -> (n,) scores.  A level keeps its best
    `nms_pre` (<= 0: all).  `sort_levels`: take the top-k even where it keeps everything -- `proposal_table` visits a
    level in the order given, so its per-level NMS needs every level in descending score."""
    scores = [per_anchor(c.detach(), cls_width) for c in cls_scores]
    deltas = [per_anchor(r.detach(), reg_dim) for r in bbox_preds]
    for i in range(scores[0].shape[0]):
        img_scores, img_deltas, img_anchors, ids = [], [], [], []
        for lvl, (s, d, a) in enumerate(zip(scores, deltas, level_anchors)):
            s, d = objectness(s[i]), d[i]
            if sort_levels or 0 < nms_pre < s.shape[0]:
                k = min(nms_pre, s.shape[0]) if nms_pre > 0 else s.shape[0]
                s, top = torch.topk(s, k)                      # descending; equal scores: lowest index first
                d, a = d[top], a[top]
            img_scores.append(s)
            img_deltas.append(d)
            img_anchors.append(a)
            ids.append(torch.full((s.shape[0],), lvl, dtype=torch.long, device=s.device))
        yield (torch.cat(img_scores), torch.cat(img_deltas), torch.cat(img_anchors), torch.cat(ids),
               [int(s.shape[0]) for s in img_scores])


def sigmoid_objectness(s):
    """(n, 1) logits: one sigmoid per anchor"""
    return s[:, 0].sigmoid()


def softmax_objectness(s):
    """(n, 2) logits: a two-way softmax per anchor, class 1 = object"""
    return s.softmax(dim=1)[:, 1]
