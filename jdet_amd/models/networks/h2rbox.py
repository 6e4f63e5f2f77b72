"""H2RBox: rotated boxes learnt from horizontal annotations.  Mirrors python/jdet/models/networks/h2rbox.py:L10-121.

A training step sees the batch twice: view 1 is the centre crop, view 2 the same crop of the batch rotated by one random
angle; the head's consistency loss ties the two (models/roi_heads/h2rbox_head.py).  `rot` is drawn on the HOST (the
reference draws it with jt.rand and reads it back through math.cos: a sync), uniform in (-pi, pi); a test pins it with
`fixed_rot`.  The views are made by ops.rotate_crop: one launch for the cropped window on the device route
(jdet_rotate_crop), the reference's grid_sample program on the general route (`device_rotate = False`)."""
import math
import random

import torch
from torch import nn

from jdet_amd.ops.rotate_crop import crop_offsets, rotate_crop
from jdet_amd.utils.registry import BACKBONES, HEADS, MODELS, NECKS, build_from_cfg


@MODELS.register_module()
class H2RBox(nn.Module):
    def __init__(self, backbone, neck=None, roi_heads=None, crop_size=(768, 768), padding="reflection"):
        super().__init__()
        self.backbone = build_from_cfg(backbone, BACKBONES)
        self.neck = build_from_cfg(neck, NECKS) if neck is not None else None
        self.bbox_head = build_from_cfg(roi_heads, HEADS)
        self.crop_size = tuple(crop_size)
        self.padding = padding
        self.fixed_rot = None           # tests: the angle of view 2 instead of a random one
        self.device_rotate = True       # A/B switch of the two rotate_crop routes
        self._rng = random.Random()

    def rotate_crop(self, img, theta=0.0, size=(768, 768), gt_bboxes=None, padding="reflection"):
        """the view of `img` rotated by theta and centre-cropped to `size`; with `gt_bboxes` also the boxes in the
        view's frame (L53-62, L67-73)"""
        n, c, h, w = img.shape
        crop_h, crop_w = crop_offsets(h, w, size)
        out = rotate_crop(img, theta, size, padding, device_route=self.device_rotate)
        if gt_bboxes is None:
            return out
        moved = []
        for bboxes in gt_bboxes:
            # (host numbers only: a tensor built from them would be a synchronising host-to-device copy)
            x, y, wh, a = bboxes[..., 0:1], bboxes[..., 1:2], bboxes[..., 2:4], bboxes[..., 4:5]
            if theta != 0:
                # (xy - ctr) . tf^T + ctr with tf = [[cos, -sin], [sin, cos]] and ctr = (w / 2, h / 2)
                cosa, sina = math.cos(theta), math.sin(theta)
                dx, dy = x - w / 2, y - h / 2
                x, y = dx * cosa - dy * sina + w / 2, dx * sina + dy * cosa + h / 2
                a = a + theta
            moved.append(torch.cat([x - crop_w, y - crop_h, wh, a], dim=-1))
        return out, moved

    def _features(self, images):
        feat = self.backbone(images)
        return self.neck(feat) if self.neck else feat

    def forward_train(self, images, targets):
        rot = self.fixed_rot if self.fixed_rot is not None else (self._rng.random() * 2 - 1) * math.pi
        images1, gt_bboxes_batch = self.rotate_crop(images, 0, self.crop_size, [t["rboxes"] for t in targets],
                                                    self.padding)
        # (new dicts: the reference overwrites targets[i]['rboxes'], which would shift a repeated batch again)
        targets = [dict(t, rboxes=g) for t, g in zip(targets, gt_bboxes_batch)]
        feat1 = self._features(images1)
        images2 = self.rotate_crop(images, rot, self.crop_size, padding=self.padding)
        feat2 = self._features(images2)
        return self.bbox_head.execute_train(feat1, feat2, rot, targets)

    def forward_test(self, images, targets):
        return self.bbox_head(self._features(images), targets)

    def forward(self, images, targets):
        """train mode -> dict of losses; eval mode -> list of (polys, scores, labels) per image"""
        if self.training:
            return self.forward_train(images, targets)
        return self.forward_test(images, targets)

    execute = forward
