"""Single-stage detector wrapper and FCOS.  Mirrors python/jdet/models/networks/single_stage.py:L6-32 and
python/jdet/models/networks/fcos.py:L4-9 (the head arrives under the config key `roi_heads`)."""
from torch import nn

from jdet_amd.utils.registry import BACKBONES, HEADS, MODELS, NECKS, build_from_cfg


@MODELS.register_module()
class SingleStageDetector(nn.Module):
    """backbone -> neck -> dense head"""

    def __init__(self, backbone, neck=None, roi_heads=None):
        super().__init__()
        self.backbone = build_from_cfg(backbone, BACKBONES)
        self.neck = build_from_cfg(neck, NECKS) if neck is not None else None
        self.bbox_head = build_from_cfg(roi_heads, HEADS)

    def forward(self, images, targets):
        """train mode -> dict of losses; eval mode -> list of (polys, scores, labels) per image"""
        feat = self.backbone(images)
        if self.neck:
            feat = self.neck(feat)
        return self.bbox_head(feat, targets)

    execute = forward


@MODELS.register_module()
class FCOS(SingleStageDetector):
    """The reference's `train()` also calls `self.backbone.train()` (fcos.py:L7-9), which Jittor needs; here
    nn.Module.train() already recurses into the backbone, whose own train() keeps its frozen stages and norm_eval."""
