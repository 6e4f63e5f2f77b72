"""RetinaNet = backbone -> neck -> RetinaHead.  Mirrors python/jdet/models/networks/retinanet.py:L9-60 (the model of
configs/retinanet_r50v1d_fpn_{dota,dota1_5,fair}.py).

The reference rewrites each target's `rboxes` on the host here (L31-51: angle folded into [-pi/2, 0), sides ordered, the
enclosing horizontal box) before the head sees them.  That preparation lives with the head (one launch for the whole
batch on its fused route, `retina_head.prepare_gts` composed) and leaves the caller's target dicts as they are, so a
batch can be fed twice."""
from torch import nn

from jdet_amd.utils.registry import BACKBONES, HEADS, MODELS, NECKS, build_from_cfg


@MODELS.register_module()
class RetinaNet(nn.Module):
    def __init__(self, backbone, neck=None, rpn_net=None):
        super().__init__()
        self.backbone = build_from_cfg(backbone, BACKBONES)
        self.neck = build_from_cfg(neck, NECKS)
        self.rpn_net = build_from_cfg(rpn_net, HEADS)

    def forward(self, images, targets):
        """images (N, C, H, W); targets list[dict].  Training -> dict(roi_cls_loss, roi_loc_loss); eval -> a list of
        (polys, scores, labels) per image."""
        features = self.backbone(images)
        if self.neck:
            features = self.neck(features)
        return self.rpn_net(features, targets)

    execute = forward
