"""Strip R-CNN RoI head: three branches after RoIAlign -- classification (2 FCs -> fc_cls), centre / size (a 3x3
convolution + ReLU, then a 3x3 convolution + BatchNorm + ReLU, flattened -> fc_reg_xy_wh) and angle (2 FCs ->
fc_reg_theta); the two regression outputs are concatenated.

Contract of python/jdet/models/roi_heads/strip_head.py (StripHead_ L50-289, StripHead L293-646): constructor arguments,
the state-dict names `cls_fcs.{0,1}`, `reg_theta_fcs.{0,1}`, `reg_xy_wh_convs.0.conv`, `reg_xy_wh_convs.1.{conv, bn}`,
`fc_cls`, `fc_reg_xy_wh`, `fc_reg_theta` (and the empty lists `shared_convs`, `shared_fcs`, `cls_convs`, `reg_xy_wh_fcs`,
`reg_theta_convs`), loss keys `loss_cls` / `orcnn_bbox_loss`, inference output `(polys (k, 8), scores, labels)`.
Assignment, sampling, targets, losses and decoding are OrientedHead's fixed-shape path (proposal tables,
`sample_stage_rows`, no host round trip in the train step); only the layers and `_trunk` differ.

THE REGRESSION IS CLASS-SPECIFIC, whatever the config says.  The reference's constructor takes `reg_class_agnostic` as
a named parameter (L95, L116) and then overwrites it with `kwargs.get('reg_class_agnostic', False)` (L137), where the
key can never be present -- a named parameter does not reach **kwargs.  So with num_classes = 15 `fc_reg_xy_wh` has 60
outputs and `fc_reg_theta` 15, `bbox_pred = cat([xy_wh (R, 60), theta (R, 15)], 1)` (L429), and both the loss (L459) and
the decode read it as `view(R, 15, 5)`: class c owns entries 5c .. 5c + 4 OF THE CONCATENATION (class 0 the first five
xy_wh outputs, class 12 the five theta outputs 0 .. 4, ...), not (x, y, w, h of class c; theta of class c).  This file
reproduces exactly that: the shapes decide whether a reference checkpoint loads, the grouping what it means.

Also as the reference reads them: `in_channels` (256), `num_classes` (default 80), `with_cls` and `with_reg` arrive
through **kwargs there (L132-139); here they are named parameters with those defaults.  `reg_xy_wh_convs.0` has no norm
layer (the config gives no `norm_cfg`), `reg_xy_wh_convs.1` is the reference's StripBlock: convolution with a bias,
BatchNorm, ReLU.  The head's BatchNorm follows train() / eval() and sees every row of the fixed-size sample, padding
rows (which sit on a small dummy box and carry weight 0) included.

Weight init.  The reference's `init_weights` (L310-323) names attributes that do not exist (`fc_reg`, `reg_fcs`) and is
never run by its constructor.  Here: `fc_cls` ~ N(0, 0.01), `fc_reg_xy_wh` and `fc_reg_theta` ~ N(0, 0.001), the four FCs
Xavier-uniform, biases 0 -- what that method evidently intends."""
import torch
import torch.nn.functional as F
from torch import nn

from jdet_amd.models.utils.modules import ConvModule
from jdet_amd.ops.linear import Linear
from jdet_amd.utils.registry import HEADS

from .oriented_head import OrientedHead
from .roi_feature_linear import RoIFeatureLinear


@HEADS.register_module()
class StripHead(OrientedHead):
    def __init__(self, fc_out_channels=1024, num_classes=80, in_channels=256, conv_out_channels=256,
                 reg_class_agnostic=True, norm_cfg=None, conv_cfg=None, init_cfg=None, **kwargs):
        assert norm_cfg is None and conv_cfg is None, "the Strip R-CNN configuration: plain convolutions, no norm_cfg"
        # the base builds cls_fcs (2) and fc_cls; its regression layers are replaced below
        super().__init__(num_classes=num_classes, in_channels=in_channels, num_shared_convs=0, num_shared_fcs=0,
                         num_cls_convs=0, num_cls_fcs=2, num_reg_convs=0, num_reg_fcs=0, fc_out_channels=fc_out_channels,
                         conv_out_channels=conv_out_channels, reg_class_agnostic=False, **kwargs)
        del self.reg_convs, self.reg_fcs, self.fc_reg
        width = conv_out_channels
        self.reg_xy_wh_convs = nn.ModuleList([
            ConvModule(in_channels, width, 3, padding=1),
            ConvModule(width, width, 3, padding=1, bias=True, norm_cfg=dict(type="BN"))])
        self.reg_xy_wh_fcs = nn.ModuleList()
        self.reg_theta_convs = nn.ModuleList()
        self.reg_theta_fcs = nn.ModuleList([RoIFeatureLinear(in_channels, self.roi_feat_area, fc_out_channels),
                                            Linear(fc_out_channels, fc_out_channels)])
        self.fc_reg_xy_wh = RoIFeatureLinear(width, self.roi_feat_area, 4 * num_classes)
        self.fc_reg_theta = Linear(fc_out_channels, num_classes)
        self.init_weights()

    def init_weights(self):
        if not hasattr(self, "fc_reg_theta"):          # the base constructor's call: the layers are not built yet
            return
        nn.init.normal_(self.fc_cls.weight, 0, 0.01)
        nn.init.constant_(self.fc_cls.bias, 0)
        for m in (self.fc_reg_xy_wh, self.fc_reg_theta):
            nn.init.normal_(m.weight, 0, 0.001)
            nn.init.constant_(m.bias, 0)
        for m in list(self.cls_fcs) + list(self.reg_theta_fcs):
            nn.init.xavier_uniform_(m.weight)
            nn.init.constant_(m.bias, 0)

    def _trunk(self, feats, rois):
        x = self.bbox_roi_extractor(feats[:self.bbox_roi_extractor.num_inputs], rois)
        x_cls = x
        for fc in self.cls_fcs:
            x_cls = F.relu(fc(x_cls))
        x_xy_wh = x
        for conv in self.reg_xy_wh_convs:
            x_xy_wh = conv(x_xy_wh)
        x_theta = x
        for fc in self.reg_theta_fcs:
            x_theta = F.relu(fc(x_theta))
        # (R, 4 C) then (R, C): read downstream as view(R, C, 5), see the module docstring
        bbox_pred = torch.cat([self.fc_reg_xy_wh(x_xy_wh), self.fc_reg_theta(x_theta)], dim=1)
        return [self.fc_cls(x_cls), bbox_pred]
