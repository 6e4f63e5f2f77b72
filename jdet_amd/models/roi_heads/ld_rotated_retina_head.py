"""The student head of localization distillation.  Mirrors python/jdet/models/roi_heads/ld_rotated_retina_head.py
(loss: L229-360): RotatedRetinaDistributionHead plus, per pyramid level,
  loss_LD                 KL between the student's and the teacher's box-side distributions (rows of reg_max + 1 logits)
                          at temperature T, over the sides of weight > 0 -- the bbox_weights window;
  loss_KD                 the same between the class logits, over the anchors of label weight > 0;
  loss_FeatureImitation   MSE between the FPN features, reshaped to (-1, 256) as there.
Each KL term is one node per level reading the level's weight window in place (losses/kd_loss.py)."""
from jdet_amd.models.utils.level_pack import run_levels
from jdet_amd.utils.registry import HEADS, LOSSES, build_from_cfg

from ._dense_head_common import _DEFAULT_ASSIGN
from .rotated_retina_distribution_head import RotatedRetinaDistributionHead


@HEADS.register_module()
class RotatedRetinaLocalizationDistillationHead(RotatedRetinaDistributionHead):
    def __init__(self, num_classes, in_channels, feat_channels=256, stacked_convs=4, octave_base_scale=4,
                 scales_per_octave=3, anchor_ratios=[1.0, 0.5, 2.0], anchor_strides=[8, 16, 32, 64, 128],
                 anchor_base_sizes=None, target_means=(.0, .0, .0, .0, .0), target_stds=(1.0, 1.0, 1.0, 1.0, 1.0),
                 loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0), reg_max=8,
                 loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=1.0),
                 loss_ld=dict(type="KnowledgeDistillationKLDivLoss", loss_weight=0.25, T=10),
                 loss_kd=dict(type="KnowledgeDistillationKLDivLoss", loss_weight=10, T=2),
                 loss_im=dict(type="IMLoss", loss_weight=2.0), imitation_method="finegrained",
                 test_cfg=dict(nms_pre=2000, min_bbox_size=0, score_thr=0.05, nms=dict(type="nms_rotated", iou_thr=0.1),
                               max_per_img=2000),
                 train_cfg=_DEFAULT_ASSIGN):
        super().__init__(num_classes, in_channels, feat_channels=feat_channels, stacked_convs=stacked_convs,
                         octave_base_scale=octave_base_scale, scales_per_octave=scales_per_octave,
                         anchor_ratios=anchor_ratios, anchor_strides=anchor_strides, anchor_base_sizes=anchor_base_sizes,
                         target_means=target_means, target_stds=target_stds, loss_cls=loss_cls, reg_max=reg_max,
                         loss_bbox=loss_bbox, test_cfg=test_cfg, train_cfg=train_cfg)
        self.loss_ld = build_from_cfg(loss_ld, LOSSES)
        self.loss_kd = build_from_cfg(loss_kd, LOSSES)
        self.loss_im = build_from_cfg(loss_im, LOSSES)
        self.imitation_method = imitation_method     # stored and unused, as in the reference

    def loss(self, cls_scores, bbox_preds, feats_student, feats_teacher, logits_teacher, gt_bboxes, gt_labels, img_metas,
             gt_bboxes_ignore=None):
        cls_scores_teacher, bbox_preds_teacher = logits_teacher[0], logits_teacher[1]
        cfg = self.train_cfg.copy()
        featmap_sizes = [tuple(featmap.shape[-2:]) for featmap in cls_scores]
        assert len(featmap_sizes) == len(self.anchor_generators)
        anchor_list, valid_flag_list = self.get_init_anchors(featmap_sizes, img_metas, cls_scores[0].device)
        label_channels = self.cls_out_channels if self.use_sigmoid_cls else 1
        targets = self.anchor_target(anchor_list, valid_flag_list, gt_bboxes, img_metas, self.target_means,
                                     self.target_stds, cfg, gt_bboxes_ignore_list=gt_bboxes_ignore,
                                     gt_labels_list=gt_labels, label_channels=label_channels, sampling=self.sampling)
        if targets is None:
            return None
        losses_cls, losses_bbox = self._stage_loss(cls_scores, bbox_preds, anchor_list, valid_flag_list, gt_bboxes,
                                                   gt_labels, img_metas, gt_bboxes_ignore, cfg, self.loss_cls,
                                                   self.loss_bbox, targets=targets,
                                                   need_anchors=cfg.get("reg_decoded_bbox", False))
        _, label_weights_list, _, bbox_weights_list, num_total_pos, num_total_neg = targets
        num_total_samples = num_total_pos + num_total_neg if self.sampling else num_total_pos
        losses_ld, losses_kd, losses_im = [], [], []
        bins = self.reg_max + 1
        for i in range(len(cls_scores)):
            # rows of one distribution: (rows * 5, reg_max + 1) views of the (rows, 5 * (reg_max + 1)) views
            pred = self._level_logits(bbox_preds[i]).reshape(-1, bins)
            soft = self._level_logits(bbox_preds_teacher[i]).reshape(-1, bins)
            losses_ld.append(self.loss_ld(pred, soft, bbox_weights_list[i], avg_factor=num_total_samples))
            cls = cls_scores[i].permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels)
            cls_t = cls_scores_teacher[i].permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels)
            losses_kd.append(self.loss_kd(cls, cls_t, label_weights_list[i], avg_factor=num_total_samples))
            fs = feats_student[i].permute(0, 2, 3, 1).reshape(-1, 256)
            ft = feats_teacher[i].permute(0, 2, 3, 1).reshape(-1, 256)
            losses_im.append(self.loss_im(fs, ft))
        return dict(loss_cls=losses_cls, loss_bbox=losses_bbox, loss_LD=losses_ld, loss_KD=losses_kd,
                    loss_FeatureImitation=losses_im)

    def forward_levels(self, feats):
        """(cls_scores, bbox_preds), each a list over the levels"""
        per_level = run_levels(list(feats), lambda x, mask: self.forward_single(x, mask=mask))
        return tuple(map(list, zip(*per_level)))

    def execute_train(self, feats, feats_teacher, logits_teacher, targets):
        outs = self.forward_levels(feats)
        if self.training:
            return self.loss(*outs, feats, feats_teacher, logits_teacher, *self.parse_targets(targets))
        return self.get_bboxes(*outs, self.parse_targets(targets, is_train=False))
