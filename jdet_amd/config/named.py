"""Model / optimizer sections of the configs BASELINE.json names, as plain dicts (the reference's files are not
on the GPU box; `Config` loads them unchanged where they are present).  Sources:
configs/s2anet/s2anet_r50_fpn_1x_dota.py, configs/rotated_retinanet/rotated_retinanet_obb_r50_fpn_1x_dota.py,
configs/oriented_rcnn_r50_fpn_1x_dota_with_flip.py, configs/faster_rcnn_RoITrans_r50_fpn_1x_dota.py."""

_SGD_1X = dict(
    optimizer=dict(type="SGD", lr=0.01 / 4., momentum=0.9, weight_decay=0.0001, grad_clip=dict(max_norm=35, norm_type=2)),
    scheduler=dict(type="StepLR", warmup="linear", warmup_iters=500, warmup_ratio=1.0 / 3, milestones=[7, 10]))

S2ANET_CFG = dict(
    model=dict(
        type="S2ANet",
        backbone=dict(type="Resnet50", frozen_stages=1, return_stages=["layer1", "layer2", "layer3", "layer4"],
                      pretrained=True),
        neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
                  add_extra_convs="on_input", num_outs=5),
        bbox_head=dict(type="S2ANetHead", num_classes=16, in_channels=256, feat_channels=256, stacked_convs=2,
                       with_orconv=True, anchor_ratios=[1.0], anchor_strides=[8, 16, 32, 64, 128], anchor_scales=[4],
                       target_means=[.0, .0, .0, .0, .0], target_stds=[1.0, 1.0, 1.0, 1.0, 1.0])),
    # configs/s2anet/s2anet_r50_fpn_1x_dota.py:L151-166 (model section identical to L2-96 there)
    optimizer=dict(type="SGD", lr=0.01 / 4., momentum=0.9, weight_decay=0.0001, grad_clip=dict(max_norm=35, norm_type=2)),
    scheduler=dict(type="StepLR", warmup="linear", warmup_iters=500, warmup_ratio=1.0 / 3, milestones=[7, 10]))


RETINANET_CFG = dict(
    # configs/rotated_retinanet/rotated_retinanet_obb_r50_fpn_1x_dota.py:L2-57 (L1Loss only matters in training)
    model=dict(
        type="RotatedRetinaNet",
        backbone=dict(type="Resnet50", frozen_stages=1, return_stages=["layer1", "layer2", "layer3", "layer4"],
                      pretrained=True),
        neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
                  add_extra_convs="on_input", num_outs=5),
        bbox_head=dict(type="RotatedRetinaHead", num_classes=16, in_channels=256, feat_channels=256, stacked_convs=4,
                       octave_base_scale=4, scales_per_octave=3, anchor_ratios=[1.0, 0.5, 2.0],
                       anchor_strides=[8, 16, 32, 64, 128], loss_bbox=dict(type="L1Loss", loss_weight=1.0))))


ORCNN_CFG = dict(
    # configs/oriented_rcnn_r50_fpn_1x_dota_with_flip.py:L2-105 (head / rpn defaults are the config's values)
    model=dict(
        type="OrientedRCNN",
        backbone=dict(type="Resnet50", frozen_stages=1, return_stages=["layer1", "layer2", "layer3", "layer4"],
                      pretrained=True),
        neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5),
        rpn=dict(type="OrientedRPNHead", in_channels=256, num_classes=1, nms_pre=2000, nms_post=2000),
        bbox_head=dict(type="OrientedHead", num_classes=15, in_channels=256, fc_out_channels=1024)),
    optimizer=dict(type="SGD", lr=0.005, momentum=0.9, weight_decay=0.0001, grad_clip=dict(max_norm=35, norm_type=2)),
    scheduler=dict(type="StepLR", warmup="linear", warmup_iters=500, warmup_ratio=1.0 / 3, milestones=[7, 10]))


def roitrans_cfg(backbone="Resnet50"):
    # configs/faster_rcnn_RoITrans_r50_fpn_1x_dota.py:L1-125
    return dict(
        type="RoITransformer",
        backbone=dict(type=backbone, frozen_stages=1, return_stages=["layer1", "layer2", "layer3", "layer4"],
                      pretrained=False),
        neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=0,
                  add_extra_convs=False, num_outs=5),
        rpn_head=dict(type="FasterrcnnHead", in_channels=256, feat_channels=256, anchor_scales=[8],
                      anchor_ratios=[0.5, 1.0, 2.0], anchor_strides=[4, 8, 16, 32, 64],
                      target_means=[.0, .0, .0, .0], target_stds=[1.0, 1.0, 1.0, 1.0],
                      loss_cls=dict(type="CrossEntropyLossForRcnn", use_sigmoid=True, loss_weight=1.0),
                      loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=1.0)),
        bbox_roi_extractor=dict(type="SingleRoIExtractor",
                                roi_layer=dict(type="ROIAlign", output_size=7, sampling_ratio=2, version=1),
                                out_channels=256, featmap_strides=[4, 8, 16, 32]),
        bbox_head=dict(type="SharedFCBBoxHeadRbbox", num_fcs=2, in_channels=256, fc_out_channels=1024,
                       roi_feat_size=7, num_classes=16, target_means=[0., 0., 0., 0., 0.],
                       target_stds=[0.1, 0.1, 0.2, 0.2, 0.1], reg_class_agnostic=True, with_module=False,
                       loss_cls=dict(type="CrossEntropyLossForRcnn", use_sigmoid=False, loss_weight=1.0),
                       loss_bbox=dict(type="SmoothL1Loss", beta=1.0, loss_weight=1.0)),
        rbbox_roi_extractor=dict(type="RboxSingleRoIExtractor",
                                 roi_layer=dict(type="ROIAlignRotated", output_size=7, sampling_ratio=2),
                                 out_channels=256, featmap_strides=[4, 8, 16, 32]),
        rbbox_head=dict(type="SharedFCBBoxHeadRbbox", num_fcs=2, in_channels=256, fc_out_channels=1024,
                        roi_feat_size=7, num_classes=16, target_means=[0., 0., 0., 0., 0.],
                        target_stds=[0.05, 0.05, 0.1, 0.1, 0.05], reg_class_agnostic=False,
                        loss_cls=dict(type="CrossEntropyLossForRcnn", use_sigmoid=False, loss_weight=1.0),
                        loss_bbox=dict(type="SmoothL1Loss", beta=1.0, loss_weight=1.0)),
        train_cfg=dict(
            rpn=dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3,
                                   ignore_iof_thr=-1, iou_calculator=dict(type="BboxOverlaps2D_v1")),
                     sampler=dict(type="RandomSampler", num=256, pos_fraction=0.5, neg_pos_ub=-1,
                                  add_gt_as_proposals=False),
                     allowed_border=0, pos_weight=-1, debug=False),
            rpn_proposal=dict(nms_across_levels=False, nms_pre=2000, nms_post=2000, max_num=2000, nms_thr=0.7,
                              min_bbox_size=0),
            rcnn=[dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5,
                                     ignore_iof_thr=-1, iou_calculator=dict(type="BboxOverlaps2D_v1")),
                       sampler=dict(type="RandomSampler", num=512, pos_fraction=0.25, neg_pos_ub=-1,
                                    add_gt_as_proposals=True),
                       pos_weight=-1, debug=False),
                  dict(assigner=dict(type="MaxIoUAssignerRbbox", pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5,
                                     ignore_iof_thr=-1, iou_calculator=dict(type="BboxOverlaps2D_rotated")),
                       sampler=dict(type="RandomSamplerRotated", num=512, pos_fraction=0.25, neg_pos_ub=-1,
                                    add_gt_as_proposals=True),
                       pos_weight=-1, debug=False)]),
        test_cfg=dict(rpn=dict(nms_across_levels=False, nms_pre=2000, nms_post=2000, max_num=2000, nms_thr=0.7,
                               min_bbox_size=0),
                      rcnn=dict(score_thr=0.05, nms=dict(type="py_cpu_nms_poly_fast", iou_thr=0.1),
                                max_per_img=2000)))


def roitrans_train_cfg(backbone="Resnet50"):
    # optimizer / schedule: configs/faster_rcnn_RoITrans_r50_fpn_1x_dota.py:L196-213
    return dict(model=roitrans_cfg(backbone),
                optimizer=dict(type="SGD", lr=0.0025, momentum=0.9, weight_decay=0.0001,
                               grad_clip=dict(max_norm=35, norm_type=2)),
                scheduler=dict(type="StepLR", warmup="linear", warmup_iters=500, warmup_ratio=1.0 / 3,
                               milestones=[8, 11]))


def _gaussian_retinanet_cfg(head_type, loss_bbox, reg_decoded_bbox):
    return dict(
        model=dict(
            type="RotatedRetinaNet",
            backbone=dict(type="Resnet50", frozen_stages=1, return_stages=["layer1", "layer2", "layer3", "layer4"],
                          pretrained=True),
            neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
                      add_extra_convs="on_input", num_outs=5),
            bbox_head=dict(
                type=head_type, num_classes=16, in_channels=256, feat_channels=256, stacked_convs=4,
                octave_base_scale=4, scales_per_octave=3, anchor_ratios=[1.0, 0.5, 2.0],
                anchor_strides=[8, 16, 32, 64, 128], target_means=[.0, .0, .0, .0, .0],
                target_stds=[1.0, 1.0, 1.0, 1.0, 1.0],
                loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                loss_bbox=loss_bbox,
                test_cfg=dict(nms_pre=2000, min_bbox_size=0, score_thr=0.05, nms=dict(type="nms_rotated", iou_thr=0.1),
                              max_per_img=2000),
                train_cfg=dict(
                    assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0,
                                  ignore_iof_thr=-1, iou_calculator=dict(type="FakeBboxOverlaps2D_rotated")),
                    bbox_coder=dict(type="DeltaXYWHABBoxCoder", target_means=(0., 0., 0., 0., 0.),
                                    target_stds=(1., 1., 1., 1., 1.), clip_border=True),
                    reg_decoded_bbox=reg_decoded_bbox, allowed_border=-1, pos_weight=-1, debug=False))),
        **_SGD_1X)


# The RotatedRetinaNet variants that swap the box loss for a Gaussian one (model section L1-61, optimizer and scheduler
# from L132 on, of each file; tests/golden/configs/ holds them as `Config` reads them):
# projects/rotated_retinanet_gwd/configs/rotated_retinanet_hbb_gwd_r50_fpn_1x_dota.py (L34-37: GDLoss gwd, L56 decoded)
GWD_RETINANET_CFG = _gaussian_retinanet_cfg(
    "RotatedRetinaHead", dict(type="GDLoss", loss_type="gwd", loss_weight=5.0), True)
# projects/rotated_retinanet_kld/configs/rotated_retinanet_hbb_kld_r50_fpn_1x_dota.py (L34-39: GDLoss_v1 kld, L58 decoded)
KLD_RETINANET_CFG = _gaussian_retinanet_cfg(
    "RotatedRetinaHead", dict(type="GDLoss_v1", loss_type="kld", fun="log1p", tau=1.0, loss_weight=5.5), True)
# projects/rotated_retinanet_kfiou/configs/rotated_retinanet_hbb_kfiou_r50_fpn_1x_dota.py (L17 KFIoURRetinaHead,
# L34-36 KFLoss, L55 delta targets)
KFIOU_RETINANET_CFG = _gaussian_retinanet_cfg(
    "KFIoURRetinaHead", dict(type="KFLoss", loss_weight=5.0), False)


ATSS_RETINANET_CFG = dict(
    # configs/rotated_retinanet/rotated_retinanet_obb_r50_fpn_1x_dota_atss.py: model L2-55, optimizer L128-135,
    # scheduler L137-142 (tests/golden/configs/rotated_retinanet_obb_r50_fpn_1x_dota_atss.yaml holds them as `Config`
    # reads them).  One square anchor per location; ATSS picks 9 candidates per level and gt.
    model=dict(
        type="RotatedRetinaNet",
        backbone=dict(type="Resnet50", frozen_stages=1, return_stages=["layer1", "layer2", "layer3", "layer4"],
                      pretrained=True),
        neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
                  add_extra_convs="on_input", num_outs=5),
        bbox_head=dict(
            type="RotatedATSSHead", num_classes=16, in_channels=256, feat_channels=256, stacked_convs=4,
            octave_base_scale=4, scales_per_octave=1, anchor_ratios=[1.0], anchor_strides=[8, 16, 32, 64, 128],
            target_means=[.0, .0, .0, .0, .0], target_stds=[1.0, 1.0, 1.0, 1.0, 1.0],
            loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
            loss_bbox=dict(type="L1Loss", loss_weight=1.0),
            test_cfg=dict(nms_pre=2000, min_bbox_size=0, score_thr=0.05, nms=dict(type="nms_rotated", iou_thr=0.1),
                          max_per_img=2000),
            train_cfg=dict(
                assigner=dict(type="ATSSAssignerRbbox", topk=9, iou_calculator=dict(type="BboxOverlaps2D_rotated")),
                bbox_coder=dict(type="DeltaXYWHABBoxCoder", target_means=(0., 0., 0., 0., 0.),
                                target_stds=(1., 1., 1., 1., 1.), clip_border=True),
                allowed_border=-1, pos_weight=-1, debug=False))),
    **_SGD_1X)


FCOS_CFG = dict(
    # configs/fcos/fcos_obb_r50_fpn_1x_dota.py: model L2-42, optimizer L118-129.  Anchor-free: one point per location,
    # targets by jdet_fcos_targets, box loss the polygon IoU (jdet_poly_iou_loss); GroupNorm towers (the head's default).
    model=dict(
        type="FCOS",
        backbone=dict(type="Resnet50", frozen_stages=1, norm_eval=True,
                      return_stages=["layer1", "layer2", "layer3", "layer4"], pretrained=True),
        neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
                  add_extra_convs="on_output", num_outs=5, relu_before_extra_convs=True),
        roi_heads=dict(
            type="FCOSHead", num_classes=15, in_channels=256, stacked_convs=4, feat_channels=256,
            strides=[8, 16, 32, 64, 128], scale_theta=True, norm_on_bbox=True,
            loss_cls=dict(type="FocalLoss", gamma=2.0, alpha=0.25, loss_weight=1.0),
            loss_bbox=dict(type="PolyIoULoss", loss_weight=1.0),
            loss_centerness=dict(type="CrossEntropyLoss", use_bce=True, loss_weight=1.0),
            test_cfg=dict(centerness_factor=0.5, nms_pre=1000, min_bbox_size=0, score_thr=0.05,
                          nms=dict(type="obb_nms", iou_thr=0.1), max_per_img=2000))),
    optimizer=dict(type="SGD", lr=0.0025, momentum=0.9, weight_decay=0.0001, grad_clip=dict(max_norm=35, norm_type=2)),
    scheduler=dict(type="StepLR", warmup="linear", warmup_iters=500, warmup_ratio=1.0 / 3, milestones=[8, 11]))


H2RBOX_CFG = dict(
    # configs/h2rbox/h2rbox_obb_r50_adamw_fpn_1x_dota.py: model L2-52, optimizer L126-131, scheduler L133-138
    # (tests/golden/configs/h2rbox_obb_r50_adamw_fpn_1x_dota.yaml holds them as `Config` reads them).  FCOS trained from
    # HORIZONTAL boxes: two views of every batch (jdet_rotate_crop), the horizontal IoU loss on the circumscribed boxes
    # and the view-consistency loss (jdet_h2rbox_aug_loss_*); rect_classes are the 0-based labels of inference.
    model=dict(
        type="H2RBox", crop_size=(1024, 1024), padding="reflection",
        backbone=dict(type="Resnet50", frozen_stages=1, norm_eval=True,
                      return_stages=["layer1", "layer2", "layer3", "layer4"], pretrained=True),
        neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
                  add_extra_convs="on_output", num_outs=5, relu_before_extra_convs=True),
        roi_heads=dict(
            type="H2RBoxHead", num_classes=15, in_channels=256, stacked_convs=4, feat_channels=256,
            strides=[8, 16, 32, 64, 128], scale_theta=True, norm_on_bbox=True, crop_size=(1024, 1024),
            rect_classes=[9, 11],
            loss_cls=dict(type="FocalLoss", gamma=2.0, alpha=0.25, loss_weight=1.0),
            loss_bbox=dict(type="IoULoss", loss_weight=1.0),
            loss_centerness=dict(type="CrossEntropyLoss", use_bce=True, loss_weight=1.0),
            loss_bbox_aug=dict(type="H2RBoxLoss", loss_weight=0.4,
                               center_loss_cfg=dict(type="L1Loss", loss_weight=0.0),
                               shape_loss_cfg=dict(type="IoULoss", loss_weight=1.0),
                               angle_loss_cfg=dict(type="L1Loss", loss_weight=1.0)),
            test_cfg=dict(centerness_factor=0.5, nms_pre=1000, min_bbox_size=0, score_thr=0.05,
                          nms=dict(type="obb_nms", iou_thr=0.1), max_per_img=2000))),
    optimizer=dict(type="AdamW", lr=0.0001, betas=(0.9, 0.999), weight_decay=0.05),
    scheduler=dict(type="StepLR", warmup="linear", warmup_iters=500, warmup_ratio=1.0 / 3, milestones=[8, 11]))


REPPOINTS_CFG = dict(
    # configs/rotated_reppoints_obb_r50_fpn_1x_dota.py: model L2-65, optimizer L138-146, scheduler L148-153
    # (tests/golden/configs/rotated_reppoints_obb_r50_fpn_1x_dota.yaml holds them as `Config` reads them).  Anchor-free:
    # nine points per location, twice; init targets by jdet_convex_point_assign, refine targets by jdet_convex_iou +
    # jdet_assign_max_iou, both point losses the convex GIoU (jdet_convex_giou_loss); GroupNorm in the FPN and the towers.
    model=dict(
        type="RotatedRetinaNet",
        backbone=dict(type="Resnet50", frozen_stages=1, return_stages=["layer1", "layer2", "layer3", "layer4"],
                      pretrained=True),
        neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
                  add_extra_convs="on_input", norm_cfg=dict(type="GN", num_groups=32), num_outs=5),
        bbox_head=dict(
            type="RotatedRepPointsHead", num_classes=15, in_channels=256, feat_channels=256, point_feat_channels=256,
            stacked_convs=3, num_points=9, gradient_mul=0.3, point_strides=[8, 16, 32, 64, 128], point_base_scale=2,
            norm_cfg=dict(type="GN", num_groups=32),
            loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
            loss_bbox_init=dict(type="ConvexGIoULoss", loss_weight=0.375),
            loss_bbox_refine=dict(type="ConvexGIoULoss", loss_weight=1.0),
            transform_method="rotrect", use_reassign=False, topk=6, anti_factor=0.75,
            train_cfg=dict(
                init=dict(assigner=dict(type="ConvexAssigner", scale=4, pos_num=1, assigned_labels_filled=-1),
                          allowed_border=-1, pos_weight=-1, debug=False),
                refine=dict(assigner=dict(type="MaxConvexIoUAssigner", pos_iou_thr=0.4, neg_iou_thr=0.3, min_pos_iou=0,
                                          ignore_iof_thr=-1, assigned_labels_filled=-1,
                                          iou_calculator=dict(type="ConvexOverlaps")),
                            allowed_border=-1, pos_weight=-1, debug=False)),
            test_cfg=dict(nms_pre=2000, min_bbox_size=0, score_thr=0.05, nms=dict(iou_thr=0.4), max_per_img=2000))),
    optimizer=dict(type="SGD", lr=0.008, momentum=0.9, weight_decay=0.0001, grad_clip=dict(max_norm=35, norm_type=2)),
    scheduler=dict(type="StepLR", warmup="linear", warmup_iters=500, warmup_ratio=1.0 / 3, milestones=[7, 10]))


GLIDING_CFG = dict(
    # configs/gliding_r50_fpn_1x_dota_with_flip.py: model L2-116, optimizer L195, scheduler L197-202
    # (tests/golden/configs/gliding_r50_fpn_1x_dota_with_flip.yaml holds them as `Config` reads them)
    model=dict(
        type="GlidingVertex",
        backbone=dict(type="Resnet50", frozen_stages=1, return_stages=["layer1", "layer2", "layer3", "layer4"],
                      pretrained=True),
        neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5),
        rpn=dict(
            type="GlidingRPNHead", in_channels=256, num_classes=2, min_bbox_size=0, nms_thresh=0.7, nms_pre=2000,
            nms_post=2000, feat_channels=256,
            anchor_generator=dict(type="AnchorGenerator", scales=[8], ratios=[0.5, 1.0, 2.0],
                                  strides=[4, 8, 16, 32, 64]),
            bbox_coder=dict(type="GVDeltaXYWHBBoxCoder", target_means=(.0, .0, .0, .0),
                            target_stds=(1.0, 1.0, 1.0, 1.0)),
            loss_cls=dict(type="CrossEntropyLoss", loss_weight=1.0),
            loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=1.0),
            assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3,
                          ignore_iof_thr=-1, match_low_quality=True, assigned_labels_filled=-1),
            sampler=dict(type="RandomSampler", num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False)),
        bbox_head=dict(
            type="GlidingHead", num_classes=15, in_channels=256, representation_dim=1024, pooler_resolution=7,
            pooler_scales=[1 / 4., 1 / 8., 1 / 16., 1 / 32., 1 / 64.], pooler_sampling_ratio=0, score_thresh=0.05,
            nms_thresh=0.1, detections_per_img=2000, box_weights=(10., 10., 5., 5.),
            assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5,
                          ignore_iof_thr=-1, match_low_quality=False, assigned_labels_filled=-1,
                          iou_calculator=dict(type="BboxOverlaps2D")),
            sampler=dict(type="RandomSampler", num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True),
            bbox_coder=dict(type="GVDeltaXYWHBBoxCoder", target_means=(.0, .0, .0, .0),
                            target_stds=(0.1, 0.1, 0.2, 0.2)),
            fix_coder=dict(type="GVFixCoder"), ratio_coder=dict(type="GVRatioCoder"),
            bbox_roi_extractor=dict(type="SingleRoIExtractor",
                                    roi_layer=dict(type="ROIAlign", output_size=7, sampling_ratio=2, version=1),
                                    out_channels=256, featmap_strides=[4, 8, 16, 32]),
            cls_loss=dict(type="CrossEntropyLoss"),
            bbox_loss=dict(type="SmoothL1Loss", beta=1.0, loss_weight=1.0),
            fix_loss=dict(type="SmoothL1Loss", beta=1.0 / 3.0, loss_weight=1.0),
            ratio_loss=dict(type="SmoothL1Loss", beta=1.0 / 3.0, loss_weight=16.0),
            with_bbox=True, with_shared_head=False, start_bbox_type="hbb", end_bbox_type="poly", with_avg_pool=False,
            pos_weight=-1, reg_class_agnostic=False, ratio_thr=0.8, max_per_img=2000)),
    optimizer=dict(type="SGD", lr=0.005, momentum=0.9, weight_decay=0.0001, grad_clip=dict(max_norm=35, norm_type=2)),
    scheduler=dict(type="StepLR", warmup="linear", warmup_iters=500, warmup_ratio=0.001, milestones=[7, 10]))


# ---- localization distillation (configs/ld/): an R18 RetinaNet-OBB, the same with distribution heads on R18 / R50, and
# the R50 -> R18 distillation recipe.  tests/golden/configs/*_ld_*.yaml / rotated_retinanet_obb_*r18*.yaml hold the
# model sections as `Config` reads them.
def _ld_retinanet_cfg(head_type, backbone="Resnet18", **head):
    in_channels = [64, 128, 256, 512] if backbone == "Resnet18" else [256, 512, 1024, 2048]
    return dict(
        model=dict(
            type="RotatedRetinaNet",
            backbone=dict(type=backbone, frozen_stages=1, return_stages=["layer1", "layer2", "layer3", "layer4"],
                          pretrained=True),
            neck=dict(type="FPN", in_channels=in_channels, out_channels=256, start_level=1, add_extra_convs="on_input",
                      num_outs=5),
            bbox_head=dict(
                type=head_type, num_classes=16, in_channels=256, feat_channels=256, stacked_convs=4,
                octave_base_scale=4, scales_per_octave=3, anchor_ratios=[1.0, 0.5, 2.0],
                anchor_strides=[8, 16, 32, 64, 128], target_means=[.0, .0, .0, .0, .0],
                target_stds=[1.0, 1.0, 1.0, 1.0, 1.0],
                loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                loss_bbox=dict(type="L1Loss", loss_weight=1.0), **head,
                test_cfg=dict(nms_pre=2000, min_bbox_size=0, score_thr=0.05, nms=dict(type="nms_rotated", iou_thr=0.1),
                              max_per_img=2000),
                train_cfg=dict(
                    assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0,
                                  ignore_iof_thr=-1, iou_calculator=dict(type="BboxOverlaps2D_rotated")),
                    bbox_coder=dict(type="DeltaXYWHABBoxCoder", target_means=(0., 0., 0., 0., 0.),
                                    target_stds=(1., 1., 1., 1., 1.), clip_border=True),
                    allowed_border=-1, pos_weight=-1, debug=False))),
        **_SGD_1X)


# configs/ld/rotated_retinanet_obb_r18_fpn_1x_dota.py
RETINANET_R18_CFG = _ld_retinanet_cfg("RotatedRetinaHead")
# configs/ld/rotated_retinanet_obb_distribution_r18_fpn_1x_dota.py, ..._r50_fpn_1x_dota.py (reg_max: the head's default, 8)
DIST_RETINANET_R18_CFG = _ld_retinanet_cfg("RotatedRetinaDistributionHead")
DIST_RETINANET_R50_CFG = _ld_retinanet_cfg("RotatedRetinaDistributionHead", backbone="Resnet50")
# configs/ld/ld_rotated_retinanet_obb_r18_r50_fpn_1x_dota.py.  teacher_config: the R50 config above instead of its file
# name; teacher_ckpt: None instead of the file's https link -- pass a local checkpoint of the teacher to distil from
LD_RETINANET_CFG = _ld_retinanet_cfg(
    "RotatedRetinaLocalizationDistillationHead",
    loss_ld=dict(type="KnowledgeDistillationKLDivLoss", loss_weight=10, T=10),
    loss_kd=dict(type="KnowledgeDistillationKLDivLoss", loss_weight=10, T=2),
    loss_im=dict(type="IMLoss", loss_weight=0), imitation_method="finegrained", reg_max=8)
LD_RETINANET_CFG["model"] = dict(LD_RETINANET_CFG["model"], type="KnowledgeDistillationSingleStageDetector",
                                 teacher_config=DIST_RETINANET_R50_CFG, teacher_ckpt=None)


# ---- Circular Smooth Label (projects/csl/configs/rotated_retinanet_obb_csl_gaussian_r50_fpn_1x_dota.py): RetinaNet-OBB
# on R50 whose angle is classified into 45 bins of 4 degrees under a gaussian window of radius 3.
# tests/golden/configs/rotated_retinanet_obb_csl_gaussian_r50_fpn_1x_dota.yaml holds it as `Config` reads it.
CSL_RETINANET_CFG = _ld_retinanet_cfg(
    "CSLRRetinaHead", backbone="Resnet50", angle_coder=dict(type="CSLCoder", omega=4, window="gaussian", radius=3),
    loss_angle=dict(type="SmoothFocalLoss", gamma=2.0, alpha=0.25, loss_weight=0.8))


# ---- the reference's own RetinaNet (configs/retinanet_r50v1d_fpn_{dota,dota1_5,fair}.py): Resnet50_v1d, a bilinear FPN
# merge halved at every step, RetinaHead on 21 horizontal anchors per location.  The three files differ in n_class only
# (dota1_5 says 15, as dota does).  tests/golden/configs/retinanet_r50v1d_fpn_*.yaml hold them as `Config` reads them.
def _retinanet_v1d_cfg(n_class):
    return dict(
        model=dict(
            type="RetinaNet",
            backbone=dict(type="Resnet50_v1d", return_stages=["layer1", "layer2", "layer3", "layer4"], pretrained=True),
            neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
                      add_extra_convs="on_output", num_outs=5, upsample_cfg=dict(mode="bilinear", tf_mode=True),
                      upsample_div_factor=2, relu_before_extra_convs=True),
            rpn_net=dict(
                type="RetinaHead", n_class=n_class, in_channels=256, stacked_convs=4, mode="R", score_threshold=0.05,
                nms_iou_threshold=0.3, max_dets=10000, roi_beta=1 / 9., cls_loss_weight=1., loc_loss_weight=0.2,
                anchor_generator=dict(
                    type="AnchorGeneratorRotated", strides=[8, 16, 32, 64, 128],
                    ratios=[1, 0.5, 2.0, 0.3333333333333333, 3.0, 5.0, 0.2],
                    scales=[1, 1.2599210498948732, 1.5874010519681994], base_sizes=[32, 64, 128, 256, 512],
                    angles=[-90, -75, -60, -45, -30, -15], mode="H"))),
        optimizer=dict(type="GradMutilpySGD", lr=3 * 5e-4, momentum=0.9, weight_decay=1e-4,
                       grad_clip=dict(max_norm=30., norm_type=2)),
        scheduler=dict(type="StepLR", warmup="linear", warmup_iters=14000, warmup_ratio=0.1, milestones=[27]))


RETINANET_V1D_DOTA_CFG = _retinanet_v1d_cfg(15)
RETINANET_V1D_DOTA1_5_CFG = _retinanet_v1d_cfg(15)
RETINANET_V1D_FAIR_CFG = _retinanet_v1d_cfg(37)


# configs/lsknet-s_fpn_1x_dota_with_flip.py:L2-200 -- Oriented R-CNN on an LSKNet_s backbone, AdamW: the model, optimizer
# and scheduler sections as `Config` reads them (tests/golden/configs/lsknet-s_fpn_1x_dota_with_flip.yaml).  The
# `pretrained` file is the reference's converted ImageNet backbone; where it is absent the init stays in place.
LSKNET_S_ORCNN_CFG = {'model': {'type': 'OrientedRCNN',
           'backbone': {'type': 'LSKNet_s',
                        'img_size': 1024,
                        'num_stages': 4,
                        'out_indices': [0, 1, 2, 3],
                        'pretrained': 'weights/lsk_s_backbone-e9d2e551_jittor.pkl'},
           'neck': {'type': 'FPN', 'in_channels': [64, 128, 320, 512], 'out_channels': 256, 'num_outs': 5},
           'rpn': {'type': 'OrientedRPNHead',
                   'in_channels': 256,
                   'num_classes': 1,
                   'min_bbox_size': 0,
                   'nms_thresh': 0.8,
                   'nms_pre': 2000,
                   'nms_post': 2000,
                   'feat_channels': 256,
                   'bbox_type': 'obb',
                   'reg_dim': 6,
                   'background_label': 0,
                   'reg_decoded_bbox': False,
                   'pos_weight': -1,
                   'anchor_generator': {'type': 'AnchorGenerator',
                                        'scales': [8],
                                        'ratios': [0.5, 1.0, 2.0],
                                        'strides': [4, 8, 16, 32, 64]},
                   'bbox_coder': {'type': 'MidpointOffsetCoder',
                                  'target_means': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                                  'target_stds': [1.0, 1.0, 1.0, 1.0, 0.5, 0.5]},
                   'loss_cls': {'type': 'CrossEntropyLossForRcnn', 'use_sigmoid': True, 'loss_weight': 1.0},
                   'loss_bbox': {'type': 'SmoothL1Loss', 'beta': 0.1111111111111111, 'loss_weight': 1.0},
                   'assigner': {'type': 'MaxIoUAssigner',
                                'pos_iou_thr': 0.7,
                                'neg_iou_thr': 0.3,
                                'min_pos_iou': 0.3,
                                'ignore_iof_thr': -1,
                                'match_low_quality': True,
                                'assigned_labels_filled': -1},
                   'sampler': {'type': 'RandomSampler',
                               'num': 256,
                               'pos_fraction': 0.5,
                               'neg_pos_ub': -1,
                               'add_gt_as_proposals': False}},
           'bbox_head': {'type': 'OrientedHead',
                         'num_classes': 15,
                         'in_channels': 256,
                         'fc_out_channels': 1024,
                         'score_thresh': 0.05,
                         'assigner': {'type': 'MaxIoUAssigner',
                                      'pos_iou_thr': 0.5,
                                      'neg_iou_thr': 0.5,
                                      'min_pos_iou': 0.5,
                                      'ignore_iof_thr': -1,
                                      'match_low_quality': False,
                                      'assigned_labels_filled': -1,
                                      'iou_calculator': {'type': 'BboxOverlaps2D_rotated_v1'}},
                         'sampler': {'type': 'RandomSamplerRotated',
                                     'num': 512,
                                     'pos_fraction': 0.25,
                                     'neg_pos_ub': -1,
                                     'add_gt_as_proposals': True},
                         'bbox_coder': {'type': 'OrientedDeltaXYWHTCoder',
                                        'target_means': [0.0, 0.0, 0.0, 0.0, 0.0],
                                        'target_stds': [0.1, 0.1, 0.2, 0.2, 0.1]},
                         'bbox_roi_extractor': {'type': 'OrientedSingleRoIExtractor',
                                                'roi_layer': {'type': 'ROIAlignRotated_v1',
                                                              'output_size': 7,
                                                              'sampling_ratio': 2},
                                                'out_channels': 256,
                                                'extend_factor': [1.4, 1.2],
                                                'featmap_strides': [4, 8, 16, 32]},
                         'loss_cls': {'type': 'CrossEntropyLoss'},
                         'loss_bbox': {'type': 'SmoothL1Loss', 'beta': 1.0, 'loss_weight': 1.0},
                         'with_bbox': True,
                         'with_shared_head': False,
                         'with_avg_pool': False,
                         'with_cls': True,
                         'with_reg': True,
                         'start_bbox_type': 'obb',
                         'end_bbox_type': 'obb',
                         'reg_dim': None,
                         'reg_class_agnostic': True,
                         'reg_decoded_bbox': False,
                         'pos_weight': -1}},
 'optimizer': {'type': 'AdamW', 'lr': 0.0001, 'betas': [0.9, 0.999], 'weight_decay': 0.05},
 'scheduler': {'type': 'StepLR',
               'warmup': 'linear',
               'warmup_iters': 500,
               'warmup_ratio': 0.001,
               'milestones': [7, 10]}}


# configs/strip_rcnn_s_fpn_1x_dota_with_flip.py:L2-197 -- Strip R-CNN: a StripNet_S backbone, OrientedRPNHead and a StripHead
# under AdamW: the model, optimizer and scheduler sections as `Config` reads them
# (tests/golden/configs/strip_rcnn_s_fpn_1x_dota_with_flip.yaml).  `reg_class_agnostic` is what the file says; StripHead,
# like the reference, regresses per class whatever it says (models/roi_heads/strip_head.py).  Where the `pretrained` file
# is absent the init stays in place.
STRIP_RCNN_S_CFG = {'model': {'type': 'StripRCNN',
           'backbone': {'type': 'StripNet_S',
                        'img_size': 1024,
                        'num_stages': 4,
                        'out_indices': [0, 1, 2, 3],
                        'pretrained': './weights/stripnet_s_jittor.pkl'},
           'neck': {'type': 'FPN', 'in_channels': [64, 128, 320, 512], 'out_channels': 256, 'num_outs': 5},
           'rpn': {'type': 'OrientedRPNHead',
                   'in_channels': 256,
                   'num_classes': 1,
                   'min_bbox_size': 0,
                   'nms_thresh': 0.8,
                   'nms_pre': 2000,
                   'nms_post': 2000,
                   'feat_channels': 256,
                   'bbox_type': 'obb',
                   'reg_dim': 6,
                   'background_label': 0,
                   'reg_decoded_bbox': False,
                   'pos_weight': -1,
                   'anchor_generator': {'type': 'AnchorGenerator',
                                        'scales': [8],
                                        'ratios': [0.5, 1.0, 2.0],
                                        'strides': [4, 8, 16, 32, 64]},
                   'bbox_coder': {'type': 'MidpointOffsetCoder',
                                  'target_means': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                                  'target_stds': [1.0, 1.0, 1.0, 1.0, 0.5, 0.5]},
                   'loss_cls': {'type': 'CrossEntropyLossForRcnn', 'use_sigmoid': True, 'loss_weight': 1.0},
                   'loss_bbox': {'type': 'SmoothL1Loss', 'beta': 0.1111111111111111, 'loss_weight': 1.0},
                   'assigner': {'type': 'MaxIoUAssigner',
                                'pos_iou_thr': 0.7,
                                'neg_iou_thr': 0.3,
                                'min_pos_iou': 0.3,
                                'ignore_iof_thr': -1,
                                'match_low_quality': True,
                                'assigned_labels_filled': -1},
                   'sampler': {'type': 'RandomSampler',
                               'num': 256,
                               'pos_fraction': 0.5,
                               'neg_pos_ub': -1,
                               'add_gt_as_proposals': False}},
           'bbox_head': {'type': 'StripHead',
                         'num_classes': 15,
                         'in_channels': 256,
                         'fc_out_channels': 1024,
                         'score_thresh': 0.05,
                         'assigner': {'type': 'MaxIoUAssigner',
                                      'pos_iou_thr': 0.5,
                                      'neg_iou_thr': 0.5,
                                      'min_pos_iou': 0.5,
                                      'ignore_iof_thr': -1,
                                      'match_low_quality': False,
                                      'assigned_labels_filled': -1,
                                      'iou_calculator': {'type': 'BboxOverlaps2D_rotated_v1'}},
                         'sampler': {'type': 'RandomSamplerRotated',
                                     'num': 512,
                                     'pos_fraction': 0.25,
                                     'neg_pos_ub': -1,
                                     'add_gt_as_proposals': True},
                         'bbox_coder': {'type': 'OrientedDeltaXYWHTCoder',
                                        'target_means': [0.0, 0.0, 0.0, 0.0, 0.0],
                                        'target_stds': [0.1, 0.1, 0.2, 0.2, 0.1]},
                         'bbox_roi_extractor': {'type': 'OrientedSingleRoIExtractor',
                                                'roi_layer': {'type': 'ROIAlignRotated_v1',
                                                              'output_size': 7,
                                                              'sampling_ratio': 2},
                                                'out_channels': 256,
                                                'extend_factor': [1.4, 1.2],
                                                'featmap_strides': [4, 8, 16, 32]},
                         'loss_cls': {'type': 'CrossEntropyLoss'},
                         'loss_bbox': {'type': 'SmoothL1Loss', 'beta': 1.0, 'loss_weight': 1.0},
                         'with_bbox': True,
                         'with_shared_head': False,
                         'with_avg_pool': False,
                         'with_cls': True,
                         'with_reg': True,
                         'start_bbox_type': 'obb',
                         'end_bbox_type': 'obb',
                         'reg_dim': None,
                         'reg_class_agnostic': True,
                         'reg_decoded_bbox': False,
                         'pos_weight': -1}},
 'optimizer': {'type': 'AdamW', 'lr': 0.0001, 'betas': [0.9, 0.999], 'weight_decay': 0.05},
 'scheduler': {'type': 'StepLR',
               'warmup': 'linear',
               'warmup_iters': 500,
               'warmup_ratio': 0.001,
               'milestones': [7, 10]}}
