# ViTPose-huge-simple on MI355X, inference and evaluation settings. Mirrors the model / codec / test keys and the val dataset of
# the reference's configs/body_2d_keypoint/topdown_heatmap/coco/td-hm_ViTPose-huge-simple_8xb64-210e_coco-256x192.py; training /
# optimizer entries are not part of the inference hot path and are left out. Backbone: ViT-H (1280 wide, 32 layers, 16 heads of 80), the one of
# configs/td-hm_ViTPose-huge_mi355x_coco-256x192.py. Neck and head are the reference's: ReLU + bilinear x4 upsampling
# (FeatureMapProcessor), then one 3x3 convolution to the 17 maps, decoded by the UDP codec with DARK refinement. On the device the
# convolution runs in front of the upsampling, as nine taps at 16 x 12 (csrc/pp_simple_head.hip): pp_relu_operand, one pp_gemm_ws,
# pp_taps_upsample4_conv3x3, pp_udp_heatmap_decode - the x4 map is never built, and model.extract_feat returns the backbone's maps.
#   python tools/test.py configs/td-hm_ViTPose-huge-simple_mi355x_coco-256x192.py CHECKPOINT \
#       --cfg-options test_dataloader.dataset.data_root=/data/coco/
# The reference evaluates this model on the boxes of a person detector (`bbox_file=...detections_AP_H_56_person.json`). To mirror
# that evaluation, pass the detections file on the command line (detector score x mean keypoint score, OKS-NMS per image):
#   python tools/test.py configs/td-hm_ViTPose-huge-simple_mi355x_coco-256x192.py CHECKPOINT --bbox-file COCO_val2017_detections_AP_H_56_person.json [--nms device]
# The dataset dict below stays without `bbox_file` (CocoDataset still refuses it: the detections enter beside the dataset, as
# datasets.DetectionBoxes); without the flag this config evaluates on the GROUND-TRUTH boxes of the annotation file, like the
# ProbPose configs - the models are then compared on equal boxes, but that AP is not the number the reference's config reports.
custom_imports = dict(imports=["probpose_code_amd"], allow_failed_imports=False)
default_scope = "mmpose"

TEST_BATCH_SIZE = 64
COCO_ROOT = "PATH/TO/COCO/DATASET/"

codec = dict(type="UDPHeatmap", input_size=(192, 256), heatmap_size=(48, 64), sigma=2)

model = dict(
    type="TopdownPoseEstimator",
    # MI355X-only key: operand precision of the MFMA kernels (see the ProbPose config)
    precision="f16x3",
    data_preprocessor=dict(
        type="PoseDataPreprocessor", mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], bgr_to_rgb=True
    ),
    backbone=dict(
        type="mmpretrain.VisionTransformer",
        arch="huge",
        img_size=(256, 192),
        patch_size=16,
        qkv_bias=True,
        drop_path_rate=0.55,
        with_cls_token=False,
        out_type="featmap",
        patch_cfg=dict(padding=2),
        init_cfg=None,
    ),
    neck=dict(type="FeatureMapProcessor", scale_factor=4.0, apply_relu=True),
    head=dict(
        type="HeatmapHead",
        in_channels=1280,
        out_channels=17,
        deconv_out_channels=[],
        deconv_kernel_sizes=[],
        final_layer=dict(kernel_size=3, padding=1),
        loss=dict(type="KeypointMSELoss", use_target_weight=True),
        decoder=codec,
    ),
    test_cfg=dict(flip_test=True, flip_mode="heatmap", shift_heatmap=False),
)

val_pipeline = [
    dict(type="LoadImage"),
    dict(type="GetBBoxCenterScale"),
    dict(type="TopdownAffine", input_size=codec["input_size"], use_udp=True),
    dict(type="PackPoseInputs"),
]
test_dataloader = dict(
    batch_size=TEST_BATCH_SIZE,
    num_workers=4,
    persistent_workers=True,
    drop_last=False,
    sampler=dict(type="DefaultSampler", shuffle=False, round_up=False),
    dataset=dict(
        type="CocoDataset",
        data_root=COCO_ROOT,
        data_mode="topdown",
        ann_file="annotations/person_keypoints_val2017.json",
        data_prefix=dict(img="val2017/"),
        test_mode=True,
        pipeline=val_pipeline,
    ),
)
val_dataloader = test_dataloader

# (the metric reads the dataset's annotation file; `test_evaluator.ann_file=...` evaluates against another one)
test_evaluator = dict(type="CocoMetric")
val_evaluator = test_evaluator
