# ProbPose-small on MI355X: evaluation on the CropCOCO and COCO val sets, the val parts of the reference's
# configs/body_2d_keypoint/topdown_probmap/coco/td-pm_ProbPose-small_8xb64-210e_coco-256x192.py (:113-199): the two val
# datasets on ground-truth boxes, their CombinedDataset and the two-metric evaluator. Set the dataset roots on the command line:
#   python tools/test.py configs/td-pm_ProbPose-small_mi355x_cropcoco-coco-val-256x192.py CHECKPOINT --cfg-options \
#       test_dataloader.dataset.datasets.0.data_root=/data/CropCOCO/ test_dataloader.dataset.datasets.1.data_root=/data/coco/
# The metrics read the annotation files of their datasets (the reference's CocoMetric does so through the MessageHub
# when `ann_file` is not set); set `test_evaluator.metrics.<i>.ann_file=...` to evaluate against another file.
_base_ = ["./td-pm_ProbPose-small_mi355x_coco-256x192.py"]

COCO_ROOT = "PATH/TO/COCO/DATASET/"
CropCOCO_ROOT = "PATH/TO/CropCOCO/DATASET/"
COCO_NAME = "COCO"
CropCOCO_NAME = "CropCOCO"
INPUT_PADDING = 1.25
TEST_BATCH_SIZE = 64

val_pipeline = [
    dict(type="LoadImage", pad_to_aspect_ratio=False),
    dict(type="GetBBoxCenterScale"),
    dict(type="TopdownAffine", input_size=(192, 256), use_udp=True, input_padding=INPUT_PADDING),
    dict(type="PackPoseInputs"),
]
coco_val = dict(
    type="CocoDataset",
    data_root=COCO_ROOT,
    data_mode="topdown",
    ann_file="annotations/person_keypoints_val2017.json",
    test_mode=True,
    pipeline=[],
    data_prefix=dict(img="val2017/"),
)
CropCOCO_val = dict(
    type="CocoCropDataset",
    data_root=CropCOCO_ROOT,
    data_mode="topdown",
    ann_file="annotations/person_keypoints_val2017.json",
    test_mode=True,
    pipeline=[],
    data_prefix=dict(img="val2017/"),
)
combined_val_dataset = dict(
    type="CombinedDataset",
    metainfo=dict(from_file="configs/_base_/datasets/coco.py"),
    datasets=[CropCOCO_val, coco_val],
    pipeline=val_pipeline,
    test_mode=True,
)
test_dataloader = dict(
    _delete_=True,
    batch_size=TEST_BATCH_SIZE,
    num_workers=4,
    persistent_workers=True,
    drop_last=False,
    sampler=dict(type="DefaultSampler", shuffle=False, round_up=False),
    dataset=combined_val_dataset,
)
val_dataloader = test_dataloader

_metric = dict(
    type="CocoMetric",
    extended=[False, True],
    match_by_bbox=[False, False],
    ignore_border_points=[False, False],
    padding=INPUT_PADDING,
    score_thresh_type="prob",
    keypoint_score_thr=0.45,
)
test_evaluator = dict(
    type="MultiDatasetEvaluator",
    metrics=[dict(_metric, prefix=CropCOCO_NAME), dict(_metric, prefix=COCO_NAME)],
    datasets=combined_val_dataset["datasets"],
)
val_evaluator = test_evaluator
