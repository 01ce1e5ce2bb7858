"""Golden instances of a detector-box evaluation from the REFERENCE's own code (build container only):
``BaseCocoStyleDataset._load_detection_results`` and ``filter_data`` (mmpose/datasets/datasets/base/base_coco_style_dataset.py
:430-514) through ``CocoDataset(bbox_file=..., filter_cfg=...)``, loaded behind the stubs of ``make_golden_dataset.py`` with the
reference's real ``bbox_xywh2xyxy`` (mmpose/structures/bbox/transforms.py) in place.

Input: a small hand-made annotation + detections pair (3 images, 12 entries: two of another category, a score exactly at
the threshold and one just below it, a box partly outside its image, an exact duplicate box with another score, an entry
with a segmentation, a five-value box). Output: detboxes_cases.json (both input files, the threshold, the scalar fields of
every instance, unfiltered and filtered) and detboxes_cases.npz (the array fields). Data only.
Run: python tests/golden/make_golden_detboxes.py"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_dataset as mgd  # noqa: E402
from _ref_import import load_reference_bbox  # noqa: E402

THR = 0.3


def annotation_file():
    images = [dict(id=42, file_name="000042.jpg", width=320, height=240), dict(id=7, file_name="000007.jpg", width=200, height=160),
              dict(id=19, file_name="000019.jpg", width=96, height=128)]
    cats = [dict(id=1, name="person", supercategory="person", keypoints=[], skeleton=[])]
    return dict(images=images, annotations=[], categories=cats)


def detections_file():
    below = float(np.nextafter(np.float32(THR), np.float32(0)))  # the float32 just below float32(THR)
    return [
        dict(image_id=42, category_id=1, bbox=[10.5, 20.25, 100.0, 150.5], score=0.987),
        dict(image_id=42, category_id=18, bbox=[5.0, 5.0, 50.0, 50.0], score=0.9),  # not a person
        dict(image_id=7, category_id=1, bbox=[30.0, 12.5, 60.0, 120.0], score=THR),  # exactly at the threshold: stays
        dict(image_id=42, category_id=1, bbox=[10.5, 20.25, 100.0, 150.5], score=0.45),  # duplicate box, other score
        dict(image_id=7, category_id=1, bbox=[150.0, 100.0, 90.25, 80.5], score=0.71),  # runs past the right / bottom edges
        dict(image_id=19, category_id=1, bbox=[-12.5, -3.0, 60.0, 90.0], score=0.66),  # starts outside: not clipped
        dict(image_id=7, category_id=1, bbox=[1.0, 2.0, 30.0, 40.0], score=below),  # just below: dropped
        dict(image_id=19, category_id=3, bbox=[0.0, 0.0, 10.0, 10.0], score=0.99),  # not a person
        dict(image_id=19, category_id=1, bbox=[20.0, 30.0, 40.0, 50.0], score=0.05, segmentation=[[20, 30, 60, 30, 60, 80]]),
        dict(image_id=42, category_id=1, bbox=[200.125, 100.0, 80.0, 120.0, 0.5], score=0.31),  # a fifth value is cut off
        dict(image_id=7, category_id=1, bbox=[30.0, 12.5, 60.0, 120.0], score=0.2999),
        dict(image_id=42, category_id=1, bbox=[0.0, 0.0, 319.0, 239.0], score=1.0),
    ]


def record(sample, tag, arrays):
    out = []
    for k, v in sample.items():
        if isinstance(v, np.ndarray):
            arrays[f"{tag}/{k}"] = v
            out.append([k, "ndarray", None])
        elif isinstance(v, tuple):
            out.append([k, "tuple", list(v)])
        else:
            out.append([k, type(v).__name__, v])
    return out


def main():
    reg = mgd.load_reference()
    base = sys.modules["mmpose.datasets.datasets.base.base_coco_style_dataset"]
    base.bbox_xywh2xyxy = load_reference_bbox().bbox_xywh2xyxy
    ann, dets = annotation_file(), detections_file()
    arrays, cases = {}, {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        ann_path, det_path = os.path.join(tmp, "person_keypoints.json"), os.path.join(tmp, "detections.json")
        json.dump(ann, open(ann_path, "w"))
        json.dump(dets, open(det_path, "w"))
        os.chdir(mgd.REF)
        try:
            kw = dict(ann_file=ann_path, bbox_file=det_path, data_root="data/root/", data_prefix=dict(img="val2017/"), test_mode=True,
                      pipeline=[])
            for tag, filter_cfg in (("all", None), ("thr", dict(bbox_score_thr=THR))):
                d = reg["CocoDataset"](filter_cfg=filter_cfg, **kw)
                d.filter_cfg = filter_cfg  # (mmengine's BaseDataset keeps it and filters inside full_init; the stub does neither)
                d.data_list = d.filter_data()
                cases[tag] = [record(d.get_data_info(i), f"{tag}/{i}", arrays) for i in range(len(d))]
        finally:
            os.chdir(cwd)
    doc = dict(annotations=ann, detections=dets, bbox_score_thr=THR, data_root="data/root/", data_prefix="val2017/", cases=cases)
    with open(os.path.join(HERE, "detboxes_cases.json"), "w") as f:
        json.dump(doc, f, indent=0)
    np.savez_compressed(os.path.join(HERE, "detboxes_cases.npz"), **arrays)
    print({k: len(v) for k, v in cases.items()}, len(arrays), "arrays")


if __name__ == "__main__":
    main()
