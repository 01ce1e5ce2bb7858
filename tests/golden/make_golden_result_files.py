"""Golden results files from the REFERENCE's own code (build container only): ``CocoMetric.process`` then
``compute_metrics`` with ``format_only=True``, which scores the instances, drops duplicates, runs the suppression and writes
``{outfile_prefix}.keypoints.json`` through ``results2json`` (mmpose/evaluation/metrics/coco_metric.py:236-358, 459-586,
630-669).

mmengine and xtcocotools are absent here, so coco_metric.py is loaded behind stubs of what it imports: a ``BaseMetric``
holding ``results``, mmengine's ``dump`` for a ``.json`` path (``json.dump`` with its numpy ``default``, text written as is),
``load`` / ``get_local_path``, a silent logger, a dict-backed COCO index (only its ``anns`` are read under ``format_only``),
a dict registry. ``oks_nms`` / ``soft_oks_nms`` (functional/nms.py) and ``bbox_xyxy2xywh`` (structures/bbox/transforms.py)
are the reference's own; the evaluator and the padding search are never reached and are stubbed to None.

Input: a few seeded top-down samples over four images - boxes on some and not on others, an instance the suppression
removes, samples repeated across the two batches, one without ``keypoints_visible``, one with ``bbox_scales``.
Output: result_files.json (the samples, the batches, and per metric setting the reference's exact file text).
Run: python tests/golden/make_golden_result_files.py"""
import contextlib
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

REF = _ref_import.REF
K = 17
SIGMAS = np.array([0.26, 0.25, 0.25, 0.35, 0.35, 0.79, 0.79, 0.72, 0.72, 0.62, 0.62, 1.07, 1.07, 0.87, 0.87, 0.89, 0.89],
                  np.float32) / 10.0  # parse_pose_metainfo keeps the sigmas as float32

CASES = [  # CocoMetric keyword arguments; the first is the ProbPose config's
    dict(score_mode="bbox_keypoint", score_thresh_type="prob", keypoint_score_thr=0.45, nms_mode="oks_nms", nms_thr=0.9),
    dict(score_mode="bbox_keypoint", score_thresh_type="score", keypoint_score_thr=0.2, nms_mode="soft_oks_nms", nms_thr=0.9),
    dict(score_mode="keypoint", nms_mode="none"),
    dict(score_mode="bbox_rle", nms_mode="oks_nms", nms_thr=0.9),
]


def make_samples():
    rng = np.random.default_rng(2026)
    samples = []
    # (image id, persons); images in an order that is not sorted, as in a real dataset
    for img_id, n in ((30, 3), (10, 2), (20, 1), (5, 2)):
        for p in range(n):
            w, h = rng.uniform(60, 250), rng.uniform(120, 400)
            x0, y0 = rng.uniform(0, 640 - w), rng.uniform(0, 480 - h)
            kp = np.stack([rng.uniform(x0, x0 + w, K), rng.uniform(y0, y0 + h, K)], -1)
            if img_id == 30 and p == 2:  # a near copy of person 0: the suppression removes one of the two
                kp = samples[-2]["pred_instances"]["keypoints"][0].astype(np.float64) + rng.normal(0, 0.5, (K, 2))
                x0, y0, w, h = (float(v) for v in samples[-2]["_box"])
            pi = dict(keypoints=kp[None].astype(np.float32), keypoint_scores=rng.uniform(0.05, 1, (1, K)).astype(np.float32),
                      keypoints_probs=rng.beta(3, 1.5, (1, K)).astype(np.float32))
            s = dict(id=int(1000 + 10 * img_id + p), img_id=img_id, _box=[x0, y0, w, h], pred_instances=pi, gt_instances={})
            if img_id != 10:  # the instances of image 10 come without boxes: their entries have no "bbox"
                pi["bboxes"] = np.array([[x0, y0, x0 + w, y0 + h]], np.float32)
            if not (img_id == 5 and p == 1):
                pi["keypoints_visible"] = rng.uniform(0, 1, (1, K)).astype(np.float32)
            if img_id == 20:
                pi["bbox_scores"] = np.array([rng.uniform(0.5, 1)], np.float32)
                s["gt_instances"]["bbox_scales"] = np.array([[w * 1.25, h * 1.25]], np.float32)
            else:
                s["gt_instances"]["bbox_scores"] = np.array([rng.uniform(0.5, 1)], np.float32)
            if p != 1:
                s["category_id"] = 1
            samples.append(s)
    for s in samples:
        del s["_box"]
    return samples


def encode(v):
    if isinstance(v, np.ndarray):
        return dict(dtype=str(v.dtype), shape=list(v.shape), data=v.flatten().tolist())
    if isinstance(v, dict):
        return {k: encode(x) for k, x in v.items()}
    return v


# --------------------------------------------------------------------------------------------------------------- stubs
def _shell(name, path=None):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    sys.modules[name] = m
    return m


def _set_default(obj):  # mmengine/fileio/handlers/json_handler.py
    if isinstance(obj, (set, range)):
        return list(obj)
    if isinstance(obj, np.ndarray):
        return obj.tolist()
    if isinstance(obj, np.generic):
        return obj.item()
    raise TypeError(f"{type(obj)} is unsupported for json dump")


def _dump(obj, file, **kwargs):  # mmengine.fileio.dump to a local .json path: the handler's text, written as is
    kwargs.setdefault("default", _set_default)
    with open(file, "w", encoding="utf-8") as f:
        json.dump(obj, f, **kwargs)


class _COCO:
    def __init__(self, path):
        self.dataset = json.load(open(path))
        self.anns = {a["id"]: a for a in self.dataset.get("annotations", [])}


class _BaseMetric:
    def __init__(self, collect_device="cpu", prefix=None):
        self.collect_device, self.prefix, self.results = collect_device, prefix, []


def load_reference_metric():
    nms = _ref_import.load_reference_nms()
    bbox = _ref_import.load_reference_bbox()
    _shell("mmengine")
    _shell("mmengine.evaluator").BaseMetric = _BaseMetric
    fio = _shell("mmengine.fileio")
    fio.dump, fio.load = _dump, (lambda p: json.load(open(p)))
    fio.get_local_path = contextlib.contextmanager(lambda p: (yield p))
    lg = _shell("mmengine.logging")
    quiet = types.SimpleNamespace(info=lambda *a, **k: None, get_info=lambda *a, **k: None)
    lg.MMLogger = lg.MessageHub = types.SimpleNamespace(get_current_instance=lambda: quiet)
    lg.print_log = lambda *a, **k: None
    _shell("xtcocotools")
    _shell("xtcocotools.coco").COCO = _COCO
    reg = _shell("mmpose.registry")
    reg.METRICS = _ref_import._DictRegistry()
    sys.modules["mmpose.structures.bbox"].bbox_xyxy2xywh = bbox.bbox_xyxy2xywh
    kp = _shell("mmpose.structures.keypoint")
    kp.find_min_padding_exact = kp.fix_bbox_aspect_ratio = None
    _shell("mmpose.evaluation")
    fn = _shell("mmpose.evaluation.functional")
    fn.oks_nms, fn.soft_oks_nms = nms.oks_nms, nms.soft_oks_nms
    fn.transform_ann = fn.transform_pred = fn.transform_sigmas = None
    _shell("mmpose.evaluation.metrics", os.path.join(REF, "mmpose/evaluation/metrics"))
    _shell("mmpose.evaluation.metrics._mask")
    _shell("mmpose.evaluation.metrics._cocoeval").COCOeval = None
    name = "mmpose.evaluation.metrics.coco_metric"
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, "mmpose/evaluation/metrics/coco_metric.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod.CocoMetric


def main():
    CocoMetric = load_reference_metric()
    samples = make_samples()
    batches = [[0, 6], [4, len(samples)]]  # samples 4 and 5 in both batches, as in multi-batch testing
    doc = dict(num_keypoints=K, batches=batches, samples=[encode(s) for s in samples], cases=[])
    with tempfile.TemporaryDirectory() as tmp:
        gt = os.path.join(tmp, "gt.json")  # the metric indexes an annotation file; format_only reads nothing of it
        json.dump(dict(images=[dict(id=i) for i in (30, 10, 20, 5)], annotations=[], categories=[dict(id=1, name="person")]),
                  open(gt, "w"))
        for n, kw in enumerate(CASES):
            prefix = os.path.join(tmp, f"case{n}")
            m = CocoMetric(ann_file=gt, format_only=True, outfile_prefix=prefix, **kw)
            m.dataset_meta = dict(dataset_name="coco", num_keypoints=K, sigmas=SIGMAS)
            for lo, hi in batches:
                m.process(None, [dict(s) for s in samples[lo:hi]])
            assert m.compute_metrics(m.results) == {}
            with open(prefix + ".keypoints.json", encoding="utf-8") as f:
                text = f.read()
            doc["cases"].append(dict(kwargs=kw, n_results=len(json.loads(text)), file=text))
    with open(os.path.join(HERE, "result_files.json"), "w") as f:
        json.dump(doc, f, indent=0)
    print([c["n_results"] for c in doc["cases"]], "results per case;", os.path.getsize(os.path.join(HERE, "result_files.json")), "bytes")


if __name__ == "__main__":
    main()
