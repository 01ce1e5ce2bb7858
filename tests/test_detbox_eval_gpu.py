"""Evaluation on detector boxes end to end on the MI355X: ``runner.test_dataset`` over ``datasets.DetectionBoxes`` with the
metric's OKS-NMS on the device and on the host (the same metrics, the same results file byte for byte), the score threshold,
and ``tools/test.py --bbox-file ... --nms device`` in a child process. All data is generated here."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BASE_CONFIG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")
LOW = 0.05  # the detector's low scores; the threshold test cuts at 0.3

CONFIG = '''_base_ = [{base!r}]
val_pipeline = [
    dict(type="LoadImage", pad_to_aspect_ratio=False),
    dict(type="GetBBoxCenterScale"),
    dict(type="TopdownAffine", input_size=(192, 256), use_udp=True, input_padding=1.25),
    dict(type="PackPoseInputs"),
]
test_dataloader = dict(_delete_=True, batch_size=8, dataset=dict(
    type="CocoDataset", data_root={root!r}, data_mode="topdown", ann_file="annotations/person_keypoints_val2017.json",
    test_mode=True, pipeline=val_pipeline, data_prefix=dict(img="val2017/")))
test_evaluator = dict(type="CocoMetric", keypoint_score_thr=0.0)
'''


def _same(a, b):
    return a.keys() == b.keys() and all((isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k] for k in a)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """Three small JPEGs with six persons, a detections file of twelve entries (the persons' boxes, jittered; exact duplicates
    with another score; low scores; one box of another category), a single-dataset ProbPose-S config, the model."""
    from probpose_code_amd import apis, synthetic
    from probpose_code_amd.config import Config

    tmp = tmp_path_factory.mktemp("detbox_eval")
    root = str(tmp / "coco") + "/"
    assert synthetic.synthetic_coco_dataset(root, 3, seed=21, image_size=(320, 240), fmt="jpg", persons=(2, 2), invalid_image=False) == 6
    anns = json.load(open(os.path.join(root, "annotations", "person_keypoints_val2017.json")))["annotations"]
    rng = np.random.default_rng(4)
    dets = []
    for n, a in enumerate(anns):
        x, y, w, h = a["bbox"]
        box = [round(x + float(rng.uniform(-3, 3)), 2), round(y + float(rng.uniform(-3, 3)), 2), round(w * float(rng.uniform(0.95, 1.05)), 2),
               round(h * float(rng.uniform(0.95, 1.05)), 2)]
        dets.append(dict(image_id=a["image_id"], category_id=1, bbox=box, score=round(float(rng.uniform(0.6, 0.99)), 3)))
        if n % 2 == 0:  # the same box again with another score: the same crop, the same pose
            dets.append(dict(image_id=a["image_id"], category_id=1, bbox=list(box), score=round(float(rng.uniform(0.35, 0.55)), 3)))
    dets.append(dict(image_id=anns[0]["image_id"], category_id=1, bbox=[200.0, 10.0, 90.0, 200.0], score=LOW))
    dets.append(dict(image_id=anns[-1]["image_id"], category_id=1, bbox=[5.0, 100.0, 60.0, 120.0], score=LOW))
    dets.append(dict(image_id=anns[2]["image_id"], category_id=3, bbox=[0.0, 0.0, 50.0, 50.0], score=0.9))
    assert len(dets) == 12
    det_file = tmp / "detections.json"
    det_file.write_text(json.dumps(dets))
    cfg_file = tmp / "probpose_small_coco_single.py"
    cfg_file.write_text(CONFIG.format(base=BASE_CONFIG, root=root))
    cfg = Config.fromfile(str(cfg_file))
    model = apis.init_model(cfg, dict(state_dict=synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device="cuda:0")
    return dict(tmp=tmp, cfg=cfg, cfg_file=str(cfg_file), det_file=str(det_file), dets=dets, model=model)


def _run(setup, backend, thr=None, sink=None):
    from probpose_code_amd import runner
    from probpose_code_amd.datasets import DetectionBoxes, build_dataset

    cfg = setup["cfg"]
    view = DetectionBoxes(build_dataset(cfg.test_dataloader.dataset), setup["det_file"], thr)
    prefix = str(setup["tmp"] / f"results_{backend}_{thr}")
    ev = runner.build_evaluator(dict(cfg.test_evaluator, nms_backend=backend, outfile_prefix=prefix), view, device="cuda:0")
    metrics = runner.test_dataset(setup["model"], view, ev, batch_size=8, workers=2, sink=sink)
    return view, ev.metrics[0], metrics, prefix + ".keypoints.json"


@pytest.fixture(scope="module")
def runs(setup):
    return {b: _run(setup, b) for b in ("device", "host")}


@pytest.mark.gpu
def test_backends_agree_and_the_detector_score_takes_part(setup, runs):
    from probpose_code_amd.evaluation import instance_score

    (view, dev, m_dev, f_dev), (_, host, m_host, f_host) = runs["device"], runs["host"]
    assert len(view) == 11 and dev.nms_backend == "device" and host.nms_backend == "host"
    assert m_dev and _same(m_dev, m_host), (m_dev, m_host)
    assert open(f_dev, "rb").read() == open(f_host, "rb").read()
    assert dev.nms_fallbacks == 0
    res = json.load(open(f_dev))
    boxes = [(r["image_id"], tuple(r["bbox"])) for r in res]
    assert len(set(boxes)) == len(boxes) and 3 <= len(res) <= 8  # of a duplicated box at most one is left
    valid = dev._instances()
    flat = [p for persons in valid.values() for p in persons]
    assert [float(p["score"]) for p in flat] == [r["score"] for r in res]
    by_id = {i: d for i, d in enumerate(d for d in setup["dets"] if d["category_id"] == 1)}
    for p in flat:
        mean_kpt = instance_score(1.0, p["keypoint_scores"], p["keypoint_probs"], keypoint_score_thr=0.0)
        assert p["bbox_score"] == np.float32(by_id[p["id"]]["score"])  # the detector's score reached the metric
        assert 0 < p["score"] < mean_kpt and p["score"] == p["bbox_score"] * mean_kpt
    # of a duplicated box the entry with the lower detector score never stays
    kept = {p["id"] for p in flat}
    twins = 0
    for i, d in by_id.items():
        twin = [j for j, e in by_id.items() if j != i and e["image_id"] == d["image_id"] and e["bbox"] == d["bbox"]]
        if twin and d["score"] < by_id[twin[0]]["score"]:
            assert i not in kept
            twins += 1
    assert twins == 3


@pytest.mark.gpu
def test_score_threshold_drops_boxes_before_the_model(setup):
    seen = []
    view, metric, metrics, _ = _run(setup, "device", thr=0.3, sink=seen.append)
    expected = sum(d["category_id"] == 1 and d["score"] >= 0.3 for d in setup["dets"])
    assert expected == 9 and len(view) == expected and sum(len(b) for b in seen) == expected
    assert all(float(s.gt_instances.bbox_scores[0]) >= 0.3 for b in seen for s in b)
    assert metrics and metric.nms_fallbacks == 0


@pytest.mark.gpu
def test_tools_test_cli_with_bbox_file_writes_the_same_metrics(setup, runs):
    out = setup["tmp"] / "m.json"
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "test.py"), setup["cfg_file"], "synthetic",
           "--bbox-file", setup["det_file"], "--nms", "device", "--out", str(out), "--workers", "2"]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "11 instances" in r.stdout
    assert _same(json.load(open(out)), runs["device"][2])
