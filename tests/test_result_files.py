"""Keypoint results files (host side): ``CocoMetric(outfile_prefix / format_only)`` writes the reference's
``results2json`` file byte for byte (tests/golden/make_golden_result_files.py ran the reference's own ``compute_metrics``),
the option checks of the metric and of ``runner.build_metric``, ``datasets.COCO.loadRes``, and the CLI's flags."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "result_files.json")))


def _decode(v):
    if isinstance(v, dict) and set(v) == {"dtype", "shape", "data"}:
        return np.array(v["data"], v["dtype"]).reshape(v["shape"])
    if isinstance(v, dict):
        return {k: _decode(x) for k, x in v.items()}
    return v


def _gt_file(tmp_path):
    """Three images (one without annotations), two persons."""
    kp = lambda x0, y0: [float(x0 + 3 * k) if i < 2 else 2 for k in range(17) for i in range(3)]  # noqa: E731
    doc = dict(images=[dict(id=i, file_name=f"{i}.jpg", width=640, height=480) for i in (7, 3, 9)],
               categories=[dict(id=1, name="person", supercategory="person")],
               annotations=[dict(id=70, image_id=7, category_id=1, iscrowd=0, area=900.0, bbox=[10, 20, 60, 80], keypoints=kp(10, 20)),
                            dict(id=30, image_id=3, category_id=1, iscrowd=0, area=400.0, bbox=[100, 50, 50, 60], keypoints=kp(100, 50))])
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(doc))
    return str(path)


@pytest.mark.parametrize("case", range(len(GOLDEN["cases"])))
def test_format_only_writes_the_reference_file_byte_for_byte(tmp_path, case):
    from probpose_code_amd.evaluation import CocoMetric

    c = GOLDEN["cases"][case]
    samples = [_decode(s) for s in GOLDEN["samples"]]
    kept = copy.deepcopy(samples)
    prefix = str(tmp_path / "out" / "results")  # a directory that does not exist yet
    m = CocoMetric(None, format_only=True, outfile_prefix=prefix, device="cpu", **c["kwargs"])  # no ground truth, no GPU
    for lo, hi in GOLDEN["batches"]:
        m.process(None, samples[lo:hi])
    assert m.compute_metrics() == {}
    with open(prefix + ".keypoints.json", "rb") as f:
        assert f.read() == c["file"].encode("utf-8")
    res = json.loads(c["file"])
    assert len(res) == c["n_results"] and len({r["image_id"] for r in res}) == 4
    assert any("bbox" in r for r in res) and any("bbox" not in r for r in res)
    for s, k in zip(samples, kept):  # the samples are not modified
        assert all(np.array_equal(s["pred_instances"][f], k["pred_instances"][f]) for f in k["pred_instances"])


def test_fixture_covers_duplicates_and_suppression():
    lo0, hi0 = GOLDEN["batches"][0]
    lo1, hi1 = GOLDEN["batches"][1]
    assert lo1 < hi0 and hi1 == len(GOLDEN["samples"])  # samples in both batches
    n = {json.dumps(c["kwargs"], sort_keys=True): c["n_results"] for c in GOLDEN["cases"]}
    assert min(n.values()) == len(GOLDEN["samples"]) - 1 and max(n.values()) == len(GOLDEN["samples"])


def test_metric_option_checks():
    from probpose_code_amd.evaluation import CocoMetric

    with pytest.raises(AssertionError, match="outfile_prefix"):
        CocoMetric(None, format_only=True)
    with pytest.raises(AssertionError, match="outfile_prefix"):
        CocoMetric([], format_only=True, outfile_prefix=None)
    with pytest.raises(ValueError, match="ground truth"):
        CocoMetric(None)
    m = CocoMetric([], outfile_prefix="/tmp/x")
    assert m.outfile_prefix == "/tmp/x" and m.format_only is False
    assert CocoMetric([]).outfile_prefix is None  # by default nothing is written


def test_build_metric_passes_the_file_options(tmp_path):
    from probpose_code_amd import runner

    gt = _gt_file(tmp_path)
    m = runner.build_metric(dict(type="CocoMetric", ann_file=gt, outfile_prefix=str(tmp_path / "r"), prefix="COCO"))
    assert m.outfile_prefix == str(tmp_path / "r") and not m.format_only and len(m.gt) == 2
    m = runner.build_metric(dict(type="CocoMetric", format_only=True, outfile_prefix=str(tmp_path / "r")))  # no ann_file
    assert m.format_only and m.gt is None
    with pytest.raises(AssertionError):
        runner.build_metric(dict(type="CocoMetric", ann_file=gt, format_only=True))
    with pytest.raises(ValueError):
        runner.build_metric(dict(type="CocoMetric", outfile_prefix=str(tmp_path / "r")))  # evaluation needs a ground truth
    for k, v in (("collect_device", "gpu"), ("pred_converter", dict(num_keypoints=17)), ("gt_converter", dict(num_keypoints=17))):
        with pytest.raises(NotImplementedError, match=k):
            runner.build_metric(dict(type="CocoMetric", ann_file=gt, **{k: v}))


def test_load_res_keypoint_rule(tmp_path):
    from probpose_code_amd.datasets import COCO

    gt = COCO(_gt_file(tmp_path))
    kp = np.arange(51, dtype=np.float64)
    kp[0::3] = np.linspace(5, 40, 17)
    kp[1::3] = np.linspace(90, 20, 17)
    res = [dict(image_id=3, category_id=1, keypoints=kp.tolist(), score=0.5, bbox=[1, 2, 3, 4], visibility=[1.0] * 17),
           dict(image_id=9, category_id=1, keypoints=(kp + 1).tolist(), score=0.25),
           dict(image_id=3, category_id=1, keypoints=(kp * 2).tolist(), score=0.75)]
    kept = copy.deepcopy(res)
    path = tmp_path / "res.json"
    path.write_text(json.dumps(res))
    for src in (res, str(path)):
        dt = gt.loadRes(src)
        assert res == kept  # the caller's list is not written into
        anns = dt.dataset["annotations"]
        assert [a["id"] for a in anns] == [1, 2, 3] and sorted(dt.anns) == [1, 2, 3]
        assert anns[0]["bbox"] == [5.0, 20.0, 35.0, 70.0] and anns[0]["area"] == 35.0 * 70.0  # the file's bbox is replaced
        assert anns[1]["bbox"] == [6.0, 21.0, 35.0, 70.0] and anns[2]["area"] == 70.0 * 140.0
        assert anns[0]["score"] == 0.5 and anns[0]["visibility"] == [1.0] * 17 and anns[0]["keypoints"] == kp.tolist()
        assert dt.dataset["categories"] == gt.dataset["categories"] and dt.dataset["categories"] is not gt.dataset["categories"]
        assert dt.getImgIds() == gt.getImgIds() == [7, 3, 9]
        assert [a["id"] for a in dt.loadAnns(dt.getAnnIds(imgIds=[3]))] == [1, 3] and dt.getAnnIds(imgIds=[7]) == []
    with pytest.raises(AssertionError, match="do not correspond"):
        gt.loadRes([dict(res[0]), dict(res[1], image_id=4)])
    with pytest.raises(ValueError):
        gt.loadRes([])
    with pytest.raises(NotImplementedError):
        gt.loadRes([dict(image_id=3, category_id=1, bbox=[1, 2, 3, 4], score=0.5)])
    with pytest.raises(NotImplementedError):
        gt.loadRes([res[0], dict(image_id=3, category_id=1, segmentation=[[1, 2, 3, 4]], score=0.5)])


def test_compute_metrics_loads_what_results2json_writes(tmp_path, monkeypatch):
    """The evaluator receives the results read back by loadRes (ids, areas, boxes from the keypoints); stopped before the
    GPU by a stand-in that records its inputs."""
    from probpose_code_amd import evaluation as E

    seen = []

    class Stop(Exception):
        pass

    def fake(gts, dts, *a, **k):
        seen.append((gts, dts))
        raise Stop

    monkeypatch.setattr(E, "COCOeval", fake)
    samples = [_decode(s) for s in GOLDEN["samples"]]
    m = E.CocoMetric([], outfile_prefix=str(tmp_path / "r"), prob_thr=0.5, **GOLDEN["cases"][0]["kwargs"])
    m.process(None, samples)
    with pytest.raises(Stop):
        m.compute_metrics()
    res = json.loads(GOLDEN["cases"][0]["file"])
    assert open(str(tmp_path / "r") + ".keypoints.json").read() == GOLDEN["cases"][0]["file"]
    dts = seen[0][1]
    assert [d["id"] for d in dts] == list(range(1, len(res) + 1))
    for r, d in zip(res, dts):
        kp = np.array(r["keypoints"]).reshape(-1, 3)
        assert d["keypoints"] == r["keypoints"] and d["score"] == r["score"] and d["image_id"] == r["image_id"]
        assert d["bbox"] == [kp[:, 0].min(), kp[:, 1].min(), np.ptp(kp[:, 0]), np.ptp(kp[:, 1])]


def test_eval_results_cli_help_lists_its_flags():
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tools", "eval_results.py"), "--help"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    for flag in ("ann_file", "results_file", "--extended", "--match-by-bbox", "--ignore-border-points", "--padding", "--confidence-thr",
                 "--prefix", "--out", "--device"):
        assert flag in r.stdout, flag
