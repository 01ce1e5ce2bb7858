"""Keypoint results files on the MI355X: a seeded synthetic CropCOCO + COCO pair through ``runner.test_dataset`` with
``outfile_prefix`` set, the files read back with ``datasets.COCO.loadRes`` and scored by ``evaluation.COCOeval`` (the
device evaluator), against the run's own metrics, the oracle evaluator, ``tools/test.py`` and ``tools/eval_results.py``
in child processes, and a ``format_only`` metric fed the same predictions. All data is generated here."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EVAL_CONFIG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_cropcoco-coco-val-256x192.py")
NAMES = ("CropCOCO", "COCO")  # metric i of the config <-> dataset i
DATASET_NAMES = dict(CropCOCO="coco_crop", COCO="coco")
SETTINGS = ((False, False, False), (True, False, False), (False, True, False), (True, True, True))  # extended, bbox, no border


def _same(a, b):
    return a.keys() == b.keys() and all((isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k] for k in a)


def _roots(tmp):
    from probpose_code_amd import synthetic as S

    roots = [str(tmp / "cropcoco") + "/", str(tmp / "coco") + "/"]
    S.synthetic_coco_dataset(roots[0], 13, seed=21, persons=(1, 8), id_base=1)
    S.synthetic_coco_dataset(roots[1], 15, seed=22, persons=(1, 8), id_base=2)
    return roots


def _options(roots, prefixes=None):
    opts = {f"test_dataloader.dataset.datasets.{i}.data_root": r for i, r in enumerate(roots)}
    for i, p in enumerate(prefixes or []):
        opts[f"test_evaluator.metrics.{i}.outfile_prefix"] = p
    return opts


def _ann(root):
    return os.path.join(root, "annotations", "person_keypoints_val2017.json")


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    import torch

    from probpose_code_amd import apis, runner, synthetic
    from probpose_code_amd.config import Config
    from probpose_code_amd.datasets import build_dataset

    tmp = tmp_path_factory.mktemp("result_files")
    roots = _roots(tmp)
    prefixes = [str(tmp / "run" / n.lower()) for n in NAMES]
    cfg = Config.fromfile(EVAL_CONFIG)
    cfg.merge_from_dict(_options(roots, prefixes))
    model = apis.init_model(cfg, dict(state_dict=synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device="cuda:0")
    dataset = build_dataset(cfg.test_dataloader.dataset)
    ev = runner.build_evaluator(cfg.test_evaluator, dataset, device="cuda:0")
    batches = []
    metrics = runner.test_dataset(model, dataset, ev, batch_size=64, workers=4, sink=batches.append)
    torch.cuda.synchronize()
    by_name = {}
    for s in (s for b in batches for s in b):
        d = runner.sample_to_dict(s)
        by_name.setdefault(d["dataset_name"], []).append(d)
    return dict(tmp=tmp, roots=roots, prefixes=prefixes, cfg=cfg, dataset=dataset, evaluator=ev, metrics=metrics, by_name=by_name)


@pytest.mark.gpu
def test_outfile_prefix_leaves_the_metrics_as_they_are(run):
    from probpose_code_amd import runner

    cfg = run["cfg"]
    assert [m.outfile_prefix for m in run["evaluator"].metrics] == run["prefixes"]
    for p in run["prefixes"]:
        res = json.loads(_read(p + ".keypoints.json"))
        assert len(res) > 20 and all(len(r["keypoints"]) == 51 and "bbox" in r and len(r["visibility"]) == 17 for r in res)
    plain_cfg = dict(cfg.test_evaluator)
    plain_cfg["metrics"] = [dict(m, outfile_prefix=None) for m in cfg.test_evaluator["metrics"]]
    plain = runner.build_evaluator(plain_cfg, run["dataset"], device="cuda:0")
    ref = {}
    for name, metric in plain.metrics_dict.items():
        assert metric.outfile_prefix is None
        metric.process(None, run["by_name"][name])
        ref.update(metric.compute_metrics())
    assert "CropCOCO/Ex_AP" in ref and "COCO/AP" in ref
    assert _same(run["metrics"], ref), (run["metrics"], ref)


@pytest.mark.gpu
def test_loaded_file_scores_as_the_run_did(run):
    """COCOeval(gt, gt.loadRes(file)) over the config's settings equals compute_metrics exactly (JSON floats round-trip),
    more settings equal a metric that ran them, and every evaluation matches the oracle evaluator to 1e-12."""
    from oracle import exmap_ref
    from probpose_code_amd.datasets import COCO
    from probpose_code_amd.evaluation import COCO_SIGMAS, COCOeval

    metrics = run["metrics"]
    for name, root, prefix, metric in zip(NAMES, run["roots"], run["prefixes"], run["evaluator"].metrics):
        gt = COCO(_ann(root))
        dt = gt.loadRes(prefix + ".keypoints.json")
        thr = metric.prob_thr
        more = None
        for ext, mbb, nobrd in SETTINGS:
            e = COCOeval(gt, dt, "keypoints", extended_oks=ext, match_by_bbox=mbb, confidence_thr=thr, padding=1.25, ignore_near_bbox=nobrd,
                         device="cuda:0")
            e.evaluate()
            e.accumulate()
            e.summarize()
            key = f"{name}/" + ("Ex_" if ext else "") + ("bbox_" if mbb else "") + "{}" + ("_NoBrd" if nobrd else "")
            if not mbb and not nobrd:
                got = {key.format(k): float(v) for k, v in zip(e.stats_names, e.stats)}
                assert _same(got, {k: metrics[k] for k in got}), (name, ext)
            else:  # settings beyond the config: a CocoMetric that runs them on the same predictions
                if more is None:
                    from probpose_code_amd.evaluation import CocoMetric

                    m = CocoMetric(metric.gt, extended=[s[0] for s in SETTINGS], match_by_bbox=[s[1] for s in SETTINGS],
                                   ignore_border_points=[s[2] for s in SETTINGS], padding=1.25, score_thresh_type="prob",
                                   keypoint_score_thr=0.45, prob_thr=thr, prefix=name, device="cuda:0")
                    m.process(None, run["by_name"][DATASET_NAMES[name]])
                    more = m.compute_metrics()
                got = {key.format(k): float(v) for k, v in zip(e.stats_names, e.stats)}
                assert _same(got, {k: more[k] for k in got}), (name, ext, mbb, nobrd)
            ref = exmap_ref.evaluate(gt.loadAnns(gt.getAnnIds()), dt.dataset["annotations"], COCO_SIGMAS, extended_oks=ext,
                                     match_by_bbox=mbb, confidence_thr=thr, padding=1.25, ignore_near_bbox=nobrd)
            assert list(ref["stats_names"]) == list(e.stats_names)
            np.testing.assert_allclose(e.stats, np.asarray(ref["stats"], np.float64), rtol=0, atol=1e-12, err_msg=f"{name} {ext} {mbb}")
        assert all(v >= 0 for k, v in metrics.items() if k.startswith(f"{name}/A"))  # instances were evaluated (-1: none)


@pytest.mark.gpu
def test_image_subset_narrows_the_evaluation(run):
    from probpose_code_amd.datasets import COCO
    from probpose_code_amd.evaluation import COCOeval

    root, prefix, thr = run["roots"][1], run["prefixes"][1], run["evaluator"].metrics[1].prob_thr
    gt = COCO(_ann(root))
    dt = gt.loadRes(prefix + ".keypoints.json")
    ids = gt.getImgIds()[1::2]
    e = COCOeval(gt, dt, "keypoints", extended_oks=True, confidence_thr=thr, device="cuda:0")
    e.params.imgIds = ids
    e.evaluate()
    e.accumulate()
    e.summarize()
    keep = set(ids)  # the same evaluation on lists holding only those images
    f = COCOeval([a for a in gt.loadAnns(gt.getAnnIds()) if a["image_id"] in keep], [a for a in dt.dataset["annotations"] if a["image_id"] in keep],
                 "keypoints", extended_oks=True, confidence_thr=thr, device="cuda:0")
    f.evaluate()
    f.accumulate()
    f.summarize()
    assert np.array_equal(e.stats, f.stats, equal_nan=True)
    full = COCOeval(gt, dt, "keypoints", extended_oks=True, confidence_thr=thr, device="cuda:0")
    full.evaluate()
    assert e._meta["N_gt"] < full._meta["N_gt"]


@pytest.mark.gpu
def test_format_only_writes_the_same_bytes(run):
    from probpose_code_amd import runner

    for name, prefix in zip(NAMES, run["prefixes"]):
        preds = run["by_name"][DATASET_NAMES[name]]
        out = str(run["tmp"] / "format_only" / name.lower())
        m = runner.build_metric(dict(type="CocoMetric", format_only=True, outfile_prefix=out, score_thresh_type="prob",
                                     keypoint_score_thr=0.45, extended=[False, True], padding=1.25, prefix=name), device="cuda:0")
        assert m.gt is None
        m.process(None, preds)
        assert m.compute_metrics() == {}
        assert _read(out + ".keypoints.json") == _read(prefix + ".keypoints.json"), name


@pytest.mark.gpu
def test_cli_test_and_eval_results_print_the_same_numbers(run):
    tmp = run["tmp"]
    cli_prefixes = [str(tmp / "cli" / n.lower()) for n in NAMES]
    out = tmp / "cli_metrics.json"
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.join(ROOT, "tools", "test.py"), EVAL_CONFIG, "synthetic",
           "--cfg-options"] + [f"{k}={v}" for k, v in _options(run["roots"], cli_prefixes).items()] + ["--out", str(out), "--workers", "4"]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    test_metrics = json.load(open(out))
    assert _same(test_metrics, run["metrics"])
    test_lines = {ln for ln in r.stdout.splitlines() if ": " in ln}
    for name, root, cli_prefix, prefix, metric in zip(NAMES, run["roots"], cli_prefixes, run["prefixes"], run["evaluator"].metrics):
        assert _read(cli_prefix + ".keypoints.json") == _read(prefix + ".keypoints.json"), name
        mout = tmp / f"eval_{name}.json"
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "eval_results.py"), _ann(root),
               cli_prefix + ".keypoints.json", "--confidence-thr", repr(float(metric.prob_thr)), "--padding", "1.25", "--prefix", name,
               "--out", str(mout)]
        e = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert e.returncode == 0, e.stdout[-3000:] + e.stderr[-3000:]
        got = json.load(open(mout))
        assert f"{name}/AP" in got and f"{name}/Ex_AP" in got and len(got) == len([k for k in test_metrics if k.startswith(name + "/")
                                                                                      and "prob_" not in k])
        assert _same(got, {k: test_metrics[k] for k in got}), name
        printed = [ln for ln in e.stdout.splitlines() if ": " in ln]
        assert len(printed) == len(got) and set(printed) <= test_lines, name
        ex = subprocess.run(cmd[:-2] + ["--extended"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert ex.returncode == 0, ex.stderr[-3000:]
        only = [ln for ln in ex.stdout.splitlines() if ": " in ln]
        assert only and all(ln.startswith(f"{name}/Ex_") for ln in only) and set(only) <= test_lines
