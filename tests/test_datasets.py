"""COCO-style datasets, the batch plan, the evaluator routing, list indices in --cfg-options, the evaluation config and the
argument checks of pp_warp_affine_u8_batch - all without a GPU. The dataset samples are held to the reference's own
parse_data_info / _is_valid_instance / get_data_info (tests/golden/make_golden_dataset.py)."""
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EVAL_CONFIG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_cropcoco-coco-val-256x192.py")


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    doc = json.load(open(os.path.join(HERE, "golden", "dataset_cases.json")))
    arrays = np.load(os.path.join(HERE, "golden", "dataset_cases.npz"))
    path = tmp_path_factory.mktemp("ann") / "person_keypoints.json"
    path.write_text(json.dumps(doc["annotations"]))
    return doc, arrays, str(path)


def _kw(doc, path):
    return dict(ann_file=path, data_root=doc["data_root"], data_prefix=dict(img=doc["data_prefix"]), test_mode=True, pipeline=[])


def _check_sample(sample, expected, arrays, tag):
    fields = [f for f in sample if f != "pad_to_contain"]
    assert fields == [e[0] for e in expected], tag  # the same fields in the same order
    for name, kind, value in expected:
        got = sample[name]
        if kind == "ndarray":
            ref = arrays[f"{tag}/{name}"]
            assert isinstance(got, np.ndarray) and got.dtype == ref.dtype and got.shape == ref.shape, (tag, name)
            assert np.array_equal(got, ref, equal_nan=True) and got.tobytes() == ref.tobytes(), (tag, name)
        else:
            assert type(got).__name__ == kind, (tag, name, type(got).__name__, kind)
            got = got.item() if isinstance(got, np.generic) else got
            assert json.loads(json.dumps(got)) == value, (tag, name)


@pytest.mark.parametrize("name", ["CocoDataset", "CocoCropDataset"])
def test_datasets_reproduce_the_reference_samples(golden, name):
    from probpose_code_amd import DATASETS

    doc, arrays, path = golden
    ds = DATASETS.build(dict(type=name, **_kw(doc, path)))
    expected = doc["cases"][name]
    assert len(ds) == len(expected) == 6
    for i, exp in enumerate(expected):
        _check_sample(ds.get_data_info(i), exp, arrays, f"{name}/{i}")
    assert ds.get_data_info(-1)["sample_idx"] == len(ds) - 1


def test_combined_dataset_order_names_and_reference_samples(golden):
    from probpose_code_amd import DATASETS

    doc, arrays, path = golden
    comb = DATASETS.build(dict(type="CombinedDataset", metainfo=dict(from_file="configs/_base_/datasets/coco.py"),
                               datasets=[dict(type="CocoCropDataset", **_kw(doc, path)), dict(type="CocoDataset", **_kw(doc, path))],
                               pipeline=[], test_mode=True))
    expected = doc["cases"]["CombinedDataset"]
    assert len(comb) == len(expected) == 12
    names = [comb.get_data_info(i)["dataset_name"] for i in range(len(comb))]
    assert names == ["coco_crop"] * 6 + ["coco"] * 6
    ids = [comb.get_data_info(i)["id"] for i in range(len(comb))]
    assert ids[:6] == ids[6:] == [101, 102, 103, 105, 31, 51]  # images in getImgIds() order, all-invalid image 7 absent
    for i, exp in enumerate(expected):
        _check_sample(comb.get_data_info(i), exp, arrays, f"CombinedDataset/{i}")
    assert comb.metainfo["dataset_name"] == "coco"


def test_metainfo_reuses_the_package_tables():
    from probpose_code_amd import datasets as D
    from probpose_code_amd.evaluation import COCO_SIGMAS
    from probpose_code_amd.synthetic import COCO_FLIP_INDICES

    a, b = D.coco_pose_metainfo("coco"), D.coco_pose_metainfo("coco_crop")
    assert a["flip_indices"] == list(COCO_FLIP_INDICES) and np.allclose(a["sigmas"], COCO_SIGMAS)
    assert a["dataset_name"] == "coco" and b["dataset_name"] == "coco_crop"
    assert D.CocoDataset.DATASET_NAME == "coco" and D.CocoCropDataset.DATASET_NAME == "coco_crop"


@pytest.mark.parametrize("bad", [dict(bbox_file="dets.json"), dict(data_mode="bottomup"), dict(filter_cfg=dict(bbox_score_thr=0.3)),
                                 dict(indices=10), dict(sample_interval=2)])
def test_unsupported_dataset_options_are_refused(golden, bad):
    from probpose_code_amd import DATASETS

    doc, _, path = golden
    with pytest.raises(NotImplementedError):
        DATASETS.build(dict(type="CocoDataset", **dict(_kw(doc, path), **bad)))


def test_coco_index():
    from probpose_code_amd.datasets import COCO

    import tempfile

    doc = dict(images=[dict(id=4), dict(id=2)], annotations=[dict(id=9, image_id=2), dict(id=8, image_id=4), dict(id=7, image_id=2)],
               categories=[dict(id=1, name="person")])
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(doc, f)
    c = COCO(f.name)
    os.unlink(f.name)
    assert c.getImgIds() == [4, 2]
    assert c.getAnnIds(imgIds=2) == [9, 7] and c.getAnnIds(imgIds=[4, 2]) == [8, 9, 7] and c.getAnnIds() == [9, 8, 7]
    assert [a["id"] for a in c.loadAnns([7, 8])] == [7, 8] and c.loadImgs(2)[0]["id"] == 2
    assert c.getCatIds() == [1] and c.loadCats(c.getCatIds())[0]["name"] == "person"


# ------------------------------------------------------------------------------------------------------------ batch plan
def test_batch_plan_covers_every_instance_once_in_order():
    from probpose_code_amd.runner import last_use, plan_batches

    # image a: 2 instances, b: 3 (split across batches 0 / 1), c: 1, d: 4 (split across 1 / 2), e: 1 (last, partial batch)
    keys = ["a", "a", "b", "b", "b", "c", "d", "d", "d", "d", "e"]
    plan = plan_batches(keys, 4)
    assert [b.indices for b in plan] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
    assert sum((b.indices for b in plan), []) == list(range(len(keys)))
    assert [b.images for b in plan] == [["a", "b"], ["b", "c", "d"], ["d", "e"]]
    assert [b.crop_image for b in plan] == [[0, 0, 1, 1], [0, 1, 2, 2], [0, 0, 1]]
    for b in plan:  # the tables name the right image for every crop
        assert [b.images[j] for j in b.crop_image] == [keys[i] for i in b.indices]
    assert last_use(plan) == dict(a=0, b=1, c=1, d=2, e=2)
    assert plan_batches([], 4) == [] and len(plan_batches(keys, 64)) == 1
    with pytest.raises(ValueError):
        plan_batches(keys, 0)


def test_batch_plan_crosses_the_dataset_boundary(golden):
    from probpose_code_amd import DATASETS
    from probpose_code_amd.runner import plan_batches

    doc, _, path = golden
    comb = DATASETS.build(dict(type="CombinedDataset", metainfo=dict(from_file="configs/_base_/datasets/coco.py"),
                               datasets=[dict(type="CocoCropDataset", **_kw(doc, path)), dict(type="CocoDataset", **_kw(doc, path))]))
    infos = [comb.get_data_info(i) for i in range(len(comb))]
    plan = plan_batches([d["img_path"] for d in infos], 4)
    assert [len(b.indices) for b in plan] == [4, 4, 4]
    mid = [infos[i]["dataset_name"] for i in plan[1].indices]
    assert mid == ["coco_crop", "coco_crop", "coco", "coco"]
    # both datasets use the same files here: image 3's path is read in batch 1 by both datasets' instances
    assert [plan[1].images[j] for j in plan[1].crop_image] == [infos[i]["img_path"] for i in plan[1].indices]


# ------------------------------------------------------------------------------------------------------------ evaluator
class _StubMetric:
    def __init__(self, tag):
        self.tag, self.seen = tag, []

    def process(self, data_batch, data_samples):
        self.seen.extend(s["id"] for s in data_samples)

    def compute_metrics(self):
        return {f"{self.tag}/AP": float(len(self.seen)), f"{self.tag}/ids": list(self.seen)}


def test_multi_dataset_evaluator_routes_by_dataset_name_and_prefixes():
    from probpose_code_amd import EVALUATORS

    crop, coco = _StubMetric("CropCOCO"), _StubMetric("COCO")
    ev = EVALUATORS.build(dict(type="MultiDatasetEvaluator", metrics=[crop, coco],
                               datasets=[dict(type="CocoCropDataset"), dict(type="CocoDataset")]))
    assert list(ev.metrics_dict) == ["coco_crop", "coco"]
    ev.process([dict(id=1, dataset_name="coco"), dict(id=2, dataset_name="coco_crop"), dict(id=3, dataset_name="coco")])
    ev.process([dict(id=4, dataset_name="coco_crop")])
    assert crop.seen == [2, 4] and coco.seen == [1, 3]
    assert ev.evaluate() == {"CropCOCO/AP": 2.0, "CropCOCO/ids": [2, 4], "COCO/AP": 2.0, "COCO/ids": [1, 3]}
    with pytest.raises(KeyError):
        ev.process([dict(id=5, dataset_name="mpii")])


def test_evaluator_builds_coco_metrics_from_the_config(golden):
    from probpose_code_amd import Config, runner
    from probpose_code_amd.datasets import build_dataset
    from probpose_code_amd.evaluation import CocoMetric

    doc, _, path = golden
    cfg = Config.fromfile(EVAL_CONFIG)
    for i in (0, 1):
        cfg.merge_from_dict({f"test_dataloader.dataset.datasets.{i}.ann_file": path,
                             f"test_dataloader.dataset.datasets.{i}.data_root": doc["data_root"]})
    ds = build_dataset(cfg.test_dataloader.dataset)
    ev = runner.build_evaluator(cfg.test_evaluator, ds, device="cpu")
    assert list(ev.metrics_dict) == ["coco_crop", "coco"]
    for m, prefix in zip(ev.metrics, ("CropCOCO", "COCO")):
        assert isinstance(m, CocoMetric) and m.prefix == prefix
        assert m.extended == [False, True] and m.score_thresh_type == "prob" and m.keypoint_score_thr == 0.45 and m.padding == 1.25
        assert [g["id"] for g in m.gt] == [a["id"] for a in sorted(doc["annotations"]["annotations"],
                                                                   key=lambda a: [11, 3, 7, 5].index(a["image_id"]))]


# ------------------------------------------------------------------------------------------------------------ config
def test_merge_from_dict_indexes_lists_and_keeps_old_keys():
    from probpose_code_amd.config import Config

    cfg = Config(dict(a=dict(b=[dict(c=1), dict(c=2)], d=3), e=[1, 2, 3]))
    cfg.merge_from_dict({"a.b.1.c": 5, "a.d": 4, "e.0": 9, "a.new.key": "x", "f": 1, "a.b.-1.g": 7})
    assert cfg.a.b[0].c == 1 and cfg.a.b[1].c == 5 and cfg.a.b[1].g == 7
    assert cfg.a.d == 4 and cfg.e == [9, 2, 3] and cfg.a.new.key == "x" and cfg.f == 1
    cfg.merge_from_dict({"g.0": 1})  # a digit key under a dict is a dict key, as before
    assert cfg.g == {"0": 1}
    with pytest.raises(KeyError):
        cfg.merge_from_dict({"a.b.2.c": 1})
    with pytest.raises(KeyError):
        cfg.merge_from_dict({"a.b.x": 1})


def test_evaluation_config_loads():
    from probpose_code_amd.config import Config

    cfg = Config.fromfile(EVAL_CONFIG)
    ds = cfg.test_dataloader.dataset
    assert ds.type == "CombinedDataset" and [d.type for d in ds.datasets] == ["CocoCropDataset", "CocoDataset"]
    assert [t["type"] for t in ds.pipeline] == ["LoadImage", "GetBBoxCenterScale", "TopdownAffine", "PackPoseInputs"]
    assert cfg.test_dataloader.batch_size == 64 and cfg.test_dataloader.sampler == dict(type="DefaultSampler", shuffle=False, round_up=False)
    ev = cfg.test_evaluator
    assert ev.type == "MultiDatasetEvaluator" and [m.prefix for m in ev.metrics] == ["CropCOCO", "COCO"]
    assert [d.type for d in ev.datasets] == ["CocoCropDataset", "CocoDataset"]
    assert cfg.model.type == "TopdownPoseEstimator"  # the model comes from the base config
    cfg.merge_from_dict({"test_dataloader.dataset.datasets.1.data_root": "/data/coco/"})
    assert cfg.test_dataloader.dataset.datasets[1].data_root == "/data/coco/"
    assert cfg.test_dataloader.dataset.datasets[0].data_root == "PATH/TO/CropCOCO/DATASET/"


def test_cli_parses_cfg_options():
    import importlib.util

    spec = importlib.util.spec_from_file_location("pp_tools_test", os.path.join(ROOT, "tools", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opts = mod.parse_cfg_options(["a.0.b=/data/x/", "n=3", "f=0.5", "l=[1,2]", "t=true", "s=abc"])
    assert opts == {"a.0.b": "/data/x/", "n": 3, "f": 0.5, "l": [1, 2], "t": True, "s": "abc"}


# ------------------------------------------------------------------------------------------------------------ C entry
def test_batch_warp_entry_rejects_bad_arguments():
    from probpose_code_amd import _lib

    f = _lib.lib.pp_warp_affine_u8_batch
    P = 4096  # a non-NULL address: argument checks run before anything is read or launched
    good = dict(images=P, hw=P, c=3, crop=P, inv=P, mh=480, mw=640, out=P, n=4, oh=256, ow=192)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["images"], a["hw"], a["c"], a["crop"], a["inv"], a["mh"], a["mw"], a["out"], a["n"], a["oh"], a["ow"], None)

    for k in ("images", "hw", "crop", "inv", "out"):
        assert call(**{k: None}) == _lib.PP_ERR_INVALID_ARG, k
    assert call(c=0) == _lib.PP_ERR_INVALID_ARG and call(c=5) == _lib.PP_ERR_INVALID_ARG
    assert call(mh=0) == _lib.PP_ERR_INVALID_ARG and call(oh=0) == _lib.PP_ERR_INVALID_ARG and call(n=-1) == _lib.PP_ERR_INVALID_ARG
    assert call(mh=32768) == _lib.PP_ERR_UNSUPPORTED and call(mw=40000) == _lib.PP_ERR_UNSUPPORTED
    assert call(n=65536) == _lib.PP_ERR_UNSUPPORTED
    assert "32768" in _lib.last_error() or "below" in _lib.last_error()
    assert call(n=0, images=None) == _lib.PP_OK  # nothing to do
    assert "pp_warp_affine_u8_batch" in _lib.SIGNATURES
