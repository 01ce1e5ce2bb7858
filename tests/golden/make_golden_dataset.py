"""Golden samples of the COCO-style datasets from the REFERENCE's own code (build container only): ``parse_data_info`` /
``_is_valid_instance`` / ``get_data_info`` of mmpose/datasets/datasets/base/base_coco_style_dataset.py, the metainfo of
coco_dataset.py / cococrop_dataset.py (parse_pose_metainfo of mmpose/datasets/datasets/utils.py over
configs/_base_/datasets/coco.py and coco_crop.py) and CombinedDataset.get_data_info (mmpose/datasets/dataset_wrappers.py).

mmengine and xtcocotools are absent here, so the reference modules are loaded behind stubs of what they import: a minimal
``BaseDataset`` (mmengine's ``_join_prefix`` / ``full_init`` / ``get_data_info`` + ``sample_idx``), an identity pipeline,
a dict-backed COCO index, ``Config.fromfile`` for the metainfo files. ``find_min_padding_exact`` (``pad_to_contain``, a
training field the test path does not produce) is stubbed to None.

Input: a small hand-made annotation file with the corner cases (crowd, num_keypoints 0 and missing, boxes partly outside the
image and of zero size, a missing area, v = 3 keypoints, crowdIndex, an image whose instances are all invalid).
Output: dataset_cases.json (the annotation file, the fields of every sample in order, scalar types) and dataset_cases.npz
(the array fields). Run: python tests/golden/make_golden_dataset.py"""
import contextlib
import copy
import importlib.util
import json
import os
import sys
import tempfile
import types
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PROBPOSE_REFERENCE", "/root/reference")


def _kp(rng, vis_pattern):
    out = []
    for v in vis_pattern:
        if v == 0:
            out += [0, 0, 0]
        else:
            out += [round(float(rng.uniform(20, 600)), 2), round(float(rng.uniform(20, 440)), 2), int(v)]
    return out


def annotation_file():
    rng = np.random.default_rng(7)
    images = [
        dict(id=11, file_name="000011.jpg", width=640, height=480),
        dict(id=3, file_name="000003.jpg", width=320, height=240, crowdIndex=0.35),
        dict(id=7, file_name="000007.jpg", width=500, height=375),  # every instance invalid
        dict(id=5, file_name="000005.jpg", width=64, height=48),
    ]
    full = [2] * 17
    anns = [
        dict(id=101, image_id=11, category_id=1, bbox=[10.5, 20.25, 100.0, 200.0], area=12345.5, iscrowd=0, num_keypoints=17,
             keypoints=_kp(rng, full)),
        dict(id=102, image_id=11, category_id=1, bbox=[-15.0, -8.0, 80.0, 120.0], area=900.0, iscrowd=0, num_keypoints=9,
             keypoints=_kp(rng, [2, 1, 0, 3, 3, 2, 2, 0, 1, 0, 0, 2, 2, 0, 0, 3, 0])),  # partly outside, v = 3
        dict(id=103, image_id=11, category_id=1, bbox=[600.0, 400.0, 100.0, 150.0], iscrowd=0, num_keypoints=4,
             keypoints=_kp(rng, [0] * 13 + [2, 2, 1, 1])),  # missing area, runs past the right / bottom edges
        dict(id=104, image_id=11, category_id=1, bbox=[100.0, 100.0, 50.0, 80.0], area=400.0, iscrowd=1, num_keypoints=5,
             keypoints=_kp(rng, [2] * 5 + [0] * 12)),  # crowd
        dict(id=105, image_id=11, category_id=1, bbox=[200.0, 50.0, 60.0, 90.0], area=700.0, iscrowd=0,
             keypoints=_kp(rng, [1] * 6 + [0] * 11)),  # num_keypoints missing
        dict(id=31, image_id=3, category_id=1, bbox=[5.0, 6.0, 100.0, 120.0], area=3000.0, iscrowd=0, num_keypoints=17,
             keypoints=_kp(rng, [3] * 8 + [2] * 9)),
        dict(id=32, image_id=3, category_id=1, bbox=[40.0, 30.0, 0.0, 50.0], area=10.0, iscrowd=0, num_keypoints=3,
             keypoints=_kp(rng, [2, 2, 2] + [0] * 14)),  # zero width
        dict(id=33, image_id=3, category_id=1, bbox=[330.0, 250.0, 40.0, 40.0], area=10.0, iscrowd=0, num_keypoints=3,
             keypoints=_kp(rng, [2, 2, 2] + [0] * 14)),  # wholly outside: clipped to zero size
        dict(id=71, image_id=7, category_id=1, bbox=[10.0, 10.0, 50.0, 50.0], area=50.0, iscrowd=0, num_keypoints=0,
             keypoints=[0] * 51),  # num_keypoints 0
        dict(id=72, image_id=7, category_id=1, bbox=[10.0, 10.0, 50.0, 50.0], area=50.0, iscrowd=1, num_keypoints=2,
             keypoints=_kp(rng, [2, 2] + [0] * 15)),  # crowd
        dict(id=73, image_id=7, category_id=1, bbox=[10.0, 10.0, 50.0, 50.0], area=50.0, iscrowd=0, keypoints=[0] * 51),  # no keypoints
        dict(id=51, image_id=5, category_id=1, bbox=[1.0, 2.0, 30.0, 40.0], iscrowd=0, num_keypoints=2,
             keypoints=[10.0, 12.0, 2, 20.5, 22.25, 1] + [0] * 45),  # missing area (clipped box)
        dict(id=74, image_id=7, category_id=1, keypoints=_kp(rng, full)),  # no bbox: parse_data_info drops it
    ]
    cats = [dict(id=1, name="person", supercategory="person", keypoints=[], skeleton=[])]
    return dict(images=images, annotations=anns, categories=cats)


# --------------------------------------------------------------------------------------------------------------- stubs
def _shell(name, path=None):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    sys.modules[name] = m
    return m


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class _Registry(dict):
    def register_module(self, name=None, force=False, module=None):
        def deco(cls):
            self[name or cls.__name__] = cls
            return cls

        return deco if module is None else deco(module)

    @property
    def module_dict(self):
        return self


class _COCO:
    def __init__(self, path):
        self.dataset = json.load(open(path))
        self.imgs = {i["id"]: i for i in self.dataset["images"]}
        self.anns = {a["id"]: a for a in self.dataset["annotations"]}
        self.cats = {c["id"]: c for c in self.dataset["categories"]}
        self.img_to_anns = defaultdict(list)
        for a in self.dataset["annotations"]:
            self.img_to_anns[a["image_id"]].append(a)

    def getImgIds(self):
        return list(self.imgs)

    def getAnnIds(self, imgIds):
        return [a["id"] for a in self.img_to_anns.get(imgIds, [])]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]

    def loadImgs(self, i):
        return [self.imgs[i]]

    def getCatIds(self):
        return list(self.cats)

    def loadCats(self, ids):
        return [self.cats[i] for i in ids]


class _BaseDataset:
    """mmengine.dataset.BaseDataset, the part a test-mode COCO dataset runs through."""

    METAINFO: dict = dict()

    def __init__(self, ann_file="", metainfo=None, data_root="", data_prefix=dict(img=""), filter_cfg=None, indices=None,
                 serialize_data=True, pipeline=(), test_mode=False, lazy_init=False, max_refetch=1000):
        self.ann_file, self.data_root, self.data_prefix = ann_file, data_root, copy.copy(data_prefix)
        self.test_mode, self._fully_initialized = test_mode, False
        self._metainfo = self._load_metainfo(copy.deepcopy(metainfo))
        self.pipeline = lambda d: d
        if self.data_root:  # _join_prefix
            if self.ann_file and not os.path.isabs(self.ann_file):
                self.ann_file = os.path.join(self.data_root, self.ann_file)
            for k, p in self.data_prefix.items():
                if not os.path.isabs(p):
                    self.data_prefix[k] = os.path.join(self.data_root, p)
        if not lazy_init:
            self.full_init()

    @classmethod
    def _load_metainfo(cls, metainfo=None):
        return copy.deepcopy(metainfo or {})

    @property
    def metainfo(self):
        return copy.deepcopy(self._metainfo)

    def full_init(self):
        if self._fully_initialized:
            return
        self.data_list = self.load_data_list()
        self._fully_initialized = True

    def get_data_info(self, idx):
        data_info = copy.deepcopy(self.data_list[idx])
        data_info["sample_idx"] = idx if idx >= 0 else len(self) + idx
        return data_info

    def __len__(self):
        return len(self.data_list)

    def __getitem__(self, idx):
        return self.prepare_data(idx)


def load_reference():
    for name, sub in (("mmpose", "mmpose"), ("mmpose.datasets", "mmpose/datasets"), ("mmpose.datasets.datasets", "mmpose/datasets/datasets"),
                      ("mmpose.datasets.datasets.base", "mmpose/datasets/datasets/base"),
                      ("mmpose.datasets.datasets.body", "mmpose/datasets/datasets/body")):
        _shell(name, os.path.join(REF, sub))
    mmengine = _shell("mmengine")
    ds = _shell("mmengine.dataset")
    ds.BaseDataset, ds.force_full_init = _BaseDataset, (lambda f: f)
    fio = _shell("mmengine.fileio")
    fio.exists, fio.load = os.path.exists, (lambda p: json.load(open(p)))
    fio.get_local_path = contextlib.contextmanager(lambda p: (yield p))
    lg = _shell("mmengine.logging")

    class _Hub:
        @staticmethod
        def get_current_instance():
            return types.SimpleNamespace(update_info_dict=lambda d: None)

    lg.MessageHub = _Hub
    ut = _shell("mmengine.utils")
    ut.is_list_of = lambda seq, t: isinstance(seq, list) and all(isinstance(x, t) for x in seq)

    class _Config:
        @staticmethod
        def fromfile(path):
            ns = {}
            exec(compile(open(path).read(), path, "exec"), ns)  # noqa: S102
            return types.SimpleNamespace(dataset_info=ns["dataset_info"])

    mmengine.Config = _Config
    rg = _shell("mmengine.registry")
    rg.build_from_cfg = lambda cfg, reg: reg[cfg["type"]](**{k: v for k, v in cfg.items() if k != "type"})
    xt = _shell("xtcocotools")
    xc = _shell("xtcocotools.coco")
    xc.COCO = _COCO
    xt.coco = xc
    reg = _shell("mmpose.registry")
    reg.DATASETS = _Registry()
    st = _shell("mmpose.structures")
    sb = _shell("mmpose.structures.bbox")
    sb.bbox_xywh2xyxy = None  # imported, not called on this path
    sk = _shell("mmpose.structures.keypoint")
    sk.find_min_padding_exact = lambda bbox, kpts: None
    st.bbox, st.keypoint = sb, sk
    _load("mmpose.datasets.datasets.utils", "mmpose/datasets/datasets/utils.py")
    base = _load("mmpose.datasets.datasets.base.base_coco_style_dataset", "mmpose/datasets/datasets/base/base_coco_style_dataset.py")
    sys.modules["mmpose.datasets.datasets.base"].BaseCocoStyleDataset = base.BaseCocoStyleDataset
    _load("mmpose.datasets.datasets.body.coco_dataset", "mmpose/datasets/datasets/body/coco_dataset.py")
    _load("mmpose.datasets.datasets.body.cococrop_dataset", "mmpose/datasets/datasets/body/cococrop_dataset.py")
    _load("mmpose.datasets.dataset_wrappers", "mmpose/datasets/dataset_wrappers.py")
    return reg.DATASETS


SKIP = ("pad_to_contain",)  # training field, stubbed above; not produced by the test path


def record(sample, tag, arrays):
    """field name -> JSON description; arrays go to ``arrays`` under ``tag/field``."""
    out = []
    for k, v in sample.items():
        if k in SKIP:
            continue
        if isinstance(v, np.ndarray):
            arrays[f"{tag}/{k}"] = v
            out.append([k, "ndarray", None])
        elif isinstance(v, np.generic):
            out.append([k, type(v).__name__, v.item()])
        else:
            out.append([k, type(v).__name__, v])
    return out


def main():
    reg = load_reference()
    ann = annotation_file()
    arrays, cases = {}, {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "person_keypoints.json")
        json.dump(ann, open(path, "w"))
        os.chdir(REF)  # the metainfo files are named relative to the reference tree
        try:
            kw = dict(ann_file=path, data_root="data/root/", data_prefix=dict(img="val2017/"), test_mode=True, pipeline=[])
            for name in ("CocoDataset", "CocoCropDataset"):
                d = reg[name](**kw)
                cases[name] = [record(d.get_data_info(i), f"{name}/{i}", arrays) for i in range(len(d))]
            comb = reg["CombinedDataset"](metainfo=dict(from_file="configs/_base_/datasets/coco.py"),
                                          datasets=[dict(type="CocoCropDataset", **kw), dict(type="CocoDataset", **kw)], pipeline=[],
                                          test_mode=True)
            cases["CombinedDataset"] = [record(comb.get_data_info(i), f"CombinedDataset/{i}", arrays) for i in range(len(comb))]
        finally:
            os.chdir(cwd)
    doc = dict(annotations=ann, data_root="data/root/", data_prefix="val2017/", cases=cases)
    with open(os.path.join(HERE, "dataset_cases.json"), "w") as f:
        json.dump(doc, f, indent=0, sort_keys=False)
    np.savez_compressed(os.path.join(HERE, "dataset_cases.npz"), **arrays)
    print({k: len(v) for k, v in cases.items()}, len(arrays), "arrays")


if __name__ == "__main__":
    main()
