"""COCO-style datasets in top-down test mode with ground-truth boxes - what the ProbPose config's ``test_dataloader`` builds
(reference config td-pm_ProbPose-small_8xb64-210e_coco-256x192.py:113-199): ``CocoDataset``, ``CocoCropDataset`` and the
``CombinedDataset`` that concatenates them, registered in ``DATASETS`` under the reference's names.

The instance parsing follows mmpose/datasets/datasets/base/base_coco_style_dataset.py (cited per method) and the sample
access mmengine's ``BaseDataset`` [3P] (``get_data_info`` = a copy of the parsed instance + ``sample_idx``). ``COCO`` is the
slice of the ``xtcocotools.COCO`` index [3P] those methods call. Not built (``NotImplementedError``): detector boxes
(``bbox_file``), bottom-up mode, ``filter_cfg``, ``indices``, ``sample_interval != 1``. Detector boxes enter beside the
dataset instead: ``DetectionBoxes(dataset, bbox_file, bbox_score_thr)`` is a view of a built dataset whose samples are the
boxes of a detections file.
"""
import copy
import json
import os
import os.path as osp
from collections import defaultdict
from typing import Dict, List, Optional, Sequence

import numpy as np

from .apis import coco_dataset_meta
from .registry import DATASETS
from .visualization import COCO_SKELETON

# configs/_base_/datasets/coco.py: joint_weights (the sigmas are evaluation.COCO_SIGMAS, the flip indices synthetic.COCO_FLIP_INDICES)
COCO_JOINT_WEIGHTS = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.2, 1.2, 1.5, 1.5, 1.0, 1.0, 1.2, 1.2, 1.5, 1.5)
COCO_UPPER_BODY_IDS = tuple(range(11))      # keypoint_info type="upper": nose .. right_wrist
COCO_LOWER_BODY_IDS = tuple(range(11, 17))  # type="lower": hips, knees, ankles


def coco_pose_metainfo(dataset_name: str = "coco") -> dict:
    """The keys of ``parse_pose_metainfo(configs/_base_/datasets/coco.py)`` (mmpose/datasets/datasets/utils.py:115-190) that
    samples carry, derived from the tables the package already has. ``coco_crop.py`` differs only in ``dataset_name``."""
    from .evaluation import COCO_SIGMAS

    meta = coco_dataset_meta()
    flip = list(meta["flip_indices"])
    flip_pairs = []
    for k, s in enumerate(flip):  # utils.py:148-155: (swap, name) per keypoint with a partner, first occurrence kept
        if s != k and (s, k) not in flip_pairs:
            flip_pairs.append((s, k))
    meta.update(dataset_name=dataset_name, upper_body_ids=list(COCO_UPPER_BODY_IDS), lower_body_ids=list(COCO_LOWER_BODY_IDS),
                flip_indices=flip, flip_pairs=flip_pairs, skeleton_links=[tuple(l) for l in COCO_SKELETON],
                num_skeleton_links=len(COCO_SKELETON), dataset_keypoint_weights=np.array(COCO_JOINT_WEIGHTS, dtype=np.float32),
                sigmas=np.array(COCO_SIGMAS, dtype=np.float32))
    return meta


_METAINFO_FILES = {"coco.py": "coco", "coco_crop.py": "coco_crop"}


def _metainfo_from(metainfo: Optional[dict], default_name: str) -> dict:
    if metainfo is None:
        return coco_pose_metainfo(default_name)
    src = metainfo.get("from_file") if isinstance(metainfo, dict) else None
    name = _METAINFO_FILES.get(osp.basename(str(src))) if src else None
    if name is None or len(metainfo) != 1:
        raise NotImplementedError(f"metainfo={metainfo!r}: only dict(from_file='configs/_base_/datasets/coco.py' or 'coco_crop.py')")
    return coco_pose_metainfo(name)


class COCO:
    """The slice of ``xtcocotools.coco.COCO`` [3P] the datasets and the metric read: one annotation JSON, indexed once.
    Images in file order; the annotations of an image in file order."""

    def __init__(self, annotation_file: Optional[str] = None):
        self.dataset: dict = {}
        if annotation_file is not None:
            with open(annotation_file) as f:
                self.dataset = json.load(f)
        self.createIndex()

    def createIndex(self) -> None:
        self.anns, self.imgs, self.cats = {}, {}, {}
        self.imgToAnns: Dict[int, list] = defaultdict(list)
        for ann in self.dataset.get("annotations", []):
            self.imgToAnns[ann["image_id"]].append(ann)
            self.anns[ann["id"]] = ann
        for img in self.dataset.get("images", []):
            self.imgs[img["id"]] = img
        for cat in self.dataset.get("categories", []):
            self.cats[cat["id"]] = cat

    @staticmethod
    def _list(v):
        return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v]

    def getImgIds(self) -> List[int]:
        return list(self.imgs.keys())

    def getAnnIds(self, imgIds=()) -> List[int]:
        imgIds = self._list(imgIds)
        if not imgIds:
            return [a["id"] for a in self.dataset.get("annotations", [])]
        return [a["id"] for i in imgIds if i in self.imgToAnns for a in self.imgToAnns[i]]

    def loadAnns(self, ids=()) -> List[dict]:
        return [self.anns[i] for i in self._list(ids)]

    def loadImgs(self, ids=()) -> List[dict]:
        return [self.imgs[i] for i in self._list(ids)]

    def getCatIds(self) -> List[int]:
        return list(self.cats.keys())

    def loadCats(self, ids=()) -> List[dict]:
        return [self.cats[i] for i in self._list(ids)]

    def loadRes(self, res) -> "COCO":
        """Keypoint results -> an index over this set's images whose annotations are the results: the keypoint branch of
        ``xtcocotools.coco.COCO.loadRes`` [3P]. ``res``: a results file (``CocoMetric``'s ``{prefix}.keypoints.json``) or a
        list of result dicts. Every result gets ``id`` = its position + 1 and ``area`` / ``bbox`` from the extent of its
        keypoints (a ``bbox`` it carries is replaced); the categories are this set's. The caller's dicts are left as they
        are (xtcocotools writes into them). Refused: results on an image outside this set (AssertionError, as
        xtcocotools), an empty list (ValueError; xtcocotools fails with an IndexError), results without keypoints
        (NotImplementedError)."""
        if isinstance(res, (str, bytes, os.PathLike)):
            with open(res) as f:
                res = json.load(f)
        assert isinstance(res, list), "results in not an array of objects"
        if not res:
            raise ValueError("COCO.loadRes: no results (an empty result list)")
        img_ids = set(self.imgs)
        assert all(r["image_id"] in img_ids for r in res), "Results do not correspond to current coco set"
        anns = []
        for i, r in enumerate(res):
            if "keypoints" not in r:
                raise NotImplementedError(f"COCO.loadRes: result {i} has no keypoints (only keypoint results are supported)")
            kp = np.asarray(r["keypoints"], np.float64)
            x, y = kp[0::3], kp[1::3]
            x0, x1, y0, y1 = float(x.min()), float(x.max()), float(y.min()), float(y.max())
            anns.append(dict(r, id=i + 1, area=(x1 - x0) * (y1 - y0), bbox=[x0, y0, x1 - x0, y1 - y0]))
        out = COCO()
        out.dataset = dict(images=list(self.dataset.get("images", [])), categories=copy.deepcopy(self.dataset.get("categories", [])),
                           annotations=anns)
        out.createIndex()
        return out


class BaseCocoStyleDataset:
    """base_coco_style_dataset.py:21-364, top-down test mode on ground-truth boxes. Samples are the valid person instances
    of the annotation file, images in ``getImgIds()`` order; ``dataset[i]`` / ``get_data_info(i)`` is a fresh copy of
    sample i with ``sample_idx`` and the metainfo keys the pipeline reads."""

    DATASET_NAME = "coco"

    def __init__(self, ann_file: str = "", bbox_file: Optional[str] = None, data_mode: str = "topdown", metainfo: Optional[dict] = None,
                 data_root: Optional[str] = None, data_prefix: dict = dict(img=""), filter_cfg: Optional[dict] = None,
                 indices=None, serialize_data: bool = True, pipeline: Sequence = (), test_mode: bool = False,
                 lazy_init: bool = False, max_refetch: int = 1000, sample_interval: int = 1):
        if data_mode not in {"topdown", "bottomup"}:
            raise ValueError(f'{self.__class__.__name__} got invalid data_mode: {data_mode}. Should be "topdown" or "bottomup".')
        if data_mode != "topdown":
            raise NotImplementedError(f"{self.__class__.__name__}: data_mode='bottomup' is not supported (top-down only)")
        if bbox_file:
            raise NotImplementedError(f"{self.__class__.__name__}: bbox_file (evaluation on detector boxes) is not supported")
        if filter_cfg is not None:
            raise NotImplementedError(f"{self.__class__.__name__}: filter_cfg is not supported")
        if indices is not None:
            raise NotImplementedError(f"{self.__class__.__name__}: indices is not supported")
        if sample_interval != 1:
            raise NotImplementedError(f"{self.__class__.__name__}: sample_interval != 1 is not supported")
        self.data_mode, self.test_mode, self.data_root = data_mode, test_mode, data_root
        self._metainfo = _metainfo_from(metainfo, self.DATASET_NAME)
        # mmengine BaseDataset._join_prefix: relative paths are taken under data_root
        self.ann_file = osp.join(data_root, ann_file) if (ann_file and data_root and not osp.isabs(ann_file)) else ann_file
        self.data_prefix = {k: (osp.join(data_root, v) if (data_root and not osp.isabs(v)) else v) for k, v in dict(data_prefix).items()}
        from .transforms import Compose

        self.pipeline = Compose(list(pipeline))
        self.data_list: List[dict] = []
        self._fully_initialized = False
        if not lazy_init:
            self.full_init()

    @property
    def metainfo(self) -> dict:
        return copy.deepcopy(self._metainfo)

    def full_init(self) -> None:
        if self._fully_initialized:
            return
        instances, _ = self._load_annotations()
        self.data_list = [d for d in instances if self._is_valid_instance(d)]  # _get_topdown_data_infos (:366-372)
        self._fully_initialized = True

    def _load_annotations(self):
        """:223-260."""
        if not osp.isfile(self.ann_file):
            raise FileNotFoundError(f"Annotation file `{self.ann_file}`does not exist")
        self.coco = COCO(self.ann_file)
        if "categories" in self.coco.dataset:
            self._metainfo["CLASSES"] = self.coco.loadCats(self.coco.getCatIds())
        instance_list, image_list = [], []
        for img_id in self.coco.getImgIds():
            img = self.coco.loadImgs(img_id)[0]
            img.update({"img_id": img_id, "img_path": osp.join(self.data_prefix["img"], img["file_name"])})
            image_list.append(img)
            for ann in self.coco.loadAnns(self.coco.getAnnIds(imgIds=img_id)):
                info = self.parse_data_info(dict(raw_ann_info=ann, raw_img_info=img))
                if info:
                    instance_list.append(info)
        return instance_list, image_list

    def parse_data_info(self, raw_data_info: dict) -> Optional[dict]:
        """:262-343 (``pad_to_contain``, a training field, is not computed: the metric reads it from the annotation file)."""
        ann, img = raw_data_info["raw_ann_info"], raw_data_info["raw_img_info"]
        if "bbox" not in ann or "keypoints" not in ann:
            return None
        img_w, img_h = img["width"], img["height"]
        x, y, w, h = ann["bbox"]
        x1, y1 = np.clip(x, 0, img_w - 1), np.clip(y, 0, img_h - 1)
        x2, y2 = np.clip(x + w, 0, img_w - 1), np.clip(y + h, 0, img_h - 1)
        bbox = np.array([x1, y1, x2, y2], dtype=np.float32).reshape(1, 4)
        _keypoints = np.array(ann["keypoints"], dtype=np.float32).reshape(1, -1, 3)
        keypoints = _keypoints[..., :2]
        keypoints_visibility = (_keypoints[..., 2] == 2).astype(np.float32)
        keypoints_visible = np.minimum(1, _keypoints[..., 2])
        num_keypoints = ann["num_keypoints"] if "num_keypoints" in ann else np.count_nonzero(keypoints.max(axis=2))
        if "area" in ann:
            area = np.array(ann["area"], dtype=np.float32)
        else:
            area = np.array(np.clip((x2 - x1) * (y2 - y1) * 0.53, a_min=1.0, a_max=None), dtype=np.float32)
        data_info = {
            "img_id": ann["image_id"],
            "img_path": img["img_path"],
            "bbox": bbox,
            "bbox_score": np.ones(1, dtype=np.float32),
            "num_keypoints": num_keypoints,
            "keypoints": keypoints,
            "keypoints_visible": keypoints_visible,
            "keypoints_visibility": keypoints_visibility,
            "area": area,
            "iscrowd": ann.get("iscrowd", 0),
            "segmentation": ann.get("segmentation", None),
            "id": ann["id"],
            "category_id": np.array(ann["category_id"]),
            "raw_ann_info": copy.deepcopy(ann),
            "source_dataset": self._metainfo["dataset_name"],
        }
        if "crowdIndex" in img:
            data_info["crowd_index"] = img["crowdIndex"]
        return data_info

    @staticmethod
    def _is_valid_instance(data_info: Dict) -> bool:
        """:345-364."""
        if "iscrowd" in data_info and data_info["iscrowd"]:
            return False
        if "num_keypoints" in data_info and data_info["num_keypoints"] == 0:
            return False
        if "bbox" in data_info:
            bbox = data_info["bbox"][0]
            w, h = bbox[2:4] - bbox[:2]
            if w <= 0 or h <= 0:
                return False
        if "keypoints" in data_info:
            if np.max(data_info["keypoints"]) <= 0:
                return False
        return True

    METAINFO_KEYS = ("dataset_name", "upper_body_ids", "lower_body_ids", "flip_pairs", "dataset_keypoint_weights", "flip_indices",
                     "skeleton_links")

    def get_data_info(self, idx: int) -> dict:
        """mmengine BaseDataset.get_data_info (a copy + ``sample_idx``), then the metainfo keys (:176-205)."""
        self.full_init()
        data_info = copy.deepcopy(self.data_list[idx])
        data_info["sample_idx"] = idx if idx >= 0 else len(self) + idx
        for key in self.METAINFO_KEYS:
            assert key not in data_info, f'"{key}" is a reserved key for `metainfo`, but already exists in the `data_info`.'
            data_info[key] = copy.deepcopy(self._metainfo[key])
        return data_info

    def __len__(self) -> int:
        self.full_init()
        return len(self.data_list)

    def __getitem__(self, idx: int) -> Optional[dict]:
        return self.pipeline(self.get_data_info(idx))


@DATASETS.register_module(name="CocoDataset", force=True)
class CocoDataset(BaseCocoStyleDataset):
    """mmpose/datasets/datasets/body/coco_dataset.py: metainfo of configs/_base_/datasets/coco.py."""

    DATASET_NAME = "coco"


@DATASETS.register_module(name="CocoCropDataset", force=True)
class CocoCropDataset(BaseCocoStyleDataset):
    """mmpose/datasets/datasets/body/cococrop_dataset.py: metainfo of configs/_base_/datasets/coco_crop.py (= coco.py but for
    ``dataset_name``)."""

    DATASET_NAME = "coco_crop"


@DATASETS.register_module(name="CombinedDataset", force=True)
class CombinedDataset:
    """mmpose/datasets/dataset_wrappers.py:20-141 without resampling: the sub-datasets concatenated in order. A sample keeps
    its sub-dataset's fields (``dataset_name``, ``sample_idx`` within it); the combined metainfo overwrites five keys (:136)."""

    METAINFO_KEYS = ("upper_body_ids", "lower_body_ids", "flip_pairs", "dataset_keypoint_weights", "flip_indices")

    def __init__(self, metainfo: dict, datasets: list, pipeline: Sequence = (), sample_ratio_factor=None, test_mode: bool = False,
                 **kwargs):
        if sample_ratio_factor is not None:
            raise NotImplementedError("CombinedDataset: sample_ratio_factor (training-time resampling) is not supported")
        from .transforms import Compose

        self.datasets = [d if isinstance(d, BaseCocoStyleDataset) else DATASETS.build(d) for d in datasets]
        self._lens = [len(d) for d in self.datasets]
        self.pipeline = Compose(list(pipeline))
        self._metainfo = _metainfo_from(metainfo, "coco")
        self.test_mode = test_mode

    @property
    def metainfo(self) -> dict:
        return copy.deepcopy(self._metainfo)

    def __len__(self) -> int:
        return sum(self._lens)

    def _get_subset_index(self, index: int):
        """:54-88."""
        if index >= len(self) or index < -len(self):
            raise ValueError(f"index({index}) is out of bounds for dataset with length({len(self)}).")
        if index < 0:
            index = index + len(self)
        subset = 0
        while index >= self._lens[subset]:
            index -= self._lens[subset]
            subset += 1
        return subset, index

    def get_data_info(self, idx: int) -> dict:
        """:120-141 (the sub-datasets' pipelines are empty in the configs this serves: their sample is the data info)."""
        subset, local = self._get_subset_index(idx)
        data_info = self.datasets[subset][local]
        data_info.pop("dataset", None)
        for key in self.METAINFO_KEYS:
            data_info[key] = copy.deepcopy(self._metainfo[key])
        return data_info

    def __getitem__(self, idx: int) -> Optional[dict]:
        return self.pipeline(self.get_data_info(idx))


class DetectionBoxes:
    """The person boxes of a detector in place of a dataset's ground-truth boxes: a view of a built ``CocoDataset`` /
    ``CocoCropDataset`` whose samples are the reference's ``_load_detection_results`` (base_coco_style_dataset.py:430-486)
    over ``bbox_file`` followed by ``filter_data``'s ``bbox_score_thr`` rule (:488-514). It offers what the test loop and
    ``runner.build_evaluator`` read of a dataset (``len``, ``get_data_info``, ``[]``, ``pipeline``, ``metainfo``, ``ann_file``,
    the class's ``DATASET_NAME``). The dataset constructors themselves still refuse ``bbox_file`` / ``filter_cfg``.

    ``bbox_file``: a JSON list of ``{image_id, category_id, bbox: [x, y, w, h], score[, segmentation]}``. Entries in file
    order; ``category_id != 1`` skipped; ``bbox`` float32 xyxy, NOT clipped to the image; ``bbox_score`` float32 (1,);
    keypoints zero, ``keypoints_visible`` one; ``id`` counts the kept entries from 0. An instance with
    ``bbox_score < bbox_score_thr`` (strict, in the array's dtype) is dropped afterwards, so ids keep their gaps."""

    DATASET_NAME = "coco"
    _views: Dict[str, type] = {}

    def __new__(cls, dataset=None, *args, **kwargs):
        if cls is DetectionBoxes and isinstance(dataset, BaseCocoStyleDataset):  # the view class that carries the dataset's name
            cls = DetectionBoxes._views.get(type(dataset).DATASET_NAME, cls)
        return super().__new__(cls)

    def __init__(self, dataset, bbox_file: str, bbox_score_thr: Optional[float] = None):
        if isinstance(dataset, CombinedDataset):
            raise NotImplementedError("DetectionBoxes: a CombinedDataset is not supported (detector boxes are read for one "
                                      "CocoDataset / CocoCropDataset; wrap the sub-dataset that has a detections file)")
        if not isinstance(dataset, BaseCocoStyleDataset):
            raise TypeError(f"DetectionBoxes wraps a built CocoDataset / CocoCropDataset, got {type(dataset).__name__}")
        if type(dataset).DATASET_NAME != type(self).DATASET_NAME:
            raise TypeError(f"{type(self).__name__} views a {type(self).DATASET_NAME!r} dataset, got {type(dataset).DATASET_NAME!r}")
        dataset.full_init()
        self.dataset, self.bbox_file, self.bbox_score_thr = dataset, bbox_file, bbox_score_thr
        self.ann_file, self.pipeline, self.test_mode = dataset.ann_file, dataset.pipeline, dataset.test_mode
        self.data_list = self._load_detection_results()
        if bbox_score_thr is not None:  # filter_data (:511-512)
            self.data_list = [d for d in self.data_list if not d["bbox_score"] < bbox_score_thr]

    @property
    def metainfo(self) -> dict:
        return self.dataset.metainfo

    def _load_detection_results(self) -> List[dict]:
        if not osp.isfile(self.bbox_file):
            raise FileNotFoundError(f"Bbox file `{self.bbox_file}` does not exist")
        with open(self.bbox_file) as f:
            det_results = json.load(f)
        if not (isinstance(det_results, list) and all(isinstance(d, dict) for d in det_results)):
            raise TypeError(f"BBox file `{self.bbox_file}` should be a list of dict, but got {type(det_results)}")
        coco = self.dataset.coco
        num_keypoints = self.dataset._metainfo["num_keypoints"]
        data_list = []
        for n, det in enumerate(det_results):
            if det["category_id"] != 1:  # non-human instances
                continue
            if det["image_id"] not in coco.imgs:
                raise KeyError(f"BBox file `{self.bbox_file}`: entry {n} names image_id {det['image_id']!r}, which the annotation "
                               f"file `{self.ann_file}` does not have")
            img = coco.loadImgs(det["image_id"])[0]
            bbox = np.array(det["bbox"][:4], dtype=np.float32).reshape(1, 4)
            bbox[:, 2:] = bbox[:, 2:] + bbox[:, :2]  # bbox_xywh2xyxy, in float32
            data_list.append({
                "img_id": det["image_id"],
                "img_path": osp.join(self.dataset.data_prefix["img"], img["file_name"]),
                "img_shape": (img["height"], img["width"]),
                "bbox": bbox,
                "bbox_score": np.array(det["score"], dtype=np.float32).reshape(1),
                "keypoints": np.zeros((1, num_keypoints, 2), dtype=np.float32),
                "keypoints_visible": np.ones((1, num_keypoints), dtype=np.float32),
                "id": len(data_list),
                "segmentation": det.get("segmentation", None),
            })
        return data_list

    def get_data_info(self, idx: int) -> dict:
        """As the wrapped dataset's: a copy + ``sample_idx``, then the metainfo keys."""
        data_info = copy.deepcopy(self.data_list[idx])
        data_info["sample_idx"] = idx if idx >= 0 else len(self) + idx
        for key in self.dataset.METAINFO_KEYS:
            assert key not in data_info, f'"{key}" is a reserved key for `metainfo`, but already exists in the `data_info`.'
            data_info[key] = copy.deepcopy(self.dataset._metainfo[key])
        return data_info

    def __len__(self) -> int:
        return len(self.data_list)

    def __getitem__(self, idx: int) -> Optional[dict]:
        return self.pipeline(self.get_data_info(idx))


@DATASETS.register_module(name="CocoDetectionBoxes", force=True)
class CocoDetectionBoxes(DetectionBoxes):
    """``DetectionBoxes`` over a ``CocoDataset`` (what ``DetectionBoxes(dataset, ...)`` returns for one): the class carries the
    ``DATASET_NAME`` that pairs its samples with their metric."""

    DATASET_NAME = "coco"


@DATASETS.register_module(name="CocoCropDetectionBoxes", force=True)
class CocoCropDetectionBoxes(DetectionBoxes):
    """``DetectionBoxes`` over a ``CocoCropDataset``."""

    DATASET_NAME = "coco_crop"


DetectionBoxes._views.update(coco=CocoDetectionBoxes, coco_crop=CocoCropDetectionBoxes)


def build_dataset(cfg):
    """A dataset config (``cfg.test_dataloader.dataset``) -> the dataset object."""
    return DATASETS.build(dict(cfg))
