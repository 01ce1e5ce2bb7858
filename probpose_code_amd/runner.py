"""The test loop of ``tools/test.py CONFIG CHECKPOINT`` (mmengine ``Runner.test()`` [3P] over the config's ``test_dataloader``
and ``test_evaluator``): the person instances of a dataset in batches, the model, one metric per dataset.

``test_dataset`` keeps every stage busy at once:
  * decode: the distinct images of the next batches are decoded on a thread pool (``apis.load_image_bgr``), at least two
    batches ahead; an image is dropped once its last instance has been batched. With ``decode="device"`` the threads run only
    the Huffman half (``jpeg.entropy_decode``) and the images of a batch are reconstructed on the device in ONE
    ``pp_jpeg_reconstruct_bgr_batch`` call on the producer stream, ahead of the warp that reads them in place. With
    ``decode_entropy="device"`` on top the threads only read the file and prepare its scan (``jpeg.scan_prepare``), and the
    images of a batch go through ONE ``jpeg.decode_scans``: Huffman decoding and reconstruction on the producer stream;
  * crops: the val pipeline through ``Compose.batched`` - box arithmetic on the host, ONE ``pp_warp_affine_u8_batch`` launch
    for the batch, its images uploaded with one copy - on a producer stream, under the model step of the batch before;
  * model: ``test_step_stream`` (full batches replay the captured graph, a partial last batch runs kernel by kernel);
  * metric: ``MultiDatasetEvaluator`` routes every sample to the metric of its ``dataset_name``;
  * pictures (``show_dir``, the reference's ``tools/test.py --show-dir``: PoseVisualizationHook.after_test_iter): every
    delivered batch is drawn by ONE ``draw_datasamples`` per scratch chunk - one picture per instance, the pose panel and,
    with ``test_cfg.output_heatmaps``, the probability-area panel from the heatmaps the engine left on the device - coded on
    the device (``jpeg.encode_batch`` / ``png.encode_batch``) and written on the thread pool.
"""
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .registry import DATASETS, EVALUATORS

MAX_WORKERS = 16  # a job's share of a GPU machine's CPUs; never sized from os.cpu_count()


class Batch(NamedTuple):
    """One batch of the plan: dataset ``indices`` (consecutive), the distinct ``images`` it reads (keys, in order of first
    use) and ``crop_image[i]`` = the position in ``images`` of instance ``indices[i]``."""

    indices: List[int]
    images: List[str]
    crop_image: List[int]


def plan_batches(image_keys: Sequence[str], batch_size: int) -> List[Batch]:
    """Instances in dataset order, ``batch_size`` per batch, the last one partial (DefaultSampler(shuffle=False,
    round_up=False), drop_last=False). ``image_keys[i]``: the source image of instance i."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    plan = []
    for lo in range(0, len(image_keys), batch_size):
        idx = list(range(lo, min(lo + batch_size, len(image_keys))))
        slot: Dict[str, int] = {}
        crop_image = [slot.setdefault(image_keys[i], len(slot)) for i in idx]
        plan.append(Batch(idx, list(slot), crop_image))
    return plan


def last_use(plan: Sequence[Batch]) -> Dict[str, int]:
    """image key -> the last batch that reads it (its decoded pixels are released after that batch is built)."""
    out: Dict[str, int] = {}
    for k, b in enumerate(plan):
        for key in b.images:
            out[key] = k
    return out


def sample_to_dict(ds) -> dict:
    """PoseDataSample -> the dict ``BaseDataElement.to_dict()`` gives the metric: metainfo keys, ``pred_instances`` and
    ``gt_instances`` as dicts of their fields; a one-element ``category_id`` array as an int."""
    if hasattr(ds, "to_dict"):
        d = ds.to_dict()
    else:
        d = dict(ds.metainfo)
        for name in ("pred_instances", "gt_instances"):
            if hasattr(ds, name):
                d[name] = dict(getattr(ds, name).all_items())
    if isinstance(d.get("category_id"), np.ndarray) and d["category_id"].size == 1:
        d["category_id"] = int(d["category_id"])  # the dataset keeps np.array(ann["category_id"]); the metric hashes it
    return d


def _coco_gt(ann_file: str) -> list:
    from .datasets import COCO

    coco = COCO(ann_file)
    return coco.loadAnns(coco.getAnnIds(imgIds=coco.getImgIds()))


def build_metric(cfg, ann_file: Optional[str] = None, device: str = "cuda"):
    """A ``CocoMetric`` config -> ``evaluation.CocoMetric``: ``ann_file`` loaded through the COCO index (its annotation list is
    the ground truth; when the config has none, the paired dataset's file, as the reference's CocoMetric takes it from the
    MessageHub, coco_metric.py:196-216), every other key passed on unchanged (``outfile_prefix`` / ``format_only`` among
    them). A ``format_only`` metric needs no annotation file (coco_metric.py:156-167)."""
    from .evaluation import CocoMetric

    if not isinstance(cfg, dict):
        return cfg  # a metric object already
    cfg = dict(cfg)
    kind = cfg.pop("type", "CocoMetric")
    if kind not in ("CocoMetric", "mmpose.CocoMetric"):
        raise NotImplementedError(f"metric type {kind!r}: only CocoMetric is implemented")
    for k in ("collect_device", "pred_converter", "gt_converter"):
        if cfg.get(k):
            raise NotImplementedError(f"CocoMetric({k}=...) is not supported")
        cfg.pop(k, None)
    path = cfg.pop("ann_file", None) or ann_file
    if path is None and not cfg.get("format_only"):
        raise ValueError("CocoMetric needs an ann_file (in its config or from its dataset)")
    cfg.setdefault("device", device)
    return CocoMetric(_coco_gt(path) if path is not None else None, **cfg)


@EVALUATORS.register_module(name="MultiDatasetEvaluator", force=True)
class MultiDatasetEvaluator:
    """mmpose/evaluation/evaluators/mutli_dataset_evaluator.py: metric i belongs to dataset config i and is keyed by that
    dataset class's ``dataset_name``; ``process`` routes every sample to the metric of its ``dataset_name``; ``evaluate``
    merges the metrics' (prefixed) results into one dict. ``ann_files``: dataset_name -> annotation file, for metrics
    whose config names none."""

    def __init__(self, metrics: Sequence, datasets: Sequence[dict], ann_files: Optional[Dict[str, str]] = None, device: str = "cuda"):
        assert len(metrics) == len(datasets), "the argument datasets should have same length as metrics"
        self.metrics_dict = {}
        for dcfg, mcfg in zip(datasets, metrics):
            cls = DATASETS.get(dcfg["type"]) if isinstance(dcfg["type"], str) else dcfg["type"]
            if cls is None:
                raise KeyError(f"{dcfg['type']} is not in the dataset registry")
            name = cls.DATASET_NAME
            self.metrics_dict[name] = build_metric(mcfg, (ann_files or {}).get(name), device)

    @property
    def metrics(self):
        return list(self.metrics_dict.values())

    def process(self, data_samples: Sequence, data_batch: Optional[dict] = None) -> None:
        routed: Dict[str, list] = {}
        for s in data_samples:
            s = s if isinstance(s, dict) else sample_to_dict(s)
            name = s.get("dataset_name")
            if name not in self.metrics_dict:
                raise KeyError(f"sample of dataset {name!r}: no metric for it (metrics: {list(self.metrics_dict)})")
            routed.setdefault(name, []).append(s)
        for name, metric in self.metrics_dict.items():
            if name in routed:
                metric.process(None, routed[name])

    def evaluate(self) -> dict:
        out = {}
        for metric in self.metrics_dict.values():
            res = metric.compute_metrics()
            dup = set(out) & set(res)
            if dup:
                raise ValueError(f"metrics of two datasets give the same key(s) {sorted(dup)}: set a distinct `prefix` per metric")
            out.update(res)
        return out


def build_evaluator(cfg, dataset=None, device: str = "cuda"):
    """``cfg.test_evaluator`` -> an evaluator; ``dataset`` (the built test dataset) supplies the annotation files of metrics
    that name none. A single metric config is a one-dataset evaluator."""
    subsets = getattr(dataset, "datasets", [dataset] if dataset is not None else [])
    ann_files = {type(d).DATASET_NAME: d.ann_file for d in subsets if hasattr(d, "ann_file")}
    cfg = dict(cfg)
    kind = cfg.pop("type", "MultiDatasetEvaluator")
    if kind in ("CocoMetric", "mmpose.CocoMetric"):
        if dataset is None or len(subsets) != 1:
            raise ValueError("a single CocoMetric evaluates a single dataset")
        return EVALUATORS.build(dict(type="MultiDatasetEvaluator", metrics=[dict(cfg, type=kind)],
                                     datasets=[dict(type=type(subsets[0]).__name__)]), ann_files=ann_files, device=device)
    return EVALUATORS.build(dict(cfg, type=kind), ann_files=ann_files, device=device)


def show_file_names(img_paths: Sequence[str], existing: Sequence[str]) -> List[str]:
    """The picture names of ``--show-dir`` for the samples of ``img_paths``, in order (visualization_hook.py:152-157):
    ``<stem>_<index>.<suffix>``, where stem and suffix are the image's base name cut at its last dot and index is the number of
    names in the directory that START WITH the stem - ``existing`` (the names there when the run began, and those given out
    earlier in the run) and the names given out before it in this call. As in the reference the stem ``a1`` therefore also
    counts the names of ``a12``. A pure function: the writes are asynchronous, the directory is not listed again."""
    names, out = list(existing), []
    for path in img_paths:
        base = os.path.basename(path)
        if "." not in base:
            raise ValueError(f"{path!r}: a picture name needs the suffix of its image")
        stem, suffix = base.rsplit(".", 1)
        name = f"{stem}_{sum(1 for f in names if f.startswith(stem))}.{suffix}"
        out.append(name)
        names.append(name)
    return out


def _write_bytes(path: str, data: bytes) -> None:
    with open(path, "wb") as f:
        f.write(data)


def _write_pillow(path: str, rgb: np.ndarray) -> None:
    from PIL import Image

    Image.fromarray(rgb).save(path)


def _show_sample(sample):
    """``merge_data_samples([sample])`` without the revert: the sample's instances, ``input_center`` / ``input_scale`` stacked
    and - with heatmaps in ``pred_fields`` - its un-reverted (1, K, h, w) maps, still on the device (``draw_datasamples``
    reverts them inside its launches)."""
    from .structures import PixelData, PoseDataSample

    meta = dict(sample.metainfo)
    meta["input_center"] = np.array([sample.input_center])
    meta["input_scale"] = np.array([sample.input_scale])
    merged = PoseDataSample(metainfo=meta)
    if "gt_instances" in sample:
        merged.gt_instances = sample.gt_instances
    if "pred_instances" in sample:
        merged.pred_instances = sample.pred_instances
    if "pred_fields" in sample and "heatmaps" in sample.pred_fields:
        merged.pred_fields = PixelData(heatmaps=torch.as_tensor(sample.pred_fields.heatmaps)[None])
    return merged


def _pipeline_of(model, dataset):
    from . import apis
    from .transforms import LoadImage, TopdownAffine

    pipe = getattr(dataset, "pipeline", None)
    if pipe is None or not pipe.transforms:
        return apis._val_pipeline(model)
    dev = str(next(model.parameters()).device)
    for t in pipe.transforms:
        if isinstance(t, (TopdownAffine, LoadImage)) and t.device is None:
            t.device = dev
    return pipe


LOSS_NOTE = ("loss/*: instance-weighted means of the batches' evaluation-mode loss dictionaries (no gradients). loss/loss_visibility is not "
             "exactly the whole-set value: its class-balancing weights are normalised per batch. A batch without annotated keypoints "
             "inside the image has no mae_oks / mae_err and is left out of their means.")


def _with_targets(pipeline, model):
    """``pipeline`` with ``GenerateTarget(encoder=<the head's ProbMap codec>, device=True)`` in front of ``PackPoseInputs`` - a new
    Compose, the dataset's own is left as it is."""
    from .transforms import Compose, GenerateTarget, PackPoseInputs

    codec = model.head.decoder
    gen = GenerateTarget(encoder=dict(type="ProbMap", input_size=tuple(codec.input_size), heatmap_size=tuple(codec.heatmap_size),
                                      sigma=codec.sigma), device=True)
    ts = list(pipeline.transforms)
    if any(isinstance(t, GenerateTarget) for t in ts):
        return pipeline
    at = next((i for i, t in enumerate(ts) if isinstance(t, PackPoseInputs)), len(ts))
    return Compose(ts[:at] + [gen] + ts[at:])


def test_dataset(model, dataset, evaluator=None, batch_size: int = 64, workers: int = 8, depth: int = 2,
                 sink: Optional[Callable[[list], None]] = None, decode: str = "host", decode_entropy: str = "host",
                 show_dir: Optional[str] = None, show_kpt_thr: float = 0.3, loss: bool = False) -> dict:
    """Run ``model`` over every instance of ``dataset`` (``get_data_info(i)``, i in order) and return the evaluator's metrics
    (``{}`` without one). ``sink``, when given, receives every batch's list of PoseDataSample, in order. ``decode``: "host"
    (``apis.load_image_bgr`` on the threads) or "device" (the split JPEG decoder of ``jpeg``: the same pixels; a file outside
    its subset is decoded on the host as before). ``decode_entropy`` (with ``decode="device"`` only): "host" (the threads decode
    the Huffman codes) or "device" (they only prepare the scan; the device decodes the codes as well, and an image it refuses
    steps down to the host as in ``jpeg.decode_scans``). The samples are the same whatever the choice.

    ``show_dir``: a directory (created when missing) that receives one picture per instance, named by ``show_file_names``: the
    sample drawn on its image with its box (``add_datasample(draw_gt=False, draw_bbox=True, draw_heatmap=True,
    kpt_thr=show_kpt_thr)`` of the reference's hook) - (H, W), or (2H, W) with the probability-area panel when
    ``model.test_cfg.output_heatmaps`` is on. An image's pixels are then kept until the batches that read it have been DRAWN.
    ``.jpg`` / ``.jpeg`` names are coded by ``jpeg.encode_batch(entropy="device", quality=75, subsampling="4:2:0")``, ``.png`` names
    by ``png.encode_batch``, any other suffix by Pillow from a host copy; the files are written on the loop's thread pool.
    The samples given to ``sink`` and the evaluator are the same with and without it.

    ``loss`` (off by default; ``ProbMapHead`` models on annotated keypoints): ``GenerateTarget(device=True)`` joins the pipeline and
    every batch is also scored by ``model.loss`` - the evaluation-mode loss, one extra unflipped pass in a workspace of its own, the
    batch's targets encoded by one ``pp_probmap_encode`` launch. The result then also holds ``loss/<key>`` for every key of the loss
    dictionary: the instance-weighted mean over the batches (``LOSS_NOTE`` says what that is not). The samples and the metrics are
    the same with and without it."""
    from . import jpeg
    from .apis import load_image_bgr
    from .transforms import BatchStaging, pseudo_collate

    if decode not in ("host", "device"):
        raise ValueError(f'decode must be "host" or "device", got {decode!r}')
    if decode_entropy not in jpeg.ENTROPY:
        raise ValueError(f"decode_entropy must be one of {jpeg.ENTROPY}, got {decode_entropy!r}")
    if decode_entropy == "device" and decode != "device":
        raise ValueError('decode_entropy="device" needs decode="device"')
    decode_fn = (jpeg.prepare_or_host if decode_entropy == "device" else jpeg.decode_or_host) if decode == "device" else load_image_bgr
    jpeg_staging = BatchStaging()

    n = len(dataset)
    infos = [dataset.get_data_info(i) for i in range(n)]
    plan = plan_batches([d["img_path"] for d in infos], batch_size)
    last = last_use(plan)
    pipeline = _pipeline_of(model, dataset)
    if loss:
        pipeline = _with_targets(pipeline, model)
    held: List[dict] = []  # loss: the collated batches whose samples have not come back yet, in order
    loss_sum: Dict[str, torch.Tensor] = {}  # key -> (2,) float64 on the device: sum of value * n, sum of n, over the batches with a finite value
    device = next(model.parameters()).device
    ahead = max(2, depth)
    pool = ThreadPoolExecutor(max_workers=max(1, min(MAX_WORKERS, int(workers))))
    decoded: Dict[str, object] = {}  # image key -> future of its pixels
    submitted = 0  # batches whose images have been queued for decoding

    def queue_until(k):
        nonlocal submitted
        while submitted < min(k, len(plan)):
            for key in plan[submitted].images:
                if key not in decoded:
                    decoded[key] = pool.submit(decode_fn, key)
            submitted += 1

    producer = torch.cuda.Stream(device=device)
    on_device: Dict[str, torch.Tensor] = {}  # decode="device": image key -> its reconstructed pixels, until its last batch
    fell_back = set()

    def reconstruct(keys):
        """The pixels of a batch's images; the coefficient sets among them that are not on the device yet in one call, the
        prepared scans in one call."""
        results = {key: decoded[key].result() for key in keys if key not in on_device}
        todo = [key for key, r in results.items() if isinstance(r, jpeg.JpegCoefficients)]
        scans = [key for key, r in results.items() if isinstance(r, jpeg.JpegScan)]
        host = set(results) - set(todo) - set(scans) - fell_back  # files outside the decoder's subset: counted once
        jpeg.fallbacks += len(host)
        fell_back.update(host)
        if scans:
            with torch.cuda.stream(producer):
                on_device.update(zip(scans, jpeg.decode_scans([results[key] for key in scans], device, jpeg_staging)))
        if todo:
            with torch.cuda.stream(producer):
                on_device.update(zip(todo, jpeg.reconstruct_batch([results[key] for key in todo], device, jpeg_staging)))
        return [on_device[key] if key in on_device else results[key] for key in keys]

    kept: Dict[str, object] = {}  # show_dir: image key -> its pixels (BGR), until the last batch that reads it has been drawn
    writes = []

    def show(k, samples):
        """Batch k, delivered: its pictures drawn by one draw_datasamples per chunk, coded per suffix in one call, written on the pool."""
        from . import png

        paths = [infos[i]["img_path"] for i in plan[k].indices]
        names = show_file_names(paths, taken)
        taken.extend(names)
        frames = visualizer.draw_datasamples([kept[p] for p in paths], [_show_sample(s) for s in samples], draw_bbox=True, draw_heatmap=True,
                                             kpt_thr=show_kpt_thr, channel_order="bgr", staging=show_staging)
        for key in plan[k].images:
            if last[key] == k:
                del kept[key]
        kinds = [("jpeg" if n.lower().endswith((".jpg", ".jpeg")) else "png" if n.lower().endswith(".png") else "other") for n in names]
        for kind in ("jpeg", "png"):
            sel = [i for i, v in enumerate(kinds) if v == kind]
            if not sel:
                continue
            pics = [frames[i] for i in sel]
            files = (jpeg.encode_batch(pics, quality=75, subsampling="4:2:0", channel_order="rgb", entropy="device", staging=show_staging)
                     if kind == "jpeg" else png.encode_batch(pics, channel_order="rgb", staging=show_staging))
            writes.extend(pool.submit(_write_bytes, os.path.join(show_dir, names[i]), data) for i, data in zip(sel, files))
        writes.extend(pool.submit(_write_pillow, os.path.join(show_dir, names[i]), frames[i].cpu().numpy()) for i, v in enumerate(kinds) if v == "other")

    def batches():
        for k, b in enumerate(plan):
            queue_until(k + 1 + ahead)
            pixels = reconstruct(b.images) if decode == "device" else [decoded[key].result() for key in b.images]
            if show_dir is not None:
                for key, px in zip(b.images, pixels):
                    kept[key] = px
                    if isinstance(px, torch.Tensor) and px.is_cuda:  # (reconstructed on the producer stream, drawn on the caller's)
                        px.record_stream(torch.cuda.current_stream(device))
            data_list = []
            for i, j in zip(b.indices, b.crop_image):
                d = dict(infos[i])
                d["img"] = pixels[j]  # the instances of an image share its array: one upload per batch, one table entry
                data_list.append(d)
            for key in b.images:
                if last[key] == k:
                    del decoded[key]
                    on_device.pop(key, None)
            with torch.cuda.stream(producer):
                packed = pipeline.batched(data_list)
            consumer = torch.cuda.current_stream(device)
            consumer.wait_stream(producer)
            for p in packed:
                if isinstance(p["inputs"], torch.Tensor) and p["inputs"].is_cuda:
                    p["inputs"].record_stream(consumer)
            if packed:
                data = pseudo_collate(packed)
                if loss:
                    held.append(data)
                yield data

    def score(samples):
        """The loss dictionary of the batch whose samples have just come back, added to the running sums on the device (no host wait)."""
        data = model.data_preprocessor(held.pop(0), False)
        assert len(data["data_samples"]) == len(samples)
        values = model.loss(data["inputs"], data["data_samples"], slot=depth)
        n = float(len(samples))
        for key, v in values.items():
            v = v.reshape(-1)[0].double()
            ok = torch.isfinite(v)
            term = torch.stack([torch.where(ok, v * n, torch.zeros_like(v)), ok.double() * n])
            loss_sum[key] = term if key not in loss_sum else loss_sum[key] + term

    if show_dir is not None:
        from .visualization import PoseLocalVisualizer

        os.makedirs(show_dir, exist_ok=True)
        taken = sorted(os.listdir(show_dir))  # the names that count towards an index: those on disk now, then those given out
        visualizer = PoseLocalVisualizer(device=device)
        visualizer.set_dataset_meta(getattr(model, "dataset_meta", None))
        show_staging = BatchStaging()
    try:
        with torch.no_grad():
            for k, samples in enumerate(model.test_step_stream(batches(), depth=depth, max_batch=batch_size)):
                if show_dir is not None:
                    show(k, samples)
                if sink is not None:
                    sink(samples)
                if evaluator is not None:
                    evaluator.process(samples)
                if loss:
                    score(samples)
        for w in writes:
            w.result()  # (a failed write is this call's failure)
    finally:
        pool.shutdown(wait=True, cancel_futures=True)
    metrics = evaluator.evaluate() if evaluator is not None else {}
    if loss and loss_sum:
        totals = torch.stack(list(loss_sum.values())).cpu().numpy()  # one copy
        for key, (s, c) in zip(loss_sum, totals):
            metrics["loss/" + key] = float(s / c) if c > 0 else float("nan")
    return metrics
