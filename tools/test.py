"""Counterpart of the reference's ``tools/test.py CONFIG CHECKPOINT``: evaluate a config's test set end to end - the
``test_dataloader`` (COCO-style datasets on ground-truth boxes) through the model, the ``test_evaluator`` over the results
(probpose_code_amd.runner.test_dataset) - and print the metrics.

    python tools/test.py configs/td-pm_ProbPose-small_mi355x_cropcoco-coco-val-256x192.py CHECKPOINT \
        --cfg-options test_dataloader.dataset.datasets.0.data_root=/data/CropCOCO/ \
                      test_dataloader.dataset.datasets.1.data_root=/data/coco/ --out metrics.json

CHECKPOINT may be "synthetic" (seeded random weights: a plumbing check, as in demo/image_demo.py).

On the boxes of a person detector instead (the COCO top-down protocol: every box scored detector score x mean keypoint score,
duplicates removed by OKS-NMS per image), for a single-dataset config:

    python tools/test.py configs/td-hm_ViTPose-base_mi355x_coco-256x192.py CHECKPOINT \
        --cfg-options test_dataloader.dataset.data_root=/data/coco/ \
        --bbox-file /data/coco/person_detection_results/COCO_val2017_detections_AP_H_56_person.json --nms device

``--loss`` adds the head's evaluation-mode loss dictionary (``model.eval(); model(..., mode="loss")`` of the reference: forward
values, no gradients) as ``loss/<key>`` lines beside the metrics.

``--show-dir DIR`` dumps one picture per evaluated instance (the reference's PoseVisualizationHook); add
``--cfg-options model.test_cfg.output_heatmaps=True`` for the probability-area panel under the pose."""
import ast
import json
import os
import sys
import time
from argparse import ArgumentParser

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_cfg_options(items):
    """``key=value`` pairs (mmengine's DictAction): values read as Python literals where they parse as one (numbers, booleans,
    lists, tuples, None), as strings otherwise."""
    opts = {}
    for it in items or []:
        if "=" not in it:
            raise ValueError(f"--cfg-options takes key=value pairs, got {it!r}")
        k, v = it.split("=", 1)
        try:
            opts[k] = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            opts[k] = {"true": True, "false": False, "none": None}.get(v.lower(), v)
    return opts


def build_parser():
    ap = ArgumentParser(description="Evaluate a config's test set (COCO-style datasets, ground-truth boxes)")
    ap.add_argument("config")
    ap.add_argument("checkpoint", help='a checkpoint file, or "synthetic" for seeded random weights')
    ap.add_argument("--cfg-options", nargs="+", default=None, metavar="KEY=VALUE",
                    help="override config keys; integer parts index lists, e.g. test_dataloader.dataset.datasets.0.data_root=DIR")
    ap.add_argument("--out", default=None, help="write the metrics as JSON to this file")
    ap.add_argument("--batch-size", type=int, default=None, help="instances per step (default: test_dataloader.batch_size, else 64)")
    ap.add_argument("--workers", type=int, default=8, help="image decoding threads (at most 16)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--decode", default="host", choices=["host", "device"],
                    help="device: JPEG files are Huffman-decoded on the threads and reconstructed on the GPU (the same pixels)")
    ap.add_argument("--decode-entropy", default="host", choices=["host", "device"],
                    help="device (needs --decode device): the files' Huffman codes are decoded on the GPU as well (the same pixels)")
    ap.add_argument("--precision", default=None, choices=[None, "f16x3", "bf16", "f32"],
                    help="overrides model.precision of the config (default there: f16x3)")
    ap.add_argument("--bbox-file", default=None, metavar="FILE",
                    help="evaluate on the person boxes of this detections file (a JSON list of image_id / category_id / bbox xywh / "
                         "score) instead of the ground-truth boxes; single-dataset configs")
    ap.add_argument("--bbox-score-thr", type=float, default=None, metavar="T",
                    help="with --bbox-file: drop boxes whose score is below T before the model sees them")
    ap.add_argument("--nms", default="host", choices=["host", "device"],
                    help="where the metric's OKS-NMS runs (CocoMetric nms_backend); device: all images in two launches, the same kept sets")
    ap.add_argument("--show-dir", default=None, metavar="DIR",
                    help="write one picture per evaluated instance into DIR, named <image stem>_<index>.<suffix>: the pose on the image and, with "
                         "model.test_cfg.output_heatmaps=True, the probability areas under it; drawn and coded (.jpg, .png) on the GPU")
    ap.add_argument("--loss", action="store_true",
                    help="also report the evaluation-mode loss dictionary of the head (ProbMapHead.loss: no gradients, not a training step) as "
                         "loss/<key>, the instance-weighted mean over the batches; targets are encoded on the GPU, one launch per batch")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.loss and args.bbox_file:
        ap.error("--loss needs the ground-truth keypoints of the annotation file: not with --bbox-file")
    if args.bbox_score_thr is not None and not args.bbox_file:
        ap.error("--bbox-score-thr needs --bbox-file")
    if args.decode_entropy == "device" and args.decode != "device":
        ap.error("--decode-entropy device needs --decode device")

    from probpose_code_amd import apis, runner, synthetic
    from probpose_code_amd.config import Config
    from probpose_code_amd.datasets import DetectionBoxes, build_dataset

    cfg = Config.fromfile(args.config)
    opts = parse_cfg_options(args.cfg_options)
    if args.precision:
        opts["model.precision"] = args.precision
    if opts:
        cfg.merge_from_dict(opts)
    ckpt = args.checkpoint
    if ckpt == "synthetic":  # (the backbone's arch and the head kind - ProbMapHead with its towers, or ViTPose's HeatmapHead - from the config)
        ckpt = dict(state_dict=synthetic.synthetic_state_dict(synthetic.arch_of(cfg), seed=0, logit_scale=2.0, head=synthetic.head_kind_of(cfg)))
    model = apis.init_model(cfg, ckpt, device=args.device)
    loader = cfg["test_dataloader"]
    dataset = build_dataset(loader["dataset"])
    if args.bbox_file:
        dataset = DetectionBoxes(dataset, args.bbox_file, args.bbox_score_thr)
    ev_cfg = dict(cfg["test_evaluator"])
    if args.nms != "host":  # (a metric config's own nms_backend stands when the flag is left at its default)
        if "metrics" in ev_cfg:
            ev_cfg["metrics"] = [dict(m, nms_backend=args.nms) if isinstance(m, dict) else m for m in ev_cfg["metrics"]]
        else:
            ev_cfg["nms_backend"] = args.nms
    evaluator = runner.build_evaluator(ev_cfg, dataset, device=args.device)
    batch_size = args.batch_size or int(loader.get("batch_size", 64))
    t0 = time.perf_counter()
    metrics = runner.test_dataset(model, dataset, evaluator, batch_size=batch_size, workers=args.workers, decode=args.decode,
                                  decode_entropy=args.decode_entropy, show_dir=args.show_dir, loss=args.loss)
    dt = time.perf_counter() - t0
    for k, v in metrics.items():
        print(f"{k}: {v:.4f}")
    if args.loss:
        print(runner.LOSS_NOTE)
    print(f"{len(dataset)} instances in {dt:.2f} s ({len(dataset) / dt:.1f} instances/s)", file=sys.stderr)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(metrics, f, indent=1)
    return metrics


if __name__ == "__main__":
    main()
