"""Throughput of dataset evaluation (runner.test_dataset) on a seeded synthetic COCO-format set: a few hundred 640x480 JPEGs
written by PIL into a temp directory, 1-8 boxes per image, synthetic weights. One rate per run of its own:

    end_to_end      test_dataset without the metric (decode + crops + model)
    end_to_end_eval test_dataset with the two-metric evaluator of the CropCOCO / COCO config
    decode_only     the decode of every image on the same number of threads
    model_only      test_step_stream on pre-made crops, batches of --batch-size
    per_image_loop  apis.inference_topdown, one image (all its boxes) per call

    python scripts/bench_dataset_eval.py --images 300 --step end_to_end    (default: all steps, one JSON line each)

--decode device runs end_to_end* and decode_only through the split JPEG decoder (Huffman decoding on the threads, the rest
on the GPU: decode_only then ends with the pixels on the device, the host figure with the pixels in host memory);
--decode both prints the host line, the device line and the host line again (the spread of the host figure).
--decode-entropy device (with --decode device or both) lets the device decode the Huffman codes too: the threads only read
and prepare the files, the images of a batch go through one jpeg.decode_scans; --decode-entropy both prints the device
decoder's line with the host's Huffman decoding, with the device's, and the first again."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                      "td-pm_ProbPose-small_mi355x_cropcoco-coco-val-256x192.py")
STEPS = ("end_to_end", "end_to_end_eval", "decode_only", "model_only", "per_image_loop")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=300, help="images in all, half in each of the two datasets")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--step", choices=STEPS, action="append")
    ap.add_argument("--data", default=None, help="reuse / keep the generated set in this directory")
    ap.add_argument("--decode", default="host", choices=["host", "device", "both"], help="image decoder of the end_to_end* and decode_only steps")
    ap.add_argument("--decode-entropy", default="host", choices=["host", "device", "both"],
                    help="where the device decoder's Huffman codes are decoded (needs --decode device or both)")
    args = ap.parse_args()
    if args.decode_entropy != "host" and args.decode == "host":
        ap.error("--decode-entropy device needs --decode device")

    import torch

    from probpose_code_amd import apis, jpeg, runner, synthetic
    from probpose_code_amd.config import Config
    from probpose_code_amd.datasets import build_dataset

    tmp = args.data or tempfile.mkdtemp(prefix="pp_bench_ds_")
    roots = [os.path.join(tmp, "cropcoco") + "/", os.path.join(tmp, "coco") + "/"]
    for i, r in enumerate(roots):
        if not os.path.exists(os.path.join(r, "annotations", "person_keypoints_val2017.json")):
            synthetic.synthetic_coco_dataset(r, args.images // 2, seed=100 + i, fmt="jpg", invalid_image=False, id_base=i + 1)
    cfg = Config.fromfile(CONFIG)
    cfg.merge_from_dict({f"test_dataloader.dataset.datasets.{i}.data_root": r for i, r in enumerate(roots)})
    model = apis.init_model(cfg, dict(state_dict=synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device="cuda:0")
    dataset = build_dataset(cfg.test_dataloader.dataset)
    n = len(dataset)
    infos = [dataset.get_data_info(i) for i in range(n)]
    paths = list(dict.fromkeys(d["img_path"] for d in infos))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def decode_all_on_device(pool, entropy):
        if entropy == "device":  # the threads read and prepare, the images of a batch in one decode_scans
            futures = [pool.submit(jpeg.scan_prepare, p, True) for p in paths]
            for lo in range(0, len(futures), 16):
                jpeg.decode_scans([f.result() for f in futures[lo:lo + 16]], "cuda:0", staging)
            return
        futures = [pool.submit(jpeg.entropy_decode, p) for p in paths]
        for lo in range(0, len(futures), 16):  # the images of a batch in one reconstruct call
            jpeg.reconstruct_batch([f.result() for f in futures[lo:lo + 16]], "cuda:0", staging)

    from probpose_code_amd.transforms import BatchStaging

    staging = BatchStaging()
    decoded_steps = ("end_to_end", "end_to_end_eval", "decode_only")
    entropies = ("host", "device", "host") if args.decode_entropy == "both" else (args.decode_entropy,)
    runs = [(step, mode, entropy) for step in args.step or STEPS
            for mode in ((("host", "device", "host") if args.decode == "both" else (args.decode,)) if step in decoded_steps else ("host",))
            for entropy in (entropies if mode == "device" and step in decoded_steps else ("host",))]
    for step, mode, entropy in runs:
        if step in ("end_to_end", "end_to_end_eval"):
            kw = dict(decode=mode, decode_entropy=entropy)
            runner.test_dataset(model, dataset, None, args.batch_size, args.workers, **kw)  # warm-up: graph capture, pinned buffers
            ev = runner.build_evaluator(cfg.test_evaluator, dataset) if step == "end_to_end_eval" else None
            dt = timed(lambda: runner.test_dataset(model, dataset, ev, args.batch_size, args.workers, **kw))
        elif step == "decode_only":
            with ThreadPoolExecutor(max_workers=min(16, args.workers)) as pool:
                if mode == "device":
                    decode_all_on_device(pool, entropy)  # warm-up: pinned buffer, allocator
                    dt = timed(lambda: decode_all_on_device(pool, entropy))
                else:
                    dt = timed(lambda: list(pool.map(apis.load_image_bgr, paths)))
        elif step == "model_only":
            g = torch.Generator().manual_seed(0)
            crops = torch.randint(0, 256, (args.batch_size, 3, 256, 192), dtype=torch.uint8, generator=g).cuda()
            from probpose_code_amd.apis import pack_crops

            c = np.tile(np.array([[96.0, 128.0]], np.float32), (args.batch_size, 1))
            s = np.tile(np.array([[192.0, 256.0]], np.float32), (args.batch_size, 1))
            nb = (n + args.batch_size - 1) // args.batch_size

            def run():
                with torch.no_grad():
                    for _ in model.test_step_stream((pack_crops(crops, c, s, model.dataset_meta) for _ in range(nb)), depth=2,
                                                    max_batch=args.batch_size):
                        pass

            run()
            dt = timed(run)
        else:
            per_img = {}
            for d in infos:
                per_img.setdefault(d["img_path"], []).append(d["bbox"][0])

            def loop():
                for p, boxes in per_img.items():
                    apis.inference_topdown(model, apis.load_image_bgr(p), np.stack(boxes))

            loop()
            dt = timed(loop)
        print(json.dumps(dict(step=step, instances=n, images=len(paths), seconds=round(dt, 4), instances_per_s=round(n / dt, 1),
                              batch_size=args.batch_size, workers=args.workers, **(dict(decode=mode, decode_entropy=entropy) if step in decoded_steps else {}))), flush=True)


if __name__ == "__main__":
    main()
