"""What tools/test.py --show-dir costs. One JSON line per figure; the paths alternate inside every round of this one process,
medians over --rounds rounds (default 7) after one untimed round, the shader clock read right behind the timed work.

(a) figure "draw": 64 one-instance pictures with heatmaps (17 keypoints, 64 x 48 maps) at 640 x 480 and at 1920 x 1080:
    batch  visualization.draw_datasamples, one call (cut into chunks of 1 GiB of scratch)
    loop   the per-sample path, 64 times: structures.revert_heatmaps_max + PoseLocalVisualizer.draw_datasample on the reverted
           maps, kept on the device (merge_data_samples itself would also carry them through host memory: not timed)
    wall time around a device synchronise; launches (pp_launch_count) and host-to-device copies (counted in one extra round
    through a wrapper around Tensor.to / Tensor.copy_) per path.
(b) figure "dataset": runner.test_dataset on the set of scripts/bench_dataset_eval.py (300 images of 640 x 480, 8 threads,
    no metric), end to end: plain, with show_dir and output_heatmaps off (pose panel only), with show_dir and output_heatmaps on.

    python scripts/bench_show_dir.py [--rounds 7] [--figure draw] [--figure dataset] [--images 300] [--data DIR]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_cropcoco-coco-val-256x192.py")


class CopyCounter:
    """Counts host-to-device copies made through Tensor.to / Tensor.copy_ / Tensor.cuda while active."""

    def __enter__(self):
        import torch

        self.n, self._saved = 0, (torch.Tensor.to, torch.Tensor.copy_, torch.Tensor.cuda)
        to, copy_, cuda = self._saved
        counter = self

        def counted_to(t, *a, **k):
            r = to(t, *a, **k)
            counter.n += int(not t.is_cuda and r.is_cuda)
            return r

        def counted_copy(t, src, *a, **k):
            counter.n += int(t.is_cuda and isinstance(src, torch.Tensor) and not src.is_cuda)
            return copy_(t, src, *a, **k)

        def counted_cuda(t, *a, **k):
            counter.n += int(not t.is_cuda)
            return cuda(t, *a, **k)

        torch.Tensor.to, torch.Tensor.copy_, torch.Tensor.cuda = counted_to, counted_copy, counted_cuda
        return self

    def __exit__(self, *exc):
        import torch

        torch.Tensor.to, torch.Tensor.copy_, torch.Tensor.cuda = self._saved


def draw_figure(rounds, n_pictures=64):
    import torch

    from probpose_code_amd import _lib
    from probpose_code_amd import visualization as V
    from probpose_code_amd.structures import InstanceData, PixelData, PoseDataSample, _image_padding, revert_heatmaps_max
    from scripts.bench_jpeg_encode import shader_clock

    dev, K = torch.device("cuda:0"), 17
    vis = V.PoseLocalVisualizer(device=dev)
    for W, H in ((640, 480), (1920, 1080)):
        rng = np.random.default_rng(H)
        images, many, loop_in = [], [], []
        yy, xx = np.mgrid[0:64, 0:48].astype(np.float32)
        for i in range(n_pictures):
            images.append(torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev))
            w, h = rng.uniform(0.2, 0.6) * W, rng.uniform(0.3, 0.9) * H
            x, y = rng.uniform(-0.1 * w, W - 0.9 * w), rng.uniform(-0.1 * h, H - 0.9 * h)  # some boxes overhang: a padded canvas
            center = np.array([[x + w / 2, y + h / 2]], np.float32)
            scale = np.array([[max(w, h * 0.75), max(h, w / 0.75)]], np.float32) * 1.25
            sig = rng.uniform(0.8, 2.5, (K, 1, 1)).astype(np.float32)
            cy, cx = rng.uniform(8, 56, (K, 1, 1)).astype(np.float32), rng.uniform(6, 42, (K, 1, 1)).astype(np.float32)
            maps = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sig * sig)).astype(np.float32)
            maps_d = torch.from_numpy(maps / maps.sum(axis=(1, 2), keepdims=True))[None].to(dev)
            kp = np.stack([x + (cx.ravel() + 0.5) / 48 * w, y + (cy.ravel() + 0.5) / 64 * h], -1)[None]
            inst = dict(keypoints=kp, keypoints_visible=rng.uniform(0.2, 1, (1, K)).astype(np.float32),
                        keypoints_probs=rng.uniform(0.7, 1, (1, K)).astype(np.float32), bboxes=np.array([[x, y, x + w, y + h]], np.float32))
            meta = dict(ori_shape=(H, W), img_shape=(H, W), input_center=center, input_scale=scale)
            ds = PoseDataSample(metainfo=meta)
            ds.pred_instances = InstanceData(**inst)
            ds.pred_fields = PixelData(heatmaps=maps_d)
            many.append(ds)
            pad = _image_padding(center.astype(np.float64), scale.astype(np.float64), (H, W))
            loop_in.append((maps_d, center.astype(np.float64) + pad[:2], scale.astype(np.float64), (H + pad[1] + pad[3], W + pad[0] + pad[2]),
                            dict(meta, image_pad=pad), inst))

        def batch():
            return vis.draw_datasamples(images, many, draw_bbox=True, draw_heatmap=True)

        def loop():
            out = []
            for img, (maps_d, centers, scales, padded, meta, inst) in zip(images, loop_in):
                one = PoseDataSample(metainfo=meta)
                one.pred_instances = InstanceData(**inst)
                one.pred_fields = PixelData(heatmaps=revert_heatmaps_max(maps_d, centers, scales, padded, device=dev))
                out.append(vis.draw_datasample(img, one, draw_bbox=True, draw_heatmap=True))
            return out

        paths = dict(batch=batch, loop=loop)
        a, b = batch(), loop()
        equal = all(torch.equal(x, y) for x, y in zip(a, b))
        del a, b
        counts = {}
        for name, fn in paths.items():
            _lib.reset_launch_counts()
            with CopyCounter() as cc:
                fn()
            torch.cuda.synchronize()
            counts[name] = dict(launches=sum(_lib.launch_count(f) for f in ("pp_render_batch.hip", "pp_render.hip", "pp_warp.hip")),
                                host_to_device_copies=cc.n)
        ms = {name: [] for name in paths}
        for _ in range(rounds):
            for name, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        sclk = shader_clock()
        for name in paths:
            print(json.dumps(dict(figure="draw", size=f"{W}x{H}", pictures=n_pictures, path=name, wall_ms=round(statistics.median(ms[name]), 2),
                                  min_ms=round(min(ms[name]), 2), max_ms=round(max(ms[name]), 2), rounds=rounds, **counts[name],
                                  pictures_equal=equal, sclk_mhz=sclk)), flush=True)


def dataset_figure(rounds, images, data, batch_size=64, workers=8):
    import torch

    from probpose_code_amd import apis, runner, synthetic
    from probpose_code_amd.config import Config
    from probpose_code_amd.datasets import build_dataset
    from scripts.bench_jpeg_encode import shader_clock

    tmp = data or tempfile.mkdtemp(prefix="pp_bench_ds_")
    roots = [os.path.join(tmp, "cropcoco") + "/", os.path.join(tmp, "coco") + "/"]
    for i, r in enumerate(roots):
        if not os.path.exists(os.path.join(r, "annotations", "person_keypoints_val2017.json")):
            synthetic.synthetic_coco_dataset(r, images // 2, seed=100 + i, fmt="jpg", invalid_image=False, id_base=i + 1)
    cfg = Config.fromfile(CONFIG)
    cfg.merge_from_dict({f"test_dataloader.dataset.datasets.{i}.data_root": r for i, r in enumerate(roots)})
    model = apis.init_model(cfg, dict(state_dict=synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device="cuda:0")
    dataset = build_dataset(cfg.test_dataloader.dataset)
    n = len(dataset)
    show_dir = os.path.join(tmp, "show")

    def run(show, heatmaps):
        model.test_cfg["output_heatmaps"] = heatmaps
        shutil.rmtree(show_dir, ignore_errors=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.test_dataset(model, dataset, None, batch_size, workers, show_dir=show_dir if show else None)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    paths = dict(plain=(False, False), show_dir_pose_panel=(True, False), show_dir_with_heatmaps=(True, True))
    for args in paths.values():
        run(*args)  # warm-up: graph captures (with and without heatmaps), pinned buffers
    s = {name: [] for name in paths}
    for _ in range(rounds):
        for name, args in paths.items():
            s[name].append(run(*args))
    sclk = shader_clock()
    shutil.rmtree(show_dir, ignore_errors=True)
    for name in paths:
        med = statistics.median(s[name])
        print(json.dumps(dict(figure="dataset", path=name, instances=n, seconds=round(med, 4), min_s=round(min(s[name]), 4),
                              max_s=round(max(s[name]), 4), instances_per_s=round(n / med, 1), rounds=rounds, batch_size=batch_size,
                              workers=workers, sclk_mhz=sclk)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--figure", choices=["draw", "dataset"], action="append")
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--data", default=None, help="reuse / keep the generated set in this directory")
    args = ap.parse_args()
    for figure in args.figure or ["draw", "dataset"]:
        if figure == "draw":
            draw_figure(args.rounds)
        else:
            dataset_figure(args.rounds, args.images, args.data)


if __name__ == "__main__":
    main()
