"""The --draw-heatmap picture of a 1920 x 1080 frame with 4 persons and 17 keypoints (csrc/pp_render.hip): GPU time of the four
stages from device events after warm-up, the numpy restatement of tests/render_ref.py on the host (thresholds on a pool of
16 threads, one map per task), bytes moved and the resulting share of HBM bandwidth. Prints one JSON line.

    python scripts/bench_render.py [--steps 50] [--warmup 5] [--skip-host]
    rocprofv3 --kernel-trace --stats -d OUT -o render -- python scripts/bench_render.py --steps 20 --skip-host
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_PEAK = 8.0e12  # MI355X HBM3E, spec (6.29e12 measured with a float4 copy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true", help="no numpy timing (profiling runs)")
    args = ap.parse_args()

    import render_ref as R
    from probpose_code_amd import visualization as V

    assert torch.cuda.is_available(), "bench_render.py measures the MI355X"
    H, W, K, n = 1080, 1920, 17, 4
    pad = (90, 61, 37, 75)
    Hp, Wp = H + pad[1] + pad[3], W + pad[0] + pad[2]
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    maps = R.posterior_like_maps(K, Hp, Wp, seed=1)
    kp = np.stack([rng.uniform(0, W, (n, K)), rng.uniform(0, H, (n, K))], -1).astype(np.float32)
    vis = rng.uniform(0.2, 1, (n, K)).astype(np.float32)
    boxes = np.concatenate([kp.min(1), kp.max(1)], 1).astype(np.float32)

    dev = torch.device("cuda:0")
    img_d = torch.from_numpy(img).to(dev)
    maps_d = torch.from_numpy(maps).to(dev)
    out = torch.empty((2 * H, W, 3), dtype=torch.uint8, device=dev)
    canvas = torch.empty((Hp, Wp, 3), dtype=torch.uint8, device=dev)

    def stages():
        V.draw_poses(img_d, kp, vis, boxes, out=out[:H])
        V.render_probability_areas(maps_d, img_d, pad, boxes, out=canvas)
        V.resize_rgb(canvas, (H, W), out=out[H:])

    for _ in range(args.warmup):
        stages()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(args.steps):
        stages()
    ev[1].record()
    torch.cuda.synchronize()
    gpu_us = ev[0].elapsed_time(ev[1]) * 1e3 / args.steps

    # thresholds alone (the three select passes)
    ev[0].record()
    for _ in range(args.steps):
        V.probability_area_thresholds(maps_d)
    ev[1].record()
    torch.cuda.synchronize()
    thr_us = ev[0].elapsed_time(ev[1]) * 1e3 / args.steps

    got = out.cpu().numpy()
    P = K * Hp * Wp * 4
    bytes_moved = {
        "thresholds (3 passes over the maps)": 3 * P,
        "compose (maps, image, canvas)": P + H * W * 3 + Hp * Wp * 3,
        "poses (image in, panel out)": 2 * H * W * 3,
        "resize (canvas in, panel out)": Hp * Wp * 3 + H * W * 3,
    }
    total_bytes = sum(bytes_moved.values())
    res = dict(workload=f"{W}x{H} frame, {n} persons, {K} keypoints, canvas {Wp}x{Hp}", gpu_us=round(gpu_us, 1),
               gpu_thresholds_us=round(thr_us, 1), bytes=total_bytes, bytes_by_stage=bytes_moved,
               achieved_tb_s=round(total_bytes / (gpu_us * 1e-6) / 1e12, 3),
               hbm_share_of_spec_peak=round(total_bytes / (gpu_us * 1e-6) / HBM_PEAK, 3), target_us=1000.0,
               device=torch.cuda.get_device_name(0))
    if not args.skip_host:
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as pool:
            tds = list(pool.map(R.threshold_fp64, maps))
        thr = np.array([t for t, _ in tds], np.float32)
        draw = np.array([d for _, d in tds], np.int32)
        t1 = time.perf_counter()
        top = R.draw_poses(img, kp, vis, R.int_boxes(boxes), V.COCO_SKELETON, V.COCO_LINK_COLORS, V.COCO_KEYPOINT_COLORS, 0.3, 3, 1, 0.8)
        panel = R.resize(R.compose(img, pad, maps, thr, draw, R.aspect_boxes(boxes, pad)), H, W)
        t2 = time.perf_counter()
        want = np.concatenate([top, panel])
        res.update(host_numpy_s=round(t2 - t0, 3), host_thresholds_s=round(t1 - t0, 3), host_threads=16,
                   speedup=round((t2 - t0) / (gpu_us * 1e-6), 1), byte_equal_to_restatement=bool(np.array_equal(got, want)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
