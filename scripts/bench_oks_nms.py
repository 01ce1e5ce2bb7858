"""dev only: OKS-NMS of a detector-box evaluation at COCO-val2017 scale, host loop (evaluation.oks_nms) against the device batch
(pp_oks_nms_batch), in one process, alternating, medians of 7. The input is a seeded synthetic set shaped like a person
detector's file: 5000 images, instance counts drawn to average about twenty with a tail to a hundred, clusters of
near-duplicate poses so that suppression happens. One JSON line per figure:
  * the shader clock, idle and under the timed launches (pp_clock_probe);
  * pp_oks_nms_batch alone, device events around the call: its two launches behind the table upload they wait for;
  * CocoMetric._instances() wall time for both backends (grouping, scoring and suppression; the device figure includes the
    uploads, the copy back and the host runs of undecided images), and whether the kept sets agree.
    python scripts/bench_oks_nms.py [--images 5000] [--rounds 7]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from probpose_code_amd import _lib
from probpose_code_amd.evaluation import COCO_SIGMAS, OKS_NMS_GUARD, CocoMetric

K = 17
dev = torch.device("cuda:0")


def synthetic_results(n_images, seed=0):
    """``CocoMetric.results`` entries of one detector-box run: per image a few persons, every person found several times
    (jitter of a few pixels: near-duplicates), plus stray boxes."""
    rng = np.random.default_rng(seed)
    res, nid = [], 0
    for img in range(n_images):
        n = int(min(100, rng.gamma(2.0, 10.0)))
        persons = rng.uniform(30, 600, (max(1, n // 4), K, 2))
        sizes = rng.uniform(40, 300, len(persons))
        for _ in range(n):
            p = int(rng.integers(0, len(persons)))
            kp = persons[p] + rng.normal(0, rng.choice([0.5, 2.0, 8.0, 40.0]), (K, 2))
            res.append(dict(id=nid, img_id=img, category_id=1, keypoints=kp[None], keypoint_scores=rng.uniform(0.05, 1, (1, K)).astype(np.float32),
                            keypoints_visible=np.ones((1, K), np.float32), keypoint_probs=rng.uniform(0, 1, (1, K)).astype(np.float32),
                            bbox_scores=np.round(rng.uniform(0.05, 1, 1), 3).astype(np.float32),
                            areas=np.array([sizes[p] * sizes[p] * 0.75 * rng.uniform(0.9, 1.1)], np.float32)))
            nid += 1
    return res


def clock_ghz(busy=None, window_us=200_000):
    """Average shader clock over `window_us` (pp_clock_probe: one sleeping wavefront on a side stream) while `busy()` runs over and over."""
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    _lib.call("pp_clock_probe", out.data_ptr(), None, int(window_us), side.cuda_stream)
    t_end = time.perf_counter() + window_us * 1e-6
    while busy is not None and time.perf_counter() < t_end:
        busy()
    torch.cuda.synchronize()
    cyc, ticks = (int(v) for v in out.tolist())
    return cyc / max(1, ticks) * 0.1


def say(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--thr", type=float, default=0.9)
    args = ap.parse_args()
    res = synthetic_results(args.images)
    counts = np.bincount([r["img_id"] for r in res], minlength=args.images)
    say(figure="input", device=torch.cuda.get_device_name(0), images=args.images, instances=len(res), mean_per_image=float(counts.mean()),
        max_per_image=int(counts.max()), nms_thr=args.thr)

    metrics = {b: CocoMetric([], nms_thr=args.thr, nms_backend=b, device=str(dev)) for b in ("host", "device")}
    for m in metrics.values():
        m.results = res
    # the arrays of the device call, as CocoMetric builds them (for the launches alone)
    grab = {}
    import probpose_code_amd.evaluation as E

    real = E.oks_nms_batch
    E.oks_nms_batch = lambda *a, **k: grab.setdefault("args", (a, k)) and real(*a, **k)
    valid_dev = metrics["device"]._instances()  # (also the warm-up of the device path)
    E.oks_nms_batch = real
    (kp, ar, off, thr, sg, guard, f32, _), _ = grab["args"]
    off = np.ascontiguousarray(off, np.int64)
    N, n_img = int(off[-1]), len(off) - 1
    kp_d = torch.from_numpy(np.ascontiguousarray(kp, np.float64)).to(dev)
    ar_d = torch.from_numpy(np.asarray(ar, np.float64)).to(dev)
    sg_d = torch.from_numpy(np.asarray(sg, np.float64)).to(dev)
    size = int(_lib.lib.pp_oks_nms_workspace_bytes(off.ctypes.data, N, n_img))
    ws = torch.empty(size // 8 + 1, dtype=torch.int64, device=dev)
    keep, status = torch.empty(N, dtype=torch.uint8, device=dev), torch.empty(n_img, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        _lib.call("pp_oks_nms_batch", kp_d.data_ptr(), ar_d.data_ptr(), off.ctypes.data, sg_d.data_ptr(), N, n_img, K, float(thr), float(guard),
                  int(f32), ws.data_ptr(), size, keep.data_ptr(), status.data_ptr(), stream)

    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    say(figure="shader_clock_ghz", idle=round(clock_ghz(), 3), under_oks_nms_batch=round(clock_ghz(launch), 3))
    pairs = int(sum(int(n) * (int(n) - 1) // 2 for n in np.diff(off)))
    times = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            launch()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 10)
    times.sort()
    st = status.cpu().numpy()
    say(figure="pp_oks_nms_batch_ms", how="device events around 10 calls (table upload + oks_nms_pairs + oks_nms_sweep), median of rounds",
        median=round(times[len(times) // 2], 4), min=round(times[0], 4), max=round(times[-1], 4), pairs=pairs, workspace_bytes=size,
        guard=OKS_NMS_GUARD, undecided_images=int((st == _lib.PP_OKS_NMS_UNDECIDED).sum()), host_images=int((st == _lib.PP_OKS_NMS_HOST).sum()))

    wall = {"host": [], "device": []}
    valid = {}
    for _ in range(args.rounds):  # alternating in one process
        for b in ("host", "device"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            valid[b] = metrics[b]._instances()
            torch.cuda.synchronize()
            wall[b].append(time.perf_counter() - t0)
    ids = {b: {i: [p["id"] for p in ps] for i, ps in v.items()} for b, v in valid.items()}
    for b in ("host", "device"):
        w = sorted(wall[b])
        say(figure=f"CocoMetric._instances_s[{b}]", median=round(w[len(w) // 2], 4), min=round(w[0], 4), max=round(w[-1], 4),
            kept=sum(len(v) for v in valid[b].values()), nms_fallbacks=metrics[b].nms_fallbacks)
    say(figure="kept_sets_equal", value=ids["host"] == ids["device"] and {i: [p["id"] for p in ps] for i, ps in valid_dev.items()} == ids["host"])


if __name__ == "__main__":
    main()
