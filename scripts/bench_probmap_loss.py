"""dev only: time the loss mode. In ONE run, the paths alternated round by round: pp_probmap_encode and pp_probmap_loss_maps at bs 64 and
bs 512 (17 x 64 x 48), the whole model.loss call beside test_step of the same batch, and the numpy / torch-CPU restatement of the
same batch. Device events, medians of 7, the shader clock (pp_clock_probe, measured under the load it stands beside) with every figure.
    python scripts/bench_probmap_loss.py [--no-model]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

import probpose_code_amd as pp
from probpose_code_amd import _lib
from probpose_code_amd import synthetic as S
from probpose_code_amd.losses import OKSHeatmapLoss

K, H, W = 17, 64, 48
ROUNDS, ITERS = 7, 20
dev = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clock_ghz(busy, window_us=100_000):
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    _lib.call("pp_clock_probe", out.data_ptr(), None, int(window_us), side.cuda_stream)
    t_end = time.perf_counter() + window_us * 1e-6
    while time.perf_counter() < t_end:
        busy()
    torch.cuda.synchronize()
    cyc, ticks = (int(v) for v in out.tolist())
    return cyc / max(1, ticks) * 0.1


def alternated(paths):
    """{name: fn} -> {name: (median us, min, max)}: ROUNDS rounds, in each every path timed once (ITERS back-to-back calls between two
    device events), so that a clock or thermal drift meets all paths alike."""
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in paths}
    for _ in range(ROUNDS):
        for n, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / ITERS * 1e3)
    return {n: (sorted(v)[len(v) // 2], min(v), max(v)) for n, v in times.items()}


def report(res, clocks, note=""):
    for n, (med, lo, hi) in res.items():
        print(f"  {n:<34s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f}; shader clock {clocks[n]:.2f} GHz) {note}")


def host_restatement(kp, vis, pred, w):
    """The same batch on the CPU: the codec's numpy encode per instance, the map loss as torch-CPU ops in float32 (the reference's form)."""
    codec = pp.KEYPOINT_CODECS.build(dict(type="ProbMap", input_size=(192, 256), heatmap_size=(48, 64), sigma=-1))
    t0 = time.perf_counter()
    maps = np.stack([codec.encode(kp[b:b + 1], vis[b:b + 1])["heatmaps"] for b in range(kp.shape[0])])
    t1 = time.perf_counter()
    p, t = torch.from_numpy(pred), torch.from_numpy(maps)
    B = p.shape[0]
    kx = torch.tensor([[1, 0, -1], [2, 0, -2], [1, 0, -1]], dtype=torch.float32).view(1, 1, 3, 3)
    ky = torch.tensor([[1, 2, 1], [0, 0, 0], [-1, -2, -1]], dtype=torch.float32).view(1, 1, 3, 3)
    gx = torch.nn.functional.conv2d(p.reshape(B * K, 1, H, W), kx, padding="same")
    gy = torch.nn.functional.conv2d(p.reshape(B * K, 1, H, W), ky, padding="same")
    m = torch.from_numpy(w)[:, :, None, None]
    loss = (0.05 * (gx ** 2 + gy ** 2).reshape(B, K, H, W) * m + 0.95 * p * (1 - t) * m).mean()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, float(loss)


def main():
    print(torch.cuda.get_device_name(0), f"- medians of {ROUNDS} rounds of {ITERS} calls, paths alternated")
    rng = np.random.default_rng(0)
    codec = pp.KEYPOINT_CODECS.build(dict(type="ProbMap", input_size=(192, 256), heatmap_size=(48, 64), sigma=-1))
    loss_mod = OKSHeatmapLoss(use_target_weight=True, smoothing_weight=0.05)
    for B in (64, 512):
        kp_h = np.stack([rng.uniform(-20, 212, (B, K)), rng.uniform(-20, 276, (B, K))], -1).astype(np.float32)
        vis_h = (rng.random((B, K)) < 0.85).astype(np.float32)
        kp, vis = torch.from_numpy(kp_h).to(dev), torch.from_numpy(vis_h).to(dev)
        enc = codec.encode_device(kp, vis)
        pred = (enc["heatmaps"] * 0.3).clamp(0, 1).roll(1, -1).contiguous()
        paths = dict(pp_probmap_encode=lambda: codec.encode_device(kp, vis),
                     pp_probmap_loss_maps=lambda: loss_mod(pred, enc["heatmaps"], enc["keypoint_weights"]))
        res = alternated(paths)
        clocks = {n: clock_ghz(fn) for n, fn in paths.items()}
        print(f"bs {B} ({B * K} maps of {H} x {W}; the calls include their output allocations):")
        report(res, clocks)
        if B == 64:
            e_us, l_us, _ = host_restatement(kp_h, vis_h, pred.cpu().numpy(), enc["keypoint_weights"].cpu().numpy())
            print(f"  numpy encode on the host           {e_us:9.0f} us;  torch-CPU map loss ({torch.get_num_threads()} threads) {l_us:9.0f} us")
    if "--no-model" in sys.argv:
        return
    from probmap_loss_cases import make_samples  # (sample construction only)
    from probpose_code_amd import apis
    from probpose_code_amd.config import Config

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py"))
    model = apis.init_model(cfg, dict(state_dict=S.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device="cuda:0")
    B = 64
    crops = S.synthetic_crops(B, seed=1).to(dev)
    g = dict(keypoints=np.stack([rng.uniform(0, 192, (B, K)), rng.uniform(0, 256, (B, K))], -1).astype(np.float32),
             keypoints_visible=np.ones((B, K), np.float32), keypoints_visibility=(rng.random((B, K)) < 0.5).astype(np.float32))
    samples = make_samples(g, device_targets=True)
    for s in samples:
        s.set_metainfo(dict(flip_indices=list(S.COCO_FLIP_INDICES), input_center=np.array([96.0, 128.0], np.float32),
                            input_scale=np.array([192.0, 256.0], np.float32), input_size=(192, 256)))
        s.gt_instances.bboxes = np.array([[0, 0, 192, 256]], np.float32)
        s.gt_instances.bbox_scores = np.ones(1, np.float32)
    paths = {"model.loss (one pass, with accuracies)": lambda: model.loss(crops, samples),
             "model.loss (compute_acc=False)": lambda: model.loss(crops, samples, train_cfg=dict(compute_acc=False)),
             "test_step (flip test)": lambda: model.test_step(dict(inputs=list(crops), data_samples=samples))}
    res = alternated(paths)
    clocks = {n: clock_ghz(fn) for n, fn in paths.items()}
    print(f"bs {B}, precision {model.precision} (host work between the launches included; test_step runs two passes):")
    report(res, clocks)


if __name__ == "__main__":
    main()
