"""dev only: time pp_udp_heatmap_decode (the ViTPose baseline's UDP-DARK decode) beside pp_probmap_decode_flags (ProbPose's
Sparsemax + OKS decode, which does strictly more: the yardstick) on the same shapes in the same run - B = 64 and 512, 17 x 64 x 48
logits with the flipped pass, row-major and phase-separated - and the ViTPose-S step beside the ProbPose-S step through
StepPipeline(depth=2) at bs 64. Prints the shader clock (pp_clock_probe) first.
    python scripts/bench_udp_decode.py [--no-steps]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from probpose_code_amd import _lib
from probpose_code_amd import synthetic as S
from probpose_code_amd.codecs import oks_kernel_taps
from probpose_code_amd.engine import ProbPoseEngine
from probpose_code_amd.pipeline import StepPipeline

K, H, W = 17, 64, 48
dev = torch.device("cuda:0")


def clock_ghz(busy=None, window_us=200_000):
    """Average shader clock over a window of `window_us` (pp_clock_probe: one sleeping wavefront on a side stream) while `busy()` is
    launched over and over on the current stream."""
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    _lib.call("pp_clock_probe", out.data_ptr(), None, int(window_us), side.cuda_stream)
    t_end = time.perf_counter() + window_us * 1e-6
    while busy is not None and time.perf_counter() < t_end:
        busy()
    torch.cuda.synchronize()
    cyc, ticks = (int(v) for v in out.tolist())
    return cyc / max(1, ticks) * 0.1


def timed(fn, iters=50, rounds=5):
    """Median over `rounds` of the mean launch time of `iters` back-to-back launches, HIP events, after a warm-up."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters * 1e3)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


print(torch.cuda.get_device_name(0))
g = torch.Generator(device="cpu").manual_seed(0)
taps, radius = oks_kernel_taps(K, H, W)
taps, radius = torch.from_numpy(taps).to(dev), torch.from_numpy(radius).to(dev)
fi = torch.tensor(list(S.COCO_FLIP_INDICES), dtype=torch.int32, device=dev)
for B in (64, 512):
    # blob-shaped logits (a peak of height 4 - 8 on noise of sigma 1): what a trained head emits, for both kernels
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    cx, cy = torch.rand(2 * B, K, 1, 1, generator=g) * (W - 1), torch.rand(2 * B, K, 1, 1, generator=g) * (H - 1)
    amp = 4 + 4 * torch.rand(2 * B, K, 1, 1, generator=g)
    logits = (amp * torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 8.0) + torch.randn(2 * B, K, H, W, generator=g)).to(dev).contiguous()
    locs = torch.empty(B, K, 2, device=dev)
    kpts = torch.empty(B, K, 2, dtype=torch.float64, device=dev)
    scores = torch.empty(B, K, device=dev)
    nbytes = 2 * B * K * H * W * 4
    for phased in (0, 2):
        def udp():
            _lib.call("pp_udp_heatmap_decode", logits.data_ptr(), logits[B:].data_ptr(), fi.data_ptr(), B, K, H, W, 192.0, 256.0, 11, None,
                      locs.data_ptr(), kpts.data_ptr(), scores.data_ptr(), phased, None)

        def probmap():
            _lib.call("pp_probmap_decode_flags", logits.data_ptr(), logits[B:].data_ptr(), fi.data_ptr(), taps.data_ptr(), radius.data_ptr(), B, K, H,
                      W, 192.0, 256.0, 0.5, 1.0, None, None, locs.data_ptr(), kpts.data_ptr(), scores.data_ptr(), 1 | phased, None)

        for name, fn in (("pp_udp_heatmap_decode", udp), ("pp_probmap_decode_flags", probmap), ("pp_udp_heatmap_decode", udp),
                         ("pp_probmap_decode_flags", probmap)):  # alternated: A B A B
            med, lo, hi = timed(fn)
            print(f"B {B:3d} {'phased   ' if phased else 'row-major'} {name:24s} {med:7.1f} us (min {lo:.1f}, max {hi:.1f})  "
                  f"{nbytes / med / 1e3:7.1f} GB/s of logits")
        print(f"    shader clock under pp_udp_heatmap_decode launches {clock_ghz(udp):.2f} GHz, under pp_probmap_decode_flags {clock_ghz(probmap):.2f} GHz")

if "--no-steps" not in sys.argv:
    B = 64
    crops = [S.synthetic_crops(B, seed=100 + i).to(dev) for i in range(4)]
    engines = {"ProbPose-S (probmap head)": ProbPoseEngine(S.synthetic_state_dict("small", seed=0, logit_scale=2.0), 12, precision="f16x3"),
               "ViTPose-S (heatmap head)": ProbPoseEngine(S.synthetic_state_dict("small", seed=0, logit_scale=2.0, head="heatmap"), 12, precision="f16x3")}
    pipes = {n: StepPipeline(e, B, S.COCO_FLIP_INDICES, flip_test=True, depth=2, use_graph="full") for n, e in engines.items()}
    for rnd in range(3):  # alternated, three rounds
        for name, pipe in pipes.items():
            for i in range(6):  # warm-up (captures the slots' graphs in the first round)
                pipe.result(pipe.submit(crops[i % 4]))
            torch.cuda.synchronize()
            n, t0, pending = 40, time.perf_counter(), []
            for i in range(n):
                if len(pending) >= 2:
                    pipe.result(pending.pop(0))
                pending.append(pipe.submit(crops[i % 4]))
            while pending:
                pipe.result(pending.pop(0))
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            print(f"round {rnd} {name:28s} bs {B} f16x3 StepPipeline(depth=2): {dt * 1e3:7.3f} ms / step = {B / dt:7.0f} crops / s")
    def step():
        p = pipes["ViTPose-S (heatmap head)"]
        p.result(p.submit(crops[0]))

    print(f"shader clock under the ViTPose-S steps {clock_ghz(step, 400_000):.2f} GHz")
