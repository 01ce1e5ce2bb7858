"""dev only: time the two swapped head x codec launches beside what they replace / stand next to, in one run, alternated (A B A B),
17 x 64 x 48 with the flipped pass, phase-separated input, bs 64 and bs 512, the shader clock recorded under each:
  * pp_argmax_probmap_decode (Sparsemax + UDP argmax + DARK, one launch) beside the two-launch chain it replaces:
    pp_probmap_decode_flags(PP_DECODE_LOGITS | PP_DECODE_PHASED, avg_out = maps) -> pp_udp_heatmap_decode(maps);
  * pp_expmax_heatmap_decode on ViTPose-like dense maps beside pp_probmap_decode_flags on Sparsemax logits (a dense map's support is
    the whole map: the convolution takes several bands where a Sparsemax map takes one box);
  * the two swapped steps at bs 64 (StepPipeline, depth 2, graphs) beside their default-codec steps.
    python scripts/bench_codec_swap.py [--no-steps] [--lib OTHER.so]
--lib: also time pp_probmap_decode_flags / pp_udp_heatmap_decode of another build of the library (an A/B of the existing launches)."""
import ctypes
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
PHASED = 2
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


def timed(fn, iters=200, rounds=5):
    """Median over `rounds` of the mean time of `iters` back-to-back calls, HIP events, after a warm-up."""
    for _ in range(10):
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


other = None
if "--lib" in sys.argv:
    other = ctypes.CDLL(os.path.abspath(sys.argv[sys.argv.index("--lib") + 1]))
    for name in ("pp_probmap_decode_flags", "pp_udp_heatmap_decode"):
        getattr(other, name).restype, getattr(other, name).argtypes = _lib.SIGNATURES[name]

print(torch.cuda.get_device_name(0))
g = torch.Generator(device="cpu").manual_seed(0)
taps, radius = oks_kernel_taps(K, H, W)
taps, radius = torch.from_numpy(taps).to(dev), torch.from_numpy(radius).to(dev)
fi = torch.tensor(list(S.COCO_FLIP_INDICES), dtype=torch.int32, device=dev)
yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
for B in (64, 512):
    cx, cy = torch.rand(2 * B, K, 1, 1, generator=g) * (W - 1), torch.rand(2 * B, K, 1, 1, generator=g) * (H - 1)
    blob = torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 8.0)
    # head logits: a peak of height 4 - 8 on noise of sigma 1 (what a trained ProbMapHead emits); ViTPose maps: a Gaussian of height
    # 0.3 - 1 on noise of sigma 0.02 (dense: every pixel is non-zero). The layout does not change the values' statistics.
    logits = ((4 + 4 * torch.rand(2 * B, K, 1, 1, generator=g)) * blob + torch.randn(2 * B, K, H, W, generator=g)).to(dev).contiguous()
    dense = ((0.3 + 0.7 * torch.rand(2 * B, K, 1, 1, generator=g)) * blob + 0.02 * torch.randn(2 * B, K, H, W, generator=g)).to(dev).contiguous()
    maps = torch.empty(B, K, H, W, device=dev)
    locs = torch.empty(B, K, 2, device=dev)
    kpts = torch.empty(B, K, 2, dtype=torch.float64, device=dev)
    scores = torch.empty(B, K, device=dev)
    out3 = (locs.data_ptr(), kpts.data_ptr(), scores.data_ptr())

    def argmax_fused():
        _lib.call("pp_argmax_probmap_decode", logits.data_ptr(), logits[B:].data_ptr(), fi.data_ptr(), B, K, H, W, 192.0, 256.0, 0.5, 1.0, 11, None,
                  *out3, PHASED, None)

    def chain(lib=_lib.lib):
        lib.pp_probmap_decode_flags(logits.data_ptr(), logits[B:].data_ptr(), fi.data_ptr(), taps.data_ptr(), radius.data_ptr(), B, K, H, W, 192.0,
                                    256.0, 0.5, 1.0, maps.data_ptr(), None, *out3, 1 | PHASED, None)
        lib.pp_udp_heatmap_decode(maps.data_ptr(), None, None, B, K, H, W, 192.0, 256.0, 11, None, *out3, 0, None)

    def expmax():
        _lib.call("pp_expmax_heatmap_decode", dense.data_ptr(), dense[B:].data_ptr(), fi.data_ptr(), taps.data_ptr(), radius.data_ptr(), B, K, H, W,
                  192.0, 256.0, None, None, *out3, PHASED, None)

    def probmap(lib=_lib.lib):
        lib.pp_probmap_decode_flags(logits.data_ptr(), logits[B:].data_ptr(), fi.data_ptr(), taps.data_ptr(), radius.data_ptr(), B, K, H, W, 192.0,
                                    256.0, 0.5, 1.0, None, None, *out3, 1 | PHASED, None)

    def udp(lib=_lib.lib):
        lib.pp_udp_heatmap_decode(dense.data_ptr(), dense[B:].data_ptr(), fi.data_ptr(), B, K, H, W, 192.0, 256.0, 11, None, *out3, PHASED, None)

    pairs = [("pp_argmax_probmap_decode (one launch)", argmax_fused), ("probmap_decode_flags -> udp_heatmap_decode (chain)", chain),
             ("pp_expmax_heatmap_decode (dense maps)", expmax), ("pp_probmap_decode_flags (Sparsemax logits)", probmap),
             ("pp_udp_heatmap_decode (dense maps)", udp)]
    if other is not None:
        pairs += [("  other build: pp_probmap_decode_flags", lambda: probmap(other)), ("  other build: pp_udp_heatmap_decode", lambda: udp(other)),
                  ("  other build: chain", lambda: chain(other))]
    for rnd in range(2):  # alternated: every launch once, then every launch again
        for name, fn in pairs:
            med, lo, hi = timed(fn)
            print(f"B {B:3d} phased round {rnd} {name:52s} {med:7.1f} us (min {lo:.1f}, max {hi:.1f})")
    print(f"    shader clock under pp_argmax_probmap_decode {clock_ghz(argmax_fused):.2f} GHz, under the chain {clock_ghz(chain):.2f} GHz, "
          f"under pp_expmax_heatmap_decode {clock_ghz(expmax):.2f} GHz, under pp_probmap_decode_flags {clock_ghz(probmap):.2f} GHz")

if "--no-steps" not in sys.argv:
    B = 64
    crops = [S.synthetic_crops(B, seed=100 + i).to(dev) for i in range(4)]
    pm = S.synthetic_state_dict("small", seed=0, logit_scale=2.0)
    hm = S.synthetic_state_dict("small", seed=0, logit_scale=2.0, head="heatmap")
    engines = {"ProbPose-S + ProbMap (default)": ProbPoseEngine(pm, 12, precision="f16x3"),
               "ProbPose-S + ArgMaxProbMap": ProbPoseEngine(pm, 12, precision="f16x3", decode="dark"),
               "ViTPose-S + UDPHeatmap (default)": ProbPoseEngine(hm, 12, precision="f16x3"),
               "ViTPose-S + UDPExpMaxHeatmap": ProbPoseEngine(hm, 12, precision="f16x3", decode="expmax")}
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
            print(f"round {rnd} {name:34s} bs {B} f16x3 StepPipeline(depth=2): {dt * 1e3:7.3f} ms / step = {B / dt:7.0f} crops / s")

    def step():
        p = pipes["ProbPose-S + ArgMaxProbMap"]
        p.result(p.submit(crops[0]))

    print(f"shader clock under the ProbPose-S + ArgMaxProbMap steps {clock_ghz(step, 400_000):.2f} GHz")
