"""dev only: the ViTPose family in one run - the step time of ViTPose-S / -B / -L / -H (HeatmapHead, synthetic weights) at bs 64 with
flip test, f16x3, through StepPipeline(depth=2), and pp_attention per launch at (192 tokens, head dim 64) beside (192, 80) with 16
heads and n_seq = 128 (one bs-64 step with the flipped pass) in the three precisions, alternated A B A B. Prints the shader clock
(pp_clock_probe) first and under each load. The only derived expectation: the head-dim-80 launch runs 1.375x the MFMAs of the
head-dim-64 launch (q . k padded to 96: 1.5x; P V over 80 columns: 1.25x) and moves 1.25x the bytes.
    python scripts/bench_vitpose_family.py [--archs small,base,large,huge] [--no-steps]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from probpose_code_amd import _lib
from probpose_code_amd import synthetic as S
from probpose_code_amd.engine import ProbPoseEngine
from probpose_code_amd.pipeline import StepPipeline
from probpose_code_amd.weights import to_split

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
print(f"shader clock, idle: {clock_ghz():.2f} GHz")

# ---- pp_attention per launch: (192, 64) beside (192, 80), 16 heads, n_seq = 128
N_SEQ, TOKENS, HEADS = 128, 192, 16
g = torch.Generator(device="cpu").manual_seed(0)
for prec_name, prec in (("f16x3", 2), ("bf16", 0), ("f32", 1)):
    launches = {}
    for hd in (64, 80):
        E = HEADS * hd
        qkv = torch.randn(N_SEQ * TOKENS, 3 * E, generator=g)
        qkv = to_split(qkv) if prec == 2 else qkv.to(torch.bfloat16 if prec == 0 else torch.float32)
        qkv = qkv.to(dev)
        out = torch.empty(N_SEQ * TOKENS, E, dtype=qkv.dtype, device=dev)

        def launch(qkv=qkv, out=out, hd=hd):
            _lib.call("pp_attention", prec, qkv.data_ptr(), out.data_ptr(), N_SEQ, TOKENS, HEADS, hd, hd ** -0.5, None)

        launches[hd] = (launch, 4 * N_SEQ * TOKENS * E * qkv.element_size())
    med = {}
    for hd in (64, 80, 64, 80):  # alternated: A B A B
        fn, nbytes = launches[hd]
        m, lo, hi = timed(fn)
        med.setdefault(hd, []).append(m)
        print(f"pp_attention {prec_name:5s} n_seq {N_SEQ} heads {HEADS} (192, {hd}): {m:7.1f} us / launch (min {lo:.1f}, max {hi:.1f})  {nbytes / m / 1e3:7.1f} GB/s")
    r = min(med[80]) / min(med[64])
    print(f"    {prec_name}: head dim 80 / head dim 64 = {r:.2f}x (MFMA work 1.375x, bytes 1.25x); shader clock under (192, 64) "
          f"{clock_ghz(launches[64][0]):.2f} GHz, under (192, 80) {clock_ghz(launches[80][0]):.2f} GHz")
    del launches

# ---- step time per arch: bs 64, flip test, f16x3, two steps in flight
if "--no-steps" not in sys.argv:
    archs = "small,base,large,huge"
    if "--archs" in sys.argv:
        archs = sys.argv[sys.argv.index("--archs") + 1]
    B = 64
    crops = [S.synthetic_crops(B, seed=100 + i).to(dev) for i in range(4)]
    for arch in archs.split(","):
        a = S.ARCHS[arch]
        eng = ProbPoseEngine(S.synthetic_state_dict(arch, seed=0, logit_scale=2.0, head="heatmap"), a["num_heads"], precision="f16x3")
        print(f"ViTPose-{arch} (E {a['embed_dims']}, {a['num_layers']} layers, {a['num_heads']} heads of {a['embed_dims'] // a['num_heads']}): {eng.layer_plan}")
        pipe = StepPipeline(eng, B, S.COCO_FLIP_INDICES, flip_test=True, depth=2, use_graph="full")
        for rnd in range(3):
            for i in range(6 if rnd == 0 else 2):  # warm-up (captures the slots' graphs in the first round)
                pipe.result(pipe.submit(crops[i % 4]))
            torch.cuda.synchronize()
            n, t0, pending = 20, time.perf_counter(), []
            for i in range(n):
                if len(pending) >= 2:
                    pipe.result(pending.pop(0))
                pending.append(pipe.submit(crops[i % 4]))
            while pending:
                pipe.result(pending.pop(0))
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            print(f"round {rnd} ViTPose-{arch:5s} bs {B} f16x3 flip StepPipeline(depth=2): {dt * 1e3:8.3f} ms / step = {B / dt:7.0f} crops / s", flush=True)

        def step(pipe=pipe):
            pipe.result(pipe.submit(crops[0]))

        print(f"    shader clock under the ViTPose-{arch} steps {clock_ghz(step, 400_000):.2f} GHz", flush=True)
        del pipe, eng
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
