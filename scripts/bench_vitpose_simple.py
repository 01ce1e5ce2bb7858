"""dev only: ViTPose-S-simple (FeatureMapProcessor x4 + 3x3 final layer, composed: csrc/pp_simple_head.hip) beside ViTPose-S classic and
ProbPose-S in ONE process, the paths alternated, medians of 7, synthetic weights, f16x3. One JSON line per figure:

  step        the step at bs 64 with flip test through StepPipeline(depth=2) (two batches in flight, captured graphs), per model;
  head_launch the head's launches alone by device events (engine.profile: pp_relu_operand, the tap GEMM, pp_taps_upsample4_conv3x3 and
              the decode), at bs 1 and bs 64 with flip test, from features that stay in place;
  gather_bw   the gather kernel's bytes (tap planes read + logits written) over its time, and that as a share of the 8.0 TB/s HBM peak.

Every line carries the shader clock (pp_clock_probe on a side stream) read BEHIND the timed work it belongs to, under the same load.
    python scripts/bench_vitpose_simple.py [--rounds 7] [--steps 20]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from probpose_code_amd import _lib
from probpose_code_amd import synthetic as S
from probpose_code_amd.engine import ProbPoseEngine
from probpose_code_amd.pipeline import StepPipeline

dev = torch.device("cuda:0")
HBM_PEAK = 8.0e12  # bytes / s, the MI355X's HBM3E specification
MODELS = {"vitpose_s_simple": "heatmap-simple", "vitpose_s_classic": "heatmap", "probpose_s": "probmap"}


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def clock_ghz(busy, window_us=200_000):
    """Average shader clock over `window_us` (pp_clock_probe: one sleeping wavefront on a side stream) while `busy()` is launched over and over."""
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    _lib.call("pp_clock_probe", out.data_ptr(), None, int(window_us), side.cuda_stream)
    t_end = time.perf_counter() + window_us * 1e-6
    while time.perf_counter() < t_end:
        busy()
    torch.cuda.synchronize()
    cyc, ticks = (int(v) for v in out.tolist())
    return cyc / max(1, ticks) * 0.1


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    rounds, steps, B = arg("--rounds", 7), arg("--steps", 20), 64
    emit(figure="device", name=torch.cuda.get_device_name(0), rounds=rounds, steps_per_round=steps)
    engines = {name: ProbPoseEngine(S.synthetic_state_dict("small", seed=0, logit_scale=2.0, head=head), 12, precision="f16x3")
               for name, head in MODELS.items()}
    crops = [S.synthetic_crops(B, seed=100 + i).to(dev) for i in range(4)]

    # ---- the step at bs 64 with flip test, two batches in flight; the three models alternated round by round
    pipes = {name: StepPipeline(eng, B, S.COCO_FLIP_INDICES, flip_test=True, depth=2, use_graph="full") for name, eng in engines.items()}

    def run_steps(pipe, n):
        pending = []
        for i in range(n):
            if len(pending) >= 2:
                pipe.result(pending.pop(0))
            pending.append(pipe.submit(crops[i % 4]))
        while pending:
            pipe.result(pending.pop(0))
        torch.cuda.synchronize()

    for pipe in pipes.values():
        run_steps(pipe, 6)  # warm-up: captures the slots' graphs
    ms = {name: [] for name in pipes}
    for _ in range(rounds):
        for name, pipe in pipes.items():
            run_steps(pipe, 2)
            t0 = time.perf_counter()
            run_steps(pipe, steps)
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    for name, pipe in pipes.items():
        med = statistics.median(ms[name])
        emit(figure="step", model=name, bs=B, flip_test=True, precision="f16x3", in_flight=2, ms_per_step_median=round(med, 4),
             ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4), crops_per_s=round(B / med * 1e3, 1),
             shader_clock_ghz=round(clock_ghz(lambda p=pipe: p.result(p.submit(crops[0])), 400_000), 3))
    del pipes

    # ---- the head launches alone, by device events, from features that stay in place
    eng = engines["vitpose_s_simple"]
    cls = engines["vitpose_s_classic"]
    for bs in (1, 64):
        per, counts = {}, {"simple": {}, "classic": {}}
        for e, label in ((eng, "simple"), (cls, "classic")):
            feat = e.run_backbone(crops[0][:bs], True).clone()
            for _ in range(3):
                e.run_head(feat, True, S.COCO_FLIP_INDICES)
            per[label] = (e, feat, {})
        for _ in range(rounds):  # alternated: simple, classic, simple, classic ...
            for label, (e, feat, acc) in per.items():
                e.profile = {}
                for _ in range(10):
                    e.run_head(feat, True, S.COCO_FLIP_INDICES)
                torch.cuda.synchronize()
                for tag, evs in e.profile.items():  # per tag: the sum over its launches of one head, and how many those are
                    acc.setdefault(tag, []).append(sum(a.elapsed_time(b) for a, b in evs) / 10 * 1e3)
                    counts[label][tag] = len(evs) // 10
                e.profile = None
        for label, (e, feat, acc) in per.items():
            us = {tag: round(statistics.median(v), 2) for tag, v in acc.items()}
            emit(figure="head_launch", model="vitpose_s_" + label, bs=bs, flip_test=True, us_per_head_by_tag_median=us, launches_per_head=counts[label],
                 us_head_total=round(sum(us.values()), 2), note="device events around every launch: the launches of a head run one after the other",
                 shader_clock_ghz=round(clock_ghz(lambda e=e, f=feat: e.run_head(f, True, S.COCO_FLIP_INDICES)), 3))
        if bs == 64:
            nb = 2 * bs
            nbytes = nb * 9 * eng.K * eng.Np * 4 + nb * eng.K * eng.Hh * eng.Wh * 4
            t_us = statistics.median(per["simple"][2]["taps_upsample"])
            ws = eng._workspace(bs, 2)

            def gather(ws=ws, nb=nb):
                _lib.call("pp_taps_upsample4_conv3x3", ws["taps"].data_ptr(), eng.w["final.b"].data_ptr(), ws["logits"].data_ptr(), nb, eng.K, eng.Hp, eng.Wp,
                          _lib.stream_ptr(dev))

            emit(figure="gather_bw", kernel="pp_taps_upsample4_conv3x3", n_img=nb, bytes=nbytes, us_median=round(t_us, 2),
                 tb_per_s=round(nbytes / t_us / 1e6, 3), share_of_hbm_peak=round(nbytes / (t_us * 1e-6) / HBM_PEAK, 4), hbm_peak_tb_per_s=HBM_PEAK / 1e12,
                 shader_clock_ghz=round(clock_ghz(gather), 3))


if __name__ == "__main__":
    main()
