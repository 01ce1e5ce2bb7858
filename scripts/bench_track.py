"""The closed device loop of the pose tracker (tracking.PoseTracker: warp, model step, record pack, pp_track_update, one copy - no host
round trip between two frames) beside the host loop it replaces, on the same device-resident frames, in ONE run:

    loop         --frames seeded photo-like frames (scripts/bench_jpeg_decode.photo_like) of 640x480 and of 1920x1080 lying on the device, 1, 4 and
                 16 tracks. "device": PoseTracker at --depth; "host": per frame apis.inference_topdown on the current boxes, then
                 tracking.next_boxes_host on its samples (the yardstick: what a caller could do before, measured in the same run). The two are
                 alternated inside every round, medians of --rounds with min - max in ms per frame (wall clock around the whole loop, device
                 synchronised), the shader clock read right behind the timed work. kpt_thr = 0 and dup_oks_thr = 2 keep every track alive in both
                 loops, so both run the same number of crops in every frame; ``boxes_equal`` says whether they ended on the same boxes.
    video_demo   demo/video_demo.py on --video-frames full-HD frames (synthetic checkpoint, --decode device), frames per second of its loop
                 without and with --track (--demo-rounds alternations). Without the flag every frame gets the one whole-image box.

One JSON line per figure; nothing is asserted about which loop wins.

    python scripts/bench_track.py [--rounds 7] [--frames 128] [--depth 2] [--video-frames 64] [--demo-rounds 3]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "demo"))
from scripts.bench_jpeg_decode import photo_like  # noqa: E402
from scripts.bench_jpeg_encode import shader_clock  # noqa: E402

CFG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")
PARAMS = dict(kpt_thr=0.0, dup_oks_thr=2.0)


def first_boxes(n, W, H):
    """n boxes of a quarter of the frame's height, 3:4, on a grid."""
    cols = int(np.ceil(np.sqrt(n)))
    h = H / 4
    w = 0.75 * h
    out = []
    for i in range(n):
        cx, cy = (i % cols + 0.5) * W / cols, (i // cols + 0.5) * H / max(1, int(np.ceil(n / cols)))
        out.append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
    return np.array(out, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--video-frames", type=int, default=64)
    ap.add_argument("--demo-rounds", type=int, default=3)
    args = ap.parse_args()

    import torch

    from probpose_code_amd import apis, jpeg, synthetic, tracking
    from probpose_code_amd.evaluation import COCO_SIGMAS
    from probpose_code_amd.video import MjpegAviWriter

    dev = "cuda:0"
    model = apis.init_model(CFG, dict(state_dict=synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device=dev)
    hd = None
    for W, H in ((640, 480), (1920, 1080)):
        rng = np.random.default_rng(W)
        four = [torch.from_numpy(photo_like(rng, H, W)).to(dev) for _ in range(4)]
        if W == 1920:
            hd = four
        frames = [four[k % 4].roll(shifts=3 * k, dims=1) for k in range(args.frames)]  # (a drifting picture: every frame differs)
        for n in (1, 4, 16):
            boxes0 = first_boxes(n, W, H)

            tr = tracking.PoseTracker(model, n, depth=args.depth, **PARAMS)

            def device_loop():
                tr.start(boxes0)
                for f in frames:
                    while tr.in_flight >= args.depth:
                        tr.result()
                    tr.submit(f)
                tr.drain()
                return tr.frame_state["boxes"]

            def host_loop():
                boxes, alive, lost = boxes0.copy(), np.ones(n, np.int32), np.zeros(n, np.int32)
                used = boxes
                for f in frames:
                    used = boxes
                    samples = apis.inference_topdown(model, f, boxes)
                    kp = np.stack([np.asarray(s.pred_instances.keypoints)[0] for s in samples])
                    rec = np.zeros(kp.shape[:2] + (7,))
                    rec[..., 3] = np.stack([np.asarray(s.pred_instances.keypoints_probs).reshape(-1) for s in samples])
                    boxes, alive, lost = tracking.next_boxes_host(rec, None, None, (192, 256), boxes, alive, lost, COCO_SIGMAS, image_keypoints=kp, **PARAMS)
                return used

            paths = dict(device=device_loop, host=host_loop)
            with torch.no_grad():
                ends = {name: fn() for name, fn in paths.items()}  # warm-up: graph captures, pinned buffers
                ends = {name: fn() for name, fn in paths.items()}
                ms = {name: [] for name in paths}
                for _ in range(args.rounds):
                    for name, fn in paths.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        ms[name].append((time.perf_counter() - t0) * 1e3 / len(frames))
            sclk = shader_clock()
            for name in paths:
                print(json.dumps(dict(figure="loop", size=f"{W}x{H}", tracks=n, path=name, ms_per_frame=round(statistics.median(ms[name]), 3),
                                      min_ms=round(min(ms[name]), 3), max_ms=round(max(ms[name]), 3), rounds=args.rounds, frames=len(frames),
                                      depth=args.depth, boxes_equal=bool(np.array_equal(ends["device"], ends["host"])), sclk_mhz=sclk)), flush=True)

    # pp_track_update alone (the rule + the next crop parameters, one launch), device-event time per launch over 200 launches in a row
    for n in (1, 4, 16, 64):
        tr = tracking.PoseTracker(model, n, depth=1, **PARAMS)
        tr.start(first_boxes(n, 1920, 1080))
        tr.submit(hd[0])
        tr.result()  # the block now holds real records
        us = []
        for _ in range(args.rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(tr.stream):
                e0.record(tr.stream)
                for _ in range(200):
                    tr._update(tr._dev[0], tr._dev[1])
                e1.record(tr.stream)
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / 200)
        us = us[1:]
        print(json.dumps(dict(figure="update_call", tracks=n, keypoints=17, us_per_launch=round(statistics.median(us), 2), min_us=round(min(us), 2),
                              max_us=round(max(us), 2), rounds=args.rounds, launches=200, sclk_mhz=shader_clock())), flush=True)

    if args.video_frames > 0:
        import video_demo

        files = jpeg.encode_batch([f.flip(-1) for f in hd], channel_order="rgb")
        with tempfile.TemporaryDirectory() as td:
            src = os.path.join(td, "in.avi")
            with MjpegAviWriter(src, 25) as w:
                for k in range(args.video_frames):
                    w.write(files[k % 4])
            fps = {"plain": [], "track": []}
            for r in range(args.demo_rounds + 1):  # (the first alternation is the warm-up)
                for e in fps:
                    done = video_demo.main([src, CFG, "synthetic", "--out-video", os.path.join(td, f"out_{e}.avi"), "--decode", "device"]
                                           + (["--track"] if e == "track" else []))
                    if r:
                        fps[e].append(done["frames"] / done["seconds"])
            for e, v in fps.items():
                print(json.dumps(dict(figure="video_demo", size="1920x1080", frames=args.video_frames, path=e, frames_per_s=round(statistics.median(v), 1),
                                      min=round(min(v), 1), max=round(max(v), 1), rounds=args.demo_rounds, sclk_mhz=shader_clock())), flush=True)


if __name__ == "__main__":
    main()
