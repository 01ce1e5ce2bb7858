"""Times of the device Huffman coder (csrc/pp_jpeg_entropy.hip) beside the host coder it can replace, on the seeded
photo-like frames of scripts/bench_jpeg_encode.py (640x480 and 1920x1080, quality 75, 4:2:0), in ONE run with the two paths
alternated and medians of --rounds:

    entropy_call   pp_jpeg_entropy_encode_batch alone (its seven launches) in device-event time, n = 1 and n = 16, with the
                   shader clock read right behind the timed launches;
    encode_batch   jpeg.encode_batch to the file bytes in host memory, entropy="device" beside entropy="host" (the yardstick:
                   the path as it was, measured in the same run), n = 1 and n = 16, at 1 and 8 workers;
    video_demo     demo/video_demo.py on --frames full-HD frames (synthetic checkpoint, --decode device), frames per second of
                   its loop with --entropy host and --entropy device (--demo-rounds alternations).

With ``--optimize both`` the optimised coder (pp_jpeg_entropy_encode_opt_batch, csrc/pp_jpeg_entropy_opt.hip: the image's own
Huffman tables, built on the device) is timed in the same alternations - entropy_call and encode_batch carry an ``optimize``
field - and the ``file`` figures give the sizes of both kinds of file, also for the drawn demo frame of
scripts/bench_png_encode.py. With ``--parent-lib PATH`` (an earlier build of the library) that build's
pp_jpeg_entropy_encode_batch is timed in the same alternation as this build's (``lib: "parent"``): the default path must lie
within the spread two identical builds show.

With ``--restart-rows N`` and / or ``--restart-interval R`` the coder with restart intervals
(pp_jpeg_entropy_encode_restart_batch) is timed in the same alternations: entropy_call gains a line per kind (``restart``:
"rows N" - a marker every N MCU rows - resp. "interval R" - R MCUs, 1 being the worst case) beside the interval-free call;
with ``--restart-rows`` encode_batch gains device and host entropy at ``restart_rows=N``, and video_demo runs with
``--restart-rows N`` on both sides.

One JSON line per figure.

    python scripts/bench_jpeg_entropy.py [--rounds 7] [--frames 64] [--demo-rounds 3] [--optimize off|both] [--parent-lib PATH]
                                         [--restart-rows N] [--restart-interval R]"""
import argparse
import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--demo-rounds", type=int, default=3)
    ap.add_argument("--optimize", default="off", choices=["off", "both"], help="both: the optimised coder beside the default one")
    ap.add_argument("--parent-lib", default=None, help="an earlier build of libprobpose_mi355x.so: its entropy call is timed beside this build's")
    ap.add_argument("--restart-rows", type=int, default=0, help="N > 0: the coder with a restart marker every N MCU rows beside the interval-free one")
    ap.add_argument("--restart-interval", type=int, default=0, help="R > 0: the coder at a restart interval of R MCUs (1: the worst case) as well")
    args = ap.parse_args()

    import torch

    from probpose_code_amd import _lib, jpeg
    from probpose_code_amd.transforms import BatchStaging
    from probpose_code_amd.video import MjpegAviWriter

    dev = torch.device("cuda:0")
    staging = BatchStaging()
    hd_frames = None
    both = args.optimize == "both"
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.pp_jpeg_entropy_encode_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p]
    if both:
        from scripts.bench_png_encode import drawn_demo_frame

        drawn = torch.from_numpy(np.ascontiguousarray(drawn_demo_frame(dev))).to(dev)
        plain, opt = (jpeg.encode_batch([drawn], channel_order="rgb", staging=staging, entropy="device", optimize=o)[0] for o in (False, True))
        assert opt == jpeg.encode_batch([drawn], channel_order="rgb", staging=staging, entropy="host", optimize=True)[0], "the two coders disagree"
        print(json.dumps(dict(figure="file", size=f"drawn {drawn.shape[1]}x{drawn.shape[0]}", file_bytes=[len(plain)], optimized_file_bytes=[len(opt)],
                              ratio=round(len(opt) / len(plain), 4))), flush=True)
    for W, H in ((640, 480), (1920, 1080)):
        rng = np.random.default_rng(W)
        host_frames = [photo_like(rng, H, W) for _ in range(4)]
        frames = [torch.from_numpy(host_frames[k % 4]).to(dev) for k in range(16)]
        size = f"{W}x{H}"
        if W == 1920:
            hd_frames = frames
        a = jpeg.encode_batch(frames[:4], channel_order="rgb", staging=staging, entropy="host")
        b = jpeg.encode_batch(frames[:4], channel_order="rgb", staging=staging, entropy="device")
        assert a == b, "the two coders disagree"
        sizes = dict(figure="file", size=size, file_bytes=[len(f) for f in a])
        if both:
            o = jpeg.encode_batch(frames[:4], channel_order="rgb", staging=staging, entropy="device", optimize=True)
            assert o == jpeg.encode_batch(frames[:4], channel_order="rgb", staging=staging, entropy="host", optimize=True), "the two optimised coders disagree"
            sizes.update(optimized_file_bytes=[len(f) for f in o], ratio=round(sum(len(f) for f in o) / sum(len(f) for f in a), 4))
        print(json.dumps(sizes), flush=True)

        for n in (1, 16):
            qt = jpeg.quality_tables(75)
            stream = torch.cuda.current_stream(dev)
            # name -> (the call, its staged job): this build's default coder, its optimised coder, the parent build's default coder
            calls = {}
            kinds = ("default",) + (("optimize",) if both else ()) + (("parent",) if parent is not None else ())
            kinds += (("rows",) if args.restart_rows else ()) + (("interval",) if args.restart_interval else ())
            mcus_x = int(jpeg.encode_plan(W, H, "4:2:0").mcus_x)
            restart = {"rows": [args.restart_rows * mcus_x] * n, "interval": [args.restart_interval] * n}
            for name in kinds:
                forward = jpeg._stage_encode(frames[:n], qt, "4:2:0", "rgb", dev, staging, entropy=True, optimize=name == "optimize", restart=restart.get(name))
                _lib.call("pp_jpeg_forward_batch", *forward.args, stream.cuda_stream)
                job = forward.entropy
                ent_args = (job.desc_ptr, n, max(int(i.coef_count) // 64 for i in job.infos), stream.cuda_stream)
                if name == "parent":
                    fn = (lambda a=ent_args: parent.pp_jpeg_entropy_encode_batch(*a))
                elif name in restart:
                    fn = (lambda a=ent_args: _lib.call("pp_jpeg_entropy_encode_restart_batch", *a))
                else:
                    fn = (lambda a=ent_args, f=("pp_jpeg_entropy_encode_opt_batch" if name == "optimize" else "pp_jpeg_entropy_encode_batch"): _lib.call(f, *a))
                calls[name] = (fn, forward)
            for fn, _ in calls.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            us = {name: [] for name in calls}
            for _ in range(args.rounds):
                for name, (fn, _) in calls.items():  # (alternated)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    us[name].append(e0.elapsed_time(e1) * 1e3)
            sclk = shader_clock()  # right behind the timed launches
            for name, (_, forward) in calls.items():
                job = forward.entropy
                res = job.results.cpu().numpy()[:16 * n].view(jpeg._ENT_RESULT)
                assert (res["status"] == 0).all()
                kind = {"rows": f"rows {args.restart_rows}", "interval": f"interval {args.restart_interval}"}.get(name, "none")
                print(json.dumps(dict(figure="entropy_call", size=size, n=n, lib="parent" if name == "parent" else "this", optimize=name == "optimize", restart=kind,
                                      device_event_us=round(statistics.median(us[name]), 1), min_us=round(min(us[name]), 1),
                                      max_us=round(max(us[name]), 1), rounds=args.rounds, stream_bytes=int(res["bytes"].sum()),
                                      coefficient_bytes=int(sum(2 * int(i.coef_count) for i in job.infos)), sclk_mhz=sclk)), flush=True)
            del calls, forward, job

        for n in (1, 16):
            for workers in (1, 8):
                paths = {(e, o, r): (lambda e=e, o=o, r=r: jpeg.encode_batch(frames[:n], channel_order="rgb", workers=workers, staging=staging, entropy=e,
                                                                             optimize=o, restart_rows=r))
                         for e in ("host", "device") for o in ((False, True) if both else (False,)) for r in sorted({0, args.restart_rows})}
                times = {k: [] for k in paths}
                for fn in paths.values():
                    fn()  # warm-up
                for _ in range(args.rounds):
                    for name, fn in paths.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        times[name].append(time.perf_counter() - t0)
                for (name, o, r), ts in times.items():
                    print(json.dumps(dict(figure="encode_batch", size=size, entropy=name, optimize=o, restart_rows=r, n=n, workers=workers,
                                          ms=round(statistics.median(ts) * 1e3, 3),
                                          min_ms=round(min(ts) * 1e3, 3), max_ms=round(max(ts) * 1e3, 3), rounds=args.rounds)), flush=True)

    if args.frames > 0:
        import video_demo

        with tempfile.TemporaryDirectory() as td:
            src = os.path.join(td, "in.avi")
            with MjpegAviWriter(src, 25) as w:
                for k in range(0, args.frames, 16):
                    for f in jpeg.encode_batch([hd_frames[(k + j) % 16] for j in range(min(16, args.frames - k))], channel_order="rgb", staging=staging):
                        w.write(f)
            fps = {"host": [], "device": []}
            for _ in range(args.demo_rounds):
                for e in fps:
                    done = video_demo.main([src, CFG, "synthetic", "--out-video", os.path.join(td, f"out_{e}.avi"), "--decode", "device", "--entropy", e] +
                                           (["--restart-rows", str(args.restart_rows)] if args.restart_rows else []))
                    fps[e].append(done["frames"] / done["seconds"])
            same = open(os.path.join(td, "out_host.avi"), "rb").read() == open(os.path.join(td, "out_device.avi"), "rb").read()
            for e, v in fps.items():
                print(json.dumps(dict(figure="video_demo", size="1920x1080", frames=args.frames, entropy=e, restart_rows=args.restart_rows, frames_per_s=round(statistics.median(v), 1),
                                      min=round(min(v), 1), max=round(max(v), 1), rounds=args.demo_rounds, outputs_equal=same, sclk_mhz=shader_clock())),
                      flush=True)


if __name__ == "__main__":
    main()
