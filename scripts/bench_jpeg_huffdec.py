"""Times of the device Huffman decoder (csrc/pp_jpeg_huffdec.hip) beside the host decoder it can replace, on the seeded
photo-like frames of scripts/bench_jpeg_encode.py (640x480 and 1920x1080, quality 75, 4:2:0), in ONE run with the two paths
alternated and medians of --rounds:

    huffman_call   pp_jpeg_huffman_decode_batch alone (sync_passes + 4 launches) in device-event time, n = 1 and n = 16, with
                   the passes the images needed and the shader clock read right behind the timed launches;
    decode_batch   jpeg.decode_batch from the file bytes in host memory to BGR pixels on the device, entropy="device" beside
                   entropy="host" (the yardstick: the path as it was, measured in the same run; its Huffman decoding on a pool
                   of 1 and of 8 threads, as runner.test_dataset spreads it), n = 1 and n = 16;
    video_demo     demo/video_demo.py on --frames full-HD frames (synthetic checkpoint, --decode device), frames per second of
                   its loop without and with --decode-entropy device (--demo-rounds alternations).

--restart-interval R (MCUs, or "row" for one MCU row of the frame) also writes the frames with that restart interval (the
host coder writes them) and measures them beside the files without one: huffman_call with the two alternated call by
call, decode_batch for each. One JSON line per figure, ``restart_interval`` in it.

    python scripts/bench_jpeg_huffdec.py [--rounds 7] [--frames 64] [--demo-rounds 3] [--restart-interval row]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

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
    ap.add_argument("--restart-interval", default="0", help='MCUs between restart markers of a second set of files, or "row"; 0: none')
    args = ap.parse_args()
    if args.restart_interval != "row" and not 0 <= int(args.restart_interval) <= 65535:
        ap.error("--restart-interval is 0..65535 or row")

    import torch

    from probpose_code_amd import _lib, jpeg
    from probpose_code_amd.transforms import BatchStaging
    from probpose_code_amd.video import MjpegAviWriter

    dev = torch.device("cuda:0")
    staging = BatchStaging()
    hd_files = None
    for W, H in ((640, 480), (1920, 1080)):
        rng = np.random.default_rng(W)
        frames = [torch.from_numpy(photo_like(rng, H, W)).to(dev) for _ in range(4)]
        ri = (W + 15) // 16 if args.restart_interval == "row" else int(args.restart_interval)
        sets = {}
        for r in dict.fromkeys((0, ri)):
            four = jpeg.encode_batch(frames, channel_order="rgb", staging=staging, restart_interval=r)
            sets[r] = [four[k % 4] for k in range(16)]
            a = jpeg.decode_batch(four, dev, entropy="host", staging=staging)
            b = jpeg.decode_batch(four, dev, entropy="device", staging=staging)
            assert all(torch.equal(x, y) for x, y in zip(a, b)), "the two decoders disagree"
            print(json.dumps(dict(figure="file", size=f"{W}x{H}", restart_interval=r, file_bytes=[len(f) for f in four])), flush=True)
        size = f"{W}x{H}"
        if W == 1920:
            hd_files = sets[ri]

        for n in (1, 16):
            stream = torch.cuda.current_stream(dev)
            jobs, scans = {}, {}
            for r, files in sets.items():
                scans[r] = [jpeg.scan_prepare(f, restart=True) for f in files[:n]]
                jobs[r] = jpeg._stage_huffman(scans[r], dev, BatchStaging(), jpeg.DEFAULT_SYNC_PASSES, False)
                for _ in range(3):
                    _lib.call("pp_jpeg_huffman_decode_batch", *jobs[r].args, stream.cuda_stream)
            torch.cuda.synchronize()
            us = {r: [] for r in jobs}
            for _ in range(args.rounds):
                for r, job in jobs.items():  # alternated call by call
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    _lib.call("pp_jpeg_huffman_decode_batch", *job.args, stream.cuda_stream)
                    e1.record()
                    e1.synchronize()
                    us[r].append(e0.elapsed_time(e1) * 1e3)
            sclk = shader_clock()  # right behind the timed launches
            for r, job in jobs.items():
                res = job.results.cpu().numpy().view(jpeg._HD_RESULT)
                assert (res["status"] == 0).all()
                print(json.dumps(dict(figure="huffman_call", size=size, restart_interval=r, n=n, device_event_us=round(statistics.median(us[r]), 1),
                                      min_us=round(min(us[r]), 1), max_us=round(max(us[r]), 1), rounds=args.rounds, sync_passes=jpeg.DEFAULT_SYNC_PASSES,
                                      passes_used=int(res["passes"].max()), stream_bytes=int(sum(s.stream.size for s in scans[r])),
                                      coefficient_bytes=int(sum(2 * int(s.info.coef_count) for s in scans[r])), sclk_mhz=sclk)), flush=True)
            del jobs

        for r, files in sets.items():
            for n in (1, 16):
                for workers in (1, 8):
                    pool = ThreadPoolExecutor(max_workers=workers)

                    def host(n=n, pool=pool, files=files):  # the path as it is: Huffman decoding on the threads, one reconstruct call
                        return jpeg.reconstruct_batch(list(pool.map(jpeg.entropy_decode, files[:n])), dev, staging)

                    paths = {"host": host, "device": lambda n=n, files=files: jpeg.decode_batch(files[:n], dev, entropy="device", staging=staging)}
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
                    pool.shutdown()
                    for name, ts in times.items():
                        print(json.dumps(dict(figure="decode_batch", size=size, restart_interval=r, entropy=name, n=n, workers=workers,
                                              ms=round(statistics.median(ts) * 1e3, 3), min_ms=round(min(ts) * 1e3, 3), max_ms=round(max(ts) * 1e3, 3),
                                              rounds=args.rounds)), flush=True)

    if args.frames > 0:
        import video_demo

        with tempfile.TemporaryDirectory() as td:
            src = os.path.join(td, "in.avi")
            with MjpegAviWriter(src, 25) as w:
                for k in range(args.frames):
                    w.write(hd_files[k % 16])
            fps = {"host": [], "device": []}
            for _ in range(args.demo_rounds):
                for e in fps:
                    done = video_demo.main([src, CFG, "synthetic", "--out-video", os.path.join(td, f"out_{e}.avi"), "--decode", "device",
                                            "--decode-entropy", e])
                    fps[e].append(done["frames"] / done["seconds"])
            same = open(os.path.join(td, "out_host.avi"), "rb").read() == open(os.path.join(td, "out_device.avi"), "rb").read()
            for e, v in fps.items():
                print(json.dumps(dict(figure="video_demo", size="1920x1080", frames=args.frames, decode_entropy=e, frames_per_s=round(statistics.median(v), 1),
                                      min=round(min(v), 1), max=round(max(v), 1), rounds=args.demo_rounds, outputs_equal=same, sclk_mhz=shader_clock())),
                      flush=True)
    print(json.dumps(dict(figure="counters", fallbacks=jpeg.fallbacks, unsynchronised=jpeg.unsynchronised)), flush=True)


if __name__ == "__main__":
    main()
