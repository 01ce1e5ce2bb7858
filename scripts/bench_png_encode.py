"""Times and file sizes of the device PNG writer beside what writes a ``.png`` without it, on seeded photo-like frames (smooth
fields, blobs, mild noise) of 640x480 and 1920x1080 and on one drawn demo frame, all lying on the device as a renderer
leaves them, in ONE run with the paths alternated:

    (a) host_png       device-to-host copy of the frames + Pillow ``save`` as PNG at its default level (the path without the switch)
    (b) host_png_l1    the same with ``compress_level=1``
    (c) device         png.encode_batch: eight launches, the histogram round trip, the used bytes of each stream

for n = 1 and n = 16 frames per call (the host paths at 1 and 8 threads), in ms per call (median of --rounds alternations;
all end with the file bytes in host memory); the file sizes of the three; then the eight launches alone (both C calls, the
codes of an earlier run in place) in device-event time, with the shader clock read right behind the timed launches. One JSON
line per figure.

``--match lz`` measures the ``lz`` match mode in place of the run coder; ``--match both`` alternates the two modes inside every
round of the same process (path "device" is runs, "device_lz" is lz; the files' sizes and the launches of both). With
``--parent-lib PATH`` (an earlier build of the library) the launches of that build are timed in the same alternation
(paths "parent_runs", "parent_lz"): its spread across the rounds (min_us .. max_us) is the yardstick for "did not move".

``--code device`` measures ``code="device"`` (the codes built by a ninth launch, no round trip) in place of the host build;
``--code both`` alternates the two inside every round: the write calls as paths "device" / "device_lz" (host build) and
"device_devcode" / "device_lz_devcode", and beside the two halves of the host build the nine launches of the device build
(tokens, code, deflate) in ONE event pair. ``--device-only`` leaves the Pillow paths out.

    python scripts/bench_png_encode.py [--rounds 7] [--match runs|lz|both] [--code host|device|both] [--parent-lib PATH] [--device-only]"""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.bench_jpeg_decode import photo_like  # noqa: E402
from scripts.bench_jpeg_encode import shader_clock  # noqa: E402


def drawn_demo_frame(dev):
    """The demo picture with two seeded poses drawn on it by the visualizer: (H, W, 3) uint8 RGB on the host."""
    from PIL import Image

    from probpose_code_amd.structures import InstanceData, PoseDataSample
    from probpose_code_amd.visualization import PoseLocalVisualizer

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with Image.open(os.path.join(root, "demo", "resources", "synthetic_person.png")) as im:
        rgb = np.asarray(im.convert("RGB"), dtype=np.uint8).copy()
    H, W = rgb.shape[:2]
    rng = np.random.default_rng(3)
    ds = PoseDataSample()
    ds.pred_instances = InstanceData(keypoints=(rng.random((2, 17, 2)) * [W, H]).astype(np.float32), keypoints_visible=np.ones((2, 17), np.float32),
                                     bboxes=np.array([[10, 10, W * 0.6, H * 0.9], [W * 0.3, 20, W - 10, H - 10]], np.float32))
    return PoseLocalVisualizer(device=str(dev)).draw_datasample(rgb, ds).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--match", default="runs", choices=["runs", "lz", "both"])
    ap.add_argument("--code", default="host", choices=["host", "device", "both"])
    ap.add_argument("--parent-lib", default=None, help="an earlier build of libprobpose_mi355x.so: its launches are timed beside this build's")
    ap.add_argument("--device-only", action="store_true", help="leave the Pillow paths out of the write calls")
    args = ap.parse_args()
    modes = ("runs", "lz") if args.match == "both" else (args.match,)
    codes = ("host", "device") if args.code == "both" else (args.code,)
    label = {"runs": "device", "lz": "device_lz"}
    suffix = {"host": "", "device": "_devcode"}

    import torch
    from PIL import Image

    from probpose_code_amd import png
    from probpose_code_amd.transforms import BatchStaging

    dev = torch.device("cuda:0")
    staging = BatchStaging()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        P = ctypes.c_void_p
        parent.pp_png_tokens_batch.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, P]
        parent.pp_png_deflate_batch.argtypes = [P, ctypes.c_int, ctypes.c_longlong, P]
        parent.pp_png_tokens_batch_lz.argtypes = parent.pp_png_tokens_batch.argtypes
        parent.pp_png_deflate_batch_lz.argtypes = parent.pp_png_deflate_batch.argtypes

    def pil_save(arr, level):
        b = io.BytesIO()
        Image.fromarray(arr).save(b, "PNG", **({} if level is None else dict(compress_level=level)))
        return b.getvalue()

    sets = []
    for W, H in ((640, 480), (1920, 1080)):
        rng = np.random.default_rng(W)
        sets.append((f"{W}x{H}", [photo_like(rng, H, W) for _ in range(4)]))
    demo = drawn_demo_frame(dev)
    sets.append((f"demo {demo.shape[1]}x{demo.shape[0]}", [demo]))
    for size, host_frames in sets:
        frames = [torch.from_numpy(host_frames[k % len(host_frames)]).to(dev) for k in range(16)]
        default, level1 = len(pil_save(host_frames[0], None)), len(pil_save(host_frames[0], 1))
        for m in modes:
            ours = png.encode_batch(frames[:1], channel_order="rgb", staging=staging, match=m)[0]
            assert all(png.encode_batch(frames[:1], channel_order="rgb", staging=staging, match=m, code=c)[0] == ours for c in codes), "code= changes the file"
            with Image.open(io.BytesIO(ours)) as a:
                assert np.array_equal(np.asarray(a), host_frames[0]), "the file does not hold the pixels"
            print(json.dumps(dict(figure="file", size=size, match=m, device_file_bytes=len(ours), pillow_default_bytes=default,
                                  pillow_level1_bytes=level1, raw_bytes=int(host_frames[0].size), over_default=round(len(ours) / default, 3),
                                  over_level1=round(len(ours) / level1, 3))), flush=True)
        for n in (1, 16):
            for threads in ((1,) if n == 1 else (1, 8)):
                with ThreadPoolExecutor(max_workers=threads) as pool:
                    paths = {} if args.device_only else {
                        "host_png": lambda: list(pool.map(lambda a: pil_save(a, None), [f.cpu().numpy() for f in frames[:n]])),
                        "host_png_l1": lambda: list(pool.map(lambda a: pil_save(a, 1), [f.cpu().numpy() for f in frames[:n]])),
                    }
                    if args.device_only and threads > 1:
                        continue  # (the threads are the host paths')
                    for m in modes:
                        for c in codes:
                            paths[label[m] + suffix[c]] = lambda m=m, c=c: png.encode_batch(frames[:n], channel_order="rgb", staging=staging, match=m, code=c)
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
                for name, ts in times.items():
                    print(json.dumps(dict(figure="write_call", size=size, path=name, n=n, threads=threads, ms=round(statistics.median(ts) * 1e3, 3),
                                          min_ms=round(min(ts) * 1e3, 3), max_ms=round(max(ts) * 1e3, 3), rounds=args.rounds)), flush=True)
        for n in (1, 16):
            stream = torch.cuda.current_stream(dev)
            jobs = {m: png._stage(frames[:n], None, 1, dev, staging, m == "lz") for m in modes}
            for job in jobs.values():
                png._run(job)  # (leaves the codes of these frames on the device: the timed launches below need no host in between)
            halves, nine = {}, {}
            for m, j in jobs.items():
                if "host" in codes:
                    halves[label[m]] = ((lambda j=j: png._launch_tokens(j, stream)), (lambda j=j: png._launch_deflate(j, stream)))
                if "device" in codes:  # tokens, code, deflate with nothing between them: one event pair
                    nine[label[m] + "_devcode"] = lambda j=j: (png._launch_tokens(j, stream), png._launch_code(j, stream), png._launch_deflate(j, stream))
                if parent is not None:
                    lz = "_lz" if m == "lz" else ""
                    halves["parent_" + m] = (
                        lambda j=j, f=getattr(parent, "pp_png_tokens_batch" + lz): f(j.block.base, len(j.lens), j.max_height, max(j.lens), stream.cuda_stream),
                        lambda j=j, f=getattr(parent, "pp_png_deflate_batch" + lz): f(j.block.base, len(j.lens), max(j.lens), stream.cuda_stream))
            us = {k: {"both": [], "tokens": [], "deflate": []} for k in list(halves) + list(nine)}
            for _ in range(3 + args.rounds):
                for k, (tokens, deflate) in halves.items():  # the modes (and builds) alternate inside a round
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    e[0].record()
                    tokens()
                    e[1].record()
                    deflate()
                    e[2].record()
                    e[2].synchronize()
                    us[k]["tokens"].append(e[0].elapsed_time(e[1]) * 1e3)
                    us[k]["deflate"].append(e[1].elapsed_time(e[2]) * 1e3)
                    us[k]["both"].append(e[0].elapsed_time(e[2]) * 1e3)
                for k, all_nine in nine.items():
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    e[0].record()
                    all_nine()
                    e[1].record()
                    e[1].synchronize()
                    us[k]["both"].append(e[0].elapsed_time(e[1]) * 1e3)
            sclk = shader_clock()  # right behind the timed launches
            for k, u in us.items():
                split = dict(tokens_us=round(statistics.median(u["tokens"][3:]), 1), deflate_us=round(statistics.median(u["deflate"][3:]), 1)) if k in halves else {}
                print(json.dumps(dict(figure="launches", size=size, path=k, n=n, device_event_us=round(statistics.median(u["both"][3:]), 1), **split,
                                      min_us=round(min(u["both"][3:]), 1), max_us=round(max(u["both"][3:]), 1),
                                      stream_bytes=int(sum(next(iter(jobs.values())).lens)), sclk_mhz=sclk, rounds=args.rounds)), flush=True)
            del jobs, halves, nine


if __name__ == "__main__":
    main()
