"""Times of the split JPEG encoder beside what writes a picture without it, on seeded photo-like frames (smooth fields, blobs,
mild noise) of 640x480 and 1920x1080 that lie on the device as a renderer leaves them, quality 75 and 4:2:0 (Pillow's
defaults), in ONE run with the paths alternated:

    (a) host_jpeg   device-to-host copy of the frames + Pillow ``save`` as JPEG (same quality and subsampling)
    (b) host_png    device-to-host copy + Pillow ``save`` as PNG
    (c) device      jpeg.encode_batch: two launches, one copy of the coefficients, Huffman coding on the threads

for n = 1 and n = 16 frames per call at 1 and 8 threads, in ms per call (median of --rounds alternations; all end with the
file bytes in host memory); then the forward call alone (its two launches) in device-event time, with the bytes it moves
computed from the shapes - pixels in, planes out and in, coefficients out - and their share of the 8 TB/s HBM peak, and the
shader clock read right behind the timed launches. One JSON line per figure.

    python scripts/bench_jpeg_encode.py [--rounds 7]"""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.bench_jpeg_decode import HBM_PEAK, photo_like  # noqa: E402


def shader_clock():
    """The current shader clock in MHz as rocm-smi prints it (read only), or None."""
    import re

    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30)
        for line in r.stdout.splitlines():
            m = re.search(r"\((\d+)Mhz\)", line)
            if "sclk" in line and m:
                return int(m.group(1))
    except Exception:  # noqa: BLE001
        pass
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()

    import torch
    from PIL import Image

    from probpose_code_amd import _lib, jpeg
    from probpose_code_amd.transforms import BatchStaging

    dev = torch.device("cuda:0")
    staging = BatchStaging()
    for W, H in ((640, 480), (1920, 1080)):
        rng = np.random.default_rng(W)
        host_frames = [photo_like(rng, H, W) for _ in range(4)]
        frames = [torch.from_numpy(host_frames[k % 4]).to(dev) for k in range(16)]
        size = f"{W}x{H}"
        # the two writers agree on the picture
        ours = jpeg.encode_batch(frames[:1], channel_order="rgb", staging=staging)[0]
        buf = io.BytesIO()
        Image.fromarray(host_frames[0]).save(buf, "JPEG", quality=75, subsampling=2)
        with Image.open(io.BytesIO(ours)) as a, Image.open(io.BytesIO(buf.getvalue())) as b:
            assert np.array_equal(np.asarray(a), np.asarray(b)), "encoders disagree"
        print(json.dumps(dict(figure="file", size=size, device_file_bytes=len(ours), pillow_file_bytes=len(buf.getvalue()))), flush=True)

        def pil_save(arr, fmt):
            b = io.BytesIO()
            if fmt == "JPEG":
                Image.fromarray(arr).save(b, "JPEG", quality=75, subsampling=2)
            else:
                Image.fromarray(arr).save(b, "PNG")
            return b.getvalue()

        for n in (1, 16):
            for threads in (1, 8):
                with ThreadPoolExecutor(max_workers=threads) as pool:
                    paths = {
                        "host_jpeg": lambda: list(pool.map(lambda a: pil_save(a, "JPEG"), [f.cpu().numpy() for f in frames[:n]])),
                        "host_png": lambda: list(pool.map(lambda a: pil_save(a, "PNG"), [f.cpu().numpy() for f in frames[:n]])),
                        "device": lambda: jpeg.encode_batch(frames[:n], channel_order="rgb", workers=threads, staging=staging),
                    }
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
            qt = jpeg.quality_tables(75)
            job = jpeg._stage_encode(frames[:n], qt, "4:2:0", "rgb", dev, staging)
            call_args, infos = job.args, job.infos
            stream = torch.cuda.current_stream(dev).cuda_stream
            for _ in range(3):
                _lib.call("pp_jpeg_forward_batch", *call_args, stream)
            torch.cuda.synchronize()
            us = []
            for _ in range(30):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.call("pp_jpeg_forward_batch", *call_args, stream)
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            sclk = shader_clock()  # right behind the timed launches
            moved = sum(3 * i.width * i.height + 2 * int(i.coef_count) + 2 * int(i.coef_count) for i in infos)  # pixels in, planes out + in, coefficients (int16) out
            med = statistics.median(us)
            print(json.dumps(dict(figure="forward_call", size=size, n=n, device_event_us=round(med, 1), min_us=round(min(us), 1), bytes_moved=int(moved), sclk_mhz=sclk,
                                  gb_per_s=round(moved / med / 1e3, 1), share_of_hbm_peak=round(moved / (med * 1e-6) / HBM_PEAK, 4))), flush=True)
            del job


if __name__ == "__main__":
    main()
