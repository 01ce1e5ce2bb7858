"""Rates of the split JPEG decoder beside the host decoder, on seeded photo-like 4:2:0 quality-90 files (smooth fields, blobs,
mild noise) of 640x480 and 1920x1080, in ONE run with the two paths alternated:

    (a) host      apis.load_image_bgr on the threads + the upload of the pixels
    (b) device    jpeg.entropy_decode on the same threads + jpeg.reconstruct_batch (16 images per call)

at 1 and 8 threads, in images/s (median of --rounds alternations; both end with the pixels on the device); then the
reconstruct call alone (its two launches, no upload) in device-event time at n = 1 and n = 16, with the bytes it moves
computed from the shapes - coefficients in, planes out and in, pixels out - and their share of the 8 TB/s HBM peak.
One JSON line per figure.

    python scripts/bench_jpeg_decode.py [--images 64] [--rounds 5]"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK = 8.0e12  # bytes/s, MI355X specification


def photo_like(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.zeros((H, W, 3), np.float32)
    for c in range(3):
        img[:, :, c] = 128 + 50 * np.sin(xx / rng.uniform(60, 300) + rng.uniform(0, 6)) + 40 * np.cos(yy / rng.uniform(60, 300) + rng.uniform(0, 6))
    for _ in range(12):  # blobs
        cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0.03, 0.15) * W
        img += (rng.uniform(-70, 70, 3) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * r * r))[:, :, None]).astype(np.float32)
    img += rng.normal(0, 4, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64, help="640x480 files (a quarter as many 1920x1080 ones)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import torch
    from PIL import Image

    from probpose_code_amd import _lib, apis, jpeg
    from probpose_code_amd.transforms import BatchStaging

    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="pp_bench_jpeg_")
    staging = BatchStaging()
    for (W, H), count in (((640, 480), args.images), ((1920, 1080), max(16, args.images // 4))):
        rng = np.random.default_rng(W)
        paths = []
        for k in range(count):
            buf = io.BytesIO()
            Image.fromarray(photo_like(rng, H, W)).save(buf, "JPEG", quality=90, subsampling=2)
            paths.append(os.path.join(tmp, f"{W}x{H}_{k:04d}.jpg"))
            with open(paths[-1], "wb") as f:
                f.write(buf.getvalue())
        size = f"{W}x{H}"
        print(json.dumps(dict(figure="files", size=size, count=count, mean_file_bytes=round(sum(os.path.getsize(p) for p in paths) / count))), flush=True)
        first = jpeg.entropy_decode(paths[0])
        assert torch.equal(jpeg.reconstruct_batch([first], dev, staging)[0].cpu(), torch.from_numpy(apis.load_image_bgr(paths[0]))), "decoders disagree"

        def host(pool):
            return [torch.from_numpy(a).to(dev, non_blocking=False) for a in pool.map(apis.load_image_bgr, paths)]

        def device(pool):
            futures = [pool.submit(jpeg.entropy_decode, p) for p in paths]
            out = []
            for lo in range(0, len(futures), 16):
                out += jpeg.reconstruct_batch([f.result() for f in futures[lo:lo + 16]], dev, staging)
            return out

        for threads in (1, 8):
            with ThreadPoolExecutor(max_workers=threads) as pool:
                times = {"host": [], "device": []}
                host(pool), device(pool)  # warm-up
                for _ in range(args.rounds):
                    for name, fn in (("host", host), ("device", device)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn(pool)
                        torch.cuda.synchronize()
                        times[name].append(time.perf_counter() - t0)
                with ThreadPoolExecutor(max_workers=threads) as p2:  # the Huffman half alone, no device work
                    t0 = time.perf_counter()
                    list(p2.map(jpeg.entropy_decode, paths))
                    t_entropy = time.perf_counter() - t0
            for name in ("host", "device"):
                ts = times[name]
                print(json.dumps(dict(figure="decode_rate", size=size, path=name, threads=threads, images_per_s=round(count / statistics.median(ts), 1),
                                      min=round(count / max(ts), 1), max=round(count / min(ts), 1), rounds=args.rounds)), flush=True)
            print(json.dumps(dict(figure="entropy_decode_only", size=size, threads=threads, images_per_s=round(count / t_entropy, 1))), flush=True)

        coefs = [jpeg.entropy_decode(p) for p in paths[:16]]
        for n in (1, 16):
            job = jpeg._stage(coefs[:n], dev, staging, None, None)
            call_args = job.args
            stream = torch.cuda.current_stream(dev).cuda_stream
            for _ in range(3):
                _lib.call("pp_jpeg_reconstruct_bgr_batch", *call_args, stream)
            torch.cuda.synchronize()
            us = []
            for _ in range(30):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.call("pp_jpeg_reconstruct_bgr_batch", *call_args, stream)
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            moved = sum(2 * c.coef.size + 2 * c.coef.size + 3 * c.info.width * c.info.height for c in coefs[:n])  # coefficients (int16) in, planes out + in, pixels out
            med = statistics.median(us)
            print(json.dumps(dict(figure="reconstruct_call", size=size, n=n, device_event_us=round(med, 1), min_us=round(min(us), 1), bytes_moved=int(moved),
                                  gb_per_s=round(moved / med / 1e3, 1), share_of_hbm_peak=round(moved / (med * 1e-6) / HBM_PEAK, 4))), flush=True)
            del job


if __name__ == "__main__":
    main()
