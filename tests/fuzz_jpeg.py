#!/usr/bin/env python
"""Differential fuzz of the split JPEG decoder (csrc/pp_jpeg_host.h + csrc/pp_jpeg.hip) against tests/jpeg_ref.py (the numpy
restatement of libjpeg's integer rules): random sizes of 1..700 a side, biased to the widths where jpeg_color_kernel starts
another workgroup column (256 / 257, 512 / 513) and to multiples of 8 and 16 plus or minus 1; random sampling, quality, content
and stream layout (Pillow's own file, or its coefficients rewritten by tests/jpeg_write.py with random tables, slots, segments,
fill bytes and restart interval); batches of 1..16 images through the guarded call of tests/jpeg_harness.py (canaries around
every image and the scratch, two calls compared, launches counted). No file may take the host fallback; every image equals
the reference byte for byte. A mismatch prints its seed and leaves the file in the temp dir.
python tests/fuzz_jpeg.py [seconds]"""
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import jpeg_ref as J  # noqa: E402
import jpeg_write as JW  # noqa: E402
from jpeg_harness import raw_reconstruct  # noqa: E402
from make_golden_jpeg import content, encode  # noqa: E402
from probpose_code_amd import jpeg  # noqa: E402

SIDE_MAX = 700
BATCH_PIXELS = 150_000  # the reference parses a file bit by bit in Python: so many pixels a batch, then only small images


def draw_side(rng) -> int:
    kind = rng.random()
    if kind < 0.25:
        v = int(rng.choice([256, 257, 512, 513]))
    elif kind < 0.6:
        v = int(rng.choice([8, 16])) * int(rng.integers(1, SIDE_MAX // 8 + 1)) + int(rng.integers(-1, 2))
    else:
        v = int(rng.integers(1, SIDE_MAX + 1))
    return min(max(v, 1), SIDE_MAX)


def draw_layout(rng, ncomp: int) -> dict:
    slots = lambda: tuple(int(v) for v in rng.integers(0, 4, 2)[[0, 1, 1]])  # noqa: E731
    shared = rng.random() < 0.3
    dc, ac = slots(), slots()
    if shared:
        dc, ac = (dc[0],) * 3, (ac[0],) * 3
    ids = [(1, 2, 3), (0, 1, 2), (82, 71, 66), tuple(int(v) for v in rng.choice(256, 3, replace=False))][int(rng.integers(0, 4))]
    jfif = bool(rng.random() < 0.6) or ids == (82, 71, 66)  # (R, G, B without JFIF is on the refusal list)
    extra = tuple(k for k in ("com", "app1", "app2") if rng.random() < 0.3)
    return dict(restart=int(rng.choice([0, 0, 1, 2, 3, 5, 7, 8, 64, 65535, int(rng.integers(1, 65536))])),
                huffman="fibonacci" if rng.random() < 0.3 else "optimal", dc_slots=dc, ac_slots=ac, q_slots=tuple(int(v) for v in rng.choice(4, 2, replace=False)[[0, 1, 1]]),
                dqt_split=bool(rng.random() < 0.5), dht_split=bool(rng.random() < 0.5), pq=int(rng.random() < 0.3),
                sof=0xC1 if rng.random() < 0.3 else 0xC0, comp_ids=ids, fill=int(rng.choice([0, 0, 1, 2, 5])), jfif=jfif,
                adobe=1 if rng.random() < 0.2 else None, extra=extra)


def draw_file(rng, budget: int):
    """(description, file bytes) of one random case of at most ``budget`` pixels."""
    H, W = draw_side(rng), draw_side(rng)
    if H * W > budget:  # keep one side, shorten the other
        if rng.random() < 0.5:
            H = max(1, min(H, budget // W))
        else:
            W = max(1, min(W, budget // H))
        if H * W > budget:
            H, W = max(1, min(H, 64)), max(1, min(W, 64))
    sampling = ["420", "422", "444", "grey"][int(rng.integers(0, 4))]
    quality = int(rng.choice([1, 30, 75, 90, 95, 100, int(rng.integers(1, 101))]))
    kind = ["noise", "smooth", "bilevel"][int(rng.integers(0, 3))]
    restart = int(rng.choice([0, 0, 1, 3, 11]))
    px = content(kind, H, W, 1 if sampling == "grey" else 3, rng)
    optimize = bool(rng.random() < 0.3)
    try:
        data = encode(px, sampling, quality, restart, **(dict(optimize=True) if optimize else {}))
    except OSError:  # Pillow's output buffer is too small for some optimised files of noise at high quality
        data, optimize = encode(px, sampling, quality, restart), False
    what = f"{H}x{W} {sampling} q{quality} {kind} r{restart}{' optimize' if optimize else ''}"
    if rng.random() < 0.6:
        layout = draw_layout(rng, 1 if sampling == "grey" else 3)
        data = JW.write(J.parse(data), **layout)
        what += f" {layout}"
    return what, data, H, W


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    n, bad, seed, pixels = 0, 0, 0, 0
    t_end = time.time() + seconds
    while time.time() < t_end:
        rng = np.random.default_rng(77000 + seed)
        seed += 1
        budget, cases = BATCH_PIXELS, []
        for _ in range(int(rng.integers(1, 17))):
            what, data, H, W = draw_file(rng, max(budget, 4096))
            budget = max(0, budget - H * W)
            cases.append((what, data, (H, W, 3)))
        problems = []
        try:
            coefs = []
            for what, data, shape in cases:
                info = jpeg.probe(data)
                assert info.supported == 1, f"refused ({info.reason.decode()}): {what}"
                coefs.append(jpeg.entropy_decode(data))
            images = raw_reconstruct(jpeg, coefs)
            for i, ((what, data, shape), img) in enumerate(zip(cases, images)):
                ref = J.decode_rgb(data)[:, :, ::-1]
                if img.shape != shape or ref.shape != shape or not np.array_equal(img, ref):
                    wrong = int((img != ref).any(axis=2).sum()) if img.shape == ref.shape else -1
                    problems.append((i, f"{wrong} of {shape[0] * shape[1]} pixels differ: {what}"))
        except (AssertionError, jpeg.JpegUnsupported) as e:
            problems.append((None, str(e)))
        n += len(cases)
        pixels += sum(s[0] * s[1] for _, _, s in cases)
        for i, text in problems:
            bad += 1
            keep = cases if i is None else [cases[i]]
            paths = []
            for k, (_, data, _) in enumerate(keep):
                paths.append(os.path.join(tempfile.gettempdir(), f"fuzz_jpeg_seed{seed - 1}_{k if i is None else i}.jpg"))
                with open(paths[-1], "wb") as f:
                    f.write(data)
            print(f"MISMATCH seed {seed - 1} batch of {len(cases)}: {text} -> {paths[0] if len(paths) == 1 else os.path.dirname(paths[0])}", flush=True)
    print(f"{n} images ({pixels} pixels) in {seed} batches in {seconds:.0f} s, {bad} mismatches, {jpeg.fallbacks} fallbacks")
    print("JPEG FUZZ", "FAILED" if bad or jpeg.fallbacks or n == 0 else "OK")
    return 1 if bad or jpeg.fallbacks or n == 0 else 0


if __name__ == "__main__":
    sys.exit(main())
