"""Writes tests/golden/jpeg_cases.npz: the JPEG test grid encoded by Pillow (bundled libjpeg-turbo) and Pillow's own decode
of every file as RGB, plus two files the GPU decoder must refuse (progressive, CMYK). Data from Pillow, nothing from the reference project. The GPU tests read the file, so they do not
depend on the Pillow build of the machine they run on.

    python tests/golden/make_golden_jpeg.py

The grid: every size x sampling x quality, with the content class and the restart interval rotating so that each
(content, restart) pair meets every size, every sampling and every quality; one file more with optimised Huffman tables
and one with custom quantisation tables. The sizes are the smallest that reach a single partial MCU, odd chroma widths and
heights on both axes, the first / last-column rules of the upsampling and its edge-row replication; 5x3 and 6x4 have
chroma planes two samples wide, which libjpeg replicates instead of interpolating.
"""
import io
import os

import numpy as np

SIZES = [(1, 1), (1, 17), (17, 1), (5, 3), (6, 4), (8, 8), (9, 7), (16, 16), (17, 33), (33, 17), (37, 29), (31, 50), (48, 64)]  # H x W
SAMPLING = ["444", "422", "420", "grey"]
QUALITY = [1, 30, 75, 95, 100]
CONTENT = ["noise", "smooth", "bilevel"]
RESTART = [0, 1, 3]
_SUB = {"444": 0, "422": 1, "420": 2}


def content(kind: str, H: int, W: int, channels: int, rng) -> np.ndarray:
    if kind == "noise":
        a = rng.integers(0, 256, (H, W, channels))
    elif kind == "smooth":
        yy, xx = np.mgrid[0:H, 0:W]
        a = np.stack([(xx * (3 + c) + yy * (5 - c) + 40 * c) % 256 if c % 2 else 255 * (xx + yy) / max(1, H + W - 2) for c in range(channels)], axis=2)
        a = a + rng.integers(-3, 4, (H, W, channels))
    else:
        a = 255 * rng.integers(0, 2, (H, W, channels))
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(pixels: np.ndarray, sampling: str, quality: int, restart: int, **extra) -> bytes:
    from PIL import Image

    im = Image.fromarray(pixels[:, :, 0], "L") if sampling == "grey" else Image.fromarray(pixels, "RGB")
    kw = dict(quality=quality, restart_marker_blocks=restart, **extra)
    if sampling != "grey":
        kw["subsampling"] = _SUB[sampling]
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def grid():
    """Yields (name, jpeg bytes), deterministic."""
    i = 0
    for H, W in SIZES:
        for sampling in SAMPLING:
            for quality in QUALITY:
                kind, restart = CONTENT[i % 3], RESTART[(i // 3) % 3]
                rng = np.random.default_rng(1000 + i)
                px = content(kind, H, W, 1 if sampling == "grey" else 3, rng)
                yield f"{H}x{W}_{sampling}_q{quality}_{kind}_r{restart}", encode(px, sampling, quality, restart)
                i += 1
    rng = np.random.default_rng(7)
    yield "37x29_420_q75_smooth_optimize", encode(content("smooth", 37, 29, 3, rng), "420", 75, 0, optimize=True)
    qt = [[int(v) for v in rng.integers(1, 64, 64)], [int(v) for v in rng.integers(1, 128, 64)]]
    yield "31x50_422_noise_qtables", encode(content("noise", 31, 50, 3, rng), "422", 75, 0, qtables=qt)


def refused():
    """Yields (name, jpeg bytes) of files outside the GPU decoder's subset: the host decoder must take them."""
    from PIL import Image

    rng = np.random.default_rng(11)
    px = content("smooth", 24, 40, 3, rng)
    yield "progressive", encode(px, "420", 80, 0, progressive=True)
    buf = io.BytesIO()
    Image.fromarray(content("noise", 16, 24, 4, rng), "CMYK").save(buf, "JPEG", quality=80)
    yield "cmyk", buf.getvalue()


def truncations(data: bytes):
    """Damaged copies of a grid file: half of it, its last bytes of entropy data gone (with and without the EOI marker)."""
    return {"half": data[:len(data) // 2], "last_mcu": data[:-6], "last_mcu_eoi": data[:-6] + b"\xff\xd9"}


def pillow_rgb(data: bytes) -> np.ndarray:
    from PIL import Image

    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def main():
    from PIL import features

    assert features.check_feature("libjpeg_turbo"), "the golden pixels are libjpeg-turbo's"
    out = {}
    names = []
    for name, data in grid():
        names.append(name)
        out["jpg_" + name] = np.frombuffer(data, np.uint8)
        out["rgb_" + name] = pillow_rgb(data)
    out["names"] = np.array(names)
    out["refused_names"] = np.array([n for n, _ in refused()])
    for name, data in refused():
        out["refused_" + name] = np.frombuffer(data, np.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_cases.npz")
    np.savez_compressed(path, **out)
    print(f"{len(names)} files, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
