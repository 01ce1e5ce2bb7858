"""What the PNG writer's format prescribes, restated without the library: the five row filters with the choice rule in
numpy, and a walk over the bytes of a stream that counts the tokens of the run rule. Beside them the pictures and the raw
streams both test files (tests/test_png_host.py, tests/test_png_gpu.py) code, computed once and shared (do not modify)."""
import os

import numpy as np

TILE = 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def filter_rows(rgb: np.ndarray):
    """(H, W, 3) uint8 RGB -> (the filtered stream as bytes, the filter type of every row, the rows whose smallest cost is
    shared by several filters). bpp = 3; what lies above or left of the picture is 0; the smallest sum of min(b, 256 - b)
    wins, the lowest number on a tie."""
    H, W, _ = rgb.shape
    x = rgb.reshape(H, 3 * W).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255  # (5, H, 3W)
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)  # (5, H)
    types = cost.argmin(axis=0)  # (the first of equal minima: the lowest number)
    ties = np.flatnonzero((cost == cost.min(axis=0)).sum(axis=0) > 1)
    rows = np.empty((H, 1 + 3 * W), np.uint8)
    rows[:, 0] = types
    rows[:, 1:] = cand[types, np.arange(H)]
    return rows.tobytes(), types, ties


def emission(k: int, L: int):
    """What byte k of a run of length L emits: None, "lit" or a match length."""
    if k == 0:
        return "lit"
    j = k - 1
    g = j // 258
    m = min(258, L - 1 - 258 * g)
    if m < 3:
        return "lit"
    return m if j % 258 == 0 else None


def tokens(stream: bytes):
    """(literals, the list of match lengths) of a stream: tiles of TILE bytes, runs that end at their borders, byte by byte."""
    lits, matches = 0, []
    for t0 in range(0, len(stream), TILE):
        tile = stream[t0:t0 + TILE]
        p = 0
        while p < len(tile):
            q = p
            while q + 1 < len(tile) and tile[q + 1] == tile[p]:
                q += 1
            for k in range(q - p + 1):
                e = emission(k, q - p + 1)
                if e == "lit":
                    lits += 1
                elif e is not None:
                    matches.append(e)
            p = q + 1
    return lits, matches


_PICTURES, _STREAMS = {}, {}


def pictures():
    """{name: (H, W, 3) uint8 RGB}: the sizes and contents the issue lists, and two ramps that make Average and Paeth win."""
    if not _PICTURES:
        from PIL import Image

        rng = np.random.default_rng(11)
        yy, xx = np.mgrid[0:201, 0:150]
        photo = 128 + 70 * np.sin(xx / 23.0) * np.cos(yy / 31.0) + 30 * np.sin((xx + 2 * yy) / 7.0)
        photo = np.clip(photo[:, :, None] + np.array([0, 12, -9]) + rng.normal(0, 3, (201, 150, 3)), 0, 255).astype(np.uint8)
        y32, x32 = np.mgrid[0:40, 0:40]
        with Image.open(os.path.join(ROOT, "demo", "resources", "synthetic_person.png")) as im:
            demo = np.asarray(im.convert("RGB"), dtype=np.uint8)
        p = {
            "1x1": np.array([[[7, 200, 31]]], np.uint8),
            "1x7": rng.integers(0, 256, (1, 7, 3), dtype=np.uint8),
            "7x1": rng.integers(0, 256, (7, 1, 3), dtype=np.uint8),
            "photo 150x201": photo,
            "noise row bytes 4096": rng.integers(0, 256, (3, 1365, 3), dtype=np.uint8),
            "flat row bytes 4099": np.full((3, 1366, 3), 90, np.uint8),
            "zeros": np.zeros((37, 53, 3), np.uint8),
            "all 255": np.full((37, 53, 3), 255, np.uint8),
            "noise": rng.integers(0, 256, (61, 45, 3), dtype=np.uint8),
            "horizontal ramp": np.repeat(np.tile((np.arange(200) % 256).astype(np.uint8)[None, :, None], (9, 1, 1)), 3, axis=2),
            "vertical ramp": np.repeat(np.tile((np.arange(200) % 256).astype(np.uint8)[:, None, None], (1, 9, 1)), 3, axis=2),
            "ramp down-left": np.repeat((128 + 3 * x32 - 3 * y32)[:, :, None].astype(np.uint8), 3, axis=2),
            "ramp down-right": np.repeat((2 * x32 + 2 * y32)[:, :, None].astype(np.uint8), 3, axis=2),
            "demo picture": demo,
        }
        for v in p.values():
            v.setflags(write=False)
        _PICTURES.update(p)
    return _PICTURES


def _runs(lengths, lead=0):
    out = bytearray((7 * i + 1) & 255 for i in range(lead))
    v = 200
    for n in lengths:
        out += bytes([v]) * n
        v = (v + 13) & 255
    return bytes(out)


def streams():
    """{name: bytes}: the raw streams of the deflate stage's tests."""
    if not _STREAMS:
        rng = np.random.default_rng(5)
        every = bytearray(range(256))
        for m in range(3, 259):  # a run of 1 + m bytes: every match length, so every length symbol
            if len(every) % TILE + m + 2 > TILE:  # (a run that would cross a tile border begins behind it)
                every += bytes(1 + (i & 1) for i in range(TILE - len(every) % TILE))
            every += bytes([(5 * m) & 255]) * (m + 1) + bytes([(5 * m + 1) & 255])
        _STREAMS.update({
            "runs 1 2 3 4": _runs([1, 2, 3, 4]),
            "runs 258 .. 262": _runs([258, 259, 260, 261, 262]),
            "runs 517 .. 520": _runs([517, 518, 519, 520]),
            "run 4096": _runs([4096]),
            "run across a tile border": _runs([600], lead=3800),
            "one byte": b"\x2a",
            "one value": bytes(10000),
            "every value and length": bytes(every),
            "noise 8193": rng.integers(0, 256, 8193, dtype=np.uint8).tobytes(),
            "sparse 70000": np.where(rng.random(70000) < 0.06, rng.integers(0, 256, 70000), 0).astype(np.uint8).tobytes(),
        })
    return _STREAMS
