"""The inputs the device Huffman decoder's tests share (tests/test_jpeg_huffdec_references.py, _host.py, _gpu.py): the corpus
without restart intervals, the named slow-synchronising stream, and searches for files in which the true decoder meets a
given boundary situation (tests/jpeg_huffdec_ref.situations names them). Everything is made once and cached; do not modify
what these functions return."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import jpeg_huffdec_ref as R  # noqa: E402
import jpeg_ref as J  # noqa: E402
import jpeg_sources as S  # noqa: E402
from make_golden_jpeg import content, encode  # noqa: E402

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def corpus():
    """name -> bytes: the committed grid's files without a restart interval (Pillow's annex K tables, one with optimised tables,
    one with custom quantisation tables)."""
    g = J.golden()
    return {n: g["jpg"][n] for n in g["names"] if n.endswith(("_r0", "optimize", "qtables"))}


def prepared(data: bytes) -> dict:
    return _once(("prepared", data), lambda: R.prepare(data))


def reference(data: bytes, passes: int = R.DEFAULT_PASSES) -> dict:
    """jpeg_huffdec_ref.decode of a file, computed once per setting."""
    return _once(("decoded", data, passes), lambda: R.decode(prepared(data), passes))


def photo(H: int, W: int, seed: int) -> np.ndarray:
    """A photo-like picture: a smooth field plus noise of sigma 6."""
    rng = np.random.default_rng([H, W, seed])
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a = np.stack([128 + 90 * np.sin(xx / (17.0 + 5 * c) + seed) * np.cos(yy / (23.0 - 4 * c)) for c in range(3)], axis=2)
    return np.clip(a + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8)


SLOW_NAME = "noise_160x208_420_q95"


def slow_stream() -> bytes:
    """The named slow-synchronising stream: uniform noise, 4:2:0, quality 95 - a synchronisation distance of several KB - and
    longer than one workgroup's 32 KiB of subsequences, so a state has to cross a workgroup border."""
    return _once("slow", lambda: encode(content("noise", 160, 208, 3, np.random.default_rng(95)), "420", 95, 0))


def find(situation: str, sampling: str = "420", H: int = 24, W: int = 40, tries: int = 400, **extra) -> bytes:
    """A small Pillow file in which the true decoder meets ``situation``: quality and content seed vary until the reference
    finds it. AssertionError if none of ``tries`` files does."""
    def make():
        for t in range(tries):
            kind = ("noise", "smooth", "bilevel")[t % 3]
            data = encode(content(kind, H, W, 1 if sampling == "grey" else 3, np.random.default_rng([t, H, W])), sampling,
                          (95, 75, 100, 50, 88, 30, 98)[t % 7], 0, **extra)
            if situation in R.situations(R.prepare(data)):
                return data
        raise AssertionError(f"no file with {situation} in {tries} tries")

    return _once(("find", situation, sampling, H, W, tuple(sorted(extra.items()))), make)


def find_length(length: int, tries: int = 4000) -> bytes:
    """A small grey Pillow file whose entropy-coded segment is exactly ``length`` bytes."""
    def make():
        for t in range(tries):
            H, W = 8 * (1 + t % 3), 8 * (1 + (t // 3) % 4)
            rng = np.random.default_rng([t, length])
            data = encode(content(("noise", "smooth")[t % 2], H, W, 1, rng), "grey", int(rng.integers(20, 101)), 0)
            if len(R.prepare(data)["stream"]) == length:
                return data
        raise AssertionError(f"no file with a segment of {length} bytes in {tries} tries")

    return _once(("length", length), make)
