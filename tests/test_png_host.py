"""CPU: the host form of the PNG writer (``png.encode_host``, ``png.zlib_compress_host``, ``pp_deflate_build_code``) - the
sequential run of the core the kernels share (csrc/pp_png_core.h) - judged by decoders and by the restatement in
tests/png_ref.py: Pillow opens every file to the pixels, every chunk's CRC is ``zlib.crc32``'s, ``zlib.decompress`` of the
IDAT chunk is the restated filtered stream byte for byte, the raw streams inflate to themselves with the restated number of
tokens, and the code builder keeps its lengths at 15 bits with a Kraft sum of exactly 1. No GPU is used."""
import ctypes
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import png_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def png(lib_built):
    from probpose_code_amd import png

    return png


_FILES = {}


def host_file(png, name):
    """``encode_host`` of picture ``name`` (RGB order), computed once."""
    if name not in _FILES:
        _FILES[name] = png.encode_host(R.pictures()[name], channel_order="rgb")
    return _FILES[name]


def chunks(data: bytes):
    """[(type, payload)] of a PNG file; asserts the signature, the framing and every CRC."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        payload = data[at + 8:at + 8 + n]
        assert len(payload) == n
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + payload) & 0xFFFFFFFF, kind
        out.append((kind, payload))
        at += 12 + n
    assert at == len(data)
    return out


def check_file(png, data: bytes, rgb: np.ndarray):
    """What every file of the writer owes: framing, CRCs, the restated filtered stream inside, Pillow's pixels, the bound."""
    from PIL import Image

    H, W, _ = rgb.shape
    parts = chunks(data)
    assert [k for k, _ in parts] == [b"IHDR", b"IDAT", b"IEND"]
    assert parts[0][1] == struct.pack(">II5B", W, H, 8, 2, 0, 0, 0) and parts[2][1] == b""
    stream = parts[1][1]
    assert stream[:2] == b"\x78\x01"
    assert zlib.decompress(stream) == R.filter_rows(rgb)[0]
    with Image.open(io.BytesIO(data)) as im:
        assert (im.format, im.mode, im.size) == ("PNG", "RGB", (W, H))
        assert np.array_equal(np.asarray(im), rgb)
    bound = int(png._lib.lib.pp_png_encoded_bound(W, H))
    assert bound > H * W * 3 and len(data) <= bound  # (noise does not compress: the bound must lie above the raw size)


@pytest.mark.parametrize("name", list(R.pictures()))
def test_host_files_open_everywhere_and_hold_the_restated_stream(png, name):
    check_file(png, host_file(png, name), R.pictures()[name])


def test_channel_orders_give_the_same_file(png):
    rgb = R.pictures()["photo 150x201"]
    assert png.encode_host(np.ascontiguousarray(rgb[:, :, ::-1]), channel_order="bgr") == host_file(png, "photo 150x201")
    assert png.encode_host(rgb[:, :, ::-1]) == host_file(png, "photo 150x201")  # a view with negative strides; "bgr" is the default


def test_every_filter_is_chosen_and_a_tie_goes_to_the_lower_number(png):
    chosen, tied = set(), []
    for name, rgb in R.pictures().items():
        want, types, ties = R.filter_rows(rgb)
        got = zlib.decompress(chunks(host_file(png, name))[1][1])
        rows = np.frombuffer(got, np.uint8).reshape(rgb.shape[0], -1)
        assert np.array_equal(rows[:, 0], types), name
        chosen |= set(int(t) for t in types)
        tied += [(name, int(r), int(types[r])) for r in ties]
    assert chosen == {0, 1, 2, 3, 4}, chosen
    assert ("zeros", 0, 0) in tied  # every cost 0: None
    assert ("all 255", 1, 2) in tied  # under a row of the same value Up and Paeth both predict exactly: Up


def test_noise_has_no_match_and_a_flat_picture_has_them(png):
    assert R.tokens(R.filter_rows(R.pictures()["noise"])[0])[1] == []
    assert 258 in R.tokens(R.filter_rows(R.pictures()["zeros"])[0])[1]


@pytest.mark.parametrize("name", list(R.streams()))
def test_deflate_stage_on_raw_streams(png, name):
    raw = R.streams()[name]
    z, count = png.zlib_compress_host(raw, return_tokens=True)
    assert zlib.decompress(z) == raw
    lits, matches = R.tokens(raw)
    assert count == lits + len(matches)
    assert len(z) <= int(png._lib.lib.pp_deflate_bound(len(raw)))
    if name == "every value and length":
        assert set(matches) == set(range(3, 259)) and len(set(raw)) == 256
    if name == "run across a tile border":
        assert matches == [258, 37, 258, 45]  # 296 bytes of the run end the first tile, 304 begin the second


def _code(png, hist):
    h = np.zeros(288, np.uint32)
    h[:len(hist)] = hist
    code = np.zeros(png.CODE_BYTES // 4, np.uint32)
    png._lib.call("pp_deflate_build_code", h.ctypes.data, code.ctypes.data)
    return code


def _fibonacci():
    h = np.zeros(286, np.uint32)
    a, b = 1, 1
    for s in range(40):
        h[s] = a
        a, b = b, a + b
    return h


HISTOGRAMS = {
    "Fibonacci counts": _fibonacci(),
    "two symbols": np.bincount([65] * 9 + [256], minlength=286),
    "all equal": np.full(286, 77),
    "no match": np.concatenate([1 + np.random.default_rng(2).integers(0, 1000, 256), [1], np.zeros(29, np.int64)]),
}


@pytest.mark.parametrize("name", list(HISTOGRAMS))
def test_code_builder_keeps_15_bits_and_a_complete_code(png, name):
    hist = HISTOGRAMS[name]
    code = _code(png, hist)
    sym, header_bits, header = code[:288], int(code[288]), code[292:]
    lengths = (sym >> 16).astype(np.int64)
    assert lengths.max() <= 15 and (lengths[286:] == 0).all()
    assert all(lengths[s] > 0 for s in range(286) if hist[s] or s == 256)
    assert sum(2 ** (15 - int(n)) for n in lengths if n) == 2 ** 15  # Kraft: exactly 1
    if name == "Fibonacci counts":
        assert lengths.max() == 15  # Huffman's own tree is 39 deep
    assert np.array_equal(code, _code(png, hist))
    # the header inflates: behind it the end-of-block code, the padding and the Adler-32 of nothing
    bits = int.from_bytes(header.astype("<u4").tobytes(), "little") | (int(sym[256]) & 0xFFFF) << header_bits
    nbits = header_bits + int(lengths[256])
    assert zlib.decompress(bits.to_bytes((nbits + 7) // 8, "little") + b"\x00\x00\x00\x01") == b""


def test_refusals_leave_the_counters_untouched(png):
    import torch

    from probpose_code_amd.visualization import PoseLocalVisualizer

    good = np.zeros((8, 8, 3), np.uint8)
    before = (png.host_calls, png.tokens_calls, png.deflate_calls)
    png._lib.reset_launch_counts()
    for bad in (np.zeros((8, 8, 3), np.float32), np.zeros((8, 8), np.uint8), np.zeros((8, 8, 4), np.uint8), np.zeros((0, 8, 3), np.uint8),
                torch.zeros((8, 8, 3), dtype=torch.int8), [[1, 2, 3]]):
        with pytest.raises(ValueError):
            png.encode_host(bad)
        with pytest.raises(ValueError):
            png.encode_batch([good, bad])
    for call in (png.encode_host, lambda im, **kw: png.encode_batch([im], **kw)):
        with pytest.raises(ValueError, match="channel_order"):
            call(good, channel_order="xyz")
    with pytest.raises(ValueError):
        png.encode_batch(good)  # one picture is no sequence of pictures
    with pytest.raises(ValueError):
        png.zlib_compress_device([b"abc", b""])
    with pytest.raises(ValueError, match="png_encoder"):
        PoseLocalVisualizer(png_encoder="gpu")
    assert (png.host_calls, png.tokens_calls, png.deflate_calls) == before
    assert png._lib.launch_count("pp_png.hip") == 0
    lib = png._lib.lib
    assert lib.pp_png_encoded_bound(65536, 1) < 0 and lib.pp_png_encoded_bound(0, 1) < 0
    assert lib.pp_png_encoded_bound(65535, 65535) < 0  # a stream bound of 2^31 bytes or more
    assert lib.pp_deflate_bound(0) < 0 and lib.pp_deflate_scratch_bytes(0) < 0
    size = ctypes.c_size_t(0)
    assert lib.pp_png_encode(good.ctypes.data, 8, 8, 23, 1, good.ctypes.data, 0, ctypes.byref(size)) == png._lib.PP_ERR_INVALID_ARG
    assert lib.pp_png_tokens_batch(None, 1, 0, 16, None) == png._lib.PP_ERR_INVALID_ARG
    assert lib.pp_png_deflate_batch(None, 1, 0, None) == png._lib.PP_ERR_INVALID_ARG
