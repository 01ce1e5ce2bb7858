"""CPU: the ``lz`` match mode of the PNG writer's host form (``png.encode_host(match="lz")``, ``png.zlib_compress_host(match="lz",
period=...)``: the sequential run of the core the kernels share, csrc/pp_png_core.h) against the rule restated in numpy and
the token reader of tests/png_lz_ref.py. For every picture and raw stream of tests/png_ref.py and the cases of png_lz_ref:
``zlib.decompress`` returns the input, the tokens read out of the stream are the restated ones one by one (so the format is
pinned, not the round trip alone), ``tokens_out`` is their number, Pillow opens the files to the pixels, the stream fits
``pp_deflate_bound_lz``; ``match="runs"`` still gives the bytes of the unsuffixed calls, whatever ``period`` says. The size
criterion takes no constant of its own: on the demo picture, the drawn frame and its 2x bilinear resize the ``lz`` stream must
be smaller than the midpoint of the runs stream and ``zlib.compress(filtered, 1)``; on the photo and noise pictures it may
be at most 64 bytes longer than the runs stream (the longer header). No GPU is used."""
import ctypes
import io
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import png_lz_ref as Z  # noqa: E402
import png_ref as R  # noqa: E402
import render_ref  # noqa: E402


@pytest.fixture(scope="module")
def png(lib_built):
    from probpose_code_amd import png

    return png


def all_pictures():
    return {**R.pictures(), **Z.pictures()}


def all_streams():
    return {**{k: (v, 0) for k, v in R.streams().items()}, **Z.streams()}


def check_stream(png, raw: bytes, period: int, z: bytes, tokens_out=None):
    assert zlib.decompress(z) == raw
    got, head = Z.read_tokens(z, with_header=True)
    want = Z.tokens(raw, period)
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{len(got)} tokens, {len(want)} restated; the first difference at {first}: {got[first:first + 3]} / {want[first:first + 3]}")
    assert tokens_out is None or tokens_out == len(want)
    assert len(z) <= int(png._lib.lib.pp_deflate_bound_lz(len(raw)))
    assert head["hlit"] == 286 and not any(16 <= l for l in head["lengths"])
    used = {t[1] for t in want if isinstance(t, tuple)}
    assert head["hdist"] >= 2 or not used  # (a complete code has two symbols at least)
    return want, head


@pytest.mark.parametrize("name", list(all_streams()))
def test_raw_streams_hold_the_restated_tokens(png, name):
    raw, period = all_streams()[name]
    z, count = png.zlib_compress_host(raw, return_tokens=True, match="lz", period=period)
    check_stream(png, raw, period, z, count)
    assert png.zlib_compress_host(raw, match="lz", period=period) == z
    assert png.zlib_compress_host(raw) == png.zlib_compress_host(raw, match="runs", period=period), "period is ignored in runs mode"


@pytest.mark.parametrize("name", list(all_pictures()))
def test_pictures_hold_the_restated_tokens_and_pillow_opens_them(png, name):
    from PIL import Image

    rgb = all_pictures()[name]
    H, W, _ = rgb.shape
    data = png.encode_host(rgb, channel_order="rgb", match="lz")
    assert data[:41] == png.encode_host(rgb, channel_order="rgb")[:33] + (len(data) - 57).to_bytes(4, "big") + b"IDAT"
    z = data[41:-16]
    assert data[-16:-12] == (zlib.crc32(b"IDAT" + z) & 0xFFFFFFFF).to_bytes(4, "big")
    check_stream(png, R.filter_rows(rgb)[0], 1 + 3 * W, z)
    with Image.open(io.BytesIO(data)) as im:
        assert (im.format, im.mode, im.size) == ("PNG", "RGB", (W, H))
        assert np.array_equal(np.asarray(im), rgb)
    assert png.encode_host(np.ascontiguousarray(rgb[:, :, ::-1]), match="lz") == data, "B, G, R in memory gives the same file"
    assert png.encode_host(rgb, channel_order="rgb", match="runs") == png.encode_host(rgb, channel_order="rgb")


def test_the_cases_are_what_they_claim(png):
    """The restatement itself shows what each case is there for."""
    assert Z.far_candidates(4) == (4, 7) and Z.far_candidates(7) == (7, 4, 10)  # width 1 drops S - 3 = 1, width 2 keeps all three
    assert Z.far_candidates(32764) == (32764, 32761, 32767) and Z.far_candidates(32767) == (32767, 32764)
    assert Z.far_candidates(32770) == (32767,) and Z.far_candidates(0) == ()
    raw, near_at, far_at = Z.margin_stream()
    ln, dn, lf, df, reach, kind = Z.choices(raw, 100)
    assert (lf[near_at], reach[near_at], kind[near_at]) == (reach[near_at] + 2, 4, 1) and (lf[far_at], reach[far_at], kind[far_at]) == (reach[far_at] + 3, 4, 2)
    toks, starts = Z.tokens(raw, 100, with_starts=True)
    assert near_at in starts and far_at in starts and (4, 1) in toks and (7, 100) in toks and (6, 100) not in toks
    S = Z.streams()
    dists = {k: sorted({t[1] for t in Z.tokens(*S[k]) if isinstance(t, tuple)}) for k in S}
    assert dists["one distance symbol"] == [100] and dists["no distance symbol"] == [] and dists["noise 8193"] == []
    assert dists["13 extra bits"] == [30300] and dists["P + 3 = 32767 in range"] == [32767]
    assert dists["P + 3 = 32770 dropped"] == [] and dists["P = 32770 dropped, P - 3 kept"] == [32767]
    assert len(S["last tile of one byte"][0]) % R.TILE == 1
    raw, period = S["matches at a tile border"]
    toks, starts = Z.tokens(raw, period, with_starts=True)
    at = dict(zip(starts, toks))
    assert at[R.TILE - 10] == (10, 100) and at[R.TILE] == (30, 100), "the match is cut at the border and goes on behind it from the tile before"
    raw, period = S["g below d"]
    assert Z.match_lengths(np.frombuffer(raw, np.uint8), 50)[49] == 0 and Z.tokens(raw, period)[50] == (100, 50)  # (overlaps its output)
    rows = R.filter_rows(Z.pictures()["width 1365"])[0]
    far = [t for t in Z.tokens(rows, 4096) if isinstance(t, tuple) and t[1] >= 4093]
    assert len(far) >= 16, "rows of 4096 bytes (P = 1 + 3 x 1365): every far source lies in the tile before"
    assert Z.tokens(*S["long pixel run"])[:10] == [9, 140, 77] + [(258, 3)] * 6 + [(3, 3)]


def test_code_edge_cases_in_the_header(png):
    S = Z.streams()
    for name, used in (("one distance symbol", 1), ("no distance symbol", 0)):
        raw, period = S[name]
        _, head = Z.read_tokens(png.zlib_compress_host(raw, match="lz", period=period), with_header=True)
        lengths = head["lengths"][286:]
        assert sorted(l for l in lengths if l) == [1, 1], (name, lengths)  # completed by an unused symbol
    _, head = Z.read_tokens(png.zlib_compress_host(S["13 extra bits"][0], match="lz", period=30300), with_header=True)
    assert head["hdist"] == 30 and head["lengths"][286 + 29] > 0


def test_build_code_lz_is_complete_and_fits_the_header(png):
    rng = np.random.default_rng(2)
    for kind in range(4):
        hist = np.zeros(320, np.uint32)
        if kind == 0:  # Fibonacci counts in both alphabets: the length limit binds
            fib = [1, 1]
            while len(fib) < 40:
                fib.append(fib[-1] + fib[-2])
            hist[:40] = fib
            hist[288:318] = fib[:30]
        elif kind == 1:
            hist[:286] = rng.integers(1, 1000, 286)
            hist[288:318] = rng.integers(1, 1000, 30)
        elif kind == 2:
            hist[65], hist[300] = 5, 9
        code = np.zeros(png.CODE_BYTES_LZ, np.uint8)
        assert png._lib.lib.pp_deflate_build_code_lz(hist.ctypes.data, code.ctypes.data) == 0
        words = code.view(np.uint32)
        for table, n in ((words[:286], 286), (words[368:398], 30)):
            lens = table >> 16
            assert lens.max() <= 15 and sum(1 << (15 - int(l)) for l in lens if l) == 1 << 15
        assert 0 < int(words[288]) <= 2302


def test_bad_arguments(png):
    with pytest.raises(ValueError, match="match"):
        png.encode_host(R.pictures()["1x1"], match="lazy")
    with pytest.raises(ValueError, match="match"):
        png.zlib_compress_host(b"abc", match="LZ")
    with pytest.raises(ValueError, match="period"):
        png.zlib_compress_host(b"abc", match="lz", period=-1)
    assert png.zlib_compress_host(b"abc", match="runs", period=-1) == png.zlib_compress_host(b"abc")
    out, size = np.zeros(64, np.uint8), ctypes.c_size_t(0)
    assert png._lib.lib.pp_zlib_compress_lz(out.ctypes.data, 3, -1, out.ctypes.data, 64, ctypes.byref(size), None) == png._lib.PP_ERR_INVALID_ARG
    assert png._lib.lib.pp_deflate_bound_lz(0) < 0 and png._lib.lib.pp_deflate_scratch_bytes_lz(2 ** 31) < 0
    assert png._lib.lib.pp_deflate_scratch_bytes_lz(4097) % 256 == 0
    from probpose_code_amd.visualization import PoseLocalVisualizer

    with pytest.raises(ValueError, match="png_match"):
        PoseLocalVisualizer(png_encoder="device", png_match="zlib")
    assert PoseLocalVisualizer(png_encoder="device", png_match="lz").png_match == "lz"


def test_a_capacity_one_byte_short_is_reported(png):
    raw, period = Z.streams()["margin"]
    z = png.zlib_compress_host(raw, match="lz", period=period)
    src = np.frombuffer(raw, np.uint8)
    out, size = np.full(len(z) + 8, 0xA5, np.uint8), ctypes.c_size_t(0)
    lib = png._lib.lib
    assert lib.pp_zlib_compress_lz(src.ctypes.data, src.size, period, out.ctypes.data, len(z) - 1, ctypes.byref(size), None) == png._lib.PP_ERR_WORKSPACE
    assert size.value == len(z) and (out == 0xA5).all()
    assert lib.pp_zlib_compress_lz(src.ctypes.data, src.size, period, out.ctypes.data, len(z), ctypes.byref(size), None) == 0
    assert out[:len(z)].tobytes() == z and (out[len(z):] == 0xA5).all()


_DRAWN = {}


def drawn_pictures():
    """The three pictures of the size criterion: the demo picture, the frame ``render_ref.render`` draws on it (two seeded poses
    above, 17 seeded posterior maps composed below: 270 x 720), and that frame resized 2x bilinear (540 x 720 ... 1440)."""
    if not _DRAWN:
        from probpose_code_amd import visualization as V

        demo = R.pictures()["demo picture"]
        H, W = demo.shape[:2]
        rng = np.random.default_rng(3)
        kp = (rng.random((2, 17, 2)) * [W, H]).astype(np.float32)
        boxes = np.array([[10, 10, W * 0.6, H * 0.9], [W * 0.3, 20, W - 10, H - 10]], np.float32)
        maps = render_ref.posterior_like_maps(17, H, W, seed=7)
        frame = render_ref.render(demo, kp, np.ones((2, 17), np.float32), boxes, maps, (0, 0, 0, 0), boxes, V.COCO_SKELETON, V.COCO_LINK_COLORS,
                                  V.COCO_KEYPOINT_COLORS)
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        _DRAWN.update({"demo picture": demo, "drawn frame": frame,
                       "drawn frame 2x bilinear": np.ascontiguousarray(render_ref.resize(frame, 2 * frame.shape[0], 2 * frame.shape[1]), dtype=np.uint8)})
    return _DRAWN


@pytest.mark.parametrize("name", ["demo picture", "drawn frame", "drawn frame 2x bilinear"])
def test_lz_lands_nearer_zlib_level_1_than_runs(png, name):
    rgb = drawn_pictures()[name]
    filtered = R.filter_rows(rgb)[0]
    runs = len(png.encode_host(rgb, channel_order="rgb")) - 57
    lz_file = png.encode_host(rgb, channel_order="rgb", match="lz")
    lz = len(lz_file) - 57
    level1 = len(zlib.compress(filtered, 1))
    print(f"{name}: runs {runs}, lz {lz}, zlib level 1 {level1}, zlib level 6 {len(zlib.compress(filtered, 6))}")
    assert zlib.decompress(lz_file[41:-16]) == filtered
    assert lz < (runs + level1) / 2


@pytest.mark.parametrize("name", ["photo 150x201", "noise", "noise row bytes 4096"])
def test_lz_costs_a_longer_header_at_most_where_nothing_repeats(png, name):
    rgb = R.pictures()[name]
    runs, lz = (len(png.encode_host(rgb, channel_order="rgb", match=m)) for m in ("runs", "lz"))
    print(f"{name}: runs {runs}, lz {lz}")
    assert lz <= runs + 64
