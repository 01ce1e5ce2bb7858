"""CPU: the host form of the optimised Huffman tables (csrc/pp_jpeg_opt_core.h behind pp_jpeg_symbol_histogram,
pp_jpeg_optimal_table, pp_jpeg_write_headers_tables and pp_jpeg_entropy_encode_opt) against the restatement
(tests/jpeg_opt_ref.py), which tests/test_jpeg_opt_references.py pins to Pillow: histograms and tables value for value, files
byte for byte at restart intervals 0, 1, 3 and one above the MCU count; every file decodes - here and in Pillow - to what the
default file decodes to and is no longer than it; the error contracts; and ``optimize=False`` writes today's bytes."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_enc_ref as E  # noqa: E402
import jpeg_opt_ref as O  # noqa: E402

SIZES = ((8, 8), (17, 13), (64, 96), (250, 187))  # width x height
QUALITIES = (1, 24, 75, 95, 100)


@pytest.fixture(scope="module")
def jpeg(lib_built):
    from probpose_code_amd import jpeg

    return jpeg


def as_coefficients(jpeg, fwd):
    """A ``jpeg_enc_ref.forward``-shaped dict as JpegCoefficients."""
    info = jpeg.encode_plan(fwd["width"], fwd["height"], {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}[fwd["hs"], fwd["vs"]])
    coef = np.ascontiguousarray(E.flat_coefficients(fwd), np.int16)
    assert coef.size == info.coef_count
    return jpeg.JpegCoefficients(info, coef, np.asarray(fwd["qtables"], np.uint16))


_FWD = {}


def forward(content, W, H, ss, q):
    key = (content, W, H, ss, q)
    if key not in _FWD:
        _FWD[key] = E.forward(E.image(content, W, H), q, ss)
    return _FWD[key]


def crafted():
    equal = np.zeros(257, np.int64)
    equal[O.AC_SYMBOLS[:12]] = 16
    return {"length limited": O.length_limited_coefficients(), "all equal": O.coefficients_for_luma_symbols(equal, 4, 4),
            "single symbol": O.geometry_for_blocks(3, 2)}


@pytest.mark.parametrize("subsampling", sorted(E.SUBSAMPLING))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_histograms_and_tables_equal_the_restatement_on_the_grid(jpeg, size, subsampling):
    W, H = size
    for q in QUALITIES:
        for content in E.CONTENTS:
            fwd = forward(content, W, H, subsampling, q)
            hist = jpeg.symbol_histogram(as_coefficients(jpeg, fwd))
            assert hist.dtype == np.uint32 and np.array_equal(hist, O.histogram(fwd)), (size, subsampling, q, content)
            for t in range(4):
                bits, vals = jpeg.optimal_table(hist[t])
                want = O.optimal_table(hist[t])
                assert np.array_equal(bits, want[0]) and np.array_equal(vals, want[1]), (size, subsampling, q, content, t)
                assert vals.size <= (12, 162)[t & 1], "more symbols than the annex K table"


def test_tables_of_crafted_histograms_equal_the_restatement(jpeg):
    equal = np.zeros(257, np.int64)
    equal[O.AC_SYMBOLS[:16]] = 7
    one = np.zeros(257, np.int64)
    one[0x21] = 1000
    full = np.arange(1, 258, dtype=np.int64)  # every symbol, all frequencies different
    ties = np.zeros(257, np.int64)
    ties[:200] = np.repeat(np.arange(1, 41), 5)  # five-way ties at forty frequencies
    big = np.zeros(257, np.int64)
    big[[0, 1, 2, 0xF0]] = [2 ** 32 - 2 ** 30, 2 ** 29, 2 ** 29 - 1, 1]  # sums near 2^32
    for name, freq in (("fibonacci", O.fibonacci_histogram(24)), ("equal", equal), ("one", one), ("full", full), ("ties", ties), ("big", big),
                       ("limited", O.histogram(O.length_limited_coefficients())[O.AC_LUMA])):
        bits, vals = jpeg.optimal_table(freq.astype(np.uint32))
        want = O.optimal_table(freq)
        assert want[0].size == 16 and np.array_equal(bits, want[0]) and np.array_equal(vals, want[1]), name
    bits, vals = jpeg.optimal_table(np.zeros(257, np.uint32))  # (no scan has an empty table; libjpeg would read out of bounds)
    assert not bits.any() and vals.size == 0
    deep = np.zeros(257, np.int64)
    a, b = 1, 2
    for s in O.AC_SYMBOLS[:40]:  # forty Fibonacci counts: a tree 40 deep, beyond libjpeg's 32
        deep[s] = a
        a, b = b, a + b
    assert deep.max() < 2 ** 32
    with pytest.raises(ValueError):
        O.optimal_table(deep)
    with pytest.raises(jpeg._lib.ProbPoseLibraryError, match="PP_ERR_INVALID_ARG"):
        jpeg.optimal_table(deep.astype(np.uint32))


def _restart_cases():
    yield "length limited", O.length_limited_coefficients()
    yield "single symbol", O.geometry_for_blocks(3, 2)
    for content, W, H, ss, q in (("noise", 17, 13, "4:2:0", 75), ("gradient", 64, 96, "4:2:2", 24), ("noise", 64, 96, "4:4:4", 100),
                                 ("checker", 17, 13, "4:4:4", 95), ("noise", 250, 187, "4:2:0", 75)):
        yield f"{content} {W}x{H} {ss} q{q}", forward(content, W, H, ss, q)


def test_files_equal_the_restatement_at_every_restart_interval(jpeg):
    for name, fwd in _restart_cases():
        c = as_coefficients(jpeg, fwd)
        mcus = fwd["mcus_x"] * fwd["mcus_y"]
        for ri in (0, 1, 3, mcus + 1):
            assert np.array_equal(jpeg.symbol_histogram(c, ri), O.histogram(fwd, ri)), (name, ri)
            got, want = jpeg.entropy_encode(c, ri, optimize=True), O.encode(fwd, ri)
            assert got == want, (name, ri, len(got), len(want))
            tables = O.tables_of(fwd, ri)
            bits, vals = np.stack([b for b, _ in tables]), np.stack([np.pad(v, (0, 256 - v.size)) for _, v in tables])
            assert jpeg.write_headers(c.qtables, c.info, ri, tables=(bits, vals)) == O.headers(fwd, tables, ri), (name, ri)
            assert got.startswith(O.headers(fwd, tables, ri))


def _dht_bytes(data):
    tables, _ = O.split_file(data)
    return sum(2 + 2 + 17 + v.size for _, v in tables)


def _pillow_pixels(data):
    from PIL import Image

    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB")).copy()


@pytest.mark.parametrize("subsampling", sorted(E.SUBSAMPLING))
def test_files_decode_to_the_default_files_coefficients_and_pixels_and_are_no_longer(jpeg, subsampling):
    cases = [(f"{content} {W}x{H} q{q}", forward(content, W, H, subsampling, q)) for (W, H) in SIZES for q in (1, 75, 100) for content in ("noise", "flat0", "gradient")]
    if subsampling == "4:4:4":
        cases += list(crafted().items())
    for name, fwd in cases:
        c = as_coefficients(jpeg, fwd)
        for ri in (0, 3):
            plain, opt = jpeg.entropy_encode(c, ri), jpeg.entropy_encode(c, ri, optimize=True)
            assert plain == jpeg.entropy_encode(c, ri, optimize=False), name
            back = jpeg.entropy_decode(opt)
            assert np.array_equal(back.coef, c.coef) and np.array_equal(back.qtables, c.qtables) and back.info.restart_interval == ri, (name, ri)
            assert np.array_equal(jpeg.entropy_decode(plain).coef, c.coef)
            assert np.array_equal(_pillow_pixels(opt), _pillow_pixels(plain)), (name, ri)
            assert len(opt) <= len(plain) + (_dht_bytes(opt) - _dht_bytes(plain)), (name, ri, len(opt), len(plain))
            assert len(opt) <= len(plain), (name, ri)  # (the tables themselves never grow either: no more symbols than annex K's)


def test_the_length_limited_case_round_trips(jpeg):
    fwd = O.length_limited_coefficients()
    assert (fwd["mcus_x"], fwd["mcus_y"], fwd["hs"], fwd["vs"]) == (17, 17, 1, 1)
    c = as_coefficients(jpeg, fwd)
    hist = jpeg.symbol_histogram(c)[O.AC_LUMA]
    assert max(O.code_sizes(hist)) > 16
    data = jpeg.entropy_encode(c, optimize=True)
    tables, _ = O.split_file(data)
    assert tables[O.AC_LUMA][0][15] > 0 and O.kraft(tables[O.AC_LUMA][0]) < 1.0
    assert np.array_equal(jpeg.entropy_decode(data).coef, c.coef)
    assert np.array_equal(_pillow_pixels(data), _pillow_pixels(jpeg.entropy_encode(c)))


def _raw_encode(jpeg, name, c, capacity, ri=0):
    out = np.full(capacity + 64, 0xA5, np.uint8)
    size = ctypes.c_size_t(123)
    qt = np.ascontiguousarray(c.qtables, np.uint16)
    st = getattr(jpeg._lib.lib, name)(c.coef.ctypes.data, qt.ctypes.data, ctypes.byref(c.info), ri, out.ctypes.data, capacity, ctypes.byref(size))
    assert (out[capacity:] == 0xA5).all(), "bytes behind the capacity written"
    return st, size.value, out[:capacity]


def test_error_contracts(jpeg):
    _lib = jpeg._lib
    c = as_coefficients(jpeg, forward("noise", 64, 96, "4:2:0", 75))
    data = jpeg.entropy_encode(c, optimize=True)
    st, size, out = _raw_encode(jpeg, "pp_jpeg_entropy_encode_opt", c, len(data))
    assert (st, size, out.tobytes()) == (_lib.PP_OK, len(data), data)
    st, size, _ = _raw_encode(jpeg, "pp_jpeg_entropy_encode_opt", c, len(data) - 1)  # one byte short
    assert (st, size) == (_lib.PP_ERR_WORKSPACE, 0)
    st, size, _ = _raw_encode(jpeg, "pp_jpeg_entropy_encode_opt", c, 100)  # not even the headers
    assert (st, size) == (_lib.PP_ERR_WORKSPACE, 0)
    for at, value in ((7, 1024), (7, -1024), (0, 4000), (64 * 5, -4000)):  # AC outside +-1023, DC differences outside +-2047
        bad = jpeg.JpegCoefficients(c.info, c.coef.copy(), c.qtables)
        bad.coef[at] = value
        for name in ("pp_jpeg_entropy_encode_opt", "pp_jpeg_entropy_encode"):
            assert _raw_encode(jpeg, name, bad, len(data) + 4096)[:2] == (_lib.PP_ERR_INVALID_ARG, 0), (at, value, name)
        with pytest.raises(_lib.ProbPoseLibraryError, match="PP_ERR_INVALID_ARG"):
            jpeg.symbol_histogram(bad)
    # a plan of more than 2^32 / 64 blocks: 32-bit frequencies would not be exact. The plan is refused before any coefficient is read.
    huge = jpeg.encode_plan(65535, 65535, "4:4:4")
    assert huge.coef_count // 64 > (2 ** 32 - 1) // 64
    hist = np.zeros((4, 257), np.uint32)
    qt = jpeg.quality_tables(75)
    out, size, one = np.zeros(4096, np.uint8), ctypes.c_size_t(0), np.zeros(64, np.int16)
    assert _lib.lib.pp_jpeg_symbol_histogram(one.ctypes.data, ctypes.byref(huge), 0, hist.ctypes.data) == _lib.PP_ERR_INVALID_ARG
    assert b"32-bit" in _lib.lib.pp_last_error()
    assert _lib.lib.pp_jpeg_entropy_encode_opt(one.ctypes.data, qt.ctypes.data, ctypes.byref(huge), 0, out.ctypes.data, out.size,
                                               ctypes.byref(size)) == _lib.PP_ERR_INVALID_ARG
    assert _lib.lib.pp_jpeg_entropy_opt_scratch_bytes(ctypes.byref(huge), 1) == _lib.PP_ERR_INVALID_ARG
    largest = jpeg.encode_plan(65535, 32760, "4:2:0")  # (the other side of the limit is a size query away)
    assert largest.coef_count // 64 <= (2 ** 32 - 1) // 64 and _lib.lib.pp_jpeg_entropy_opt_scratch_bytes(ctypes.byref(largest), 1) > 0
    # tables that are no prefix code
    bits, vals = np.zeros((4, 16), np.uint8), np.zeros((4, 256), np.uint8)
    bits[:, 0] = 3
    with pytest.raises(_lib.ProbPoseLibraryError, match="PP_ERR_INVALID_ARG"):
        jpeg.write_headers(qt, c.info, 0, tables=(bits, vals))
    assert _lib.lib.pp_jpeg_encoded_bound(ctypes.byref(c.info)) >= len(data)


def test_the_default_writes_todays_bytes(jpeg):
    """``optimize=False`` and ``tables=None`` are the calls of before: annex K's tables, the same files (the default coder's own
    tests pin those to Pillow)."""
    for name, fwd in _restart_cases():
        c = as_coefficients(jpeg, fwd)
        for ri in (0, 3):
            data = jpeg.entropy_encode(c, ri)
            assert data == jpeg.entropy_encode(c, ri, optimize=False) == jpeg.entropy_encode(c, restart_interval=ri)
            head = jpeg.write_headers(c.qtables, c.info, ri)
            assert head == jpeg.write_headers(c.qtables, c.info, ri, tables=None) and data.startswith(head)
            tables, _ = O.split_file(data)
            assert [int(b.sum()) for b, _ in tables] == [12, 162, 12, 162]
            assert data != jpeg.entropy_encode(c, ri, optimize=True)
