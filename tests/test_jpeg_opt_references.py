"""CPU: the restatement of the optimised Huffman tables (tests/jpeg_opt_ref.py) - the arbiter of csrc/pp_jpeg_opt_core.h and
csrc/pp_jpeg_entropy_opt.hip - equals libjpeg-turbo: for every image of the grid the four DHT tables and the bytes between SOS
and EOI of Pillow's ``optimize=True`` file are the restatement's, computed from the coefficients tests/jpeg_enc_ref.py gives
(which tests/test_jpeg_enc_references.py pins to Pillow's). Two cases of the grid Pillow cannot write into memory (its own
output-buffer limit); nothing else is left out. Where Pillow is built on another libjpeg the committed fixture
(tests/golden/jpeg_opt_cases.npz) holds the same pin, one of its cases a picture whose table needs the 16-bit limit. Single
mistakes - a tie going to the smaller symbol, no pseudo-symbol, no annex K.3 step, huffval ordered by symbol only - are shown
to fail it, and crafted histograms check the builder where no picture reaches."""
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
PILLOW_CANNOT = {((250, 187), "4:4:4", 95, "noise"), ((250, 187), "4:4:4", 100, "noise")}


def _turbo():
    try:
        from PIL import features

        return bool(features.check_feature("libjpeg_turbo"))
    except Exception:  # noqa: BLE001
        return False


needs_turbo = pytest.mark.skipif(not _turbo(), reason="Pillow is not built on libjpeg-turbo: the committed fixture holds the pin")


@needs_turbo
@pytest.mark.parametrize("subsampling", sorted(E.SUBSAMPLING))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_pillow(size, subsampling):
    W, H = size
    tables = 0
    for quality in QUALITIES:
        for content in E.CONTENTS:
            what = (size, subsampling, quality, content)
            if what in PILLOW_CANNOT:
                continue
            rgb = E.image(content, W, H)
            want_tables, want_scan = O.split_file(O.pillow_optimized(rgb, quality, subsampling))  # (any failure of Pillow's fails the test)
            fwd = E.forward(rgb, quality, subsampling)
            got = O.tables_of(fwd)
            assert O.same_tables(got, want_tables), what
            assert O.scan_bytes(fwd, got) == want_scan, what
            assert all(b.size == 16 for b, _ in got)
            tables += 4
    assert tables == 4 * (len(QUALITIES) * len(E.CONTENTS) - sum(1 for c in PILLOW_CANNOT if c[0] == size and c[1] == subsampling))


def test_the_grid_holds_1192_tables():
    assert 4 * (len(SIZES) * len(E.SUBSAMPLING) * len(QUALITIES) * len(E.CONTENTS) - len(PILLOW_CANNOT)) == 1192


@needs_turbo
def test_pillow_writes_the_length_limited_picture_as_the_restatement_does():
    rgb = O.pillow_limited_image()
    fwd = E.forward(rgb, O.PILLOW_LIMITED_QUALITY, "4:4:4")
    hist = O.histogram(fwd)[O.AC_LUMA]
    assert [int(hist[s]) for s in O.PILLOW_LIMITED_SYMBOLS] == list(O.PILLOW_LIMITED_COUNTS) and hist[0] == 48 * 48 and hist.sum() == sum(O.PILLOW_LIMITED_COUNTS) + 48 * 48
    assert max(O.code_sizes(hist)) == 18
    want_tables, want_scan = O.split_file(O.pillow_optimized(rgb, O.PILLOW_LIMITED_QUALITY, "4:4:4"))
    got = O.tables_of(fwd)
    assert O.same_tables(got, want_tables) and O.scan_bytes(fwd, got) == want_scan


_GOLDEN = []


def _golden():
    """[(case, forward dict, Pillow's tables, Pillow's scan)] of the committed fixture, computed once."""
    if not _GOLDEN:
        z = np.load(os.path.join(HERE, "golden", "jpeg_opt_cases.npz"))
        for i, case in enumerate(str(c) for c in z["cases"]):
            content, W, H, ss, q = case.split("|")
            bits, vals = z[f"bits_{i}"], z[f"vals_{i}"]
            tables = [(bits[t], vals[t][:int(bits[t].sum())]) for t in range(4)]
            _GOLDEN.append((case, E.forward(O.case_image(content, int(W), int(H)), int(q), ss), tables, z[f"scan_{i}"].tobytes()))
    return _GOLDEN


def test_restatement_equals_the_committed_fixture():
    cases = _golden()
    assert len(cases) >= 6 and tuple(c[0] for c in cases) == O.FIXTURE_CASES
    for case, fwd, tables, scan in cases:
        got = O.tables_of(fwd)
        assert O.same_tables(got, tables), case
        assert O.scan_bytes(fwd, got) == scan, case
    assert any(max(O.code_sizes(O.histogram(fwd)[O.AC_LUMA])) > 16 for _, fwd, _, _ in cases), "no case needs the length limit"


@pytest.mark.parametrize("fault", O.FAULTS)
def test_single_faults_are_rejected(fault):
    """Each mistake changes a table of at least one committed case (and the restatement without it matches all)."""
    differs = [case for case, fwd, tables, _ in _golden() if not O.same_tables(O.tables_of(fwd, faults=(fault,)), tables)]
    assert differs, f"no fixture notices {fault}"


def _check_code(bits, vals, freq):
    """A table is a prefix code for exactly the symbols of ``freq``, with no code of all ones and none longer than 16 bits."""
    assert bits.size == 16 and int(bits.sum()) == vals.size
    assert sorted(vals.tolist()) == np.flatnonzero(np.asarray(freq[:256])).tolist()
    assert O.kraft(bits) <= 1.0
    code, length = O.derive(bits, vals)
    for s in vals.tolist():
        assert 1 <= length[s] <= 16 and code[s] != (1 << length[s]) - 1, s
    return length


def test_crafted_length_limiting():
    freq = O.fibonacci_histogram(24)
    assert np.count_nonzero(freq) >= 20
    sizes = O.code_sizes(freq)
    assert max(sizes) > 16 and max(sizes) == 24
    bits, vals = O.optimal_table(freq)
    length = _check_code(bits, vals, freq)
    assert length.max() == 16
    order = np.argsort(-freq[:256], kind="stable")[:24]
    assert (np.diff(length[order]) >= 0).all(), "a rarer symbol got a shorter code"
    unlimited = O.optimal_table(freq, faults=("no_k3",))
    assert unlimited[0].size == 32 and unlimited[0][16:].any()


def test_crafted_all_frequencies_equal():
    freq = np.zeros(257, np.int64)
    freq[O.AC_SYMBOLS[:16]] = 7
    bits, vals = O.optimal_table(freq)
    length = _check_code(bits, vals, freq)
    # sixteen equal symbols and the pseudo-symbol: fifteen codes of four bits, two of five - one of them the pseudo-symbol's;
    # the tie rule pairs the pseudo-symbol (the largest entry) with the largest symbol, which gets the longer code
    assert bits.tolist() == [0, 0, 0, 15, 1] + [0] * 11
    assert length[O.AC_SYMBOLS[15]] == 5 and vals[-1] == O.AC_SYMBOLS[15]
    assert vals[:-1].tolist() == sorted(vals[:-1].tolist())


def test_crafted_one_symbol_only():
    freq = np.zeros(257, np.int64)
    freq[0x21] = 1000
    bits, vals = O.optimal_table(freq)
    assert bits.tolist() == [1] + [0] * 15 and vals.tolist() == [0x21]  # code "0"; "1" is the pseudo-symbol's
    _check_code(bits, vals, freq)
    without = O.optimal_table(freq, faults=("no_pseudo_symbol",))
    assert int(without[0].sum()) == 0, "without the pseudo-symbol a lone symbol gets no code at all"


def test_crafted_empty_chroma():
    """All-zero chroma: DC category 0 and EOB only, each once per block, each a one-bit code."""
    fwd = O.geometry_for_blocks(3, 2)
    hist = O.histogram(fwd)
    assert hist[O.DC_CHROMA].tolist() == [12] + [0] * 256 and hist[O.AC_CHROMA].tolist() == [12] + [0] * 256
    for t in (O.DC_CHROMA, O.AC_CHROMA):
        bits, vals = O.optimal_table(hist[t])
        assert bits.tolist() == [1] + [0] * 15 and vals.tolist() == [0]
    data = O.encode(fwd)
    tables, scan = O.split_file(data)
    assert O.same_tables(tables, O.tables_of(fwd)) and len(scan) == (18 * 2 + 7) // 8
