"""CPU: the sequential restatement of the device Huffman decoder (tests/jpeg_huffdec_ref.py) - the same subsequences, state,
invalid-code rule and passes as csrc/pp_jpeg_huffdec.hip - gives the coefficients of jpeg_ref.parse and jpeg.entropy_decode;
its pass count for every corpus file is within the default sync_passes; the named slow-synchronising stream needs more than
sync_passes = 1 and is refused there, not decoded wrongly; and the comparison catches each of three single faults."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_huffdec_cases as C  # noqa: E402
import jpeg_huffdec_ref as R  # noqa: E402
import jpeg_ref as J  # noqa: E402
import jpeg_sources as S  # noqa: E402


@pytest.fixture(scope="module")
def jpeg(lib_built):
    from probpose_code_amd import jpeg

    return jpeg


def _cases():
    """name -> bytes: the corpus, the layout sources and the size cases that have no restart interval."""
    cases = dict(C.corpus())
    for name in S.SMALL_SOURCES:
        if S.SOURCES[name][5] == 0:
            cases[name] = S.source(name)
    for name in ("33x17_420", "37x29_444", "48x64_grey"):
        for layout in ("fibonacci", "shared_pair_slots_2_3", "slots_3_2_split", "pq1_sof1"):
            cases[f"{name}/{layout}"] = S.transcoded(name, layout)
    return cases


def test_constants_are_the_kernels(jpeg):
    assert (R.S, R.INNER, R.DEFAULT_PASSES, R.MAX_PASSES) == (jpeg.SUBSEQUENCE_BYTES, jpeg.INNER_ITERATIONS, jpeg.DEFAULT_SYNC_PASSES,
                                                              jpeg.MAX_SYNC_PASSES)
    core = open(os.path.join(HERE, "..", "probpose_code_amd", "csrc", "pp_jpeg_huffdec_core.h")).read()
    for text in (f"HD_S = {R.S};", f"HD_WG = {R.WG};", f"HD_INNER = {R.INNER};", f"HD_MAX_PASSES = {R.MAX_PASSES};",
                 f"HD_DEFAULT_PASSES = {R.DEFAULT_PASSES};"):
        assert text in core, text
    assert R.covered_bytes(R.DEFAULT_PASSES) >= 8192 > R.covered_bytes(R.DEFAULT_PASSES - 1)


def test_restatement_equals_the_reference_parser_and_the_host_decoder(jpeg):
    cases = _cases()
    assert len(cases) >= 100
    samplings = set()
    for name, data in cases.items():
        want = J.flat_coefficients(J.parse(data))
        r = C.reference(data)
        assert r["status"] == R.OK, (name, r["status"])
        assert r["coef"].dtype == np.int16 and np.array_equal(r["coef"], want), name
        assert np.array_equal(jpeg.entropy_decode(data).coef, want), name
        assert r["passes"] <= R.DEFAULT_PASSES, (name, r["passes"])
        p = C.prepared(data)
        samplings.add((p["ncomp"], p["hs"], p["vs"]))
        assert r["blocks"] >= p["mcus_x"] * p["mcus_y"] * (1 if p["ncomp"] == 1 else p["hs"] * p["vs"] + 2), name
    assert samplings == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}


def test_corpus_pass_counts_are_within_the_default():
    worst = max(C.reference(data)["passes"] for data in C.corpus().values())
    assert 1 <= worst <= R.DEFAULT_PASSES


def test_slow_stream_needs_more_than_one_pass_and_is_refused_there(jpeg):
    data = C.slow_stream()
    p = C.prepared(data)
    assert len(p["stream"]) > R.S * R.WG, "the stream must cross a workgroup border"
    needed = R.passes_needed(p)
    assert 1 < needed <= R.DEFAULT_PASSES, needed
    want = J.flat_coefficients(J.parse(data))
    for passes in range(1, needed):
        r = R.decode(p, passes)
        assert r["status"] == R.NOT_SYNCHRONISED and r["coef"] is None, passes
    r = C.reference(data, needed)
    assert r["status"] == R.OK and r["passes"] == needed and np.array_equal(r["coef"], want)
    assert np.array_equal(C.reference(data)["coef"], want)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_single_faults_are_caught(fault):
    """A restatement with one mistake differs from the reference parser on at least one input (and the sound one on none)."""
    inputs = {"slow": C.slow_stream(), "ff00_split": C.find("ff00_split"), "420": S.source("33x17_420")}
    caught = []
    for name, data in inputs.items():
        want = J.flat_coefficients(J.parse(data))
        assert np.array_equal(C.reference(data)["coef"], want), name
        r = R.decode(C.prepared(data), R.DEFAULT_PASSES, fault=fault)
        if r["status"] != R.OK or not np.array_equal(r["coef"], want):
            caught.append(name)
    assert caught, fault
    if fault == "ff00_boundary":
        assert "ff00_split" in caught
    if fault == "accept_first":
        assert "slow" in caught


def test_boundary_situations_are_found():
    """The searches the GPU tests rely on: each situation occurs in a small Pillow file (or a hand-built stream)."""
    for situation in ("ff00_split", "code_straddles", "extra_bits_straddle", "ends_at_63", "zrl", "longest_codes"):
        assert situation in R.situations(C.prepared(C.find(situation))), situation
    for length, name in ((R.S, "len_S"), (R.S - 1, "len_S-1"), (R.S + 1, "len_S+1"), (2 * R.S, "len_2S")):
        assert name in R.situations(C.prepared(C.find_length(length))), name
