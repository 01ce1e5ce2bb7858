"""CPU: the PNG writer's device code build, run one step after another on the host (``pp_deflate_build_code_steps``,
``pp_deflate_build_code_steps_lz``: the steps of csrc/pp_png_code_core.h, the text the ``png_code`` kernel runs), against the
host builders ``pp_deflate_build_code`` / ``pp_deflate_build_code_lz``. Every one of the ``CODE_BYTES`` / ``CODE_BYTES_LZ`` bytes
must be equal: on the named histograms of tests/png_code_ref.py, on 2 000 random histograms of runs mode and on 2 000 of lz
mode. Histogram (a) is held to what it is there for by the Python restatement of the merge: its code-length tree is deeper
than 7, so the limit-7 repair runs. Also what ``code=``, ``png_code=`` and ``--png-code`` refuse. No GPU is used."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import png_code_ref as C  # noqa: E402


@pytest.fixture(scope="module")
def png(lib_built):
    from probpose_code_amd import png

    return png


def build(png, fn, hist, size):
    """The code struct `fn` makes of `hist`, as bytes; the buffer starts as 0xA5 so that a byte left unwritten shows."""
    hist = np.ascontiguousarray(hist, np.uint32)
    code = np.full(size + 64, 0xA5, np.uint8)
    assert getattr(png._lib.lib, fn)(hist.ctypes.data, code.ctypes.data) == 0
    assert (code[size:] == 0xA5).all(), f"{fn} wrote behind the struct"
    return code[:size].tobytes()


def differing(png, hists, lz):
    """The indices of the histograms whose two codes differ in any byte."""
    host, steps, size = (("pp_deflate_build_code_lz", "pp_deflate_build_code_steps_lz", png.CODE_BYTES_LZ) if lz else
                         ("pp_deflate_build_code", "pp_deflate_build_code_steps", png.CODE_BYTES))
    return [i for i, h in enumerate(hists) if build(png, host, h, size) != build(png, steps, h, size)]


def test_constants_mirror_the_structs(png):
    assert (png.CODE_BYTES, png.CODE_BYTES_LZ, png.HIST_BYTES, png.HIST_BYTES_LZ) == (1472, 1600, 4 * C.HIST_WORDS, 4 * C.HIST_WORDS_LZ)
    assert png.LAUNCHES_CODE == ("png_code",) and png.LAUNCHES_CODE_LZ == ("png_code_lz",)
    assert isinstance(png.code_calls, int)


def test_histogram_a_has_a_code_length_tree_deeper_than_7():
    hist, want = C.deep_lengths()
    counts = hist[:C.SYMS].copy()
    assert counts[256] > 0 and int((counts > 0).sum()) == 222
    depths = C.huffman_depths(counts)
    assert depths == want and max(depths.values()) == 15, "build_lengths at limit 15 returns exactly these lengths, with no repair"
    cl_counts = np.bincount(list(depths.values()) + [0] * (C.SYMS - len(depths)) + [1], minlength=16)
    assert cl_counts.tolist() == C.DEEP_CL_COUNTS
    cl_depths = C.huffman_depths(list(cl_counts) + [0, 0, 0])
    assert max(cl_depths.values()) == 10 > 7, "the case no longer reaches the repair loop of the code-length code"


def test_what_the_other_named_histograms_reach():
    named = C.named_runs()
    assert max(C.huffman_depths(named["b: Fibonacci on 40 symbols"][:C.SYMS]).values()) == 39
    counts = named["c: all counts zero"][:C.SYMS].copy()
    counts[256] = 1
    assert C.huffman_depths(counts) == {0: 1, 256: 1}
    assert int(named["f: all 286 at 2^32 - 1"][:C.SYMS].astype(np.uint64).sum()) >= 1 << 32
    assert int((named["g: 257 used symbols"] > 0).sum()) == 257
    dist = C.named_distances()
    assert set(C.huffman_depths(dist["all zero"])) == {0, 1}
    assert max(C.huffman_depths(dist["Fibonacci over all 30"]).values()) == 29


def test_named_histograms_runs(png):
    named = C.named_runs()
    bad = differing(png, named.values(), False)
    assert not bad, [list(named)[i] for i in bad]


def test_named_histograms_lz(png):
    named = C.named_lz()
    assert len(named) == 35
    bad = differing(png, named.values(), True)
    assert not bad, [list(named)[i] for i in bad]
    # HDIST as the cases say: all zero -> two symbols, only symbol 29 -> all thirty
    words = np.frombuffer(build(png, "pp_deflate_build_code_steps_lz", named["c: all counts zero | all zero"], png.CODE_BYTES_LZ), np.uint32)
    assert (int(words[292]) >> 24) & 31 == 2 - 1  # header word 0: 78 01, BFINAL, BTYPE, HLIT; HDIST at bits 24 .. 28
    words = np.frombuffer(build(png, "pp_deflate_build_code_steps_lz", named["c: all counts zero | only symbol 29"], png.CODE_BYTES_LZ), np.uint32)
    assert (int(words[292]) >> 24) & 31 == 30 - 1


def test_2000_random_histograms_runs(png):
    bad = differing(png, C.random_runs(2000, 23), False)
    assert not bad, f"{len(bad)} of 2000 differ, the first: {bad[:5]}"


def test_2000_random_histograms_lz(png):
    bad = differing(png, C.random_lz(2000, 29), True)
    assert not bad, f"{len(bad)} of 2000 differ, the first: {bad[:5]}"


def test_the_steps_keep_the_bounds_of_the_format(png):
    for h in list(C.named_runs().values()) + list(C.random_runs(50, 31)):
        words = np.frombuffer(build(png, "pp_deflate_build_code_steps", h, png.CODE_BYTES), np.uint32)
        assert int((words[:288] >> 16).max()) <= 15 and 0 < int(words[288]) <= 16 + 3 + 14 + 19 * 3 + 287 * 7
        assert not words[286:288].any() and not words[289:292].any()
    for h in list(C.named_lz().values()) + list(C.random_lz(50, 37)):
        words = np.frombuffer(build(png, "pp_deflate_build_code_steps_lz", h, png.CODE_BYTES_LZ), np.uint32)
        assert int((words[:288] >> 16).max()) <= 15 and int((words[368:400] >> 16).max()) <= 15 and 0 < int(words[288]) <= 2302
        assert not words[398:400].any()


def test_bad_arguments(png):
    lib = png._lib.lib
    buf = np.zeros(png.CODE_BYTES_LZ, np.uint8)
    for fn in ("pp_deflate_build_code_steps", "pp_deflate_build_code_steps_lz"):
        assert getattr(lib, fn)(None, buf.ctypes.data) == png._lib.PP_ERR_INVALID_ARG
        assert getattr(lib, fn)(buf.ctypes.data, None) == png._lib.PP_ERR_INVALID_ARG
    picture = np.zeros((2, 2, 3), np.uint8)
    with pytest.raises(ValueError, match="code"):
        png.encode_batch([picture], code="gpu")
    with pytest.raises(ValueError, match="code"):
        png.encode_batch([picture], match="lz", code=None)
    with pytest.raises(ValueError, match="code"):
        png.zlib_compress_device([b"abc"], code="Device")
    with pytest.raises(ValueError, match="code"):
        png.imwrite_device(os.devnull, picture, code="both")
    from probpose_code_amd.visualization import PoseLocalVisualizer

    with pytest.raises(ValueError, match="png_code"):
        PoseLocalVisualizer(png_encoder="device", png_code="gpu")
    assert PoseLocalVisualizer(png_encoder="device", png_code="device").png_code == "device"
    assert PoseLocalVisualizer().png_code == "host"


def test_the_demo_refuses_another_png_code():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo", "image_demo.py"), "x.png", "x.py", "synthetic", "--png-code", "gpu"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--png-code" in r.stderr and "invalid choice" in r.stderr, r.stderr[-500:]
