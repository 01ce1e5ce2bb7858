"""CPU: what the device Huffman coder with restart intervals (pp_jpeg_entropy_encode_restart_batch,
pp_jpeg_entropy_encode_opt_restart_batch) shows without a GPU - its symbols and scratch query, the argument refusals of
``entropy_encode_device(restart_interval=)`` and ``encode_batch(restart_rows=)`` - and the proof, from the host coder's own
streams, that the hand-made coefficient sets of tests/jpeg_entropy_restart_cases.py hold every form the GPU test relies on."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_entropy_restart_cases as RC  # noqa: E402


@pytest.fixture(scope="module")
def jpeg():
    from probpose_code_amd import jpeg

    return jpeg


@pytest.fixture(scope="module")
def parsed(jpeg):
    """name -> (c, R, host file, unstuffed intervals, marker numbers, bits per interval) of the hand-made sets."""
    out = {}
    for name, (c, R) in RC.hand_made(jpeg).items():
        f = jpeg.entropy_encode(c, R)
        parts, markers = RC.split_scan(RC.scan_of(jpeg, c, f, R))
        bits = RC.interval_bits(c, f, R)
        assert [len(p) for p in parts] == [(b + 7) // 8 for b in bits], name  # (the reading of the stream and the arithmetic agree)
        assert markers == [j % 8 for j in range(len(parts) - 1)], name
        out[name] = (c, R, f, parts, markers, bits)
    return out


def test_the_new_symbols_exist(jpeg):
    lib = jpeg._lib.lib
    for name in ("pp_jpeg_entropy_restart_scratch_bytes", "pp_jpeg_entropy_encode_restart_batch", "pp_jpeg_entropy_encode_opt_restart_batch"):
        assert callable(getattr(lib, name)), name
    assert lib.pp_jpeg_entropy_encode_restart_batch(None, 0, 0, None) == jpeg._lib.PP_OK
    assert lib.pp_jpeg_entropy_encode_opt_restart_batch(None, 0, 0, None) == jpeg._lib.PP_OK
    assert lib.pp_jpeg_entropy_encode_restart_batch(None, 1, 3, None) == jpeg._lib.PP_ERR_INVALID_ARG
    assert lib.pp_jpeg_entropy_encode_opt_restart_batch(None, -1, 3, None) == jpeg._lib.PP_ERR_INVALID_ARG


def test_the_descriptor_keeps_its_size_and_names_the_interval(jpeg):
    d, r = jpeg._ENT_DESC, jpeg._ENT_RESTART_DESC
    assert d.itemsize == r.itemsize == 64 and jpeg._ENT_OPT_RESTART_DESC.itemsize == jpeg._ENT_OPT_DESC.itemsize == 72
    assert r.fields["restart_interval"][1] == 56 and r.fields["reserved"][1] == 60 and d.fields["reserved"][1] == 56
    for name in d.names[:-1]:
        assert d.fields[name] == r.fields[name], name
    assert jpeg._ENT_OPT_RESTART_DESC.fields["record"][1] == 64


def test_the_scratch_query_is_at_least_the_old_one_and_monotone(jpeg):
    lib = jpeg._lib.lib
    for ss in ("4:4:4", "4:2:2", "4:2:0"):
        last = 0
        for W, H in ((1, 1), (8, 8), (17, 33), (96, 64), (250, 130), (640, 480), (1920, 1080), (8000, 6000)):
            info = jpeg.encode_plan(W, H, ss)
            old, new = int(lib.pp_jpeg_entropy_scratch_bytes(ctypes.byref(info), 1)), int(lib.pp_jpeg_entropy_restart_scratch_bytes(ctypes.byref(info), 1))
            assert new >= old > 0 and new % 256 == 0, (ss, W, H)
            # per MCU sixteen bytes of interval table and seven padding bits, alignment and stuffing chunk counters aside
            assert new - old <= 17 * info.mcus_x * info.mcus_y + 4096, (ss, W, H, old, new)
            assert new >= last, (ss, W, H)
            last = new
    infos = [jpeg.encode_plan(W, H, "4:2:0") for W, H in ((8, 8), (250, 130), (17, 33))]
    each = [int(lib.pp_jpeg_entropy_restart_scratch_bytes(ctypes.byref(i), 1)) for i in infos]
    assert int(lib.pp_jpeg_entropy_restart_scratch_bytes((jpeg.JpegInfo * 3)(*infos), 3)) == sum(each)
    assert lib.pp_jpeg_entropy_restart_scratch_bytes(None, 1) == jpeg._lib.PP_ERR_INVALID_ARG
    bad = jpeg.encode_plan(16, 16, "4:2:0")
    bad.mcus_x = 7
    assert lib.pp_jpeg_entropy_restart_scratch_bytes(ctypes.byref(bad), 1) == jpeg._lib.PP_ERR_INVALID_ARG


def test_entropy_encode_device_refuses_bad_intervals_before_any_gpu_work(jpeg):
    c = RC.hand_made(jpeg)["zeros r1"][0]
    for bad in (True, 1.0, "1", -1, 65536, None, [1, 2], [True], [0.5], (70000,)):
        with pytest.raises(ValueError, match="restart_interval"):
            jpeg.entropy_encode_device([c], "cuda:0", restart_interval=bad)
    with pytest.raises(ValueError, match="restart_interval"):
        jpeg.entropy_encode_device([], "cuda:0", restart_interval=[1])
    assert jpeg.entropy_encode_device([], "cuda:0", restart_interval=3) == []


def test_encode_batch_refuses_bad_restart_rows_before_any_gpu_work(jpeg):
    img = np.zeros((16, 64, 3), np.uint8)
    for entropy in ("host", "device"):
        for bad in (True, 1.0, "1", -1, 65536, None):
            with pytest.raises(ValueError, match="restart_rows"):
                jpeg.encode_batch([img], restart_rows=bad, entropy=entropy)
        with pytest.raises(ValueError, match="restart_rows.*restart_interval|restart_interval.*restart_rows"):
            jpeg.encode_batch([img], restart_rows=1, restart_interval=4, entropy=entropy)
        # 64 pixels of 4:4:4 are eight MCUs a row: 8192 rows of them are 65536 MCUs, one more than a DRI segment holds
        with pytest.raises(ValueError, match="image 1 .*65535"):
            jpeg.encode_batch([np.zeros((8, 8, 3), np.uint8), img], subsampling="4:4:4", restart_rows=8192, entropy=entropy)
        with pytest.raises(ValueError, match="subsampling"):
            jpeg.encode_batch([img], subsampling="4:1:1", restart_rows=1, entropy=entropy)
    with pytest.raises(ValueError, match="restart_rows.*entropy_encode_device|entropy_encode_device.*restart_rows") as e:
        jpeg.encode_batch([img], entropy="device", restart_interval=4)
    assert "restart" in str(e.value)
    assert jpeg.encode_batch([], restart_rows=2) == [] and jpeg.encode_batch([], restart_rows=2, entropy="device") == []


def test_the_visualizer_takes_restart_rows():
    from probpose_code_amd.visualization import PoseLocalVisualizer

    assert PoseLocalVisualizer(device="cuda:0").jpeg_restart_rows == 0
    assert PoseLocalVisualizer(device="cuda:0", jpeg_restart_rows=2).jpeg_restart_rows == 2
    for bad in (True, 1.5, -1, 65536):
        with pytest.raises(ValueError, match="jpeg_restart_rows"):
            PoseLocalVisualizer(device="cuda:0", jpeg_restart_rows=bad)


# ------------------------------------------------------------------------------ the forms of the hand-made sets
def test_an_interval_ends_at_each_bit_phase(parsed):
    bits = parsed["phases r1"][5]
    assert len(bits) == 64 and {b % 8 for b in bits[:-1]} == set(range(8))


def test_padding_bytes_and_whole_data_bytes_come_out_as_ff_in_front_of_markers(parsed):
    padded = whole = 0
    for name in ("ff ends 4:4:4", "ff ends 4:2:0"):
        c, R, f, parts, markers, bits = parsed[name]
        assert len(parts) == 32
        for j, (p, b) in enumerate(zip(parts[:-1], bits)):
            assert p[-1] == 0xFF, (name, j)  # ten one bits end every interval: its last byte is FF whatever the phase
            padded += b % 8 != 0
            whole += b % 8 == 0
        assert f.count(b"\xff\x00\xff\xd0") >= 1 and sum(f.count(bytes((0xFF, 0x00, 0xFF, 0xD0 + k))) for k in range(8)) == 31, name
    assert padded >= 8 and whole >= 2, (padded, whole)


def test_marker_numbers_wrap_and_an_interval_count_that_does_not_divide(parsed):
    c, R, f, parts, markers, bits = parsed["ragged r2"]
    assert R == 2 and len(parts) == 10 and markers == [0, 1, 2, 3, 4, 5, 6, 7, 0]
    c, R, f, parts, markers, bits = parsed["ragged r3"]
    mcus = c.info.mcus_x * c.info.mcus_y
    assert R == 3 and mcus == 20 and mcus % R != 0 and len(parts) == 7
    assert len(parsed["phases r1"][4]) == 63


def test_an_interval_of_the_mcu_count_or_more_gives_dri_and_the_plain_scan(jpeg, parsed):
    for name in ("single whole", "single beyond", "single largest"):
        c, R, f, parts, markers, bits = parsed[name]
        assert R >= c.info.mcus_x * c.info.mcus_y and len(parts) == 1 and markers == []
        plain = jpeg.entropy_encode(c, 0)
        assert RC.scan_of(jpeg, c, f, R) == RC.scan_of(jpeg, c, plain, 0)
        assert bytes((0xFF, 0xDD, 0, 4, R >> 8, R & 255)) in f and b"\xff\xdd" not in plain[:plain.index(b"\xff\xda")]
        assert jpeg.probe(f).restart_interval == R


def test_one_eight_byte_stretch_holds_several_markers(jpeg, parsed):
    c, R, f, parts, markers, bits = parsed["zeros r1"]
    assert c.info.hs == c.info.vs == 1 and R == 1 and [len(p) for p in parts] == [2] * 12 and set(bits) == {14}
    opt = jpeg.entropy_encode(c, 1, optimize=True)
    oparts, omarkers = RC.split_scan(RC.plain_scan(opt))
    assert [len(p) for p in oparts] == [1] * 12 and set(RC.interval_bits(c, opt, 1)) == {6}, "single-symbol tables: six bits an MCU"
    c, R, f, parts, markers, bits = parsed["short r1"]
    assert {len(p) for p in parts} == {2, 3}
    ends = np.cumsum([len(p) for p in parts])[:-1]
    assert max(int(((ends >= lo) & (ends < lo + 8)).sum()) for lo in range(0, int(ends[-1]), 8)) >= 3


def test_the_dc_reset_is_visible(jpeg, parsed):
    c, R, f, parts, markers, bits = parsed["dc reset r1"]
    carried = RC.interval_bits(c, f, R, reset=False)
    assert bits[0] == carried[0] and all(b > k for b, k in zip(bits[1:], carried[1:])), "a difference near 900 takes more bits than one below 7"
    plain = RC.scan_of(jpeg, c, jpeg.entropy_encode(c, 0), 0)
    first = len(parts[0]) - 1  # (the first interval's bytes but its padded last are the plain scan's)
    assert RC.scan_of(jpeg, c, f, R)[:first] == plain[:first] and b"".join(parts) != plain.replace(b"\xff\x00", b"\xff")


def test_the_reset_decides_validity_as_the_host_coder_says(jpeg):
    for name, (c, R, valid) in RC.reset_decides(jpeg).items():
        for optimize in (False, True):
            if valid:
                assert jpeg.entropy_encode(c, R, optimize).endswith(b"\xff\xd9"), name
            else:
                with pytest.raises(jpeg._lib.ProbPoseLibraryError):
                    jpeg.entropy_encode(c, R, optimize)
    d = RC.reset_decides(jpeg)
    assert d["ramp r0"][2] and not d["ramp r3"][2] and not d["swing r0"][2] and d["swing r1"][2]
