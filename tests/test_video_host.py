"""CPU: the Motion-JPEG AVI writer and reader (probpose_code_amd/video.py) - round trip, the RIFF structure checked by a small
walker restated here, refusals - and the host-only parts of the device entropy coder: ``pp_jpeg_write_headers`` against the
host coder's file, and ``encode_batch``'s refusals, which come before any GPU work."""
import ctypes
import io
import os
import struct

import numpy as np
import pytest


def _frames(n=5, size=(96, 64)):
    """n Pillow-made JPEG files of one size, at least one of odd and one of even byte length."""
    from PIL import Image

    out = []
    for i in range(n):
        rng = np.random.default_rng(10 + i)
        a = (np.add.outer(np.arange(size[1]) * 2, np.arange(size[0]))[:, :, None] + rng.integers(0, 40 + 30 * i, (size[1], size[0], 3))) % 256
        b = io.BytesIO()
        Image.fromarray(a.astype(np.uint8)).save(b, "JPEG", quality=70 + i)
        out.append(b.getvalue())
    return out


def _walk(data, at, end, path, found):
    """Every chunk of data[at:end) as (path, fourcc, start of its body, size); a size field must equal what follows it."""
    while at < end:
        assert at % 2 == 0, f"chunk at odd offset {at}"
        assert at + 8 <= end, f"{path}: a chunk header runs past its parent"
        cid, size = struct.unpack("<4sI", data[at:at + 8])
        assert at + 8 + size <= end, f"{path}/{cid}: size {size} runs past its parent"
        if cid in (b"RIFF", b"LIST"):
            kind = data[at + 8:at + 12]
            found.append((path, cid + b":" + kind, at + 8, size))
            _walk(data, at + 12, at + 8 + size, path + "/" + kind.decode(), found)
        else:
            found.append((path, cid, at + 8, size))
        at += 8 + size + (size & 1)
    assert at == end or at == end + 1, f"{path}: chunks end at {at}, the parent at {end}"


def test_round_trip_and_structure(tmp_path, lib_built):
    from PIL import Image

    from probpose_code_amd.video import MjpegAviWriter, read_mjpeg_avi

    frames = _frames()
    assert {len(f) % 2 for f in frames} == {0, 1}
    path = str(tmp_path / "a.avi")
    with MjpegAviWriter(path, 25) as w:
        for f in frames:
            w.write(f)
    avi = read_mjpeg_avi(path)
    assert (avi.fps, avi.width, avi.height, avi.frame_count, len(avi)) == (25.0, 96, 64, 5, 5)
    assert list(avi) == frames and list(avi) == frames  # (it can be iterated again)
    data = open(path, "rb").read()
    found = []
    _walk(data, 0, len(data), "", found)
    kinds = [(p, c) for p, c, _, _ in found]
    assert kinds[:6] == [("", b"RIFF:AVI "), ("/AVI ", b"LIST:hdrl"), ("/AVI /hdrl", b"avih"), ("/AVI /hdrl", b"LIST:strl"),
                         ("/AVI /hdrl/strl", b"strh"), ("/AVI /hdrl/strl", b"strf")]
    assert kinds[6] == ("/AVI ", b"LIST:movi") and kinds[7:12] == [("/AVI /movi", b"00dc")] * 5 and kinds[12:] == [("/AVI ", b"idx1")]
    by = {c: (o, s) for _, c, o, s in found if c != b"00dc"}
    assert by[b"RIFF:AVI "][1] == len(data) - 8
    avih = struct.unpack("<14I", data[by[b"avih"][0]:by[b"avih"][0] + 56])
    assert avih[0] == 40000 and avih[3] & 0x10 and avih[4] == 5 and avih[6] == 1 and avih[8:10] == (96, 64)
    o, s = by[b"strh"]
    assert s == 56 and data[o:o + 8] == b"vidsMJPG"
    scale, rate, _, length = struct.unpack("<4I", data[o + 20:o + 36])
    assert (rate / scale, length) == (25.0, 5)
    o, s = by[b"strf"]
    size, width, height, planes, bits, compression = struct.unpack("<IiiHH4s", data[o:o + 20])
    assert s == 40 and (size, width, height, planes, bits, compression) == (40, 96, 64, 1, 24, b"MJPG")
    movi_fourcc = by[b"LIST:movi"][0]
    o, s = by[b"idx1"]
    assert s == 16 * 5
    chunks = [(o_, s_) for _, c, o_, s_ in found if c == b"00dc"]
    for i in range(5):
        cid, flags, off, size = struct.unpack("<4sIII", data[o + 16 * i:o + 16 * i + 16])
        assert cid == b"00dc" and flags & 0x10
        at = movi_fourcc + off
        assert data[at:at + 4] == b"00dc" and struct.unpack("<I", data[at + 4:at + 8])[0] == size == len(frames[i])
        assert (at + 8, size) == chunks[i] and data[at + 8:at + 8 + size] == frames[i]
        with Image.open(io.BytesIO(data[at + 8:at + 8 + size])) as im:
            im.load()
            assert im.size == (96, 64) and im.format == "JPEG"


def test_fractional_frame_rates_survive(tmp_path, lib_built):
    from probpose_code_amd.video import MjpegAviWriter, read_mjpeg_avi

    for fps in (29.97, 30000 / 1001, 12.5):
        path = str(tmp_path / "f.avi")
        with MjpegAviWriter(path, fps) as w:
            w.write(_frames(1)[0])
        assert abs(read_mjpeg_avi(path).fps - fps) < 1e-6 * fps


def test_refusals_of_the_writer(tmp_path, lib_built):
    from probpose_code_amd.video import MjpegAviWriter, read_mjpeg_avi

    frames, other = _frames(3), _frames(1, size=(64, 96))[0]
    path = str(tmp_path / "b.avi")
    with MjpegAviWriter(path, 30) as w:
        w.write(frames[0])
        with pytest.raises(ValueError, match="64 x 96"):
            w.write(other)
        with pytest.raises(ValueError, match="not a JPEG"):
            w.write(b"RIFF not a picture")
        w.write(frames[1])
    assert list(read_mjpeg_avi(path)) == frames[:2]
    # a limit that admits two frames and their index but not the third
    limit = 224 + sum(8 + len(f) + len(f) % 2 for f in frames[:2]) + 8 + 16 * 2 + 20
    path = str(tmp_path / "c.avi")
    w = MjpegAviWriter(path, 30, max_bytes=limit)
    w.write(frames[0])
    w.write(frames[1])
    with pytest.raises(ValueError, match="max_bytes"):
        w.write(frames[2])
    w.close()
    assert os.path.getsize(path) <= limit
    avi = read_mjpeg_avi(path)
    assert avi.frame_count == 2 and list(avi) == frames[:2]
    data = open(path, "rb").read()
    _walk(data, 0, len(data), "", [])
    for bad in (0, -1.0):
        with pytest.raises(ValueError):
            MjpegAviWriter(str(tmp_path / "d.avi"), bad)


def test_refusals_of_the_reader(tmp_path, lib_built):
    from probpose_code_amd.video import MjpegAviWriter, read_mjpeg_avi

    path = str(tmp_path / "x.avi")
    open(path, "wb").write(b"\xff\xd8 not an AVI file at all, just bytes")
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        read_mjpeg_avi(path)
    open(path, "wb").write(b"RIFF\x04\0\0\0WAVE")
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        read_mjpeg_avi(path)
    good = str(tmp_path / "g.avi")
    with MjpegAviWriter(good, 25) as w:
        w.write(_frames(1)[0])
    data = open(good, "rb").read()
    assert data.count(b"MJPG") == 2
    strf_only = data[::-1].replace(b"GPJM", b"462H", 1)[::-1]  # (the last of the two: biCompression)
    assert strf_only.count(b"vidsMJPG") == 1
    for patched in (data.replace(b"vidsMJPG", b"vidsH264"), data.replace(b"MJPG", b"H264"), strf_only):
        open(path, "wb").write(patched)
        with pytest.raises(ValueError, match="Motion-JPEG"):
            read_mjpeg_avi(path)


def test_encode_batch_refuses_other_entropy_settings_without_a_gpu(lib_built):
    from probpose_code_amd import _lib, jpeg

    img = np.zeros((8, 8, 3), np.uint8)
    _lib.reset_launch_counts()
    calls = (jpeg.entropy_device_calls, jpeg.forward_calls)
    with pytest.raises(ValueError, match="entropy"):
        jpeg.encode_batch([img], entropy="gpu")
    with pytest.raises(ValueError, match="restart"):
        jpeg.encode_batch([img], entropy="device", restart_interval=4)
    assert _lib.launch_count("pp_jpeg_enc.hip") == 0 and _lib.launch_count("pp_jpeg_entropy.hip") == 0
    assert (jpeg.entropy_device_calls, jpeg.forward_calls) == calls


def test_write_headers_is_a_prefix_of_the_host_coders_file(lib_built):
    from probpose_code_amd import _lib, jpeg

    rng = np.random.default_rng(4)
    for ss in ("4:4:4", "4:2:2", "4:2:0"):
        for tables in ("equal", "different"):
            info = jpeg.encode_plan(37, 21, ss)
            qt = jpeg.quality_tables(60)
            if tables == "different":
                qt[2] = np.clip(qt[2] + 3, 1, 255)
            coef = np.where(rng.random(int(info.coef_count)) < 0.1, rng.integers(-200, 201, int(info.coef_count)), 0).astype(np.int16)
            file = jpeg.entropy_encode(jpeg.JpegCoefficients(info, coef, qt))
            head = jpeg.write_headers(qt, info)
            assert file.startswith(head) and head.endswith(bytes([0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
            assert head.count(b"\xff\xdb") == (2 if tables == "equal" else 3)
            with_dri = jpeg.write_headers(qt, info, restart_interval=5)
            assert jpeg.entropy_encode(jpeg.JpegCoefficients(info, coef, qt), restart_interval=5).startswith(with_dri) and len(with_dri) == len(head) + 6
    info = jpeg.encode_plan(8, 8, "4:2:0")
    with pytest.raises(_lib.ProbPoseLibraryError):
        jpeg.write_headers(np.zeros((3, 64), np.uint16), info)  # a table value of 0
    size = ctypes.c_size_t(0)
    out = np.empty(100, np.uint8)
    st = _lib.lib.pp_jpeg_write_headers(jpeg.quality_tables(75).ctypes.data, ctypes.byref(info), 0, out.ctypes.data, out.size, ctypes.byref(size))
    assert st == _lib.PP_ERR_WORKSPACE and size.value == 0


def test_the_demo_reads_a_directory_in_sorted_order_and_an_avi(tmp_path, lib_built):
    import sys

    from probpose_code_amd.video import MjpegAviWriter

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "demo"))
    import video_demo

    frames = _frames(3)
    d = tmp_path / "frames"
    d.mkdir()
    for name, f in zip(("b.jpg", "a.JPG", "c.jpeg"), frames):
        (d / name).write_bytes(f)
    (d / "notes.txt").write_text("not a frame")
    got, fps = video_demo.frame_source(str(d))
    assert fps is None and list(got) == [frames[1], frames[0], frames[2]]  # a.JPG, b.jpg, c.jpeg
    path = str(tmp_path / "v.avi")
    with MjpegAviWriter(path, 15) as w:
        for f in frames:
            w.write(f)
    got, fps = video_demo.frame_source(path)
    assert fps == 15.0 and list(got) == frames
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="no .jpg"):
        video_demo.frame_source(str(empty))
