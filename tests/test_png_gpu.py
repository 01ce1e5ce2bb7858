"""GPU: the device PNG writer (csrc/pp_png.hip) against its own host form (``png.encode_host``, ``png.zlib_compress_host``: the
sequential run of the same core) - every comparison is byte for byte - and against Pillow, which opens the files to the
pixels. The pictures of tests/png_ref.py and one 640 x 480 frame as ONE mixed batch through the raw C calls, every scratch
share, stream, histogram, code and result slot inside canary bytes, coded twice into fresh buffers; the deflate stage alone
on the raw streams; a capacity one byte short; strided views; ``encode_batch`` and the visualizer's switch by launch counts.

The coder's work is divided in tiles of 4096 bytes of the filtered stream. 150 x 201 has 90 651 bytes (23 tiles, the last of
539 bytes), rows of 1365 and 1366 pixels have 4096 and 4099 bytes, the 640 x 480 frame has 226 tiles: the scans over tiles
and the 64-bit prefix sums cross workgroup edges, and runs meet tile borders."""
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import png_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5
GUARD = 4096
TAGS = ("png_filter", "png_clear", "png_hist", "png_bits", "png_scan", "png_zero", "png_pack", "png_crc")


def _align(v, a=256):
    return (v + a - 1) // a * a


@pytest.fixture(scope="module")
def png():
    from probpose_code_amd import png

    return png


_SET = {}


def picture_set(png):
    """{name: (RGB picture, its host file)}: the shared pictures and one 640 x 480 frame, coded on the host once."""
    if not _SET:
        rng = np.random.default_rng(21)
        yy, xx = np.mgrid[0:480, 0:640]
        frame = 120 + 80 * np.sin(xx / 41.0) * np.cos(yy / 29.0) + 25 * np.cos((3 * xx - yy) / 17.0)
        frame = np.clip(frame[:, :, None] + np.array([5, -14, 20]) + rng.normal(0, 2, (480, 640, 3)), 0, 255).astype(np.uint8)
        frame[400:, :300] = 255  # a flat corner: long runs beside noise
        frame.setflags(write=False)
        for name, rgb in list(R.pictures().items()) + [("frame 640x480", frame)]:
            _SET[name] = (rgb, png.encode_host(rgb, channel_order="rgb"))
    return _SET


def _guarded(sizes):
    """A canary-filled device buffer with a region of each size, GUARD bytes before, between and behind them."""
    offs, at = [], GUARD
    for s in sizes:
        offs.append(at)
        at += _align(s) + GUARD
    t = torch.full((at,), CANARY, dtype=torch.uint8, device=DEV)
    assert t.data_ptr() % 256 == 0
    return t, offs


def _outside(host, offs, sizes):
    mask = np.ones(host.size, bool)
    for o, s in zip(offs, sizes):
        mask[o:o + s] = False
    return host[mask]


def raw_call(png, items, capacities=None, rgb=1):
    """pp_png_tokens_batch, the code build and pp_png_deflate_batch on buffers of this test's own. items: (H, W, 3) uint8
    device tensors (views with whole pixels, any row stride) or bytes. Everything the kernels may write lies inside canary
    bytes; the calls run twice, the second time into fresh buffers. Returns [(status, bytes, crc, stream)]."""
    _lib = png._lib
    n = len(items)
    lens = [len(x) if isinstance(x, bytes) else x.shape[0] * (1 + 3 * x.shape[1]) for x in items]
    shares = [int(_lib.lib.pp_deflate_scratch_bytes(ln)) for ln in lens]
    assert min(shares) > 0 and all(s % 256 == 0 for s in shares)
    if capacities is None:
        capacities = [int(_lib.lib.pp_deflate_bound(ln)) for ln in lens]
    pictures = [x for x in items if not isinstance(x, bytes)]
    bases = [x._base if x._base is not None else x for x in pictures]
    before = [b.clone() for b in bases]
    runs = []
    for _ in range(2):
        scratch, s_off = _guarded(shares)
        out, o_off = _guarded(capacities)
        data, d_off = _guarded(lens)
        res, (r_off,) = _guarded([16 * n])
        hist, (h_off,) = _guarded([png.HIST_BYTES * n])
        code, (c_off,) = _guarded([png.CODE_BYTES * n])
        for x, o in zip(items, d_off):
            if isinstance(x, bytes):
                data[o:o + len(x)] = torch.from_numpy(np.frombuffer(x, np.uint8).copy()).to(DEV)
        data_in = data.cpu().numpy()
        desc = np.zeros(n, png._DESC)
        for i, x in enumerate(items):
            raw = isinstance(x, bytes)
            desc[i] = (0 if raw else x.data_ptr(), data.data_ptr() + d_off[i], hist.data_ptr() + h_off + png.HIST_BYTES * i,
                       code.data_ptr() + c_off + png.CODE_BYTES * i, scratch.data_ptr() + s_off[i], out.data_ptr() + o_off[i],
                       res.data_ptr() + r_off + 16 * i, lens[i], capacities[i], 0 if raw else x.shape[1], 0 if raw else x.shape[0],
                       0 if raw else x.stride(0), rgb, png._IDAT_REGISTER, 0)
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(DEV)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.reset_launch_counts()
        _lib.call("pp_png_tokens_batch", desc_d.data_ptr(), n, max([x.shape[0] for x in pictures], default=0), max(lens), stream)
        torch.cuda.synchronize()
        hist_h = hist.cpu().numpy()
        assert (_outside(hist_h, [h_off], [png.HIST_BYTES * n]) == CANARY).all(), "bytes outside the histograms written"
        codes = np.zeros(png.CODE_BYTES * n, np.uint8)
        counts = np.ascontiguousarray(hist_h[h_off:h_off + png.HIST_BYTES * n])
        for i in range(n):
            _lib.call("pp_deflate_build_code", counts.ctypes.data + png.HIST_BYTES * i, codes.ctypes.data + png.CODE_BYTES * i)
        code[c_off:c_off + codes.size] = torch.from_numpy(codes).to(DEV)
        _lib.call("pp_png_deflate_batch", desc_d.data_ptr(), n, max(lens), stream)
        torch.cuda.synchronize()
        want = [1 if (t != "png_filter" or pictures) else 0 for t in TAGS]
        assert [_lib.launch_count(t) for t in TAGS] == want and _lib.launch_count("pp_png.hip") == sum(want)
        assert np.array_equal(desc_d.cpu().numpy(), desc.view(np.uint8))
        for b, was in zip(bases, before):
            assert torch.equal(b, was), "the kernels changed a picture"
        scratch_h, out_h, res_h, data_h, code_h = (t.cpu().numpy() for t in (scratch, out, res, data, code))
        assert (_outside(scratch_h, s_off, shares) == CANARY).all(), "bytes outside the scratch shares written"
        assert (_outside(res_h, [r_off], [16 * n]) == CANARY).all(), "bytes outside the result slots written"
        assert (_outside(data_h, d_off, lens) == CANARY).all(), "bytes outside the filtered streams written"
        assert np.array_equal(hist.cpu().numpy(), hist_h), "the second half changed a histogram"
        assert (_outside(code_h, [c_off], [codes.size]) == CANARY).all() and np.array_equal(code_h[c_off:c_off + codes.size], codes)
        for x, o in zip(items, d_off):
            if isinstance(x, bytes):
                assert np.array_equal(data_h[o:o + len(x)], data_in[o:o + len(x)]), "the kernels changed a raw stream"
        slots = res_h[r_off:r_off + 16 * n].view(png._RESULT)
        used, got = [], []
        for o, cap, r in zip(o_off, capacities, slots):
            status, size = int(r["status"]), int(r["bytes"])
            used.append(size if status == _lib.PP_OK else 0)
            assert 0 <= used[-1] <= cap
            got.append((status, size, int(r["crc"]), out_h[o:o + used[-1]].tobytes()))
        assert (_outside(out_h, o_off, used) == CANARY).all(), "bytes behind a stream, or of a stream that did not fit, written"
        runs.append(got)
    assert runs[0] == runs[1], "a second launch into fresh buffers gives other bytes"
    return runs[0]


def test_one_mixed_batch_gives_the_host_files_and_pillow_opens_them(png):
    from PIL import Image

    named = picture_set(png)
    order = [k for k in named if k != "1x1"] + ["1x1"]  # the smallest picture behind the largest
    tensors = [torch.from_numpy(named[k][0].copy()).to(DEV) for k in order]
    got = raw_call(png, tensors)
    bad = []
    for k, t, (status, size, crc, stream) in zip(order, tensors, got):
        rgb, want = named[k]
        data = png._frame(rgb.shape[1], rgb.shape[0], stream, crc)
        if status != 0 or data != want:
            first = next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), min(len(data), len(want)))
            bad.append((k, status, len(data), len(want), first))
            continue
        assert len(data) <= int(png._lib.lib.pp_png_encoded_bound(rgb.shape[1], rgb.shape[0]))
        with Image.open(io.BytesIO(data)) as im:
            assert (im.format, im.mode, im.size) == ("PNG", "RGB", (rgb.shape[1], rgb.shape[0]))
            assert np.array_equal(np.asarray(im), rgb), k
    assert not bad, f"{len(bad)} of {len(order)} files differ (name, status, bytes, host bytes, first difference): {bad}"


def test_a_picture_alone_and_bgr_order(png):
    """n = 1: the grids are sized by the picture itself; B, G, R in memory gives the file of the R, G, B picture."""
    rgb, want = picture_set(png)["photo 150x201"]
    for order, px in ((1, rgb), (0, rgb[:, :, ::-1])):
        (status, size, crc, stream), = raw_call(png, [torch.from_numpy(px.copy()).to(DEV)], rgb=order)
        assert status == 0 and png._frame(150, 201, stream, crc) == want


def test_views_with_a_row_stride_are_read_in_place(png):
    rgb, _ = picture_set(png)["frame 640x480"]
    base = torch.from_numpy(rgb.copy()).to(DEV)
    crop = base[37:188, 100:301]  # 151 rows of 201 pixels, 1920 bytes from row to row
    assert crop.stride(0) == 1920 and crop._base is base
    (status, size, crc, stream), = raw_call(png, [crop])
    want = png.encode_host(rgb[37:188, 100:301], channel_order="rgb")
    assert status == 0 and png._frame(201, 151, stream, crc) == want
    rows = base[11:111]  # a vertical crop: whole rows, which encode_batch hands over as they lie
    png._lib.reset_launch_counts()
    assert png.encode_batch([rows], channel_order="rgb") == [png.encode_host(rgb[11:111], channel_order="rgb")]
    assert torch.equal(base.cpu(), torch.from_numpy(rgb.copy()))


def test_the_deflate_stage_alone_equals_the_host_form(png):
    named = R.streams()
    got = raw_call(png, list(named.values()))
    for (name, raw), (status, size, crc, stream) in zip(named.items(), got):
        assert status == 0 and stream == png.zlib_compress_host(raw), name
        assert zlib.decompress(stream) == raw, name
        assert (~crc & 0xFFFFFFFF) == zlib.crc32(b"IDAT" + stream), name
    png._lib.reset_launch_counts()
    before = png.tokens_calls, png.deflate_calls
    assert png.zlib_compress_device(list(named.values())) == [s for _, _, _, s in got]
    assert (png.tokens_calls, png.deflate_calls) == (before[0] + 1, before[1] + 1)
    assert [png._lib.launch_count(t) for t in TAGS] == [0, 1, 1, 1, 1, 1, 1, 1]


def test_a_capacity_one_byte_short_is_reported_and_nothing_is_written(png):
    rgb, want = picture_set(png)["photo 150x201"]
    small, want_small = picture_set(png)["1x7"]
    need = len(want) - 57  # the file without its framing: the zlib stream
    tensors = [torch.from_numpy(rgb.copy()).to(DEV), torch.from_numpy(small.copy()).to(DEV)]
    got = raw_call(png, tensors, capacities=[need - 1, int(png._lib.lib.pp_deflate_bound(22))])
    assert got[0][:2] == (png._lib.PP_ERR_WORKSPACE, need) and got[0][3] == b""
    assert got[1][0] == 0 and png._frame(7, 1, got[1][3], got[1][2]) == want_small
    exact = raw_call(png, tensors[:1], capacities=[need])
    assert exact[0][0] == 0 and png._frame(150, 201, exact[0][3], exact[0][2]) == want


def test_encode_batch_gives_the_host_files_in_eight_launches(png):
    from probpose_code_amd import jpeg

    named = picture_set(png)
    pictures = [named[k][0] for k in named]
    tensors = [torch.from_numpy(p.copy()).to(DEV) if i % 2 else p.copy() for i, p in enumerate(pictures)]  # device tensors and host arrays
    before = png.tokens_calls, png.deflate_calls, png.host_calls, jpeg.forward_calls
    assert png.LAUNCHES_TOKENS + png.LAUNCHES_DEFLATE == TAGS  # what the module documents
    png._lib.reset_launch_counts()
    files = png.encode_batch(tensors, channel_order="rgb")
    assert [png._lib.launch_count(t) for t in TAGS] == [1] * 8 and png._lib.launch_count("pp_png.hip") == 8
    assert (png.tokens_calls, png.deflate_calls, png.host_calls, jpeg.forward_calls) == (before[0] + 1, before[1] + 1, before[2], before[3])
    assert files == [named[k][1] for k in named]
    assert png.encode_batch(tensors, channel_order="rgb") == files
    for t, p in zip(tensors, pictures):
        assert np.array_equal(t.cpu().numpy() if isinstance(t, torch.Tensor) else t, p)
    bgr = torch.from_numpy(np.ascontiguousarray(pictures[3][:, :, ::-1])).to(DEV)
    assert png.encode_batch([bgr]) == [files[3]]
    assert png.encode_batch([]) == []


def test_imwrite_device_writes_the_file(png, tmp_path):
    rgb, want = picture_set(png)["demo picture"]
    path = str(tmp_path / "demo.png")
    png.imwrite_device(path, torch.from_numpy(rgb.copy()).to(DEV), channel_order="rgb")
    with open(path, "rb") as f:
        assert f.read() == want


def test_visualizer_writes_png_with_the_device_kernels_only_when_asked(png, tmp_path):
    from PIL import Image

    from probpose_code_amd.structures import InstanceData, PoseDataSample
    from probpose_code_amd.visualization import PoseLocalVisualizer

    _lib = png._lib
    rgb = picture_set(png)["photo 150x201"][0].copy()
    rng = np.random.default_rng(3)
    ds = PoseDataSample()
    ds.pred_instances = InstanceData(keypoints=(rng.random((2, 17, 2)) * [150, 201]).astype(np.float32),
                                     keypoints_visible=np.ones((2, 17), np.float32), bboxes=np.array([[10, 10, 120, 140], [60, 20, 140, 190]], np.float32))
    shown = {}
    for kind in ("host", "device"):
        vis = PoseLocalVisualizer(device=DEV) if kind == "host" else PoseLocalVisualizer(device=DEV, png_encoder="device")
        for ext in ("png", "jpg"):
            path = str(tmp_path / f"{kind}.{ext}")
            _lib.reset_launch_counts()
            frame = vis.add_datasample("x", rgb, ds, out_file=path)
            used = _lib.launch_count("pp_png.hip")
            assert used == (8 if (kind, ext) == ("device", "png") else 0), (kind, ext, used)
            assert _lib.launch_count("jpeg_enc_color") == 0
            with Image.open(path) as im:
                assert im.format == ("JPEG" if ext == "jpg" else "PNG")
                shown[kind, ext] = np.asarray(im.convert("RGB"))
            if ext == "png":
                assert np.array_equal(shown[kind, ext], frame)
    assert not np.array_equal(shown["host", "png"], rgb), "nothing was drawn"
    assert np.array_equal(shown["host", "png"], shown["device", "png"])
    with open(str(tmp_path / "device.png"), "rb") as f:
        assert f.read() == png.encode_host(shown["device", "png"], channel_order="rgb")
