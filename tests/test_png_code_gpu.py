"""GPU: the PNG writer's code build on the device (csrc/pp_png.hip: png_code, png_code_lz - the steps of
csrc/pp_png_code_core.h run by a workgroup) against the host builders ``pp_deflate_build_code`` / ``pp_deflate_build_code_lz``,
byte for byte; tests/test_png_code_host.py holds the same steps to the same builders on the CPU.

The kernel alone through the raw C call: one batch per mode of every named histogram of tests/png_code_ref.py and 200 random
ones in one launch, histograms and codes inside canary bytes, run twice into fresh buffers; descriptors the call skips (a
length of 0, a NULL code) among good ones; n == 0. Then end to end: ``encode_batch`` and ``zlib_compress_device`` with
``code="device"`` give the host form's bytes in both match modes with nine launches and no host build call, ``code="host"``
beside them still gives the same files; the visualizer's switch."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import png_code_ref as C  # noqa: E402
import png_lz_ref as Z  # noqa: E402
import png_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5
GUARD = 4096
TAGS_RUNS = ("png_filter", "png_clear", "png_hist", "png_bits", "png_scan", "png_zero", "png_pack", "png_crc")
TAGS_LZ = ("png_filter", "png_clear_lz", "png_parse_lz", "png_bits_lz", "png_scan_lz", "png_zero_lz", "png_pack_lz", "png_crc_lz")
ALL_TAGS = tuple(dict.fromkeys(TAGS_RUNS + TAGS_LZ + ("png_code", "png_code_lz")))


def _align(v, a=256):
    return (v + a - 1) // a * a


@pytest.fixture(scope="module")
def png():
    from probpose_code_amd import png

    return png


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


def host_codes(png, hists, lz):
    fn, CB = ("pp_deflate_build_code_lz", png.CODE_BYTES_LZ) if lz else ("pp_deflate_build_code", png.CODE_BYTES)
    hists = np.ascontiguousarray(hists, np.uint32)
    codes = np.zeros((len(hists), CB), np.uint8)
    for i in range(len(hists)):
        assert getattr(png._lib.lib, fn)(hists[i].ctypes.data, codes[i].ctypes.data) == 0
    return codes


def code_call(png, hists, lz, lens=None, no_code=()):
    """pp_png_code_batch(_lz) alone on hand-made histograms ((n, 288) or (n, 320) uint32). Every descriptor has small valid
    dummy data / scratch / out / result buffers and (unless `lens` says otherwise) a stream of one byte; descriptors in
    `no_code` get a NULL code. Histograms, codes and the dummies lie inside canary bytes; the call runs twice into fresh
    buffers. Returns the (n, CODE_BYTES) bytes of the code region."""
    _lib = png._lib
    hists = np.ascontiguousarray(hists, np.uint32)
    n = len(hists)
    HB, CB, fn, tag = (png.HIST_BYTES_LZ, png.CODE_BYTES_LZ, "pp_png_code_batch_lz", "png_code_lz") if lz else (png.HIST_BYTES, png.CODE_BYTES, "pp_png_code_batch", "png_code")
    assert hists.shape == (n, HB // 4)
    lens = [1] * n if lens is None else lens
    share = int(getattr(_lib.lib, "pp_deflate_scratch_bytes_lz" if lz else "pp_deflate_scratch_bytes")(1))
    cap = int(getattr(_lib.lib, "pp_deflate_bound_lz" if lz else "pp_deflate_bound")(1))
    assert share > 0 and cap > 0
    runs = []
    for _ in range(2):
        hist, (h_off,) = _guarded([HB * n])
        code, (c_off,) = _guarded([CB * n])
        dummy, (d_off, s_off, o_off, r_off) = _guarded([16 * n, share * n, _align(cap) * n, 16 * n])
        hist[h_off:h_off + HB * n] = torch.from_numpy(hists.view(np.uint8).reshape(-1)).to(DEV)
        hist_in, dummy_in = hist.cpu().numpy(), dummy.cpu().numpy()
        desc = np.zeros(n, png._DESC)
        for i in range(n):
            desc[i] = (0, dummy.data_ptr() + d_off + 16 * i, hist.data_ptr() + h_off + HB * i, 0 if i in no_code else code.data_ptr() + c_off + CB * i,
                       dummy.data_ptr() + s_off + share * i, dummy.data_ptr() + o_off + _align(cap) * i, dummy.data_ptr() + r_off + 16 * i, lens[i], cap,
                       0, 0, 0, 1, png._IDAT_REGISTER, 0)
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(DEV)
        torch.cuda.synchronize()
        _lib.reset_launch_counts()
        _lib.call(fn, desc_d.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert {t: _lib.launch_count(t) for t in ALL_TAGS} == {t: int(t == tag) for t in ALL_TAGS} and _lib.launch_count("pp_png.hip") == 1
        assert np.array_equal(desc_d.cpu().numpy(), desc.view(np.uint8))
        assert np.array_equal(hist.cpu().numpy(), hist_in), "the call changed a histogram or a byte beside one"
        assert np.array_equal(dummy.cpu().numpy(), dummy_in), "the call wrote a stream, a scratch share, an output or a result slot"
        code_h = code.cpu().numpy()
        assert (_outside(code_h, [c_off], [CB * n]) == CANARY).all(), "bytes outside the code structs written"
        runs.append(code_h[c_off:c_off + CB * n].reshape(n, CB).copy())
    assert np.array_equal(runs[0], runs[1]), "a second launch into fresh buffers gives other bytes"
    return runs[0]


@pytest.mark.parametrize("lz", [False, True], ids=["runs", "lz"])
def test_the_kernel_alone_gives_the_host_builders_bytes(png, lz):
    named = C.named_lz() if lz else C.named_runs()
    hists = np.concatenate([np.stack(list(named.values())), C.random_lz(200, 41) if lz else C.random_runs(200, 43)])
    names = list(named) + [f"random {i}" for i in range(200)]
    got, want = code_call(png, hists, lz), host_codes(png, hists, lz)
    bad = [(names[i], int(np.flatnonzero(got[i] != want[i])[0])) for i in range(len(hists)) if not np.array_equal(got[i], want[i])]
    assert not bad, f"{len(bad)} of {len(hists)} codes differ (name, first differing byte): {bad[:8]}"


@pytest.mark.parametrize("lz", [False, True], ids=["runs", "lz"])
def test_descriptors_the_call_skips(png, lz):
    """A stream of length 0 and a NULL code among good descriptors: the good ones are built, the slot that stood for the
    refused descriptor's code keeps its canary bytes."""
    hists = (C.random_lz if lz else C.random_runs)(4, 47)
    got, want = code_call(png, hists, lz, lens=[1, 0, 1, 1], no_code=(2,)), host_codes(png, hists, lz)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3])
    assert (got[1] == CANARY).all(), "the code of a descriptor without a stream was written"
    assert (got[2] == CANARY).all(), "the slot no descriptor named was written"
    _lib = png._lib
    _lib.reset_launch_counts()
    assert getattr(_lib.lib, "pp_png_code_batch_lz" if lz else "pp_png_code_batch")(None, 0, torch.cuda.current_stream().cuda_stream) == _lib.PP_OK
    assert _lib.launch_count("png_code") == 0 and _lib.launch_count("png_code_lz") == 0 and _lib.launch_count("pp_png.hip") == 0
    assert getattr(_lib.lib, "pp_png_code_batch_lz" if lz else "pp_png_code_batch")(None, 1, None) == _lib.PP_ERR_INVALID_ARG


def _recording(png, monkeypatch):
    """png._lib.call replaced by one that notes the names of the calls it passes on."""
    names, real = [], png._lib.call

    def call(fn, *args):
        names.append(fn)
        return real(fn, *args)

    monkeypatch.setattr(png._lib, "call", call)
    return names


@pytest.mark.parametrize("match", ["runs", "lz"])
def test_encode_batch_with_the_device_build_gives_the_host_files(png, match, monkeypatch):
    named = {**R.pictures(), **Z.pictures()}
    order = [k for k in named if k != "1x1"] + ["1x1"]  # one mixed batch, the smallest picture behind the largest
    want = [png.encode_host(named[k], channel_order="rgb", match=match) for k in order]
    tensors = [torch.from_numpy(named[k].copy()).to(DEV) for k in order]
    tags = TAGS_LZ if match == "lz" else TAGS_RUNS
    code_tag, build = ("png_code_lz", "pp_deflate_build_code_lz") if match == "lz" else ("png_code", "pp_deflate_build_code")
    assert (png.LAUNCHES_CODE_LZ if match == "lz" else png.LAUNCHES_CODE) == (code_tag,)
    names = _recording(png, monkeypatch)
    png._lib.reset_launch_counts()
    before = png.tokens_calls, png.code_calls, png.deflate_calls, png.host_calls
    got = png.encode_batch(tensors, channel_order="rgb", match=match, code="device")
    assert {t: png._lib.launch_count(t) for t in ALL_TAGS} == {t: int(t in tags or t == code_tag) for t in ALL_TAGS}
    assert png._lib.launch_count("pp_png.hip") == 9
    assert (png.tokens_calls, png.code_calls, png.deflate_calls, png.host_calls) == (before[0] + 1, before[1] + 1, before[2] + 1, before[3])
    assert not [f for f in names if f.startswith("pp_deflate_build_code")], "the device build called the host builder"
    suffix = "_lz" if match == "lz" else ""
    assert [f for f in names if f.startswith("pp_png_")] == [f"pp_png_tokens_batch{suffix}", f"pp_png_code_batch{suffix}", f"pp_png_deflate_batch{suffix}"]
    bad = [(k, len(g), len(w)) for k, g, w in zip(order, got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(order)} files differ (name, bytes, host bytes): {bad}"
    # the default beside it: the round trip, one host build per picture, the same files
    del names[:]
    png._lib.reset_launch_counts()
    assert png.encode_batch(tensors, channel_order="rgb", match=match, code="host") == want
    assert names.count(build) == len(order) and not [f for f in names if f.startswith("pp_png_code_batch")]
    assert png._lib.launch_count(code_tag) == 0 and png._lib.launch_count("pp_png.hip") == 8
    assert png.code_calls == before[1] + 1
    assert png.encode_batch(tensors[-2:], channel_order="rgb", match=match) == want[-2:], "the default is the host build"
    assert png.encode_batch([], code="device") == []


@pytest.mark.parametrize("match", ["runs", "lz"])
def test_zlib_compress_device_with_the_device_build(png, match):
    named = {**{k: (v, 0) for k, v in R.streams().items()}, **Z.streams()}
    for period in (0, 100):
        raws = [raw for raw, p in named.values() if p == period]
        assert raws
        want = [png.zlib_compress_host(r, match=match, period=period) for r in raws]
        png._lib.reset_launch_counts()
        got = png.zlib_compress_device(raws, match=match, period=period, code="device")
        assert png._lib.launch_count("pp_png.hip") == 8 and png._lib.launch_count("png_code_lz" if match == "lz" else "png_code") == 1
        assert got == want
        assert [zlib.decompress(z) for z in got] == [bytes(r) for r in raws]
        assert png.zlib_compress_device(raws, match=match, period=period, code="host") == want


@pytest.mark.parametrize("match", ["runs", "lz"])
def test_the_visualizer_switch(png, match, tmp_path):
    from probpose_code_amd.structures import InstanceData, PoseDataSample
    from probpose_code_amd.visualization import PoseLocalVisualizer

    _lib = png._lib
    rgb = R.pictures()["photo 150x201"].copy()
    rng = np.random.default_rng(3)
    ds = PoseDataSample()
    ds.pred_instances = InstanceData(keypoints=(rng.random((2, 17, 2)) * [150, 201]).astype(np.float32),
                                     keypoints_visible=np.ones((2, 17), np.float32), bboxes=np.array([[10, 10, 120, 140], [60, 20, 140, 190]], np.float32))
    files = {}
    for code in ("host", "device"):
        vis = PoseLocalVisualizer(device=DEV, png_encoder="device", png_code=code, png_match=match)
        path = str(tmp_path / f"{code}.png")
        _lib.reset_launch_counts()
        frame = vis.add_datasample("x", rgb, ds, out_file=path)
        assert _lib.launch_count("png_code_lz" if match == "lz" else "png_code") == int(code == "device")
        assert _lib.launch_count("pp_png.hip") == (9 if code == "device" else 8)
        with open(path, "rb") as f:
            files[code] = f.read()
        assert files[code] == png.encode_host(frame, channel_order="rgb", match=match)
    assert files["device"] == files["host"]
    # without the device writer the switch has no effect
    _lib.reset_launch_counts()
    PoseLocalVisualizer(device=DEV, png_code="device", png_match=match).add_datasample("x", rgb, ds, out_file=str(tmp_path / "pillow.png"))
    assert _lib.launch_count("pp_png.hip") == 0
