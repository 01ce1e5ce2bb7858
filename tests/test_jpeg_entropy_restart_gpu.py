"""GPU: the device Huffman coder with restart intervals (pp_jpeg_entropy_encode_restart_batch and
pp_jpeg_entropy_encode_opt_restart_batch, csrc/pp_jpeg_entropy.hip / pp_jpeg_entropy_opt.hip) against the host coder
``jpeg.entropy_encode(c, R, optimize)`` on the same coefficients - byte for byte, no tolerance anywhere. The hand-made sets of
tests/jpeg_entropy_restart_cases.py (whose forms tests/test_jpeg_entropy_restart_host.py proves) and a dozen real pictures as
ONE mixed batch with an interval of its own per image; intervals that straddle the 256-block chunks and markers next to the
2048-byte stuffing chunks; every stream, scratch share and record inside canary bytes, each call run twice into fresh
buffers; images that the reset alone makes invalid or valid; an interval out of range; a capacity one byte short; the launch
counts; and the writer end to end - ``encode_batch(restart_rows=)`` against the host path, through Pillow, back through the
device Huffman decoder, and as the frames of demo/video_demo.py."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import jpeg_enc_ref as E  # noqa: E402
import jpeg_entropy_restart_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5
GUARD = 4096
CFG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")
# the launches the header states for the two calls, and those of the calls without intervals
RST_TAGS = ("jpeg_ent_rst_bits", "jpeg_ent_rst_scan", "jpeg_ent_rst_zero", "jpeg_ent_rst_pack", "jpeg_ent_rst_ffcount", "jpeg_ent_rst_ffscan",
            "jpeg_ent_rst_stuff")
OPT_RST_TAGS = ("jpeg_opt_clear", "jpeg_opt_rst_hist", "jpeg_opt_build", "jpeg_opt_rst_bits", "jpeg_opt_rst_scan", "jpeg_opt_rst_zero",
                "jpeg_opt_rst_pack", "jpeg_opt_rst_ffcount", "jpeg_opt_rst_ffscan", "jpeg_opt_rst_stuff")
ENT_TAGS = ("jpeg_ent_bits", "jpeg_ent_scan", "jpeg_ent_zero", "jpeg_ent_pack", "jpeg_ent_ffcount", "jpeg_ent_ffscan", "jpeg_ent_stuff")
OPT_TAGS = ("jpeg_opt_clear", "jpeg_opt_hist", "jpeg_opt_build", "jpeg_opt_bits", "jpeg_opt_scan", "jpeg_opt_zero", "jpeg_opt_pack",
            "jpeg_opt_ffcount", "jpeg_opt_ffscan", "jpeg_opt_stuff")


def _align(v, a=256):
    return (v + a - 1) // a * a


@pytest.fixture(scope="module")
def jpeg():
    from probpose_code_amd import jpeg

    return jpeg


_HOST = {}


def host_scan(jpeg, name, c, R, optimize):
    """The scan bytes of the host coder's file, or None where it refuses the coefficients; computed once per case."""
    key = (name, R, optimize)
    if key not in _HOST:
        try:
            _HOST[key] = RC.plain_scan(jpeg.entropy_encode(c, R, optimize))
        except jpeg._lib.ProbPoseLibraryError:
            _HOST[key] = None
    return _HOST[key]


def _guarded(sizes):
    """A canary-filled device buffer with a region of each size, GUARD bytes before, between and behind them."""
    offs, at = [], GUARD
    for s in sizes:
        offs.append(at)
        at += _align(s) + GUARD
    t = torch.full((at,), CANARY, dtype=torch.uint8, device=DEV)
    assert t.data_ptr() % 256 == 0
    return t, offs


def _outside(buf, offs, sizes):
    mask = np.ones(buf.size, bool)
    for o, s in zip(offs, sizes):
        mask[o:o + s] = False
    return buf[mask]


def raw_restart(jpeg, coefs, intervals, optimize, capacities=None):
    """One of the two new calls on buffers of this test's own: every scratch share, stream, record and the result slots inside
    canary bytes. Runs the call twice, the second time into fresh buffers, and asserts the same bytes, untouched coefficients and
    the header's launch count. Returns [(status, bytes, stream)]."""
    _lib = jpeg._lib
    n = len(coefs)
    infos = [c.info for c in coefs]
    shares = [int(_lib.lib.pp_jpeg_entropy_restart_scratch_bytes(ctypes.byref(i), 1)) for i in infos]
    assert min(shares) > 0 and all(s % 256 == 0 for s in shares)
    if capacities is None:
        capacities = [int(_lib.lib.pp_jpeg_encoded_bound(ctypes.byref(i))) for i in infos]
    rec_bytes = jpeg._OPT_RECORD.itemsize
    c_off, at = [], 0
    for c in coefs:
        c_off.append(at)
        at = _align(at + 2 * c.coef.size)
    coef_host = np.full(at, 0x5A, np.uint8)
    for o, c in zip(c_off, coefs):
        coef_host[o:o + 2 * c.coef.size] = np.ascontiguousarray(c.coef, np.int16).view(np.uint8)
    coef_d = torch.from_numpy(coef_host).to(DEV)
    name = "pp_jpeg_entropy_encode_opt_restart_batch" if optimize else "pp_jpeg_entropy_encode_restart_batch"
    runs = []
    for _ in range(2):
        scratch, s_off = _guarded(shares)
        out, o_off = _guarded(capacities)
        res, (r_off,) = _guarded([16 * n])
        rec, k_off = _guarded([rec_bytes] * n)
        desc = np.zeros(n, jpeg._ENT_OPT_RESTART_DESC if optimize else jpeg._ENT_RESTART_DESC)
        for i, info in enumerate(infos):
            row = (coef_d.data_ptr() + c_off[i], scratch.data_ptr() + s_off[i], out.data_ptr() + o_off[i], res.data_ptr() + r_off + 16 * i,
                   capacities[i], info.hs, info.vs, info.mcus_x, info.mcus_y, intervals[i], 0)
            desc[i] = row + (rec.data_ptr() + k_off[i],) if optimize else row
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(DEV)
        _lib.reset_launch_counts()
        _lib.call(name, desc_d.data_ptr(), n, max(int(i.coef_count) // 64 for i in infos), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        if optimize:
            assert [_lib.launch_count(t) for t in OPT_RST_TAGS] == [1] * 10 and _lib.launch_count("pp_jpeg_entropy_opt.hip") == 10
            assert _lib.launch_count("pp_jpeg_entropy.hip") == 0 and _lib.launch_count("jpeg_opt_hist") == 0
        else:
            assert [_lib.launch_count(t) for t in RST_TAGS] == [1] * 7 and _lib.launch_count("pp_jpeg_entropy.hip") == 7
            assert _lib.launch_count("pp_jpeg_entropy_opt.hip") == 0
        assert [_lib.launch_count(t) for t in ENT_TAGS] == [0] * 7
        assert np.array_equal(coef_d.cpu().numpy(), coef_host), "the kernels changed the coefficients"
        assert np.array_equal(desc_d.cpu().numpy(), desc.view(np.uint8))
        scratch_h, out_h, res_h, rec_h = scratch.cpu().numpy(), out.cpu().numpy(), res.cpu().numpy(), rec.cpu().numpy()
        assert (_outside(scratch_h, s_off, shares) == CANARY).all(), "bytes outside the scratch shares written"
        assert (_outside(res_h, [r_off], [16 * n]) == CANARY).all(), "bytes outside the result slots written"
        assert (_outside(rec_h, k_off, [rec_bytes if optimize else 0] * n) == CANARY).all(), "bytes outside the records written"
        slots = res_h[r_off:r_off + 16 * n].view(jpeg._ENT_RESULT)
        used, got = [], []
        for o, cap, r in zip(o_off, capacities, slots):
            status, size = int(r["status"]), int(r["bytes"])
            u = size if status == _lib.PP_OK else (0 if status == _lib.PP_ERR_WORKSPACE else min(max(size, 0), cap))
            assert 0 <= u <= cap
            used.append(u)
            got.append((status, size, out_h[o:o + u].tobytes()))
        assert (_outside(out_h, o_off, used) == CANARY).all(), "bytes behind a stream written"
        runs.append(got)
    ok = [g[0] == _lib.PP_OK for g in runs[0]]
    assert [g[0] for g in runs[0]] == [g[0] for g in runs[1]], "a second launch gives another status"
    assert [g for g, k in zip(runs[0], ok) if k] == [g for g, k in zip(runs[1], ok) if k], "a second launch into fresh buffers gives other bytes"
    return runs[0]


def check_batch(jpeg, named, both=(False, True)):
    """named: [(name, JpegCoefficients, R)] coded as one batch by both new calls; every stream equals the host coder's."""
    for optimize in both:
        got = raw_restart(jpeg, [c for _, c, _ in named], [R for _, _, R in named], optimize)
        bad = []
        for (name, c, R), (status, size, stream) in zip(named, got):
            want = host_scan(jpeg, name, c, R, optimize)
            assert want is not None, name
            if status != 0 or size != len(want) or stream != want:
                first = next((i for i, (a, b) in enumerate(zip(stream, want)) if a != b), min(len(stream), len(want)))
                bad.append((name, R, status, size, len(want), first))
        assert not bad, f"optimize={optimize}: {len(bad)} of {len(named)} streams differ (name, R, status, bytes, host bytes, first difference): {bad[:8]}"


_REAL = {}


def real(jpeg, content, W, H, ss, q):
    """JpegCoefficients of forward_batch on a test picture, computed once."""
    key = (content, W, H, ss, q)
    if key not in _REAL:
        (_REAL[key],) = jpeg.forward_batch([torch.from_numpy(E.image(content, W, H).copy()).to(DEV)], q, ss, "rgb")
    return _REAL[key]


def _mcus(c):
    return c.info.mcus_x * c.info.mcus_y


def test_hand_made_sets_and_real_pictures_as_one_mixed_batch(jpeg):
    named = [(name, c, R) for name, (c, R) in RC.hand_made(jpeg).items()]
    pictures = [("noise", 250, 130, "4:2:0", 100, 5), ("noise", 250, 130, "4:4:4", 75, 1), ("gradient", 250, 130, "4:2:2", 75, 16),
                ("checker", 96, 64, "4:2:0", 50, 6), ("noise", 96, 64, "4:2:2", 100, 0), ("gradient", 96, 64, "4:4:4", 1, 7),
                ("noise", 17, 33, "4:2:0", 75, 2), ("checker", 17, 33, "4:4:4", 100, 3), ("gradient", 9, 17, "4:2:2", 50, 1),
                ("noise", 16, 16, "4:2:0", 75, 65535), ("checker", 250, 130, "4:4:4", 100, 9), ("noise", 8, 8, "4:4:4", 75, 1)]
    for content, W, H, ss, q, R in pictures:
        named.append((f"{content} {W}x{H} {ss} q{q}", real(jpeg, content, W, H, ss, q), R))
    largest = max(range(len(named)), key=lambda i: named[i][1].coef.size)
    assert _mcus(named[-1][1]) == 1 and largest < len(named) - 1, "a 1-MCU image sits behind the largest"
    named.insert(largest + 1, named.pop())
    assert _mcus(named[largest + 1][1]) == 1
    intervals = [R for _, _, R in named]
    assert 0 in intervals and len(set(intervals)) >= 8 and len(pictures) == 12
    check_batch(jpeg, named)
    # the same images with interval 0 throughout: the bytes of the calls without intervals
    zero = [(name, c, 0) for name, c, _ in named[::3]]
    check_batch(jpeg, zero)
    assert jpeg.entropy_encode_device([c for _, c, _ in zero], DEV) == [jpeg.entropy_encode(c) for _, c, _ in zero]


def test_intervals_that_straddle_the_chunks_of_256_blocks(jpeg):
    named = []
    for ss, R in (("4:2:0", 5), ("4:2:2", 7), ("4:4:4", 3), ("4:2:0", 43)):
        c = real(jpeg, "noise", 250, 130, ss, 75)
        bpi, nblk = R * (c.info.hs * c.info.vs + 2), c.coef.size // 64
        starts = range(0, nblk, bpi)
        assert nblk > 3 * RC.ENT_CHUNK and RC.ENT_CHUNK % bpi != 0
        assert sum(s // RC.ENT_CHUNK != (min(s + bpi, nblk) - 1) // RC.ENT_CHUNK for s in starts) >= 3, "intervals with blocks in two chunks"
        named.append((f"noise 250x130 {ss} q75", c, R))
    check_batch(jpeg, named)
    for one in named[:2]:
        check_batch(jpeg, [one])  # (n = 1: the grids are sized by the image itself)


def test_markers_within_eight_bytes_of_a_stuffing_chunk_edge(jpeg):
    """Found by reading the host coder's streams: pictures and intervals whose unstuffed stream is several chunks of 2048 bytes
    with an interval end at most eight bytes from a chunk edge, on either side."""
    found = {"before": [], "behind": []}
    for ss in ("4:4:4", "4:2:2", "4:2:0"):
        c = real(jpeg, "noise", 250, 130, ss, 100)
        name = f"noise 250x130 {ss} q100"
        for R in (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13):
            parts, _ = RC.split_scan(host_scan(jpeg, name, c, R, False))
            ends = np.cumsum([len(p) for p in parts])[:-1]
            assert ends[-1] > 4 * RC.STUFF_CHUNK
            off = ends % RC.STUFF_CHUNK
            if ((off >= RC.STUFF_CHUNK - 8) & (ends > RC.STUFF_CHUNK)).any():
                found["before"].append((name, c, R))
            if ((off <= 8) & (ends > RC.STUFF_CHUNK)).any():
                found["behind"].append((name, c, R))
    assert found["before"] and found["behind"], {k: len(v) for k, v in found.items()}
    check_batch(jpeg, found["before"][:3] + found["behind"][:3])


def test_the_reset_alone_makes_an_image_invalid_or_valid(jpeg):
    _lib = jpeg._lib
    cases = RC.reset_decides(jpeg)
    good = RC.hand_made(jpeg)["ragged r3"]
    named = [("ragged r3", good[0], good[1])] + [(name, c, R) for name, (c, R, _) in cases.items()] + [("ragged r3", good[0], good[1])]
    for optimize in (False, True):
        got = raw_restart(jpeg, [c for _, c, _ in named], [R for _, _, R in named], optimize)
        for (name, c, R), (status, size, stream) in zip(named, got):
            want = host_scan(jpeg, name, c, R, optimize)
            if name in cases:
                assert (want is not None) == cases[name][2], name
            if want is None:
                assert status == _lib.PP_ERR_INVALID_ARG, (name, optimize, status)
            else:
                assert (status, size, stream) == (_lib.PP_OK, len(want), want), (name, optimize, status, size, len(want))
    with pytest.raises(_lib.ProbPoseLibraryError, match="image 1"):
        jpeg.entropy_encode_device([good[0], cases["ramp r3"][0]], DEV, restart_interval=[3, 3])
    assert jpeg.entropy_encode_device([cases["swing r1"][0]], DEV, restart_interval=1) == [jpeg.entropy_encode(cases["swing r1"][0], 1)]


def test_an_interval_out_of_range_fails_its_image_alone(jpeg):
    _lib = jpeg._lib
    sets = RC.hand_made(jpeg)
    a, b = sets["phases r1"], sets["ragged r2"]
    for optimize in (False, True):
        for bad in (-1, 65536, 2 ** 31 - 1, -2 ** 31):
            got = raw_restart(jpeg, [a[0], b[0], a[0]], [a[1], bad, a[1]], optimize)
            assert got[1][0] == _lib.PP_ERR_INVALID_ARG and got[1][1] == 0 and got[1][2] == b"", (optimize, bad, got[1][:2])
            want = host_scan(jpeg, "phases r1", a[0], a[1], optimize)
            assert got[0] == got[2] == (_lib.PP_OK, len(want), want), (optimize, bad)


def test_a_capacity_one_byte_short_reports_the_need_and_writes_nothing(jpeg):
    _lib = jpeg._lib
    sets = RC.hand_made(jpeg)
    names = ("ff ends 4:2:0", "ragged r2", "zeros r1")
    for optimize in (False, True):
        want = [host_scan(jpeg, n, sets[n][0], sets[n][1], optimize) for n in names]
        assert all(RC.split_scan(w)[1] for w in want), "every stream holds markers: the need counts them"
        caps = [len(want[0]), len(want[1]) - 1, len(want[2])]
        got = raw_restart(jpeg, [sets[n][0] for n in names], [sets[n][1] for n in names], optimize, capacities=caps)
        assert got[1] == (_lib.PP_ERR_WORKSPACE, len(want[1]), b"")
        assert got[0] == (_lib.PP_OK, len(want[0]), want[0]) and got[2] == (_lib.PP_OK, len(want[2]), want[2]), "a stream that fits its capacity exactly"


def test_the_calls_without_intervals_keep_their_launches_and_ignore_the_field(jpeg):
    _lib = jpeg._lib
    sets = RC.hand_made(jpeg)
    cs = [sets["ragged r2"][0], sets["phases r1"][0]]
    for optimize, tags, other in ((False, ENT_TAGS, "pp_jpeg_entropy_opt.hip"), (True, OPT_TAGS, "pp_jpeg_entropy.hip")):
        _lib.reset_launch_counts()
        files = jpeg.entropy_encode_device(cs, DEV, optimize=optimize)
        assert [_lib.launch_count(t) for t in tags] == [1] * len(tags) and _lib.launch_count(other) == 0
        assert [_lib.launch_count(t) for t in RST_TAGS + OPT_RST_TAGS[3:]] == [0] * 14 and _lib.launch_count("jpeg_opt_rst_hist") == 0
        assert files == [jpeg.entropy_encode(c, 0, optimize) for c in cs]
        calls, rst = jpeg.entropy_device_calls, jpeg.entropy_restart_device_calls
        assert jpeg.entropy_encode_device(cs, DEV, optimize=optimize, restart_interval=[0, 0]) == files
        assert (jpeg.entropy_device_calls, jpeg.entropy_restart_device_calls) == (calls + 1, rst), "all intervals 0: the call made without the keyword"
        _lib.reset_launch_counts()
        got = jpeg.entropy_encode_device(cs, DEV, optimize=optimize, restart_interval=[2, 0])
        assert (jpeg.entropy_device_calls, jpeg.entropy_restart_device_calls) == (calls + 2, rst + 1)
        assert [_lib.launch_count(t) for t in (OPT_RST_TAGS if optimize else RST_TAGS)] == [1] * len(tags)
        assert got == [jpeg.entropy_encode(cs[0], 2, optimize), files[1]]
    # the old raw call with a non-zero interval in the descriptor: the bytes without intervals
    c = cs[0]
    info = c.info
    share, cap = int(_lib.lib.pp_jpeg_entropy_scratch_bytes(ctypes.byref(info), 1)), int(_lib.lib.pp_jpeg_encoded_bound(ctypes.byref(info)))
    coef_d = torch.from_numpy(np.ascontiguousarray(c.coef, np.int16)).to(DEV)
    scratch, out, res = (torch.zeros(k, dtype=torch.uint8, device=DEV) for k in (share, _align(cap), 256))
    desc = np.zeros(1, jpeg._ENT_RESTART_DESC)
    desc[0] = (coef_d.data_ptr(), scratch.data_ptr(), out.data_ptr(), res.data_ptr(), cap, info.hs, info.vs, info.mcus_x, info.mcus_y, 2, 0)
    desc_d = torch.from_numpy(desc.view(np.uint8)).to(DEV)
    _lib.call("pp_jpeg_entropy_encode_batch", desc_d.data_ptr(), 1, int(info.coef_count) // 64, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    slot = res.cpu().numpy()[:16].view(jpeg._ENT_RESULT)[0]
    want = host_scan(jpeg, "ragged r2", c, 0, False)
    assert (int(slot["status"]), int(slot["bytes"])) == (_lib.PP_OK, len(want)) and out.cpu().numpy()[:len(want)].tobytes() == want


# ---------------------------------------------------------------------------------------------------- end to end
def _mixed_frames():
    return [torch.from_numpy(E.image(content, W, H).copy()).to(DEV)
            for content, W, H in (("noise", 96, 64), ("gradient", 250, 130), ("checker", 17, 33), ("noise", 8, 8), ("gradient", 64, 96))]


def test_encode_batch_with_restart_rows_on_the_device_equals_the_host_path(jpeg):
    from PIL import Image

    frames = _mixed_frames()
    for ss in ("4:2:0", "4:4:4"):
        for optimize in (False, True):
            kw = dict(quality=75, subsampling=ss, channel_order="rgb", optimize=optimize)
            calls, rst = jpeg.entropy_device_calls, jpeg.entropy_restart_device_calls
            host = jpeg.encode_batch(frames, entropy="host", restart_rows=1, **kw)
            assert jpeg.entropy_device_calls == calls
            dev = jpeg.encode_batch(frames, entropy="device", restart_rows=1, **kw)
            assert (jpeg.entropy_device_calls, jpeg.entropy_restart_device_calls) == (calls + 1, rst + 1), "one device call per batch"
            assert dev == host, (ss, optimize, [len(a) == len(b) for a, b in zip(dev, host)])
            plain = jpeg.encode_batch(frames, entropy="device", **kw)
            assert jpeg.entropy_restart_device_calls == rst + 1, "without the keyword: the call without intervals"
            for f, p, im in zip(dev, plain, frames):
                info = jpeg.probe(f)
                assert info.restart_interval == info.mcus_x, "a marker every MCU row of the image's own width"
                assert len(RC.split_scan(RC.plain_scan(f))[0]) == info.mcus_y and jpeg.probe(p).restart_interval == 0
                a, b = np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), np.asarray(Image.open(io.BytesIO(p)).convert("RGB"))
                assert a.shape == tuple(im.shape) and np.array_equal(a, b), "Pillow reads the pixels of the file without markers"
            two = jpeg.encode_batch(frames[:2], entropy="device", restart_rows=2, **kw)
            assert two == jpeg.encode_batch(frames[:2], entropy="host", restart_rows=2, **kw)
            assert [jpeg.probe(f).restart_interval for f in two] == [2 * jpeg.probe(f).mcus_x for f in two]


def test_the_device_decoder_reads_what_the_device_coder_wrote(jpeg):
    files = []
    for optimize in (False, True):
        files += jpeg.encode_batch(_mixed_frames(), quality=90, subsampling="4:2:0", channel_order="rgb", entropy="device", restart_rows=1, optimize=optimize)
    assert all(jpeg.probe(f).restart_interval > 0 for f in files)
    want = [t.cpu().numpy() for t in jpeg.decode_batch(files, DEV, entropy="host")]
    calls, falls, unsync = jpeg.huffman_device_calls, jpeg.fallbacks, jpeg.unsynchronised
    got = jpeg.decode_batch(files, DEV, entropy="device")
    assert jpeg.huffman_device_calls == calls + 1 and jpeg.fallbacks == falls and jpeg.unsynchronised == unsync, "no fallback, no unsynchronised image"
    for g, w in zip(got, want):
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), w)


def test_imwrite_device_and_the_visualizer_pass_restart_rows_through(jpeg, tmp_path):
    img = torch.from_numpy(E.image("gradient", 96, 64).copy()).to(DEV)
    path = str(tmp_path / "a.jpg")
    jpeg.imwrite_device(path, img, quality=75, subsampling="4:2:0", channel_order="rgb", entropy="device", restart_rows=2)
    data = open(path, "rb").read()
    assert data == jpeg.encode_batch([img], quality=75, subsampling="4:2:0", channel_order="rgb", entropy="host", restart_rows=2)[0]
    assert jpeg.probe(data).restart_interval == 2 * jpeg.probe(data).mcus_x


def test_video_demo_writes_the_same_video_with_device_and_host_entropy(jpeg, tmp_path):
    from probpose_code_amd.video import MjpegAviWriter, read_mjpeg_avi

    sys.path.insert(0, os.path.join(ROOT, "demo"))
    import video_demo

    frames = jpeg.encode_batch([torch.from_numpy(E.image(content, 96, 64).copy()).to(DEV) for content in ("gradient", "noise", "checker")],
                               quality=90, channel_order="rgb")
    src = str(tmp_path / "in.avi")
    with MjpegAviWriter(src, 12.5) as w:
        for f in frames:
            w.write(f)
    outs = []
    for entropy in ("device", "host"):
        dst = str(tmp_path / f"{entropy}.avi")
        rst = jpeg.entropy_restart_device_calls
        done = video_demo.main([src, CFG, "synthetic", "--out-video", dst, "--decode", "device", "--entropy", entropy, "--restart-rows", "1",
                                "--bboxes", "10,4,80,60", "--quality", "80", "--encode-batch", "2", "--device", DEV])
        assert done["frames"] == 3 and jpeg.entropy_restart_device_calls == rst + (2 if entropy == "device" else 0)
        outs.append(open(dst, "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) > 1000
    written = list(read_mjpeg_avi(str(tmp_path / "device.avi")))
    assert len(written) == 3 and all(jpeg.probe(f).restart_interval == jpeg.probe(f).mcus_x == 6 for f in written)
