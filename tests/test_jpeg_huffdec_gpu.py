"""GPU: the device Huffman decoder (csrc/pp_jpeg_huffdec.hip behind pp_jpeg_huffman_decode_batch) byte for byte against
jpeg.entropy_decode of the same file: the smallest streams, streams whose length, byte stuffing, codes and extra bits meet
the subsequence boundaries (each situation asserted through tests/jpeg_huffdec_ref.py), files with their own Huffman tables,
a stream over several workgroups, mixed batches, refusal - not wrong data - of a stream the passes do not synchronise, damaged
streams, and the callers (decode_batch, imread_device, LoadImage, the video demo) end to end. Every raw call runs twice on buffers inside canary bytes."""
import io
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import jpeg_huffdec_cases as C  # noqa: E402
import jpeg_huffdec_ref as R  # noqa: E402
import jpeg_ref as J  # noqa: E402
import jpeg_sources as S  # noqa: E402
from make_golden_jpeg import content, encode  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5
GUARD = 256
CFG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")
TAGS = ("jpeg_hd_sync", "jpeg_hd_scan", "jpeg_hd_zero", "jpeg_hd_write", "jpeg_hd_dc")


@pytest.fixture(scope="module")
def jpeg(lib_built):
    from probpose_code_amd import jpeg

    return jpeg


def _align(v, a=256):
    return (v + a - 1) // a * a


def raw_decode(jpeg, scans, sync_passes=None, check_launches=True):
    """pp_jpeg_huffman_decode_batch on buffers of this test's own: every coefficient buffer, scratch share and result slot
    between GUARD canary bytes, the input block compared afterwards. Runs the call twice with identical results. Returns
    [(coefficients int16, result record)]."""
    import ctypes

    _lib = jpeg._lib
    n = len(scans)
    passes = jpeg.DEFAULT_SYNC_PASSES if sync_passes is None else sync_passes
    lens = [int(s.stream.size) for s in scans]
    shares = []
    for s, ln in zip(scans, lens):
        one = int(_lib.lib.pp_jpeg_huffman_scratch_bytes(ctypes.byref(s.info), (ctypes.c_longlong * 1)(ln), 1))
        assert one > 0 and one % 256 == 0
        shares.append(one)
    infos = (jpeg.JpegInfo * n)(*[s.info for s in scans])
    assert int(_lib.lib.pp_jpeg_huffman_scratch_bytes(infos, (ctypes.c_longlong * n)(*lens), n)) == sum(shares)
    off, o_tab, o_str = _align(72 * n), [], []
    for s in scans:
        o_tab.append(off)
        off = _align(off + s.tables.size)
        o_str.append(off)
        off = _align(off + max(1, s.stream.size))
    host = np.zeros(off, np.uint8)
    counts = [int(s.info.coef_count) for s in scans]

    def guarded(sizes):
        offs, at = [], GUARD
        for z in sizes:
            offs.append(at)
            at += _align(z) + GUARD
        return offs, torch.full((at,), CANARY, dtype=torch.uint8, device=DEV)

    o_coef, coef = guarded([2 * c for c in counts])
    o_scr, scratch = guarded(shares)
    o_res, results = guarded([16] * n)
    block = torch.empty(off, dtype=torch.uint8, device=DEV)
    desc = host[:72 * n].view(jpeg._HD_DESC)
    for i, s in enumerate(scans):
        host[o_tab[i]:o_tab[i] + s.tables.size] = s.tables
        host[o_str[i]:o_str[i] + s.stream.size] = s.stream
        desc[i] = (block.data_ptr() + o_str[i], block.data_ptr() + o_tab[i], coef.data_ptr() + o_coef[i], scratch.data_ptr() + o_scr[i],
                   results.data_ptr() + o_res[i], lens[i], s.info.hs, s.info.vs, s.info.mcus_x, s.info.mcus_y, s.info.ncomp, 0)
    block.copy_(torch.from_numpy(host))
    args = (block.data_ptr(), n, max(lens), max(c // 64 for c in counts), passes, torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        coef.fill_(CANARY)
        results.fill_(CANARY)
        _lib.reset_launch_counts()
        _lib.call("pp_jpeg_huffman_decode_batch", *args)
        torch.cuda.synchronize()
        if check_launches:
            got = tuple(_lib.launch_count(t) for t in TAGS) + (_lib.launch_count("pp_jpeg_huffdec.hip"),)
            assert got == (passes, 1, 1, 1, 1, passes + 4), f"launches per call {got}"
        runs.append((coef.cpu().numpy(), results.cpu().numpy(), scratch.cpu().numpy()))
    assert np.array_equal(block.cpu().numpy(), host), "the kernels changed their input"
    (c1, r1, s1), (c2, r2, _) = runs
    out = []
    for name, buf, offs, sizes in (("coefficients", c1, o_coef, [2 * c for c in counts]), ("scratch", s1, o_scr, shares), ("results", r1, o_res, [16] * n)):
        mask = np.ones(len(buf), bool)
        for o, z in zip(offs, sizes):
            mask[o:o + z] = False
        assert (buf[mask] == CANARY).all(), f"bytes outside the {name} written"
    assert np.array_equal(r1, r2), "a second launch gives other result slots"
    for i in range(n):
        res = r1[o_res[i]:o_res[i] + 16].view(jpeg._HD_RESULT)[0]
        a, b = c1[o_coef[i]:o_coef[i] + 2 * counts[i]], c2[o_coef[i]:o_coef[i] + 2 * counts[i]]
        if int(res["status"]) == jpeg._lib.PP_OK:
            assert np.array_equal(a, b), "a second launch gives other coefficients"
        out.append((a.view(np.int16).copy(), res))
    return out


def _check_exact(jpeg, files, sync_passes=None):
    """Every file of the batch decodes with PP_OK to entropy_decode's coefficients."""
    scans = [jpeg.scan_prepare(f) for f in files]
    got = raw_decode(jpeg, scans, sync_passes)
    for f, s, (coef, res) in zip(files, scans, got):
        want = jpeg.entropy_decode(f)
        assert int(res["status"]) == jpeg._lib.PP_OK and int(res["reason"]) == 0, (bytes(s.info.reason), res)
        assert coef.size == want.coef.size and coef.tobytes() == want.coef.tobytes()
        assert np.array_equal(s.qtables, want.qtables)
        assert int(res["blocks"]) >= want.coef.size // 64 and 1 <= int(res["passes"]) <= (sync_passes or jpeg.DEFAULT_SYNC_PASSES)
    return got


def _corpus_file(prefix):
    names = [n for n in C.corpus() if n.startswith(prefix)]
    assert names, prefix
    return C.corpus()[names[0]]


SMALL = ["33x17_420", "37x29_444", "31x50_422", "48x64_grey"]


def test_smallest_streams(jpeg):
    grey8 = _corpus_file("8x8_grey_q75")
    assert len(C.prepared(grey8)["stream"]) < R.S and jpeg.probe(grey8).coef_count == 64
    one_mcu = _corpus_file("16x16_420_q")
    assert jpeg.probe(one_mcu).coef_count == 6 * 64
    _check_exact(jpeg, [grey8])
    _check_exact(jpeg, [one_mcu])
    files = [S.transcoded(name, "plain") for name in SMALL]
    for f in files:
        _check_exact(jpeg, [f])
    _check_exact(jpeg, files)


def test_lengths_at_the_subsequence_size(jpeg):
    files = []
    for length, name in ((R.S, "len_S"), (R.S - 1, "len_S-1"), (R.S + 1, "len_S+1"), (2 * R.S, "len_2S")):
        f = C.find_length(length)
        assert name in R.situations(C.prepared(f)) and jpeg.scan_prepare(f).stream.size == length
        _check_exact(jpeg, [f])
        files.append(f)
    _check_exact(jpeg, files)


@pytest.mark.parametrize("situation", ["ff00_split", "code_straddles", "extra_bits_straddle", "ends_at_63", "zrl", "longest_codes"])
def test_boundary_situations(jpeg, situation):
    files = [C.find(situation, sampling) for sampling in ("420", "444", "grey")]
    for f in files:
        assert situation in R.situations(C.prepared(f))
        assert C.reference(f)["status"] == R.OK
        _check_exact(jpeg, [f])
    _check_exact(jpeg, files)


def test_hand_built_streams_with_other_tables(jpeg):
    """What Pillow does not write: Fibonacci-shaped tables (codes of every length up to 16), shared and moved table slots."""
    files = [S.transcoded(name, layout) for name in ("33x17_420", "37x29_444", "48x64_grey")
             for layout in ("fibonacci", "shared_pair_slots_2_3", "slots_3_2_split", "pq1_sof1", "ids_rgb_with_jfif")]
    assert any(max(len(c) for c in t) == 16 for f in files for t in C.prepared(f)["tables"])
    assert any("longest_codes" in R.situations(C.prepared(f)) for f in files)
    _check_exact(jpeg, files)


def test_files_with_their_own_tables(jpeg):
    files = []
    for i, sampling in enumerate(("444", "422", "420")):
        px = C.photo(72, 104, i)
        plain, own = encode(px, sampling, 85, 0), encode(px, sampling, 85, 0, optimize=True)
        assert C.prepared(plain)["tables"] != C.prepared(own)["tables"], "optimize=True writes the file's own DHT"
        files.append(own)
    _check_exact(jpeg, files)
    for f in files:
        _check_exact(jpeg, [f])


def test_a_stream_across_three_workgroups(jpeg):
    f = encode(C.photo(480, 640, 3), "420", 90, 0)
    scan = jpeg.scan_prepare(f)
    nsub = -(-scan.stream.size // R.S)
    assert -(-nsub // R.WG) >= 3, f"{scan.stream.size} bytes span {-(-nsub // R.WG)} workgroups"
    ((coef, res),) = _check_exact(jpeg, [f])
    want = jpeg.entropy_decode(f).coef
    assert coef[-64] == want[-64] and coef[64 * (scan.info.comp_bw[0] * scan.info.comp_bh[0] - 1)] == want[64 * (scan.info.comp_bw[0] * scan.info.comp_bh[0] - 1)]
    assert int(res["blocks"]) >= 80 * 60 * 6 // 4


@pytest.mark.parametrize("size", [(9, 1037), (1037, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_long_and_tall_images(jpeg, size):
    H, W = size
    files = [S.encoded(H, W, sampling, 75, "noise", 0) for sampling in ("420", "422", "444", "grey")]
    _check_exact(jpeg, files)


def test_mixed_batch_of_sixteen_and_the_empty_batch(jpeg):
    files = [S.transcoded(name, "plain") for name in SMALL]
    files += [C.find_length(R.S), C.find("ff00_split"), _corpus_file("8x8_grey_q75"), _corpus_file("1x1_444_q"), _corpus_file("17x33_444_q")]
    flat = encode(np.full((200, 264, 3), 128, np.uint8), "444", 75, 0)  # the most blocks, a short stream
    noisy = encode(content("noise", 64, 80, 3, np.random.default_rng(4)), "420", 100, 0)  # the longest stream, few blocks
    files += [flat, noisy, encode(C.photo(120, 88, 1), "422", 60, 0), encode(C.photo(40, 200, 2), "420", 92, 0, optimize=True),
              encode(content("bilevel", 56, 56, 1, np.random.default_rng(6)), "grey", 50, 0), _corpus_file("48x64_420_q95"),
              _corpus_file("31x50_422_q")]
    assert len(files) == 16
    scans = [jpeg.scan_prepare(f) for f in files]
    by_stream = max(range(16), key=lambda i: scans[i].stream.size)
    by_blocks = max(range(16), key=lambda i: scans[i].info.coef_count)
    assert by_stream != by_blocks and files[by_blocks] is flat and files[by_stream] is noisy
    assert len({(s.info.ncomp, s.info.hs, s.info.vs) for s in scans}) == 4
    _check_exact(jpeg, files)
    # n = 0: PP_OK without a launch
    jpeg._lib.reset_launch_counts()
    jpeg._lib.call("pp_jpeg_huffman_decode_batch", None, 0, 0, 0, 3, None)
    assert jpeg._lib.launch_count("pp_jpeg_huffdec.hip") == 0
    assert jpeg.huffman_decode_device([], DEV)[0] == [] and jpeg.decode_batch([], DEV, entropy="device") == []
    for bad in ((None, 1, 10, 1, 3), (1, -1, 10, 1, 3), (1, 1, 10, 1, 0), (1, 1, 10, 1, jpeg.MAX_SYNC_PASSES + 1), (1, 1, 1 << 28, 1, 3), (1, 1, 10, 0, 3)):
        assert jpeg._lib.lib.pp_jpeg_huffman_decode_batch(*bad, None) == jpeg._lib.PP_ERR_INVALID_ARG
    assert jpeg._lib.launch_count("pp_jpeg_huffdec.hip") == 0


def test_an_unsynchronised_stream_is_refused_and_its_neighbours_stay_exact(jpeg):
    slow = C.slow_stream()
    needed = R.passes_needed(C.prepared(slow))
    assert 1 < needed <= jpeg.DEFAULT_SYNC_PASSES
    left, right = S.transcoded("33x17_420", "plain"), C.find("ff00_split")
    files = [left, slow, right]
    scans = [jpeg.scan_prepare(f) for f in files]
    got = raw_decode(jpeg, scans, sync_passes=needed - 1)
    assert int(got[1][1]["status"]) == jpeg._lib.PP_ERR_UNSUPPORTED and int(got[1][1]["reason"]) == R.NOT_SYNCHRONISED
    assert jpeg.HD_REASONS[int(got[1][1]["reason"])] == "not synchronised"
    for i in (0, 2):
        assert int(got[i][1]["status"]) == jpeg._lib.PP_OK and got[i][0].tobytes() == jpeg.entropy_decode(files[i]).coef.tobytes()
    # at the default setting the reference says it fits, and it is exact; the passes used are the reference's
    assert C.reference(slow)["status"] == R.OK
    got = _check_exact(jpeg, files)
    assert int(got[1][1]["passes"]) == C.reference(slow)["passes"] == needed
    # through the public call: the result slots and tensors of huffman_decode_device
    coefs, res = jpeg.huffman_decode_device(scans, DEV, sync_passes=needed - 1)
    assert [int(r["status"]) for r in res] == [0, jpeg._lib.PP_ERR_UNSUPPORTED, 0]
    assert coefs[0].dtype == torch.int16 and coefs[0].cpu().numpy().tobytes() == jpeg.entropy_decode(left).coef.tobytes()
    # decode_batch: the refused image comes back with the host path's pixels
    want = [t.cpu().numpy() for t in jpeg.decode_batch(files, DEV, entropy="host")]
    falls, unsync = jpeg.fallbacks, jpeg.unsynchronised
    got = jpeg.decode_batch(files, DEV, entropy="device", sync_passes=needed - 1)
    assert jpeg.unsynchronised == unsync + 1 and jpeg.fallbacks == falls + 1
    for g, w in zip(got, want):
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), w)
    got = jpeg.decode_batch(files, DEV, entropy="device")
    assert jpeg.unsynchronised == unsync + 1
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)


def damaged(data: bytes):
    """The damaged copies scripts/jpeg_huffdec_host_check.cpp runs under the sanitisers: the segment without its last 1, 6, 17
    and 39 bytes (EOI put back) and 32 single bit flips at fixed places of the segment."""
    p = C.prepared(data)
    off, n = p["offset"], len(p["stream"])
    out = [data[:off + n - cut] + b"\xff\xd9" for cut in (1, 6, 17, 39) if cut < n]
    for k in range(32):
        at = off + n * k // 32
        out.append(data[:at] + bytes([data[at] ^ (1 << (k % 8))]) + data[at + 1:])
    return out


def test_damaged_streams_end_in_a_status(jpeg):
    sources = [S.transcoded("33x17_420", "plain"), S.transcoded("48x64_grey", "plain"), C.find("ff00_split", "444")]
    cases = [d for f in sources for d in damaged(f)]
    scans, kept = [], []
    for d in cases:
        try:
            scans.append(jpeg.scan_prepare(d))
            kept.append(d)
        except jpeg.JpegUnsupported:
            with pytest.raises(jpeg.JpegUnsupported):  # what the preparation refuses, the host decoder refuses
                jpeg.entropy_decode(d)
    assert len(kept) >= 90
    refused = exact = 0
    for lo in range(0, len(kept), 16):
        got = raw_decode(jpeg, scans[lo:lo + 16], sync_passes=jpeg.MAX_SYNC_PASSES, check_launches=False)
        for d, (coef, res) in zip(kept[lo:lo + 16], got):
            try:
                want = jpeg.entropy_decode(d)
            except jpeg.JpegUnsupported:
                assert int(res["status"]) == jpeg._lib.PP_ERR_UNSUPPORTED and int(res["reason"]) in jpeg.HD_REASONS
                refused += 1
                continue
            if int(res["status"]) == jpeg._lib.PP_OK:
                assert coef.tobytes() == want.coef.tobytes()
                exact += 1
            else:  # the host accepts it: only a stream that did not synchronise may be refused here
                assert int(res["reason"]) == R.NOT_SYNCHRONISED
    assert refused >= 20 and exact >= 20, (refused, exact)


def test_decode_batch_with_device_entropy_equals_host_entropy(jpeg, tmp_path):
    files = [S.transcoded(s, l) for s, l in S.layout_cases() if s in ("33x17_420", "37x29_444", "31x50_422", "48x64_grey")]
    assert len(files) == 48
    refused = J.golden()["refused"]["progressive"]
    path = str(tmp_path / "one.jpg")
    with open(path, "wb") as f:
        f.write(files[0])
    files = files + [refused, path]
    calls, falls, unsync = jpeg.huffman_device_calls, jpeg.fallbacks, jpeg.unsynchronised
    got = jpeg.decode_batch(files, DEV, entropy="device")
    assert jpeg.huffman_device_calls == calls + 1 and jpeg.unsynchronised == unsync and jpeg.fallbacks == falls + 1
    want = jpeg.decode_batch(files, DEV, entropy="host")
    assert jpeg.huffman_device_calls == calls + 1
    prepared = 0
    for f, g, w in zip(files, got, want):
        assert g.is_cuda and g.dtype == torch.uint8 and np.array_equal(g.cpu().numpy(), w.cpu().numpy())
        assert np.array_equal(g.cpu().numpy(), jpeg.imread_device(f, DEV).cpu().numpy())
        try:
            jpeg.scan_prepare(f)
            prepared += 1
        except jpeg.JpegUnsupported:
            pass
    assert 20 <= prepared < len(files), "files with a restart interval go the host way, the others the device way"
    assert np.array_equal(jpeg.imread_device(path, DEV, entropy="device").cpu().numpy(), want[-1].cpu().numpy())
    with pytest.raises(ValueError, match="entropy"):
        jpeg.decode_batch(files, DEV, entropy="gpu")
    with pytest.raises(ValueError, match="entropy"):
        jpeg.imread_device(path, DEV, entropy="gpu")
    with pytest.raises(OSError):
        jpeg.decode_batch([str(tmp_path / "missing.jpg")], DEV, entropy="device")
    # the transform: a device tensor with the host decoder's bytes
    from probpose_code_amd import transforms as T

    one = T.Compose([dict(type="MI355XLoadImage", imdecode_backend="mi355x-huffman")])(dict(img_path=path))
    ref = T.Compose([dict(type="MI355XLoadImage")])(dict(img_path=path))
    assert one["img"].is_cuda and np.array_equal(one["img"].cpu().numpy(), ref["img"]) and tuple(one["img_shape"]) == tuple(ref["img_shape"])


def test_video_demo_with_device_entropy_decode_writes_the_same_file(jpeg, tmp_path):
    from PIL import Image

    from probpose_code_amd.video import MjpegAviWriter

    sys.path.insert(0, os.path.join(ROOT, "demo"))
    import video_demo

    src = str(tmp_path / "in.avi")
    with MjpegAviWriter(src, 12.5) as w:
        for i in range(3):
            b = io.BytesIO()
            Image.fromarray(C.photo(64, 96, i)).save(b, "JPEG", quality=90)
            w.write(b.getvalue())
    outs = []
    for extra in ([], ["--decode-entropy", "device"]):
        dst = str(tmp_path / f"out{len(outs)}.avi")
        calls = jpeg.huffman_device_calls
        done = video_demo.main([src, CFG, "synthetic", "--out-video", dst, "--decode", "device", "--bboxes", "10,4,80,60", "--quality", "80",
                                "--device", DEV] + extra)
        assert done["frames"] == 3 and jpeg.huffman_device_calls == calls + (3 if extra else 0)
        outs.append(open(dst, "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) > 1000
    with pytest.raises(SystemExit):
        video_demo.main([src, CFG, "synthetic", "--out-video", str(tmp_path / "x.avi"), "--decode-entropy", "device"])
