"""GPU: the device Huffman decoder on files with a restart interval (pp_jpeg_hd_desc.restart_interval > 0) byte for byte
against jpeg.entropy_decode of the same file: the committed grid's restart files and the hand-built layouts in one mixed
batch, every interval geometry, markers at the subsequence and workgroup borders (each situation found and asserted on the
CPU by tests/jpeg_huffdec_restart_cases.py), the bounded synchronisation distance, damaged markers and bits (the streams
scripts/jpeg_huffdec_host_check.cpp has run under the sanitisers), and the callers end to end. Every raw call runs twice on
buffers inside canary bytes."""
import ctypes
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
import jpeg_huffdec_restart_cases as RC  # noqa: E402
import jpeg_sources as S  # noqa: E402
from make_golden_jpeg import content, encode  # noqa: E402
from test_jpeg_gpu import _same_samples, small_model  # noqa: E402,F401  (the dataset and model of the decoder's own loop test)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5
GUARD = 256
CFG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")
TAGS = ("jpeg_hd_sync", "jpeg_hd_scan", "jpeg_hd_zero", "jpeg_hd_write", "jpeg_hd_dc")
NOT_SYNCHRONISED = 1


@pytest.fixture(scope="module")
def jpeg(lib_built):
    from probpose_code_amd import jpeg

    return jpeg


def _align(v, a=256):
    return (v + a - 1) // a * a


def restart_decode(jpeg, scans, sync_passes=None, check_launches=True):
    """pp_jpeg_huffman_decode_batch on buffers of this test's own, each image's restart interval in its descriptor: every
    coefficient buffer, scratch share and result slot between GUARD canary bytes, the input block compared afterwards. Runs
    the call twice with identical bytes. Returns [(coefficients int16, result record)]."""
    _lib = jpeg._lib
    n = len(scans)
    passes = jpeg.DEFAULT_SYNC_PASSES if sync_passes is None else sync_passes
    lens = [int(s.stream.size) for s in scans]
    shares = [int(_lib.lib.pp_jpeg_huffman_scratch_bytes(ctypes.byref(s.info), (ctypes.c_longlong * 1)(ln), 1)) for s, ln in zip(scans, lens)]
    assert all(z > 0 and z % 256 == 0 for z in shares)
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
                   results.data_ptr() + o_res[i], lens[i], s.info.hs, s.info.vs, s.info.mcus_x, s.info.mcus_y, s.info.ncomp, s.info.restart_interval)
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
    for name, buf, offs, sizes in (("coefficients", c1, o_coef, [2 * c for c in counts]), ("scratch", s1, o_scr, shares), ("results", r1, o_res, [16] * n)):
        mask = np.ones(len(buf), bool)
        for o, z in zip(offs, sizes):
            mask[o:o + z] = False
        assert (buf[mask] == CANARY).all(), f"bytes outside the {name} written"
    assert np.array_equal(r1, r2), "a second launch gives other result slots"
    out = []
    for i in range(n):
        res = r1[o_res[i]:o_res[i] + 16].view(jpeg._HD_RESULT)[0]
        a, b = c1[o_coef[i]:o_coef[i] + 2 * counts[i]], c2[o_coef[i]:o_coef[i] + 2 * counts[i]]
        if int(res["status"]) == jpeg._lib.PP_OK:
            assert np.array_equal(a, b), "a second launch gives other coefficients"
        out.append((a.view(np.int16).copy(), res))
    return out


def _check_exact(jpeg, files, sync_passes=None):
    """Every file of the batch is prepared and decodes with PP_OK to entropy_decode's coefficients."""
    scans = [jpeg.scan_prepare(f, restart=True) for f in files]
    got = restart_decode(jpeg, scans, sync_passes)
    for k, (f, s, (coef, res)) in enumerate(zip(files, scans, got)):
        want = jpeg.entropy_decode(f)
        assert int(res["status"]) == jpeg._lib.PP_OK and int(res["reason"]) == 0, (k, int(s.info.restart_interval), res)
        assert coef.size == want.coef.size and coef.tobytes() == want.coef.tobytes(), k
        assert np.array_equal(s.qtables, want.qtables)
        assert int(res["blocks"]) >= want.coef.size // 64 and 1 <= int(res["passes"]) <= (sync_passes or jpeg.DEFAULT_SYNC_PASSES)
    return got


def test_one_mixed_batch_of_every_restart_file(jpeg):
    restart = list(RC.golden_restart().values())
    layouts = [S.transcoded(s, l) for s, l in RC.restart_layouts()]
    plain = RC.golden_plain(12)
    assert len(restart) > 100 and len(layouts) >= 25 and len(plain) == 12
    assert {jpeg.probe(f).restart_interval for f in restart} == {1, 3}
    files = restart + layouts
    step = len(files) // 12
    for k, f in enumerate(plain):  # a dozen files without a restart interval among them
        files.insert(k * (step + 1), f)
    ris = [jpeg.probe(f).restart_interval for f in files]
    assert ris.count(0) == 12 and 65535 in ris and 7 in ris and 5 in ris
    fills = sum(any(m > f0 + 1 for f0, m in RC.segment(f)[2]) for f in layouts)
    assert fills >= 8, "layouts with fill bytes in front of RSTn: decoded on the device, none turned away"
    _check_exact(jpeg, files)


def _geometry_files():
    files, notes = [], []
    for sampling, (H, W) in (("grey", (40, 48)), ("444", (40, 48)), ("422", (40, 72)), ("420", (64, 80))):
        hs, vs = {"grey": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}[sampling]
        mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
        px = content("noise" if sampling in ("grey", "420") else "smooth", H, W, 1 if sampling == "grey" else 3, np.random.default_rng([H, W, hs]))
        for ri in (1, mx, 7, mx * my - 1, mx * my, 65535):
            assert mx % 7 != 0 and 1 < mx < mx * my - 1
            files.append(encode(px, sampling, 85, ri))
            notes.append((sampling, ri, mx * my))
    for sampling in ("grey", "420"):  # one MCU
        px = content("noise", 8 if sampling == "grey" else 16, 8 if sampling == "grey" else 16, 1 if sampling == "grey" else 3, np.random.default_rng(5))
        files.append(encode(px, sampling, 90, 1))
        notes.append((sampling, 1, 1))
    return files, notes


def test_interval_geometry(jpeg):
    files, notes = _geometry_files()
    wraps = 0
    for f, (sampling, ri, mcus) in zip(files, notes):
        info = jpeg.probe(f)
        assert info.restart_interval == ri and info.mcus_x * info.mcus_y == mcus, (sampling, ri)
        marks = RC.segment(f)[2]
        assert len(marks) == -(-mcus // ri) - 1, (sampling, ri)
        wraps += len(marks) + 1 >= 17  # the marker numbers wrap twice
    assert wraps >= 4 and any(m == 1 for _, _, m in notes) and any(ri == m for _, ri, m in notes if m > 1)
    _check_exact(jpeg, files)
    for f in files[::5]:
        _check_exact(jpeg, [f])


def test_markers_at_the_borders(jpeg):
    files = []
    for situation in RC.SITUATIONS:
        f = RC.find(situation)
        assert situation in RC.situations(f), situation  # found on the CPU
        files.append(f)
    long = RC.long_noise()
    _, n, marks = RC.segment(long)
    at = {m // RC.SUB % RC.WG for m, _ in marks}
    assert n > 65536 and 0 in {m // RC.SUB % RC.WG for m, _ in marks if m // RC.SUB >= RC.WG} and RC.WG - 1 in at
    _check_exact(jpeg, files + [long])
    for f in files:
        _check_exact(jpeg, [f])


def test_synchronisation_is_bounded_by_the_interval(jpeg):
    """Pass 0 leaves every subsequence behind its workgroup's first marker true; pass 1 carries the border state at most one
    interval - fewer than 32 subsequences - into each workgroup: two launches, whatever the stream's own synchronisation
    distance."""
    f = RC.long_noise()
    info = jpeg.probe(f)
    assert (info.hs, info.vs, info.restart_interval) == (2, 2, 1)
    _, n, marks = RC.segment(f)
    assert n > 65536 and -(-(-(-n // RC.SUB)) // RC.WG) >= 3
    bounds = [0] + [m + 1 for _, m in marks] + [n]
    assert max(b - a for a, b in zip(bounds, bounds[1:])) < 31 * RC.SUB
    ((coef, res),) = _check_exact(jpeg, [f], sync_passes=2)
    assert int(res["passes"]) <= 2
    scan = jpeg.scan_prepare(f, restart=True)
    ((coef, res),) = restart_decode(jpeg, [scan], sync_passes=1)  # the first launch passes no state across a workgroup border
    assert int(res["status"]) == jpeg._lib.PP_OK or int(res["reason"]) == NOT_SYNCHRONISED
    if int(res["status"]) == jpeg._lib.PP_OK:
        assert coef.tobytes() == jpeg.entropy_decode(f).coef.tobytes()


def _damage_sources():
    out = []
    for sampling, (H, W) in (("grey", (24, 40)), ("444", (24, 32)), ("422", (16, 64)), ("420", (48, 64))):
        px = content("noise", H, W, 1 if sampling == "grey" else 3, np.random.default_rng([H, W, 11]))
        out.append(encode(px, sampling, 80, 1 if sampling in ("grey", "422") else 2))
    return out


def test_damaged_markers_and_bits_end_in_the_host_decoders_verdict(jpeg):
    cases = []
    for f in _damage_sources():
        assert len(RC.segment(f)[2]) >= 5
        cases += [d for _, d in RC.marker_damage(f)] + RC.bit_flips(f)
    kinds = {k for f in _damage_sources() for k, _ in RC.marker_damage(f)}
    assert kinds == {"deleted", "doubled", "swapped", "d7_to_d0"}
    scans, kept = [], []
    for d in cases:
        try:
            scans.append(jpeg.scan_prepare(d, restart=True))
            kept.append(d)
        except jpeg.JpegUnsupported:
            with pytest.raises(jpeg.JpegUnsupported):  # what the preparation refuses, the host decoder refuses
                jpeg.entropy_decode(d)
    assert len(kept) >= 100
    refused = exact = 0
    reasons = set()
    for lo in range(0, len(kept), 64):
        got = restart_decode(jpeg, scans[lo:lo + 64], sync_passes=jpeg.MAX_SYNC_PASSES, check_launches=False)
        for d, (coef, res) in zip(kept[lo:lo + 64], got):
            try:
                want = jpeg.entropy_decode(d)
            except jpeg.JpegUnsupported:
                assert int(res["status"]) == jpeg._lib.PP_ERR_UNSUPPORTED and int(res["reason"]) in jpeg.HD_REASONS
                reasons.add(int(res["reason"]))
                refused += 1
                continue
            if int(res["status"]) == jpeg._lib.PP_OK:
                assert coef.tobytes() == want.coef.tobytes()
                exact += 1
            else:  # the host accepts it: only a stream that did not synchronise may be refused here
                assert int(res["reason"]) == NOT_SYNCHRONISED
    assert refused >= 20 and exact >= 20, (refused, exact)
    assert 7 in reasons and "restart" in jpeg.HD_REASONS[7]


def test_decode_batch_of_restart_files_on_the_device_equals_the_host_path(jpeg):
    files = list(RC.golden_restart().values())[::6] + [S.transcoded(s, l) for s, l in RC.restart_layouts()[::3]] + _geometry_files()[0][::4]
    assert len(files) >= 30 and all(jpeg.probe(f).restart_interval > 0 for f in files)
    want = [t.cpu().numpy() for t in jpeg.decode_batch(files, DEV, entropy="host")]
    calls, falls, unsync = jpeg.huffman_device_calls, jpeg.fallbacks, jpeg.unsynchronised
    got = jpeg.decode_batch(files, DEV, entropy="device")
    assert jpeg.huffman_device_calls == calls + 1 and jpeg.fallbacks == falls and jpeg.unsynchronised == unsync
    for g, w in zip(got, want):
        assert g.is_cuda and g.dtype == torch.uint8 and np.array_equal(g.cpu().numpy(), w)
    assert np.array_equal(jpeg.imread_device(files[0], DEV, entropy="device").cpu().numpy(), want[0])
    assert jpeg.huffman_device_calls == calls + 2 and jpeg.fallbacks == falls


def test_video_demo_reads_a_restart_interval_video_on_the_device(jpeg, tmp_path):
    from probpose_code_amd.video import MjpegAviWriter

    sys.path.insert(0, os.path.join(ROOT, "demo"))
    import video_demo

    frames = jpeg.encode_batch([torch.from_numpy(C.photo(64, 96, i)).to(DEV) for i in range(3)], quality=90, restart_interval=4)
    assert all(jpeg.probe(f).restart_interval == 4 and len(RC.segment(f)[2]) >= 3 for f in frames)
    src = str(tmp_path / "in.avi")
    with MjpegAviWriter(src, 12.5) as w:
        for f in frames:
            w.write(f)
    outs = []
    for extra in ([], ["--decode-entropy", "device"]):
        dst = str(tmp_path / f"out{len(outs)}.avi")
        calls, falls = jpeg.huffman_device_calls, jpeg.fallbacks
        done = video_demo.main([src, CFG, "synthetic", "--out-video", dst, "--decode", "device", "--bboxes", "10,4,80,60", "--quality", "80",
                                "--device", DEV] + extra)
        assert done["frames"] == 3 and jpeg.huffman_device_calls == calls + (3 if extra else 0) and jpeg.fallbacks == falls
        outs.append(open(dst, "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) > 1000


def test_test_dataset_decodes_the_huffman_codes_on_the_device(jpeg, small_model):  # noqa: F811
    from probpose_code_amd import runner

    model, dataset, _, n = small_model
    assert len(dataset) == n > 8
    runs = {}
    for mode, entropy in (("host", "host"), ("device", "device")):
        got = []
        calls, falls, unsync = jpeg.huffman_device_calls, jpeg.fallbacks, jpeg.unsynchronised
        runner.test_dataset(model, dataset, None, batch_size=8, workers=4, sink=got.extend, decode=mode, decode_entropy=entropy)
        torch.cuda.synchronize()
        runs[mode] = got
        if entropy == "device":
            assert jpeg.huffman_device_calls > calls and jpeg.fallbacks == falls and jpeg.unsynchronised == unsync
        else:
            assert jpeg.huffman_device_calls == calls
    _same_samples(runs["host"], runs["device"])
