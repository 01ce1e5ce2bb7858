"""GPU: the device Huffman coder (csrc/pp_jpeg_entropy.hip) against the host coder ``jpeg.entropy_encode`` on the same
coefficients - every comparison is byte for byte, no tolerance anywhere. Coefficients of real pictures (``forward_batch``) at
every size x sampling x quality x content as ONE mixed batch, hand-made coefficient arrays at the edges of the code (DC
differences of +-2047, AC values of +-1023, zero runs of 15 and 16, one to three ZRLs, no EOB, a padded last byte that is FF),
random blocks at three densities; every stream and every scratch share inside canary bytes, coded twice into fresh buffers;
one invalid image in a batch of three; a capacity too small; ``encode_batch(entropy="device")`` against ``entropy="host"``.

The coder's work is divided in chunks: ENT_CHUNK = 256 blocks per workgroup for the bit offsets, STUFF_CHUNK = 2048 bytes per
workgroup pass for the byte stuffing. 250 x 130 has 864 (4:2:0), 1088 (4:2:2) and 1632 (4:4:4) blocks - none a multiple of
256, each several chunks - and its noise streams are many times 2048 bytes long, so both scans cross chunk edges."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_enc_ref as E  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5
GUARD = 4096
ENT_CHUNK = 256     # blocks per workgroup of jpeg_ent_bits / jpeg_ent_pack
STUFF_CHUNK = 2048  # unstuffed bytes per workgroup pass of jpeg_ent_ffcount / jpeg_ent_stuff
SIZES = ((1, 1), (8, 8), (9, 17), (16, 16), (17, 33), (250, 130))  # width x height
SAMPLINGS = ("4:4:4", "4:2:2", "4:2:0")
QUALITIES = (1, 50, 75, 100)
CONTENTS = ("noise", "gradient", "checker")  # noise, smooth, bilevel
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def _align(v, a=256):
    return (v + a - 1) // a * a


@pytest.fixture(scope="module")
def jpeg():
    from probpose_code_amd import jpeg

    return jpeg


# ------------------------------------------------------------------------------------------- hand-made coefficients
def _blank(jpeg, W, H, ss, quality=75):
    info = jpeg.encode_plan(W, H, ss)
    return info, np.zeros(int(info.coef_count), np.int16), jpeg.quality_tables(quality)


def _blocks(coef):
    return coef.reshape(-1, 64)


def hand_made(jpeg):
    """name -> JpegCoefficients. In a 4:4:4 file of one MCU row every component's blocks lie in scan order."""
    cases = {}
    for ss in SAMPLINGS:  # DC category 0 and only EOB
        info, coef, qt = _blank(jpeg, 17, 33, ss)
        cases[f"zeros {ss}"] = jpeg.JpegCoefficients(info, coef, qt)
    info, coef, qt = _blank(jpeg, 48, 8, "4:4:4")  # 6 MCUs: per component DC 1023, -1024, 1023 ... : differences 1023, -2047, +2047 ...
    _blocks(coef)[:, 0] = np.tile([1023, -1024], 9)
    cases["dc +-2047"] = jpeg.JpegCoefficients(info, coef, qt)
    info, coef, qt = _blank(jpeg, 40, 8, "4:4:4")
    b = _blocks(coef)
    b[:, 1:] = 1023
    b[1::2, 1:] = -1023
    b[::3, 5::7] = 0
    cases["ac +-1023"] = jpeg.JpegCoefficients(info, coef, qt)
    # one AC value at zigzag 16 (a run of exactly 15: no ZRL), 17 (a run of exactly 16: one ZRL), 33 (two), 49 (three), 63 (three, no EOB)
    for ss in ("4:4:4", "4:2:0"):
        info, coef, qt = _blank(jpeg, 40, 16, ss)
        b = _blocks(coef)
        for i in range(b.shape[0]):
            b[i, ZIGZAG[(16, 17, 33, 49, 63)[i % 5]]] = (3, -1, 1023, -1023, 1)[(i // 5) % 5]
            b[i, 0] = (i * 37) % 200 - 100
        cases[f"single ac {ss}"] = jpeg.JpegCoefficients(info, coef, qt)
    info, coef, qt = _blank(jpeg, 24, 8, "4:2:2")  # runs of 15 and 16 between two values, in every block
    b = _blocks(coef)
    b[:, ZIGZAG[1]] = 5
    b[0::2, ZIGZAG[17]] = -7  # 15 zeros between zigzag 1 and 17
    b[1::2, ZIGZAG[18]] = 9   # 16 zeros between zigzag 1 and 18
    b[:, ZIGZAG[34]] = 2      # and 16 resp. 15 zeros again
    cases["runs 15 16"] = jpeg.JpegCoefficients(info, coef, qt)
    for W in (8, 16, 24, 32):  # the last Cr block ends in 1023 at zigzag 63: the padded last byte is FF and gets its 00
        info, coef, qt = _blank(jpeg, W, 8, "4:2:0")
        coef[-1] = 1023
        coef[5] = W  # (moves the bit phase of the end from case to case)
        cases[f"last byte ff {W}"] = jpeg.JpegCoefficients(info, coef, qt)
    for density, seed in ((0.01, 1), (0.1, 2), (1.0, 3)):
        for k, (W, H, ss) in enumerate(((40, 24, "4:2:0"), (33, 17, "4:2:2"), (23, 41, "4:4:4"))):
            info, coef, qt = _blank(jpeg, W, H, ss)
            rng = np.random.default_rng(100 * seed + k)
            b = _blocks(coef)
            b[:] = np.where(rng.random(b.shape) < density, rng.integers(-1023, 1024, b.shape), 0)
            b[:, 0] = rng.integers(-1000, 1001, b.shape[0])  # (any two differ by less than 2047)
            cases[f"random {density} {ss}"] = jpeg.JpegCoefficients(info, coef, qt)
    return cases


# ------------------------------------------------------------------------------------- the host files, read back
def scan_of(jpeg, c, file):
    """The bytes between the SOS header and EOI of a host file."""
    head = jpeg.write_headers(c.qtables, c.info)
    assert file.startswith(head) and file.endswith(b"\xff\xd9")
    return file[len(head):-2]


def code_sizes(file):
    """{(class, id): {symbol: code length}} from the DHT segments of a file."""
    out, o = {}, 2
    while file[o + 1] != 0xDA:
        marker, size = file[o + 1], (file[o + 2] << 8) | file[o + 3]
        if marker == 0xC4:
            seg = file[o + 4:o + 2 + size]
            counts, vals, k, sizes = seg[1:17], seg[17:], 0, {}
            for length in range(1, 17):
                for _ in range(counts[length - 1]):
                    sizes[vals[k]] = length
                    k += 1
            out[seg[0] >> 4, seg[0] & 15] = sizes
        o += 2 + size
    return out


def scan_order(info):
    """(component, block index inside the component) of every block, in scan order."""
    order = []
    for my in range(info.mcus_y):
        for mx in range(info.mcus_x):
            for c in range(3):
                h, v = (info.hs, info.vs) if c == 0 else (1, 1)
                for bv in range(v):
                    for bh in range(h):
                        order.append((c, (my * v + bv) * info.comp_bw[c] + mx * h + bh))
    return order


def scan_bits(c, file):
    """Bits of the scan before padding, recomputed from the coefficients with the code lengths the file's DHT segments state."""
    sizes = code_sizes(file)
    info, planes, at = c.info, [], 0
    for k in range(3):
        nb = info.comp_bw[k] * info.comp_bh[k]
        planes.append(c.coef[at:at + 64 * nb].reshape(nb, 64).astype(np.int64))
        at += 64 * nb
    pred, bits = [0, 0, 0], 0
    for comp, idx in scan_order(info):
        zz = planes[comp][idx][ZIGZAG]
        dc, ac = sizes[0, min(comp, 1)], sizes[1, min(comp, 1)]
        s = int(abs(zz[0] - pred[comp])).bit_length()
        pred[comp] = zz[0]
        bits += dc[s] + s
        prev = 0
        for k in np.flatnonzero(zz[1:]) + 1:
            run = k - prev - 1
            prev = k
            bits += (run // 16) * ac[0xF0]
            s = int(abs(zz[k])).bit_length()
            bits += ac[((run % 16) << 4) | s] + s
        if prev != 63:
            bits += ac[0]
    return bits


_HOST = {}


def host_file(jpeg, name, c):
    if name not in _HOST:
        _HOST[name] = jpeg.entropy_encode(c)
    return _HOST[name]


def test_the_hand_made_set_covers_every_bit_and_byte_phase(jpeg):
    """Computed from the host coder alone: the scans of the hand-made set end at all eight bit positions of a byte and at all
    four byte positions of a word (the packer writes 32-bit words), one stream has a stuffed byte in its middle, and the
    'last byte ff' files end FF 00 FF D9."""
    bit_phases, byte_phases, stuffed_inside = set(), set(), 0
    for name, c in hand_made(jpeg).items():
        f = host_file(jpeg, name, c)
        scan = scan_of(jpeg, c, f)
        bits = scan_bits(c, f)
        unstuffed = scan.replace(b"\xff\x00", b"\xff")
        assert len(unstuffed) == (bits + 7) // 8, name
        bit_phases.add(bits % 8)
        byte_phases.add(len(unstuffed) % 4)
        stuffed_inside += b"\xff\x00" in scan[:-2]
        if name.startswith("last byte ff"):
            assert f.endswith(b"\xff\x00\xff\xd9"), name
    assert bit_phases == set(range(8)), bit_phases
    assert byte_phases == set(range(4)), byte_phases
    assert stuffed_inside >= 1


# ------------------------------------------------------------------------------------------------- the raw call
def _guarded(sizes):
    """A canary-filled device buffer with a region of each size, GUARD bytes before, between and behind them."""
    offs, at = [], GUARD
    for s in sizes:
        offs.append(at)
        at += _align(s) + GUARD
    t = torch.full((at,), CANARY, dtype=torch.uint8, device=DEV)
    assert t.data_ptr() % 256 == 0
    return t, offs


def raw_entropy(jpeg, coefs, capacities=None):
    """pp_jpeg_entropy_encode_batch on buffers of this test's own: every scratch share, every stream and the result slots
    inside canary bytes. Runs the call twice, the second time into fresh buffers. Returns [(status, bytes, stream)]."""
    _lib = jpeg._lib
    n = len(coefs)
    infos = [c.info for c in coefs]
    shares = [int(_lib.lib.pp_jpeg_entropy_scratch_bytes(ctypes.byref(i), 1)) for i in infos]
    assert min(shares) > 0 and all(s % 256 == 0 for s in shares)
    assert sum(shares) == int(_lib.lib.pp_jpeg_entropy_scratch_bytes((jpeg.JpegInfo * n)(*infos), n))
    if capacities is None:
        capacities = [int(_lib.lib.pp_jpeg_encoded_bound(ctypes.byref(i))) for i in infos]
    c_off, at = [], 0
    for c in coefs:
        c_off.append(at)
        at = _align(at + 2 * c.coef.size)
    coef_host = np.full(at, 0x5A, np.uint8)
    for o, c in zip(c_off, coefs):
        coef_host[o:o + 2 * c.coef.size] = np.ascontiguousarray(c.coef, np.int16).view(np.uint8)
    coef_d = torch.from_numpy(coef_host).to(DEV)
    assert coef_d.data_ptr() % 256 == 0
    runs = []
    for _ in range(2):
        scratch, s_off = _guarded(shares)
        out, o_off = _guarded(capacities)
        res, (r_off,) = _guarded([16 * n])
        desc = np.zeros(n, jpeg._ENT_DESC)
        for i, info in enumerate(infos):
            desc[i] = (coef_d.data_ptr() + c_off[i], scratch.data_ptr() + s_off[i], out.data_ptr() + o_off[i], res.data_ptr() + r_off + 16 * i,
                       capacities[i], info.hs, info.vs, info.mcus_x, info.mcus_y, 0)
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(DEV)
        _lib.reset_launch_counts()
        _lib.call("pp_jpeg_entropy_encode_batch", desc_d.data_ptr(), n, max(int(i.coef_count) // 64 for i in infos),
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        tags = ("jpeg_ent_bits", "jpeg_ent_scan", "jpeg_ent_zero", "jpeg_ent_pack", "jpeg_ent_ffcount", "jpeg_ent_ffscan", "jpeg_ent_stuff")
        assert [_lib.launch_count(t) for t in tags] == [1] * 7 and _lib.launch_count("pp_jpeg_entropy.hip") == 7
        assert np.array_equal(coef_d.cpu().numpy(), coef_host), "the kernels changed the coefficients"
        assert np.array_equal(desc_d.cpu().numpy(), desc.view(np.uint8))
        scratch_h, out_h, res_h = scratch.cpu().numpy(), out.cpu().numpy(), res.cpu().numpy()
        mask = np.ones(scratch_h.size, bool)
        for o, s in zip(s_off, shares):
            mask[o:o + s] = False
        assert (scratch_h[mask] == CANARY).all(), "bytes outside the scratch shares written"
        slots = res_h[r_off:r_off + 16 * n].view(jpeg._ENT_RESULT)
        mask = np.ones(res_h.size, bool)
        mask[r_off:r_off + 16 * n] = False
        assert (res_h[mask] == CANARY).all(), "bytes outside the result slots written"
        mask, got = np.ones(out_h.size, bool), []
        for o, cap, r in zip(o_off, capacities, slots):
            status, size = int(r["status"]), int(r["bytes"])
            used = size if status == _lib.PP_OK else (0 if status == _lib.PP_ERR_WORKSPACE else min(size, cap))
            assert 0 <= used <= cap
            mask[o:o + used] = False
            got.append((status, size, out_h[o:o + used].tobytes()))
        assert (out_h[mask] == CANARY).all(), "bytes behind a stream written"
        runs.append(got)
    ok = [g[0] == _lib.PP_OK for g in runs[0]]
    assert [g for g, k in zip(runs[0], ok) if k] == [g for g, k in zip(runs[1], ok) if k], "a second launch into fresh buffers gives other bytes"
    assert [g[0] for g in runs[0]] == [g[0] for g in runs[1]]
    return runs[0]


def check_batch(jpeg, named):
    """named: [(name, JpegCoefficients)] coded as one batch; every file equals the host coder's."""
    got = raw_entropy(jpeg, [c for _, c in named])
    bad = []
    for (name, c), (status, size, stream) in zip(named, got):
        want = scan_of(jpeg, c, host_file(jpeg, name, c))
        if status != 0 or size != len(want) or stream != want:
            first = next((i for i, (a, b) in enumerate(zip(stream, want)) if a != b), min(len(stream), len(want)))
            bad.append((name, status, size, len(want), first))
    assert not bad, f"{len(bad)} of {len(named)} streams differ (name, status, bytes, host bytes, first difference): {bad[:8]}"


_REAL = {}


def real_cases(jpeg):
    """[(name, JpegCoefficients)] of forward_batch on every size x sampling x quality x content, computed once."""
    if not _REAL:
        for ss in SAMPLINGS:
            for q in QUALITIES:
                keys = [(content, W, H) for (W, H) in SIZES for content in CONTENTS]
                imgs = [torch.from_numpy(E.image(*k).copy()).to(DEV) for k in keys]
                for k, c in zip(keys, jpeg.forward_batch(imgs, q, ss, "rgb")):
                    _REAL[f"{k[0]} {k[1]}x{k[2]} {ss} q{q}"] = c
    return list(_REAL.items())


def test_real_images_as_one_mixed_batch_with_a_1x1_image_behind_the_largest(jpeg):
    named = real_cases(jpeg)
    assert len(named) == len(SIZES) * len(SAMPLINGS) * len(QUALITIES) * len(CONTENTS)
    big = [i for i, (n, c) in enumerate(named) if c.info.width == 250]
    small = [i for i, (n, c) in enumerate(named) if c.info.width == 1]
    order = [i for i in range(len(named)) if i not in small] + small  # every 1x1 image comes after every 250x130 one
    assert max(order.index(i) for i in big) < min(order.index(i) for i in small)
    for _, c in named:
        if c.info.width == 250:
            assert (c.coef.size // 64) % ENT_CHUNK != 0 and c.coef.size // 64 > 3 * ENT_CHUNK
    longest = max(len(host_file(jpeg, n, c)) for n, c in named)
    assert longest > 8 * STUFF_CHUNK
    check_batch(jpeg, [named[i] for i in order])


def test_real_images_singly_across_the_chunk_edges(jpeg):
    """n = 1: the grids are sized by the image itself. The 250 x 130 noise pictures at quality 100 (the longest streams)."""
    for name, c in real_cases(jpeg):
        if name.startswith("noise 250x130") and name.endswith("q100"):
            check_batch(jpeg, [(name, c)])


def test_hand_made_coefficients(jpeg):
    named = list(hand_made(jpeg).items())
    check_batch(jpeg, named)
    for pair in named[::4]:
        check_batch(jpeg, [pair])


def test_entropy_encode_device_returns_the_host_files(jpeg):
    named = list(hand_made(jpeg).items())
    before = jpeg.entropy_device_calls
    files = jpeg.entropy_encode_device([c for _, c in named], DEV)
    assert jpeg.entropy_device_calls == before + 1
    assert files == [host_file(jpeg, n, c) for n, c in named]
    assert jpeg.entropy_encode_device([], DEV) == []


def _invalid(jpeg):
    info, coef, qt = _blank(jpeg, 32, 8, "4:4:4")
    _blocks(coef)[:, 0] = np.tile([1024, -1024], 6)  # DC differences of 2048
    return jpeg.JpegCoefficients(info, coef, qt)


def test_an_invalid_image_fails_alone(jpeg):
    _lib = jpeg._lib
    hm = hand_made(jpeg)
    batch = [("ac +-1023", hm["ac +-1023"]), ("invalid", _invalid(jpeg)), ("random 0.1 4:2:0", hm["random 0.1 4:2:0"])]
    got = raw_entropy(jpeg, [c for _, c in batch])
    assert [g[0] for g in got] == [_lib.PP_OK, _lib.PP_ERR_INVALID_ARG, _lib.PP_OK]
    for i in (0, 2):
        assert got[i][2] == scan_of(jpeg, batch[i][1], host_file(jpeg, *batch[i]))
    with pytest.raises(_lib.ProbPoseLibraryError) as host:
        jpeg.entropy_encode(batch[1][1])
    # the path encode_batch(entropy="device") takes from the result slots on (_entropy_collect): no picture quantises to a DC
    # difference of 2048, so the slots are reached with hand-made coefficients
    with pytest.raises(type(host.value)) as dev:
        jpeg.entropy_encode_device([c for _, c in batch], DEV)
    assert dev.value.status == host.value.status == "PP_ERR_INVALID_ARG"
    ac = _blank(jpeg, 8, 8, "4:2:0")
    ac[1][7] = 1024
    assert raw_entropy(jpeg, [jpeg.JpegCoefficients(*ac)])[0][0] == _lib.PP_ERR_INVALID_ARG


def test_a_capacity_below_the_need_is_reported_and_nothing_is_written(jpeg):
    _lib = jpeg._lib
    hm = hand_made(jpeg)
    batch = [("random 1.0 4:4:4", hm["random 1.0 4:4:4"]), ("random 1.0 4:2:0", hm["random 1.0 4:2:0"])]
    need = [len(scan_of(jpeg, c, host_file(jpeg, n, c))) for n, c in batch]
    got = raw_entropy(jpeg, [c for _, c in batch], capacities=[need[0] - 1, need[1]])
    assert (got[0][0], got[0][1]) == (_lib.PP_ERR_WORKSPACE, need[0])
    assert got[1] == (_lib.PP_OK, need[1], scan_of(jpeg, batch[1][1], host_file(jpeg, *batch[1])))
    assert _lib.lib.pp_jpeg_entropy_encode_batch(None, 0, 0, None) == _lib.PP_OK


def test_encode_batch_with_device_entropy_equals_host_entropy(jpeg):
    rgbs = [E.image("noise", 250, 130), E.image("gradient", 17, 33), E.image("checker", 9, 17)]
    for ss in SAMPLINGS:
        for order in ("bgr", "rgb"):
            frames = [torch.from_numpy(np.array(r if order == "rgb" else r[:, :, ::-1], order="C")).to(DEV) for r in rgbs]
            calls = jpeg.entropy_device_calls
            host = jpeg.encode_batch(frames, quality=75, subsampling=ss, channel_order=order, entropy="host")
            assert jpeg.entropy_device_calls == calls, "the host path counted a device call"
            dev = jpeg.encode_batch(frames, quality=75, subsampling=ss, channel_order=order, entropy="device")
            assert jpeg.entropy_device_calls == calls + 1, "one device call per batch"
            assert dev == host, (ss, order, [len(a) == len(b) for a, b in zip(dev, host)])


def test_imwrite_device_passes_the_keyword_through(jpeg, tmp_path):
    t = torch.from_numpy(E.image("noise", 17, 33).copy()).to(DEV)
    calls = jpeg.entropy_device_calls
    jpeg.imwrite_device(str(tmp_path / "d.jpg"), t, channel_order="rgb", entropy="device")
    jpeg.imwrite_device(str(tmp_path / "h.jpg"), t, channel_order="rgb")
    assert jpeg.entropy_device_calls == calls + 1
    assert open(tmp_path / "d.jpg", "rb").read() == open(tmp_path / "h.jpg", "rb").read()
