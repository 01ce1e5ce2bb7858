"""Hand-made coefficient sets for the device Huffman coder with restart intervals, and the reading of a host file's scan that
proves what each set contains. Everything here is the host coder's (``jpeg.entropy_encode``) or plain arithmetic on the
coefficients with the code lengths a file's own DHT segments state - nothing of the code under test. The CPU test asserts the
forms, the GPU test codes the same sets."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_jpeg_entropy_gpu import ZIGZAG, code_sizes, scan_order  # noqa: E402

ENT_CHUNK = 256     # blocks per workgroup of the bit phases
STUFF_CHUNK = 2048  # unstuffed bytes per workgroup pass of the stuffing phases


def blank(jpeg, W, H, ss, quality=75):
    info = jpeg.encode_plan(W, H, ss)
    return info, np.zeros(int(info.coef_count), np.int16), jpeg.quality_tables(quality)


def mcu_blocks(info):
    """Per MCU the flat block indices (into coef.reshape(-1, 64)) of its blocks, in scan order."""
    base = [0, info.comp_bw[0] * info.comp_bh[0], info.comp_bw[0] * info.comp_bh[0] + info.comp_bw[1] * info.comp_bh[1]]
    bpm = info.hs * info.vs + 2
    flat = [base[c] + i for c, i in scan_order(info)]
    return [flat[m * bpm:(m + 1) * bpm] for m in range(info.mcus_x * info.mcus_y)]


def split_scan(scan: bytes):
    """The entropy-coded bytes of a file (SOS header to EOI, both excluded) -> (the unstuffed bytes of every interval, the
    marker numbers between them). In such bytes FF is followed by 00 (a data FF) or by D0..D7 (a marker)."""
    parts, markers, cur, i = [], [], bytearray(), 0
    while i < len(scan):
        b = scan[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        nxt = scan[i + 1]
        if nxt == 0:
            cur.append(0xFF)
        else:
            assert 0xD0 <= nxt <= 0xD7, f"FF {nxt:02X} inside a scan"
            parts.append(bytes(cur))
            markers.append(nxt - 0xD0)
            cur = bytearray()
        i += 2
    parts.append(bytes(cur))
    return parts, markers


def interval_bits(c, file: bytes, R: int, reset: bool = True):
    """Bits of every restart interval before padding, from the coefficients and the code lengths of the file's DHT segments.
    ``reset=False``: with the DC prediction carried across the interval starts (what a coder without the reset would count)."""
    sizes = code_sizes(file)
    info, planes, at = c.info, [], 0
    for k in range(3):
        nb = info.comp_bw[k] * info.comp_bh[k]
        planes.append(np.asarray(c.coef[at:at + 64 * nb]).reshape(nb, 64).astype(np.int64))
        at += 64 * nb
    bpm = info.hs * info.vs + 2
    mcus = info.mcus_x * info.mcus_y
    per = mcus if (R <= 0 or R >= mcus) else R
    out, pred, bits = [], [0, 0, 0], 0
    for s, (comp, idx) in enumerate(scan_order(info)):
        mcu = s // bpm
        if s % bpm == 0 and mcu > 0 and mcu % per == 0:
            out.append(bits)
            bits = 0
            if reset:
                pred = [0, 0, 0]
        zz = planes[comp][idx][ZIGZAG]
        dc, ac = sizes[0, min(comp, 1)], sizes[1, min(comp, 1)]
        n = int(abs(zz[0] - pred[comp])).bit_length()
        pred[comp] = zz[0]
        bits += dc[n] + n
        prev = 0
        for k in np.flatnonzero(zz[1:]) + 1:
            run = k - prev - 1
            prev = k
            bits += (run // 16) * ac[0xF0]
            n = int(abs(zz[k])).bit_length()
            bits += ac[((run % 16) << 4) | n] + n
        if prev != 63:
            bits += ac[0]
    out.append(bits)
    return out


def scan_of(jpeg, c, file: bytes, R: int, tables=None) -> bytes:
    """The bytes between the SOS header and EOI of a host file coded at interval R."""
    head = jpeg.write_headers(c.qtables, c.info, R, tables)
    assert file.startswith(head) and file.endswith(b"\xff\xd9")
    return file[len(head):-2]


def plain_scan(file: bytes) -> bytes:
    """The same for any file: from behind its SOS header to its EOI."""
    o = 2
    while file[o + 1] != 0xDA:
        o += 2 + ((file[o + 2] << 8) | file[o + 3])
    o += 2 + ((file[o + 2] << 8) | file[o + 3])
    assert file.endswith(b"\xff\xd9")
    return file[o:-2]


def hand_made(jpeg):
    """name -> (JpegCoefficients, restart interval). What each is for is asserted by tests/test_jpeg_entropy_restart_host.py."""
    cases = {}
    # 64 MCUs of 4:4:4 with a few small values each, one MCU per interval: interval ends at every bit phase, marker numbers wrap
    info, coef, qt = blank(jpeg, 512, 8, "4:4:4")
    rng = np.random.default_rng(7)
    b = coef.reshape(-1, 64)
    b[:, ZIGZAG[1:6]] = rng.integers(-9, 10, (b.shape[0], 5))
    b[:, 0] = rng.integers(-300, 301, b.shape[0])
    cases["phases r1"] = (jpeg.JpegCoefficients(info, coef, qt), 1)
    # every MCU's last (Cr) block ends in 1023 at zigzag 63 - ten one bits - and a luma value moves the phase from MCU to MCU:
    # intervals end in FF, as a padded byte and as a whole data byte
    for ss, W in (("4:4:4", 256), ("4:2:0", 512)):
        info, coef, qt = blank(jpeg, W, 8 if ss == "4:4:4" else 16, ss)
        b = coef.reshape(-1, 64)
        for m, blocks in enumerate(mcu_blocks(info)):
            b[blocks[-1], 63] = 1023
            b[blocks[0], ZIGZAG[1]] = (1, 2, 4, 8, 16, 32, 64, 128)[m % 8] * (1 if m % 3 else -1)
            b[blocks[0], ZIGZAG[2]] = m % 5
        cases[f"ff ends {ss}"] = (jpeg.JpegCoefficients(info, coef, qt), 1)
    # 20 MCUs, random: three MCUs per interval (seven intervals, the last of two MCUs), two (ten intervals: the numbers wrap)
    for R in (3, 2):
        info, coef, qt = blank(jpeg, 80, 64, "4:2:0")
        assert info.mcus_x * info.mcus_y == 20
        rng = np.random.default_rng(11 + R)
        b = coef.reshape(-1, 64)
        b[:] = np.where(rng.random(b.shape) < 0.2, rng.integers(-1023, 1024, b.shape), 0)
        b[:, 0] = rng.integers(-1000, 1001, b.shape[0])
        cases[f"ragged r{R}"] = (jpeg.JpegCoefficients(info, coef, qt), R)
    # an interval of at least the MCU count: DRI in the header, no marker in the scan
    for name in ("whole", "beyond", "largest"):
        info, coef, qt = blank(jpeg, 33, 17, "4:2:2")
        rng = np.random.default_rng(5)
        b = coef.reshape(-1, 64)
        b[:] = np.where(rng.random(b.shape) < 0.1, rng.integers(-1023, 1024, b.shape), 0)
        b[:, 0] = rng.integers(-1000, 1001, b.shape[0])
        mcus = info.mcus_x * info.mcus_y
        cases[f"single {name}"] = (jpeg.JpegCoefficients(info, coef, qt), {"whole": mcus, "beyond": mcus + 1, "largest": 65535}[name])
    # one MCU per interval in 4:4:4, all zero: fourteen bits, two bytes an interval with annex K's tables, six bits, one byte
    # with the single-symbol optimised ones - eight bytes hold four resp. eight interval ends
    info, coef, qt = blank(jpeg, 96, 8, "4:4:4")
    cases["zeros r1"] = (jpeg.JpegCoefficients(info, coef, qt), 1)
    info, coef, qt = blank(jpeg, 96, 8, "4:4:4")  # and with a value in every other MCU: two and three bytes
    coef.reshape(-1, 64)[0:12:2, ZIGZAG[1]] = 3
    cases["short r1"] = (jpeg.JpegCoefficients(info, coef, qt), 1)
    # DC values far from zero and close to each other: the reset at an interval start changes the code of its first blocks
    info, coef, qt = blank(jpeg, 64, 16, "4:2:0")
    coef.reshape(-1, 64)[:, 0] = 900 + np.arange(coef.size // 64) % 7
    cases["dc reset r1"] = (jpeg.JpegCoefficients(info, coef, qt), 1)
    return cases


def reset_decides(jpeg):
    """name -> (JpegCoefficients, R, valid): 4:4:4, one MCU row. 'ramp': every component's DC climbs 0, 1000, 2000, 3000 - legal
    differences unless an interval starts at 3000 (R = 1 and R = 3: a difference of 3000, beyond 2047, only because of the reset).
    'swing': -1500, 1500, -1500, 1500 - differences of 3000 unless every MCU starts an interval (R = 1)."""
    out = {}
    for name, dcs in (("ramp", (0, 1000, 2000, 3000)), ("swing", (-1500, 1500, -1500, 1500))):
        for R in (0, 1, 2, 3):
            info, coef, qt = blank(jpeg, 32, 8, "4:4:4")
            coef.reshape(3, 4, 64)[:, :, 0] = dcs
            valid = (R in (0, 2)) if name == "ramp" else (R == 1)
            out[f"{name} r{R}"] = (jpeg.JpegCoefficients(info, coef, qt), R, valid)
    return out
