"""The inputs the restart-interval tests of the device Huffman decoder share (tests/test_jpeg_huffdec_restart_host.py, _gpu.py):
the restart files of the committed grid and of jpeg_sources' layouts, an independent search for the bounds of a segment
and its markers, the marker damage scripts/jpeg_huffdec_host_check.cpp runs under the sanitisers, and searches by content
seed for files in which a marker meets a given boundary situation. Everything is made once and cached; do not modify what
these functions return."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import jpeg_ref as J  # noqa: E402
import jpeg_sources as S  # noqa: E402
from make_golden_jpeg import content, encode  # noqa: E402

SUB = 128  # HD_S: raw bytes per subsequence
WG = 256  # HD_WG: subsequences per workgroup
MAX_H, MAX_W = 256, 320  # no picture of these tests is larger
SITUATIONS = ("ff_at_127", "ff_at_0", "ff_at_126", "after_ff00", "aligned", "pad7")

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def golden_restart():
    """name -> bytes: the committed grid's files with a restart interval (r1, r3)."""
    g = J.golden()
    return {n: g["jpg"][n] for n in g["names"] if n.endswith(("_r1", "_r3"))}


def golden_plain(count: int):
    g = J.golden()
    names = [n for n in g["names"] if n.endswith("_r0")]
    return [g["jpg"][n] for n in names[::max(1, len(names) // count)][:count]]


def restart_layouts():
    """(source, layout) of jpeg_sources.layout_cases() with a DRI segment, pictures of at most MAX_H x MAX_W."""
    return [(s, l) for s, l in S.layout_cases() if S.LAYOUTS[l].get("restart") and S.SOURCES[s][0] <= MAX_H and S.SOURCES[s][1] <= MAX_W]


def _headers(data: bytes):
    """[(marker, payload)] up to and including SOS, and the offset behind the SOS header."""
    pos, out = 2, []
    while True:
        while data[pos] == 0xFF:
            pos += 1
        m, n = data[pos], (data[pos + 1] << 8) | data[pos + 2]
        out.append((m, data[pos + 3:pos + 1 + n]))
        pos += 1 + n
        if m == 0xDA:
            return out, pos


def frame(data: bytes):
    """(restart interval, luma blocks per MCU, MCUs) from the DRI and SOF segments."""
    ri, lum, mcus = 0, 1, 0
    for m, s in _headers(data)[0]:
        if m == 0xDD:
            ri = (s[0] << 8) | s[1]
        elif m in (0xC0, 0xC1):
            hs, vs = (s[7] >> 4, s[7] & 15) if s[5] == 3 else (1, 1)
            lum = hs * vs
            mcus = -(-((s[3] << 8) | s[4]) // (8 * hs)) * -(-((s[1] << 8) | s[2]) // (8 * vs))
    return ri, lum, mcus


def segment(data: bytes):
    """(offset, length, markers) of the entropy-coded segment of a file with one scan, by its own search: from behind the SOS
    header to the first FF that neither 00 nor - behind fill bytes - D0..D7 follows. markers: (offset of the first FF, offset
    of the D0..D7 byte) inside the segment."""
    pos = _headers(data)[1]
    start, p, marks = pos, pos, []
    while True:
        p = data.index(b"\xff", p)
        m = p + 1
        while data[m] == 0xFF:
            m += 1
        if data[m] == 0x00 and m == p + 1:
            p += 2
        elif 0xD0 <= data[m] <= 0xD7:
            marks.append((p - start, m - start))
            p = m + 1
        else:
            return start, p - start, marks


def dht_codes(data: bytes):
    """Per component of the scan (DC codes, AC codes) as {bit string: symbol}, read from the file's DHT and SOS segments."""
    dc, ac = {}, {}
    for m, s in _headers(data)[0]:
        if m == 0xC4:
            o = 0
            while o < len(s):
                counts = list(s[o + 1:o + 17])
                (ac if s[o] >> 4 else dc)[s[o] & 15] = J._huff_table(counts, list(s[o + 17:o + 17 + sum(counts)]))
                o += 17 + sum(counts)
        elif m == 0xDA:
            return [(dc[s[2 + 2 * c] >> 4], ac[s[2 + 2 * c] & 15]) for c in range(s[0])]


def paddings(data: bytes):
    """The padding bits in front of every marker (and of EOI): each interval decoded by the reference's bit reader."""
    off, n, marks = segment(data)
    tabs = dht_codes(data)
    ri, lum, mcus = frame(data)
    blocks = [t for c, t in enumerate(tabs) for _ in range(lum if c == 0 else 1)]
    bounds = [0] + [m + 1 for _, m in marks]
    ends = [f for f, _ in marks] + [n]
    out = []
    for lo, hi in zip(bounds, ends):
        br = J._Bits(data[off + lo:off + hi])
        for _ in range(min(ri, mcus)):
            for dct, act in blocks:
                sz = br.symbol(dct)
                br.p += sz
                k = 1
                while k < 64:
                    rs = br.symbol(act)
                    if rs & 15 == 0:
                        if rs >> 4 != 15:
                            break
                        k += 16
                        continue
                    k += (rs >> 4) + 1
                    br.p += rs & 15
        mcus -= min(ri, mcus)
        out.append(len(br.bits) - br.p)
    return out


def situations(data: bytes) -> set:
    """Which of SITUATIONS the markers of a restart file meet."""
    off, n, marks = segment(data)
    found = set()
    for f, _ in marks:
        for name, r in (("ff_at_127", 127), ("ff_at_0", 0), ("ff_at_126", 126)):
            if f % SUB == r:
                found.add(name)
        if f >= 2 and data[off + f - 2:off + f] == b"\xff\x00":
            found.add("after_ff00")
    pads = paddings(data)[:-1]
    if 0 in pads:
        found.add("aligned")
    if 7 in pads:
        found.add("pad7")
    return found


def find(situation: str, tries: int = 600) -> bytes:
    """A small Pillow file with a restart interval in which a marker meets ``situation``: sampling, quality, interval and content
    seed vary until one does. AssertionError if none of ``tries`` files does."""
    def make():
        for t in range(tries):
            sampling = ("420", "444", "grey", "422")[t % 4]
            kind = ("noise", "smooth", "bilevel")[t % 3]
            H, W = (24, 40) if situation in ("aligned", "pad7", "after_ff00") else (48, 72)
            data = encode(content(kind, H, W, 1 if sampling == "grey" else 3, np.random.default_rng([t, H, W])), sampling,
                          (95, 75, 100, 50, 88, 30, 98)[t % 7], (1, 2, 3)[t % 3])
            if situation in ("aligned", "pad7"):  # (these decode every interval: only then)
                if situation in situations(data):
                    return data
                continue
            off, _, marks = segment(data)
            at = {"ff_at_127": 127, "ff_at_0": 0, "ff_at_126": 126}.get(situation)
            if any(f % SUB == at if at is not None else (f >= 2 and data[off + f - 2:off + f] == b"\xff\x00") for f, _ in marks):
                return data
        raise AssertionError(f"no restart file with {situation} in {tries} tries")

    return _once(("find", situation), make)


def long_noise() -> bytes:
    """Uniform noise, 4:2:0, quality 95, a marker behind every MCU, a stream of more than 64 KiB (three workgroups) with a
    marker in the first and in the last subsequence of a workgroup's 256; the content seed varies until the markers lie so."""
    def make():
        for seed in range(200):
            data = encode(content("noise", MAX_H, MAX_W, 3, np.random.default_rng([95, seed])), "420", 95, 1)
            _, n, marks = segment(data)
            subs = {f // SUB % WG for f, _ in marks if f // SUB >= WG}
            if n > 65536 and 0 in subs and WG - 1 in {f // SUB % WG for f, _ in marks}:
                return data
        raise AssertionError("no noise picture with markers at a workgroup's first and last subsequence")

    return _once("long_noise", make)


def marker_damage(data: bytes):
    """[(kind, bytes)]: the marker damage of scripts/jpeg_huffdec_host_check.cpp on up to 12 markers of a file - one deleted, one
    doubled (an empty interval), two neighbours' numbers swapped, D7 changed to D0."""
    off, _, marks = segment(data)
    at = [off + m for f, m in marks if m == f + 1]
    out = []
    for q in range(0, len(at), max(1, len(at) // 12)):
        a = at[q]
        out.append(("deleted", data[:a - 1] + data[a + 1:]))
        out.append(("doubled", data[:a + 1] + data[a - 1:a + 1] + data[a + 1:]))
        if q + 1 < len(at):
            b = at[q + 1]
            out.append(("swapped", data[:a] + data[b:b + 1] + data[a + 1:b] + data[a:a + 1] + data[b + 1:]))
        if data[a] == 0xD7:
            out.append(("d7_to_d0", data[:a] + b"\xd0" + data[a + 1:]))
    return out


def bit_flips(data: bytes):
    """The 32 single bit flips at fixed places of the segment (markers included) the sanitiser program runs."""
    off, n, _ = segment(data)
    out = []
    for k in range(32):
        at = off + n * k // 32
        out.append(data[:at] + bytes([data[at] ^ (1 << (k % 8))]) + data[at + 1:])
    return out
