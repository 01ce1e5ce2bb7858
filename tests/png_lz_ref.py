"""What the PNG writer's ``lz`` match mode prescribes, restated without the library: the candidates' match lengths, the choice
with its one-byte lookahead and margin and the chain of token starts in numpy (``tokens``), and a reader of the tokens of a
zlib stream with one dynamic deflate block (``read_tokens``), so that a test pins the format and not just the round trip.
A token is an int (a literal's byte) or a pair (length, distance). Both test files of the mode (tests/test_png_lz_host.py,
tests/test_png_lz_gpu.py) share the cases below, computed once (do not modify)."""
import numpy as np

import png_ref as R

TILE = R.TILE
NEAR = (1, 3)
NEAR_MIN, FAR_MIN, MARGIN = 3, 4, 3


def far_candidates(period: int):
    """F = (P, P - 3, P + 3) in this order without the members below 4 or above 32768; empty for period 0."""
    return tuple(d for d in (period, period - 3, period + 3) if period > 0 and 4 <= d <= 32768)


def match_lengths(s: np.ndarray, d: int) -> np.ndarray:
    """m_d(g) for every g: 0 if g < d, else the largest m <= min(258, E(g) - g) with s[g + i] == s[g + i - d] for i < m."""
    n = s.size
    g = np.arange(n, dtype=np.int64)
    eq = np.zeros(n, bool)
    if d < n:
        eq[d:] = s[d:] == s[:-d]
    first_unequal = np.minimum.accumulate(np.where(eq, n, g)[::-1])[::-1]  # at or behind g
    end = np.minimum(n, TILE * (g // TILE + 1))
    return np.minimum(np.minimum(first_unequal, end) - g, 258)


def _best(s, cands, minimum):
    """(the largest m_d over the candidates where it reaches the minimum, else 0; the first d that attains it)."""
    best = np.zeros(s.size, np.int64)
    dist = np.zeros(s.size, np.int64)
    for d in cands:
        m = match_lengths(s, d)
        better = m > best  # (strictly: the first candidate keeps a tie)
        best[better], dist[better] = m[better], d
    best[best < minimum] = 0
    return best, dist


def choices(stream: bytes, period: int = 0):
    """Per position: (Ln, dn, Lf, df, reach, kind) with kind 0 a literal, 1 the near match, 2 the far match - what the
    position emits if it starts a token."""
    s = np.frombuffer(stream, np.uint8)
    n = s.size
    g = np.arange(n, dtype=np.int64)
    end = np.minimum(n, TILE * (g // TILE + 1))
    ln, dn = _best(s, NEAR, NEAR_MIN)
    lf, df = _best(s, far_candidates(period), FAR_MIN)
    ahead = np.zeros(n, np.int64)
    ahead[:-1] = ln[1:]
    ahead[g + 1 >= end] = 0
    reach = np.where(ahead > 0, np.maximum(ln, 1 + ahead), ln)
    kind = np.where((lf > 0) & (lf >= reach + MARGIN), 2, np.where(ln > 0, 1, 0))
    return ln, dn, lf, df, reach, kind


def tokens(stream: bytes, period: int = 0, with_starts: bool = False):
    """The token sequence of a stream: a tile's first byte starts a token, and so does the byte behind every token."""
    ln, dn, lf, df, _, kind = (a.tolist() for a in choices(stream, period))
    out, starts, n = [], [], len(stream)
    for t0 in range(0, n, TILE):
        p, t1 = t0, min(n, t0 + TILE)
        while p < t1:
            starts.append(p)
            if kind[p] == 2:
                out.append((lf[p], df[p]))
                p += lf[p]
            elif kind[p] == 1:
                out.append((ln[p], dn[p]))
                p += ln[p]
            else:
                out.append(stream[p])
                p += 1
        assert p == t1, "a match crossed its tile's border"
    return (out, starts) if with_starts else out


# --------------------------------------------------------------------------------------------------------- the reader
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class _Bits:
    def __init__(self, data: bytes):
        self.data, self.at, self.acc, self.n = data, 0, 0, 0

    def need(self, k):
        while self.n < k:
            self.acc |= (self.data[self.at] if self.at < len(self.data) else 0) << self.n
            self.at += 1
            self.n += 8

    def take(self, k):
        self.need(k)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v


def _table(lengths):
    """{(length, code read LSB-first as its bits arrive): symbol} of a canonical code, which must be complete."""
    per, code, nxt = [0] * 17, 0, [0] * 17
    for l in lengths:
        per[l] += 1
    per[0] = 0
    for l in range(1, 17):
        code = (code + per[l - 1]) << 1
        nxt[l] = code
    assert sum(per[l] << (16 - l) for l in range(1, 17)) == 1 << 16, "the code is not complete"
    table = {}
    for sym, l in enumerate(lengths):
        if l:
            table[l, nxt[l]] = sym
            nxt[l] += 1
    return table


def _symbol(bits: _Bits, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | bits.take(1)
        sym = table.get((l, code))
        if sym is not None:
            return sym
    raise AssertionError("no code matches the bits")


def read_tokens(z: bytes, with_header: bool = False):
    """The tokens of a zlib stream that holds one final dynamic block; with_header also {hlit, hdist, lengths}. Checks the
    zlib header, that both codes are complete, that the block is final and that the Adler-32 follows it at a byte border."""
    assert z[0] == 0x78 and (z[0] * 256 + z[1]) % 31 == 0 and not z[1] & 0x20
    bits = _Bits(z[2:])
    assert bits.take(1) == 1 and bits.take(2) == 2, "one final dynamic block"
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[_CL_ORDER[i]] = bits.take(3)
    cl_table = _table(cl)
    lengths = []
    while len(lengths) < hlit + hdist:
        sym = _symbol(bits, cl_table)
        if sym < 16:
            lengths.append(sym)
        elif sym == 16:
            lengths += [lengths[-1]] * (3 + bits.take(2))
        elif sym == 17:
            lengths += [0] * (3 + bits.take(3))
        else:
            lengths += [0] * (11 + bits.take(7))
    assert len(lengths) == hlit + hdist
    lit, dist = _table(lengths[:hlit]), _table(lengths[hlit:]) if sum(1 for l in lengths[hlit:] if l) > 1 else None
    if dist is None:  # one distance code of one bit (what runs mode writes)
        dist = {(l, 0): s for s, l in enumerate(lengths[hlit:]) if l}
    out = []
    while True:
        sym = _symbol(bits, lit)
        if sym < 256:
            out.append(sym)
        elif sym == 256:
            break
        else:
            length = _LEN_BASE[sym - 257] + bits.take(_LEN_EXTRA[sym - 257])
            d = _symbol(bits, dist)
            out.append((length, _DIST_BASE[d] + bits.take(_DIST_EXTRA[d])))
    bits.take(bits.n % 8)
    at = 2 + bits.at - bits.n // 8
    assert at + 4 == len(z), "the Adler-32 does not end the stream"
    return (out, {"hlit": hlit, "hdist": hdist, "lengths": lengths}) if with_header else out


def expand(toks) -> bytes:
    """The bytes a token list stands for."""
    out = bytearray()
    for t in toks:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------- the cases
_PICTURES, _STREAMS = {}, {}


def _repeat_rows(rng, width, height):
    row = rng.integers(0, 256, (1, width, 3), dtype=np.uint8)
    return np.repeat(row, height, axis=0)


def _walk_rows(rng, width, height):
    """A row that is a random walk of small steps, repeated with 128 added per row: Up leaves 128s, Sub leaves the steps, so
    every filtered row repeats the row above but for its first pixel."""
    row = np.cumsum(rng.integers(-9, 10, (1, width, 3)), axis=1)
    return ((row + 128 * np.arange(height)[:, None, None]) & 255).astype(np.uint8)


def pictures():
    """{name: (H, W, 3) uint8 RGB}: the pictures of this mode's own cases (those of png_ref come on top)."""
    if not _PICTURES:
        rng = np.random.default_rng(17)
        p = {
            "width 1": rng.integers(0, 4, (40, 1, 3), dtype=np.uint8),  # P = 4; P - 3 = 1 is dropped
            "width 2": rng.integers(0, 3, (40, 2, 3), dtype=np.uint8),
            "width 1365": _walk_rows(rng, 1365, 5),  # P = 4096: every far source lies in the tile before
            "width 10921 h2": _repeat_rows(rng, 10921, 2),  # P + 3 = 32767 in range
            "width 10921 h3": _repeat_rows(rng, 10921, 3),
            "width 10922 h2": _repeat_rows(rng, 10922, 2),  # P + 3 = 32770 dropped
            "width 10922 h3": _repeat_rows(rng, 10922, 3),
            "width 10923 h2": _repeat_rows(rng, 10923, 2),  # P = 32770 dropped, P - 3 = 32767 kept
            "width 10923 h3": _repeat_rows(rng, 10923, 3),
        }
        for v in p.values():
            v.setflags(write=False)
        _PICTURES.update(p)
    return _PICTURES


def margin_stream():
    """(a raw stream for period 100, the position where Lf = reach + 2 so that the near match is taken, the position where
    Lf = reach + 3 so that the far match is taken). Rows of 100 noise bytes below 200; a marked row holds five bytes of 250 from
    column 9 on, so at column 10 Ln = 4, Ln of the next byte is 3 and reach = 4; the row above repeats the marked row from
    column 10 on for Lf bytes."""
    rng = np.random.default_rng(23)
    rows = rng.integers(0, 200, (12, 100), dtype=np.uint8)
    marks = []
    for y, lf in ((3, 6), (7, 7)):
        rows[y, 9:14] = 250
        rows[y - 1, 10:10 + lf] = rows[y, 10:10 + lf]
        rows[y - 1, 10 + lf] = rows[y, 10 + lf] ^ 1
        rows[y - 1, 9] = 201
        marks.append(100 * y + 10)
    return rows.tobytes(), marks[0], marks[1]


def _gap(rng, base, gap):
    return base + bytes(rng.integers(0, 256, gap - len(base), dtype=np.uint8)) + base


def streams():
    """{name: (bytes, period)}: the raw streams of this mode's own cases."""
    if not _STREAMS:
        rng = np.random.default_rng(29)
        base = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
        cut = bytearray(rng.integers(0, 256, 2 * TILE, dtype=np.uint8).tobytes())
        cut[TILE - 20:TILE + 20] = bytes([77]) * 40  # a run over the border, and
        cut[TILE - 50:TILE - 20] = cut[TILE - 150:TILE - 120]  # a far match (period 100) that ends before it
        cut[TILE - 10:TILE + 30] = cut[TILE - 110:TILE - 70]  # a far match that would cross it
        one = bytearray(rng.integers(0, 256, 600, dtype=np.uint8).tobytes())
        for i in range(0, 600, 2):  # no byte equals the byte 1 or 3 before it ...
            one[i] = one[i] & 0x7F
            one[i + 1] = one[i + 1] | 0x80
        one[400:420] = one[300:320]  # ... and one far match at distance 100: exactly one distance symbol
        margin = margin_stream()[0]
        _STREAMS.update({
            "last tile of one byte": (R.streams()["sparse 70000"][:2 * TILE + 1], 0),
            "matches at a tile border": (bytes(cut), 100),
            "noise 8193": (R.streams()["noise 8193"], 0),
            "noise 8193 with a period": (R.streams()["noise 8193"], 64),
            "margin": (margin, 100),
            "g below d": (base[:50] + base[:50] + base[:50], 50),  # positions 0 .. 49 have no source at distance 50
            "period longer than the stream": (base, 1000),
            "one distance symbol": (bytes(one), 100),
            "no distance symbol": (bytes(one[:300]), 0),
            "long pixel run": (bytes([9, 140, 77]) * (258 + 258 + 2) + base[:40], 0),  # equal pixels: matches at distance 3
            "13 extra bits": (base + bytes(rng.integers(0, 256, 30000, dtype=np.uint8)) + base, 30300),
            "rows of 300 in three tiles": (bytes(rng.integers(0, 256, 300, dtype=np.uint8)) * 40, 300),
            # a repeat exactly `gap` bytes back, against periods whose P + 3, nothing, or P - 3 is that distance
            "P + 3 = 32767 in range": (_gap(rng, base, 32767), 32764),
            "P + 3 = 32770 dropped": (_gap(rng, base, 32770), 32767),
            "P = 32770 dropped, P - 3 kept": (_gap(rng, base, 32767), 32770),
        })
    return _STREAMS
