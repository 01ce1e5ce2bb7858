"""A test-side baseline JPEG writer: the quantised coefficients tests/jpeg_ref.py parsed out of a file, written back as a
Huffman stream of another layout - other tables, slots, segments, markers, restart intervals - that decodes to the very same
pixels. Plain Python and numpy: nothing of the product, nothing of any other project (the procedures are ITU T.81's:
annex K.2 for the tables, annex F.1.2 for the codes, annex B for the segments).

    write(parsed, **layout) -> bytes        parsed: what jpeg_ref.parse returns

The coefficient values are only ever those of an encoder's file: the writer moves them, it never invents any.

Layout knobs (defaults in brackets):
    restart     restart interval in MCUs, 0..65535 [0]: any value - one that does not divide an MCU row, one above the MCU count
    huffman     "optimal" [default]: the file's own statistics, T.81 K.2 with the 16-bit limit and the all-ones code reserved;
                "fibonacci": deliberately degenerate - Fibonacci weights, the smallest for the most common symbol - so that
                the symbols of everyday use get the longest codes (10..16 bits) and a decoder's short lookup table is no help
    dc_slots, ac_slots, q_slots     the table slot (0..3) of each component [(0, 1, 1)]; components that share a slot share
                a table: (0, 0, 0) is one Huffman pair for all of them
    dqt_split, dht_split    one segment per table instead of one segment that holds every table [False]
    pq          1: 16-bit quantisation table entries [0];  sof: 0xC0 or 0xC1 [0xC0]
    comp_ids    the component identifiers [(1, 2, 3)]
    fill        so many 0xFF fill bytes in front of every marker but SOI, RSTn and EOI included [0]
    jfif        an APP0 JFIF segment [True];  adobe: None or the transform byte of an APP14 Adobe segment [None]
    extra       further leading segments, in this order: any of "com", "app1" (Exif-like), "app2" [()]
    scans       "interleaved" [default] or "separate": one scan per component (which the split decoder must refuse)
``relayout(parsed, hs, vs)`` re-declares the block grids under another luma sampling (1x2: 4:4:0, 4x1: 4:1:1 - also refused)."""
import numpy as np

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                    21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                    61, 54, 47, 55, 62, 63])

# the symbols a baseline table may hold: DC categories, and AC (run, size) pairs with EOB and ZRL
DC_SYMBOLS = list(range(16))
AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]


# ------------------------------------------------------------------------------------------------ Huffman tables (T.81 K.2)
def code_lengths(freq: dict) -> dict:
    """symbol -> code length by figure K.1 (with the reserved symbol 256 of frequency 1) and figure K.3 (no code above 16
    bits); the reserved symbol is dropped from the longest length, so no code is all ones."""
    f = {int(s): int(n) for s, n in freq.items() if n > 0}
    assert f and all(0 <= s < 256 for s in f)
    f[256] = 1
    size = {s: 0 for s in f}
    others = {s: -1 for s in f}
    while True:
        live = [s for s in f if f[s] > 0]
        if len(live) < 2:
            break
        v1 = min(live, key=lambda s: (f[s], -s))  # least frequency, the larger symbol on a tie
        v2 = min((s for s in live if s != v1), key=lambda s: (f[s], -s))
        f[v1] += f[v2]
        f[v2] = 0
        while True:
            size[v1] += 1
            if others[v1] < 0:
                break
            v1 = others[v1]
        others[v1] = v2
        while True:
            size[v2] += 1
            if others[v2] < 0:
                break
            v2 = others[v2]
    top = max(max(size.values()), 16)
    bits = [0] * (top + 1)
    for s in size:
        bits[size[s]] += 1
    for i in range(top, 16, -1):  # figure K.3: shorten the codes above 16 bits, pair by pair
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1  # the reserved symbol
    order = sorted((s for s in size if s != 256), key=lambda s: (size[s], s))  # figure K.4
    lengths, k = {}, 0
    for length in range(1, 17):
        for _ in range(bits[length]):
            lengths[order[k]] = length
            k += 1
    assert k == len(order)
    return lengths


def fibonacci_weights(freq: dict, alphabet) -> dict:
    """Weights that make the code a chain: Fibonacci numbers, the smallest for the most common symbol of ``freq``, larger
    ones for the rarer, the largest for symbols of ``alphabet`` the file does not use at all."""
    used = sorted((s for s in freq if freq[s] > 0), key=lambda s: (-freq[s], s))
    order = used + [s for s in alphabet if s not in set(used)]
    w, a, b = {}, 1, 2
    for s in order:
        w[s] = a
        a, b = b, a + b
    return w


def canonical(lengths: dict):
    """symbol -> length  =>  (the 16 counts, the symbols in code order, symbol -> (code, length)) (T.81 annex C)."""
    symbols = sorted(lengths, key=lambda s: (lengths[s], s))
    counts = [sum(1 for s in symbols if lengths[s] == n) for n in range(1, 17)]
    codes, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(counts[n - 1]):
            codes[symbols[k]] = (code, n)
            code += 1
            k += 1
        code <<= 1
    assert all(c != (1 << n) - 1 for c, n in codes.values()), "an all-ones code"
    return counts, symbols, codes


# ------------------------------------------------------------------------------------------------ symbols of the blocks
def _magnitude(v: int):
    n = abs(v).bit_length()
    return n, (v if v >= 0 else v + (1 << n) - 1)


def _block_symbols(zz, pred: int, out: list, dc_key, ac_key):
    """One block in zigzag order -> (table key, symbol, extra bits, number of extra bits) appended to ``out``."""
    n, bits = _magnitude(int(zz[0]) - pred)
    out.append((dc_key, n, bits, n))
    last = 0
    for k in np.flatnonzero(zz[1:]).tolist():
        k += 1
        run = k - last - 1
        while run > 15:
            out.append((ac_key, 0xF0, 0, 0))
            run -= 16
        n, bits = _magnitude(int(zz[k]))
        out.append((ac_key, (run << 4) | n, bits, n))
        last = k
    if last < 63:
        out.append((ac_key, 0x00, 0, 0))


def _pack(symbols, codes) -> bytes:
    """The symbols of one entropy-coded segment -> its bytes: padded with one bits, 0xFF stuffed."""
    parts = []
    for key, sym, extra, n in symbols:
        code, length = codes[key][sym]
        parts.append(format(code, f"0{length}b"))
        if n:
            parts.append(format(extra, f"0{n}b"))
    s = "".join(parts)
    s += "1" * (-len(s) % 8)
    return int(s, 2).to_bytes(len(s) // 8, "big").replace(b"\xff", b"\xff\x00") if s else b""


# ------------------------------------------------------------------------------------------------ the file
def relayout(parsed: dict, hs: int, vs: int) -> dict:
    """The same blocks declared under luma sampling hs x vs: every component's block grid cropped to the whole MCUs all of
    them can fill. A plain re-layout: the picture it gives is of no interest, the stream is a regular one."""
    assert parsed["ncomp"] == 3
    samp = [(hs, vs), (1, 1), (1, 1)]
    mx = min(c.shape[1] // h for c, (h, _) in zip(parsed["coef"], samp))
    my = min(c.shape[0] // v for c, (_, v) in zip(parsed["coef"], samp))
    assert mx >= 1 and my >= 1, "the source has too few blocks for this sampling"
    out = dict(parsed)
    out.update(hs=hs, vs=vs, mcus_x=mx, mcus_y=my, width=8 * hs * mx - 3, height=8 * vs * my - 1,
               coef=[np.ascontiguousarray(c[:my * v, :mx * h]) for c, (h, v) in zip(parsed["coef"], samp)],
               comp_bw=[mx * h for h, _ in samp], comp_bh=[my * v for _, v in samp])
    return out


def _segment(marker: int, payload: bytes, fill: int) -> bytes:
    return b"\xff" * fill + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def write(parsed: dict, **layout) -> bytes:
    return _build(parsed, **layout)[0]


def code_length_histogram(parsed: dict, **layout) -> np.ndarray:
    """How many coded symbols of ``write(parsed, **layout)`` take a code of each length 0..16 (for tests of the layouts)."""
    return _build(parsed, **layout)[1]


def _build(parsed: dict, restart: int = 0, huffman: str = "optimal", dc_slots=(0, 1, 1), ac_slots=(0, 1, 1), q_slots=(0, 1, 1),
          dqt_split: bool = False, dht_split: bool = False, pq: int = 0, sof: int = 0xC0, comp_ids=(1, 2, 3), fill: int = 0,
          jfif: bool = True, adobe=None, extra=(), scans: str = "interleaved"):
    ncomp, hs, vs = parsed["ncomp"], parsed["hs"], parsed["vs"]
    W, H, mx, my = parsed["width"], parsed["height"], parsed["mcus_x"], parsed["mcus_y"]
    assert 0 <= restart <= 65535 and huffman in ("optimal", "fibonacci") and scans in ("interleaved", "separate")
    assert pq in (0, 1) and sof in (0xC0, 0xC1) and len(set(comp_ids[:ncomp])) == ncomp
    samp = [(hs, vs)] + [(1, 1)] * (ncomp - 1)
    zz = [c.reshape(c.shape[0], c.shape[1], 64)[:, :, NATURAL] for c in parsed["coef"]]
    for c in range(ncomp):
        assert zz[c].shape[:2] == (my * samp[c][1], mx * samp[c][0]) and 0 <= min(dc_slots[c], ac_slots[c], q_slots[c]) and \
            max(dc_slots[c], ac_slots[c], q_slots[c]) <= 3

    # the entropy-coded segments as symbols: one list per restart interval (and per scan)
    def scan_segments(comps):
        segs, cur, pred, count = [], [], [0] * ncomp, 0
        if scans == "interleaved":  # MCU by MCU (a single component is sampled 1x1: its MCU is one block)
            units = [[(c, y * samp[c][1] + v, x * samp[c][0] + u) for c in comps for v in range(samp[c][1]) for u in range(samp[c][0])]
                     for y in range(my) for x in range(mx)]
        else:  # a scan of one component: its blocks in raster order, only those that hold samples (T.81 A.2.2)
            c = comps[0]
            bw, bh = -(-(-(-W * samp[c][0] // hs)) // 8), -(-(-(-H * samp[c][1] // vs)) // 8)
            units = [[(c, y, x)] for y in range(bh) for x in range(bw)]
        for unit in units:
            if restart and count and count % restart == 0:
                segs.append(cur)
                cur, pred = [], [0] * ncomp
            for c, by, bx in unit:
                _block_symbols(zz[c][by, bx], pred[c], cur, ("dc", dc_slots[c]), ("ac", ac_slots[c]))
                pred[c] = int(zz[c][by, bx, 0])
            count += 1
        segs.append(cur)
        return segs

    scan_list = [list(range(ncomp))] if scans == "interleaved" else [[c] for c in range(ncomp)]
    scan_syms = [scan_segments(comps) for comps in scan_list]

    # Huffman tables from the statistics of the components that share a slot
    freq = {}
    for segs in scan_syms:
        for seg in segs:
            for key, sym, _, _ in seg:
                freq.setdefault(key, {}).setdefault(sym, 0)
                freq[key][sym] += 1
    tables, codes = {}, {}
    for key in sorted(freq):
        f = freq[key] if huffman == "optimal" else fibonacci_weights(freq[key], DC_SYMBOLS if key[0] == "dc" else AC_SYMBOLS)
        counts, symbols, codes[key] = canonical(code_lengths(f))
        tables[key] = bytes([(key[0] == "ac") << 4 | key[1]]) + bytes(counts) + bytes(symbols)

    qt = {}
    for c in range(ncomp):
        t = np.asarray(parsed["qtables"][c], np.uint16)[NATURAL]
        assert q_slots[c] not in qt or np.array_equal(qt[q_slots[c]], t), "two tables for one slot"
        assert pq or int(t.max()) < 256
        qt[q_slots[c]] = t
    dqt = [bytes([pq << 4 | slot]) + (t.astype(">u2").tobytes() if pq else t.astype(np.uint8).tobytes()) for slot, t in sorted(qt.items())]
    dht = [tables[key] for key in sorted(tables)]

    out = [b"\xff\xd8"]
    if jfif:
        out.append(_segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00", fill))
    for kind in extra:
        if kind == "com":
            out.append(_segment(0xFE, b"written by tests/jpeg_write.py \xff\xd9\xff\xda", fill))
        elif kind == "app1":  # an Exif header and an empty little-endian TIFF directory
            out.append(_segment(0xE1, b"Exif\x00\x00II*\x00\x08\x00\x00\x00\x00\x00\x00\x00\x00\x00", fill))
        elif kind == "app2":
            out.append(_segment(0xE2, b"TEST_PROFILE\x00" + bytes(range(256)), fill))
        else:
            raise ValueError(kind)
    if adobe is not None:
        out.append(_segment(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([adobe]), fill))
    out += [_segment(0xDB, t, fill) for t in dqt] if dqt_split else [_segment(0xDB, b"".join(dqt), fill)]
    frame = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([ncomp])
    for c in range(ncomp):
        frame += bytes([comp_ids[c], samp[c][0] << 4 | samp[c][1], q_slots[c]])
    out.append(_segment(sof, frame, fill))
    out += [_segment(0xC4, t, fill) for t in dht] if dht_split else [_segment(0xC4, b"".join(dht), fill)]
    if restart:
        out.append(_segment(0xDD, restart.to_bytes(2, "big"), fill))
    for comps, segs in zip(scan_list, scan_syms):
        head = bytes([len(comps)])
        for c in comps:
            head += bytes([comp_ids[c], dc_slots[c] << 4 | ac_slots[c]])
        out.append(_segment(0xDA, head + b"\x00\x3f\x00", fill))
        for i, seg in enumerate(segs):
            if i:
                out.append(b"\xff" * fill + bytes([0xFF, 0xD0 + (i - 1) % 8]))
            out.append(_pack(seg, codes))
    out.append(b"\xff" * fill + b"\xff\xd9")
    hist = np.zeros(17, np.int64)
    for key in freq:
        for sym, n in freq[key].items():
            hist[codes[key][sym][1]] += n
    return b"".join(out), hist

