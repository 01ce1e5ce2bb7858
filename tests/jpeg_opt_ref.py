"""numpy / Python restatement of the JPEG writer's optimised Huffman tables (csrc/pp_jpeg_opt_core.h, csrc/pp_jpeg_entropy_opt.hip):
the symbol histogram of a scan, libjpeg's jpeg_gen_optimal_table and the coder that uses the tables it gives.

  * histogram: four tables of 257 bins - DC luma, AC luma, DC chroma, AC chroma; per block the DC category of the difference
    to the block before of its component (0 at the start and at every restart interval), (run << 4) | size per non-zero AC
    coefficient, 0xF0 per sixteen zeros in front of one, 0x00 unless zigzag position 63 is non-zero;
  * code lengths as jchuff.c builds them: freq[256] = 1 (the pseudo-symbol: no code of all ones); the two least frequent
    non-zero entries are merged, each search scanning upward with ``<=`` (a tie goes to the LARGER symbol), c2 the least entry
    other than c1; every member of both trees (the others[] chain) gets one bit longer; counts per length; annex K.3 from
    length 32 down to 17; one code off the longest length in use; huffval by length, then by symbol;
  * the file: the marker segments of csrc/pp_jpeg_enc_host.h with these four tables in the DHT segments, the scan coded with
    them, MSB first, padded with ones, FF stuffed, RSTn between restart intervals.

It is written the way libjpeg is (the chain walk, the two scans), not the way the product is (tree ids, one ordered key), so
that the two do not share a mistake. tests/test_jpeg_opt_references.py pins it to Pillow's ``optimize=True`` files: tables and
scan, byte for byte. ``faults`` switches single mistakes on, for the tests that show the pin rejects them."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA = range(4)
DHT_IDS = (0x00, 0x10, 0x01, 0x11)  # Tc << 4 | Th of the four tables, in the order the file holds them
FAULTS = ("tie_to_smaller", "no_pseudo_symbol", "no_k3", "vals_by_symbol")


# ------------------------------------------------------------------------------------------------------- the symbols
def scan_blocks(fwd: dict):
    """A ``jpeg_enc_ref.forward`` dict -> (zz (nblk, 64) int64 in zigzag order, comp (nblk,), mcu (nblk,)), blocks in scan order."""
    hs, vs, mx, my = fwd["hs"], fwd["vs"], fwd["mcus_x"], fwd["mcus_y"]
    mcus, lum = mx * my, hs * vs
    y, cb, cr = (np.asarray(c, np.int64) for c in fwd["coef"])
    assert y.shape == (my * vs, mx * hs, 64) and cb.shape == cr.shape == (my, mx, 64)
    row, col = np.divmod(np.arange(mcus), mx)
    j = np.arange(lum)
    yb = y[(row[:, None] * vs + j[None, :] // hs), (col[:, None] * hs + j[None, :] % hs)]  # (mcus, lum, 64)
    blocks = np.concatenate([yb, cb.reshape(mcus, 1, 64), cr.reshape(mcus, 1, 64)], axis=1).reshape(-1, 64)
    comp = np.tile(np.array([0] * lum + [1, 2]), mcus)
    return blocks[:, ZIGZAG], comp, np.repeat(np.arange(mcus), lum + 2)


def _size(v):
    """Magnitude category: bits of |v|."""
    return np.frexp(np.abs(v).astype(np.float64))[1].astype(np.int64)


def tokens(fwd: dict, restart_interval: int = 0) -> dict:
    """Every code of the scan, in order: ``table`` (0..3), ``symbol``, the appended bits ``extra`` / ``nextra`` and the ``mcu``
    it belongs to."""
    zz, comp, mcu = scan_blocks(fwd)
    nblk = zz.shape[0]
    diff = np.zeros(nblk, np.int64)
    for c in range(3):
        idx = np.flatnonzero(comp == c)
        dc = zz[idx, 0]
        prev = np.concatenate([[0], dc[:-1]])
        if restart_interval:
            first = np.concatenate([[True], mcu[idx][1:] != mcu[idx][:-1]])  # the component's first block of its MCU
            prev[first & (mcu[idx] % restart_interval == 0)] = 0
        diff[idx] = dc - prev
    chroma = (comp > 0).astype(np.int64)
    blk, k, sub, table, symbol, value = [], [], [], [], [], []

    def add(b, kk, s, t, sym, val):
        blk.append(b), k.append(kk), sub.append(np.full(b.shape, s)), table.append(t), symbol.append(sym), value.append(val)

    every = np.arange(nblk)
    add(every, np.zeros(nblk, np.int64), 0, 2 * chroma, _size(diff), diff)
    bb, kk = np.nonzero(zz[:, 1:])
    kk = kk + 1
    same = np.concatenate([[False], bb[1:] == bb[:-1]])
    prev = np.where(same, np.concatenate([[0], kk[:-1]]), 0)
    run = kk - prev - 1
    ac = zz[bb, kk]
    for n in range(3):  # up to three ZRLs in front of a coefficient
        m = (run >> 4) > n
        add(bb[m], kk[m], n, 2 * chroma[bb[m]] + 1, np.full(m.sum(), 0xF0), np.zeros(m.sum(), np.int64))
    add(bb, kk, 3, 2 * chroma[bb] + 1, ((run & 15) << 4) | _size(ac), ac)
    last = np.zeros(nblk, np.int64)
    last[bb] = kk  # (sorted by block, then position: the last assignment is the last non-zero position)
    eob = np.flatnonzero(last != 63)
    add(eob, np.full(eob.size, 64), 0, 2 * chroma[eob] + 1, np.zeros(eob.size, np.int64), np.zeros(eob.size, np.int64))
    blk, k, sub, table, symbol, value = (np.concatenate(a) for a in (blk, k, sub, table, symbol, value))
    order = np.lexsort((sub, k, blk))
    blk, table, symbol, value = blk[order], table[order], symbol[order], value[order]
    nextra = symbol & 15
    nextra[symbol == 0xF0] = 0
    dc_tok = (table & 1) == 0
    nextra[dc_tok] = symbol[dc_tok]
    extra = np.where(value < 0, value + (1 << nextra) - 1, value) & ((1 << nextra) - 1)
    return dict(table=table, symbol=symbol, extra=extra, nextra=nextra, mcu=mcu[blk])


def histogram(fwd: dict, restart_interval: int = 0) -> np.ndarray:
    """(4, 257) int64; bin 256 stays 0."""
    t = tokens(fwd, restart_interval)
    return np.stack([np.bincount(t["symbol"][t["table"] == i], minlength=257) for i in range(4)])


# ------------------------------------------------------------------------------------------------ the table builder
def code_sizes(freq, faults=()):
    """jpeg_gen_optimal_table up to the code sizes: [257] ints, before any limiting."""
    freq = [int(f) for f in freq[:256]] + [0 if "no_pseudo_symbol" in faults else 1]
    codesize, others = [0] * 257, [-1] * 257
    strict = "tie_to_smaller" in faults
    live = [i for i in range(257) if freq[i]]
    while True:
        c1, v = -1, None
        for i in live:  # (upward)
            if freq[i] and (v is None or (freq[i] < v if strict else freq[i] <= v)):
                v, c1 = freq[i], i
        c2, v = -1, None
        for i in live:
            if freq[i] and i != c1 and (v is None or (freq[i] < v if strict else freq[i] <= v)):
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        live.remove(c2)
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    return codesize


def optimal_table(freq, faults=()):
    """(bits, vals): codes per length 1..16 (1..32 where the ``no_k3`` fault leaves longer ones) and the symbols in code order."""
    codesize = code_sizes(freq, faults)
    if max(codesize) > 32:
        raise ValueError("code tree deeper than 32")
    bits = [0] * 33
    for s in codesize:
        if s:
            bits[s] += 1
    if "no_k3" not in faults:
        for i in range(32, 16, -1):
            while bits[i] > 0:
                j = i - 2
                while bits[j] == 0:
                    j -= 1
                bits[i] -= 2
                bits[i - 1] += 1
                bits[j + 1] += 2
                bits[j] -= 1
    if "no_pseudo_symbol" not in faults:
        i = 32 if "no_k3" in faults else 16
        while bits[i] == 0:
            i -= 1
        bits[i] -= 1
    if "vals_by_symbol" in faults:
        vals = [i for i in range(256) if codesize[i]]
    else:
        vals = [i for length in range(1, 33) for i in range(256) if codesize[i] == length]
    top = 32 if any(bits[17:]) else 16
    return np.array(bits[1:top + 1], np.uint8), np.array(vals, np.uint8)


def tables_of(fwd: dict, restart_interval: int = 0, faults=()) -> list:
    return [optimal_table(h, faults) for h in histogram(fwd, restart_interval)]


def same_tables(a, b) -> bool:
    return len(a) == len(b) and all(x[0].shape == y[0].shape and np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def derive(bits, vals):
    """(code[256], length[256]) int64 of a table; length 0: the symbol has no code."""
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, k = 0, 0
    for n in range(1, len(bits) + 1):
        for _ in range(int(bits[n - 1])):
            code[vals[k]], length[vals[k]] = c, n
            c, k = c + 1, k + 1
        c <<= 1
    return code, length


def kraft(bits) -> float:
    return float(sum(int(b) * 2.0 ** -(n + 1) for n, b in enumerate(bits)))


# ----------------------------------------------------------------------------------------------------------- the coder
def _pack(value, nbits) -> bytes:
    """MSB-first bits of (value, nbits) pairs, the last byte padded with ones, FF followed by 00."""
    total = int(nbits.sum())
    if total == 0:
        return b""
    start = np.cumsum(nbits) - nbits
    idx = np.repeat(np.arange(nbits.size), nbits)
    pos = np.arange(total) - np.repeat(start, nbits)
    bit = ((value[idx] >> (nbits[idx] - 1 - pos)) & 1).astype(np.uint8)
    bit = np.concatenate([bit, np.ones(-total % 8, np.uint8)])
    return np.packbits(bit).tobytes().replace(b"\xff", b"\xff\x00")


def scan_bytes(fwd: dict, tables, restart_interval: int = 0) -> bytes:
    """The entropy-coded segment (SOS header to EOI, both excluded) of ``fwd`` with the four ``tables`` [(bits, vals)]."""
    t = tokens(fwd, restart_interval)
    code, length = (np.stack(a) for a in zip(*[derive(b, v) for b, v in tables]))
    c, n = code[t["table"], t["symbol"]], length[t["table"], t["symbol"]]
    assert (n > 0).all(), "a symbol of the scan has no code"
    value, nbits = (c << t["nextra"]) | t["extra"], n + t["nextra"]
    if not restart_interval:
        return _pack(value, nbits)
    interval = t["mcu"] // restart_interval
    cuts = np.searchsorted(interval, np.arange(int(interval[-1]) + 2))
    out = []
    for i in range(len(cuts) - 1):
        if i:
            out.append(bytes([0xFF, 0xD0 + (i - 1) % 8]))
        out.append(_pack(value[cuts[i]:cuts[i + 1]], nbits[cuts[i]:cuts[i + 1]]))
    return b"".join(out)


def headers(fwd: dict, tables, restart_interval: int = 0) -> bytes:
    """SOI .. SOS as csrc/pp_jpeg_enc_host.h writes them, the four DHT segments immediately before DRI / SOS."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)

    qt = np.asarray(fwd["qtables"])
    out = [b"\xff\xd8", seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    ids = [0, 1, 1 if np.array_equal(qt[1], qt[2]) else 2]
    for i in range(ids[2] + 1):
        out.append(seg(0xDB, bytes([i]) + bytes(int(v) for v in qt[i][ZIGZAG])))
    out.append(seg(0xC0, bytes([8]) + fwd["height"].to_bytes(2, "big") + fwd["width"].to_bytes(2, "big") +
                   bytes([3, 1, (fwd["hs"] << 4) | fwd["vs"], ids[0], 2, 0x11, ids[1], 3, 0x11, ids[2]])))
    for tid, (bits, vals) in zip(DHT_IDS, tables):
        out.append(seg(0xC4, bytes([tid]) + bytes(bits.tolist()) + bytes(vals.tolist())))
    if restart_interval:
        out.append(seg(0xDD, restart_interval.to_bytes(2, "big")))
    out.append(seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


def encode(fwd: dict, restart_interval: int = 0, faults=()) -> bytes:
    """The whole optimised file of a ``jpeg_enc_ref.forward`` dict."""
    tables = tables_of(fwd, restart_interval, faults)
    return headers(fwd, tables, restart_interval) + scan_bytes(fwd, tables, restart_interval) + b"\xff\xd9"


# ------------------------------------------------------------------------------------------- reading a finished file
def split_file(data: bytes):
    """(tables [(bits, vals)] in the order DC luma, AC luma, DC chroma, AC chroma, the bytes between the SOS header and EOI)."""
    found, o = {}, 2
    while True:
        assert data[o] == 0xFF, "marker expected"
        marker, size = data[o + 1], int.from_bytes(data[o + 2:o + 4], "big")
        body = data[o + 4:o + 2 + size]
        o += 2 + size
        if marker == 0xC4:
            at = 0
            while at < len(body):  # (a segment may hold several tables)
                bits = np.frombuffer(body, np.uint8, 16, at + 1)
                n = int(bits.sum())
                found[body[at]] = (bits.copy(), np.frombuffer(body, np.uint8, n, at + 17).copy())
                at += 17 + n
        if marker == 0xDA:
            break
    assert data.endswith(b"\xff\xd9")
    return [found[i] for i in DHT_IDS], data[o:-2]


def pillow_optimized(rgb: np.ndarray, quality: int, subsampling: str) -> bytes:
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, "JPEG", quality=quality, subsampling={"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}[subsampling],
                                                    optimize=True)
    return buf.getvalue()


# -------------------------------------------------------------------------------------------------- crafted histograms
AC_SYMBOLS = [(r << 4) | s for r in range(16) for s in range(1, 11)]  # run 0 first


def fibonacci_histogram(n: int = 24) -> np.ndarray:
    """257 bins with n AC symbols whose counts follow the Fibonacci numbers 1, 2, 3, 5 ... (beside the pseudo-symbol's 1), the
    largest count on the first of AC_SYMBOLS: in an unlimited Huffman tree the rarest symbol sits n levels deep."""
    fib = [1, 2]
    while len(fib) < n:
        fib.append(fib[-1] + fib[-2])
    f = np.zeros(257, np.int64)
    f[AC_SYMBOLS[:n]] = fib[n - 1::-1]
    return f


def geometry_for_blocks(bw: int, bh: int) -> dict:
    """The 4:4:4 plan of a bw x bh block image as a ``jpeg_enc_ref.forward``-shaped dict with zero coefficients, quality 100."""
    return dict(width=8 * bw, height=8 * bh, ncomp=3, hs=1, vs=1, mcus_x=bw, mcus_y=bh, comp_bw=[bw] * 3, comp_bh=[bh] * 3,
                coef_count=192 * bw * bh, restart_interval=0, coef=[np.zeros((bh, bw, 64), np.int16) for _ in range(3)],
                qtables=np.ones((3, 64), np.uint16))


def coefficients_for_luma_symbols(freq, bw: int, bh: int, seed: int = 0, per_block: int = 62) -> dict:
    """A 4:4:4 ``forward``-shaped dict whose luma AC codes are ``freq``'s (run, size) symbols, each as often as ``freq`` says, in
    a seeded random order: a symbol becomes one coefficient of its size behind ``run`` zeros, a block takes symbols while
    they fit in front of zigzag 63, which stays zero, at most ``per_block`` of them. (So EOB joins them once per luma block,
    bw * bh times; ZRL never.)"""
    fwd = geometry_for_blocks(bw, bh)
    y = fwd["coef"][0].reshape(-1, 64)
    todo = np.repeat(np.arange(256), np.asarray(freq[:256], np.int64))
    assert not ((todo & 15) == 0).any(), "(run, size) symbols only"
    np.random.default_rng(seed).shuffle(todo)
    b, k, held = 0, 0, 0  # the block being filled, the last zigzag position it uses, its symbols
    for n, sym in enumerate(todo.tolist()):
        run, size = sym >> 4, sym & 15
        if k + run + 1 > 62 or held == per_block:
            b, k, held = b + 1, 0, 0
        k, held = k + run + 1, held + 1
        y[b, ZIGZAG[k]] = (1 << size) - 1 if n & 1 else -(1 << (size - 1))
    assert b < y.shape[0], "the symbols need more blocks"
    return fwd


LIMITED_COUNTS = (4461, 2752, 1709, 1043, 666, 377, 144, 89, 55, 34, 21, 13, 8, 5, 3, 2, 1)


def length_limited_coefficients() -> dict:
    """Coefficients of a 17 x 17 block 4:4:4 plan whose luma AC table needs the 16-bit limit. With the pseudo-symbol's 1 and EOB's
    289 (once per luma block) the counts are 1, 1, 2, 3, 5 ... 144, 289, 377, 666, 1043 ...: the sum of all counts below one
    stays below the next but one, so the unlimited tree is a chain with one level per symbol - 18 deep."""
    f = np.zeros(257, np.int64)
    f[AC_SYMBOLS[:len(LIMITED_COUNTS)]] = LIMITED_COUNTS
    return coefficients_for_luma_symbols(f, 17, 17)


# A picture Pillow itself codes with a length-limited table: grey pixels (flat chroma) whose luma coefficients at quality 50 are
# small values (sizes 1 and 2) behind runs of 0..14 zeros, at most six per block of a 48 x 48 block image, with the counts
# below. With the pseudo-symbol's 1 and EOB's 2304 they are 1, 1, 2, 3, 5 ... 987, 2304, 2584, 4888: a chain, 18 deep.
PILLOW_LIMITED_SYMBOLS = [0x01, 0x02, 0x11, 0x12] + [(r << 4) | 1 for r in range(2, 15)]
PILLOW_LIMITED_COUNTS = (4888, 2584, 987, 610, 377, 233, 144, 89, 55, 34, 21, 13, 8, 5, 3, 2, 1)
PILLOW_LIMITED_QUALITY = 50


def pillow_limited_image() -> np.ndarray:
    """(384, 384, 3) uint8 RGB: the inverse DCT of those coefficients times quality 50's luma table, rounded. The steps of the
    table (10 and more) are far above the rounding's share in any coefficient, so the compressor finds the coefficients again."""
    import jpeg_enc_ref as E

    f = np.zeros(257, np.int64)
    f[PILLOW_LIMITED_SYMBOLS] = PILLOW_LIMITED_COUNTS
    fwd = coefficients_for_luma_symbols(f, 48, 48, per_block=6)
    q = E.quality_tables(PILLOW_LIMITED_QUALITY)[0].astype(np.float64)
    F = (fwd["coef"][0].astype(np.float64) * q).reshape(48, 48, 8, 8)
    u, x = np.mgrid[0:8, 0:8]
    C = np.where(u == 0, np.sqrt(0.5), 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16)  # C[u, x]
    px = np.einsum("ux,abuv,vy->axby", C, F, C).reshape(384, 384) + 128.0
    assert px.min() >= 0.0 and px.max() <= 255.0, "the picture would be clipped"
    grey = np.rint(px).astype(np.uint8)
    rgb = np.repeat(grey[:, :, None], 3, axis=2)
    rgb.setflags(write=False)
    return rgb


# ------------------------------------------------------------------------------------------------- the committed fixture
FIXTURE_CASES = ("noise|8|8|4:4:4|75", "gradient|17|13|4:2:0|24", "checker|17|13|4:2:2|95", "noise|64|96|4:2:0|75", "gradient|64|96|4:4:4|100",
                 "flat0|64|96|4:2:2|1", "noise|250|187|4:2:0|24", "limited|384|384|4:4:4|50")


def case_image(content: str, W: int, H: int) -> np.ndarray:
    import jpeg_enc_ref as E

    if content == "limited":
        assert (W, H) == (384, 384)
        return pillow_limited_image()
    return E.image(content, W, H)


def write_fixture(path: str) -> None:
    """tests/golden/jpeg_opt_cases.npz: the four tables and the scan of Pillow's ``optimize=True`` file of every FIXTURE_CASES
    entry (python tests/jpeg_opt_ref.py, with a Pillow on libjpeg-turbo)."""
    out = dict(cases=np.array(FIXTURE_CASES))
    for i, case in enumerate(FIXTURE_CASES):
        content, W, H, ss, q = case.split("|")
        tables, scan = split_file(pillow_optimized(case_image(content, int(W), int(H)), int(q), ss))
        out[f"bits_{i}"] = np.stack([b for b, _ in tables])
        out[f"vals_{i}"] = np.stack([np.pad(v, (0, 256 - v.size)) for _, v in tables])
        out[f"scan_{i}"] = np.frombuffer(scan, np.uint8)
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    import os

    write_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_opt_cases.npz"))
