"""numpy restatement of the baseline JPEG decoder the split GPU decoder reproduces (csrc/pp_jpeg_host.h + csrc/pp_jpeg.hip):
a file -> quantised coefficients and quantisation tables -> pixels, by libjpeg's integer rules with the IDCT in int64:

  * IDCT: jidctint "islow" (CONST_BITS 13, PASS1_BITS 2): dequantise, columns (descale by 11, round half up), rows (descale
    by 18), + 128, clamp to [0, 255];
  * component planes cropped to ceil(W h_c / h_max) x ceil(H v_c / v_max); the neighbour of an edge sample is that sample;
  * fancy upsampling (h2v1: 3:1 weights, rounding 1 / 2; h2v2: 9:3:3:1 weights, rounding 8 / 7) of chroma planes more than
    two samples wide, plain replication of narrower ones (libjpeg's jdsample picks its interpolating routines only for
    downsampled_width > 2);
  * YCbCr -> RGB with 16-bit fixed-point constants.

It is the arbiter of the kernels' arithmetic: tests/test_jpeg_references.py pins it to Pillow's bundled libjpeg-turbo, bit
for bit. It parses only what the tests need (one interleaved Huffman scan; fill bytes in front of any marker) and raises ValueError on anything else."""
import numpy as np

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                    21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                    61, 54, 47, 55, 62, 63])


def _huff_table(counts, symbols):
    """The canonical code of a DHT table: the bit string of every code -> its symbol."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[format(code, f"0{length}b")] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return table


class _Bits:
    """One entropy-coded segment as a string of '0' / '1' (slicing a string is what Python does fastest here)."""

    def __init__(self, segment: bytes):
        raw = segment.replace(b"\xff\x00", b"\xff")
        self.bits = bin(int.from_bytes(raw, "big"))[2:].zfill(8 * len(raw)) if raw else ""
        self.p = 0

    def symbol(self, table):
        bits, p = self.bits, self.p
        for length in range(1, 17):  # (past the end the slice stays as short as one already tried: no false match)
            s = table.get(bits[p:p + length])
            if s is not None:
                self.p = p + length
                return s
        if p + 16 > len(bits):
            raise IndexError("data ends early")
        raise ValueError("bad Huffman code")

    def extend(self, s):
        chunk = self.bits[self.p:self.p + s]
        if len(chunk) < s:
            raise IndexError("data ends early")
        self.p += s
        v = int(chunk, 2)
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def parse(data: bytes) -> dict:
    """File -> dict(width, height, ncomp, hs, vs, mcus_x, mcus_y, comp_bw, comp_bh, restart_interval, coef: per component
    (block_rows, block_cols, 64) int16 in natural order, padded to whole MCUs, qtables: (ncomp, 64) uint16 natural order)."""
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    pos, q, dc, ac, frame, ri = 2, {}, {}, {}, None, 0
    while True:
        if data[pos] != 0xFF:
            raise ValueError("marker expected")
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        n = (data[pos] << 8) | data[pos + 1]
        s = data[pos + 2:pos + n]
        pos += n
        if m in (0xC0, 0xC1):
            if s[0] != 8:
                raise ValueError("precision")
            frame = dict(height=(s[1] << 8) | s[2], width=(s[3] << 8) | s[4],
                         comps=[(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(s[5])])
        elif m == 0xC4:
            o = 0
            while o < len(s):
                counts = list(s[o + 1:o + 17])
                total = sum(counts)
                (ac if s[o] >> 4 else dc)[s[o] & 15] = _huff_table(counts, list(s[o + 17:o + 17 + total]))
                o += 17 + total
        elif m == 0xDB:
            o = 0
            while o < len(s):
                t = np.zeros(64, np.uint16)
                if s[o] >> 4:
                    t[NATURAL] = np.frombuffer(s[o + 1:o + 129], ">u2")
                    step = 129
                else:
                    t[NATURAL] = np.frombuffer(s[o + 1:o + 65], np.uint8)
                    step = 65
                q[s[o] & 15] = t
                o += step
        elif m == 0xDD:
            ri = (s[0] << 8) | s[1]
        elif m == 0xDA:
            break
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        else:
            raise ValueError(f"marker {m:#x}")
    comps = frame["comps"]
    ncomp = len(comps)
    if s[0] != ncomp or ncomp not in (1, 3):
        raise ValueError("one interleaved scan of 1 or 3 components")
    tables = [(dc[s[2 + 2 * c] >> 4], ac[s[2 + 2 * c] & 15]) for c in range(ncomp)]
    W, H = frame["width"], frame["height"]
    hs, vs = (comps[0][1], comps[0][2]) if ncomp == 3 else (1, 1)
    samp = [(hs, vs)] + [(1, 1)] * (ncomp - 1)
    if ncomp == 3 and (comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1) or (hs, vs) not in ((1, 1), (2, 1), (2, 2))):
        raise ValueError("sampling")
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    coef = [np.zeros((my * v, mx * h, 64), np.int16) for h, v in samp]
    # entropy-coded segments: split at the RSTn markers, end at EOI
    segs, start, p = [], pos, pos
    while True:
        p = data.index(b"\xff", p)
        m = p + 1
        while data[m] == 0xFF:  # fill bytes in front of a marker
            m += 1
        nxt = data[m]
        if nxt == 0x00 and m == p + 1:
            p += 2
        elif 0xD0 <= nxt <= 0xD7:
            if nxt != 0xD0 + len(segs) % 8:
                raise ValueError("wrong restart marker")
            segs.append(data[start:p])
            start = p = m + 1
        elif nxt == 0xD9:
            segs.append(data[start:p])
            break
        else:
            raise ValueError("marker inside the scan")
    per = ri if ri else mx * my
    if len(segs) != -(-mx * my // per):
        raise ValueError("restart segments")
    mcu = 0
    for seg in segs:
        br, pred = _Bits(seg), [0] * ncomp
        for _ in range(min(per, mx * my - mcu)):
            y0, x0 = divmod(mcu, mx)
            for c, (h, v) in enumerate(samp):
                for bv in range(v):
                    for bh in range(h):
                        blk = coef[c][y0 * v + bv, x0 * h + bh]
                        sz = br.symbol(tables[c][0])
                        if sz:
                            pred[c] += br.extend(sz)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = br.symbol(tables[c][1])
                            r, sz = rs >> 4, rs & 15
                            if sz == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            blk[NATURAL[k]] = br.extend(sz)
                            k += 1
            mcu += 1
    return dict(width=W, height=H, ncomp=ncomp, hs=hs, vs=vs, mcus_x=mx, mcus_y=my, comp_bw=[mx * h for h, _ in samp],
                comp_bh=[my * v for _, v in samp], restart_interval=ri, coef=coef,
                qtables=np.stack([q[comps[c][3]] for c in range(ncomp)]))


def flat_coefficients(parsed: dict) -> np.ndarray:
    """The coefficient buffer of pp_jpeg_entropy_decode: every component's blocks, one after the other."""
    return np.concatenate([c.reshape(-1) for c in parsed["coef"]])


def _pass(x, shift):
    """One 8-point pass of the islow IDCT over the last axis-free list x[0..7] of int64 arrays."""
    z1 = (x[2] + x[6]) * 4433
    tmp2 = z1 + x[6] * -15137
    tmp3 = z1 + x[2] * 6270
    tmp0 = (x[0] + x[4]) * 8192
    tmp1 = (x[0] - x[4]) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return [(o + (1 << (shift - 1))) >> shift for o in out]


def idct_plane(coef: np.ndarray, qtable: np.ndarray) -> np.ndarray:
    """(block_rows, block_cols, 64) int16 + (64,) uint16 -> the (block_rows * 8, block_cols * 8) uint8 plane."""
    bh, bw, _ = coef.shape
    d = coef.astype(np.int64).reshape(bh, bw, 8, 8) * qtable.astype(np.int64).reshape(8, 8)
    ws = np.stack(_pass([d[:, :, k, :] for k in range(8)], 11), axis=2)  # columns: ws[:, :, k, c]
    px = np.stack(_pass([ws[:, :, :, k] for k in range(8)], 18), axis=3)  # rows: px[:, :, r, k]
    px = np.clip(px + 128, 0, 255).astype(np.uint8)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h_pair(t, r_even, r_odd, shift):
    left = np.concatenate([t[:, :1], t[:, :-1]], axis=1)
    right = np.concatenate([t[:, 1:], t[:, -1:]], axis=1)
    out = np.empty((t.shape[0], 2 * t.shape[1]), np.int64)
    out[:, 0::2] = (3 * t + left + r_even) >> shift
    out[:, 1::2] = (3 * t + right + r_odd) >> shift
    return out


def upsample(p: np.ndarray, hs: int, vs: int, W: int, H: int) -> np.ndarray:
    """A chroma plane (already cropped to its real samples) -> (H, W) int64."""
    p = p.astype(np.int64)
    if (hs, vs) == (1, 1):
        return p[:H, :W]
    if p.shape[1] <= 2:  # libjpeg interpolates only planes more than two samples wide: plain replication otherwise
        return np.repeat(np.repeat(p, hs, axis=1), vs, axis=0)[:H, :W]
    if (hs, vs) == (2, 1):
        return _h_pair(p, 1, 2, 2)[:H, :W]
    above = np.concatenate([p[:1], p[:-1]], axis=0)
    below = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int64)
    out[0::2] = _h_pair(3 * p + above, 8, 7, 4)
    out[1::2] = _h_pair(3 * p + below, 8, 7, 4)
    return out[:H, :W]


def reconstruct_rgb(parsed: dict) -> np.ndarray:
    """Coefficients and tables -> (H, W, 3) uint8 RGB."""
    W, H, hs, vs = parsed["width"], parsed["height"], parsed["hs"], parsed["vs"]
    planes = [idct_plane(c, parsed["qtables"][i]) for i, c in enumerate(parsed["coef"])]
    Y = planes[0][:H, :W].astype(np.int64)
    if parsed["ncomp"] == 1:
        return np.repeat(Y[:, :, None], 3, axis=2).astype(np.uint8)
    cw, ch = -(-W // hs), -(-H // vs)
    cb = upsample(planes[1][:ch, :cw], hs, vs, W, H) - 128
    cr = upsample(planes[2][:ch, :cw], hs, vs, W, H) - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], axis=2), 0, 255).astype(np.uint8)


def decode_rgb(data: bytes) -> np.ndarray:
    return reconstruct_rgb(parse(data))


# ------------------------------------------------------------------------------------------------ the committed test grid
_GOLDEN = None


def golden():
    """tests/golden/jpeg_cases.npz (make_golden_jpeg.py), loaded once: dict(names, jpg: name -> bytes, rgb: name -> Pillow's
    (H, W, 3) uint8 RGB, refused: name -> bytes of files outside the subset)."""
    global _GOLDEN
    if _GOLDEN is None:
        import os

        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz"))
        names = [str(n) for n in z["names"]]
        _GOLDEN = dict(names=names, jpg={n: z["jpg_" + n].tobytes() for n in names}, rgb={n: z["rgb_" + n] for n in names},
                       refused={str(n): z["refused_" + str(n)].tobytes() for n in z["refused_names"]})
    return _GOLDEN


_PARSED = {}


def golden_parsed(name: str) -> dict:
    """parse() of a grid file, computed once and shared by the tests (do not modify)."""
    if name not in _PARSED:
        _PARSED[name] = parse(golden()["jpg"][name])
    return _PARSED[name]
