"""Sequential restatement of the device Huffman decoder (csrc/pp_jpeg_huffdec.hip, csrc/pp_jpeg_huffdec_core.h): the same
subsequences of S raw bytes, the same decoder state (raw bit position, block inside the MCU, zigzag index), the same rule for
a bit pattern that is no code (one bit consumed, the rest of the state kept), the same passes - launch 0 decodes every
subsequence speculatively, then a workgroup of WG subsequences iterates at most INNER times per launch, thread 0 taking the
border state the launch before left - the same verification, block count, scan, write and DC prefix sums, the same verdict.

A position counts raw bits, stuffed bytes included, and never points into a stuffed 00. Here the stream is unstuffed once
and positions are converted at the edges of a decode, which gives the same numbers.

``fault`` restates the decoder with one mistake, for the tests that show the comparison catches it:
  "accept_first"   the speculative pass is accepted unverified;
  "no_mcu_pos"     the position inside the MCU is not carried from one subsequence to the next;
  "ff00_boundary"  a stuffed 00 that begins a subsequence is read as data.
"""
import numpy as np

import jpeg_ref as J

S, WG, INNER = 128, 256, 32
DEFAULT_PASSES, MAX_PASSES = 3, 64
OK, NOT_SYNCHRONISED, ENDS_EARLY, BAD_CODE, DC_RANGE, TRAILING = 0, 1, 2, 3, 4, 5
FAULTS = ("accept_first", "no_mcu_pos", "ff00_boundary")


def covered_bytes(passes: int) -> int:
    """The synchronisation distance ``passes`` launches cover at least: thread 0 of a workgroup gains one subsequence per launch
    on the border state, every other thread INNER."""
    return S * (INNER * (passes - 1) + 2)


def prepare(data: bytes) -> dict:
    """What pp_jpeg_scan_prepare reads: geometry, each component's (DC, AC) code tables as {bit string: symbol}, the bounds of
    the entropy-coded segment (behind SOS, up to the first FF that no 00 follows). ValueError outside the subset."""
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    pos, dc, ac, frame, ri = 2, {}, {}, None, 0
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
            frame = dict(height=(s[1] << 8) | s[2], width=(s[3] << 8) | s[4], comps=[(s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15) for c in range(s[5])])
        elif m == 0xC4:
            o = 0
            while o < len(s):
                counts = list(s[o + 1:o + 17])
                total = sum(counts)
                (ac if s[o] >> 4 else dc)[s[o] & 15] = J._huff_table(counts, list(s[o + 17:o + 17 + total]))
                o += 17 + total
        elif m == 0xDD:
            ri = (s[0] << 8) | s[1]
        elif m == 0xDA:
            break
    if ri:
        raise ValueError("restart interval")
    ncomp = len(frame["comps"])
    hs, vs = frame["comps"][0] if ncomp == 3 else (1, 1)
    end = pos
    while True:
        end = data.index(b"\xff", end)
        if end + 1 < len(data) and data[end + 1] == 0:
            end += 2
        else:
            break
    tables = []
    for c in range(ncomp):
        tables += [dc[s[2 + 2 * c] >> 4], ac[s[2 + 2 * c] & 15]]
    mx, my = -(-frame["width"] // (8 * hs)), -(-frame["height"] // (8 * vs))
    return dict(ncomp=ncomp, hs=hs, vs=vs, mcus_x=mx, mcus_y=my, tables=tables, offset=pos, stream=data[pos:end])


class _Stream:
    def __init__(self, raw: bytes, fault=None):
        a = np.frombuffer(raw, np.uint8)
        n = self.n = len(a)
        stuffed = np.zeros(n, bool)
        if n > 1:
            stuffed[1:] = (a[1:] == 0) & (a[:-1] == 0xFF)
        self.true_stuffed = stuffed.copy()
        if fault == "ff00_boundary":
            stuffed[::S] = False
        self.stuffed = stuffed
        self.raw_of_data = np.flatnonzero(~stuffed)
        self.nd = len(self.raw_of_data)
        self.data_of_raw = np.concatenate([[0], np.cumsum(~stuffed)])  # data bytes in front of raw byte r (r <= n)
        d = a[~stuffed].tobytes()
        self.bits = bin(int.from_bytes(d, "big"))[2:].zfill(8 * len(d)) if d else ""

    def to_data(self, pos: int) -> int:
        r = pos >> 3
        return 8 * (int(self.data_of_raw[r]) if r <= self.n else self.nd + r - self.n) + (pos & 7)

    def to_raw(self, q: int) -> int:
        j = q >> 3
        return 8 * (int(self.raw_of_data[j]) if j < self.nd else self.n + j - self.nd) + (q & 7)

    def data_byte_limit(self, end_byte: int) -> int:
        return 8 * (int(self.data_of_raw[end_byte]) if end_byte <= self.n else self.nd + end_byte - self.n)

    def peek(self, q: int, k: int) -> str:
        return self.bits[q:q + k].ljust(k, "0")  # zeros past the stream


class _Geometry:
    def __init__(self, p):
        self.hs, self.vs, self.mcus_x, self.mcus_y, self.ncomp = p["hs"], p["vs"], p["mcus_x"], p["mcus_y"], p["ncomp"]
        self.lum = self.hs * self.vs
        self.bpm = 1 if self.ncomp == 1 else self.lum + 2
        self.mcus = self.mcus_x * self.mcus_y
        self.nblk = self.mcus * self.bpm

    def block_index(self, g: int) -> int:
        mcu, j = divmod(g, self.bpm)
        if j < self.lum:
            my, mx = divmod(mcu, self.mcus_x)
            return (my * self.vs + j // self.hs) * self.mcus_x * self.hs + mx * self.hs + j % self.hs
        return self.mcus * self.lum + (j - self.lum) * self.mcus + mcu

    def component_block(self, c: int, k: int) -> int:
        if c > 0:
            return self.mcus * self.lum + (c - 1) * self.mcus + k
        mcu, j = divmod(k, self.lum)
        my, mx = divmod(mcu, self.mcus_x)
        return (my * self.vs + j // self.hs) * self.mcus_x * self.hs + mx * self.hs + j % self.hs


class _Count:
    def __init__(self):
        self.blocks = 0

    def coef(self, k, v):
        pass

    def block_done(self):
        self.blocks += 1

    def stop(self):
        return False


class _Write:
    def __init__(self, G, coef, first):
        self.G, self.out, self.g, self.finished = G, coef, first, False

    def coef(self, k, v):
        if self.g < self.G.nblk:
            self.out[self.G.block_index(self.g) * 64 + J.NATURAL[k]] = v

    def block_done(self):
        self.g += 1
        if self.g >= self.G.nblk:
            self.finished = True

    def stop(self):
        return self.g >= self.G.nblk


def run(st: _Stream, tables, state, end_byte, G, sink, log=None):
    """One subsequence from ``state`` = (pos, blk, k) to the first symbol boundary at or behind raw byte ``end_byte``.
    Returns (exit state, bad). ``log``: a list that receives (data bit, code length, extra bits, symbol, k before) per symbol."""
    pos, blk, k = state
    q, limit, bad = st.to_data(pos), st.data_byte_limit(end_byte), False
    for _ in range(8 * S + 64):
        if q >= limit or sink.stop():
            break
        comp = 0 if blk < G.lum else 1 + blk - G.lum
        table = tables[2 * comp + (1 if k > 0 else 0)]
        word, sym = st.peek(q, 16), None
        for length in range(1, 17):
            sym = table.get(word[:length])
            if sym is not None:
                break
        if sym is None:
            q += 1
            bad = True
            continue
        q0, k0 = q, k
        q += length
        end = False
        if k == 0:
            s = sym
            if s > 11:
                bad, s = True, 0
            sink.coef(0, _extend(st, q, s) if s else 0)
            q += s
            k = 1
        else:
            r, s = sym >> 4, sym & 15
            if s == 0:
                if r == 15:
                    k += 16
                    if k > 63:
                        bad = end = True
                else:
                    end = True
            else:
                k += r
                if k > 63:
                    bad = end = True
                else:
                    if s > 10:
                        bad = True
                    sink.coef(k, _extend(st, q, s))
                    q += s
                    k += 1
                    end = k == 64
        if log is not None:
            log.append((q0, length, q - q0 - length, sym, k0))
        if end:
            sink.block_done()
            blk = 0 if blk + 1 == G.bpm else blk + 1
            k = 0
    return (st.to_raw(q), blk, k), bad


def _extend(st, q, s):
    v = int(st.peek(q, s), 2)
    return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def _end_of(i, n):
    return min((i + 1) * S, n)


def decode(p: dict, sync_passes: int = DEFAULT_PASSES, fault=None) -> dict:
    """The launches of pp_jpeg_huffman_decode_batch for one prepared file. Returns dict(status: 0 or the reason, passes, blocks,
    coef: the flat int16 coefficients in pp_jpeg_entropy_decode's layout, nsub, nwg)."""
    assert fault is None or fault in FAULTS
    st, G, T = _Stream(p["stream"], fault), _Geometry(p), p["tables"]
    n = st.n
    nsub = max(1, -(-n // S))
    nwg = -(-nsub // WG)

    def canonical(pos):
        r = pos >> 3
        return (r + 1) << 3 if r < n and st.stuffed[r] else pos

    def go(i, state):
        c = _Count()
        if fault == "no_mcu_pos":
            state = (state[0], 0, state[2])
        ex, _ = run(st, T, state, _end_of(i, n), G, c)
        return ex, c.blocks

    entry, exit_, cnt = [None] * nsub, [None] * nsub, [0] * nsub
    bexit = [[None] * nwg, [None] * nwg]
    passes_used = 0
    for launch in range(1 if fault == "accept_first" else sync_passes):
        for wg in range(nwg):
            ids = range(wg * WG, min(nsub, (wg + 1) * WG))
            if launch == 0:
                for i in ids:
                    entry[i] = (canonical(8 * S * i), 0, 0)
                    exit_[i], cnt[i] = go(i, entry[i])
            left = entry[ids[0]]
            if wg == 0:
                left = (0, 0, 0)
            elif launch > 0:
                left = bexit[(launch - 1) & 1][wg - 1]
            if fault == "accept_first":
                continue
            ex = [exit_[i] for i in ids]
            for _ in range(INNER):
                new, any_ = list(ex), False
                for t, i in enumerate(ids):
                    want = left if t == 0 else ex[t - 1]
                    if want != entry[i]:
                        entry[i] = want
                        exit_[i], cnt[i] = go(i, want)
                        any_ = True
                        if launch > 0:
                            passes_used = max(passes_used, launch)
                    new[t] = exit_[i]
                ex = new
                if not any_:
                    break
            bexit[launch & 1][wg] = exit_[ids[-1]]
    synced = fault == "accept_first" or all(entry[i] == ((0, 0, 0) if i == 0 else exit_[i - 1]) for i in range(nsub))
    first, total = [], 0
    for i in range(nsub):
        first.append(total)
        total += cnt[i]
    coef = np.zeros(G.nblk * 64, np.int64)
    out = dict(passes=passes_used + 1, blocks=total, nsub=nsub, nwg=nwg, coef=None)
    if not synced:
        return dict(out, status=NOT_SYNCHRONISED)
    bad, endpos = False, None
    for i in range(nsub):
        if first[i] >= G.nblk:
            continue
        sink = _Write(G, coef, first[i])
        state = entry[i] if fault != "no_mcu_pos" else (entry[i][0], 0, entry[i][2])
        ex, b = run(st, T, state, _end_of(i, n), G, sink)
        bad |= b
        if sink.finished:
            endpos = ex[0]
    range_bad = False
    for c in range(G.ncomp):
        s = 0
        for k in range(G.mcus * G.lum if c == 0 else G.mcus):
            at = G.component_block(c, k) * 64
            s += int(coef[at])
            range_bad |= not -32768 <= s <= 32767
            coef[at] = s
    out["coef"] = coef.astype(np.int16)
    bits = 8 * n
    data_bits = bits - (8 if n > 1 and st.true_stuffed[n - 1] else 0)
    if total < G.nblk or endpos is None or endpos > bits:
        status = ENDS_EARLY
    elif bad:
        status = BAD_CODE
    elif range_bad:
        status = DC_RANGE
    elif data_bits - endpos >= 8:
        status = TRAILING
    else:
        status = OK
    return dict(out, status=status)


def passes_needed(p: dict) -> int:
    """The smallest sync_passes at which the restatement accepts the file (MAX_PASSES + 1: none does)."""
    for passes in range(1, MAX_PASSES + 1):
        r = decode(p, passes)
        if r["status"] != NOT_SYNCHRONISED:
            return passes
        if r["passes"] < passes:  # nothing changed in the last launch and it is still not synchronised: cannot happen
            raise AssertionError("a fixed point that is no chain")
    return MAX_PASSES + 1


def situations(p: dict) -> set:
    """The boundary situations the true decoder meets in a prepared file, by name (what tests/test_jpeg_huffdec_gpu.py asserts
    its inputs hold)."""
    st, G = _Stream(p["stream"]), _Geometry(p)
    raw = p["stream"]
    n = len(raw)
    found = set()
    for name, size in (("len_S", S), ("len_S-1", S - 1), ("len_S+1", S + 1), ("len_2S", 2 * S)):
        if n == size:
            found.add(name)
    for b in range(S, n, S):
        if raw[b - 1] == 0xFF and raw[b] == 0:
            found.add("ff00_split")
    log = []
    run_all = _Count()
    state, q_end = (0, 0, 0), None
    # the true chain in one piece: run() is bounded per call, so it is called subsequence by subsequence
    for i in range(max(1, -(-n // S))):
        state, _ = run(st, p["tables"], state, _end_of(i, n), G, run_all, log)
    longest = [max(len(c) for c in t) for t in p["tables"]]
    tabs_of = {}
    edges = [st.data_byte_limit(b) for b in range(S, n, S)]
    edge_set = np.array(edges, np.int64)
    blk, prev_k = 0, 0
    for q0, length, extra, sym, k0 in log:
        comp = 0 if blk < G.lum else 1 + blk - G.lum
        t = 2 * comp + (1 if k0 > 0 else 0)
        if length == longest[t]:
            tabs_of[t] = True
        if len(edge_set):
            if ((edge_set > q0) & (edge_set < q0 + length)).any():
                found.add("code_straddles")
            if extra and ((edge_set > q0 + length) & (edge_set < q0 + length + extra)).any():
                found.add("extra_bits_straddle")
        end = False
        if k0 == 0:
            pass
        else:
            r, s = sym >> 4, sym & 15
            if s == 0:
                if r == 15:
                    found.add("zrl")
                    end = k0 + 16 > 63
                else:
                    end = True
            else:
                end = k0 + r > 63 or k0 + r + 1 == 64
                if k0 + r == 63:
                    found.add("ends_at_63")
        if end:
            blk = 0 if blk + 1 == G.bpm else blk + 1
    if tabs_of:
        found.add("longest_codes")
    return found
