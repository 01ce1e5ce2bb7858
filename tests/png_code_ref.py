"""The histograms that tests/test_png_code_host.py and tests/test_png_code_gpu.py put through the PNG writer's code build (the
host builders ``pp_deflate_build_code(_lz)`` against the steps of csrc/pp_png_code_core.h, on the host and in the kernel), and
a restatement of the Huffman merge in Python that says what each named case reaches. Not a test module."""
import numpy as np

SYMS, DIST_SYMS, DIST_AT, HIST_WORDS, HIST_WORDS_LZ = 286, 30, 288, 288, 320
# histogram (a): symbols per code length; a symbol that is to get length l has the count 2^(15 - l)
DEEP_PER_LENGTH = {4: 1, 5: 13, 6: 24, 7: 3, 8: 23, 9: 9, 10: 15, 11: 12, 12: 5, 13: 1, 15: 116}
DEEP_CL_COUNTS = [64, 1, 0, 0, 1, 13, 24, 3, 23, 9, 15, 12, 5, 1, 0, 116]  # of its 287 lengths, the distance code's 1 included


def huffman_depths(counts):
    """{symbol: depth} of build_lengths' tree before any limit: the used symbols (the lowest unused ones added up to two) in
    (count, symbol) order, the two-queue merge with a leaf taken when weight[leaf] <= weight[inner]."""
    counts = [int(c) for c in counts]
    used = [s for s, c in enumerate(counts) if c]
    for s in range(len(counts)):
        if len(used) >= 2:
            break
        if s not in used:
            used.append(s)
    order = sorted(used, key=lambda s: (counts[s], s))
    u = len(order)
    weight = [counts[s] for s in order] + [0] * u
    parent = [-1] * (2 * u)
    leaf, inner, made = 0, u, u
    while made < 2 * u - 1:
        pair = []
        for _ in range(2):
            if leaf < u and (inner >= made or weight[leaf] <= weight[inner]):
                pair.append(leaf)
                leaf += 1
            else:
                pair.append(inner)
                inner += 1
        weight[made] = weight[pair[0]] + weight[pair[1]]
        parent[pair[0]] = parent[pair[1]] = made
        made += 1
    depth = [0] * (2 * u)
    for i in range(2 * u - 3, -1, -1):
        depth[i] = depth[parent[i]] + 1
    return {order[i]: depth[i] for i in range(u)}


def _fibonacci(n):
    out, a, b = [], 1, 1
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def deep_lengths():
    """Histogram (a) and the lengths build_lengths is to give it: {symbol: length}."""
    hist, want, s = np.zeros(HIST_WORDS, np.uint32), {}, 0
    for l, k in DEEP_PER_LENGTH.items():
        for _ in range(k):
            hist[s], want[s] = 1 << (15 - l), l
            s += 1
    assert s == 222
    hist[256], hist[221] = hist[221], 0  # symbol 256 among the used ones, for one of the l15 symbols
    want[256] = want.pop(221)
    return hist, want


def named_runs():
    """{name: 288 uint32}: the named histograms (a) .. (g) of runs mode."""
    rng = np.random.default_rng(17)
    out = {"a: code-length tree deeper than 7": deep_lengths()[0]}
    h = np.zeros(HIST_WORDS, np.uint32)
    h[:40] = _fibonacci(40)
    out["b: Fibonacci on 40 symbols"] = h
    out["c: all counts zero"] = np.zeros(HIST_WORDS, np.uint32)
    h = np.zeros(HIST_WORDS, np.uint32)
    h[256], h[65] = 3, 9
    out["d: 256 and one other"] = h
    h = np.zeros(HIST_WORDS, np.uint32)
    h[:SYMS] = 77
    out["e: all 286 equal"] = h
    h = np.zeros(HIST_WORDS, np.uint32)
    h[:SYMS] = 0xFFFFFFFF
    out["f: all 286 at 2^32 - 1"] = h
    h = np.zeros(HIST_WORDS, np.uint32)
    h[:257] = rng.integers(1, 100000, 257)
    out["g: 257 used symbols"] = h
    return out


def named_distances():
    """{name: 30 uint32}: the distance counts of the named lz histograms."""
    rng = np.random.default_rng(19)
    only29, two = np.zeros(DIST_SYMS, np.uint32), np.zeros(DIST_SYMS, np.uint32)
    only29[29] = 5
    two[4] = two[17] = 6
    return {"all zero": np.zeros(DIST_SYMS, np.uint32), "only symbol 29": only29, "Fibonacci over all 30": np.array(_fibonacci(30), np.uint32),
            "two equal counts": two, "random": rng.integers(0, 1000, DIST_SYMS).astype(np.uint32)}


def named_lz():
    """{name: 320 uint32}: every named literal part with every named distance part."""
    out = {}
    for ln, lit in named_runs().items():
        for dn, dist in named_distances().items():
            h = np.zeros(HIST_WORDS_LZ, np.uint32)
            h[:HIST_WORDS] = lit
            h[DIST_AT:DIST_AT + DIST_SYMS] = dist
            out[f"{ln} | {dn}"] = h
    return out


def _random_counts(rng, n):
    """n counts of one of six kinds (h): any magnitude, many equal counts, geometric, hyperbolic, mostly one value, near
    2^32 - 1; one symbol in `keep` is used."""
    kind, keep, shift = int(rng.integers(6)), int(rng.integers(1, 17)), int(rng.integers(32))
    if kind == 0:
        c = rng.integers(0, 1 << 32, n, dtype=np.uint64) >> np.uint64(shift)
    elif kind == 1:
        c = rng.integers(1, 5, n, dtype=np.uint64)
    elif kind == 2:
        c = np.uint64(1) << rng.integers(0, 32, n, dtype=np.uint64)
    elif kind == 3:
        c = (1.0 + 1e9 / (1.0 + rng.integers(0, 100000, n))).astype(np.uint64)
    elif kind == 4:
        c = np.where(rng.integers(3, size=n) > 0, 7, rng.integers(0, 1 << 32, n, dtype=np.uint64)).astype(np.uint64)
    else:
        c = np.uint64(0xFFFFFFFF) - rng.integers(0, 3, n, dtype=np.uint64)
    return np.where(rng.integers(keep, size=n) == 0, c, 0).astype(np.uint32)


def random_runs(count, seed):
    """(count, 288) uint32: seeded random histograms (h)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((count, HIST_WORDS), np.uint32)
    for i in range(count):
        out[i, :SYMS] = _random_counts(rng, SYMS)
    return out


def random_lz(count, seed):
    """(count, 320) uint32: seeded random histograms of lz mode."""
    rng = np.random.default_rng(seed)
    out = np.zeros((count, HIST_WORDS_LZ), np.uint32)
    for i in range(count):
        out[i, :SYMS] = _random_counts(rng, SYMS)
        out[i, DIST_AT:DIST_AT + DIST_SYMS] = _random_counts(rng, DIST_SYMS)
    return out
