#!/usr/bin/env python
"""Fuzz of the fused logits decode - x / T -> Sparsemax over the H*W pixels -> * normalize -> clamp(0, 1) -> flip merge (with or without
shift_heatmap) -> OKS convolution + argmax decode - against an exact fp64 Sparsemax and the oracle's decode, visited round robin:
pp_probmap_decode_flags with LOGITS, LOGITS|PHASED and LOGITS|SHIFT (each with and without the flip pass), pp_probmap_head_decode,
pp_probmap_head_decode_phased, and the maps path with SHIFT (which tests/fuzz_decode.py does not reach).
Shapes: H >= 9, W >= 12 a multiple of 4 (phased: H even, W a multiple of 8), on both sides of the 768 / 1 792 / 3 072-quad edges of the
NV = 3 / 7 / 12 buckets, the production 64 x 48 and 96 x 72, and one shape past the largest accepted size (refused, outputs untouched); B 0 .. 128;
K 1 .. 17 with a random flip involution; option decode_wgs_per_cu 1 .. 5. Temperatures from both sides of the power-of-two multiply window,
normalize None / 0.5 .. 10. Value classes of the logit rows: peaked blobs, flat rows, rows with exactly 1 / 2 / 1023 / 1024 / 1025 / H*W candidates
(a pass and its flip partner on opposite sides of 1 024: the LDS-list and the walk forms of the threshold search), exact ties and quantised rows,
heavy tails and |x / T| up to 1e30, non-finite poison.
Every case: outputs between canaries (bit for bit), every element written, inputs bit-identical after the launch, a repeat launch bit-identical,
locs / keypoints / scores the same with and without avg_out / conv_out, and the exact equalities the code claims:
  * the phase-separated layout decodes to the planar layout's bits;
  * T = 2^k (the multiply window) equals the T = 1 launch on x * 2^-k, any other T the T = 1 launch on fl32(x / T) (correctly rounded division);
  * normalize None: avg_out == clamp(fl32(x / T), 0, 1), with the flip pass (a + flipback(b)) * 0.5f in fp32 (values: the sign of zero is free);
  * the oracle's decode of the kernel's own avg_out gives its keypoints and scores bit for bit, conv_out is the oracle's fp64 convolution of it
    rounded once;
  * a (b, k) whose row or flip partner holds a non-finite x / T is NaN in every output, every other (b, k) bit-identical to the launch without it.

Accuracy against fp64 (exact sort-based Sparsemax of the fp64 x / T, clamp, flip merge, shift), u = 2^-24, per map row:
  * x / T rounds once: |fl(z) - z| <= u |z|. The support lies within 1 of the row maximum m, so every value that can matter has |z| <= M = |m| + 1,
    and fl(z) - fl(m) rounds a difference <= 1 once more: the shifted row the threshold search sees is off by e_in <= 2 u M + u elementwise.
    Sparsemax commutes with adding a constant and is monotone, so the threshold moves by <= e_in and every probability by <= 2 e_in.
  * the threshold: the search stops when the candidate count repeats, with tau = tau' + fl(fl(s - 1) / n) from the last support (n values),
    s the fp32 sum of fl(z_i - tau'). In exact arithmetic that update IS the threshold of the support. s sums values in (0, 1 + n |tau - tau'|]
    with tau, tau' in [-1, 0], so s <= 1 + n; its summation tree is D = 4 NV + 9 deep (a thread's 4 NV quads in sequence - the LDS-list form has
    <= 16 per lane - 6 butterfly levels, 3 cross-wave adds), |s - s_exact| <= (D + 1) u s_exact. The division, subtraction and addition add
    u |s - 1| / n twice and u |tau|: |tau_fp32 - tau| <= (D + 3) u (1 + n) / n + u <= (2 D + 7) u.
  * the map: fl(fl(z_i - tau) * normalize), clamped: normalize (2 e_in + (2 D + 7) u + u) + u per pass; normalize None is clamp(fl(x / T)): u.
  * the flip merge fl(fl(a + b) * 0.5f): (bound_a + bound_b) / 2 + u.
  The 64-round cap is not in the bound: a search that ends without converging fails it.
Derived quantities: the score is the kernel's map at its argmax: within the row's bound of the fp64 map there. The convolution (taps sum to 1) moves
the bound e to e_c = e + u max|conv| per value (one rounding), so the kernel's argmax holds an fp64 convolved value within 2 e_c of the fp64
maximum; anything else is an argmax flip past a near-tie. Where the argmaxes agree at an interior pixel, the sub-pixel step x - dx / dxx
(dx = (c+ - c-) / 2, dxx = c+ + c- - 2 c) sees |d dx| <= e_c + u |dx|, |d dxx| <= 4 e_c + 4 u (|c+| + |c-| + 2 |c|), so
|loc - loc_64| <= (|d dx| + |off| |d dxx|) / (|dxx| - |d dxx|) + 2 u |off| + u |loc| per axis; when |dxx| <= 2 |d dxx| the step is
ill-conditioned and only counted.
Refusals are counted; a production shape (64 x 48, 96 x 72) is never refused.   python tests/fuzz_decode_logits.py [seconds]"""
import os
import sys
from collections import Counter

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from fuzz_layer import Guard, Refused, bits_equal, run_entries, run_twice  # noqa: E402
from oracle import decode_ref as D  # noqa: E402

U = 2.0 ** -24
SMX_CAP = 1024  # candidates (z > max - 1) the LDS-list form of the threshold search holds per row (pp_decode.hip)
MAX_PIXELS = 12288  # 3 072 quads: the NV = 12 bucket
LOGITS, PHASED, SHIFT = 1, 2, 4  # PP_DECODE_*
# temperatures: the head's 0.5, others, and both sides of the power-of-two multiply window (2^-125 .. 2^125 multiply, 2^+-126 divide)
TEMPERATURES = (0.5, 1.0, 2.0, 0.3, 0.7, 3.0, 1e-3, 2.0 ** -125, 2.0 ** 125, 2.0 ** -126, 2.0 ** 126)
NORMALIZE = (None, 0.5, 1.0, 2.0, 10.0)
CLASSES = ("peaked", "flat", "count", "ties", "heavy", "poison")
EXACT_COUNTS = (1, 2, 1023, 1024, 1025, -1)  # -1: every pixel a candidate
PRODUCTION = ((64, 48), (96, 72))
# both sides of every NV bucket edge (768 / 1 792 / 3 072 quads) and small maps down to 9 pixels high
EDGE_SHAPES = ((64, 48), (96, 72), (9, 12), (9, 16), (10, 16), (12, 16), (16, 24), (59, 52), (48, 64), (55, 56), (193, 16), (56, 56),
               (597, 12), (112, 64), (64, 112), (163, 44), (83, 148), (128, 96), (256, 48), (192, 64))
PAST_MAX = (439, 28)  # 3 073 quads: one past the largest bucket


# ----------------------------------------------------------------------------------------------------- references (imported by the CPU test)
def nv_bucket(H, W):
    q = (H * W // 4 + 255) // 256
    return 3 if q <= 3 else 7 if q <= 7 else 12 if q <= 12 else None


def t_multiplies(T):
    """The kernel multiplies by 1 / T when T is a normal power of two whose reciprocal is normal too (biased exponent 2 .. 252), else divides."""
    b = int(np.array(T, np.float32).view(np.uint32))
    return (b & 0x7FFFFF) == 0 and 2 <= (b >> 23) <= 252


def scale32(x, T):
    """fl32(x / T) as the kernel forms it (the multiply by the exact reciprocal rounds the same real number)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if t_multiplies(T):
            return x * (np.float32(1.0) / np.float32(T))
        return x / np.float32(T)


def sparsemax64(z):
    """Exact sort-based Sparsemax over the last axis in fp64 -> (p, tau) (tau relative to the row maximum, which is subtracted first)."""
    with np.errstate(invalid="ignore"):
        z = np.asarray(z, np.float64)
        z = z - z.max(axis=-1, keepdims=True)
    zs = -np.sort(-z, axis=-1)
    cs = np.cumsum(zs, axis=-1)
    j = np.arange(1, z.shape[-1] + 1)
    n = (1 + j * zs > cs).sum(axis=-1, keepdims=True)  # the condition holds on a prefix of the sorted row
    tau = (np.take_along_axis(cs, n - 1, axis=-1) - 1) / n
    return np.maximum(z - tau, 0.0), tau[..., 0]


def probs64(x, T, normalize):
    """(..., H, W) fp32 logits -> fp64 maps of one pass: clamp(normalize * sparsemax(x / T), 0, 1), or clamp(x / T, 0, 1) for normalize None."""
    z = np.asarray(x, np.float64) / float(np.float32(T))
    if normalize is None:
        return np.clip(z, 0.0, 1.0)
    p, _ = sparsemax64(z.reshape(*z.shape[:-2], -1))
    return np.clip(p.reshape(z.shape) * normalize, 0.0, 1.0)


def flip_back64(m, flip, shift=False):
    """(B, K, H, W): keypoint k of the result is channel flip[k] mirrored; with shift_heatmap column x takes mirrored column x - 1 (column 0 keeps
    its own), i.e. source column W - x for x >= 1 and W - 1 for x = 0."""
    W = m.shape[-1]
    src = np.array([(W - x if x >= 1 else W - 1) if shift else W - 1 - x for x in range(W)])
    return m[:, list(flip)][..., src]


def merge64(a, b, flip, shift):
    return (a + flip_back64(b, flip, shift)) * 0.5


def row_bound(x, T, normalize, nv):
    """(..., H, W) fp32 logits -> (...) the per-pass bound of the module docstring."""
    if normalize is None:
        return np.full(np.shape(x)[:-2], U)
    z = np.asarray(x, np.float64) / float(np.float32(T))
    with np.errstate(invalid="ignore"):
        M = np.abs(z.reshape(*z.shape[:-2], -1).max(axis=-1)) + 1.0
    e_in = 2 * U * M + U
    return normalize * (2 * e_in + (2 * (4 * nv + 9) + 7) * U + U) + U


def map_bound(x, xf, flip, T, normalize, nv):
    """(B, K) bound of the averaged map: one pass, or the flip merge of the pass and its partner (row flip[k] of the flipped pass)."""
    a = row_bound(x, T, normalize, nv)
    if xf is None:
        return a
    return (a + row_bound(xf, T, normalize, nv)[:, list(flip)]) / 2 + U


def poisoned_rows(x, xf, flip, T):
    """(B, K) bool: the (b, k) whose row, or flip partner, holds a non-finite fl32(x / T) - NaN in every output."""
    bad = ~np.isfinite(scale32(x, T)).reshape(*x.shape[:2], -1).all(axis=-1)
    if xf is not None:
        bad = bad | ~np.isfinite(scale32(xf, T)).reshape(*xf.shape[:2], -1).all(axis=-1)[:, list(flip)]
    return bad


def map_error_ratio(got, ref, bound, poisoned):
    """max |got - ref| / bound over the clean (b, k); inf when a clean row is not finite or a poisoned row is not NaN throughout."""
    got = np.asarray(got, np.float64)
    if poisoned.any() and not np.isnan(got[poisoned]).all():
        return float("inf")
    clean = ~poisoned
    if not clean.any():
        return 0.0
    g, r = got[clean], ref[clean]
    if not np.isfinite(g).all():
        return float("inf")
    return float((np.abs(g - r).reshape(g.shape[0], -1).max(axis=-1) / bound[clean]).max())


def to_phased(x):
    """(N, K, H, W) planar -> the phase-separated layout of pp_deconv_head: (N, K, 2 py + px, H/2 * W/2) blocks of pixels (2 y + py, 2 x + px)."""
    N, K, H, W = x.shape
    return np.ascontiguousarray(x.reshape(N, K, H // 2, 2, W // 2, 2).transpose(0, 1, 3, 5, 2, 4))


def candidates32(x, T):
    """(..., H, W) -> (...) the kernel's first candidate count, fl32(fl32(x / T) - max) > -1 (what picks the LDS-list or the walk form)."""
    z = scale32(x, T).reshape(*np.shape(x)[:-2], -1)
    with np.errstate(invalid="ignore", over="ignore"):
        return (z - z.max(axis=-1, keepdims=True) > np.float32(-1)).sum(axis=-1)


def make_row(cls, rng, H, W, n_cand=None):
    """z = x / T of one (H, W) row of a value class (fp64; the caller multiplies by T and rounds to fp32). `n_cand` for class "count"."""
    HW = H * W
    yy, xx = np.mgrid[0:H, 0:W]
    if cls == "peaked":  # a trained head's blob: background well below the peak, 1 - 30 candidates, centred anywhere incl. the borders
        cy, cx = rng.choice([0, H - 1, rng.uniform(0, H - 1)]), rng.choice([0, W - 1, rng.uniform(0, W - 1)])
        s = rng.uniform(0.6, 2.5)
        z = rng.uniform(1.0, 12.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) - 3.0 + 0.3 * rng.standard_normal((H, W))
    elif cls == "flat":  # random-init-like: hundreds to all H * W candidates
        z = rng.uniform(0.02, 1.2) * rng.standard_normal((H, W)) if rng.random() < 0.6 else -rng.uniform(0, rng.uniform(0.3, 1.0), (H, W))
    elif cls == "count":  # exactly n candidates in (-0.9, 0], the rest at <= -1.5
        n = HW if n_cand is None or n_cand < 0 else min(n_cand, HW)
        z = -rng.uniform(1.5, 5.0, HW)
        idx = rng.permutation(HW)[:n]
        z[idx] = -rng.uniform(0.0, 0.9, n)
        z[idx[0]] = 0.0
        z = z.reshape(H, W)
    elif cls == "ties":
        kind = rng.integers(0, 4)
        if kind == 0:  # constant row
            z = np.full((H, W), rng.uniform(-3, 3))
        elif kind == 1:  # 2- or many-way tie at the maximum, the rest below
            z = -rng.uniform(0.0, 2.0, (H, W))
            z.flat[rng.permutation(HW)[:int(rng.choice([2, 3, rng.integers(2, max(3, HW // 4))]))]] = 0.0
        elif kind == 2:  # values exactly at max - 1 (and some just above / below)
            z = -rng.uniform(1.0, 3.0, (H, W))
            idx, m = rng.permutation(HW), int(rng.integers(1, 40))
            z.flat[idx[:m]] = -rng.uniform(0.0, 1.0, m)
            z.flat[idx[0]] = 0.0
            z.flat[idx[m:m + int(rng.integers(1, 200))]] = -1.0
        else:  # quantised to a few decimals: exact ties everywhere
            z = np.round(rng.uniform(0.05, 1.5) * rng.standard_normal((H, W)), int(rng.integers(1, 4)))
    else:  # "heavy": Cauchy tails, or large magnitudes up to |x / T| = 1e30
        if rng.random() < 0.5:
            z = rng.uniform(0.05, 10.0) * rng.standard_cauchy((H, W))
        else:
            z = rng.standard_normal((H, W)) * 10.0 ** rng.uniform(0, 30)
    if rng.random() < 0.3:
        z = z + rng.uniform(-50, 50)  # the maximum subtraction matters
    return z


def logits_from_z(z, T):
    """fp32 logits x with x / T ~ z (finite: a product past the fp32 range is clipped to it)."""
    with np.errstate(over="ignore"):
        x = np.asarray(z, np.float64) * float(np.float32(T))
    return np.clip(x, -3.0e38, 3.0e38).astype(np.float32)


def random_involution(rng, K):
    """A flip permutation: random pairs and fixed points of range(K)."""
    perm, fl = rng.permutation(K), list(range(K))
    for i in range(0, K - 1, 2):
        if rng.random() < 0.7:
            a, b = int(perm[i]), int(perm[i + 1])
            fl[a], fl[b] = b, a
    return fl


def make_batch(rng, B, K, H, W, T, fl, maps=False, cls=None):
    """Logits of a launch: a value class per (b, k) of the pass; with a flip pass (fl not None) the flipped pass's row fl[k] is the partner of
    (b, k), of the same class (class "count": on the other side of 1 024 candidates). -> x, xf, their copies before the poison, classes (B, K),
    {poison kind: count}. `maps`: probability maps for the maps path instead (no poison). `cls`: the classes, else drawn."""
    flip, HW = fl is not None, H * W
    if cls is None:
        cls = rng.choice(CLASSES if not maps else CLASSES[:5], size=(B, K))
    zs, zf = np.empty((B, K, H, W)), np.empty((B, K, H, W)) if flip else None
    for b in range(B):
        for k in range(K):
            c = str(cls[b, k])
            base = c if c != "poison" else str(rng.choice(["peaked", "flat"]))
            n = n2 = None
            if c == "count":
                n = int(rng.choice(EXACT_COUNTS))
                n2 = (1025 if 0 < n <= 1024 else int(rng.choice([1, 2, 1023, 1024]))) if HW > 1024 else int(rng.choice(EXACT_COUNTS))
            zs[b, k] = make_row(base, rng, H, W, n)
            if flip:
                zf[b, fl[k]] = make_row(base, rng, H, W, n2)
    x = logits_from_z(zs, T)
    xf = logits_from_z(zf, T) if flip else None
    x_clean, xf_clean = x.copy(), None if xf is None else xf.copy()
    poison_kind = Counter()
    for b, k in zip(*np.nonzero(cls == "poison")):
        kind = str(rng.choice(["row", "partner", "other"] if flip else ["row", "other"]))
        v = np.float32(rng.choice([np.inf, -np.inf, np.nan]))
        y, xx = int(rng.integers(0, H)), int(rng.integers(0, W))
        if kind == "row":
            x[b, k, y, xx] = v
        elif kind == "partner":
            xf[b, fl[k], y, xx] = v
        else:  # another keypoint's row: (b, k) itself stays clean
            x[b, (k + 1 + int(rng.integers(0, max(1, K - 1)))) % K, y, xx] = v
        poison_kind[kind] += 1
    if maps:  # the maps path reads probability maps as they are: the Sparsemax of the logits
        x = probs64(x, T, 1.0).astype(np.float32)
        xf = probs64(xf, T, 1.0).astype(np.float32) if flip else None
        x_clean, xf_clean = x, xf
    return x, xf, x_clean, xf_clean, cls, poison_kind


# ----------------------------------------------------------------------------------------------------- GPU side
STATS = {k: Counter() for k in ("class", "poison", "form", "candidates", "nv", "temperature", "normalize", "wgs", "refused", "checks")}


def _summary():
    for k, c in STATS.items():
        print(f"{k:12s} " + ", ".join(f"{n}: {v}" for n, v in sorted(c.items(), key=lambda t: str(t[0]))))


def _main(seconds):
    from scipy.ndimage import convolve

    from probpose_code_amd import _lib as L
    from probpose_code_amd.codecs import oks_kernel_taps

    FN = dict(flags="pp_probmap_decode_flags", head="pp_probmap_head_decode", head_phased="pp_probmap_head_decode_phased")

    def call(fn, flags, a):
        """a: dict of the launch arguments (device tensors / None) -> status, raising nothing."""
        args = [L.ptr(a["hm"]), L.ptr(a["hmf"]), L.ptr(a["fi"]), L.ptr(a["taps"]), L.ptr(a["radius"]), a["B"], a["K"], a["H"], a["W"],
                a["in_w"], a["in_h"]]
        args += [a["T"], a["norm"], L.ptr(a["avg"]), L.ptr(a["conv"]), L.ptr(a["locs"]), L.ptr(a["kp"]), L.ptr(a["sc"])]
        if fn == "flags":
            args.append(flags)
        args.append(None)
        return int(getattr(L.lib, FN[fn])(*args))

    def launch(fn, flags, a):
        st = call(fn, flags, a)
        if st != L.PP_OK:
            if st in (L.PP_ERR_UNSUPPORTED, L.PP_ERR_INVALID_ARG):
                raise Refused(f"{L.lib.pp_status_string(st).decode()}: {L.last_error()}")
            raise L.ProbPoseLibraryError(FN[fn], st, L.last_error())
        torch.cuda.synchronize()

    def outputs(B, K, H, W, avg=True, conv=True, must_write=True):
        g = Guard()
        o = dict(avg=g.out("avg_out", (B, K, H, W), must_write=must_write) if avg else None,
                 conv=g.out("conv_out", (B, K, H, W), must_write=must_write) if conv else None,
                 locs=g.out("locs", (B, K, 2), must_write=must_write), kp=g.out("keypoints", (B, K, 2), torch.float64, must_write=must_write),
                 sc=g.out("scores", (B, K), must_write=must_write))
        return g, o

    def untouched(guard):
        return all(bool((full == pat).all()) for _, full, _, _, _, _, pat in guard.outs)

    def draw_shape(rng, phased):
        if rng.random() < 0.5:
            shapes = [s for s in EDGE_SHAPES if not phased or (s[0] % 2 == 0 and s[1] % 8 == 0)]
            return shapes[rng.integers(0, len(shapes))]
        while True:
            H, W = int(rng.integers(9, 300)), 4 * int(rng.integers(3, 220))  # (wide, short maps: some refused for LDS)
            if phased:
                H, W = max(10, H & ~1), max(16, W & ~7)
            if H * W <= MAX_PIXELS:
                return H, W

    def case(name, fn, flags, flip_mode, maps, rng, g):
        phased = fn == "head_phased" or bool(flags & PHASED)
        flip = bool(rng.random() < 0.5) if flip_mode is None else flip_mode
        shift = bool(flags & SHIFT) and flip
        H, W = draw_shape(rng, phased)
        HW, nv = H * W, nv_bucket(H, W)
        K = int(rng.integers(1, 18))
        r = rng.random()
        B = int(rng.integers(1, 5)) if r < 0.6 else int(rng.integers(5, 17)) if r < 0.9 else int(rng.integers(17, 129))
        B = max(1, min(B, 3_000_000 // (K * HW)))
        T = float(np.float32(1.0 if maps else TEMPERATURES[rng.integers(0, len(TEMPERATURES))]))
        normalize = 1.0 if maps else NORMALIZE[rng.integers(0, len(NORMALIZE))]
        norm_arg = -1.0 if normalize is None else float(normalize)
        wgs = None
        if rng.random() < 0.5:
            wgs = int(rng.integers(1, 6))
            L.set_option("decode_wgs_per_cu", wgs)
        fl = random_involution(rng, K)
        in_w, in_h = float(4 * W), float(4 * H)
        faults = []
        info = f"{name} B {B} K {K} {H}x{W} T {T:g} normalize {normalize} flip {flip} shift {shift} wgs {wgs}"

        x, xf, x_clean, xf_clean, cls, poison_kind = make_batch(rng, B, K, H, W, T, fl if flip else None, maps)
        bad = poisoned_rows(x, xf, fl, T) if not maps else np.zeros((B, K), bool)

        # ---- device inputs
        taps, radius = oks_kernel_taps(K, H, W)
        gin = Guard()
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
        lay = to_phased if phased else (lambda a: a)
        args = dict(B=B, K=K, H=H, W=W, in_w=in_w, in_h=in_h, T=T, norm=norm_arg)
        args.update(hm=gin.inp("logits", dev(lay(x))), hmf=gin.inp("logits_flip", dev(lay(xf))) if flip else None,
                    fi=gin.inp("flip_indices", torch.tensor(fl, dtype=torch.int32)) if flip else None,
                    taps=gin.inp("taps", torch.from_numpy(taps)), radius=gin.inp("radius", torch.from_numpy(radius)))

        # ---- refusals probed on the host side only: one shape past the largest bucket, and an empty batch that writes nothing
        if rng.random() < 0.1:
            PH, PW = PAST_MAX
            gp, op = outputs(1, 1, PH, PW, must_write=False)
            big = torch.zeros((2, 1, PH * PW), device="cuda")
            st = call(fn, flags, dict(args, B=1, K=1, H=PH, W=PW, hm=big[0], hmf=big[1] if flip else None, taps=args["taps"][:1],
                                      radius=args["radius"][:1], fi=torch.zeros(1, dtype=torch.int32, device="cuda") if flip else None, **op))
            torch.cuda.synchronize()
            if st != L.PP_ERR_UNSUPPORTED:
                faults.append(f"{PH}x{PW} not refused as UNSUPPORTED ({st})")
            if not untouched(gp):
                faults.append(f"{PH}x{PW}: refused launch wrote its outputs")
            STATS["checks"]["past-max refused"] += 1
        if rng.random() < 0.05:
            ge, oe = outputs(B, K, H, W, must_write=False)
            st = call(fn, flags, dict(args, B=0, **oe))
            torch.cuda.synchronize()
            if st != L.PP_OK or not untouched(ge):
                faults.append(f"B = 0: status {st} or outputs written")
            STATS["checks"]["B = 0"] += 1

        # ---- the launch under test, with every output, twice
        guard, o = outputs(B, K, H, W)
        try:
            faults_run, snap = run_twice(guard, lambda: launch(fn, flags, dict(args, **o)))
        except Refused:
            if (H, W) in PRODUCTION:
                return [f"production shape refused: {L.last_error()}"], float("inf"), info
            STATS["refused"][f"{'phased ' if phased else ''}{H}x{W}"] += 1
            raise
        faults += faults_run + [f for f in gin.faults() if f not in faults_run]
        avg, conv, locs, kp, sc = (t.cpu().numpy() for t in snap)

        # ---- bookkeeping of what this case covers
        STATS["nv"][nv] += 1
        STATS["wgs"][wgs if wgs else "default"] += 1
        if not maps:
            STATS["temperature"]["multiply" if t_multiplies(T) else "divide"] += 1
            STATS["normalize"][str(normalize)] += 1
            for c, n in Counter(str(c) for c in cls.ravel()).items():
                STATS["class"][c] += n
            for kd, n in poison_kind.items():
                STATS["poison"][kd] += n
            STATS["poison"]["(b, k) NaN"] += int(bad.sum())
            if normalize is not None:
                n0 = candidates32(x, T)
                n1 = candidates32(xf, T)[:, fl] if flip else np.zeros_like(n0)
                for b, k in zip(*np.nonzero(~bad)):
                    a0, a1 = int(n0[b, k]), int(n1[b, k])
                    STATS["form"]["walk" if max(a0, a1) > SMX_CAP else "LDS list"] += 1
                    if flip and (a0 > SMX_CAP) != (a1 > SMX_CAP):
                        STATS["form"]["mixed pair"] += 1
                    for a in (a0, a1) if flip else (a0,):
                        STATS["candidates"]["<= 1024" if a <= SMX_CAP else "> 1024"] += 1
                        if a in (1023, 1024, 1025):
                            STATS["candidates"][a] += 1

        # ---- avg_out / conv_out NULL: the same keypoints
        want_avg, want_conv = [(False, False), (True, False), (False, True)][rng.integers(0, 3)]
        g2, o2 = outputs(B, K, H, W, want_avg, want_conv)
        launch(fn, flags, dict(args, **o2))
        faults += ["(NULL maps) " + f for f in g2.faults()]
        s2 = {k: v for k, v in o2.items() if v is not None}
        if not bits_equal([s2["locs"], s2["kp"], s2["sc"]], snap[2:]) or (want_avg and not bits_equal([s2["avg"]], snap[:1])) or (
                want_conv and not bits_equal([s2["conv"]], snap[1:2])):
            faults.append(f"results differ with avg_out {want_avg} conv_out {want_conv}")

        def same_launch(label, a):
            gx, ox = outputs(B, K, H, W)
            a = dict(args, **a, **ox)
            try:
                launch(a.pop("fn", fn), a.pop("flags", flags), a)
            except Refused as e:
                faults.append(f"{label}: refused ({e})")
                return
            if not bits_equal([ox[k] for k in ("avg", "conv", "locs", "kp", "sc")], snap):
                faults.append(f"{label}: outputs differ")
            STATS["checks"][label] += 1

        # ---- exact equalities
        if phased:  # the planar layout, same bits
            same_launch("phased == planar", dict(fn="flags", flags=flags & ~PHASED if fn == "flags" else LOGITS, hm=dev(x).cuda(),
                                                 hmf=dev(xf).cuda() if flip else None))
        if not maps:  # T = 1 on the host-scaled logits
            lay_dev = lambda a: None if a is None else dev(lay(scale32(a, T))).cuda()  # noqa: E731
            same_launch("T == 1 on fl32(x / T)", dict(T=1.0, hm=lay_dev(x), hmf=lay_dev(xf)))
        if bad.any():  # without the poison: every other (b, k) the same bits
            gx, ox = outputs(B, K, H, W)
            launch(fn, flags, dict(args, hm=dev(lay(x_clean)).cuda(), hmf=dev(lay(xf_clean)).cuda() if flip else None, **ox))
            ref = [ox[k].cpu().numpy() for k in ("avg", "conv", "locs", "kp", "sc")]
            clean = ~bad & ~poisoned_rows(x_clean, xf_clean, fl, T)
            for nm, got, want in zip(("avg", "conv", "locs", "kp", "sc"), (avg, conv, locs, kp, sc), ref):
                if not np.array_equal(got[clean].view(np.uint8), want[clean].view(np.uint8)):
                    faults.append(f"poison leaks into a clean (b, k) through {nm}")
                if not np.isnan(got[bad]).all():
                    faults.append(f"poisoned (b, k) not NaN in {nm}")
            STATS["checks"]["poison isolated"] += 1
        if maps:  # the maps path: tta_average with shift bit for bit
            want = D.tta_average(x, xf, fl, shift_heatmap=shift) if flip else x
            if not np.array_equal(avg, want):
                faults.append("maps path: avg_out != tta_average")
        elif normalize is None:
            a = np.clip(scale32(x, T), 0, 1)
            want = D.tta_average(a, np.clip(scale32(xf, T), 0, 1), fl, shift_heatmap=shift) if flip else a
            if not (avg[~bad] == want[~bad]).all():
                faults.append("normalize None: avg_out != clamp(fl32(x / T), 0, 1) merged in fp32")
            STATS["checks"]["normalize None exact"] += 1

        # ---- oracle decode of the kernel's own map, fp64 accuracy: on a sample of the batch
        bs = sorted({0, B - 1, int(rng.integers(0, B))})
        ratio = 0.0
        kern = D.oks_kernels(K, H, W)
        for b in bs:
            ok_k = ~bad[b]
            locs_o, vals_o, conv_o = D.heatmap_expected_value(np.array(avg[b]), return_conv=True)
            kp_o = locs_o[None] / [W - 1, H - 1] * [in_w, in_h]
            if not (np.array_equal(kp[b][ok_k], kp_o[0][ok_k]) and np.array_equal(sc[b][ok_k], vals_o[ok_k])
                    and np.array_equal(conv[b][ok_k], conv_o[ok_k])):
                faults.append(f"b {b}: oracle decode of the kernel's map differs")
            if maps:
                continue
            a64 = probs64(x[b:b + 1], T, normalize)
            ref = merge64(a64, probs64(xf[b:b + 1], T, normalize), fl, shift)[0] if flip else a64[0]
            bound = map_bound(x[b:b + 1], xf[b:b + 1] if flip else None, fl, T, normalize, nv)[0]
            ratio = max(ratio, map_error_ratio(avg[b], ref, bound, bad[b]))
            for k in np.nonzero(ok_k)[0]:
                c64 = convolve(ref[k], kern[k], mode="reflect")
                idx = int(np.argmax(conv_o[k]))
                e_c = bound[k] + U * float(np.abs(c64).max())
                ratio = max(ratio, abs(float(sc[b, k]) - ref[k].flat[idx]) / bound[k])
                gap = float(c64.max() - c64.flat[idx])
                ratio = max(ratio, gap / (2 * e_c))
                if idx != int(np.argmax(c64)):
                    STATS["checks"]["argmax flip (near-tie)"] += 1
                    continue
                yi, xi = divmod(idx, W)
                if not (0 < xi < W - 1 and 0 < yi < H - 1):
                    ratio = max(ratio, 0.0 if (locs[b, k] == [xi, yi]).all() else float("inf"))
                    continue
                for ax, (cp, cm) in enumerate(((c64[yi, xi + 1], c64[yi, xi - 1]), (c64[yi + 1, xi], c64[yi - 1, xi]))):
                    c = c64[yi, xi]
                    dx, dxx = (cp - cm) / 2, cp + cm - 2 * c
                    ddx, ddxx = e_c + U * abs(dx), 4 * e_c + 4 * U * (abs(cp) + abs(cm) + 2 * abs(c))
                    if abs(dxx) <= 2 * ddxx:
                        STATS["checks"]["ill-conditioned sub-pixel step"] += 1
                        continue
                    off = -dx / dxx
                    loc = (xi, yi)[ax] + off
                    tol = (ddx + abs(off) * ddxx) / (abs(dxx) - ddxx) + 2 * U * abs(off) + U * abs(loc)
                    ratio = max(ratio, abs(float(locs[b, k, ax]) - loc) / tol)
                    STATS["checks"]["sub-pixel steps"] += 1
        return faults, ratio, info

    entries = [
        ("flags LOGITS", lambda rng, g: case("flags LOGITS", "flags", LOGITS, False, False, rng, g)),
        ("flags LOGITS + flip", lambda rng, g: case("flags LOGITS + flip", "flags", LOGITS, True, False, rng, g)),
        ("flags LOGITS|PHASED", lambda rng, g: case("flags LOGITS|PHASED", "flags", LOGITS | PHASED, False, False, rng, g)),
        ("flags LOGITS|PHASED + flip", lambda rng, g: case("flags LOGITS|PHASED + flip", "flags", LOGITS | PHASED, True, False, rng, g)),
        ("flags LOGITS|SHIFT", lambda rng, g: case("flags LOGITS|SHIFT", "flags", LOGITS | SHIFT, False, False, rng, g)),
        ("flags LOGITS|SHIFT + flip", lambda rng, g: case("flags LOGITS|SHIFT + flip", "flags", LOGITS | SHIFT, True, False, rng, g)),
        ("pp_probmap_head_decode", lambda rng, g: case("head_decode", "head", 0, None, False, rng, g)),
        ("pp_probmap_head_decode_phased", lambda rng, g: case("head_decode_phased", "head_phased", 0, None, False, rng, g)),
        ("flags SHIFT (maps) + flip", lambda rng, g: case("flags SHIFT maps", "flags", SHIFT, True, True, rng, g)),
    ]
    return run_entries(entries, seconds, 90000, "DECODE LOGITS", L, summary=_summary)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sys.exit(_main(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0))


if __name__ == "__main__":
    main()
