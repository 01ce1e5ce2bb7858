#!/usr/bin/env python
"""Fuzz of the two swapped-codec decode launches over what their argument checks admit, against references the suite already trusts:

  * pp_argmax_probmap_decode (csrc/pp_argmax_decode.hip: Sparsemax + flip average + UDP argmax + DARK in one launch) against the exact fp64
    Sparsemax of tests/fuzz_decode_logits.py (``probs64`` / ``merge64`` under ``map_bound``) and the fp64 DARK decode of tests/udp_ref.py
    (``decode_f64`` under its ``bound``) - independent of the two launches it is assembled from, and against those two chained wherever both
    admit the shape;
  * pp_expmax_heatmap_decode (the RAW load mode of csrc/pp_decode.hip) against oracle/decode_ref.py bit for bit: the fp32 flip average, the
    fp64 convolution rounded once, the first-occurrence argmax, the fp32 sub-pixel step, the fp64 rescale.

The CASE TABLE is fixed (fixed seeds, the same on every run): ``argmax_table()`` and ``expmax_table()``. tests/test_codec_swap_references.py
(CPU) pins the restated admission predicates against the real library, counts what the table reaches, holds the 2 % cap for the reference
alone and drives the checkers with reference-made outputs and single faults; tests/test_codec_swap_fuzz_gpu.py runs the table on the GPU.
Launching (``launch_*`` / ``run_*_case``: device buffers between canaries, inputs compared after the launch) and checking (``check_argmax`` /
``check_expmax``: numpy only) are separate, so the CPU test can feed the checkers.

Admission restated from the PP_REQUIRE lines:
  argmax   H, W >= 2, W % 4 == 0, PHASED: H even and W % 8 == 0, blur_kernel_size odd 1 .. 19, H * W <= 12 288 and
           512 + 4 * (region + H * ((W + 2 r) | 1)) <= 160 KiB - 256 (the kernel's static LDS, below), region = max(H (W + 24) + 32, 2 048, (H + 2 r) W) rounded up to 4;
  expmax   K <= 17, PHASED: H even and W % 8 == 0, H, W >= 9, W % 4 == 0, a band buffer that fits (``rowd_doubles``), H * W <= 12 288.
A refused case checks the status, a word of the message, and that every byte between the canaries of every output is untouched.

Checks of every admitted case, both kernels: canaries intact, inputs bit-identical after the launch, a second launch into fresh buffers
bit-identical, locs / keypoints / scores the same with and without the optional map outputs, a poisoned (b, k) NaN in every output and every
other (b, k) bit-identical to the launch without the poison, the phase-separated layout bit-identical to the planar one.
argmax: avg_out within ``map_bound(..., nv_bucket(H, W))`` of ``merge64(probs64(...))``; normalize None: the fp32 identity of
fuzz_decode_logits (clamp(fl32(x / T), 0, 1), merged in fp32); locs / scores = numpy's first-occurrence argmax / max of the kernel's own
avg_out ((-1, -1) where that maximum is <= 0), bit for bit; keypoints within ``udp_ref.decode_f64(avg_out[b], ks, input_size)["bound"]``
wherever its ``cond`` < 100 - nothing else is left out, and on the "blob" class at most 2 % may be (``BLOB_CAP``; the cap is on the aggregate
over the table, >= 2 000 blob keypoints compared). No tolerance of its own: the two bounds are the derived ones of those modules. The fused
path adds no term to either: the Sparsemax stage is the code map_bound was derived for, the copy into the blur's image moves fp32 values, and
the blur of a radius given at run time sums in the order of the compile-time form (csrc/pp_decode_stages.h).
A (b, k) whose averaged map has maximum <= 0 takes three of its seven points from keypoint k - 1 (K - 1 for k = 0); the header says that such
a (b, k) is NaN when THAT map is poisoned. The table keeps the two apart (``_keep_neighbours_clean``), so that "every other (b, k)" has no
exception.
expmax: bit for bit against the oracle, with ONE derived exception. The kernel's convolution is separable (row pass, column pass, one fused
multiply-add per tap), the oracle's - and scipy's - a raster sum over the 2-D kernel with a product and a sum per tap; both are fp64 and are
compared after the ONE rounding to fp32. With u = 2^-53, d = 2 r + 1 and A = the same convolution of |map|:
  oracle     d^2 products and d^2 sums in sequence:                              |fl - exact| <= (d^2 + 1) u A;
  kernel     d fused steps per pass, the column pass on row sums already rounded: |fl - exact'| <= (2 d + 1) u A;
  kernels    exact' uses t_i t_j for the 2-D weight w_ij = exp(-(i^2 + j^2) / 2s) / sum: the exponent (up to r^2 / s <= 34) carries 3
             roundings into the weight, the 1-D factors theirs, the two normalisations theirs: |t_i t_j - w_ij| <= 128 u w_ij
             (``SEPARABLE_ULPS``; tests/test_codec_swap_references.py measures 67 u at most over the table's shapes);
so |kernel - oracle| <= E = (d^2 + 2 d + 130) u A in fp64 (``cancel_bound``). A is the size of the LARGEST partial sum; where the result
does not cancel E is ~2^-44 of it and the fp32 roundings agree (every class but one: equal bits, asserted). Where the result is a
cancellation residue - class "cancel_rows": +-2^e pairs two columns apart in rows y, y + 2, ..., which cancel across rows - the oracle has
0.0 or a residue of its own and the kernel another (1.3e-21 against 0.0, 1.5e-17 against 2.1e-17 on values of order 1). That class is
checked as the guarantee of include/probpose_mi355x.h reads: conv_out within [fl32(c - E), fl32(c + E)] of the oracle's fp64 sum c; locs,
keypoints and scores bit for bit the oracle's argmax / sub-pixel step / rescale applied to the kernel's OWN conv_out; and the kernel's
integer argmax a pixel whose oracle value is within 2 E (and one fp32 rounding) of the oracle's maximum - an argmax that moves does so only
between pixels the oracle itself ties to within its rounding. Class "sparse_cancel" (ONE pair in one row: every product is exact in both
sums) stays under the exact check.

The LDS rule the argmax table's edges pin: the kernels of the DARK stage hold 256 bytes of LDS statically (the workgroup reduction behind
__syncthreads_or), hipFuncSetAttribute takes a dynamic size of 160 KiB less that, and so do the argument checks of
pp_argmax_probmap_decode and pp_udp_heatmap_decode (UDP_STATIC_LDS, csrc/pp_decode_stages.h).

UNPINNED, next to the notes of tests/udp_ref.py and tests/golden/make_golden_udp.py: the blur taps for blur_kernel_size 3, 5, 7 (and 9).
``udp_gaussian_taps`` (csrc/pp_decode_stages.h) and ``udp_ref.gaussian_taps`` use the sigma formula for every size; OpenCV's
GaussianBlur(..., sigmaX = 0) is understood to use fixed binomial tables for the small sizes. cv2 is not installed where the fixtures are
made and the golden generators stub it, so neither form is pinned against cv2; kernel and reference agree with each other, which is all the
checks here can say for those sizes.

python tests/fuzz_codec_swap.py [seconds]   (the table, then random cases for ``seconds``)"""
import functools
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import fuzz_decode_logits as FD  # noqa: E402
import udp_ref as R  # noqa: E402
from oracle import decode_ref as D  # noqa: E402

F32 = np.float32
LOGITS, PHASED, SHIFT = 1, 2, 4  # PP_DECODE_*
GUARD = 64  # canary elements either side of an output
FILL = -777.0
MAX_PIXELS = 12288
LDS_BYTES = 160 * 1024
RM = 9  # PP_MAX_RADIUS
STATIC_LDS = 256  # what the kernels of the DARK stage hold statically (UDP_STATIC_LDS, csrc/pp_decode_stages.h)
BLOB_CAP = 0.02  # share of the blob class's keypoints that may be left out for cond >= 100, over the whole table
BLOB_MIN = 2000
UDP_TOP_H = 1509  # the largest H pp_udp_heatmap_decode admits at W = 4, kernel size 19 (its LDS check, with the static part)
KS_ALL = tuple(range(1, 20, 2))
KS_COMPILE_TIME = (11, 17)
NORMALIZE = (None, 0.5, 1.0, 10.0)
BLOB_T = (0.5, 1.0, 0.7)
# temperatures of the other classes: fuzz_decode_logits.TEMPERATURES (make_batch keeps x / T finite at every one of them)
OK, INVALID_ARG, UNSUPPORTED = "PP_OK", "PP_ERR_INVALID_ARG", "PP_ERR_UNSUPPORTED"


# ----------------------------------------------------------------------------------------------------- admission, restated
def argmax_lds(H, W, ks):
    r = (ks - 1) // 2
    region = (max(H * (W + 24) + 32, 2048, (H + 2 * r) * W) + 3) & ~3
    return 512 + 4 * (region + H * ((W + 2 * r) | 1))


def argmax_refusal(H, W, ks, phased=False):
    """None where pp_argmax_probmap_decode admits the shape, else (status, a word of its message), in the order of the checks."""
    if H < 2 or W < 2:
        return INVALID_ARG, "at least 2 x 2"
    if ks < 1 or ks % 2 == 0:
        return INVALID_ARG, "odd"
    if ks > 2 * RM + 1:
        return UNSUPPORTED, "above 19"
    if W % 4:
        return UNSUPPORTED, "multiple of 4"
    if phased and (H % 2 or W % 8):
        return UNSUPPORTED, "even height"
    if H * W > MAX_PIXELS:
        return UNSUPPORTED, "12288"
    if argmax_lds(H, W, ks) > LDS_BYTES - STATIC_LDS:
        return UNSUPPORTED, "LDS"
    return None


def argmax_admits(H, W, ks, phased=False):
    return argmax_refusal(H, W, ks, phased) is None


def rowd_doubles(H, W, wgs=3):
    """decode_rowd_doubles of csrc/pp_decode.hip: the band buffer's capacity in doubles (option decode_wgs_per_cu = 3), -1: does not fit."""
    fixed = 512 + (((H * (W + 24) + 32) * 4 + 15) & ~15)
    full = (H + 2 * RM) * (W + 7)
    for n in range(min(5, max(1, wgs)), 0, -1):
        budget = LDS_BYTES // n - 1536
        if budget <= fixed:
            continue
        cap = min(full, (budget - fixed) // 8)
        if cap == full or cap >= (2 * RM + 16) * (W + 7):
            return cap
    return -1


def expmax_refused(H, W, K, phased=False):
    """None where pp_expmax_heatmap_decode admits the shape (B >= 1), else (status, a word of its message)."""
    if K > 17:
        return UNSUPPORTED, "17 sigmas"
    if K < 1 or H < 1 or W < 1:
        return INVALID_ARG, "bad B/K/H/W"
    if phased and (H % 2 or W % 8):
        return UNSUPPORTED, "even height"
    if H < RM or W < RM:
        return UNSUPPORTED, "radius (9)"
    if W % 4:
        return UNSUPPORTED, "multiple of 4"
    if rowd_doubles(H, W) <= 0:
        return UNSUPPORTED, "LDS"
    if FD.nv_bucket(H, W) is None:
        return UNSUPPORTED, "12288"
    return None


def radius_of(K, H, W):
    return [k.shape[0] // 2 for k in D.oks_kernels(K, H, W)]


def box_of(m, r):
    """The kernel's box of one (H, W) map: the non-zero pixels (-0.0 is zero, NaN is not) dilated by the radius -> (ya, yb, xa, xb) or None."""
    H, W = m.shape
    ys, xs = np.nonzero(m != 0)
    if ys.size == 0:
        return None
    return max(ys.min() - r, 0), min(ys.max() + r, H - 1), max(xs.min() - r, 0), min(xs.max() + r, W - 1)


def zidx_branch(m, r):
    """Which pixel outside the convolved box competes as the first 0.0f (probmap_decode_kernel): -> (branch name, flat index or -1)."""
    H, W = m.shape
    box = box_of(m, r)
    if box is None:
        return "empty", 0
    ya, yb, xa, xb = box
    if ya > 0 or xa > 0:
        return "origin", 0
    if xb < W - 1:
        return "right", xb + 1
    if yb < H - 1:
        return "below", (yb + 1) * W
    return "none", -1


def conv_bands(m, r):
    """Bands conv_banded takes for one (H, W) map of radius r at the default band buffer."""
    H, W = m.shape
    box = box_of(m, r)
    if box is None:
        return 0
    ya, yb, xa, xb = box
    cap, rows = rowd_doubles(H, W), yb - ya + 1
    nx4 = (xb - xa + 1 + 3) & ~3
    Wr = W + (((nx4 >> 2) - W) % 8)
    NR = cap // Wr
    if NR < rows + 2 * r:
        NR = cap // W
    if rows <= NR - 2 * r:
        return 1
    band = ((NR - 2 * r) * 2) // 3
    return -(-rows // band)


# ----------------------------------------------------------------------------------------------------- the case tables
def _pick(seq, i, stride=1):
    return seq[(i * stride) % len(seq)]


def _maps_kb(H, W, i, blob):
    """(K, B): K in {1, 2, 3, 17} cycling; at most 64 maps per case, 8 above 4 096 pixels. Blob cases carry as many maps as that allows."""
    if H * W > 4096:
        return _pick(((1, 8), (2, 4), (3, 2), (2, 3)), i) if blob else _pick(((2, 2), (3, 2), (1, 3), (2, 4)), i)
    return _pick(((17, 3), (2, 32), (3, 21), (1, 64)), i) if blob else _pick(((3, 3), (17, 1), (2, 4), (1, 5), (17, 2)), i)


ARGMAX_SMALL = ((2, 4), (3, 4), (2, 8), (4, 8), (5, 8), (8, 8), (9, 12), (16, 12), (16, 16))
ARGMAX_LONG = ((4, 256), (6, 512), (24, 512), (3, 1024), (2, 6144))
ARGMAX_CLASSES = FD.CLASSES + ("blob",)
FLIPS = ("none", "plain", "shift")


def largest_h(W, ks):
    """The largest H pp_argmax_probmap_decode admits at this width and kernel size."""
    H = MAX_PIXELS // W
    while not argmax_admits(H, W, ks):
        H -= 1
    return H


@functools.lru_cache(maxsize=None)
def argmax_table():
    cases = []

    def add(group, H, W, ks, i, cls=None, flip=None, phased=None, normalize="cycle", T=None, K=None, B=None, neg_at="cycle"):
        n = len(cases)
        cls = cls if cls is not None else _pick(("blob", "mixed", "blob", "peaked", "blob", "count", "ties", "blob", "flat", "heavy"), i)
        blob = cls == "blob"
        kb = _maps_kb(H, W, i, blob)
        K, B = K or kb[0], B or kb[1]
        flip = flip if flip is not None else _pick(FLIPS, i)
        can_phase = H % 2 == 0 and W % 8 == 0
        phased = (can_phase and i % 2 == 1) if phased is None else phased
        if normalize == "cycle":  # (blob cases: mostly the head's own scales - see "blob_clamped" in _argmax_data)
            normalize = _pick((1.0, 0.5, 1.0, None, 1.0, 0.5, 10.0, 1.0), i) if blob else _pick(NORMALIZE, i, 3)
        if T is None:
            T = _pick(BLOB_T, i) if cls in ("blob", "mixed") else _pick(FD.TEMPERATURES, i, 5)
        neg = None
        if K >= 2 and normalize is None and cls != "poison":
            neg = _pick((0, 1, K - 1), i) if neg_at == "cycle" else neg_at
        cases.append(dict(kind="argmax", id=n, group=group, H=H, W=W, ks=ks, B=B, K=K, T=float(F32(T)), normalize=normalize, flip=flip,
                          phased=bool(phased), cls=cls, neg_at=neg, seed=910000 + n, refused=argmax_refusal(H, W, ks, bool(phased))))

    # ---- the smallest maps (below what the chain's first launch admits: H < 9) up to 16 x 16, every kernel size
    i = 0
    for rep in range(6):
        for s, (H, W) in enumerate(ARGMAX_SMALL):
            add("small", H, W, _pick(KS_ALL, i, 3), i, phased=True if (H, W) == (2, 8) else None)
            i += 1
    for n, (H, W) in enumerate(((4, 8), (5, 8), (8, 8), (9, 12), (3, 4), (2, 8), (4, 8), (8, 8), (16, 12))):
        # the neighbour-map path on maps so small that both bottom corners of the neighbour are lit: the Hessian of those seven points is
        # well conditioned, and a decode that read the wrong neighbour would be seen
        add("small", H, W, _pick((3, 5, 11, 1, 17, 7), n), n, cls="blob", normalize=None, T=_pick((1.0, 0.5), n), K=_pick((3, 17, 3), n), B=3,
            flip=_pick(("none", "none", "plain", "shift"), n), neg_at=_pick((0, 1, 2), n))
    # ---- every (NV bucket, compile-time / run-time radius, flip, phased) at fuzz_decode_logits.EDGE_SHAPES: both sides of the bucket edges
    i = 0
    for nv in (3, 7, 12):
        shapes = [s for s in FD.EDGE_SHAPES if FD.nv_bucket(*s) == nv]
        for ct in (True, False):
            for flip in FLIPS:
                for phased in (False, True):
                    pool = [s for s in shapes if not phased or (s[0] % 2 == 0 and s[1] % 8 == 0)]
                    H, W = _pick(pool, i)
                    ks = _pick(KS_COMPILE_TIME, i) if ct else _pick((1, 3, 5, 7, 9, 13, 15, 19), i)
                    add("production", H, W, ks, i, flip=flip, phased=phased)
                    i += 1
    for H, W in FD.EDGE_SHAPES:  # every edge shape once more, whatever the draw above took
        add("production", H, W, _pick(KS_ALL, i, 7), i)
        i += 1
    for H, W in FD.PRODUCTION:  # the production sizes at every kernel size
        for ks in KS_ALL:
            add("production", H, W, ks, i, cls="blob" if (H, W) == (64, 48) else None)
            i += 1
    # ---- rows longer than the workgroup, and the largest H of a width / kernel size with the one above it (LDS or the pixel cap)
    i = 0
    for H, W in ARGMAX_LONG:
        for rep in range(2):
            ks = 1 if W == 6144 else _pick((1, 11, 5, 17, 19, 3), i)
            add("long", H, W, ks, i, cls=_pick(("blob", "mixed", "peaked", "ties"), i))
            i += 1
    for W in (4, 48, 512):
        for ks in (1, 11, 19):
            H = largest_h(W, ks)
            add("long", H, W, ks, i, cls=_pick(("blob", "mixed", "peaked"), i), K=_pick((1, 2), i), B=1, phased=False)
            add("refused", H + 1, W, ks, i, cls="peaked", K=1, B=1, phased=False, flip="none")
            i += 1
    # ---- poison in the pass, in the flip partner, in another keypoint; and the refusals of the other checks
    i = 0
    for (H, W), flip, normalize in (((9, 12), "plain", 1.0), ((2, 8), "none", None), ((16, 16), "shift", None), ((64, 48), "plain", 0.5),
                                    ((96, 72), "shift", 1.0), ((4, 256), "none", 10.0), ((16, 12), "plain", None)):
        add("poison", H, W, _pick((11, 3, 17, 19, 1, 7, 9), i), i, cls="poison", flip=flip, normalize=normalize, T=_pick((0.5, 1.0, 0.3), i),
            K=2 if H * W > 4096 else _pick((3, 17, 2), i), B=2)
        i += 1
    for (H, W), ks, phased in (((9, 10), 1, False), ((9, 6), 11, False), ((9, 16), 11, True), ((10, 12), 11, True), ((16, 16), 21, False),
                               ((16, 16), 12, False), ((439, 28), 11, False), ((3072, 4), 11, False)):
        add("refused", H, W, ks, i, cls="peaked", K=1, B=1, phased=phased, flip="none", normalize=1.0)
        i += 1
    return tuple(cases)


EXPMAX_DENSE = ("dense", "dense_neg", "constant", "zero", "ties", "tiny", "huge")
EXPMAX_SPARSE = ("sparse_mixed", "sparse_neg", "sparse_cancel", "cancel_rows")
SEPARABLE_ULPS = 128  # |t_i t_j - w_ij| / w_ij of the OKS kernels, in units of 2^-53 (module docstring)
PLACEMENTS = ("top_left", "top_right", "bottom_left", "bottom_right", "top", "bottom", "left", "right", "inside", "all_but_last_column",
              "all_but_last_row", "top_rows", "left_columns")
EXPMAX_SMALL = ((9, 12), (9, 16), (10, 16), (16, 24))


@functools.lru_cache(maxsize=None)
def expmax_table():
    cases = []

    def add(group, H, W, i, cls, K=None, B=None, flip=None, phased=None, place=None):
        n = len(cases)
        big = H * W > 4096
        if K is None:
            K = _pick((1, 2), i) if big else _pick((1, 2, 17), i)
        if B is None:
            B = max(1, min(3, (8 if big else 64) // K))
        flip = flip if flip is not None else _pick(FLIPS, i)
        can_phase = H % 2 == 0 and W % 8 == 0
        phased = (can_phase and i % 2 == 1) if phased is None else phased
        cases.append(dict(kind="expmax", id=n, group=group, H=H, W=W, B=B, K=K, flip=flip, phased=bool(phased), cls=cls, place=place,
                          seed=920000 + n, refused=expmax_refused(H, W, K, bool(phased))))

    i = 0
    for rep in range(4):  # the small shapes: every dense class, K 1 / 2 / 17, every flip mode
        for H, W in EXPMAX_SMALL:
            add("dense", H, W, i, _pick(EXPMAX_DENSE, i), phased=True if (H, W) == (10, 16) else None)
            i += 1
    for H, W in FD.EDGE_SHAPES + FD.PRODUCTION:  # the production sizes and both sides of the bucket edges; dense maps there take several bands
        add("dense", H, W, i, _pick(("dense", "dense_neg", "dense", "ties", "huge", "dense", "tiny", "constant"), i))
        i += 1
    i = 0
    for cls in EXPMAX_SPARSE:  # the rectangle at every corner and edge, without the flip pass: the map is the rectangle itself
        for place in PLACEMENTS:
            H, W = _pick(((9, 12), (16, 24), (10, 16), (64, 48), (12, 16), (9, 16)), i)
            add("sparse", H, W, i, cls, K=_pick((2, 1, 17, 3), i), flip="none", place=place)
            i += 1
    for place in PLACEMENTS:  # ... and with it (an exact mirror as the partner; with the shift the average is no longer the rectangle alone)
        H, W = _pick(((16, 24), (10, 16), (96, 72), (16, 16)), i)
        add("sparse", H, W, i, _pick(EXPMAX_SPARSE, i), K=_pick((2, 1), i), flip=_pick(("plain", "shift"), i), place=place)
        i += 1
    for place in ("top_left", "bottom_right", "inside", "top_right", "bottom_left", "inside"):
        H, W = _pick(((9, 12), (16, 24), (64, 48)), i)
        add("sparse", H, W, i, "single_neg", K=_pick((1, 2, 17), i), flip=_pick(("none", "none", "plain"), i), place=place)
        i += 1
    i = 0
    for (H, W), flip, K in (((9, 12), "plain", 3), ((10, 16), "none", 2), ((16, 24), "shift", 17), ((64, 48), "plain", 17),
                            ((96, 72), "shift", 2), ((16, 16), "plain", 1)):
        add("poison", H, W, i, "poison", K=K, B=2, flip=flip)
        i += 1
    for (H, W), K, phased in (((8, 12), 1, False), ((12, 8), 1, False), ((12, 10), 1, False), ((16, 16), 18, False), ((9, 16), 1, True),
                              ((10, 12), 1, True), ((439, 28), 1, False), ((9, 1364), 1, False)):
        add("refused", H, W, i, "dense", K=K, B=1, flip="none", phased=phased)
        i += 1
    return tuple(cases)


# ----------------------------------------------------------------------------------------------------- case data
def blob_rows(rng, n, H, W):
    """The blob rows of tests/test_codec_swap_gpu.py::make_logits: amplitude 2 / 8 / 30, sigma 1 - 2.5, centre from -1 to W / H, N(0, 0.3)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    amp = rng.choice([2.0, 8.0, 30.0], n)
    cx, cy = rng.random(n) * (W + 1) - 1, rng.random(n) * (H + 1) - 1
    sg = 1.0 + 1.5 * rng.random(n)
    z = amp[:, None, None] * np.exp(-((xx - cx[:, None, None]) ** 2 + (yy - cy[:, None, None]) ** 2) / (2 * sg[:, None, None] ** 2))
    return z + 0.3 * rng.standard_normal((n, H, W))


def none_map32(x, xf, fl, T, shift):
    """normalize None in the kernel's own fp32: clamp(fl32(x / T), 0, 1), the flip pass merged in fp32 (the identity of fuzz_decode_logits)."""
    with np.errstate(invalid="ignore"):
        a = np.clip(FD.scale32(x, T), 0, 1)
        return a if xf is None else D.tta_average(a, np.clip(FD.scale32(xf, T), 0, 1), fl, shift_heatmap=shift)


def _keep_neighbours_clean(x, xf, x_clean, xf_clean, fl, T, shift):
    """normalize None: a (b, k) whose map has maximum <= 0 reads keypoint k - 1; where that one is poisoned, (b, k) gets one positive pixel, so
    that it reads no neighbour."""
    bad = FD.poisoned_rows(x, xf, fl, T)
    avg = none_map32(x_clean, xf_clean, fl, T, shift)
    K = x.shape[1]
    for b, k in zip(*np.nonzero(~bad)):
        if bad[b, (k - 1) % K] and not avg[b, k].max() > 0:
            x[b, k, 0, 0] = x_clean[b, k, 0, 0] = F32(5.0) * F32(T)


@functools.lru_cache(maxsize=6)
def _argmax_data(cid, seed=None):
    c = argmax_table()[cid]
    rng = np.random.default_rng(c["seed"] if seed is None else seed)
    B, K, H, W, T = c["B"], c["K"], c["H"], c["W"], c["T"]
    flip, shift = c["flip"] != "none", c["flip"] == "shift"
    fl = FD.random_involution(rng, K)
    if c["cls"] == "mixed":
        cls = rng.choice(ARGMAX_CLASSES if c["neg_at"] is None else [n for n in ARGMAX_CLASSES if n != "poison"], size=(B, K))
    else:
        cls = np.full((B, K), c["cls"], dtype=object)
    cls = cls.astype(object)
    x, xf, x_clean, xf_clean, _, _ = FD.make_batch(rng, B, K, H, W, T, fl if flip else None, cls=np.where(cls == "blob", "peaked", cls))
    sel = cls == "blob"
    if sel.any():
        rows = lambda: blob_rows(rng, int(sel.sum()), H, W)  # noqa: E731
        conv = (lambda z: z.astype(F32)) if T in [float(F32(t)) for t in BLOB_T] else (lambda z: FD.logits_from_z(z, T))
        x[sel] = x_clean[sel] = conv(rows())
        if flip:
            r = conv(rows())
            for n, (b, k) in enumerate(zip(*np.nonzero(sel))):
                xf[b, fl[k]] = xf_clean[b, fl[k]] = r[n]
    if c["normalize"] in (None, 10.0):
        # clamp(x / T, 0, 1) and clamp(10 p, 0, 1) cut a blob of amplitude 8 or 30 off into a plateau of exact ones: the log map's Hessian
        # there is singular by construction. Such rows are compared like every other (cond < 100) under a name of their own; the 2 % cap
        # is for maps that are blobs when the DARK stage sees them.
        cls[sel] = "blob_clamped"
    if c["neg_at"] is not None:  # an all-negative row (and partner): with normalize None its map is all zero, the decode reads keypoint k - 1
        k = c["neg_at"]
        x[:, k] = x_clean[:, k] = -F32(1.0) - np.abs(x_clean[:, k])
        if flip:
            xf[:, fl[k]] = xf_clean[:, fl[k]] = -F32(1.0) - np.abs(xf_clean[:, fl[k]])
        cls[:, k] = "negative"
    if c["normalize"] is None:
        _keep_neighbours_clean(x, xf, x_clean, xf_clean, fl, T, shift)
    for a in (x, xf, x_clean, xf_clean):
        if a is not None:
            a.setflags(write=False)
    return dict(x=x, xf=xf, x_clean=x_clean, xf_clean=xf_clean, fl=fl, cls=cls, bad=FD.poisoned_rows(x, xf, fl, T))


def raw_dense(rng, n, H, W):
    """ViTPose-like raw maps (tests/test_codec_swap_gpu.py::make_raw_maps): blobs of sigma 2, amplitude 0.3 - 1.6, + N(0, 0.02) - 0.01."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    amp = 0.3 + 1.3 * rng.random(n)
    cx, cy = rng.random(n) * (W + 3) - 2, rng.random(n) * (H + 3) - 2
    m = amp[:, None, None] * np.exp(-((xx - cx[:, None, None]) ** 2 + (yy - cy[:, None, None]) ** 2) / 8.0)
    return (m + 0.02 * rng.standard_normal((n, H, W)) - 0.01).astype(F32)


def rectangle(place, H, W, rng):
    """(y0, y1, x0, x1) inclusive of a small rectangle (3 - 4 pixels a side) at a corner / an edge / inside, or of one of the large ones."""
    h, w = int(rng.integers(3, 5)), int(rng.integers(3, 5))
    ym, xm = int(rng.integers(1, H - h)), int(rng.integers(1, W - w))
    y0 = {"top": 0, "bottom": H - h}.get(place.split("_")[0], ym)
    x0 = xm
    if place.endswith("left"):
        x0 = 0
    if place.endswith("right"):
        x0 = W - w
    if place in ("left", "right"):
        y0 = ym
    box = dict(all_but_last_column=(0, H - 1, 0, W - 2), all_but_last_row=(0, H - 2, 0, W - 1), top_rows=(0, h - 1, 0, W - 1),
               left_columns=(0, H - 1, 0, w - 1)).get(place)
    return box if box else (y0, y0 + h - 1, x0, x0 + w - 1)


def raw_maps(cls, rng, n, H, W, place=None):
    """``n`` (H, W) fp32 raw maps of one value class of the expmax table."""
    if cls == "dense":
        return raw_dense(rng, n, H, W)
    if cls == "dense_neg":
        return -np.abs(raw_dense(rng, n, H, W)) - F32(1e-3)
    if cls == "tiny":
        return raw_dense(rng, n, H, W) * F32(1e-30)
    if cls == "huge":
        return raw_dense(rng, n, H, W) * F32(1e30)
    if cls == "constant":
        return np.broadcast_to(rng.choice([-0.3, 0.25, 1.5, -1e-30], n).astype(F32)[:, None, None], (n, H, W)).copy()
    if cls == "zero":
        m = np.zeros((n, H, W), F32)
        m[rng.random((n, H, W)) < 0.3] = -0.0
        return m
    if cls == "ties":  # quantised, signed; the zeros of either sign
        m = (np.round(rng.normal(0, 0.5, (n, H, W)) * 4) / 4).astype(F32)
        m[(m == 0) & (rng.random((n, H, W)) < 0.5)] = -0.0
        m[rng.random(n) < 0.25] *= F32(0.0)  # maps of +-0.0 only
        return m
    m = np.zeros((n, H, W), F32)
    for i in range(n):
        y0, y1, x0, x1 = rectangle(place, H, W, rng)
        h, w = y1 - y0 + 1, x1 - x0 + 1
        if cls == "sparse_mixed":
            m[i, y0:y1 + 1, x0:x1 + 1] = rng.normal(0, 0.5, (h, w))
        elif cls == "sparse_neg":  # nothing inside the convolved box is positive: the first zero outside it must win
            m[i, y0:y1 + 1, x0:x1 + 1] = -rng.uniform(0.1, 1.0, (h, w))
        elif cls == "sparse_cancel":  # +-2^e two columns apart in ONE row: the column between them convolves to exactly +0.0
            a, y, x = F32(2.0) ** int(rng.integers(-6, 3)), int(rng.integers(y0, y1 + 1)), int(rng.integers(x0, x1 - 1))
            m[i, y, x], m[i, y, x + 2] = (a, -a) if rng.random() < 0.5 else (-a, a)
        elif cls == "cancel_rows":  # such pairs in every second row: the residues of one row's terms meet the next pair's in the column pass
            for y in range(y0, y1 + 1, 2):
                a = F32(2.0) ** int(rng.integers(-6, 3))
                m[i, y, x0], m[i, y, x0 + 2] = (a, -a) if rng.random() < 0.5 else (-a, a)
        elif cls == "single_neg":
            m[i, rng.choice([y0, y1]), rng.choice([x0, x1])] = -rng.uniform(0.1, 1.0)
        else:
            raise ValueError(cls)
    return m


@functools.lru_cache(maxsize=6)
def _expmax_data(cid, seed=None):
    c = expmax_table()[cid]
    rng = np.random.default_rng(c["seed"] if seed is None else seed)
    B, K, H, W = c["B"], c["K"], c["H"], c["W"]
    flip = c["flip"] != "none"
    fl = FD.random_involution(rng, K)
    base = c["cls"] if c["cls"] != "poison" else "dense"
    x = raw_maps(base, rng, B * K, H, W, c["place"]).reshape(B, K, H, W)
    xf = None
    if flip:
        if base in EXPMAX_SPARSE + ("single_neg",):
            xf = np.empty_like(x)
            xf[:, fl] = x[..., ::-1]
        else:
            xf = raw_maps(base, rng, B * K, H, W, c["place"]).reshape(B, K, H, W)
    x_clean, xf_clean = x.copy(), None if xf is None else xf.copy()
    if c["cls"] == "poison":
        for b in range(B):
            k = int(rng.integers(0, K))
            v = F32(rng.choice([np.inf, -np.inf, np.nan]))
            y, xx = int(rng.integers(0, H)), int(rng.integers(0, W))
            if flip and b % 2:
                xf[b, fl[k], y, xx] = v
            else:
                x[b, k, y, xx] = v
    bad = ~np.isfinite(x).reshape(B, K, -1).all(-1)
    if flip:
        bad |= ~np.isfinite(xf).reshape(B, K, -1).all(-1)[:, fl]
    for a in (x, xf, x_clean, xf_clean):
        if a is not None:
            a.setflags(write=False)
    return dict(x=x, xf=xf, x_clean=x_clean, xf_clean=xf_clean, fl=fl, cls=np.full((B, K), c["cls"], dtype=object), bad=bad)


def case_data(case):
    """The inputs of a table case; a copy of a case with "reseed" set draws the same case from that seed (the tables are never written)."""
    return (_argmax_data if case["kind"] == "argmax" else _expmax_data)(case["id"], case.get("reseed"))


def input_size(case):
    return 4 * case["W"], 4 * case["H"]


# ----------------------------------------------------------------------------------------------------- references (numpy)
def argmax_map64(case, d=None, shift=None):
    """The fp64 averaged map of an argmax case and its (B, K) bound. ``shift``: FAULT - override the case's shift."""
    d = d or case_data(case)
    T, nz, flip = case["T"], case["normalize"], case["flip"] != "none"
    shift = (case["flip"] == "shift") if shift is None else shift
    with np.errstate(invalid="ignore", over="ignore"):
        a = FD.probs64(np.where(np.isfinite(d["x"]), d["x"], 0), T, nz)
        ref = FD.merge64(a, FD.probs64(np.where(np.isfinite(d["xf"]), d["xf"], 0), T, nz), d["fl"], shift) if flip else a
        bound = FD.map_bound(d["x_clean"], d["xf_clean"] if flip else None, d["fl"], T, nz, FD.nv_bucket(case["H"], case["W"]))
    return ref, bound


def _decodable(avg_b, bad_b):
    """One sample's maps for udp_ref.decode_f64: a poisoned (NaN) map is replaced by a constant one (its results are not compared, and no
    clean map of the table reads it as a neighbour)."""
    return np.where(bad_b[:, None, None], F32(0.5), avg_b).astype(F32)


def reference_outputs(case):
    """Reference-made outputs of an admitted case, in the layout ``run_*_case`` returns (the CPU test feeds them to the checkers)."""
    d = case_data(case)
    B, K, H, W = d["x"].shape
    bad = d["bad"]
    if case["kind"] == "argmax":
        avg = argmax_map64(case, d)[0].astype(F32)
        if case["normalize"] is None:  # (the fp32 identity is the reference of this mode)
            avg = none_map32(d["x"], d["xf"] if case["flip"] != "none" else None, d["fl"], case["T"], case["flip"] == "shift").copy()
        locs, kp, sc = np.empty((B, K, 2), F32), np.empty((B, K, 2)), np.empty((B, K), F32)
        for b in range(B):
            ref = R.decode_f64(_decodable(avg[b], bad[b]), case["ks"], input_size(case))
            locs[b], kp[b], sc[b] = ref["locs"], ref["keypoints"], ref["scores"]
        main = dict(avg=avg, locs=locs, keypoints=kp, scores=sc)
    else:
        flip = case["flip"] != "none"
        with np.errstate(invalid="ignore"):
            avg = D.tta_average(d["x"], d["xf"], d["fl"], shift_heatmap=case["flip"] == "shift") if flip else d["x"].copy()
        main = dict(avg=avg, **expmax_oracle(avg, bad, input_size(case)))
    for v in main.values():
        v[bad] = np.nan
    return dict(status=OK, main=main)


def expmax_oracle(avg, bad, size):
    """oracle/decode_ref.py on (B, K, H, W) averaged maps -> conv, locs, keypoints, scores (poisoned maps are decoded as zeros, not compared)."""
    B, K, H, W = avg.shape
    conv, locs, kp, sc = np.empty_like(avg), np.empty((B, K, 2), F32), np.empty((B, K, 2)), np.empty((B, K), F32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for b in range(B):
            m = np.where(bad[b][:, None, None], F32(0), avg[b]).astype(F32)
            locs[b], sc[b], conv[b] = D.heatmap_expected_value(m, return_conv=True)
            kp[b] = (locs[b][None] / [W - 1, H - 1] * list(size))[0]
    return dict(conv=conv, locs=locs, keypoints=kp, scores=sc)


def conv64(m, kern):
    """oracle/decode_ref.py::convolve_symmetric_f64 before its rounding: the raster sum in fp64 (the CPU test pins the two against each other)."""
    H, W = m.shape
    d = kern.shape[0]
    pad = np.pad(np.asarray(m, np.float64), d // 2, mode="symmetric")
    acc = np.zeros((H, W), np.float64)
    for i in range(d):
        for j in range(d):
            acc += pad[i:i + H, j:j + W] * kern[i, j]
    return acc


def cancel_bound(m, kern):
    """E of the module docstring, per pixel: (d^2 + 2 d + 130) 2^-53 times the convolution of |m|."""
    d = kern.shape[0]
    return (d * d + 2 * d + 2 + SEPARABLE_ULPS) * 2.0 ** -53 * conv64(np.abs(np.asarray(m, np.float64)), kern)


def decode_from_conv(avg, conv, size):
    """The oracle's steps behind its convolution, on given (K, H, W) convolved maps: first-occurrence argmax, sub-pixel step, rescale."""
    K, H, W = conv.shape
    flat = np.argmax(conv.reshape(K, -1), axis=1)
    locs = np.stack([flat % W, flat // W], -1).astype(F32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        locs = D.subpixel_refine(conv, locs)
    return dict(locs=locs, keypoints=(locs[None] / [W - 1, H - 1] * list(size))[0], scores=avg.reshape(K, -1)[np.arange(K), flat], flat=flat)


def check_cancel_rows(case, main, lab):
    """The derived check of class "cancel_rows" (module docstring). -> the number of maps whose conv_out is not the oracle's bits."""
    d = case_data(case)
    B, K, H, W = d["x"].shape
    kern, differ = D.oks_kernels(K, H, W), 0
    for b in range(B):
        own = decode_from_conv(main["avg"][b], main["conv"][b], input_size(case))
        for n in ("locs", "keypoints", "scores"):
            assert _same(main[n][b], own[n]), f"{lab}: sample {b}: {n} is not the oracle's decode of the kernel's own conv_out"
        for k in range(K):
            c, E = conv64(main["avg"][b, k], kern[k]), cancel_bound(main["avg"][b, k], kern[k])
            got = main["conv"][b, k].astype(np.float64)
            lo, hi = (c - E).astype(F32).astype(np.float64), (c + E).astype(F32).astype(np.float64)
            bad = (got < lo) | (got > hi)
            assert not bad.any(), (f"{lab}: conv_out ({b}, {k}) outside [fl32(c - E), fl32(c + E)] at {np.argwhere(bad)[0].tolist()}: "
                                   f"{got[bad][0]!r} against {c[bad][0]!r} +- {E[bad][0]:.3e}")
            differ += int(not _same(main["conv"][b, k], c.astype(F32)))
            won = int(own["flat"][k])
            gap = float(c.max() - c.flat[won])
            tie = 2 * float(E.max()) + 2.0 ** -23 * float(np.abs(c).max())
            assert gap <= tie, f"{lab}: ({b}, {k}): the kernel's argmax {won} is {gap:.3e} below the oracle's maximum, more than its rounding {tie:.3e}"
    return differ


# ----------------------------------------------------------------------------------------------------- checkers (numpy only)
def new_stats():
    return {}


def _stat(stats, cls):
    return stats.setdefault(str(cls), dict(compared=0, left_out=0, kp_ratio=0.0, map_ratio=0.0))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _same(a, b, rows=None):
    if a.shape != b.shape:
        return False
    a, b = _bits(a), _bits(b)
    return bool(np.array_equal(a, b) if rows is None else np.array_equal(a[rows], b[rows]))


def _label(case):
    keys = ("kind", "id", "group", "H", "W", "B", "K", "ks", "T", "normalize", "flip", "phased", "cls", "place", "neg_at")
    return ", ".join(f"{k} {case[k]}" for k in keys if k in case and case[k] is not None)


def _check_common(case, out, names):
    """Refusals; and what both kernels share: a repeat launch, the lean launch, the planar layout, the poison-free launch."""
    lab = _label(case)
    if case["refused"] is not None:
        status, word = case["refused"]
        assert out["status"] == status and word in out["error"], f"{lab}: expected {status} '{word}', got {out['status']} '{out.get('error')}'"
        assert out["untouched"], f"{lab}: a refused call wrote an output"
        return False
    assert out["status"] == OK, f"{lab}: refused ({out['status']}: {out.get('error')}), the restated check admits it"
    main, bad = out["main"], case_data(case)["bad"]
    for n in names:
        assert np.isnan(main[n][bad]).all(), f"{lab}: {n} of a poisoned (b, k) is not NaN"
        assert not np.isnan(main[n][~bad]).any(), f"{lab}: NaN in {n} of a clean (b, k)"
    for other, which in (("repeat", names), ("lean", ("locs", "keypoints", "scores")), ("planar", names)):
        if other in out:
            for n in which:
                assert _same(out[other][n], main[n]), f"{lab}: {n} of the {other} launch differs"
    if "clean" in out:
        for n in names:
            assert _same(out["clean"][n], main[n], ~bad), f"{lab}: poison leaks into a clean (b, k) through {n}"
    return True


def udp_refusal(H, W, ks):
    """pp_udp_heatmap_decode's shape checks (row-major maps, B >= 1)."""
    if H * W > MAX_PIXELS:
        return UNSUPPORTED, "12288"
    r = (ks - 1) // 2
    if 4 * (64 + H * ((W + 2 * r) | 1) + (H + 2 * r) * W) > LDS_BYTES - STATIC_LDS:
        return UNSUPPORTED, "LDS"
    return None


def chain_expected(case):
    """Both launches of the chain admit the case (pp_probmap_decode_flags has the shape checks of pp_expmax_heatmap_decode), and it has no
    poison (the chain's NaN payloads are not compared)."""
    return (case["refused"] is None and expmax_refused(case["H"], case["W"], 1, case["phased"]) is None
            and udp_refusal(case["H"], case["W"], case["ks"]) is None and not case_data(case)["bad"].any())


def check_argmax(case, out, stats=None, need_chain=False):
    """``out``: what ``run_argmax_case`` returns (numpy). Raises AssertionError; ``stats``: per class compared / left out / worst ratios."""
    stats = new_stats() if stats is None else stats
    if not _check_common(case, out, ("avg", "locs", "keypoints", "scores")):
        return stats
    lab, d = _label(case), case_data(case)
    B, K, H, W = d["x"].shape
    main, bad, cls = out["main"], d["bad"], d["cls"]
    avg, ok = main["avg"], ~d["bad"]
    flip, shift = case["flip"] != "none", case["flip"] == "shift"
    # ---- the averaged map against fp64
    ref, bound = argmax_map64(case, d)
    err = np.abs(avg.astype(np.float64) - ref).reshape(B, K, -1).max(-1)
    for b, k in zip(*np.nonzero(ok)):
        st = _stat(stats, cls[b, k])
        st["map_ratio"] = max(st["map_ratio"], float(err[b, k] / bound[b, k]))
        assert err[b, k] <= bound[b, k], f"{lab}: avg_out ({b}, {k}) [{cls[b, k]}] off by {err[b, k]:.3e} > bound {bound[b, k]:.3e}"
    if case["normalize"] is None:
        want = none_map32(d["x"], d["xf"] if flip else None, d["fl"], case["T"], shift)
        assert (avg[ok] == want[ok]).all(), f"{lab}: normalize None: avg_out != clamp(fl32(x / T), 0, 1) merged in fp32"
    # ---- locs / scores: numpy on the kernel's own map; keypoints: the fp64 DARK decode of it
    scale = np.asarray(input_size(case), np.float64) / [W - 1, H - 1]
    for b in range(B):
        ref = R.decode_f64(_decodable(avg[b], bad[b]), case["ks"], input_size(case))
        k_ok = ok[b]
        assert _same(main["locs"][b], ref["locs"], k_ok), f"{lab}: sample {b}: locs {main['locs'][b].tolist()} != {ref['locs'].tolist()}"
        assert _same(main["scores"][b], ref["scores"], k_ok), f"{lab}: sample {b}: scores are not the map's maxima"
        e = (np.abs(main["keypoints"][b] - ref["keypoints"]) / scale).max(-1)  # heatmap pixels
        for k in np.nonzero(k_ok)[0]:
            st = _stat(stats, cls[b, k])
            if not ref["cond"][k] < 100:
                st["left_out"] += 1
                if case["normalize"] is None:  # (avg_out is exact in this mode: the GPU leaves out what the reference does, to the keypoint)
                    stats["#left out under normalize None"] = stats.get("#left out under normalize None", 0) + 1
                continue
            st["compared"] += 1
            bd = float(ref["bound"][k])
            st["kp_ratio"] = max(st["kp_ratio"], float(e[k]) / bd if bd > 0 else (0.0 if e[k] == 0 else np.inf))
            assert e[k] <= bd, (f"{lab}: sample {b} keypoint {k} [{cls[b, k]}]: |gpu - fp64| = {e[k]:.3e} heatmap px > bound {bd:.3e} "
                                f"(cond {ref['cond'][k]:.1f}, step {ref['step'][k].tolist()})")
    if need_chain:
        assert ("chain" in out) == chain_expected(case), f"{lab}: chain compared {'chain' in out}, the restated checks say {chain_expected(case)}"
    if "chain" in out:  # pp_probmap_decode_flags(LOGITS | flags) then pp_udp_heatmap_decode: the same bits
        stats["#cases compared with the chain"] = stats.get("#cases compared with the chain", 0) + 1
        for n in ("avg", "locs", "keypoints", "scores"):
            assert _same(out["chain"][n], main[n]), f"{lab}: {n} differs from the two launches chained"
    return stats


def check_expmax(case, out, stats=None):
    stats = new_stats() if stats is None else stats
    if not _check_common(case, out, ("avg", "conv", "locs", "keypoints", "scores")):
        return stats
    lab, d = _label(case), case_data(case)
    main, bad, ok = out["main"], d["bad"], ~d["bad"]
    flip = case["flip"] != "none"
    with np.errstate(invalid="ignore"):
        want = D.tta_average(d["x"], d["xf"], d["fl"], shift_heatmap=case["flip"] == "shift") if flip else d["x"]
    assert _same(main["avg"], want, ok), f"{lab}: avg_out is not the {'fp32 flip average' if flip else 'input'} bit for bit"
    if case["cls"] == "cancel_rows":
        assert not bad.any()
        st = _stat(stats, case["cls"])
        st["compared"] += int(ok.sum())
        st["left_out"] += check_cancel_rows(case, main, lab)  # (this class's count of maps whose conv_out is within E, not equal)
        orc = None
    else:
        orc = expmax_oracle(main["avg"], bad, input_size(case))
    for n in ("conv", "locs", "keypoints", "scores") if orc else ():
        if not _same(main[n], orc[n], ok):
            g, w = main[n][ok], orc[n][ok]
            where = np.argwhere(_bits(g) != _bits(w))
            raise AssertionError(f"{lab}: {n} differs from the oracle at {len(where)} places, first {where[0].tolist()}: "
                                 f"{g[tuple(where[0])]!r} != {w[tuple(where[0])]!r}")
    if "flags" in out:  # pp_probmap_decode_flags on the same row-major maps
        for n in ("avg", "conv", "locs", "keypoints", "scores"):
            assert _same(out["flags"][n], main[n], ok), f"{lab}: {n} differs from pp_probmap_decode_flags"
    if orc:
        _stat(stats, case["cls"])["compared"] += int(ok.sum())
    return stats


def blob_cap(stats, cls="blob"):
    """-> (compared, left out, share left out) of the blob class."""
    st = stats.get(cls, dict(compared=0, left_out=0))
    n = st["compared"] + st["left_out"]
    return st["compared"], st["left_out"], st["left_out"] / max(1, n)


def report(stats, title=""):
    lines = [title] if title else []
    for cls, st in sorted(stats.items()):
        if cls.startswith("#"):
            lines.append(f"{cls[1:]}: {st}")
            continue
        if cls == "cancel_rows":
            lines.append(f"{cls:14s} maps {st['compared']:6d}  of them with conv_out within the derived bound, not the oracle's bits: {st['left_out']}")
            continue
        n = st["compared"] + st["left_out"]
        lines.append(f"{cls:14s} compared {st['compared']:6d}  left out (cond >= 100) {st['left_out']:5d} = {100.0 * st['left_out'] / max(1, n):5.2f} %  "
                     f"worst map error / bound {st['map_ratio']:.3f}  worst keypoint error / bound {st['kp_ratio']:.3f}")
    return "\n".join(lines)


def merge_stats(into, other):
    for cls, st in other.items():
        if cls.startswith("#"):
            into[cls] = into.get(cls, 0) + st
            continue
        t = _stat(into, cls)
        t["compared"] += st["compared"]
        t["left_out"] += st["left_out"]
        t["kp_ratio"], t["map_ratio"] = max(t["kp_ratio"], st["kp_ratio"]), max(t["map_ratio"], st["map_ratio"])
    return into


# ----------------------------------------------------------------------------------------------------- GPU side
class Guarded:
    """An output buffer between two canary runs (the style of tests/fuzz_udp_decode.py)."""

    def __init__(self, shape, dtype):
        import torch

        self.n, self.shape = int(np.prod(shape)), tuple(shape)
        self.raw = torch.full((self.n + 2 * GUARD,), FILL, dtype=dtype, device="cuda")

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD * self.raw.element_size()

    def untouched(self):
        return bool((self.raw == FILL).all())

    def get(self):
        r = self.raw.cpu().numpy()
        assert (r[:GUARD] == FILL).all() and (r[GUARD + self.n:] == FILL).all(), "a canary around an output was overwritten"
        return r[GUARD:GUARD + self.n].reshape(self.shape).copy()


def _status_name(st):
    from probpose_code_amd import _lib

    names = {_lib.PP_OK: OK, _lib.PP_ERR_INVALID_ARG: INVALID_ARG, _lib.PP_ERR_UNSUPPORTED: UNSUPPORTED}
    if st not in names:  # a HIP error is no refusal
        raise RuntimeError(f"status {st}: {_lib.last_error()}")
    return names[st]


def _device_inputs(x, xf, fl, phased):
    import torch

    lay = FD.to_phased if phased and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 else np.array  # (a shape PHASED refuses is not read)
    hx = lay(x).reshape(x.shape)
    hf = None if xf is None else lay(xf).reshape(x.shape)
    tx = torch.from_numpy(hx).cuda()
    tf = None if xf is None else torch.from_numpy(hf).cuda()
    fi = None if xf is None else torch.tensor(list(fl), dtype=torch.int32, device="cuda")
    return (hx, hf), (tx, tf, fi)


def _finish(st, outs, host, dev):
    """-> the launch's result dict; the canaries and the inputs are checked here (they need the device)."""
    import torch
    from probpose_code_amd import _lib

    torch.cuda.synchronize()
    if st != _lib.PP_OK:
        return dict(status=_status_name(st), error=_lib.last_error(), untouched=all(g.untouched() for g in outs.values()))
    res = {k: g.get() for k, g in outs.items()}
    for h, t in zip(host, dev):
        if h is not None:
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(h)), "an input was written"
    res["status"] = OK
    return res


def _outputs(B, K, H, W, avg, conv):
    import torch

    o = dict(locs=Guarded((B, K, 2), torch.float32), keypoints=Guarded((B, K, 2), torch.float64), scores=Guarded((B, K), torch.float32))
    if avg:
        o["avg"] = Guarded((B, K, H, W), torch.float32)
    if conv:
        o["conv"] = Guarded((B, K, H, W), torch.float32)
    return o


def _p(o, k):
    return o[k].ptr if k in o else None


def launch_argmax(x, xf, fl, ks, T, normalize, phased=False, shift=False, want_avg=True):
    """x, xf: (B, K, H, W) planar fp32 numpy (xf None: no flipped pass), fed in the phase-separated layout when ``phased``."""
    from probpose_code_amd import _lib

    B, K, H, W = x.shape
    host, (tx, tf, fi) = _device_inputs(x, xf, fl, phased)
    o = _outputs(B, K, H, W, want_avg, False)
    st = _lib.lib.pp_argmax_probmap_decode(tx.data_ptr(), _lib.ptr(tf), _lib.ptr(fi), B, K, H, W, 4.0 * W, 4.0 * H, float(T),
                                           -1.0 if normalize is None else float(normalize), int(ks), _p(o, "avg"), _p(o, "locs"),
                                           _p(o, "keypoints"), _p(o, "scores"), (PHASED if phased else 0) | (SHIFT if shift else 0), None)
    return _finish(int(st), o, host, (tx, tf))


def _taps(K, H, W):
    import torch
    from probpose_code_amd.codecs import oks_kernel_taps

    taps, radius = oks_kernel_taps(min(K, 17), H, W)
    return torch.from_numpy(taps).cuda(), torch.from_numpy(radius).cuda()


def launch_expmax(x, xf, fl, phased=False, shift=False, want_maps=True, K=None):
    from probpose_code_amd import _lib

    B, Kx, H, W = x.shape
    K = K or Kx
    host, (tx, tf, fi) = _device_inputs(x, xf, fl, phased)
    taps, radius = _taps(K, H, W)
    o = _outputs(B, K, H, W, want_maps, want_maps)
    st = _lib.lib.pp_expmax_heatmap_decode(tx.data_ptr(), _lib.ptr(tf), _lib.ptr(fi), taps.data_ptr(), radius.data_ptr(), B, K, H, W, 4.0 * W,
                                           4.0 * H, _p(o, "avg"), _p(o, "conv"), _p(o, "locs"), _p(o, "keypoints"), _p(o, "scores"),
                                           (PHASED if phased else 0) | (SHIFT if shift else 0), None)
    return _finish(int(st), o, host, (tx, tf))


def launch_flags(x, xf, fl, T, normalize, flags, conv=False):
    """pp_probmap_decode_flags on planar inputs (``flags`` says what they are)."""
    from probpose_code_amd import _lib

    B, K, H, W = x.shape
    host, (tx, tf, fi) = _device_inputs(x, xf, fl, bool(flags & PHASED))
    taps, radius = _taps(K, H, W)
    o = _outputs(B, K, H, W, True, conv)
    st = _lib.lib.pp_probmap_decode_flags(tx.data_ptr(), _lib.ptr(tf), _lib.ptr(fi), taps.data_ptr(), radius.data_ptr(), B, K, H, W, 4.0 * W,
                                          4.0 * H, float(T), -1.0 if normalize is None else float(normalize), _p(o, "avg"), _p(o, "conv"),
                                          _p(o, "locs"), _p(o, "keypoints"), _p(o, "scores"), int(flags), None)
    return _finish(int(st), o, host, (tx, tf))


def launch_udp(maps, ks):
    import torch
    from probpose_code_amd import _lib

    B, K, H, W = maps.shape
    t = torch.from_numpy(np.ascontiguousarray(maps)).cuda()
    o = _outputs(B, K, H, W, False, False)
    st = _lib.lib.pp_udp_heatmap_decode(t.data_ptr(), None, None, B, K, H, W, 4.0 * W, 4.0 * H, int(ks), None, _p(o, "locs"), _p(o, "keypoints"),
                                        _p(o, "scores"), 0, None)
    return _finish(int(st), o, (maps,), (t,))


def run_argmax_case(case):
    """Every launch of one argmax case -> the dict ``check_argmax`` takes."""
    d = case_data(case)
    flip, shift, ph = case["flip"] != "none", case["flip"] == "shift", case["phased"]
    xf = d["xf"] if flip else None
    args = (d["fl"], case["ks"], case["T"], case["normalize"])
    main = launch_argmax(d["x"], xf, *args, ph, shift)
    if main["status"] != OK:
        return main
    out = dict(status=OK, main=main, repeat=launch_argmax(d["x"], xf, *args, ph, shift), lean=launch_argmax(d["x"], xf, *args, ph, shift, False))
    if ph:
        out["planar"] = launch_argmax(d["x"], xf, *args, False, shift)
    if d["bad"].any():
        out["clean"] = launch_argmax(d["x_clean"], d["xf_clean"] if flip else None, *args, ph, shift)
    # the chain, where both of its launches admit the shape
    flags = LOGITS | (PHASED if ph else 0) | (SHIFT if shift else 0)
    first = launch_flags(d["x"], xf, d["fl"], case["T"], case["normalize"], flags)
    if first["status"] == OK and not d["bad"].any():
        second = launch_udp(first["avg"], case["ks"])
        if second["status"] == OK:
            out["chain"] = dict(second, avg=first["avg"])
    for k, v in out.items():
        assert k == "status" or v["status"] == OK, (k, v)
    return out


def run_expmax_case(case):
    d = case_data(case)
    flip, shift, ph = case["flip"] != "none", case["flip"] == "shift", case["phased"]
    xf = d["xf"] if flip else None
    main = launch_expmax(d["x"], xf, d["fl"], ph, shift)
    if main["status"] != OK:
        return main
    out = dict(status=OK, main=main, repeat=launch_expmax(d["x"], xf, d["fl"], ph, shift), lean=launch_expmax(d["x"], xf, d["fl"], ph, shift, False))
    if ph:
        out["planar"] = launch_expmax(d["x"], xf, d["fl"], False, shift)
    if d["bad"].any():
        out["clean"] = launch_expmax(d["x_clean"], d["xf_clean"] if flip else None, d["fl"], ph, shift)
    out["flags"] = launch_flags(d["x"], xf, d["fl"], 1.0, 1.0, SHIFT if shift else 0, conv=True)
    for k, v in out.items():
        assert k == "status" or v["status"] == OK, (k, v)
    return out


def run_case(case, stats=None):
    if case["kind"] == "argmax":
        return check_argmax(case, run_argmax_case(case), stats, need_chain=True)
    return check_expmax(case, run_expmax_case(case), stats)


def run_group(kind, groups):
    """The table's cases of these groups -> (cases run, stats)."""
    stats, n = new_stats(), 0
    for case in (argmax_table() if kind == "argmax" else expmax_table()):
        if case["group"] in groups:
            run_case(case, stats)
            n += 1
    return n, stats


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
    for kind, table in (("argmax", argmax_table()), ("expmax", expmax_table())):
        stats = new_stats()
        for case in table:
            run_case(case, stats)
        print(report(stats, f"{kind}: {len(table)} table cases"))
        if kind == "argmax":
            cmp_, out, share = blob_cap(stats)
            assert cmp_ >= BLOB_MIN and share <= BLOB_CAP, (cmp_, out, share)
    # random cases after the table: the table's generators at fresh seeds (the tables themselves never change)
    t_end, n, stats = time.time() + seconds, 0, new_stats()
    tables = argmax_table() + expmax_table()
    while time.time() < t_end:
        rng = np.random.default_rng(930000 + n)
        run_case(dict(tables[int(rng.integers(0, len(tables)))], reseed=930000 + n), stats)
        n += 1
    if n:
        print(report(stats, f"{n} random cases"))
    print("CODEC SWAP FUZZ OK")


if __name__ == "__main__":
    main()
