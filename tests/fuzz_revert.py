#!/usr/bin/env python
"""Differential fuzz of the "heatmaps back on the image" kernels of pp_warp.hip, called through the C ABI with raw pointers.

pp_revert_heatmaps_max against oracle/warp_ref.py itself (np.max over revert_heatmap: cv2's float warpAffine restated, float32 products
summed left to right), bit for bit - ``np.array_equal(got, want, equal_nan=True)``, no tolerance: the weights are exact in float32 and both
sides do the same four multiplies and three adds in the same order. Image sizes either side of the 256-thread row block, map sizes down to
1 x 1, K in {1, 2, 17, 31, 32}, 1 - 6 persons, windows inside / over each edge / wholly outside / ten times the image / slivers under a
pixel / the padded-image form of merge_data_samples; blobs, maps with negative entries (the 0 of an out-of-window person must win), all-negative
maps, and in a share of the cases a NaN, +inf or -inf at a random tap. Finite nonzero magnitudes stay within [2^-60, 2^60], so no check
depends on the subnormal flush mode.

pp_heatmap_posterior against fp64: want = hm / sum64(hm) * mean64(presence), |got - want| <= (n + 4) 2^-24 |want| per element - one rounding
each for the total's cast to float32, the divide and the multiply, at most n for the float32 mean of n presences, one spare. H * W makes the 64
partial ranges empty, exactly full and ragged.

Every output sits between two canary stretches (compared bit for bit) and is prefilled with a NaN payload no kernel writes: every element
must have been overwritten. Inputs are bit-identical after the launch, a repeat launch is bit-identical. A HIP error (or a touched canary)
ends the script at once; a mismatch is printed and counted.   python tests/fuzz_revert.py [seconds]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import warp_ref  # noqa: E402

GUARD = 256  # canary elements either side of an output
CANARY32, UNWRITTEN32 = 0x4B1DF00D, 0x7FC5A5A5  # a finite float32 pattern; a quiet NaN with a payload no arithmetic produces
CANARY64, UNWRITTEN64 = 0x4B1DF00D4B1DF00D, 0x7FF85A5A5A5A5A5A
U = 2.0 ** -24  # unit roundoff of float32

IMAGES = [(1, 1), (7, 5), (37, 53), (64, 255), (64, 256), (64, 257), (240, 320), (300, 513)]
MAPS = [(64, 48), (16, 12), (3, 2), (1, 1)]
KS = [1, 2, 17, 31, 32]
WINDOWS = ["inside", "left", "top", "right", "bottom", "outside", "huge", "sliver", "padded"]
VALUES = ["blobs", "mixed", "negative", "wide"]
POST_KS = [1, 17, 40]
POST_HW = [1, 63, 64, 65, 64 * 256 - 1, 64 * 256, 64 * 256 + 1, 270 * 360 + 7]


class GuardError(RuntimeError):
    """A kernel wrote outside its output: nothing more is launched."""


class Guarded:
    """A device buffer of 4- or 8-byte elements between two canary runs, prefilled with the "unwritten" NaN payload."""

    def __init__(self, n, itemsize, dev):
        import torch

        self.n = n
        self.np_int, self.canary, self.unwritten = (np.int32, CANARY32, UNWRITTEN32) if itemsize == 4 else (np.int64, CANARY64, UNWRITTEN64)
        host = np.full(n + 2 * GUARD, self.canary, self.np_int)
        host[GUARD:GUARD + n] = self.unwritten
        self.raw = torch.from_numpy(host).to(dev)
        self.itemsize = itemsize

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD * self.itemsize

    def set(self, values):  # values: numpy array of n elements of the same width
        import torch

        self.raw[GUARD:GUARD + self.n] = torch.from_numpy(np.ascontiguousarray(values).reshape(-1).view(self.np_int)).to(self.raw.device)

    def get(self, dtype, what, require_written=True):
        r = self.raw.cpu().numpy()
        if not ((r[:GUARD] == self.canary).all() and (r[GUARD + self.n:] == self.canary).all()):
            raise GuardError(f"{what}: canary overwritten")
        body = r[GUARD:GUARD + self.n].copy()
        if require_written:
            left = int((body == self.unwritten).sum())
            assert left == 0, f"{what}: {left} of {self.n} elements never written"
        return body.view(dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


# ------------------------------------------------------------------------------------------------------------------- revert
def inverse_map(center, scale, hm_wh):
    """The dst -> src map the kernel is handed for one person: what cv2.warpAffine derives from revert_heatmap's matrix."""
    return warp_ref.invert_affine(warp_ref.get_warp_matrix(np.asarray(center, np.float64), np.asarray(scale, np.float64), 0, hm_wh, inv=True))


def in_domain(inv, H, W):
    """The 10-fractional-bit coordinates stay far inside int32 (cv2 wraps beyond it; neither side of this fuzz goes there)."""
    m = np.abs(np.asarray(inv, np.float64))
    big = max((m[0, 1] * H + m[0, 2]), (m[1, 1] * H + m[1, 2]), m[0, 0] * W, m[1, 0] * W)
    return np.isfinite(big) and big * 1024.0 < 2.0 ** 30


def draw_window(rng, kind, H, W, h, w):
    """Centre and scale of one person's window on an (H, W) image for an (h, w) map. The window is scale[0] wide and
    scale[0] * h / w high (the reverted warp takes its size from the width alone, as the reference's does)."""
    asp = h / w
    fit = min(W, H / asp)  # the widest window that still fits
    cx, cy = rng.uniform(0, W), rng.uniform(0, H)
    s = rng.uniform(0.2, 1.0) * fit
    if kind == "inside":
        s = rng.uniform(0.1, 0.9) * fit
        cx, cy = rng.uniform(s / 2, W - s / 2), rng.uniform(s * asp / 2, H - s * asp / 2)
    elif kind == "left":
        cx = rng.uniform(-s / 4, s / 4)
    elif kind == "right":
        cx = W + rng.uniform(-s / 4, s / 4)
    elif kind == "top":
        cy = rng.uniform(-s * asp / 4, s * asp / 4)
    elif kind == "bottom":
        cy = H + rng.uniform(-s * asp / 4, s * asp / 4)
    elif kind == "outside":  # more than a pixel away from the image on one side
        side = int(rng.integers(0, 4))
        off = rng.uniform(2.0, 2.0 + fit)
        if side == 0:
            cx = -s / 2 - off
        elif side == 1:
            cx = W + s / 2 + off
        elif side == 2:
            cy = -s * asp / 2 - off
        else:
            cy = H + s * asp / 2 + off
    elif kind == "huge":
        s = 10.0 * max(W, H / asp) * rng.uniform(1.0, 1.5)
    elif kind == "sliver":
        s = rng.uniform(0.05, 1.0)
    elif kind == "padded":  # merge_data_samples: a window over the top-left corner, the image padded until it fits (+10 px)
        cx, cy = rng.uniform(-s / 4, s / 4), rng.uniform(-s * asp / 4, s * asp / 4)
        cx, cy = cx + int(max(s / 2 - cx + 10, 0)), cy + int(max(s * asp / 2 - cy + 10, 0))
    return np.array([cx, cy]), np.array([s, s * asp])


def draw_maps(rng, kind, n, K, h, w):
    """(n, K, h, w) float32; finite nonzero magnitudes within [2^-60, 2^60]."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "wide":
        hm = np.ldexp(rng.uniform(1.0, 2.0, (n, K, h, w)), rng.integers(-60, 60, (n, K, h, w))) * rng.choice([-1.0, 1.0], (n, K, h, w))
        hm[rng.random((n, K, h, w)) < 0.1] = 0.0
    else:
        mu = rng.uniform(-0.2, 1.2, (n, K, 2, 1, 1)) * np.array([h, w]).reshape(1, 1, 2, 1, 1)
        sg = rng.uniform(0.4, 0.25 * max(h, w) + 0.5, (n, K, 1, 1))
        hm = rng.uniform(0.05, 1.0, (n, K, 1, 1)) * np.exp(-((yy - mu[:, :, 0]) ** 2 + (xx - mu[:, :, 1]) ** 2) / (2 * sg * sg))
        if kind == "mixed":
            hm = hm - rng.uniform(0.0, 0.5, (n, K, 1, 1)) + rng.normal(0, 0.05, (n, K, h, w))
        elif kind == "negative":
            hm = -hm - rng.uniform(2.0 ** -20, 1.0, (n, K, 1, 1))
    hm = hm.astype(np.float32)
    hm[np.abs(hm) < 2.0 ** -60] = 0.0
    assert np.isfinite(hm).all() and (np.abs(hm[hm != 0]) >= 2.0 ** -60).all() and (np.abs(hm) <= 2.0 ** 60).all()
    return hm


def revert_case(index):
    """Case ``index``: image and map sizes round robin, everything else drawn from the case's own generator."""
    rng = np.random.default_rng(424200 + index)
    H, W = IMAGES[index % len(IMAGES)]
    h, w = MAPS[(index // len(IMAGES)) % len(MAPS)]
    K, n = int(rng.choice(KS)), int(rng.integers(1, 7))
    centers, scales, kinds = [], [], []
    for _ in range(n):
        while True:
            kind = WINDOWS[int(rng.integers(0, len(WINDOWS)))]
            c, s = draw_window(rng, kind, H, W, h, w)
            if in_domain(inverse_map(c, s, (w, h)), H, W):
                break
        centers.append(c), scales.append(s), kinds.append(kind)
    values = VALUES[int(rng.integers(0, len(VALUES)))]
    hms = draw_maps(rng, values, n, K, h, w)
    special = None
    if rng.random() < 0.35:
        special = [np.nan, np.inf, -np.inf][int(rng.integers(0, 3))]
        hms[int(rng.integers(0, n)), int(rng.integers(0, K)), int(rng.integers(0, h)), int(rng.integers(0, w))] = special
    return dict(hms=hms, centers=np.stack(centers), scales=np.stack(scales), H=H, W=W,
                label=f"revert #{index}: image {H}x{W}, map {h}x{w}, K {K}, n {n}, windows {'/'.join(kinds)}, values {values}, special {special}")


def revert_reference(case):
    """np.max over oracle.warp_ref.revert_heatmap - the reference's merge (structures/utils.py:105-123)."""
    with np.errstate(invalid="ignore"):
        return np.max([warp_ref.revert_heatmap(h, c, s, (case["H"], case["W"])) for h, c, s in zip(case["hms"], case["centers"], case["scales"])],
                      axis=0)


def compare_revert(got, want, label="revert"):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, f"{label}: shape / dtype"
    if not np.array_equal(got, want, equal_nan=True):
        with np.errstate(invalid="ignore"):
            bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        k, y, x = [int(v[0]) for v in np.nonzero(bad)]
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.size} elements differ, first at (k {k}, y {y}, x {x}): got {got[k, y, x]!r}, "
                             f"want {want[k, y, x]!r}")


def launch_revert(hms, invs, H, W, dev="cuda"):
    """One pp_revert_heatmaps_max launch on raw pointers -> the (K, H, W) output; canaries, written-everywhere and the inputs checked."""
    import torch

    from probpose_code_amd import _lib

    n, K, h, w = hms.shape
    invs = np.ascontiguousarray(invs, np.float64).reshape(n, 6)
    t_hm, t_inv = torch.from_numpy(hms).to(dev), torch.from_numpy(invs).to(dev)
    out = Guarded(K * H * W, 4, dev)
    _lib.call("pp_revert_heatmaps_max", t_hm.data_ptr(), t_inv.data_ptr(), out.ptr, n, K, h, w, H, W, _lib.stream_ptr(torch.device(dev)))
    torch.cuda.synchronize()
    got = out.get(np.float32, "revert output").reshape(K, H, W)
    assert np.array_equal(bits(t_hm.cpu().numpy()), bits(hms)) and np.array_equal(bits(t_inv.cpu().numpy()), bits(invs)), "revert: input changed"
    return got


def check_revert(case):
    invs = np.stack([inverse_map(c, s, case["hms"].shape[:1:-1]) for c, s in zip(case["centers"], case["scales"])])
    got = launch_revert(case["hms"], invs, case["H"], case["W"])
    again = launch_revert(case["hms"], invs, case["H"], case["W"])
    assert np.array_equal(bits(got), bits(again)), "revert: a second launch differs"
    compare_revert(got, revert_reference(case), case["label"])


# ---------------------------------------------------------------------------------------------------------------- posterior
def side_lengths(hw):
    """H x W = hw with H the largest divisor not above sqrt(hw): the kernel only sees the product."""
    hgt = max(d for d in range(1, int(hw ** 0.5) + 1) if hw % d == 0)
    return hgt, hw // hgt


def posterior_case(index):
    rng = np.random.default_rng(515100 + index)
    K = POST_KS[index % len(POST_KS)]
    hw = POST_HW[(index // len(POST_KS)) % len(POST_HW)]
    n = int(rng.integers(1, 5))
    expo = rng.integers(-40, 0, (K, hw))  # non-negative, 2^-40 .. 1
    if rng.random() < 0.5:  # posterior-like: most of the mass in a few pixels
        expo = np.where(rng.random((K, hw)) < 0.05, rng.integers(-4, 0, (K, hw)), rng.integers(-40, -12, (K, hw)))
    hm = np.ldexp(rng.uniform(1.0, 2.0, (K, hw)), expo)
    hm[rng.random((K, hw)) < 0.1] = 0.0
    hm[:, int(rng.integers(0, hw))] = rng.uniform(0.5, 1.0, K)  # no all-zero channel: 0 / 0 is a directed test's business
    hm = hm.astype(np.float32)
    for k in np.nonzero(rng.random(K) < 0.4)[0]:  # negative entries, at most a quarter of the positive sum in all
        neg = rng.random(hw) < 0.2
        neg[int(np.argmax(hm[k]))] = False
        pos_sum, neg_sum = float(hm[k][~neg].astype(np.float64).sum()), float(hm[k][neg].astype(np.float64).sum())
        if neg_sum > 0:
            e = 0
            while np.ldexp(neg_sum, e) > 0.25 * pos_sum:
                e -= 1
            hm[k][neg] = -np.ldexp(hm[k][neg], e)
    presence = rng.uniform(2.0 ** -10, 1.0, (n, K)).astype(np.float32)
    presence[rng.random((n, K)) < 0.1] = 1.0
    if n > 1:
        presence[int(rng.integers(0, n)), rng.random(K) < 0.1] = 0.0
    H, W = side_lengths(hw)
    return dict(hm=hm.reshape(K, H, W), presence=presence, label=f"posterior #{index}: K {K}, H*W {hw} = {H}x{W}, n {n}")


def posterior_reference(hm, presence):
    """fp64: (want, bound). total = sum64 of the float32 inputs; want = hm / total * mean64(presence); bound (n + 4) 2^-24 |want|."""
    hm64, pr64 = np.asarray(hm, np.float32).astype(np.float64), np.asarray(presence, np.float32).astype(np.float64)
    n, K = pr64.shape
    pos, neg = np.where(hm64 > 0, hm64, 0).sum(axis=(1, 2)), -np.where(hm64 < 0, hm64, 0).sum(axis=(1, 2))
    assert (neg <= 0.25 * pos).all() and (pos > 0).all(), "posterior inputs: the total must not cancel"
    want = hm64 / hm64.sum(axis=(1, 2), keepdims=True) * pr64.mean(axis=0)[:, None, None]
    assert (np.abs(want[want != 0]) >= 2.0 ** -100).all(), "posterior inputs: a wanted value below 2^-100"
    return want, (n + 4) * U * np.abs(want)


def compare_posterior(got, want, bound, label="posterior"):
    """-> the worst error / bound ratio; raises where an element is outside its bound."""
    assert got.shape == want.shape and got.dtype == np.float32, f"{label}: shape / dtype"
    assert np.isfinite(got).all(), f"{label}: non-finite output from finite inputs"
    err = np.abs(got.astype(np.float64) - want)
    bad = err > bound
    if bad.any():
        k, y, x = [int(v[0]) for v in np.nonzero(bad)]
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.size} elements outside the bound, first at (k {k}, y {y}, x {x}): got "
                             f"{got[k, y, x]!r}, want {want[k, y, x]!r}, error {err[k, y, x]:.3e} > {bound[k, y, x]:.3e}")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def launch_posterior(hm, presence_mean, dev="cuda", return_scratch=False):
    """One pp_heatmap_posterior launch (in place on a guarded copy of ``hm``); the K * 64 scratch doubles sit between canaries and must
    all be written."""
    import torch

    from probpose_code_amd import _lib

    K, H, W = hm.shape
    buf, scratch = Guarded(K * H * W, 4, dev), Guarded(K * 64, 8, dev)
    buf.set(hm)
    t_pr = presence_mean.contiguous()
    before = t_pr.cpu().numpy().copy()
    _lib.call("pp_heatmap_posterior", buf.ptr, t_pr.data_ptr(), scratch.ptr, K, H, W, _lib.stream_ptr(torch.device(dev)))
    torch.cuda.synchronize()
    got = buf.get(np.float32, "posterior maps", require_written=False).reshape(K, H, W)
    parts = scratch.get(np.float64, "posterior scratch").reshape(K, 64)
    assert np.array_equal(bits(t_pr.cpu().numpy()), bits(before)), "posterior: presence changed"
    return (got, parts) if return_scratch else got


def check_posterior(case, dev="cuda"):
    import torch

    hm, presence = case["hm"], case["presence"]
    pr = torch.from_numpy(presence).to(dev).mean(dim=0)  # the float32 mean, as structures.posterior_heatmaps takes it
    got = launch_posterior(hm, pr, dev)
    again = launch_posterior(hm, pr, dev)
    assert np.array_equal(bits(got), bits(again)), "posterior: a repeat on a fresh copy differs"
    want, bound = posterior_reference(hm, presence)
    return compare_posterior(got, want, bound, case["label"])


# --------------------------------------------------------------------------------------------------------------------- main
def run(seconds=60.0, min_cases=4):
    """Revert and posterior cases in turn until the time is up -> (revert cases, posterior cases, mismatches, worst posterior ratio).
    HIP errors and touched canaries are not caught: they end the run."""
    n_rev = n_post = bad = 0
    worst, t_end = 0.0, time.time() + seconds
    while time.time() < t_end or n_rev < min_cases:
        for kind in ("revert", "posterior"):
            try:
                if kind == "revert":
                    check_revert(revert_case(n_rev))
                else:
                    worst = max(worst, check_posterior(posterior_case(n_post)))
            except AssertionError as exc:
                bad += 1
                print(f"MISMATCH {exc}", flush=True)
            if kind == "revert":
                n_rev += 1
            else:
                n_post += 1
    return n_rev, n_post, bad, worst


if __name__ == "__main__":
    secs = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    n_rev, n_post, bad, worst = run(secs)
    print(f"{n_rev} revert cases, {n_post} posterior cases in {secs:.0f} s, {bad} mismatches; worst posterior error / bound {worst:.3f}")
    print("REVERT FUZZ", "FAILED" if bad else "OK")
    sys.exit(1 if bad else 0)
