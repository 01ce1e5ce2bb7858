"""The references and checks of tests/fuzz_revert.py, on the CPU: (a) its references agree with independent forms - the reverted maps with a
direct per-pixel fp64 bilinear interpolation at the fixed-point coordinates, the posterior with oracle.warp_ref.posterior within the stated
bound; (b) its checks reject simulated faulty kernels, emulated in numpy: a merge whose max drops NaN, maxima started at -FLT_MAX, fused
coordinate rounding on a tie row, clamp-to-edge taps where the zero border belongs, an out-of-window person skipped where it contributes 0, a
posterior total accumulated in float32 in index order, a posterior that leaves the last ragged partial range out; (c) the same inputs pass
with the kernels' arithmetic as it should be. No GPU needed: a kernel with one of these faults would fail the fuzzer."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fuzz_revert as FR  # noqa: E402
from oracle import warp_ref  # noqa: E402

FLT_MAX = np.float32(3.402823466e+38)


# ------------------------------------------------------------------------------------------- the kernels, emulated in numpy
def emulate_revert(hms, invs, H, W, keep_nan=True, start=-np.inf, fused=False, clamp_edge=False, skip_outside=False):
    """revert_heatmaps_max_kernel step by step in float32: per person the fixed-point coordinates, the four taps with the zero border, the
    float32 sum left to right, the running maximum. The keyword arguments switch single faults on."""
    n, K, h, w = hms.shape
    acc = np.full((K, H, W), start, np.float32)
    merge = np.maximum if keep_nan else np.fmax  # np.maximum keeps NaN as the kernel must; np.fmax returns the other operand (v_max_f32)
    for b in range(n):
        X, Y = warp_ref.fixed_point_coords(np.asarray(invs[b], np.float64).reshape(2, 3), (W, H), fused)
        sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
        x0, x1, y0, y1 = (sx >= 0) & (sx < w), (sx + 1 >= 0) & (sx + 1 < w), (sy >= 0) & (sy < h), (sy + 1 >= 0) & (sy + 1 < h)
        seen = (x0 | x1) & (y0 | y1)
        ax, ay = (X & 31).astype(np.float32) * np.float32(1 / 32), (Y & 31).astype(np.float32) * np.float32(1 / 32)
        one = np.float32(1)
        w00, w01, w10, w11 = (one - ay) * (one - ax), (one - ay) * ax, ay * (one - ax), ay * ax

        def tap(yy, xx, ok):
            v = hms[b][:, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
            return v if clamp_edge else np.where(ok, v, np.float32(0))

        with np.errstate(invalid="ignore"):
            v = tap(sy, sx, x0 & y0) * w00 + tap(sy, sx + 1, x1 & y0) * w01 + tap(sy + 1, sx, x0 & y1) * w10 + tap(sy + 1, sx + 1, x1 & y1) * w11
            v = np.where(seen, v, np.float32(0)).astype(np.float32)
            acc = np.where(seen | (not skip_outside), merge(acc, v), acc)
    return acc


def emulate_posterior(hm, presence_mean, float32_total=False, drop_last_part=False):
    """channel_partial_sum_kernel + channel_scale_kernel: 64 partial sums in float64 over ceil(HW / 64) elements each, their sum cast to
    float32, hm / total * presence in float32."""
    K, hw = hm.shape[0], hm.shape[1] * hm.shape[2]
    flat = hm.reshape(K, hw)
    per = (hw + 63) // 64
    parts = np.zeros((K, 64))
    for p in range(64):
        lo, hi = p * per, min(p * per + per, hw)
        if lo < hi and not (drop_last_part and hi == hw and hi - lo < per):
            parts[:, p] = flat[:, lo:hi].astype(np.float64).sum(axis=1)
    total = parts.sum(axis=1).astype(np.float32)
    if float32_total:
        total = np.cumsum(flat, axis=1, dtype=np.float32)[:, -1]  # one float32 accumulator, index order
    return (hm / total[:, None, None] * np.asarray(presence_mean, np.float32)[:, None, None]).astype(np.float32)


def _invs(case):
    return np.stack([FR.inverse_map(c, s, case["hms"].shape[:1:-1]) for c, s in zip(case["centers"], case["scales"])])


SMALL = [i for i in range(64) if i % 8 < 6]  # the fuzzer's first cases on the images up to 64 x 257 (cheap on the CPU)


@pytest.fixture(scope="module")
def small_cases():
    out = []
    for i in SMALL:
        case = FR.revert_case(i)
        out.append((case, _invs(case), FR.revert_reference(case)))
    return out


# ------------------------------------------------------------------------------------------------ (a) independent references
def bilinear64(hm, inv, H, W):
    """(value, sum |s_i| w_i) per pixel in fp64: plain bilinear interpolation of the (K, h, w) map at the coordinates X / 32, Y / 32, zero
    outside the map."""
    K, h, w = hm.shape
    X, Y = warp_ref.fixed_point_coords(np.asarray(inv, np.float64).reshape(2, 3), (W, H))
    u, v = X / 32.0, Y / 32.0
    x0, y0 = np.floor(u), np.floor(v)
    fx, fy = u - x0, v - y0
    val, mag = np.zeros((K, H, W)), np.zeros((K, H, W))
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            yy, xx = (y0 + dy).astype(np.int64), (x0 + dx).astype(np.int64)
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            s = np.where(ok, hm.astype(np.float64)[:, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0.0)
            val += s * (wy * wx)
            mag += np.abs(s) * (wy * wx)
    return val, mag


def test_revert_reference_vs_fp64_bilinear(small_cases):
    """np.max over the oracle's float32 warps == max over fp64 bilinear interpolation, within 4 * 2^-24 * sum |s_i| w_i (four float32
    products, three sums; the merged pixel takes the largest bound among its persons). Cases with a NaN / inf tap are left to
    test_emulated_kernel_equals_the_oracle."""
    checked = 0
    for case, invs, want in small_cases:
        H, W = case["H"], case["W"]
        if np.isfinite(case["hms"]).all():
            vals, mags = zip(*[bilinear64(case["hms"][b], invs[b], H, W) for b in range(len(invs))])
            ref, bound = np.max(vals, axis=0), 4 * FR.U * np.max(mags, axis=0)
            assert (np.abs(want - ref) <= bound).all(), case["label"]
            checked += 1
    assert checked >= 30


def test_emulated_kernel_equals_the_oracle(small_cases):
    """(c) The kernel's steps, restated once more (explicit border tests, no padded copy, a running maximum), are the oracle bit for bit on
    the fuzzer's own cases - NaN, infinities, out-of-window persons and all."""
    kinds = set()
    for case, invs, want in small_cases:
        FR.compare_revert(emulate_revert(case["hms"], invs, case["H"], case["W"]), want, case["label"])
        kinds.update(case["label"].split("windows ")[1].split(",")[0].split("/"))
    assert kinds == set(FR.WINDOWS)  # every kind of window is among them


def test_posterior_reference_vs_the_oracle_and_the_emulated_kernel():
    """The fp64 reference against oracle.warp_ref.posterior (float32 numpy, pairwise total) and against the emulated kernel, both within the
    fuzzer's bound, on one case of every H * W."""
    for i in range(0, 24, 3):
        for j in (i, i + 1):  # K = 1 and K = 17
            case = FR.posterior_case(j)
            want, bound = FR.posterior_reference(case["hm"], case["presence"])
            FR.compare_posterior(warp_ref.posterior(case["hm"], case["presence"]), want, bound, "oracle, " + case["label"])
            mean32 = case["presence"].sum(axis=0, dtype=np.float32) / np.float32(len(case["presence"]))
            FR.compare_posterior(emulate_posterior(case["hm"], mean32), want, bound, "emulated, " + case["label"])


# ------------------------------------------------------------------------------------------------------- (b) faulty kernels
def _rejected(small_cases, **fault):
    """The fuzzer cases (labels) whose check rejects the kernel with this fault."""
    hit = []
    for case, invs, want in small_cases:
        try:
            FR.compare_revert(emulate_revert(case["hms"], invs, case["H"], case["W"], **fault), want, case["label"])
        except AssertionError:
            hit.append(case["label"])
    return hit


def test_a_max_that_drops_nan_is_rejected(small_cases):
    hit = _rejected(small_cases, keep_nan=False)
    assert hit and all("special" in h and "special None" not in h for h in hit), hit
    # directed: one NaN tap in the middle of a window inside the image
    rng = np.random.default_rng(1)
    hms = FR.draw_maps(rng, "blobs", 2, 3, 16, 12)
    hms[1, 2, 8, 6] = np.nan
    invs = np.stack([FR.inverse_map([26.0, 18.0], [24.0, 32.0], (12, 16))] * 2)
    want = np.max([warp_ref.warp_affine_f32(h.transpose(1, 2, 0), m, (53, 37), inverse=True).transpose(2, 0, 1) for h, m in zip(hms, invs)], axis=0)
    assert np.isnan(want).sum() >= 4
    FR.compare_revert(emulate_revert(hms, invs, 37, 53), want)
    with pytest.raises(AssertionError, match="differ"):
        FR.compare_revert(emulate_revert(hms, invs, 37, 53, keep_nan=False), want)


def test_maxima_started_at_minus_flt_max_are_rejected():
    """Only a pixel whose every contribution is -inf tells -inf from -FLT_MAX: one person, a -inf tap."""
    rng = np.random.default_rng(2)
    hms = FR.draw_maps(rng, "negative", 1, 2, 16, 12)
    hms[0, 1, 8, 6] = -np.inf
    invs = FR.inverse_map([26.0, 18.0], [24.0, 32.0], (12, 16))[None]
    want = warp_ref.warp_affine_f32(hms[0].transpose(1, 2, 0), invs[0], (53, 37), inverse=True).transpose(2, 0, 1)
    assert (want == -np.inf).sum() >= 4
    FR.compare_revert(emulate_revert(hms, invs, 37, 53), want)
    with pytest.raises(AssertionError, match="differ"):
        FR.compare_revert(emulate_revert(hms, invs, 37, 53, start=-FLT_MAX), want)


def test_fused_coordinate_rounding_is_rejected_on_a_tie_row():
    rng = np.random.default_rng(3)
    M, y = warp_ref.find_tie_row(rng, 37, 16, col_scale=0.2, col_offset=0.3)
    hms = FR.draw_maps(rng, "mixed", 1, 2, 16, 12)
    want = warp_ref.warp_affine_f32(hms[0].transpose(1, 2, 0), M, (53, 37), inverse=True).transpose(2, 0, 1)
    FR.compare_revert(emulate_revert(hms, M[None], 37, 53), want)
    with pytest.raises(AssertionError, match=f"y {y},"):
        FR.compare_revert(emulate_revert(hms, M[None], 37, 53, fused=True), want)
    # (a random window is not on a tie: there the fused rounding passes, which is why the fuzzers carry tie rows)
    inv = FR.inverse_map([26.3, 18.1], [24.7, 32.9], (12, 16))
    assert np.array_equal(emulate_revert(hms, inv[None], 37, 53, fused=True), emulate_revert(hms, inv[None], 37, 53))


def test_clamped_taps_and_skipped_persons_are_rejected(small_cases):
    """A missing zero border (taps clamped to the map's edge) shows wherever a window's rim lies inside the image; a person that is skipped
    outside its window, instead of contributing 0, shows where the other maps are negative (or nobody else is there: -inf instead of 0)."""
    hit = _rejected(small_cases, clamp_edge=True)
    assert len(hit) >= 10, hit
    hit = _rejected(small_cases, skip_outside=True)
    assert len(hit) >= 10 and any("values negative" in h for h in hit) and any("values mixed" in h for h in hit), hit


def test_posterior_faults_are_rejected():
    """On the widest-range input of the largest map (H * W = 97 207, values over 2^-40 .. 1): a float32 running total in index order is off
    by far more than the bound allows, and so is a total without the last, ragged partial range."""
    index = next(i for i in range(21, 400, 24) if "H*W 97207" in FR.posterior_case(i)["label"])
    case = FR.posterior_case(index)
    hm, presence = case["hm"], case["presence"]
    assert hm.shape[0] == 1 and hm.shape[1] * hm.shape[2] == 97207
    want, bound = FR.posterior_reference(hm, presence)
    mean32 = presence.sum(axis=0, dtype=np.float32) / np.float32(len(presence))
    ratio = FR.compare_posterior(emulate_posterior(hm, mean32), want, bound)
    assert ratio <= 1.0
    seq = np.cumsum(hm.reshape(-1), dtype=np.float32)[-1]
    assert abs(float(seq) / hm.astype(np.float64).sum() - 1) > 8 * FR.U  # the float32 running total does exceed the bound on this input
    with pytest.raises(AssertionError, match="outside the bound"):
        FR.compare_posterior(emulate_posterior(hm, mean32, float32_total=True), want, bound)
    assert 97207 % ((97207 + 63) // 64) != 0  # the last range is ragged
    with pytest.raises(AssertionError, match="outside the bound"):
        FR.compare_posterior(emulate_posterior(hm, mean32, drop_last_part=True), want, bound)
    # the other sizes whose last range is ragged and holds a few hundred elements (at H * W = 65 it holds one, which may be tiny)
    for j in (12, 18):  # H * W = 16383, 16385 with K = 1
        case = FR.posterior_case(j)
        hw = case["hm"].shape[1] * case["hm"].shape[2]
        assert hw in (16383, 16385) and hw % ((hw + 63) // 64) != 0, case["label"]
        want, bound = FR.posterior_reference(case["hm"], case["presence"])
        mean32 = case["presence"].sum(axis=0, dtype=np.float32) / np.float32(len(case["presence"]))
        FR.compare_posterior(emulate_posterior(case["hm"], mean32), want, bound)
        with pytest.raises(AssertionError, match="outside the bound"):
            FR.compare_posterior(emulate_posterior(case["hm"], mean32, drop_last_part=True), want, bound, case["label"])


def test_fuzzer_inputs_stay_in_their_stated_ranges():
    """Finite nonzero magnitudes of the revert maps within [2^-60, 2^60]; posterior maps within 2^-40 .. 1 with negative parts at most a quarter
    of the positive sum (asserted inside the generators and the reference); every nonzero wanted posterior value at least 2^-100."""
    for i in range(24):
        case = FR.posterior_case(i)
        hm = case["hm"]
        nz = np.abs(hm[hm != 0])  # (negative entries are scaled down by a few powers of two to fit their quarter: 2^-44)
        assert nz.min() >= 2.0 ** -44 and nz.max() <= 1.0 and np.isfinite(hm).all(), case["label"]
        want, _ = FR.posterior_reference(hm, case["presence"])
        assert np.abs(want[want != 0]).min() >= 2.0 ** -100
    seen = set()
    for i in range(200):
        label = FR.revert_case(i)["label"] if i % 8 < 3 else ""
        seen.update(v for v in ("special nan", "special inf", "special -inf") if v in label)
    assert seen == {"special nan", "special inf", "special -inf"}
