"""The fp64 references and the accuracy bound of tests/fuzz_decode_logits.py, on the CPU: (a) the exact Sparsemax satisfies its KKT conditions and
agrees with the oracle's fp32 Sparsemax, the flip / shift restatement agrees with decode_ref.flip_back; (b) a numpy fp32 emulation of the kernel's
threshold search (pp_decode.hip: the LDS-list and the walk forms, the `alive` pruning, the 64-round cap, the kernel's summation trees) passes the
fuzzer's bound on every value class, and emulations with one fault each fail it. No GPU needed: a kernel with one of these faults would fail the
fuzzer."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fuzz_decode_logits as FD  # noqa: E402
from oracle import decode_ref as D  # noqa: E402
from oracle import model_ref as M  # noqa: E402

F32 = np.float32
THREADS, WAVE = 256, 64


# ------------------------------------------------------------------------------------------------- (a) references
def test_sparsemax64_kkt_and_oracle():
    rng = np.random.default_rng(1)
    rows = [FD.make_row(c, rng, 24, 32, n).ravel() for c, n in (("peaked", None), ("flat", None), ("count", 2), ("count", 700), ("ties", None),
                                                                 ("heavy", None), ("ties", None), ("flat", None))]
    z = np.stack(rows)
    p, tau = FD.sparsemax64(z)
    zc = z - z.max(axis=1, keepdims=True)
    assert (p >= 0).all()
    np.testing.assert_allclose(p.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    s = p > 0
    scale = 1e-12 * (1 + np.abs(z).max(axis=1, keepdims=True))
    assert (np.abs(np.where(s, p - (zc - tau[:, None]), 0)) <= scale).all()  # p_i = z_i - tau on the support
    assert (np.where(s, -np.inf, zc) <= tau[:, None] + scale).all()  # z_i <= tau off it
    want = M.sparsemax(torch.from_numpy(zc.astype(F32))).double().numpy()  # (rows shifted in fp64 first: offsets of 50 cost fp32 digits)
    np.testing.assert_allclose(p, want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("shift", [False, True])
def test_flip_and_shift_references_vs_decode_ref(shift):
    rng = np.random.default_rng(2)
    m = rng.random((2, 17, 9, 12))
    np.testing.assert_array_equal(FD.flip_back64(m, D.COCO_FLIP_INDICES, shift), D.flip_back(m, D.COCO_FLIP_INDICES, shift))
    fl = FD.random_involution(rng, 7)
    assert sorted(fl) == list(range(7)) and all(fl[fl[k]] == k for k in range(7))
    m7 = rng.random((3, 7, 10, 16)).astype(F32)
    np.testing.assert_array_equal(FD.flip_back64(m7, fl, shift), D.flip_back(m7, fl, shift))
    np.testing.assert_array_equal(FD.merge64(m7[:1], m7[1:2], fl, shift), (m7[:1] + D.flip_back(m7[1:2], fl, shift)) * 0.5)
    # to_phased is the layout of pp_deconv_head: pixel (2 y + py, 2 x + px) at [2 py + px, y, x]
    ph = FD.to_phased(m7)
    assert ph[1, 2, 1, 0, 3, 5] == m7[1, 2, 2 * 3 + 1, 2 * 5 + 0]


# ------------------------------------------------------------------------------------------------- (b) the kernel's search in fp32
def _wave_sum(v):
    """(..., 64) -> (...): the xor butterfly 32, 16, .., 1 of wave_allreduce (every lane ends with the same bits)."""
    v = v.astype(F32)
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def _seq_sum(v):
    """(..., m) -> (...): sum along the last axis one fp32 add at a time."""
    s = np.zeros(v.shape[:-1], F32)
    for i in range(v.shape[-1]):
        s = s + v[..., i]
    return s


def _search(y0, y1, nv, flip, rounds=64, ge=False):
    """The threshold search of probmap_decode_kernel on one (b, k): y0, y1 (NV * 1024,) fp32 shifted rows (-inf past the map); -> tau0, tau1."""
    cand = (lambda v, t: v >= t) if ge else (lambda v, t: v > t)
    n0, n1 = int(cand(y0, F32(-1)).sum()), int(cand(y1, F32(-1)).sum()) if flip else 0
    tau0 = tau1 = F32(-1)
    prev = None
    per_thread = lambda y: y.reshape(nv, THREADS, 4).transpose(1, 0, 2).reshape(THREADS, 4 * nv)  # noqa: E731  thread t: quads t + 256 e
    t0, t1 = per_thread(y0), per_thread(y1)
    if n0 <= FD.SMX_CAP and n1 <= FD.SMX_CAP:  # LDS-list form: candidates in (thread, e, j) order, lane l sums entries l, l + 64, ..
        lists = [t[cand(t, F32(-1))] for t in (t0, t1)]
        lists = [np.concatenate([L, np.full((-len(L)) % WAVE, -np.inf, F32)]).reshape(-1, WAVE).T for L in lists]
        for _ in range(rounds):
            d0, d1 = lists[0] - tau0, lists[1] - tau1
            k0, k1 = cand(d0, F32(0)), cand(d1, F32(0)) & flip
            s0, s1 = _wave_sum(_seq_sum(np.where(k0, d0, F32(0)))), _wave_sum(_seq_sum(np.where(k1, d1, F32(0))))
            n = (int(k0.sum()), int(k1.sum()))
            if n == prev:
                break
            prev = n
            tau0 = F32(tau0 + F32(F32(s0 - F32(1)) / F32(n[0])))
            if flip:
                tau1 = F32(tau1 + F32(F32(s1 - F32(1)) / F32(n[1])))
        return tau0, tau1
    alive = np.ones(THREADS, bool)  # walk form
    for _ in range(rounds):
        d0, d1 = t0 - tau0, t1 - tau1
        k0, k1 = cand(d0, F32(0)) & alive[:, None], cand(d1, F32(0)) & alive[:, None] & flip
        c = k0.sum(axis=1) + k1.sum(axis=1)
        s0 = _seq_sum(np.where(k0, d0, F32(0))).reshape(THREADS // WAVE, WAVE)
        s1 = _seq_sum(np.where(k1, d1, F32(0))).reshape(THREADS // WAVE, WAVE)
        alive = alive & (c != 0)
        s0, s1 = _seq_sum(_wave_sum(s0)), _seq_sum(_wave_sum(s1))
        n = (int(k0.sum()), int(k1.sum()))
        if n == prev:
            break
        prev = n
        tau0 = F32(tau0 + F32(F32(s0 - F32(1)) / F32(n[0])))
        if flip:
            tau1 = F32(tau1 + F32(F32(s1 - F32(1)) / F32(n[1])))
    return tau0, tau1


def _clamp01(v):
    return np.fmin(np.fmax(v, F32(0)), F32(1))


def emulate(x, xf, fl, T, normalize, shift, phased=False, rounds=64, ge=False, z_round=None, mirror=True, shift_cols=1, quad_swap=False,
            nan_guard=True):
    """The logits path of probmap_decode_kernel in numpy fp32 -> avg_out (B, K, H, W). x / xf: planar logits (fed through the phase-separated layout
    when `phased`). The keyword arguments after `phased` break one step each."""
    B, K, H, W = x.shape
    nv, HW = FD.nv_bucket(H, W), H * W
    flip = xf is not None

    def load(a):
        if not phased:
            return a
        P = FD.to_phased(a).reshape(B, K, 2, 2, H // 2, W // 2)
        yy, xx = np.mgrid[0:H, 0:W]
        if quad_swap:  # the two 8-byte pairs of a quad interleaved the wrong way: pixels 1 and 2 of every quad swapped
            xx = np.where(xx % 4 == 1, xx + 1, np.where(xx % 4 == 2, xx - 1, xx))
        return P[:, :, yy & 1, xx & 1, yy >> 1, xx >> 1]

    z0 = FD.scale32(load(x), T).reshape(B, K, HW)
    z1 = FD.scale32(load(xf), T).reshape(B, K, HW)[:, fl] if flip else np.full_like(z0, -np.inf)
    if z_round is not None:
        z0, z1 = (torch.from_numpy(z).to(z_round).float().numpy() for z in (z0, z1))
    out0, out1 = np.empty_like(z0), np.empty_like(z1)
    bad = np.zeros((B, K), bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            for k in range(K):
                a0, a1 = z0[b, k], z1[b, k]
                m0, m1 = np.fmax.reduce(a0), np.fmax.reduce(a1)
                if nan_guard and (not np.isfinite(a0).all() or (flip and not np.isfinite(a1).all())):
                    bad[b, k] = True
                    continue
                if normalize is None:
                    out0[b, k], out1[b, k] = _clamp01(np.fmax(a0, F32(0))), _clamp01(np.fmax(a1, F32(0)))
                    continue
                pad = np.full(nv * 1024 - HW, -np.inf, F32)
                y0, y1 = np.concatenate([a0 - m0, pad]), np.concatenate([a1 - m1, pad])
                tau0, tau1 = _search(y0, y1, nv, flip, rounds, ge)
                out0[b, k] = _clamp01(np.fmax(a0 - m0 - tau0, F32(0)) * F32(normalize))
                out1[b, k] = _clamp01(np.fmax(a1 - m1 - tau1, F32(0)) * F32(normalize))
    out0, out1 = out0.reshape(B, K, H, W), out1.reshape(B, K, H, W)
    if flip:  # out1 is already in keypoint order (row flip[k] of the flipped pass)
        src = np.arange(W)[::-1] if mirror else np.arange(W)
        if shift:
            src = np.concatenate([src[:1].repeat(shift_cols), src[:W - shift_cols]])
        out0 = ((out0 + out1[..., src]) * F32(0.5)).astype(F32)
    out0[bad] = np.nan
    return out0


def _cases():
    """A batch of the fuzzer's generator per value class, 64 x 48 and 48 x 32 maps, with a flip partner (class "count": the pass and its partner on
    either side of 1 024 candidates)."""
    rng = np.random.default_rng(7)
    out = []
    for cls in FD.CLASSES:
        for H, W in ((64, 48), (48, 32)):
            B, K, fl = 3, 3, [0, 2, 1]
            T = float(rng.choice([0.5, 0.3, 1e-3, 2.0 ** -126]))
            x, xf, *_ = FD.make_batch(rng, B, K, H, W, T, fl, cls=np.full((B, K), cls))
            out.append((cls, x, xf, fl, T))
    return out


CASES = _cases()


def _worst(normalize=1.0, shift=True, phased=True, **broken):
    """max over the value classes of the fuzzer's error ratio of an emulation (with and without the flip pass)."""
    worst = {}
    for cls, x, xf, fl, T in CASES:
        H, W = x.shape[2:]
        nv = FD.nv_bucket(H, W)
        for pass_f in (xf, None):
            got = emulate(x, pass_f, fl, T, normalize, shift, phased=phased, **broken)
            a = FD.probs64(x, T, normalize)
            ref = FD.merge64(a, FD.probs64(pass_f, T, normalize), fl, shift) if pass_f is not None else a
            r = FD.map_error_ratio(got, ref, FD.map_bound(x, pass_f, fl, T, normalize, nv), FD.poisoned_rows(x, pass_f, fl, T))
            worst[cls] = max(worst.get(cls, 0.0), r)
    return worst


def test_cases_reach_both_search_forms_and_the_boundary():
    n = [FD.candidates32(x, T) for _, x, _, _, T in CASES] + [FD.candidates32(xf, T) for _, _, xf, _, T in CASES]
    n = np.concatenate([a.ravel() for a in n])
    assert (n <= FD.SMX_CAP).any() and (n > FD.SMX_CAP).any() and 1024 in n and 1025 in n


@pytest.mark.parametrize("normalize", [1.0, 2.0, None])
def test_faithful_emulation_passes_the_bound_on_every_class(normalize):
    w = _worst(normalize)
    assert set(w) == set(FD.CLASSES) and max(w.values()) <= 1.0, w


@pytest.mark.parametrize("fault", ["one round", "two rounds", "bf16 z", "fp16 z", "partner not mirrored", "shift off by one",
                                   "phased quad mis-indexed", "no NaN guard"])
def test_broken_emulations_fail_the_bound(fault):
    kw = {"one round": dict(rounds=1), "two rounds": dict(rounds=2), "bf16 z": dict(z_round=torch.bfloat16),
          "fp16 z": dict(z_round=torch.float16), "partner not mirrored": dict(mirror=False), "shift off by one": dict(shift_cols=2),
          "phased quad mis-indexed": dict(quad_swap=True), "no NaN guard": dict(nan_guard=False)}[fault]
    w = _worst(**kw)
    assert max(w.values()) > 1.0, w


def test_ge_for_candidates_reaches_the_same_thresholds():
    """`>=` instead of `>` in the candidate tests is NOT a fault the bound can see, and none it should: a value exactly at the threshold adds
    fl(z - tau) = 0 to the sum and only one to the count, so it slows a round down but the update keeps its fixed point (tau = (sum of the
    support - 1) / n), and the count test drops the value again once tau rises past it. The variant must therefore pass the bound too."""
    w = _worst(ge=True)
    assert max(w.values()) <= 1.0, w
