"""GPU: the two swapped head x codec pairings - ``pp_argmax_probmap_decode`` (Sparsemax + UDP argmax + DARK in one launch) and
``pp_expmax_heatmap_decode`` (the expected-OKS decode on raw maps) - against the launches they are made of, against the reference's
own codecs (tests/golden/codec_swap_cases.npz), under non-finite inputs, through the engine / estimator, and their refusals.

Bit-for-bit comparisons have no tolerance to derive: the fused launch runs the device code of the two launches it replaces in the
same thread mapping (csrc/pp_decode_stages.h), and the raw-map mode is the probability-map kernel with another load. The one bound
(ArgMaxProbMap keypoints against the reference) is ``udp_ref.decode_f64``'s, the rule of
tests/test_udp_decode_gpu.py::test_fixture_cases_of_the_reference."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_codec_swap_host import CFG_HM, CFG_PM, load_fixture, unpack  # noqa: E402

pytestmark = pytest.mark.gpu

LOGITS, PHASED, SHIFT = 1, 2, 4  # PP_DECODE_*
FLIPS = {2: [1, 0], 3: [0, 2, 1], 17: [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]}
GUARD = 64


@pytest.fixture(scope="module")
def T(lib_built):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("needs the MI355X")
    return torch


class Guarded:
    """An output buffer between two canary stretches."""

    def __init__(self, torch, shape, dtype):
        self.torch = torch
        self.n = int(np.prod(shape))
        self.fill = -12345.0
        self.buf = torch.full((self.n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all() and (self.buf[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def bits(t):
    import torch

    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same(a, b):
    import torch

    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def to_phased(t):
    """(B, K, H, W) row-major -> the phase-separated layout of pp_deconv_head: pixel (2 y + py, 2 x + px) at [b, k, 2 py + px, y W/2 + x]."""
    B, K, H, W = t.shape
    return t.view(B, K, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4).contiguous().view(B, K, H, W)


def _outputs(torch, B, K, H, W, avg=True, conv=False):
    o = dict(locs=Guarded(torch, (B, K, 2), torch.float32), keypoints=Guarded(torch, (B, K, 2), torch.float64),
             scores=Guarded(torch, (B, K), torch.float32))
    if avg:
        o["avg"] = Guarded(torch, (B, K, H, W), torch.float32)
    if conv:
        o["conv"] = Guarded(torch, (B, K, H, W), torch.float32)
    return o


def _p(o, k):
    return o[k].ptr() if k in o else None


def _finish(torch, st, o, expect_ok=True):
    from probpose_code_amd import _lib

    torch.cuda.synchronize()
    if expect_ok:
        assert st == _lib.PP_OK, (st, _lib.last_error())
        assert all(g.intact() for g in o.values()), "a canary around an output was overwritten"
    return st, {k: g.t for k, g in o.items()}, o


def _tables(torch, K, H, W):
    from probpose_code_amd import oks_kernel_taps

    taps, radius = oks_kernel_taps(K, H, W)
    return torch.from_numpy(taps).cuda(), torch.from_numpy(radius).cuda()


def _fi(torch, K):
    return torch.tensor(FLIPS[K], dtype=torch.int32, device="cuda")


def launch_probmap_flags(torch, x, xf, temperature, normalize, flags, conv=False, expect_ok=True):
    from probpose_code_amd import _lib

    B, K, H, W = x.shape
    taps, radius = _tables(torch, K, H, W)
    o = _outputs(torch, B, K, H, W, conv=conv)
    st = _lib.lib.pp_probmap_decode_flags(x.data_ptr(), _lib.ptr(xf), _fi(torch, K).data_ptr() if xf is not None else None, taps.data_ptr(),
                                          radius.data_ptr(), B, K, H, W, 4.0 * W, 4.0 * H, temperature, -1.0 if normalize is None else normalize,
                                          _p(o, "avg"), _p(o, "conv"), _p(o, "locs"), _p(o, "keypoints"), _p(o, "scores"), flags, None)
    return _finish(torch, st, o, expect_ok)


def launch_udp(torch, x, ks, expect_ok=True):
    from probpose_code_amd import _lib

    B, K, H, W = x.shape
    o = _outputs(torch, B, K, H, W, avg=False)
    st = _lib.lib.pp_udp_heatmap_decode(x.data_ptr(), None, None, B, K, H, W, 4.0 * W, 4.0 * H, ks, None, _p(o, "locs"), _p(o, "keypoints"),
                                        _p(o, "scores"), 0, None)
    return _finish(torch, st, o, expect_ok)


def launch_argmax(torch, x, xf, temperature, normalize, ks, flags, avg=True, expect_ok=True, K=None):
    from probpose_code_amd import _lib

    B, Kx, H, W = x.shape
    K = K or Kx
    o = _outputs(torch, B, K, H, W, avg=avg)
    st = _lib.lib.pp_argmax_probmap_decode(x.data_ptr(), _lib.ptr(xf), _fi(torch, Kx).data_ptr() if xf is not None else None, B, K, H, W, 4.0 * W,
                                           4.0 * H, temperature, -1.0 if normalize is None else normalize, ks, _p(o, "avg"), _p(o, "locs"),
                                           _p(o, "keypoints"), _p(o, "scores"), flags, None)
    return _finish(torch, st, o, expect_ok)


def launch_expmax(torch, x, xf, flags, conv=True, expect_ok=True, K=None):
    from probpose_code_amd import _lib

    B, Kx, H, W = x.shape
    taps, radius = _tables(torch, Kx, H, W)
    K = K or Kx
    o = _outputs(torch, B, K, H, W, conv=conv)
    st = _lib.lib.pp_expmax_heatmap_decode(x.data_ptr(), _lib.ptr(xf), _fi(torch, Kx).data_ptr() if xf is not None else None, taps.data_ptr(),
                                           radius.data_ptr(), B, K, H, W, 4.0 * W, 4.0 * H, _p(o, "avg"), _p(o, "conv"), _p(o, "locs"),
                                           _p(o, "keypoints"), _p(o, "scores"), flags, None)
    return _finish(torch, st, o, expect_ok)


def make_logits(torch, B, K, H, W, seed):
    """Head-like logits: one blob per map (amplitude 2 - 30, sigma 1 - 2.5, centre from -1 to W / H) + N(0, 0.3); map 1 of every crop is
    all negative (with normalize=None its map is all zero: the decode reads the neighbour), the last map nearly flat (more Sparsemax
    candidates than the compact threshold search holds, where the map has that many pixels)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = []
    for _ in range(2):
        amp = torch.tensor([2.0, 8.0, 30.0])[torch.randint(0, 3, (B, K), generator=g)]
        cx, cy = torch.rand(B, K, generator=g) * (W + 1) - 1, torch.rand(B, K, generator=g) * (H + 1) - 1
        sg = 1.0 + 1.5 * torch.rand(B, K, generator=g)
        z = amp[..., None, None] * torch.exp(-((xx - cx[..., None, None]) ** 2 + (yy - cy[..., None, None]) ** 2) / (2 * sg[..., None, None] ** 2))
        z = z + 0.3 * torch.randn(B, K, H, W, generator=g)
        z[:, 1] = -1.0 - z[:, 1].abs()
        z[:, K - 1] = 0.01 * torch.randn(B, H, W, generator=g)
        out.append(z.contiguous().cuda())
    return out


def make_raw_maps(torch, B, K, H, W, seed):
    """ViTPose-like raw maps: Gaussian blobs (sigma 2, amplitude 0.3 - 1.6) + N(0, 0.02) - 0.01: values below 0 and above 1."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = []
    for _ in range(2):
        amp = 0.3 + 1.3 * torch.rand(B, K, generator=g)
        amp[:, 0] = 1.6
        cx, cy = torch.rand(B, K, generator=g) * (W + 3) - 2, torch.rand(B, K, generator=g) * (H + 3) - 2
        cx[:, 0], cy[:, 0] = W / 2.0, H / 2.0
        m = amp[..., None, None] * torch.exp(-((xx - cx[..., None, None]) ** 2 + (yy - cy[..., None, None]) ** 2) / 8.0)
        out.append((m + 0.02 * torch.randn(B, K, H, W, generator=g) - 0.01).contiguous().cuda())
    return out


def _check_argmax_against_chain(torch, z, zf, phased, shift, temperature, normalize, ks):
    flags = (PHASED if phased else 0) | (SHIFT if shift else 0)
    zin, zfin = (to_phased(z), to_phased(zf) if zf is not None else None) if phased else (z, zf)
    keep = zin.clone(), (zfin.clone() if zfin is not None else None)
    _, chain1, _ = launch_probmap_flags(torch, zin, zfin, temperature, normalize, LOGITS | flags)
    _, chain2, _ = launch_udp(torch, chain1["avg"].contiguous(), ks)
    _, got, _ = launch_argmax(torch, zin, zfin, temperature, normalize, ks, flags)
    label = (tuple(z.shape), phased, zf is not None, shift, temperature, normalize, ks)
    assert same(got["avg"], chain1["avg"]), label
    for k in ("locs", "keypoints", "scores"):
        assert same(got[k], chain2[k]), (k, label)
    assert same(zin, keep[0]) and (zfin is None or same(zfin, keep[1])), "an input was written"
    if normalize is None and zf is None and z.shape[1] > 2:  # (K = 2: map 1 is the flat one) map 1 is all zero: loc (-1, -1), three of its seven points come from map 0 inside the same launch
        assert bool((got["locs"][:, 1] == -1).all()) and bool(torch.isfinite(got["keypoints"][:, 1]).all())
    return got


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("phased,H,W", [(False, 16, 12), (True, 16, 16)])
def test_argmax_probmap_equals_the_two_launches_chained(T, phased, H, W):
    torch = T
    n = 0
    for K, B in itertools.product((3, 17), (1, 2)):
        z, zf = make_logits(torch, B, K, H, W, seed=100 * K + B)
        for flip, temperature, normalize, ks in itertools.product(("none", "plain", "shift"), (1.0, 0.5, 0.7), (1.0, None), (11, 17)):
            got = _check_argmax_against_chain(torch, z, zf if flip != "none" else None, phased, flip == "shift", temperature, normalize, ks)
            n += 1
    # a repeat launch gives the same bits; without avg_out the results are the same
    _, again, _ = launch_argmax(torch, to_phased(z) if phased else z, to_phased(zf) if phased else zf, 0.7, None, 17, (PHASED if phased else 0) | SHIFT)
    _, lean, _ = launch_argmax(torch, to_phased(z) if phased else z, to_phased(zf) if phased else zf, 0.7, None, 17, (PHASED if phased else 0) | SHIFT, avg=False)
    for k in ("locs", "keypoints", "scores"):
        assert same(again[k], got[k]) and same(lean[k], got[k]), k
    assert same(again["avg"], got["avg"]) and n == 144


@pytest.mark.parametrize("H,W,K,B,ks", [(64, 48, 17, 2, 11), (96, 72, 2, 1, 17)])
def test_argmax_probmap_at_the_two_row_lengths(T, H, W, K, B, ks):
    """The sizes the kernel templates dispatch on (3 and 7 quads per thread); the nearly flat last map takes the block-wide threshold
    search (more than 1 024 candidates)."""
    torch = T
    z, zf = make_logits(torch, B, K, H, W, seed=H)
    for phased, flip, normalize in ((True, "plain", 1.0), (False, "shift", 1.0), (True, "none", None), (True, "shift", None)):
        _check_argmax_against_chain(torch, z, zf if flip != "none" else None, phased, flip == "shift", 0.5, normalize, ks)
    _check_argmax_against_chain(torch, z, zf, True, False, 0.7, 1.0, 9)  # a kernel size whose radius is a run-time value


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("H,W,K,B", [(16, 12, 3, 1), (16, 12, 17, 2), (16, 16, 3, 2), (16, 16, 17, 1), (64, 48, 17, 2), (96, 72, 2, 1)])
def test_expmax_heatmap_equals_the_probability_map_launch(T, H, W, K, B):
    torch = T
    m, mf = make_raw_maps(torch, B, K, H, W, seed=7 * H + K)
    assert float(m.min()) < 0 and float(m.max()) > 1 and float(mf.min()) < 0 and float(mf.max()) > 1, "a launch that clamps must fail this test"
    for flip in ("none", "plain", "shift"):
        f = mf if flip != "none" else None
        flags = SHIFT if flip == "shift" else 0
        _, want, _ = launch_probmap_flags(torch, m, f, 1.0, 1.0, flags, conv=True)
        _, got, _ = launch_expmax(torch, m, f, flags)
        for k in ("avg", "conv", "locs", "keypoints", "scores"):
            assert same(got[k], want[k]), (k, flip)
        if f is None:
            assert same(got["avg"], m)  # raw: nothing clamped, nothing scaled
        if W % 8 == 0:
            mp, fp = to_phased(m), (to_phased(f) if f is not None else None)
            keep = mp.clone()
            _, ph, _ = launch_expmax(torch, mp, fp, flags | PHASED)
            for k in ("avg", "conv", "locs", "keypoints", "scores"):
                assert same(ph[k], got[k]), (k, flip, "phased")
            assert same(mp, keep)
            _, again, _ = launch_expmax(torch, mp, fp, flags | PHASED)
            assert all(same(again[k], ph[k]) for k in ph)


# ------------------------------------------------------------------------------------------------ C
def test_expmax_codec_on_the_reference_fixture(T, golden_dir):
    torch = T
    import probpose_code_amd as pp

    d = load_fixture(golden_dir)
    fi = [int(i) for i in d["flip_indices"]]
    n = 0
    for name in d["expmax.names"]:
        a, b = unpack(d, f"{name}.a"), unpack(d, f"{name}.b")
        K, H, W = a.shape
        codec = pp.KEYPOINT_CODECS.build(dict(type="UDPExpMaxHeatmap", input_size=tuple(int(v) for v in d[f"{name}.input_size"]), heatmap_size=(W, H)))
        ta, tb = torch.from_numpy(a).cuda()[None], torch.from_numpy(b).cuda()[None]
        outs = dict(a=codec.decode_device(ta), b=codec.decode_device(tb), plain=codec.decode_device(ta, tb, fi, return_avg=True),
                    shift=codec.decode_device(ta, tb, fi, return_avg=True, shift_heatmap=True))
        for tag, o in outs.items():
            kp, sc = o["keypoints"].cpu().numpy(), o["scores"].cpu().numpy()
            assert kp.dtype == np.float64 and sc.dtype == np.float32
            assert np.array_equal(kp.view(np.int64), d[f"{name}.{tag}.keypoints"].view(np.int64)), (name, tag)
            assert np.array_equal(sc.view(np.int32), d[f"{name}.{tag}.scores"].view(np.int32)), (name, tag)
            if "heatmaps" in o and f"{name}.{tag}.maps" in d.files:
                assert np.array_equal(o["heatmaps"][0].cpu().numpy().view(np.int32), d[f"{name}.{tag}.maps"].view(np.int32)), (name, tag)
            n += K
        kp, sc = codec.decode(a)  # one numpy sample, as the reference's decode takes it
        assert kp.shape == (1, K, 2) and np.array_equal(kp.view(np.int64), d[f"{name}.a.keypoints"].view(np.int64))
        assert sc.shape == (1, K) and np.array_equal(sc.view(np.int32), d[f"{name}.a.scores"].view(np.int32))
    assert n == 272


def test_argmax_codec_on_the_reference_fixture(T, golden_dir):
    torch = T
    import probpose_code_amd as pp
    import udp_ref as R

    d = load_fixture(golden_dir)
    compared = left_out = 0

    def keypoints_within_bound(kp, maps, ks, size, want):
        nonlocal compared, left_out
        K, H, W = maps.shape
        ref = R.decode_f64(maps, ks, size)
        scale = np.asarray(size, np.float64) / [W - 1, H - 1]
        ok = ref["cond"] < 100
        err = (np.abs(kp - ref["keypoints"]) / scale).max(1)  # heatmap pixels, per coordinate
        err32 = (np.abs(kp - want) / scale).max(1)
        print(f"max err / bound vs fp64 {np.max(err[ok] / ref['bound'][ok]):.3f}, vs the reference's fp32 {np.max(err32[ok] / (2 * ref['bound'][ok])):.3f}")
        assert (err[ok] <= ref["bound"][ok]).all(), (err, ref["bound"])
        assert (err32[ok] <= 2 * ref["bound"][ok]).all(), (err32, ref["bound"])
        compared += int(ok.sum())
        left_out += int((~ok).sum())

    for name in d["argmax.names"]:
        maps, ks, size = d[f"{name}.maps"], int(d[f"{name}.ks"]), tuple(int(v) for v in d[f"{name}.input_size"])
        n, H, W = maps.shape
        codec = pp.KEYPOINT_CODECS.build(dict(type="ArgMaxProbMap", input_size=size, heatmap_size=(W, H), blur_kernel_size=ks))
        o = codec.decode_device(torch.from_numpy(maps).cuda().view(n // 17, 17, H, W))
        assert np.array_equal(o["locs"].cpu().numpy(), d[f"{name}.locs"]) and np.array_equal(o["scores"].cpu().numpy().view(np.int32), d[f"{name}.scores"].view(np.int32)), name
        kp = o["keypoints"].cpu().numpy()
        for i in range(n // 17):
            keypoints_within_bound(kp[i], maps[17 * i:17 * i + 17], ks, size, d[f"{name}.keypoints"][i])
        k1, s1 = codec.decode(maps[:17])
        assert np.array_equal(k1[0], kp[0]) and np.array_equal(s1[0], d[f"{name}.scores"][0])
        # the Sparsemax-fused entry point on the stored logits: the same integer maximum wherever its maps' maximum is the fixture's
        z = torch.from_numpy(unpack(d, f"{name}.logits")).cuda().view(n // 17, 17, H, W)
        _, fused, _ = launch_argmax(torch, z, None, 1.0, 1.0, ks, 0)
        assert np.abs(fused["avg"].cpu().numpy().reshape(n, H, W) - maps).max() < 1e-5  # (fp32 threshold search against the fixture's fp64 one)
    a, b, fi = torch.from_numpy(d["argmax_flip.a"]).cuda(), torch.from_numpy(d["argmax_flip.b"]).cuda(), [int(i) for i in d["flip_indices"]]
    codec = pp.KEYPOINT_CODECS.build(dict(type="ArgMaxProbMap", input_size=(48, 64), heatmap_size=(12, 16)))
    for shift, tag in ((False, "argmax_flip.plain"), (True, "argmax_flip.shift")):
        o = codec.decode_device(a, b, fi, return_avg=True, shift_heatmap=shift)
        assert np.array_equal(o["heatmaps"].cpu().numpy().view(np.int32), d[f"{tag}.avg"].view(np.int32)), tag
        assert np.array_equal(o["scores"].cpu().numpy().view(np.int32), d[f"{tag}.scores"].view(np.int32)) and np.array_equal(o["locs"].cpu().numpy(), d[f"{tag}.locs"])
        for i in range(2):
            keypoints_within_bound(o["keypoints"][i].cpu().numpy(), d[f"{tag}.avg"][i], 11, (48, 64), d[f"{tag}.keypoints"][i])
    print(f"compared {compared}, left out {left_out}")
    assert compared >= 200 and left_out <= 0.01 * (compared + left_out)


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_poison(T, poison):
    torch = T
    import probpose_code_amd as pp

    B, K, H, W = 2, 17, 16, 16
    z, zf = make_logits(torch, B, K, H, W, seed=5)
    m, mf = make_raw_maps(torch, B, K, H, W, seed=6)
    for which, x, xf, launch in (("argmax", z, zf, lambda a, f, fl: launch_argmax(torch, a, f, 0.5, 1.0, 11, fl)),
                                 ("expmax", m, mf, lambda a, f, fl: launch_expmax(torch, a, f, fl))):
        for phased in (False, True):
            lay = to_phased if phased else (lambda t: t)
            fl = PHASED if phased else 0
            _, clean, _ = launch(lay(x), lay(xf), fl)
            # (b, k) = (1, 4): its own pass, then the flipped pass - keypoint 4's partner there is channel FLIPS[17][4] = 3
            for in_flip, ch in ((False, 4), (True, 3)):
                px, pf = x.clone(), xf.clone()
                (pf if in_flip else px)[1, ch, 7, 9] = poison
                _, got, _ = launch(lay(px), lay(pf), fl)
                hit = torch.zeros(B, K, dtype=torch.bool, device="cuda")
                hit[1, 4] = True
                for k in ("locs", "keypoints", "scores"):
                    g, c = got[k], clean[k]
                    assert torch.isnan(g[1, 4]).all(), (which, k, phased, in_flip)
                    mask = hit[..., None].expand_as(g) if g.dim() == 3 else hit
                    assert torch.equal(bits(g)[~mask], bits(c)[~mask]), (which, k, phased, in_flip)
                others = ~hit
                assert torch.equal(bits(got["avg"])[others], bits(clean["avg"])[others]) and torch.isnan(got["avg"][1, 4]).all()
    # the codecs' batch_decode raises, as UDPHeatmap's does
    bad = m.clone()
    bad[0, 2, 3, 3] = poison
    sizes = dict(input_size=(64, 64), heatmap_size=(16, 16))
    for name in ("UDPExpMaxHeatmap", "ArgMaxProbMap"):
        codec = pp.KEYPOINT_CODECS.build(dict(type=name, **sizes))
        codec.batch_decode(m)
        with pytest.raises(FloatingPointError, match=name):
            codec.batch_decode(bad)


# ------------------------------------------------------------------------------------------------ F
def test_refusals_write_nothing(T):
    torch = T
    from probpose_code_amd import _lib

    z, zf = make_logits(torch, 1, 17, 16, 16, seed=1)
    tall = torch.zeros(1, 1, 3072, 4, device="cuda")

    def refused(res, status, text):
        st, _, o = res
        assert st == status and text in _lib.last_error(), (st, _lib.last_error())
        assert all(g.untouched() for g in o.values()), "a refused call wrote an output"

    refused(launch_argmax(torch, z, zf, 0.5, 1.0, 11, LOGITS, expect_ok=False), _lib.PP_ERR_INVALID_ARG, "unknown flag")
    refused(launch_argmax(torch, z, zf, 0.5, 1.0, 11, 8, expect_ok=False), _lib.PP_ERR_INVALID_ARG, "unknown flag")
    refused(launch_argmax(torch, z, zf, 0.5, 1.0, 12, 0, expect_ok=False), _lib.PP_ERR_INVALID_ARG, "odd")
    refused(launch_argmax(torch, z, zf, 0.5, 1.0, 21, 0, expect_ok=False), _lib.PP_ERR_UNSUPPORTED, "above 19")
    refused(launch_argmax(torch, tall, None, 0.5, 1.0, 11, 0, expect_ok=False), _lib.PP_ERR_UNSUPPORTED, "LDS")
    refused(launch_expmax(torch, z, zf, LOGITS, expect_ok=False), _lib.PP_ERR_INVALID_ARG, "unknown flag")
    refused(launch_expmax(torch, z, zf, 16, expect_ok=False), _lib.PP_ERR_INVALID_ARG, "unknown flag")
    # K > 17: the reference's kernel table has 17 sigmas (the taps of 17 keypoints are passed: nothing is read)
    refused(launch_expmax(torch, z, None, 0, expect_ok=False, K=18), _lib.PP_ERR_UNSUPPORTED, "17 sigmas")


# ------------------------------------------------------------------------------------------------ E
@functools.lru_cache(maxsize=2)
def _state_dict(head):
    from probpose_code_amd import synthetic as S

    return S.synthetic_state_dict("small", seed=0, logit_scale=2.0) if head == "probmap" else S.synthetic_state_dict("small", seed=0, logit_scale=2.0, head="heatmap")


def _model(head, codec=None):
    from probpose_code_amd import apis

    opts = {"model.test_cfg.flip_test": True, "model.precision": "f16x3", "model.test_cfg.output_heatmaps": True}
    if codec is not None:
        opts["model.head.decoder.type"] = codec
    return apis.init_model(CFG_PM if head == "probmap" else CFG_HM, dict(state_dict=_state_dict(head)), device="cuda:0", cfg_options=opts)


def _counts():
    from probpose_code_amd import _lib

    return {k: _lib.launch_count(k) for k in ("pp_decode.hip", "pp_udp_decode.hip", "pp_argmax_decode.hip", "pp_argmax_probmap_decode", "pp_expmax_heatmap_decode")}


@pytest.mark.parametrize("head,codec,fn", [("probmap", "ArgMaxProbMap", "pp_argmax_probmap_decode"), ("heatmap", "UDPExpMaxHeatmap", "pp_expmax_heatmap_decode")])
def test_swapped_codec_end_to_end(T, head, codec, fn):
    """``keypoints_conf`` is the decode's own score (the map's maximum under DARK, the map at the convolved maximum under ExpMax), so it
    changes with the codec like ``keypoints`` and ``keypoint_scores``; every other field is the towers' and must not."""
    torch = T
    from probpose_code_amd import _lib, apis
    from probpose_code_amd import synthetic as S

    B = 2
    model, base = _model(head, codec), _model(head)
    eng = model.engine
    assert type(model.head.decoder).__name__ == codec and eng.decode == model.head.decoder.decode_kind != base.engine.decode
    crops = S.synthetic_crops(B, seed=3)
    center, scale = S.whole_image_bbox_meta(B)

    def step(m):
        return m.test_step(apis.pack_crops(crops, center, scale, m.dataset_meta))

    _lib.reset_launch_counts()
    first = step(model)
    counts = _counts()
    want = dict.fromkeys(counts, 0)
    want[fn] = 1
    want["pp_argmax_decode.hip" if head == "probmap" else "pp_decode.hip"] = 1  # (the source file's own tally)
    assert counts == want, counts
    _lib.reset_launch_counts()
    ref = step(base)
    counts = _counts()
    assert counts == dict(want, **{fn: 0, "pp_argmax_decode.hip": 0, "pp_decode.hip": int(head == "probmap"), "pp_udp_decode.hip": int(head == "heatmap")}), counts

    # the step's keypoints and scores == the codec's own decode_device on the step's averaged maps
    hm = torch.stack([torch.as_tensor(s.pred_fields.heatmaps) for s in first]).cuda().float()
    own = model.head.decoder.decode_device(hm)
    kp, sc = own["keypoints"].cpu().numpy(), own["scores"].cpu().numpy()
    for i, s in enumerate(first):
        meta = s.metainfo
        img = kp[i:i + 1] / meta["input_size"] * meta["input_scale"] + meta["input_center"] - 0.5 * meta["input_scale"]
        p = s.pred_instances
        assert np.array_equal(np.asarray(p.keypoints).view(np.int64), img.view(np.int64)), i
        conf = p.keypoints_conf if head == "probmap" else p.keypoint_scores
        assert np.array_equal(np.asarray(conf, np.float32).view(np.int32), sc[i:i + 1].view(np.int32)), i
    # the maps are the default pairing's maps; the towers' outputs are untouched by the codec
    changed = ("keypoints", "keypoint_scores", "keypoints_conf", "keypoints_visible" if head == "heatmap" else "")
    moved = False
    for a, b in zip(first, ref):
        assert torch.equal(torch.as_tensor(a.pred_fields.heatmaps), torch.as_tensor(b.pred_fields.heatmaps))
        for key, value in b.pred_instances.all_items():
            if key not in changed:
                assert np.array_equal(np.asarray(value), np.asarray(getattr(a.pred_instances, key))), key
        moved |= not np.array_equal(a.pred_instances.keypoints, b.pred_instances.keypoints)
    assert moved, "the swapped codec decoded exactly what the default one does"

    # the third batch of a size replays a graph equal to the launches one by one
    before = eng.graph_captures
    second, third = step(model), step(model)
    assert eng.graph_captures == before + 1
    for a, b, c in zip(first, second, third):
        for f in ("keypoints", "keypoint_scores", "keypoints_visible"):
            assert np.array_equal(getattr(a.pred_instances, f), getattr(c.pred_instances, f)) and np.array_equal(getattr(a.pred_instances, f), getattr(b.pred_instances, f)), f
    # test_step_stream yields the same samples (it carries no heatmaps)
    model.test_cfg["output_heatmaps"] = False
    batches = [apis.pack_crops(crops[:n], center[:n], scale[:n], model.dataset_meta) for n in (2, 1, 2)]
    plain = [model.test_step(b) for b in batches]
    for a, b in zip(plain, model.test_step_stream(batches, depth=2, max_batch=2)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(x.pred_instances.keypoints, y.pred_instances.keypoints)
            assert np.array_equal(x.pred_instances.keypoint_scores, y.pred_instances.keypoint_scores)
    for x, y in zip(plain[0], first):
        assert np.array_equal(x.pred_instances.keypoints, y.pred_instances.keypoints)

    # a batch large enough for the fused head: the decode reads the phase-separated logits
    Bp = 8
    big = S.synthetic_crops(Bp, seed=4).cuda()
    out = eng.forward(big, True, S.COCO_FLIP_INDICES, return_heatmaps=True, shift_heatmap=True)
    torch.cuda.synchronize()
    assert eng._logits_phased
    own = model.head.decoder.decode_device(out["heatmaps"].view(Bp, 17, eng.Hh, eng.Wh))
    for k in ("keypoints", "scores", "locs"):
        assert same(out[k], own[k]), k
