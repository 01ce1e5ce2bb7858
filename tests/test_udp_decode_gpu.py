"""GPU: pp_udp_heatmap_decode (csrc/pp_udp_decode.hip) against the numpy forms of tests/udp_ref.py - the fixture of the reference's
own functions, a deterministic sweep over layouts / flip / shift / sizes, a few seconds of the random fuzzer
(tests/fuzz_udp_decode.py), and the non-finite policy."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F(lib_built):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("needs the MI355X")
    import fuzz_udp_decode as Fz

    return Fz


def test_fixture_cases_of_the_reference(F, golden_dir):
    import udp_ref as R

    g = np.load(os.path.join(golden_dir, "udp_decode_cases.npz"))
    for name in g["names"]:
        maps, ks, size = g[f"{name}.maps"], int(g[f"{name}.ks"]), tuple(int(v) for v in g[f"{name}.input_size"])
        K, H, W = maps.shape
        res = F.launch(maps[None], None, None, ks, size)
        assert np.array_equal(res["locs"][0], g[f"{name}.locs"]) and np.array_equal(res["scores"], g[f"{name}.scores"]), name
        ref = R.decode_f64(maps, ks, size)
        scale = np.asarray(size, np.float64) / [W - 1, H - 1]
        ok = ref["cond"] < 100
        err = (np.abs(res["keypoints"][0] - ref["keypoints"]) / scale).max(1)  # heatmap pixels, per coordinate
        assert (err[ok] <= ref["bound"][ok]).all(), (name, err, ref["bound"])
        # against the reference's own fp32 result: two fp32 forms of the same decode, each within the bound of the fp64 one
        err32 = (np.abs(res["keypoints"][0] - g[f"{name}.keypoints"][0]) / scale).max(1)
        assert (err32[ok] <= 2 * ref["bound"][ok]).all(), (name, err32, ref["bound"])
    # the read outside a non-positive map, as the reference does it: keypoint 0 follows the LAST map's bottom-right corner
    res = F.launch(g["nonpositive_three_16x12.maps"][None], None, None, 11, (48, 64))
    want = g["nonpositive_three_16x12.keypoints"][0, 0]
    # (x only: that neighbour's bottom-left pixel is clipped like the non-positive map itself, so dyy is exactly 0 and dxy an fp32 rounding
    # residue of the size of eps32 - the y step hangs on the last bit of log(1e-3); condition number ~1e7, outside the comparable set)
    assert abs(res["keypoints"][0, 0, 0] - want[0]) < 1e-3 and not np.isclose(want[0], -1 * 48 / 11)
    # the same read with a well-conditioned Hessian: the neighbour's mass reaches both bottom corners
    yy, xx = np.mgrid[0:16, 0:12].astype(np.float64)
    wide = 0.9 * np.exp(-((xx - 5.0) ** 2 / (2 * 36.0) + (yy - 16.0) ** 2 / (2 * 16.0)))
    maps = np.stack([np.full((16, 12), -0.1), wide]).astype(np.float32)[None]
    ref = R.decode_f64(maps[0], 11, (48, 64))
    assert ref["cond"][0] < 100 and np.abs(ref["step"][0]).min() > 0.05, (ref["cond"], ref["step"])
    stats = {}
    F.check_case(maps, None, None, 11, (48, 64), np.array([["nonpositive", "blob"]]), stats=stats)
    assert stats["nonpositive"][0] == 1
    # flip-test average, with and without the one-pixel shift
    a, b, fi = g["flip.a"], g["flip.b"], g["flip.flip_indices"].tolist()
    for shift, tag in ((False, "flip.plain"), (True, "flip.shift")):
        res = F.launch(a, b, fi, 11, (48, 64), shift=shift)
        assert np.array_equal(res["avg"], g[f"{tag}.avg"]) and np.array_equal(res["scores"], g[f"{tag}.scores"])
        scale = np.array([48 / 11, 64 / 15])
        for i in range(len(a)):
            ref = R.decode_f64(g[f"{tag}.avg"][i], 11, (48, 64))
            ok = ref["cond"] < 100
            assert ok.sum() >= 6
            assert ((np.abs(res["keypoints"][i] - ref["keypoints"]) / scale).max(1)[ok] <= ref["bound"][ok]).all(), tag
            assert ((np.abs(res["keypoints"][i] - g[f"{tag}.keypoints"][i]) / scale).max(1)[ok] <= 2 * ref["bound"][ok]).all(), tag


@pytest.mark.parametrize("phased", [False, True])
@pytest.mark.parametrize("flip,shift", [(False, False), (True, False), (True, True)])
def test_layouts_flip_and_shift(F, phased, flip, shift):
    rng = np.random.default_rng(11 + 2 * phased + 4 * flip + 8 * shift)
    for (B, K, H, W, ks) in ((3, 17, 64, 48, 11), (2, 5, 96, 72, 17)):
        import udp_ref as R

        classes = rng.choice(R.ALL_CLASSES, (B, K))
        maps = np.stack([np.concatenate([R.make_maps(c, 1, H, W, rng) for c in row]) for row in classes])
        fi = rng.permutation(K).tolist()
        mf = (maps[:, np.argsort(fi)][..., ::-1] + rng.normal(0, 1e-3, maps.shape)).astype(np.float32) if flip else None
        F.check_case(maps, None if mf is None else np.ascontiguousarray(mf), fi, ks, (4 * W, 4 * H), classes, phased=phased, shift=shift)


@pytest.mark.parametrize("B,K,H,W,ks", [(512, 17, 16, 12, 11), (1, 1, 8, 6, 11), (2, 28, 33, 27, 17), (1, 3, 128, 96, 11), (1, 2, 96, 128, 19),
                                        (4, 7, 111, 109, 11), (8, 17, 64, 48, 1), (64, 17, 64, 48, 11)])
def test_sizes(F, B, K, H, W, ks):
    import udp_ref as R

    rng = np.random.default_rng(B * 1000 + K * 10 + H)
    classes = rng.choice(R.ALL_CLASSES, (B, K))
    classes[0, 0] = "blob"  # (every case compares at least one coordinate pair)
    maps = np.empty((B, K, H, W), np.float32)
    for cls in R.ALL_CLASSES:
        sel = classes == cls
        if sel.any():
            maps[sel] = R.make_maps(cls, int(sel.sum()), H, W, rng)
    stats = {}
    F.check_case(maps, None, None, ks, (4 * W, 4 * H), classes, stats=stats)
    assert set(stats) == set(classes.ravel().tolist()) and sum(v[0] + v[1] for v in stats.values()) == B * K  # every keypoint judged
    assert stats["blob"][0] >= 1


def test_random_fuzz_a_few_seconds(F):
    import udp_ref as R

    n, stats = F.run(seconds=4.0, seed=1, min_cases=16)
    compared = sum(stats.get(c, [0, 0, 0])[0] for c in R.BLOB_CLASSES)
    left_out = sum(stats.get(c, [0, 0, 0])[1] for c in R.BLOB_CLASSES)
    print({c: v for c, v in stats.items()}, f"{n} cases")
    assert compared > 2000
    for c in R.BLOB_CLASSES:  # the cap: at most 1 % of a blob class left out for an ill-conditioned fp64 Hessian
        cmp_, out, _ = stats.get(c, [0, 0, 0.0])
        assert out <= 0.01 * (cmp_ + out), f"{c}: {out} of {cmp_ + out} keypoints left out"
    assert left_out <= 0.01 * (compared + left_out)


def test_eps_identity_decides_the_step_on_a_singular_hessian(F):
    """The one place where ``H + eps32 * I`` decides the result: a stencil whose Hessian is exactly singular with the derivative in its
    null space. Kernel size 1 (the blur is the identity, the rescale factor 1) and values that the clip maps to exactly three log
    levels - A = log 50 (values >= 50), 0 (value 1), log 1e-3 (value 0) - give dxx = dyy = -A, dxy = A, dx = dy = A / 2 without a
    rounding in either form: H = [[-A, A], [A, -A]], g along its null vector (1, 1), step = g / eps32 with the identity term, 0 without
    it (the pseudo-inverse drops the zero singular value). Compared relatively: the condition number is ~1e8 by construction."""
    import udp_ref as R

    H, W, y, x = 12, 10, 5, 4
    m = np.zeros((1, 1, H, W), np.float32)
    m[0, 0, y, x] = 64.0                                            # the maximum: clipped to 50
    m[0, 0, y, x + 1] = m[0, 0, y + 1, x] = m[0, 0, y + 1, x + 1] = 55.0   # xp, yp, xpyp: clipped to 50 as well
    m[0, 0, y - 1, x - 1] = 55.0                                    # xmym
    m[0, 0, y, x - 1] = m[0, 0, y - 1, x] = 1.0                     # xm, ym: log 1 = 0
    size = (4 * W, 4 * H)
    res = F.launch(m, None, None, 1, size)
    kp32, _, locs, refined = R.decode_f32(m[0], 1, size)
    _, _, _, faulty = R.decode_f32(m[0], 1, size, eps_identity=False)
    assert np.array_equal(res["locs"][0, 0], [x, y]) and np.array_equal(faulty[0], [x, y])  # without eps * I nothing moves
    want = -0.5 * np.log(np.float32(50.0)) / R.EPS32  # loc - g / eps32, loc negligible
    assert abs(refined[0, 0] / want - 1) < 1e-5 and abs(refined[0, 1] / want - 1) < 1e-5, refined
    assert np.abs(res["keypoints"][0, 0] / kp32[0, 0] - 1).max() < 1e-5, (res["keypoints"], kp32)
    assert not (R.decode_f64(m[0], 1, size)["cond"][0] < 100)


def test_non_finite_values_give_nan_results(F):
    import udp_ref as R

    rng = np.random.default_rng(3)
    K, H, W = 6, 16, 12
    maps = R.make_maps("blob", 2 * K, H, W, rng).reshape(2, K, H, W)
    maps[0, 3] = -0.1  # a non-positive map: it reads the map before it
    poisoned = maps.copy()
    poisoned[0, 1, 5, 5] = np.nan
    poisoned[1, 0, 0, 0] = np.inf
    poisoned[1, 4, H - 1, W - 1] = -np.inf
    poisoned[0, 2, 7, 7] = np.nan  # the neighbour of the non-positive map 3
    clean = F.launch(maps, None, None, 11, (48, 64), want_avg=False)
    res = F.launch(poisoned, None, None, 11, (48, 64), want_avg=False)
    bad = np.zeros((2, K), bool)
    bad[0, [1, 2, 3]] = True
    bad[1, [0, 4]] = True
    assert np.isnan(res["keypoints"][bad]).all() and np.isnan(res["scores"][bad]).all() and np.isnan(res["locs"][bad]).all()
    assert np.array_equal(res["keypoints"][~bad], clean["keypoints"][~bad]) and np.array_equal(res["scores"][~bad], clean["scores"][~bad])
    # the flipped pass is looked at too
    fi = list(range(K))
    flipped = np.ascontiguousarray(maps[..., ::-1])
    flipped[1, 5, 2, 2] = np.nan
    res = F.launch(maps, flipped, fi, 11, (48, 64), want_avg=False)
    assert np.isnan(res["scores"][1, 5]) and np.isfinite(res["scores"][0]).all()
    # the host mirror raises
    import torch

    from probpose_code_amd import KEYPOINT_CODECS

    codec = KEYPOINT_CODECS.build(dict(type="UDPHeatmap", input_size=(48, 64), heatmap_size=(12, 16), sigma=2))
    kp, sc = codec.decode(maps[0])
    assert kp.shape == (1, K, 2) and kp.dtype == np.float64 and sc.shape == (1, K) and sc.dtype == np.float32
    assert np.array_equal(kp[0], clean["keypoints"][0]) and codec.support_batch_decoding
    with pytest.raises(FloatingPointError):
        codec.decode(poisoned[0])
    out = codec.decode_device(torch.from_numpy(maps).cuda(), torch.from_numpy(flipped).cuda(), fi, return_avg=True)
    assert out["heatmaps"].shape == (2, K, H, W)
