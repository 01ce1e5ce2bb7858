"""CPU: the two numpy restatements of the UDP-DARK decode (tests/udp_ref.py) that the GPU fuzzer judges the kernel by.

* the stepwise fp32 form equals the reference's own functions bit for bit (tests/golden/udp_decode_cases.npz, made by
  tests/golden/make_golden_udp.py from the reference's get_heatmap_maximum / gaussian_blur / refine_keypoints_dark_udp /
  UDPHeatmap.decode / flip_heatmaps);
* the error bound of udp_ref.decode_f64 (derived from the rounding points of the fp32 arithmetic, module docstring there) holds for
  the fp32 form against the fp64 form on every value class of the fuzzer, and REJECTS fp32 emulations with one fault each.

One fault the bound cannot reject on comparable keypoints, by construction: dropping ``eps32 * I``. Where the Hessian's condition
number is below 100 the term changes the step by a relative 1e-7 / sigma_min - below the fp32 noise of the log map it is added
to; it decides the result only where the Hessian is singular, which the condition rule leaves out. That emulation is therefore
rejected on a singular seven-point stencil, where the reference's step is g / eps32 and the faulty one 0.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import udp_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "udp_decode_cases.npz"))


def test_fixture_holds_the_cases_the_decode_is_specified_on(cases):
    names = list(cases["names"])
    assert {"blobs_16x12", "blobs_16x12_ks17", "peaks_ties_flat_16x12", "nonpositive_16x12", "nonpositive_three_16x12",
            "nonpositive_empty_corner_16x12", "model_64x48", "model_96x72"} <= set(names)
    assert int(cases["model_96x72.ks"]) == 17 and int(cases["model_64x48.ks"]) == 11
    # the reference's read outside the map: keypoint 0 of a sample whose map 0 is non-positive follows the LAST map's bottom-right corner
    assert np.array_equal(cases["nonpositive_three_16x12.locs"][0], [-1, -1])
    assert not np.array_equal(cases["nonpositive_three_16x12.refined"][0, 0], [-1, -1])
    assert np.array_equal(cases["nonpositive_empty_corner_16x12.refined"][0, 0], [-1, -1])
    assert cases["nonpositive_three_16x12.refined"].dtype == np.float32 and cases["blobs_16x12.keypoints"].dtype == np.float64


def test_stepwise_form_equals_the_reference_bit_for_bit(cases):
    for name in cases["names"]:
        maps, ks, size = cases[f"{name}.maps"], int(cases[f"{name}.ks"]), tuple(cases[f"{name}.input_size"])
        kp, sc, locs, refined = R.decode_f32(maps, ks, size)
        assert np.array_equal(locs, cases[f"{name}.locs"]), name
        assert np.array_equal(sc, cases[f"{name}.scores"]), name
        assert np.array_equal(refined[None], cases[f"{name}.refined"]), name
        assert kp.dtype == np.float64 and np.array_equal(kp, cases[f"{name}.keypoints"]), name
        if f"{name}.blurred" in cases:
            b = R.blur(maps, ks)
            with np.errstate(all="ignore"):
                b = b * (maps.reshape(len(maps), -1).max(1) / (b.reshape(len(b), -1).max(1) + np.float32(1e-12)))[:, None, None]
            assert b.dtype == np.float32 and np.array_equal(b, cases[f"{name}.blurred"]), name


def test_flip_average_equals_the_reference_bit_for_bit(cases):
    a, b, fi = cases["flip.a"], cases["flip.b"], cases["flip.flip_indices"].tolist()
    for shift, tag in ((False, "flip.plain"), (True, "flip.shift")):
        avg = R.flip_average(a, b, fi, shift)
        assert np.array_equal(avg, cases[f"{tag}.avg"])
        for i in range(len(a)):
            kp, sc, _, _ = R.decode_f32(avg[i], int(cases["flip.ks"]), tuple(cases["flip.input_size"]))
            assert np.array_equal(kp[0], cases[f"{tag}.keypoints"][i]) and np.array_equal(sc[0], cases[f"{tag}.scores"][i])


def _violations(maps, ks, **fault):
    """fp32 (faulty) emulation against fp64 per keypoint: (comparable, violating the bound, worst error / bound)."""
    H, W = maps.shape[-2:]
    ref = R.decode_f64(maps, ks, (4 * W, 4 * H))
    _, _, locs, refined = R.decode_f32(maps, ks, (4 * W, 4 * H), **fault)
    ok = ref["cond"] < 100
    err = np.abs(refined.astype(np.float64) - ref["refined"]).max(1)
    with np.errstate(all="ignore"):
        rel = np.where(ok, err / ref["bound"], 0.0)
    return int(ok.sum()), int((ok & (err > ref["bound"])).sum()), float(np.nanmax(rel)) if ok.any() else 0.0


@pytest.mark.parametrize("cls", R.ALL_CLASSES)
@pytest.mark.parametrize("shape_ks", [(16, 12, 11), (64, 48, 11), (33, 27, 17), (8, 6, 11)])
def test_bound_holds_for_the_fp32_form_on_every_value_class(cls, shape_ks):
    H, W, ks = shape_ks
    rng = np.random.default_rng(sum(map(ord, cls)) * 131 + H)
    n_cmp = n_bad = 0
    for _ in range(4):
        c, v, _ = _violations(R.make_maps(cls, 17, H, W, rng), ks)
        n_cmp, n_bad = n_cmp + c, n_bad + v
    assert n_bad == 0, f"{cls} {H}x{W}: {n_bad} of {n_cmp} comparable keypoints beyond the bound"
    if cls in R.BLOB_CLASSES and H >= 16:
        assert n_cmp >= 0.99 * 4 * 17, f"{cls}: more than 1 % of the keypoints have an ill-conditioned fp64 Hessian"


def _blobs(rng, n, H, W, amp, sig=2.0, noise=0.0, tilt=False):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for _ in range(n):
        cx, cy = rng.uniform(3, W - 4), rng.uniform(3, H - 4)
        dx, dy = xx - cx, yy - cy
        if tilt:  # sigma 1.5 along one diagonal, 3.5 along the other: a cross term in the log map
            u, v = (dx + dy) / np.sqrt(2), (dx - dy) / np.sqrt(2)
            q = u * u / (2 * 1.5**2) + v * v / (2 * 3.5**2)
        else:
            q = (dx * dx + dy * dy) / (2 * sig * sig)
        out.append(rng.uniform(*amp) * np.exp(-q) + rng.normal(0, noise, (H, W)) if noise else rng.uniform(*amp) * np.exp(-q))
    return np.stack(out).astype(np.float32)


def _fault_inputs(name, rng):
    H, W = 24, 20
    if name == "border":  # blobs on and beyond the borders: a reflected border doubles the mass there
        return R.make_maps("blob_border", 32, H, W, rng)
    if name in ("rescale", "clip"):  # faint blobs: the rescale to the original maximum decides what the clip at 1e-3 cuts
        return _blobs(rng, 32, H, W, (1.02e-3, 1.3e-3))
    if name == "dxy":
        return _blobs(rng, 32, H, W, (0.5, 1.0), tilt=True)
    if name == "argmax_blur":  # a hot pixel above a broad, lower blob: the blurred map peaks at the blob
        m = _blobs(rng, 32, H, W, (0.6, 0.8), sig=3.0)
        for i in range(len(m)):
            y, x = np.unravel_index(np.argmax(m[i]), m[i].shape)
            m[i, (y + H // 2) % H, (x + W // 2) % W] = 1.0
        return m
    if name == "ties":  # the same exact pattern twice: first index against last
        m = np.zeros((32, H, W), np.float32)
        pat = np.array([[0.25, 0.5, 0.25], [0.5, 1.0, 0.5], [0.25, 0.5, 0.25]], np.float32)
        for i in range(32):
            y0, x0 = rng.integers(1, H // 2 - 3), rng.integers(1, W - 4)
            m[i, y0:y0 + 3, x0:x0 + 3] = pat
            m[i, y0 + H // 2:y0 + H // 2 + 3, x0:x0 + 3] = pat
        return m
    return R.make_maps("blob", 32, H, W, rng)


@pytest.mark.parametrize("name,fault", [
    ("border", dict(border="reflect")), ("rescale", dict(rescale=False)), ("sigma", dict(sigma_ks=17)), ("clip", dict(clip_lo=1e-4)),
    ("dxy", dict(dxy_half=False)), ("argmax_blur", dict(argmax_on_blur=True)), ("ties", dict(last_tie=True))])
def test_bound_rejects_an_emulation_with_one_fault(name, fault):
    rng = np.random.default_rng(len(name) * 1000 + 7)
    maps = _fault_inputs(name, rng)
    c0, v0, worst0 = _violations(maps, 11)
    assert v0 == 0 and c0 >= 8, f"{name}: the faultless form itself misses the bound on these inputs ({v0} of {c0}, worst {worst0:.2f})"
    c, v, worst = _violations(maps, 11, **fault)
    print(f"{name}: faultless worst error / bound {worst0:.3f} on {c0} keypoints; with the fault {v} of {c} beyond the bound, worst {worst:.1f}")
    assert v >= max(2, c // 10), f"{name}: the bound lets the faulty emulation through ({v} of {c} comparable keypoints beyond it)"


def test_missing_eps_identity_is_rejected_on_a_singular_hessian():
    """See the module docstring: log map linear along y (no curvature there), curved along x."""
    f = np.float32
    p = dict(c=np.array([f(-1.0)]), xp=np.array([f(-1.25)]), xm=np.array([f(-1.25)]), yp=np.array([f(-0.5)]), ym=np.array([f(-1.5)]),
             xpyp=np.array([f(-0.75)]), xmym=np.array([f(-1.75)]))
    ref = R.newton_step_f32(p)
    bad = R.newton_step_f32(p, eps_identity=False)
    assert ref[0, 0] == 0.0 and abs(ref[0, 1] - 0.5 / R.EPS32) <= 1e-6 * 0.5 / R.EPS32  # dy / eps32: the reference's step on a ridge
    assert bad[0, 1] == 0.0  # pinv drops the zero singular value: the faulty form does not move at all
    # and on comparable keypoints the term is below the bound's resolution, as the docstring says
    rng = np.random.default_rng(5)
    c, v, _ = _violations(R.make_maps("blob", 32, 24, 20, rng), 11, eps_identity=False)
    assert c >= 30 and v == 0
