"""CPU: what tests/fuzz_codec_swap.py rests on, without a GPU.
  (a) its restated admission predicates agree with the real library (the argument checks run in front of every HIP call: dummy non-NULL
      pointers are never dereferenced) - pp_argmax_probmap_decode answers PP_OK for B = 0 only after all its checks, so every table shape,
      admitted or refused, is pinned with B = 0; pp_expmax_heatmap_decode returns early for B = 0, so only its refused shapes are, with B = 1;
      and the kernels' static LDS, which the LDS check leaves room for, is what the compiler allocates;
  (b) the table reaches what it claims: every (NV bucket, compile-time / run-time radius, flip, phased) combination, rows longer than the
      workgroup, maps lower than nine rows, the neighbour-map path at k = 0 and k > 0, every branch of the expmax kernel's first-zero rule,
      a dense map of several convolution bands;
  (c) the 2 % cap on left-out blob keypoints holds for the reference alone (the fp64 Sparsemax map rounded to fp32 standing in for avg_out);
  (d) the checkers accept reference-made outputs of every admitted case and reject single faults applied to those outputs."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import fuzz_codec_swap as F  # noqa: E402
import fuzz_decode_logits as FD  # noqa: E402
import udp_ref as R  # noqa: E402
from oracle import decode_ref as D  # noqa: E402

F32 = np.float32
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "probpose_code_amd", "csrc")


# ------------------------------------------------------------------------------------------------- (a) admission
@pytest.fixture()
def lib(lib_built):
    from probpose_code_amd import _lib

    buf = ctypes.create_string_buffer(64)
    return _lib, ctypes.addressof(buf), buf  # (buf keeps the address alive; it is never dereferenced)


def _names(_lib):
    return {_lib.PP_OK: F.OK, _lib.PP_ERR_INVALID_ARG: F.INVALID_ARG, _lib.PP_ERR_UNSUPPORTED: F.UNSUPPORTED}


def _argmax_status(_lib, p, H, W, ks, phased, K=1):
    st = _lib.lib.pp_argmax_probmap_decode(p, p, p, 0, K, H, W, 4.0 * W, 4.0 * H, 0.5, 1.0, ks, p, p, p, p, F.PHASED if phased else 0, None)
    return _names(_lib).get(int(st), int(st)), _lib.last_error()


def _agrees(want, got, label):
    status, err = got
    if want is None:
        assert status == F.OK, (label, status, err)
    else:
        assert status == want[0] and want[1] in err, (label, want, status, err)


def test_argmax_predicate_is_the_librarys(lib):
    _lib, p, _ = lib
    for c in F.argmax_table():
        assert c["refused"] == F.argmax_refusal(c["H"], c["W"], c["ks"], c["phased"])
        _agrees(c["refused"], _argmax_status(_lib, p, c["H"], c["W"], c["ks"], c["phased"], c["K"]), F._label(c))
    # the LDS edge of every width / kernel size of the table, three rows either side; and a sweep
    for W in (4, 48, 512):
        for ks in (1, 11, 19):
            top = F.largest_h(W, ks)
            assert F.argmax_admits(top, W, ks) and not F.argmax_admits(top + 1, W, ks)
            for H in range(top - 3, top + 4):
                _agrees(F.argmax_refusal(H, W, ks), _argmax_status(_lib, p, H, W, ks, False), (H, W, ks))
    rng = np.random.default_rng(3)
    seen = Counter()
    for _ in range(3000):
        W = int(rng.choice([4 * int(rng.integers(1, 40)), int(rng.integers(2, 200)), 4 * int(rng.integers(40, 1600))]))
        H = int(rng.integers(2, max(3, 2 * F.MAX_PIXELS // W)))
        ks, phased = int(rng.integers(1, 23)), bool(rng.random() < 0.3)
        want = F.argmax_refusal(H, W, ks, phased)
        _agrees(want, _argmax_status(_lib, p, H, W, ks, phased), (H, W, ks, phased))
        seen[want] += 1
    assert seen[None] > 100 and seen[(F.UNSUPPORTED, "LDS")] > 20 and seen[(F.UNSUPPORTED, "12288")] > 100, seen


def test_expmax_refusals_are_the_librarys(lib):
    _lib, p, _ = lib

    def status(H, W, K, phased):
        st = _lib.lib.pp_expmax_heatmap_decode(p, p, p, p, p, 1, K, H, W, 4.0 * W, 4.0 * H, p, p, p, p, p, F.PHASED if phased else 0, None)
        return _names(_lib).get(int(st), int(st)), _lib.last_error()

    n = 0
    for c in F.expmax_table():
        assert c["refused"] == F.expmax_refused(c["H"], c["W"], c["K"], c["phased"])
        if c["refused"] is not None:
            _agrees(c["refused"], status(c["H"], c["W"], c["K"], c["phased"]), F._label(c))
            n += 1
    assert n >= 8
    rng = np.random.default_rng(4)
    seen = Counter()
    for _ in range(3000):
        W = int(rng.choice([4 * int(rng.integers(1, 40)), int(rng.integers(2, 200)), 4 * int(rng.integers(40, 1600))]))
        H = int(rng.integers(2, max(3, 2 * F.MAX_PIXELS // W)))
        K, phased = int(rng.integers(1, 20)), bool(rng.random() < 0.3)
        want = F.expmax_refused(H, W, K, phased)
        if want is not None:  # (an admitted shape would launch)
            _agrees(want, status(H, W, K, phased), (H, W, K, phased))
            seen[want[1]] += 1
    assert all(seen[w] > 5 for w in ("17 sigmas", "even height", "radius (9)", "multiple of 4", "LDS", "12288")), seen


def test_udp_decode_refuses_the_shapes_whose_lds_only_the_static_part_overflows(lib):
    """pp_udp_heatmap_decode runs the same DARK stage: 4 (64 + H ((W + 2 r) | 1) + (H + 2 r) W) bytes of dynamic LDS, 256 held statically. 1510 x 4
    at kernel size 19 needs 163 624 + 256 bytes: once admitted (and then a HIP error), now PP_ERR_UNSUPPORTED. (B = 0 returns before this check.)"""
    _lib, p, _ = lib
    for H, refused in ((F.UDP_TOP_H, False), (F.UDP_TOP_H + 1, True), (F.UDP_TOP_H + 3, True)):
        lds = 4 * (64 + H * ((4 + 18) | 1) + (H + 18) * 4)
        assert (lds > F.LDS_BYTES - F.STATIC_LDS) == refused and lds <= F.LDS_BYTES
        if refused:
            st = _lib.lib.pp_udp_heatmap_decode(p, None, None, 1, 1, H, 4, 16.0, 4.0 * H, 19, None, p, p, p, 0, None)
            assert st == _lib.PP_ERR_UNSUPPORTED and "LDS" in _lib.last_error(), (H, st, _lib.last_error())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("src", ["pp_argmax_decode.hip", "pp_udp_decode.hip"])
def test_static_lds_of_the_dark_kernels_is_what_the_lds_check_leaves_free(src):
    """hipFuncSetAttribute takes a dynamic LDS size of one CU's 160 KiB less the kernel's static LDS (the workgroup reduction behind
    __syncthreads_or); the argument checks refuse a shape that needs more (UDP_STATIC_LDS, csrc/pp_decode_stages.h)."""
    with tempfile.TemporaryDirectory() as td:
        subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", f"-I{CSRC}", f"-I{ROOT}/include", "-c", os.path.join(CSRC, src),
                        "-o", "x.o", "--save-temps"], cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
        text = open(os.path.join(td, [f for f in os.listdir(td) if f.endswith("gfx950.s")][0])).read()
    sizes = [int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", text)]
    assert sizes and max(sizes) <= F.STATIC_LDS, sizes
    stages = open(os.path.join(CSRC, "pp_decode_stages.h")).read()
    assert f"UDP_STATIC_LDS = {F.STATIC_LDS};" in stages


# ------------------------------------------------------------------------------------------------- (b) what the table reaches
def _admitted(table):
    return [c for c in table if c["refused"] is None]


def test_argmax_table_reaches_every_dispatch_and_edge():
    table = F.argmax_table()
    assert table is F.argmax_table() and [c["seed"] for c in table] == [910000 + i for i in range(len(table))]  # fixed
    ok = _admitted(table)
    combos = Counter((FD.nv_bucket(c["H"], c["W"]), c["ks"] in F.KS_COMPILE_TIME, c["flip"], c["phased"]) for c in ok)
    missing = [(nv, ct, fl, ph) for nv in (3, 7, 12) for ct in (True, False) for fl in F.FLIPS for ph in (False, True) if not combos[(nv, ct, fl, ph)]]
    assert not missing, missing
    assert sum(c["W"] > 256 for c in ok) >= 8 and {(c["H"], c["W"]) for c in ok} >= set(F.ARGMAX_LONG)
    assert sum(c["H"] < 9 for c in ok) >= 20 and {(c["H"], c["W"]) for c in ok} >= set(F.ARGMAX_SMALL) | set(FD.EDGE_SHAPES)
    small = {c["ks"] for c in ok if c["H"] * c["W"] <= 256}
    prod = {(c["H"], c["W"], c["ks"]) for c in ok}
    assert small == set(F.KS_ALL) and all((H, W, ks) in prod for H, W in FD.PRODUCTION for ks in F.KS_ALL)
    assert {c["K"] for c in ok} >= {1, 2, 3, 17} and {c["normalize"] for c in ok} == set(F.NORMALIZE)
    assert {c["T"] for c in ok} >= {float(F32(t)) for t in FD.TEMPERATURES}
    # the neighbour-map path: an all-negative row under normalize None, at k = 0 (reads keypoint K - 1) and elsewhere
    neg = [c for c in ok if c["neg_at"] is not None]
    assert all(c["neg_at"] is not None for c in ok if c["K"] >= 2 and c["normalize"] is None and c["cls"] != "poison")
    assert sum(c["neg_at"] == 0 for c in neg) >= 3 and sum(c["neg_at"] > 0 for c in neg) >= 3
    for c in neg[:6]:
        d = F.case_data(c)
        avg = F.none_map32(d["x"], d["xf"] if c["flip"] != "none" else None, d["fl"], c["T"], c["flip"] == "shift")
        assert (avg[:, c["neg_at"]] == 0).all() and (d["cls"][:, c["neg_at"]] == "negative").all()
    # the LDS edges: the largest H and the one above, refused for LDS or for the pixel cap
    for W in (4, 48, 512):
        for ks in (1, 11, 19):
            H = F.largest_h(W, ks)
            assert any((c["H"], c["W"], c["ks"]) == (H, W, ks) for c in ok)
            assert any((c["H"], c["W"], c["ks"]) == (H + 1, W, ks) and c["refused"][1] in ("LDS", "12288") for c in table if c["refused"])
    classes = Counter()
    for c in ok:
        classes.update(Counter(F.case_data(c)["cls"].ravel().tolist()))
    assert all(classes[n] >= 10 for n in F.ARGMAX_CLASSES + ("negative", "blob_clamped")), classes
    assert all(c["B"] * c["K"] <= (8 if c["H"] * c["W"] > 4096 else 64) for c in table)


def test_expmax_table_reaches_every_zero_rule_branch_and_several_bands():
    table = F.expmax_table()
    ok = _admitted(table)
    assert all(c["B"] * c["K"] <= (8 if c["H"] * c["W"] > 4096 else 64) for c in table)
    assert {(c["H"], c["W"]) for c in ok} >= set(F.EXPMAX_SMALL) | set(FD.EDGE_SHAPES) and {c["K"] for c in ok} >= {1, 2, 17}
    assert {(c["flip"], c["phased"]) for c in ok} == {(f, p) for f in F.FLIPS for p in (False, True)}
    assert {c["cls"] for c in ok} >= set(F.EXPMAX_DENSE + F.EXPMAX_SPARSE + ("single_neg", "poison"))
    for cls in F.EXPMAX_SPARSE:
        assert {c["place"] for c in ok if c["cls"] == cls and c["flip"] == "none"} == set(F.PLACEMENTS)
    zero_wins, branches, bands, signs = Counter(), Counter(), Counter(), Counter()
    for c in ok:
        d = F.case_data(c)
        avg = F.reference_outputs(c)["main"]
        radius = F.radius_of(c["K"], c["H"], c["W"])
        for b, k in zip(*np.nonzero(~d["bad"])):
            m = avg["avg"][b, k]
            branch, idx = F.zidx_branch(m, radius[k])
            branches[branch] += 1
            x, y = avg["locs"][b, k]
            conv = avg["conv"][b, k]
            won = int(np.argmax(conv))
            if idx >= 0 and won == idx and conv.flat[won] == 0 and (m != 0).any() and conv.min() < 0:
                zero_wins[branch] += 1  # nothing in the box is positive: the first zero outside it is the maximum
            bands[min(3, F.conv_bands(m, radius[k]))] += 1
            signs["below 0"] += bool(m.min() < 0)
            signs["above 1"] += bool(m.max() > 1)
            signs["-0.0"] += bool((np.signbit(m) & (m == 0)).any())
            signs["conv +0.0 in the box"] += bool(c["cls"] == "sparse_cancel" and (conv[m.any(1)] == 0).any())
    assert all(zero_wins[b] >= 3 for b in ("origin", "right", "below")), (zero_wins, branches)
    assert all(branches[b] >= 3 for b in ("empty", "origin", "right", "below", "none")), branches
    assert bands[1] > 50 and bands[2] + bands[3] >= 10, bands
    assert all(signs[s] >= 10 for s in ("below 0", "above 1", "-0.0", "conv +0.0 in the box")), signs


# ------------------------------------------------------------------------------------------------- (c), (d) the checkers on reference-made outputs
@pytest.fixture(scope="module")
def accepted():
    """Every admitted case of both tables through its checker, fed with reference-made outputs -> {kind: stats}."""
    stats = dict(argmax=F.new_stats(), expmax=F.new_stats())
    for c in _admitted(F.argmax_table()):
        F.check_argmax(c, F.reference_outputs(c), stats["argmax"])
    for c in _admitted(F.expmax_table()):
        F.check_expmax(c, F.reference_outputs(c), stats["expmax"])
    return stats


def test_checkers_accept_reference_outputs_and_the_cap_holds_for_the_reference_alone(accepted):
    print(F.report(accepted["argmax"], "argmax (reference-made outputs)"))
    compared, left_out, share = F.blob_cap(accepted["argmax"])
    assert compared >= F.BLOB_MIN and share <= F.BLOB_CAP, (compared, left_out, share)
    assert all(st["map_ratio"] <= 1 and st["kp_ratio"] <= 1 for k, st in accepted["argmax"].items() if not k.startswith("#"))
    # why blobs under normalize None / 10 are a class of their own, outside the cap: saturated into plateaus, the reference alone leaves
    # out several times the cap there
    clamped = F.blob_cap(accepted["argmax"], "blob_clamped")
    print("blob_clamped (reference alone): compared %d, left out %d = %.1f %%" % (clamped[0], clamped[1], 100 * clamped[2]))
    assert clamped[0] >= 300 and clamped[2] > 2 * F.BLOB_CAP, clamped


def test_refused_cases_need_status_word_and_untouched_outputs():
    c = next(c for c in F.argmax_table() if c["refused"] and c["refused"][1] == "LDS")
    good = dict(status=c["refused"][0], error=f"pp_argmax_probmap_decode: ... {c['refused'][1]}", untouched=True)
    F.check_argmax(c, good)
    for bad in (dict(good, untouched=False), dict(good, status=F.INVALID_ARG), dict(good, error="H*W exceeds 12288 pixels"), F.reference_outputs(
            dict(c, refused=None, id=0))):
        with pytest.raises(AssertionError):
            F.check_argmax(c, bad)
    ok = next(c for c in F.argmax_table() if c["refused"] is None)
    with pytest.raises(AssertionError):
        F.check_argmax(ok, dict(status=F.UNSUPPORTED, error="LDS", untouched=True))


def _rejects(check, case, out):
    try:
        check(case, out)
    except AssertionError:
        return True
    return False


def _first(table, pred):
    return next(c for c in table if c["refused"] is None and pred(c))


def test_argmax_checker_rejects_a_pixel_moved_one_column(accepted):
    c = _first(F.argmax_table(), lambda c: c["cls"] == "blob" and c["normalize"] == 1.0 and (c["H"], c["W"]) == (64, 48))
    out = F.reference_outputs(c)
    avg = out["main"]["avg"]
    y, x = np.unravel_index(int(np.argmax(avg[0, 0])), avg[0, 0].shape)
    x2 = x + 1 if x + 1 < c["W"] else x - 1
    avg[0, 0, y, x], avg[0, 0, y, x2] = avg[0, 0, y, x2], avg[0, 0, y, x]
    assert _rejects(F.check_argmax, c, out)


def test_argmax_checker_rejects_the_last_tie(accepted):
    n = 0
    for c in _admitted(F.argmax_table()):
        if c["cls"] not in ("ties", "blob") or c["normalize"] is not None or n >= 3:
            continue
        out = F.reference_outputs(c)
        avg, locs = out["main"]["avg"], out["main"]["locs"]
        for b, k in zip(*np.nonzero(~F.case_data(c)["bad"])):
            m = avg[b, k]
            where = np.flatnonzero(m == m.max())
            if m.max() > 0 and len(where) > 1:
                locs[b, k] = [where[-1] % c["W"], where[-1] // c["W"]]
                assert _rejects(F.check_argmax, c, out), F._label(c)
                n += 1
                break
    assert n >= 3


def test_argmax_checker_rejects_the_neighbour_map_of_the_wrong_side(accepted):
    """A map with maximum <= 0 takes points from keypoint k - 1; outputs made with keypoint k + 1 instead must fail wherever the two
    neighbours' bottom corners differ and the Hessian is well conditioned."""
    tried = rejected = candidates = 0
    for c in _admitted(F.argmax_table()):
        if c["neg_at"] is None or c["K"] < 3:
            continue
        d, out = F.case_data(c), F.reference_outputs(c)
        k, K = c["neg_at"], c["K"]
        for b in range(c["B"]):
            hm = F._decodable(out["main"]["avg"][b], d["bad"][b])
            ref = R.decode_f64(hm, c["ks"], F.input_size(c))
            wrong = hm.copy()
            wrong[(k - 1) % K] = hm[(k + 1) % K]
            kp = R.decode_f64(wrong, c["ks"], F.input_size(c))["keypoints"][k]
            scale = np.asarray(F.input_size(c), np.float64) / [c["W"] - 1, c["H"] - 1]
            candidates += 1
            if ref["cond"][k] < 100 and (np.abs(kp - ref["keypoints"][k]) / scale).max() > ref["bound"][k]:
                faulty = dict(out, main=dict(out["main"], keypoints=out["main"]["keypoints"].copy()))
                faulty["main"]["keypoints"][b, k] = kp
                tried += 1
                rejected += _rejects(F.check_argmax, c, faulty)
    print(f"the wrong neighbour moves {tried} of {candidates} (sample, keypoint) pairs on the neighbour path past their bound; each is rejected")
    assert tried >= 3 and rejected == tried and tried >= 0.05 * candidates, (tried, rejected, candidates)


def test_argmax_checker_rejects_the_taps_of_a_smaller_kernel(accepted):
    for ks in (3, 11, 17, 19):
        c = _first(F.argmax_table(), lambda c: c["cls"] == "blob" and c["ks"] == ks and c["normalize"] in (0.5, 1.0) and c["H"] >= 8)
        out, d = F.reference_outputs(c), F.case_data(c)
        for b in range(c["B"]):
            out["main"]["keypoints"][b] = R.decode_f64(F._decodable(out["main"]["avg"][b], d["bad"][b]), ks - 2, F.input_size(c))["keypoints"]
        assert _rejects(F.check_argmax, c, out), F._label(c)


def test_argmax_checker_rejects_a_flipped_pass_that_is_not_shifted(accepted):
    for nz in (1.0, None):
        c = _first(F.argmax_table(), lambda c: c["flip"] == "shift" and c["normalize"] == nz and c["cls"] == "blob" and c["H"] >= 8)
        d, out = F.case_data(c), F.reference_outputs(c)
        avg = F.argmax_map64(c, d, shift=False)[0].astype(F32) if nz is not None else F.none_map32(d["x"], d["xf"], d["fl"], c["T"], False)
        out["main"]["avg"] = avg
        assert _rejects(F.check_argmax, c, out), F._label(c)


def test_expmax_checker_rejects_a_zero_outside_the_box_that_does_not_compete(accepted):
    n = 0
    for c in _admitted(F.expmax_table()):
        if c["cls"] != "sparse_neg" or c["flip"] != "none":
            continue
        out = F.reference_outputs(c)
        m = out["main"]
        if not (m["conv"].reshape(c["B"], c["K"], -1).max(-1) == 0).any():
            continue  # (a rectangle whose dilated box is the whole map: no zero to compete)
        for b in range(c["B"]):
            conv = m["conv"][b]
            flat = np.where(conv == 0, -np.inf, conv).reshape(c["K"], -1).argmax(1)  # the best of the box only
            locs = np.stack([flat % c["W"], flat // c["W"]], -1).astype(F32)
            m["locs"][b] = D.subpixel_refine(conv, locs)
            m["keypoints"][b] = m["locs"][b] / [c["W"] - 1, c["H"] - 1] * list(F.input_size(c))
            m["scores"][b] = m["avg"][b].reshape(c["K"], -1)[np.arange(c["K"]), flat]
        assert _rejects(F.check_expmax, c, out), F._label(c)
        n += 1
    assert n >= 9


def test_expmax_checker_rejects_a_convolution_rounded_twice_and_a_clamp_on_load(accepted):
    from scipy.ndimage import correlate1d

    c = _first(F.expmax_table(), lambda c: c["cls"] == "dense" and c["flip"] == "none" and (c["H"], c["W"]) == (9, 12))
    out = F.reference_outputs(c)
    kern = D.oks_kernels(c["K"], c["H"], c["W"])
    for b in range(c["B"]):
        for k in range(c["K"]):
            t = kern[k].sum(0)
            rows = correlate1d(out["main"]["avg"][b, k].astype(np.float64), t, axis=1, mode="reflect").astype(F32)  # fp32 between the passes
            out["main"]["conv"][b, k] = correlate1d(rows.astype(np.float64), t, axis=0, mode="reflect").astype(F32)
    assert _rejects(F.check_expmax, c, out)
    out = F.reference_outputs(c)
    d = F.case_data(c)
    assert d["x"].min() < 0 and d["x"].max() > 1
    clamped = np.clip(d["x"], 0, 1)
    out["main"] = dict(avg=clamped, **F.expmax_oracle(clamped, d["bad"], F.input_size(c)))
    assert _rejects(F.check_expmax, c, out)


def test_the_cancellation_bound_rests_on_measured_constants_and_rejects_a_double_rounding(accepted):
    """The derived check of class "cancel_rows": the 1-D taps against the 2-D weights stay within SEPARABLE_ULPS, conv64 is the oracle's sum,
    the class holds maps whose oracle result is an exact 0.0 inside the box, and a convolution rounded through fp32 between the passes - an
    error of 2^-24 of the partial sums, not 2^-44 - is outside the bound."""
    from scipy.ndimage import correlate1d

    from probpose_code_amd.codecs import oks_kernel_taps

    worst = 0.0
    for H, W in FD.EDGE_SHAPES + F.EXPMAX_SMALL:
        taps, radius = oks_kernel_taps(17, H, W)
        for k, w in enumerate(D.oks_kernels(17, H, W)):
            t = taps[k, :2 * radius[k] + 1]
            worst = max(worst, float((np.abs(np.outer(t, t) - w) / w).max()) / 2.0 ** -53)
    print(f"|t_i t_j - w_ij| / w_ij <= {worst:.1f} u")
    assert worst <= F.SEPARABLE_ULPS
    cases = [c for c in F.expmax_table() if c["cls"] == "cancel_rows" and c["refused"] is None]
    assert len(cases) >= len(F.PLACEMENTS)
    zeros = rejected = 0
    for c in cases[:6]:
        out = F.reference_outputs(c)
        m = out["main"]
        kern = D.oks_kernels(c["K"], c["H"], c["W"])
        for k in range(c["K"]):
            c64 = F.conv64(m["avg"][0, k], kern[k])
            assert np.array_equal(c64.astype(F32), D.convolve_symmetric_f64(m["avg"][0, k], kern[k]))
            zeros += int(((c64 == 0) & (F.cancel_bound(m["avg"][0, k], kern[k]) > 0)).any())
            t = kern[k].sum(0)
            rows = correlate1d(m["avg"][0, k].astype(np.float64), t, axis=1, mode="reflect").astype(F32)
            m["conv"][0, k] = correlate1d(rows.astype(np.float64), t, axis=0, mode="reflect").astype(F32)
        dec = F.decode_from_conv(m["avg"][0], m["conv"][0], F.input_size(c))  # (self-consistent: only the bound can reject it)
        m["locs"][0], m["keypoints"][0], m["scores"][0] = dec["locs"], dec["keypoints"], dec["scores"]
        rejected += _rejects(F.check_expmax, c, out)
    assert zeros >= 6 and rejected == 6, (zeros, rejected)
