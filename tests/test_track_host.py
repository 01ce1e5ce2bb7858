"""CPU: the pose tracker's box rule as ``tracking.next_boxes_host`` states it, on crafted records, and ``tracking.affine_params_host`` against the
val pipeline's own box arithmetic. (The device form is held to these functions bit for bit in tests/test_track_gpu.py.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cases as C  # noqa: E402


def _step(c, **kw):
    return C.run_host(c, **kw)


def test_defaults_and_parameter_checks():
    from probpose_code_amd import tracking

    assert tracking.TRACK_DEFAULTS == dict(kpt_thr=0.3, min_keypoints=4, expand=1.25, min_side=8.0, smooth=0.0, max_lost=10, dup_oks_thr=0.9)
    assert tracking.track_params(kpt_thr=0.5)["kpt_thr"] == 0.5 and tracking.track_params()["max_lost"] == 10
    with pytest.raises(TypeError, match="unknown tracking parameter"):
        tracking.track_params(kpt_threshold=0.5)
    for bad in (dict(min_keypoints=0), dict(max_lost=-1), dict(expand=0.0), dict(min_side=0.0), dict(smooth=1.0), dict(kpt_thr=float("nan")),
                dict(expand=float("inf"))):
        with pytest.raises(ValueError):
            tracking.track_params(**bad)
    assert "NOT VALIDATED ON REAL FOOTAGE" in tracking.__doc__


def test_the_box_follows_a_translating_pose():
    """A pose moving 3 px per frame: every frame's box is the pose's min/max box grown by 1.25 about its centre, `lost` stays 0 - also when
    the pose has left the box it was cropped with by more than a box width."""
    boxes, alive, lost = np.array([[40, 30, 90, 100]], np.float32), np.ones(1, np.int32), np.zeros(1, np.int32)
    for f in range(30):
        pts = C.grid_pose(17, 50 + 3 * f, 40)
        c = C.case(boxes, pts[None], np.full((1, 17), 0.9), alive=alive, lost=lost)
        boxes, alive, lost = _step(c)
        want = np.array([50 + 3 * f + 14 - 17.5, 40 + 16.5 - 20.625, 50 + 3 * f + 14 + 17.5, 40 + 16.5 + 20.625])
        assert np.allclose(boxes[0], want, atol=1e-3) and boxes.dtype == np.float32 and alive[0] == 1 and lost[0] == 0, f
    assert boxes[0, 0] > 90, "the pose has left the first box entirely"


def test_selection_by_the_prob_and_by_the_conf_gate():
    cs = C.crafted()
    moved = lambda c: not np.array_equal(_step(c)[0], c["boxes"])  # noqa: E731
    assert moved(cs["gate_prob"]) and moved(cs["gate_conf"])
    assert not moved(cs["gate_conf_low"]) and _step(cs["gate_conf_low"])[2][0] == 1
    c = dict(cs["gate_prob"], gate="conf")  # the same records read through the other column
    assert not moved(c)
    b, _, _ = _step(cs["gate_prob"], kpt_thr=0.9)  # the threshold is inclusive
    assert not np.array_equal(b, cs["gate_prob"]["boxes"])
    assert np.array_equal(_step(cs["gate_prob"], kpt_thr=np.nextafter(0.9, 1.0))[0], cs["gate_prob"]["boxes"])


def test_exactly_min_keypoints_and_one_fewer():
    cs = C.crafted()
    b, a, l = _step(cs["exactly_min"])
    assert not np.array_equal(b, cs["exactly_min"]["boxes"]) and (a[0], l[0]) == (1, 0)
    # four keypoints on one row: 21 px wide, no height -> min_side
    assert np.allclose(b[0], [30.5 - 13.125, 20 - 4, 30.5 + 13.125, 20 + 4], atol=1e-3)
    b, a, l = _step(cs["one_short"])
    assert np.array_equal(b, cs["one_short"]["boxes"]) and (a[0], l[0]) == (1, 1)


def test_lost_counts_then_death_and_dead_stays_dead():
    c = C.crafted()["one_short"]
    boxes, alive, lost = c["boxes"], c["alive"], c["lost"]
    for f in range(1, 5):
        boxes, alive, lost = _step(dict(c, boxes=boxes, alive=alive, lost=lost), max_lost=2)
        assert np.array_equal(boxes, c["boxes"])
        assert (alive[0], lost[0]) == ((1, f) if f <= 2 else (0, 3)), (f, alive, lost)  # dies at max_lost + 1, then nothing counts any more
    good = C.crafted()["follow"]
    b, a, l = _step(dict(good, alive=alive, lost=lost), max_lost=2)  # a perfect pose does not revive it
    assert np.array_equal(b, good["boxes"]) and (a[0], l[0]) == (0, 3)
    b, a, l = _step(C.crafted()["last_miss"])
    assert (a[0], l[0]) == (0, 3)
    b, a, l = _step(C.crafted()["dead"])
    assert np.array_equal(b, C.crafted()["dead"]["boxes"]) and (a[0], l[0]) == (0, 3)


def test_collinear_keypoints_get_min_side_and_non_finite_values_are_never_selected():
    cs = C.crafted()
    b, _, _ = _step(cs["collinear"])
    assert np.allclose(b[0], [50 - 4, 26 - 20, 50 + 4, 26 + 20], atol=1e-3)
    assert np.allclose(_step(cs["collinear"], min_side=30.0)[0][0], [50 - 15, 26 - 20, 50 + 15, 26 + 20], atol=1e-3)
    b, a, l = _step(cs["non_finite"])  # keypoints 0 .. 4 carry NaN / +-inf in a coordinate or in the gate: 5 .. 16 remain
    assert np.isfinite(b).all() and np.allclose(b[0], [46, 31 - 13.75, 54, 31 + 13.75], atol=1e-3) and (a[0], l[0]) == (1, 0)
    b2, _, _ = _step(dict(cs["non_finite"], gate="conf"))
    assert np.array_equal(b, b2)
    allbad = dict(cs["non_finite"], records=np.full_like(cs["non_finite"]["records"], np.nan))
    b, a, l = _step(allbad)
    assert np.array_equal(b, allbad["boxes"]) and l[0] == 1


def test_smooth_blends_with_the_old_box_and_zero_is_exactly_the_new_one():
    c = C.crafted()["smooth"]
    new, _, _ = _step(c, smooth=0.0)
    half, _, _ = _step(c)
    want = (0.5 * c["boxes"].astype(np.float64) + 0.5 * np.array([46.5, 56.5 - 20.625, 81.5, 56.5 + 20.625])).astype(np.float32)
    assert np.allclose(half, want, atol=1e-4) and np.allclose(new[0], [46.5, 35.875, 81.5, 77.125], atol=1e-3)
    inf_old = dict(c, boxes=np.array([[0, 0, np.inf, 1]], np.float32), centers=c["centers"], scales=c["scales"])
    assert np.array_equal(_step(inf_old, smooth=0.0)[0], new), "smooth = 0 never reads the old box"


def test_duplicates_the_lower_mean_gate_dies_and_ties_go_by_index():
    cs = C.crafted()
    for name, want in (("dup_tie", [1, 0, 1]), ("dup_first_lower", [0, 1, 1]), ("dup_second_lower", [1, 0, 1])):
        b, a, l, pairs = _step(cs[name], return_oks=True)
        assert a.tolist() == want and l.tolist() == [0, 0, 0], name
        oks = {(i, j): v for i, j, v in pairs}
        assert oks[(0, 1)] > 0.999 and oks[(0, 2)] < 0.01 and oks[(1, 2)] < 0.01
        assert not np.array_equal(b[1], cs[name]["boxes"][1]), "a duplicate's box was updated before it died"
        assert _step(cs[name], dup_oks_thr=1.5)[1].tolist() == [1, 1, 1]
    # three tracks on one pose, gates 0.5 / 0.9 / 0.7: (0, 1) kills 0, (1, 2) kills 2 - and 0, already dead, kills nobody
    pts = np.stack([C.grid_pose(17, 50, 40)] * 3)
    c = C.case([[40, 30, 90, 100]] * 3, pts, np.stack([np.full(17, g) for g in (0.5, 0.9, 0.7)]))
    assert _step(c)[1].tolist() == [0, 1, 0]
    # a track that missed this frame takes no part, whatever its stale pose
    c = C.case([[40, 30, 90, 100]] * 2, pts[:2], np.stack([np.full(17, 0.9), np.full(17, 0.1)]))
    b, a, l = _step(c)
    assert a.tolist() == [1, 1] and l.tolist() == [0, 1]


def test_oks_is_the_reference_formula():
    """``tracking.pose_oks`` against ``evaluation.oks_iou`` (float32 there, another summation order): equal to float32 precision."""
    from probpose_code_amd import tracking
    from probpose_code_amd.evaluation import COCO_SIGMAS, oks_iou

    rng = np.random.default_rng(3)
    for _ in range(20):
        a, b = rng.uniform(0, 200, (17, 2)), None
        b = a + rng.normal(0, 6, (17, 2))
        aa, ab = rng.uniform(500, 5000, 2)
        flat = lambda p: np.concatenate([p, np.ones((17, 1))], 1).reshape(-1)  # noqa: E731
        want = oks_iou(flat(a), flat(b)[None], aa, np.array([ab]), COCO_SIGMAS)[0]
        assert abs(tracking.pose_oks(a, b, aa, ab, COCO_SIGMAS) - want) < 1e-6


def test_tree_sum_is_the_adjacent_pair_tree():
    from probpose_code_amd import tracking

    v = np.random.default_rng(0).uniform(0, 1, 17)
    pad = np.concatenate([v, np.zeros(15)])
    want = ((((pad[0] + pad[1]) + (pad[2] + pad[3])) + ((pad[4] + pad[5]) + (pad[6] + pad[7])))
            + (((pad[8] + pad[9]) + (pad[10] + pad[11])) + ((pad[12] + pad[13]) + (pad[14] + pad[15])))) + ((((pad[16] + 0.0) + 0.0) + 0.0) + 0.0)
    assert tracking._tree_sum(v) == want and tracking._tree_sum(v[:1]) == v[0]


AFFINE_BOXES = np.array([
    [10, 20, 110, 220], [0, 0, 75, 100], [0, 0, 150, 200], [3, 5, 3 + 0.75 * 64, 5 + 64],  # the last three on the tie w == 0.75 h
    [100, 50, 101, 300], [100, 50, 400, 51], [7, 7, 8, 8],                                  # a pixel wide / high
    [-500.5, -300.25, -20, -10], [-3000, -2000, 90000, 70000], [1e6, 1e6, 1e6 + 50, 1e6 + 80], [0.1, 0.2, 33.3, 77.7]], np.float32)


def test_affine_params_host_equals_the_pipeline_arithmetic():
    from probpose_code_amd import tracking
    from probpose_code_amd import transforms as T

    rng = np.random.default_rng(11)
    x0, y0 = rng.uniform(-200, 2000, 200), rng.uniform(-200, 1200, 200)
    rand = np.stack([x0, y0, x0 + rng.uniform(0.5, 900, 200), y0 + rng.uniform(0.5, 900, 200)], -1).astype(np.float32)
    for size, pad in (((192, 256), 1.25), ((288, 384), 1.25), ((192, 256), 1.0), ((100, 300), 1.1)):
        boxes = np.concatenate([AFFINE_BOXES, rand])
        c, s, mats = T.topdown_affine_params(boxes, size, input_padding=pad)
        inv = np.stack([T.invert_affine(m) for m in mats])
        gc, gs, gm = tracking.affine_params_host(boxes, size, pad)
        assert gc.dtype == np.float32 and gs.dtype == np.float32 and gm.dtype == np.float64
        assert np.array_equal(gc.view(np.uint32), c.view(np.uint32)) and np.array_equal(gs.view(np.uint32), s.view(np.uint32)), (size, pad)
        assert np.array_equal(gm.view(np.uint64), inv.view(np.uint64)), (size, pad)


def test_affine_params_are_what_inference_topdown_cuts_with():
    """The val pipeline itself (GetBBoxCenterScale + TopdownAffine.prepare, what ``inference_topdown`` runs per box) gives the same centre and
    scale as ``affine_params_host`` - the two never meet through ``topdown_affine_params``."""
    from probpose_code_amd import tracking
    from probpose_code_amd import transforms as T

    gc, gs, gm = tracking.affine_params_host(AFFINE_BOXES, (192, 256), 1.25)
    for i, bb in enumerate(AFFINE_BOXES):
        r = T.GetBBoxCenterScale()(dict(bbox=bb[None]))
        m = T.TopdownAffine(input_size=(192, 256), use_udp=True).prepare(r)
        assert np.array_equal(r["input_center"], gc[i]) and np.array_equal(r["input_scale"], gs[i])
        assert np.array_equal(T.invert_affine(m), gm[i])


def test_entry_points_refuse_bad_arguments_before_any_launch(lib_built):
    import ctypes

    from probpose_code_amd import _lib

    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)

    def update(n=3, K=17, w=192, h=256, gate=0, ptrs=None, thr=0.3, mk=4, expand=1.25, side=8.0, smooth=0.0, ml=10, dup=0.9, pad=1.25, nxt=(None,) * 3):
        q = ptrs if ptrs is not None else [p] * 12
        return _lib.lib.pp_track_update(q[0], q[1], q[2], n, K, w, h, gate, q[3], q[4], q[5], q[6], thr, mk, expand, side, smooth, ml, dup,
                                        q[7], q[8], q[9], pad, nxt[0], nxt[1], nxt[2], None)

    _lib.reset_launch_counts()
    bad = [dict(n=0), dict(n=65), dict(n=-1), dict(K=0), dict(K=257), dict(w=1), dict(h=40000), dict(gate=2), dict(thr=float("nan")), dict(mk=0),
           dict(expand=0.0), dict(side=0.0), dict(side=float("inf")), dict(smooth=1.0), dict(smooth=-0.1), dict(ml=-1), dict(dup=float("nan")),
           dict(pad=0.0), dict(nxt=(p, None, p))]
    bad += [dict(ptrs=[None if i == k else p for i in range(12)]) for k in range(10)]
    for kw in bad:
        assert update(**kw) == _lib.PP_ERR_INVALID_ARG, kw
        assert b"pp_track_update" in _lib.lib.pp_last_error()
    for args in ((None, 3, 192, 256, 1.25, p, p, p), (p, 3, 192, 256, 1.25, None, p, p), (p, 3, 192, 256, 1.25, p, None, p), (p, 3, 192, 256, 1.25, p, p, None),
                 (p, 0, 192, 256, 1.25, p, p, p), (p, 65, 192, 256, 1.25, p, p, p), (p, 3, 1, 256, 1.25, p, p, p), (p, 3, 192, 256, -1.0, p, p, p)):
        assert _lib.lib.pp_track_affine_params(*args, None) == _lib.PP_ERR_INVALID_ARG, args
    assert _lib.launch_count("pp_track.hip") == 0 and _lib.launch_count("track_update") == 0
