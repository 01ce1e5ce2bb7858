"""CPU: the --draw-heatmap drawing (probpose_code_amd/visualization.py, csrc/pp_render.hip) - its C entry points are
exported and validate their arguments before touching a device; the numpy fp64 threshold of tests/render_ref.py (the
yardstick of the GPU tests) agrees with the reference's literal float32 sort / cumsum / searchsorted form; the demo's new
flags; the options the visualizer refuses."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import render_ref as R  # noqa: E402

NEW_SYMBOLS = ("pp_parea_scratch_bytes", "pp_parea_thresholds", "pp_parea_compose", "pp_draw_poses", "pp_resize_bilinear_u8")


def test_render_symbols_exported_under_abi_4(lib_built):
    from probpose_code_amd import _lib

    so = ctypes.CDLL(lib_built)
    for name in NEW_SYMBOLS:
        assert hasattr(so, name) and name in _lib.SIGNATURES
    assert _lib.lib.pp_abi_version() == 4


def test_render_argument_validation_without_gpu(lib_built):
    from probpose_code_amd import _lib

    L = _lib.lib
    bad = _lib.PP_ERR_INVALID_ARG
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)  # never dereferenced: the checks fail first
    # thresholds: NULL pointers, K > 22, non-positive sizes
    assert L.pp_parea_thresholds(None, 17, 8, 8, p, p, p, None) == bad
    assert L.pp_parea_thresholds(p, 17, 8, 8, p, None, p, None) == bad
    assert L.pp_parea_thresholds(p, 23, 8, 8, p, p, p, None) == bad
    assert b"K <= 22" in L.pp_last_error()
    assert L.pp_parea_thresholds(p, 17, 0, 8, p, p, p, None) == bad
    assert L.pp_parea_thresholds(p, 0, 8, 8, p, p, p, None) == bad
    assert L.pp_parea_scratch_bytes(23, 8, 8) == bad and L.pp_parea_scratch_bytes(17, -1, 8) == bad
    assert L.pp_parea_scratch_bytes(17, 8, 8) > 0
    assert L.pp_parea_thresholds(p, 1, 1 << 15, 1 << 14, p, p, p, None) == _lib.PP_ERR_UNSUPPORTED  # 2^29 values
    # compose: NULLs, K, sizes, the padded image must fit the canvas
    ok = (p, 10, 12, 2, 3, p, 17, p, p, p, 1, p, 15, 16, None)
    for i, v in ((0, None), (5, None), (7, None), (8, None), (9, None), (11, None)):
        a = list(ok)
        a[i] = v
        assert L.pp_parea_compose(*a) == bad, i
    for i, v in ((6, 23), (6, 0), (1, 0), (2, -3), (12, 0), (13, 0), (10, -1)):
        a = list(ok)
        a[i] = v
        assert L.pp_parea_compose(*a) == bad, (i, v)
    for i, v in ((3, 5), (4, 6), (3, -1), (12, 12)):  # pad + image beyond the canvas (3 + 10 > 12), negative pad
        a = list(ok)
        a[i] = v
        assert L.pp_parea_compose(*a) == bad, (i, v)
        assert b"does not fit" in L.pp_last_error()
    # pose drawing and resize
    pose = [p, 10, 12, p, p, p, 2, 17, p, p, p, 19, 0.3, 3.0, 1.0, 0.8, p, None]
    for i, v in ((0, None), (16, None), (3, None), (8, None), (1, 0), (7, 0), (6, -1), (13, -1.0)):
        a = list(pose)
        a[i] = v
        assert L.pp_draw_poses(*a) == bad, (i, v)
    assert L.pp_resize_bilinear_u8(None, 4, 4, p, 2, 2, None) == bad
    assert L.pp_resize_bilinear_u8(p, 4, 4, p, 0, 2, None) == bad


def _agree(m):
    t64, d = R.threshold_fp64(m)
    t32 = R.threshold_reference_f32(m)
    assert d == (t32 is not None)
    if d:
        assert t64 == t32, (t64, t32)
    return t64, d


def test_fp64_threshold_equals_the_reference_form_on_hand_made_maps():
    z = np.zeros((6, 7), np.float32)
    # ties at the threshold: four values 0.125 straddle the 0.75 quantile of the mass
    m = z.copy()
    m[0, :2] = 0.25
    m[1, :4] = 0.125
    m[2, :4] = 0.0625
    t, d = _agree(m)
    assert d == 1 and t == np.float32(0.125)  # target 0.9375 of 1.25 is reached at the fourth of the tied 0.125s
    assert (m > t).sum() == 2  # strict mask: the tied values themselves are out
    # one hot pixel
    m = z.copy()
    m[3, 5] = 1.0
    assert _agree(m) == (np.float32(1.0), 1) and (m > 1.0).sum() == 0
    # spike over a floor
    m = np.full((6, 7), 2.0 ** -10, np.float32)
    m[2, 2] = 0.9
    assert _agree(m) == (np.float32(0.9), 1)
    # total just below / just above 0.75 (dyadic values: exact in both forms)
    m = z.copy()
    m[0, 0], m[0, 1] = 0.5, 0.25 - 2.0 ** -12
    assert _agree(m)[1] == 0
    m[0, 1] = 0.25 + 2.0 ** -12
    assert _agree(m) == (np.float32(0.25 + 2.0 ** -12), 1)
    # all zero: not drawn
    assert _agree(z)[1] == 0
    # ours only: NaN / negative values are not drawn
    m = np.full((6, 7), 0.05, np.float32)
    m[1, 1] = np.nan
    assert R.threshold_fp64(m)[1] == 0
    m[1, 1] = -1e-3
    assert R.threshold_fp64(m)[1] == 0


def test_fp64_and_float32_masks_agree_on_1080p_maps():
    """The fp64 contract against the reference's float32 cumsum on posterior-like maps of a padded 1080p frame: the masks
    differ in at most 1 % of their pixels (float32 cumsum over ~2.5 M values drifts)."""
    maps = R.posterior_like_maps(4, 1080 + 96, 1920 + 128, seed=3)
    diff = total = 0
    for m in maps:
        t64, d = R.threshold_fp64(m)
        t32 = R.threshold_reference_f32(m)
        assert d == 1 and t32 is not None
        a, b = m > t64, m > t32
        diff += int((a != b).sum())
        total += int(a.sum())
    print(f"fp64 vs reference float32 masks: {diff} of {total} mask pixels differ")
    assert diff <= 0.01 * total


def test_restated_resize_is_identity_at_equal_size():
    img = np.random.default_rng(0).integers(0, 256, (9, 13, 3), dtype=np.uint8)
    assert np.array_equal(R.resize(img, 9, 13), img)


def test_demo_help_lists_the_drawing_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo", "image_demo.py"), "--help"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    for flag in ("--out-img", "--draw-heatmap", "--kpt-thr", "--radius", "--thickness", "--alpha", "--out-file"):
        assert flag in r.stdout, flag


def test_visualizer_refuses_options_outside_probpose(lib_built):
    from probpose_code_amd.structures import PoseDataSample
    from probpose_code_amd.visualization import COCO_SKELETON, PoseLocalVisualizer

    v = PoseLocalVisualizer(radius=3, line_width=1, alpha=0.8)
    img = np.zeros((4, 4, 3), np.uint8)
    ds = PoseDataSample()
    for kw in (dict(draw_gt=True), dict(show_kpt_idx=True), dict(skeleton_style="openpose"), dict(show=True)):
        with pytest.raises(NotImplementedError):
            v.add_datasample("x", img, ds, **kw)
    with pytest.raises(NotImplementedError):
        v.set_dataset_meta({}, skeleton_style="openpose")
    for dt in ("featmap", "contours"):
        with pytest.raises(NotImplementedError):
            v.draw_instance_heatmap(None, img, [0, 0, 0, 0], draw_type=dt)
    v.set_dataset_meta({"num_keypoints": 17})
    assert v.skeleton == COCO_SKELETON and len(v.kpt_color) == 17 and len(v.link_color) == len(COCO_SKELETON)
    with pytest.raises(RuntimeError):
        PoseLocalVisualizer(device="cpu")
