"""GPU: the --draw-heatmap drawing (csrc/pp_render.hip through probpose_code_amd/visualization.py) against the numpy
restatement of tests/render_ref.py - thresholds bit for bit, every drawn byte equal - with canary bytes around every
output buffer and two runs compared; then the whole path from inference_topdown to the (2H, W, 3) picture, and the demo."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import render_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5
GUARD = 4096


def _guarded(shape, dtype):
    """A device tensor of ``shape`` inside a buffer with GUARD canary bytes on both sides: (view, check())."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    view = buf[GUARD:GUARD + n].view(dtype).view(shape)

    def check():
        torch.cuda.synchronize()
        edge = torch.cat([buf[:GUARD], buf[GUARD + n:]])
        assert bool((edge == CANARY).all()), "a kernel wrote outside its output buffer"

    return view, check


def _thresholds_raw(maps_d):
    from probpose_code_amd import _lib

    K, H, W = maps_d.shape
    scratch = torch.empty(int(_lib.lib.pp_parea_scratch_bytes(K, H, W)), dtype=torch.uint8, device=DEV)
    thr, c1 = _guarded((K,), torch.float32)
    draw, c2 = _guarded((K,), torch.int32)
    _lib.call("pp_parea_thresholds", maps_d.data_ptr(), K, H, W, scratch.data_ptr(), thr.data_ptr(), draw.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    c1()
    c2()
    return thr.cpu().numpy(), draw.cpu().numpy()


def _special_maps(H, W, seed):
    """The hand-made cases of the CPU test at size (H, W), then posterior-like maps up to K = 17."""
    z = np.zeros((H, W), np.float32)
    cases = []
    m = z.copy()  # ties at the threshold
    m.flat[:2] = 0.25
    m.flat[5:9] = 0.125
    m.flat[20:24] = 0.0625
    cases.append(m)
    m = z.copy()  # single hot pixel
    m[H // 2, W // 3] = 1.0
    cases.append(m)
    m = np.full((H, W), 2.0 ** -24, np.float32)  # spike over a floor
    m[1, 1] = 0.9
    cases.append(m)
    m = z.copy()  # total just below 0.75
    m[0, 0], m[-1, -1] = 0.5, 0.25 - 2.0 ** -12
    cases.append(m)
    m = m.copy()  # just above
    m[-1, -1] = 0.25 + 2.0 ** -12
    cases.append(m)
    cases.append(z.copy())  # all zero
    m = R.posterior_like_maps(1, H, W, seed)[0]
    m[3, 4] = np.nan
    cases.append(m)
    m = R.posterior_like_maps(1, H, W, seed + 1)[0]
    m[0, 2] = -1e-6
    cases.append(m)
    m = R.posterior_like_maps(1, H, W, seed + 2)[0]  # many ties: values quantised
    cases.append((np.round(m / m.max() * 50) * (m.max() / 50)).astype(np.float32))
    m = R.posterior_like_maps(1, H, W, seed + 3)[0]
    m[m < np.quantile(m, 0.5)] = -0.0  # negative zeros are zeros
    cases.append(m)
    rest = R.posterior_like_maps(17 - len(cases), H, W, seed + 10)
    return np.concatenate([np.stack(cases), rest])


@pytest.mark.parametrize("H,W", [(64, 48), (270, 360), (1080 + 61 + 75, 1920 + 90 + 37)])
def test_thresholds_bit_exact_and_deterministic(H, W):
    maps = _special_maps(H, W, seed=H)
    want_t, want_d = R.thresholds(maps)
    assert list(want_d[:8]) == [1, 1, 1, 0, 1, 0, 0, 0]
    maps_d = torch.from_numpy(maps).to(DEV)
    t1, d1 = _thresholds_raw(maps_d)
    t2, d2 = _thresholds_raw(maps_d)
    assert np.array_equal(d1, want_d)
    assert np.array_equal(t1[want_d == 1].view(np.uint32), want_t[want_d == 1].view(np.uint32))
    assert np.array_equal(t1.view(np.uint32), t2.view(np.uint32)) and np.array_equal(d1, d2)


def _image(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("H,W,pad", [(64, 48, (5, 7, 3, 0)), (270, 360, (40, 12, 0, 55))])
def test_compose_and_resize_byte_equal(H, W, pad):
    from probpose_code_amd import visualization as V

    Hp, Wp = H + pad[1] + pad[3], W + pad[0] + pad[2]
    maps = R.posterior_like_maps(17, Hp, Wp, seed=W)
    maps[4] *= 0.5  # below 0.75: not drawn
    img = _image(H, W, 1)
    boxes = np.array([[10, 5, W * 0.6, H * 0.7], [-30, H * 0.5, W + 20, H + 40], [W * 0.3, -50, W * 0.5, H * 0.2]], np.float32)
    maps_d = torch.from_numpy(maps).to(DEV)
    outs = []
    for _ in range(2):
        canvas, check = _guarded((Hp, Wp, 3), torch.uint8)
        V.render_probability_areas(maps_d, img, pad, boxes, out=canvas)
        check()
        outs.append(canvas.cpu().numpy())
    thr, draw = R.thresholds(maps)
    want = R.compose(img, pad, maps, thr, draw, R.aspect_boxes(boxes, pad))
    assert np.array_equal(outs[0], want), f"{int((outs[0] != want).any(-1).sum())} canvas pixels differ"
    assert np.array_equal(outs[0], outs[1])
    for h, w in ((H, W), (max(H // 3, 1), max(W // 2, 1)), (H + 17, W * 2)):  # the panel size, a shrink, an enlargement
        dst, check = _guarded((h, w, 3), torch.uint8)
        V.resize_rgb(torch.from_numpy(want).to(DEV), (h, w), out=dst)
        check()
        assert np.array_equal(dst.cpu().numpy(), R.resize(want, h, w)), (h, w)


def _instances(n, H, W, seed):
    rng = np.random.default_rng(seed)
    kp = np.empty((n, 17, 2), np.float32)
    kp[..., 0] = rng.uniform(-0.2 * W, 1.2 * W, (n, 17))  # some off the image
    kp[..., 1] = rng.uniform(-0.2 * H, 1.2 * H, (n, 17))
    vis = rng.uniform(0, 1, (n, 17)).astype(np.float32)
    vis[:, 0] = 1.0
    c = rng.uniform(0, 1, (n, 2)) * [W, H]
    s = rng.uniform(0.1, 0.8, (n, 2)) * [W, H]
    boxes = np.concatenate([c - s, c + s], axis=1).astype(np.float32)  # overhanging the border
    return kp, vis, boxes


@pytest.mark.parametrize("n,kpt_thr,radius,thickness", [(1, 0.3, 3, 1), (4, 0.0, 3, 3), (8, 1.0, 5, 2)])
def test_draw_poses_byte_equal(n, kpt_thr, radius, thickness):
    from probpose_code_amd import visualization as V

    H, W = 240, 320
    img = _image(H, W, n)
    kp, vis, boxes = _instances(n, H, W, seed=10 + n)
    outs = []
    for _ in range(2):
        out, check = _guarded((H, W, 3), torch.uint8)
        V.draw_poses(torch.from_numpy(img).to(DEV), kp, vis, boxes, kpt_thr=kpt_thr, radius=radius, thickness=thickness, alpha=0.8,
                     out=out)
        check()
        outs.append(out.cpu().numpy())
    want = R.draw_poses(img, kp, vis, R.int_boxes(boxes), V.COCO_SKELETON, V.COCO_LINK_COLORS, V.COCO_KEYPOINT_COLORS, kpt_thr,
                        radius, thickness, 0.8)
    assert np.array_equal(outs[0], want), f"{int((outs[0] != want).any(-1).sum())} pixels differ"
    assert np.array_equal(outs[0], outs[1])
    assert not np.array_equal(want, img)


CFG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")
IMG = os.path.join(ROOT, "demo", "resources", "synthetic_person.png")


def test_end_to_end_picture_equals_the_restatement(tmp_path):
    from probpose_code_amd import apis, synthetic
    from probpose_code_amd import visualization as V
    from probpose_code_amd.structures import merge_data_samples, posterior_heatmaps
    from probpose_code_amd.apis import load_image_bgr

    model = apis.init_model(CFG, dict(state_dict=synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device=DEV,
                            cfg_options={"model.test_cfg.output_heatmaps": True})
    rgb = np.ascontiguousarray(load_image_bgr(IMG)[:, :, ::-1])
    H, W = rgb.shape[:2]
    boxes = np.array([[0.2 * W, 0.1 * H, 0.8 * W, 0.9 * H], [0.6 * W, 0.55 * H, 1.3 * W, 1.25 * H]], np.float32)  # one off the image
    merged = merge_data_samples(apis.inference_topdown(model, IMG, boxes))
    pad = np.asarray(merged.metainfo["image_pad"])
    assert pad[2] > 0 and pad[3] > 0
    vis = V.PoseLocalVisualizer(radius=3, line_width=1, alpha=0.8)
    vis.set_dataset_meta(model.dataset_meta)
    out_file = str(tmp_path / "picture.png")
    got = vis.add_datasample("result", rgb, merged, draw_heatmap=True, kpt_thr=0.3, out_file=out_file)
    assert got.shape == (2 * H, W, 3) and got.dtype == np.uint8 and got is vis.get_image()
    pi = merged.pred_instances
    maps = posterior_heatmaps(merged.pred_fields.heatmaps, pi.keypoints_probs).cpu().numpy()
    want = R.render(rgb, pi.keypoints, pi.keypoints_visible, pi.bboxes, maps, pad, merged.gt_instances.bboxes, V.COCO_SKELETON,
                    V.COCO_LINK_COLORS, V.COCO_KEYPOINT_COLORS)
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} pixels differ"
    thr, draw = R.thresholds(maps)
    assert draw.any()
    border = np.ones(maps.shape[1:], bool)
    border[pad[1]:pad[1] + H, pad[0]:pad[0] + W] = False
    in_border = [int(((maps[k] > thr[k]) & border).sum()) for k in range(len(maps)) if draw[k]]
    print(f"area pixels in the padded border per drawn keypoint: {in_border}")
    assert max(in_border) > 0
    from PIL import Image

    with Image.open(out_file) as im:
        assert np.array_equal(np.asarray(im), got)


def test_demo_writes_the_picture(tmp_path):
    out_img, out_json = str(tmp_path / "demo.png"), str(tmp_path / "demo.json")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "demo", "image_demo.py"), IMG, CFG, "synthetic",
                        "--draw-heatmap", "--out-img", out_img, "--out-file", out_json, "--bboxes", "40,30,220,330;150,200,330,420"],
                       capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    from PIL import Image

    with Image.open(out_img) as im:
        assert im.size == (270, 2 * 360) and im.mode == "RGB"
    assert os.path.getsize(out_json) > 0
