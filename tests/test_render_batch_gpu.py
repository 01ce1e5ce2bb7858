"""GPU: the batched drawing (csrc/pp_render_batch.hip through visualization.draw_datasamples) against the per-sample path
(PoseLocalVisualizer.draw_datasample, itself pinned by tests/test_visualization_gpu.py and tests/fuzz_revert.py): every
picture byte for byte, inside canaries, at every chunking; the launch counts; heatmaps through test_step_stream; and the
pictures of runner.test_dataset(show_dir=...) / tools/test.py --show-dir. No tolerance anywhere."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")
EVAL_CONFIG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_cropcoco-coco-val-256x192.py")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5
GUARD = 4096


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device=DEV)

    def check():
        torch.cuda.synchronize()
        assert bool((torch.cat([buf[:GUARD], buf[GUARD + nbytes:]]) == CANARY).all()), "a kernel wrote outside its buffer"

    return buf[GUARD:GUARD + nbytes], check


def _maps(rng, n, K, h, w):
    """(n, K, h, w) maps, the class by channel: Sparsemax-like sparse, dense Gaussian, all zero, one NaN, one negative value,
    dense again (its presence below 0.75 makes its posterior mass fall short)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.zeros((n, K, h, w), np.float32)
    for i in range(n):
        for k in range(K):
            cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.6, 0.2 * max(h, w) + 0.7)
            g = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32)
            kind = k % 6
            if kind == 0:
                g = np.where(g > 0.6, g - np.float32(0.6), 0).astype(np.float32)
                if g.sum() == 0:
                    g[min(int(cy), h - 1), min(int(cx), w - 1)] = 1
            if kind == 2:
                g[:] = 0
            else:
                g /= g.sum()
            if kind == 3:
                g[int(rng.integers(h)), int(rng.integers(w))] = np.nan
            if kind == 4:
                g[int(rng.integers(h)), int(rng.integers(w))] = -1e-6
            out[i, k] = g
    return out


def _picture(rng, H, W, n, K, hm_hw, windows, heatmap):
    """One picture's inputs: the RGB image, and what both sample forms share. windows: n (centre, scale) activation windows."""
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    kp = np.stack([rng.uniform(-0.3 * W - 3, 1.3 * W + 3, (n, K)), rng.uniform(-0.3 * H - 3, 1.3 * H + 3, (n, K))], -1).astype(np.float64)
    vis = rng.choice(np.array([0.0, 0.29999998, 0.3, 0.7, 1.0], np.float32), (n, K))
    probs = rng.choice(np.array([0.1, 0.74, 0.76, 0.95, 1.0], np.float32), (n, K)) * rng.uniform(0.9, 1.0, (n, K)).astype(np.float32)
    c = rng.uniform(0, 1, (n, 2)) * [W, H]
    s = rng.uniform(0.1, 0.8, (n, 2)) * [W, H] + 1
    boxes = np.concatenate([c - s, c + s], axis=1).astype(np.float32)
    if n == 3:
        boxes[1, 2] = np.nan  # a box that is drawn nowhere
    centers = np.array([w[0] for w in windows], np.float32).reshape(n, 2)
    scales = np.array([w[1] for w in windows], np.float32).reshape(n, 2)
    maps = _maps(rng, n, K, *hm_hw) if heatmap else None
    pad = None
    if heatmap:  # merge_data_samples' padding: every window, plus 10 pixels, inside the canvas
        from probpose_code_amd.structures import _image_padding

        pad = [int(v) for v in _image_padding(centers.astype(np.float64), scales.astype(np.float64), (H, W))]
    return dict(pad=pad, canvas=(H + pad[1] + pad[3], W + pad[0] + pad[2]) if heatmap else (H, W), img=img, kp=kp, vis=vis, probs=probs,
                boxes=boxes, centers=centers, scales=scales, maps=maps, H=H, W=W, n=n)


def _samples(p):
    """(the merged sample of the per-sample path - reverted maps on the host, image_pad, as merge_data_samples leaves them -,
    the sample of the batched path - the un-reverted maps on the device)."""
    from probpose_code_amd.structures import InstanceData, PixelData, PoseDataSample, _image_padding, revert_heatmaps_max

    def base():
        ds = PoseDataSample(metainfo=dict(ori_shape=(p["H"], p["W"]), img_shape=(p["H"], p["W"]), input_center=p["centers"].copy(),
                                          input_scale=p["scales"].copy()))
        if p["n"]:
            ds.pred_instances = InstanceData(keypoints=p["kp"].copy(), keypoints_visible=p["vis"].copy(), bboxes=p["boxes"].copy(),
                                             keypoints_probs=p["probs"].copy())
        return ds

    one, many = base(), base()
    if p["maps"] is not None:
        centers, scales = p["centers"].astype(np.float64), p["scales"].astype(np.float64)
        pad = _image_padding(centers, scales, (p["H"], p["W"]))
        padded = (p["H"] + pad[1] + pad[3], p["W"] + pad[0] + pad[2])
        maps_d = torch.from_numpy(p["maps"]).to(DEV)
        one.pred_fields = PixelData(heatmaps=revert_heatmaps_max(maps_d, centers + pad[:2], scales, padded).cpu().numpy())
        one.set_metainfo(dict(image_pad=pad))
        many.pred_fields = PixelData(heatmaps=maps_d)
    return one, many


def _mixed_batch(K, hm_hw, seed):
    """Six pictures on either side of the 256-pixel row tile; 0, 1 and 3 instances; with and without maps; windows inside the
    image, across each border and wholly outside it."""
    rng = np.random.default_rng(seed)
    spec = [  # H, W, heatmap, windows
        (1, 1, True, [((0.5, 0.5), (30, 40))]),                                                          # across all four borders
        (5, 255, True, [((-90, 2), (40, 53)), ((250, 3), (60, 80)), ((120, -60), (30, 40))]),            # left of / across the right / above
        (7, 256, False, []),                                                                             # no instance: the image itself
        (33, 257, False, [((100, 16), (60, 80))]),
        (64, 48, True, [((24, 32), (18, 24)), ((3, 5), (30, 40)), ((45, 60), (30, 40))]),                # inside, top-left, bottom-right
        (120, 90, True, [((45, 60), (48, 64))]),                                                         # inside: no padding at all
    ]
    pics = [_picture(rng, H, W, len(wins), K, hm_hw, wins, hm) for H, W, hm, wins in spec]
    assert pics[5]["pad"] == [0, 0, 0, 0] and min(pics[0]["pad"]) > 0 and pics[1]["pad"][0] > 90 and pics[1]["pad"][1] > 60
    assert all(v > 0 for v in pics[4]["pad"]) and pics[1]["pad"][2] > 0
    return pics


def _visualizer(K):
    from probpose_code_amd import visualization as V

    vis = V.PoseLocalVisualizer(radius=3, line_width=2, alpha=0.8, device=DEV)
    if K != 17:
        vis.set_dataset_meta(dict(skeleton_links=[(0, 1), (1, 2)], skeleton_link_colors=[(255, 0, 0), (0, 0, 255)],
                                  keypoint_colors=[(255, 128, 0), (0, 255, 0), (51, 153, 255)][:K]))
    return vis


def _reference(vis, pics, ones, draw_bbox, kpt_thr):
    return [vis.draw_datasample(p["img"], one, draw_bbox=bb, draw_heatmap=True, kpt_thr=t).cpu().numpy()
            for p, one, bb, t in zip(pics, ones, draw_bbox, kpt_thr)]


@pytest.fixture(scope="module")
def mixed():
    """The K = 17 batch with its per-sample pictures (computed once, read-only)."""
    pics = _mixed_batch(17, (64, 48), seed=7)
    pairs = [_samples(p) for p in pics]
    vis = _visualizer(17)
    draw_bbox = [True, True, True, False, False, True]
    want = _reference(vis, pics, [a for a, _ in pairs], draw_bbox, [0.3] * 6)
    for w in want:
        w.setflags(write=False)
    return dict(pics=pics, many=[b for _, b in pairs], ones=[a for a, _ in pairs], vis=vis, draw_bbox=draw_bbox, want=want)


def _bgr(p):
    return np.ascontiguousarray(p["img"][:, :, ::-1])


def _draw_guarded(vis, pics, many, draw_bbox, kpt_thr, images, **kw):
    from probpose_code_amd import visualization as V

    shapes = [((2 * p["H"] if p["maps"] is not None else p["H"]), p["W"], 3) for p in pics]
    guarded = [_guarded(int(np.prod(s))) for s in shapes]
    outs = [g[0].view(s) for g, s in zip(guarded, shapes)]
    plan = V.plan_render_chunks([(p["H"], p["W"]) for p in pics], [p["pad"] for p in pics], len(vis.kpt_color),
                                kw.get("scratch_bytes", V.RENDER_SCRATCH_DEFAULT))
    scratch, check_scratch = _guarded(max(max(c["scratch_bytes"] for c in plan), 1))
    got = vis.draw_datasamples(images, many, draw_bbox=draw_bbox, draw_heatmap=True, kpt_thr=kpt_thr, channel_order="bgr", out=outs,
                               scratch=scratch, **kw)
    for _, check in guarded:
        check()
    check_scratch()
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
    return [g.cpu().numpy() for g in got]


@pytest.mark.parametrize("K,hm_hw", [(17, (64, 48)), (3, (2, 2))])
def test_mixed_batch_equals_the_per_sample_pictures(K, hm_hw, mixed):
    """The per-sample path gets the RGB image, the batch the same image as BGR (host arrays and device tensors mixed), one
    kpt_thr per picture (0, 0.3, 1: the call is cut where it changes), draw_bbox on and off."""
    if K == 17:
        pics, many, ones, vis = mixed["pics"], mixed["many"], mixed["ones"], mixed["vis"]
    else:
        pics = _mixed_batch(K, hm_hw, seed=11)
        ones, many = zip(*[_samples(p) for p in pics])
        vis = _visualizer(K)
    draw_bbox = [True, True, True, False, False, True]
    kpt_thr = [0.0, 0.0, 0.3, 0.3, 1.0, 1.0]
    want = _reference(vis, pics, ones, draw_bbox, kpt_thr)
    images = [_bgr(p) if i % 2 else torch.from_numpy(_bgr(p)).to(DEV) for i, p in enumerate(pics)]
    got = _draw_guarded(vis, pics, many, draw_bbox, kpt_thr, images)
    for i, (g, w, p) in enumerate(zip(got, want, pics)):
        assert g.shape == w.shape == ((2 * p["H"] if p["maps"] is not None else p["H"]), p["W"], 3)
        assert np.array_equal(g, w), f"picture {i} {(p['H'], p['W'])}: {int((g != w).any(-1).sum())} pixels differ"
    assert np.array_equal(got[2], pics[2]["img"])  # no instance, no panel: the image, as RGB
    assert not np.array_equal(got[5][:120], pics[5]["img"]) and not np.array_equal(got[5][120:], pics[5]["img"])  # something was drawn


def test_chunking_does_not_change_a_byte(mixed):
    from probpose_code_amd import visualization as V

    pics, many, vis, want = mixed["pics"], mixed["many"], mixed["vis"], mixed["want"]
    images = [torch.from_numpy(_bgr(p)).to(DEV) for p in pics]
    before = [(im.clone(), m.pred_fields.heatmaps.clone() if p["maps"] is not None else None) for im, m, p in zip(images, many, pics)]
    s0, s1, s4, s5 = (V.render_share_bytes(17, *pics[i]["canvas"]) for i in (0, 1, 4, 5))  # the panel pictures
    calls = []
    # every panel picture in its own chunk; two chunks (pictures 0 and 1 fit, all four do not, 4 and 5 fit); one
    for budget in (1, max(s0 + s1, s4 + s5), V.RENDER_SCRATCH_DEFAULT):
        c0 = V.batch_calls
        got = _draw_guarded(vis, pics, many, mixed["draw_bbox"], 0.3, images, scratch_bytes=budget)
        calls.append(V.batch_calls - c0)
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), f"budget {budget}: picture {i} differs"
    assert calls == [4, 2, 1], calls
    again = _draw_guarded(vis, pics, many, mixed["draw_bbox"], 0.3, images)
    assert all(np.array_equal(a, w) for a, w in zip(again, want))  # a second call: the same bytes
    for (im0, hm0), im, m in zip(before, images, many):  # the inputs are untouched
        assert torch.equal(im0, im) and (hm0 is None or torch.equal(hm0.view(torch.int32), m.pred_fields.heatmaps.view(torch.int32)))


def test_launch_count_does_not_depend_on_the_number_of_pictures(mixed):
    from probpose_code_amd import _lib
    from probpose_code_amd import visualization as V

    pics, many, vis = mixed["pics"], mixed["many"], mixed["vis"]

    def tally(sel, **kw):
        _lib.reset_launch_counts()
        u0 = V.batch_uploads
        vis.draw_datasamples([_bgr(pics[i]) for i in sel], [many[i] for i in sel], draw_heatmap=True, channel_order="bgr", **kw)
        torch.cuda.synchronize()
        assert _lib.launch_count("pp_render.hip") == 0 and _lib.launch_count("pp_warp.hip") == 0
        return _lib.launch_count("pp_render_batch.hip"), V.batch_uploads - u0

    one = tally([4])
    eight = tally([4, 0, 1, 2, 3, 5, 4, 1])
    assert one == eight == (len(V.RENDER_BATCH_LAUNCHES), 1), (one, eight)
    two = tally([4, 4], scratch_bytes=V.render_share_bytes(17, *pics[4]["canvas"]))  # one share fits, two do not
    assert two == (2 * one[0], 2), two
    assert tally([2, 3]) == (1, 1)  # no panel in the call: the pose panel alone


def _fields(samples):
    out = []
    for s in samples:
        d = {k: np.asarray(v) for k, v in s.pred_instances.all_items()}
        d["heatmaps"] = s.pred_fields.heatmaps
        out.append(d)
    return out


def test_test_step_stream_carries_the_heatmaps():
    """Batches of 3 (eager) and 4 (the slots' graphs), several of each so that both slots are reused: pred_fields.heatmaps and
    every pred_instances field equal test_step's, bit for bit."""
    from probpose_code_amd import apis
    from probpose_code_amd import synthetic as S

    model = apis.init_model(CFG, dict(state_dict=S.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device=DEV,
                            cfg_options={"model.test_cfg.output_heatmaps": True})
    sizes = [3, 4, 4, 3, 4, 3, 4]
    rng = np.random.default_rng(5)
    batches = []
    for i, n in enumerate(sizes):
        center = np.stack([rng.uniform(80, 400, n), rng.uniform(100, 500, n)], -1).astype(np.float32)
        scale = (np.array([192, 256], np.float32) * rng.uniform(0.8, 2.5, (n, 1)).astype(np.float32) * 1.25).astype(np.float32)
        batches.append((S.synthetic_crops(n, seed=60 + i), center, scale))
    with torch.no_grad():
        want = []
        for c, ce, s in batches:
            want.append(_fields(model.test_step(apis.pack_crops(c, ce, s, model.dataset_meta))))
            want[-1] = [dict(d, heatmaps=d["heatmaps"].clone()) for d in want[-1]]
        torch.cuda.synchronize()
        got = [_fields(r) for r in model.test_step_stream((apis.pack_crops(c, ce, s, model.dataset_meta) for c, ce, s in batches), depth=2,
                                                          max_batch=4)]
        torch.cuda.synchronize()
    assert any(k[0] == 4 and k[3] is True and k[-1] == 1 for k in model.engine._graphs), "the full batches did not replay a heatmap graph"
    assert [len(g) for g in got] == sizes
    for b, (g, w) in enumerate(zip(got, want)):
        for x, y in zip(g, w):
            assert x.keys() == y.keys()
            for f in x:
                if f == "heatmaps":
                    assert x[f].is_cuda and x[f].shape == (17, 64, 48) and torch.equal(x[f].view(torch.int32), y[f].view(torch.int32)), f"batch {b}"
                else:
                    assert x[f].dtype == y[f].dtype and x[f].tobytes() == y[f].tobytes(), f"batch {b}: {f}"
    assert not torch.equal(got[1][0]["heatmaps"], got[2][0]["heatmaps"]), "a replay repeated the previous batch's maps"


def _same(a, b):
    return a.keys() == b.keys() and all((isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k] for k in a)


@pytest.fixture(scope="module")
def show_run(tmp_path_factory):
    """Six images (three .jpg, three .png; 1 - 3 persons each), batch_size 4, depth 2, output_heatmaps on: a run without show_dir,
    one with, and a second one into the same directory."""
    from probpose_code_amd import apis, runner
    from probpose_code_amd import synthetic as S
    from probpose_code_amd.config import Config
    from probpose_code_amd.datasets import build_dataset

    tmp = tmp_path_factory.mktemp("show_dir")
    roots = [str(tmp / "cropcoco") + "/", str(tmp / "coco") + "/"]
    n = S.synthetic_coco_dataset(roots[0], 3, seed=3, image_size=(160, 120), fmt="jpg", persons=(1, 3), invalid_image=False, id_base=1)
    n += S.synthetic_coco_dataset(roots[1], 3, seed=4, image_size=(160, 120), fmt="png", persons=(1, 3), invalid_image=False, id_base=2)
    opts = {f"test_dataloader.dataset.datasets.{i}.data_root": r for i, r in enumerate(roots)}
    cfg = Config.fromfile(EVAL_CONFIG)
    cfg.merge_from_dict(dict(opts, **{"model.test_cfg.output_heatmaps": True}))
    model = apis.init_model(cfg, dict(state_dict=S.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device=DEV)
    dataset = build_dataset(cfg.test_dataloader.dataset)
    assert len(dataset) == n and 6 <= n <= 18

    def run(show_dir):
        batches = []
        metrics = runner.test_dataset(model, dataset, runner.build_evaluator(cfg.test_evaluator, dataset, device=DEV), batch_size=4, workers=4,
                                      depth=2, sink=batches.append, show_dir=show_dir)
        torch.cuda.synchronize()
        return metrics, [s for b in batches for s in b]

    show_dir = str(tmp / "pictures")
    plain = run(None)
    shown = run(show_dir)
    first = sorted(os.listdir(show_dir))
    again = run(show_dir)
    return dict(tmp=tmp, roots=roots, opts=opts, cfg=cfg, model=model, dataset=dataset, n=n, plain=plain, shown=shown, again=again, first=first,
                show_dir=show_dir)


def test_show_dir_pictures_are_the_per_sample_pictures(show_run):
    from PIL import Image

    from probpose_code_amd import jpeg, png, runner
    from probpose_code_amd import visualization as V
    from probpose_code_amd.apis import load_image_bgr
    from probpose_code_amd.structures import merge_data_samples

    dataset, n, show_dir = show_run["dataset"], show_run["n"], show_run["show_dir"]
    (m_plain, s_plain), (m_shown, s_shown) = show_run["plain"], show_run["shown"]
    assert _same(m_plain, m_shown) and _same(m_plain, show_run["again"][0]) and len(s_plain) == len(s_shown) == n
    for a, b in zip(_fields(s_plain), _fields(s_shown)):  # the samples given to the sink do not change
        for f in a:
            assert (torch.equal(a[f], b[f]) if f == "heatmaps" else a[f].tobytes() == b[f].tobytes()), f
    paths = [dataset.get_data_info(i)["img_path"] for i in range(n)]
    names = runner.show_file_names(paths, [])
    assert show_run["first"] == sorted(names) and len(set(names)) == n
    assert n > len(set(paths)), "no image with several instances"
    vis = V.PoseLocalVisualizer(device=DEV)
    vis.set_dataset_meta(show_run["model"].dataset_meta)
    for path, name, sample in zip(paths, names, s_shown):
        rgb = np.ascontiguousarray(load_image_bgr(path)[:, :, ::-1])
        frame = vis.draw_datasample(rgb, merge_data_samples([sample]), draw_bbox=True, draw_heatmap=True, kpt_thr=0.3)
        assert frame.shape == (240, 160, 3)
        if name.endswith(".jpg"):
            want = jpeg.encode_batch([frame], quality=75, subsampling="4:2:0", channel_order="rgb", entropy="device")[0]
        else:
            want = png.encode_batch([frame], channel_order="rgb")[0]
        with open(os.path.join(show_dir, name), "rb") as f:
            assert f.read() == want, name
        with Image.open(os.path.join(show_dir, name)) as im:
            assert im.size == (160, 240)
            if name.endswith(".png"):
                assert np.array_equal(np.asarray(im), frame.cpu().numpy())
    # the second run into the same directory continues the indices
    assert sorted(os.listdir(show_dir)) == sorted(names + runner.show_file_names(paths, show_run["first"])) and len(os.listdir(show_dir)) == 2 * n


def test_show_dir_without_heatmaps_is_the_pose_panel(show_run, tmp_path):
    from PIL import Image

    from probpose_code_amd import jpeg, runner
    from probpose_code_amd import visualization as V
    from probpose_code_amd.apis import load_image_bgr
    from probpose_code_amd.structures import merge_data_samples

    model, dataset, n = show_run["model"], show_run["dataset"], show_run["n"]
    samples = []
    model.test_cfg["output_heatmaps"] = False
    try:
        runner.test_dataset(model, dataset, None, batch_size=4, workers=4, depth=2, sink=samples.extend, show_dir=str(tmp_path / "p"))
    finally:
        model.test_cfg["output_heatmaps"] = True
    paths = [dataset.get_data_info(i)["img_path"] for i in range(n)]
    names = runner.show_file_names(paths, [])
    assert sorted(os.listdir(tmp_path / "p")) == sorted(names)
    for name in names:
        with Image.open(tmp_path / "p" / name) as im:
            assert im.size == (160, 120), name
    vis = V.PoseLocalVisualizer(device=DEV)
    vis.set_dataset_meta(model.dataset_meta)
    assert "pred_fields" not in samples[0]
    frame = vis.draw_datasample(np.ascontiguousarray(load_image_bgr(paths[0])[:, :, ::-1]), merge_data_samples([samples[0]]), draw_heatmap=True)
    with open(tmp_path / "p" / names[0], "rb") as f:
        assert f.read() == jpeg.encode_batch([frame], quality=75, subsampling="4:2:0", channel_order="rgb", entropy="device")[0]


def test_tools_test_cli_show_dir(show_run, tmp_path):
    """tools/test.py --show-dir in a child process: the metrics file equals the run without the flag, one picture per instance."""
    from PIL import Image

    out, pictures = tmp_path / "m.json", tmp_path / "cli_pictures"
    opts = dict(show_run["opts"], **{"model.test_cfg.output_heatmaps": True})
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "test.py"), EVAL_CONFIG, "synthetic", "--cfg-options"] + \
          [f"{k}={v}" for k, v in opts.items()] + ["--out", str(out), "--workers", "4", "--batch-size", "4", "--show-dir", str(pictures)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert _same(json.load(open(out)), show_run["plain"][0])
    names = sorted(os.listdir(pictures))
    assert names == show_run["first"]
    for name in names:
        with Image.open(pictures / name) as im:
            assert im.size == (160, 240), name
