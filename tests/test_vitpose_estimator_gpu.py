"""GPU: the ViTPose baseline end to end - configs/td-hm_ViTPose-small_mi355x_coco-256x192.py with synthetic weights
(HeatmapHead: ProbPose's backbone and heatmap branch, no towers; UDP-DARK decode in pp_udp_heatmap_decode).

(a) the heatmaps the model returns against the CPU oracle's (oracle.model_ref: the logits of the final 1x1 conv, averaged over
    the flip) within the project's bar for heatmaps, 1e-3 absolute (tests/test_estimator_gpu.py), taken relative to the largest
    absolute value of the oracle's maps where that exceeds 1 (ProbPose's maps are bounded by 1, these are not);
(b) the keypoints against the fp64 decode (tests/udp_ref.py) of THE HEATMAPS THE GPU RETURNED, under that decode's error bound:
    the Newton step amplifies heatmap error, so a fixed pixel bar against the CPU model would measure the conditioning of the
    synthetic maps, not the kernel. Keypoints whose fp64 Hessian has a condition number >= 100 are left out of the coordinate
    comparison (maximum and score still compared). ``synthetic_state_dict(head="heatmap")`` centres the final layer's weights per
    keypoint, so that every map swings around zero and has a positive maximum (with weights of random sign 74 of the 1088
    flip-averaged maps at B = 64 had none); the head's scale itself cannot move the share left out - the decode rescales every map
    to its own maximum and takes the log, the Hessian's condition number is scale-free - so ``logit_scale`` stays at the 2.0 of the
    other tests. Share the fp64 decode of the ORACLE's maps alone leaves out, found on the CPU before any GPU run, crop seed 100
    for every batch size (with flip test / without): B = 1: 0 of 17 / 0 of 17; B = 8: 2 of 136 = 1.5 % / 0 of 136;
    B = 64: 29 of 1088 = 2.7 % / 25 of 1088 = 2.3 %; no map with a non-positive maximum in any of the six;
(c) graph replay == kernel by kernel, test_step_stream == test_step, inference_topdown on a full image == the crop path, bit for bit;
(d) tools/test.py prints the AP keys on a synthetic COCO set and tools/eval_results.py scores its results file identically.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "td-hm_ViTPose-small_mi355x_coco-256x192.py")

pytestmark = pytest.mark.gpu


def _state_dict():
    from probpose_code_amd import synthetic as S

    return S.synthetic_state_dict("small", seed=0, logit_scale=2.0, head="heatmap")


def _model(flip=True, **opts):
    from probpose_code_amd import apis

    o = {"model.test_cfg.flip_test": flip}
    o.update(opts)
    return apis.init_model(CFG, dict(state_dict=_state_dict()), device="cuda:0", cfg_options=o)


def oracle_heatmaps(sd, crops, flip):
    """HeatmapHead.predict's maps on the CPU: logits of the final 1x1 conv, (a + flip_back(b)) * 0.5 in fp32."""
    from oracle import model_ref as M
    from probpose_code_amd import synthetic as S

    with torch.no_grad():
        x = M.preprocess(crops, S.IMG_MEAN, S.IMG_STD)
        _, a = M.head_heatmap(sd, M.vit_forward(sd, x, 12), normalize=None, return_logits=True)
        if flip:
            _, b = M.head_heatmap(sd, M.vit_forward(sd, x.flip(-1), 12), normalize=None, return_logits=True)
            a = (a + b.flip(-1)[:, list(S.COCO_FLIP_INDICES)]) * 0.5
    return a.float().numpy()


def left_out_share(maps):
    import udp_ref as R

    conds = np.concatenate([R.decode_f64(m, 11, (192, 256))["cond"] for m in maps])
    return float((~(conds < 100)).mean()), float(conds[np.isfinite(conds)].max())


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("B", [1, 8, 64])
def test_heatmaps_against_the_oracle_and_keypoints_against_the_fp64_decode(B, flip):
    import udp_ref as R
    from probpose_code_amd import _lib
    from probpose_code_amd import synthetic as S

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    model = _model(flip)
    eng = model.engine
    assert eng.head_kind == "heatmap" and eng.blur_kernel_size == 11 and not eng.tower_hw
    crops = S.synthetic_crops(B, seed=100)
    _lib.reset_launch_counts()
    out = eng.forward(crops.cuda(), flip, S.COCO_FLIP_INDICES, return_heatmaps=True)
    torch.cuda.synchronize()
    assert _lib.launch_count("pp_udp_decode.hip") == 1 and _lib.launch_count("pp_decode.hip") == 0
    for tower_kernel in ("pp_winograd.hip", "pp_conv_halo.hip", "pp_head.hip"):
        assert _lib.launch_count(tower_kernel) == 0, f"{tower_kernel} launched for a head without towers"
    hm = out["heatmaps"].cpu().numpy()
    kp, sc, locs = out["keypoints"].cpu().numpy(), out["scores"].cpu().numpy(), out["locs"].cpu().numpy()
    # (a)
    ref = oracle_heatmaps(_state_dict(), crops, flip)
    bar = 1e-3 * max(1.0, float(np.abs(ref).max()))
    assert np.abs(hm - ref).max() <= bar, f"heatmaps off by {np.abs(hm - ref).max():.3e} (bar {bar:.3e}, largest |value| {np.abs(ref).max():.2f})"
    share, worst_cond = left_out_share(ref)
    assert (ref.reshape(B, 17, -1).max(-1) > 0).all(), "a synthetic map without a positive maximum"
    assert share <= 0.05, f"the synthetic head leaves out {100 * share:.1f} % of the keypoints (cond >= 100) on the oracle's own maps"
    # (b)
    scale = np.array([192 / 47, 256 / 63])
    n_out = 0
    for b in range(B):
        d = R.decode_f64(hm[b], 11, (192, 256))
        assert np.array_equal(locs[b], d["locs"]) and np.array_equal(sc[b], d["scores"]), b
        ok = d["cond"] < 100
        n_out += int((~ok).sum())
        err = (np.abs(kp[b] - d["keypoints"]) / scale).max(1)
        assert (err[ok] <= d["bound"][ok]).all(), (b, err[ok].max(), d["bound"][ok])
    assert n_out <= round(share * B * 17) + 2, f"{n_out} of {B * 17} keypoints left out on the GPU's maps, {round(share * B * 17)} on the oracle's"
    print(f"B {B} flip {flip}: heatmaps L_inf {np.abs(hm - ref).max():.2e} (bar {bar:.2e}); oracle maps leave out {100 * share:.2f} % "
          f"(largest finite condition number {worst_cond:.1f}); GPU maps {n_out} of {B * 17}")


def test_graph_replay_stream_and_full_image_equal_the_plain_step(tmp_path):
    from probpose_code_amd import apis
    from probpose_code_amd import synthetic as S

    model = _model(True)
    eng = model.engine
    crops = S.synthetic_crops(8, seed=7).cuda()
    plain = {k: v.clone() for k, v in eng.forward(crops, True, S.COCO_FLIP_INDICES, return_heatmaps=True).items() if v is not None}
    graph = eng.forward_graph(crops, True, S.COCO_FLIP_INDICES, return_heatmaps=True)
    torch.cuda.synchronize()
    for k in ("keypoints", "scores", "locs", "heatmaps"):
        assert torch.equal(plain[k], graph[k]), k
    assert torch.count_nonzero(graph["scalars"]) == 0
    # test_step_stream == test_step (batches of different sizes)
    rng = np.random.default_rng(3)
    batches = []
    for n, seed in ((8, 1), (3, 2), (8, 3)):
        c = S.synthetic_crops(n, seed=seed)
        center = np.stack([rng.uniform(80, 400, n), rng.uniform(100, 500, n)], -1).astype(np.float32)
        scale = (np.array([192, 256], np.float32) * rng.uniform(0.8, 2.5, (n, 1)).astype(np.float32) * 1.25).astype(np.float32)
        batches.append((c, center, scale))
    steps = [model.test_step(apis.pack_crops(c, ce, s, model.dataset_meta)) for c, ce, s in batches]
    streamed = list(model.test_step_stream([apis.pack_crops(c, ce, s, model.dataset_meta) for c, ce, s in batches], depth=2, max_batch=8))
    for a, b in zip(steps, streamed):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            for f in ("keypoints", "keypoint_scores", "keypoints_visible", "bboxes"):
                assert np.array_equal(getattr(x.pred_instances, f), getattr(y.pred_instances, f)), f
            assert "keypoints_probs" not in x.pred_instances
            assert np.array_equal(x.pred_instances.keypoints_visible, x.pred_instances.keypoint_scores)
    # inference_topdown on the full image == the crops it cuts, through pack_crops
    img_path = os.path.join(ROOT, "demo", "resources", "synthetic_person.png")
    bb = np.array([[40, 30, 200, 400], [100, 60, 300, 420]], np.float32)
    res = apis.inference_topdown(model, img_path, bb)
    batch = apis._frame_batch(model, img_path, bb, "xyxy")
    crops2 = torch.stack(list(batch["inputs"]))
    center = np.stack([np.asarray(s.metainfo["input_center"]) for s in batch["data_samples"]])
    scale = np.stack([np.asarray(s.metainfo["input_scale"]) for s in batch["data_samples"]])
    res2 = model.test_step(apis.pack_crops(crops2, center, scale, model.dataset_meta))
    assert len(res) == len(res2) == 2
    for x, y in zip(res, res2):
        assert np.array_equal(x.pred_instances.keypoints, y.pred_instances.keypoints)
        assert np.array_equal(x.pred_instances.keypoint_scores, y.pred_instances.keypoint_scores)
    # output_heatmaps through test_step
    m2 = _model(True, **{"model.test_cfg.output_heatmaps": True})
    r = m2.test_step(apis.pack_crops(batches[1][0], batches[1][1], batches[1][2], m2.dataset_meta))
    assert tuple(r[0].pred_fields.heatmaps.shape) == (17, 64, 48)
    # the demo runs with this config and synthetic weights
    out_file = str(tmp_path / "demo.json")
    d = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "demo", "image_demo.py"), img_path, CFG, "synthetic",
                        "--out-file", out_file, "--bboxes", "40,30,200,400;100,60,300,420"], capture_output=True, text=True)
    assert d.returncode == 0, d.stderr[-2000:]
    got = json.load(open(out_file))
    assert len(got) == 2 and "keypoints_probs" not in got[0]
    for g, s in zip(got, res):
        assert np.array_equal(np.asarray(g["keypoints"]), s.pred_instances.keypoints[0])


def test_tools_test_prints_ap_and_eval_results_scores_the_file_identically(tmp_path):
    from probpose_code_amd import synthetic

    root = str(tmp_path / "coco")
    n = synthetic.synthetic_coco_dataset(root, 12, seed=5)
    assert n > 20
    prefix = str(tmp_path / "res" / "vitpose")
    os.makedirs(os.path.dirname(prefix))
    out = str(tmp_path / "metrics.json")
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.join(ROOT, "tools", "test.py"), CFG, "synthetic", "--cfg-options",
           f"test_dataloader.dataset.data_root={root}", f"test_evaluator.outfile_prefix={prefix}", "--out", out, "--workers", "4"]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    metrics = json.load(open(out))
    ap_keys = [k for k in metrics if k.split("/")[-1] in ("AP", "AP .5", "AP .75", "AR")]
    assert any(k.split("/")[-1] == "AP" for k in metrics), list(metrics)
    printed = {ln.split(": ")[0] for ln in r.stdout.splitlines() if ": " in ln}
    assert set(ap_keys) <= printed
    assert not any("prob_" in k for k in metrics), "a model without presence probabilities reports score_acc / score_thr"
    mout = str(tmp_path / "eval.json")
    e = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "eval_results.py"),
                        os.path.join(root, "annotations", "person_keypoints_val2017.json"), prefix + ".keypoints.json", "--out", mout],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert e.returncode == 0, e.stdout[-2000:] + e.stderr[-2000:]
    got = json.load(open(mout))
    common = [k for k in got if not k.startswith("Ex_") and any(m.split("/")[-1] == k for m in metrics)]
    assert "AP" in common and len(common) >= 10
    for k in common:
        mk = next(m for m in metrics if m.split("/")[-1] == k)
        assert got[k] == metrics[mk] or (np.isnan(got[k]) and np.isnan(metrics[mk])), (k, got[k], metrics[mk])
