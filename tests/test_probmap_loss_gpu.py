"""GPU: the loss mode on the MI355X - ``pp_probmap_loss_maps`` against the fp64 restatement (tests/probmap_loss_ref.py) on the golden
batch and on small maps with border impulses, ``pp_probmap_loss_scalars`` and the whole ``ProbMapHead.loss`` against the reference's
dictionary (tests/golden/loss_cases.npz), ``forward(mode="loss")`` against the restatement fed with the engine's own maps, and the
dataset loop with ``loss=True``. Flags, weights, argmaxes and acc_* are exact; sums are held to the bounds probmap_loss_ref derives."""
import json
import math
import os

import numpy as np
import pytest
import torch

import probmap_loss_cases as C
import probmap_loss_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CONFIG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")
EVAL_CONFIG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_cropcoco-coco-val-256x192.py")
DEV = "cuda:0"
CANARY = 0xA5


def launch_maps(p, t, w, sw=0.05, gw=0.0, lw=1.0):
    """One raw pp_probmap_loss_maps call with all four outputs inside canary-filled buffers."""
    from probpose_code_amd import _lib

    B, K, H, W = p.shape
    pad = 256
    sizes = dict(map_sums=B * K * 8, argmax=B * K * 8, maxval=B * K * 8, loss=4)
    bufs = {n: torch.full((s + 2 * pad,), CANARY, dtype=torch.uint8, device=DEV) for n, s in sizes.items()}
    ins = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV) for a in (p, t, w)]
    before = [a.clone() for a in ins]
    _lib.call("pp_probmap_loss_maps", *(a.data_ptr() for a in ins), B, K, H, W, sw, gw, lw, *(bufs[n].data_ptr() + pad for n in sizes),
              _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ins, before)), "inputs changed"
    raw = {}
    for n, s in sizes.items():
        host = bufs[n].cpu().numpy()
        assert (host[:pad] == CANARY).all() and (host[pad + s:] == CANARY).all(), f"{n}: write outside the buffer"
        raw[n] = host[pad:pad + s].copy()
    return dict(map_sums=raw["map_sums"].view(np.float64).reshape(B, K), argmax=raw["argmax"].view(np.int32).reshape(B, K, 2),
                maxval=raw["maxval"].view(np.float32).reshape(B, K, 2), loss=raw["loss"].view(np.float32)[0])


def check_against_ref(got, p, t, w, sw=0.05, gw=0.0, lw=1.0, tag=""):
    r = PR.map_loss(p, t, w, sw, gw, lw)
    off = np.abs(got["map_sums"] - r["map_sums"])
    bound = PR.map_sums_bound(r)
    print(f"{tag}: loss {got['loss']:.9e} (fp64 {r['loss']:.9e}, bound {PR.map_loss_bound(r, lw):.2e}); worst map |diff| / bound "
          f"{np.max(off / np.maximum(bound, 1e-300)):.3g}")
    assert (off <= bound).all(), tag
    assert abs(float(got["loss"]) - r["loss"]) <= PR.map_loss_bound(r, lw) + PR.U * abs(r["loss"]), tag
    for i, m in enumerate((p, t)):
        idx, val = PR.argmax_first(np.asarray(m, np.float32))
        assert np.array_equal(got["argmax"][..., i], idx) and np.array_equal(got["maxval"][..., i], val), (tag, i)


@pytest.mark.gpu
def test_map_loss_golden_batch():
    g, r = C.golden(), C.reference64()
    got = launch_maps(g["pred_maps"], g["heatmaps"], g["keypoint_weights"])
    check_against_ref(got, g["pred_maps"], g["heatmaps"], g["keypoint_weights"], tag="golden")
    assert abs(float(got["loss"]) - float(g["loss_loss_kpt"])) <= 2 * r["maps_bound"]  # device and reference both within the bound of fp64
    assert (np.abs(got["map_sums"] - g["pixel_loss_map_sums"]) <= 2 * PR.map_sums_bound(r["maps"])).all()
    assert got["argmax"][0, 0, 0] == 10 * 48 + 7 and (got["map_sums"][g["keypoint_weights"] == 0] == 0).all()
    again = launch_maps(g["pred_maps"], g["heatmaps"], g["keypoint_weights"])
    assert all(np.asarray(got[n]).tobytes() == np.asarray(again[n]).tobytes() for n in got), "a repeat launch is not bit-identical"


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 5), (64, 48)])
def test_map_loss_border_impulses_masks_and_ties(H, W):
    rng = np.random.default_rng(H * 64 + W)
    spots = sorted({(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)})
    B, K = 2, len(spots) + 3  # an impulse in each corner and on each edge, then a random map, a tie map, a zero map
    p = np.zeros((B, K, H, W), np.float32)
    for k, (y, x) in enumerate(spots):
        p[:, k, y, x] = (0.75, 0.5)
    p[:, len(spots)] = rng.random((B, H, W), dtype=np.float32)
    p[:, len(spots) + 1] = np.round(rng.random((B, H, W)) * 2) / 2  # ties
    t = rng.random((B, K, H, W), dtype=np.float32)
    t[0, 0] = 0
    w = np.ones((B, K), np.float32)
    w[1, ::2] = 0
    check_against_ref(launch_maps(p, t, w, 0.05, 0.1, 2.0), p, t, w, 0.05, 0.1, 2.0, tag=f"{H}x{W} impulses")
    zero = launch_maps(p, t, np.zeros_like(w))  # an all-zero mask
    assert zero["loss"] == 0 and not zero["map_sums"].any()
    check_against_ref(zero, p, t, np.zeros_like(w), tag=f"{H}x{W} zero mask")
    one = launch_maps(p[:1, :1], t[:1, :1], w[:1, :1])  # B K = 1
    check_against_ref(one, p[:1, :1], t[:1, :1], w[:1, :1], tag=f"{H}x{W} single map")


@pytest.fixture(scope="module", params=["f32", "f16x3"])
def model(request):
    from probpose_code_amd import apis, synthetic
    from probpose_code_amd.config import Config

    cfg = Config.fromfile(CONFIG)
    cfg.merge_from_dict({"model.precision": request.param})
    return apis.init_model(cfg, dict(state_dict=synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device=DEV)


def check_dictionary(losses, targets, g, r):
    """The loss dictionary of the golden batch against the reference's, under the restatement's bounds (twice: device and reference
    each lie within one bound of fp64); flags, weights, argmaxes and accuracies exactly."""
    assert list(losses) == list(C.LOSS_KEYS) and all(isinstance(v, torch.Tensor) and v.is_cuda for v in losses.values())
    got = {k: float(v.reshape(-1)[0]) for k, v in losses.items()}
    print({k: f"{v:.9e}" for k, v in got.items()})
    for name in ("acc_pose", "acc_prob", "acc_vis"):
        assert got[name] == float(np.ravel(g["loss_" + name])[0]), name
    assert losses["acc_pose"].dtype == torch.float64 and losses["acc_prob"].dtype == torch.float32
    assert abs(got["loss_kpt"] - r["maps"]["loss"]) <= r["maps_bound"] and abs(got["loss_kpt"] - float(g["loss_loss_kpt"])) <= 2 * r["maps_bound"]
    for name, (value, bound) in r["losses"].items():
        bound = bound + PR.U * abs(value)  # (the float32 store)
        assert abs(got[name] - value) <= bound, (name, got[name], value, bound)
        assert abs(got[name] - float(np.ravel(g["loss_" + name])[0])) <= 2 * bound, name
    tg = r["targets"]
    assert np.array_equal(targets["oks_weight"].cpu().numpy(), g["oks_weight"])
    assert np.array_equal(targets["vis_weights"].cpu().numpy(), g["vis_weights"])
    assert not targets["gt_errs"].any()  # freeze_error
    ok = r["comparable"]
    err = np.abs(targets["gt_oks"].cpu().numpy().astype(np.float64) - tg["gt_oks"])
    assert (err[ok] <= tg["gt_oks_bound"][ok]).all() and (targets["gt_oks"].cpu().numpy()[~(g["in_image"] & g["annotated"])] == 0).all()


@pytest.mark.gpu
def test_head_loss_on_the_golden_batch(model):
    g, r = C.golden(), C.reference64()
    hm, sc = torch.from_numpy(g["pred_maps"].copy()).to(DEV), torch.from_numpy(g["pred_scalars"].copy()).to(DEV)
    np.random.seed(int(g["seed"]))
    losses, targets = model.head.loss_from_outputs(hm, sc, C.make_samples(g), return_targets=True)
    check_dictionary(losses, targets, g, r)
    # the same batch with the targets encoded on the device from the keypoints: flags and weights are the reference's, so is the rest
    np.random.seed(int(g["seed"]))
    losses2, targets2 = model.head.loss_from_outputs(hm, sc, C.make_samples(g, device_targets=True), return_targets=True)
    for name in ("keypoint_weights", "in_image", "annotated"):
        assert np.array_equal(targets2[name].cpu().numpy().astype(np.float32), g[name].astype(np.float32)), name
    check_dictionary(losses2, targets2, g, r)
    np.random.seed(int(g["seed"]))
    again = model.head.loss_from_outputs(hm, sc, C.make_samples(g))
    assert all(torch.equal(losses[k], again[k]) for k in losses), "the dictionary is not the same bits launch after launch"
    short = model.head.loss_from_outputs(hm, sc, C.make_samples(g), train_cfg=dict(compute_acc=False))
    assert list(short) == list(C.LOSS_KEYS[:5])


@pytest.mark.gpu
def test_forward_mode_loss_against_the_restatement_on_the_engines_own_maps(model):
    import udp_ref as R
    from probpose_code_amd import synthetic as S

    g = C.golden()
    crops = S.synthetic_crops(3, seed=1).to(DEV)
    out = model.engine.forward(crops, False, None, return_heatmaps=True)
    hm, sc = out["heatmaps"].cpu().numpy().copy(), out["scalars"].cpu().numpy().copy()
    assert hm.min() >= 0 and hm.max() <= 1
    np.random.seed(3)
    losses = model.forward(crops, C.make_samples(g), mode="loss")
    got = {k: float(v.reshape(-1)[0]) for k, v in losses.items()}
    assert list(losses) == list(C.LOSS_KEYS) and all(math.isfinite(v) for v in got.values()), got
    maps = PR.map_loss(hm, g["heatmaps"], g["keypoint_weights"], 0.05)
    print(f"{model.precision}: loss_kpt {got['loss_kpt']:.9e}, fp64 on the engine's maps {maps['loss']:.9e}")
    assert abs(got["loss_kpt"] - maps["loss"]) <= PR.map_loss_bound(maps) + PR.U * abs(maps["loss"])
    dec = {n: [R.decode_f64(m[b], 11, (192, 256)) for b in range(3)] for n, m in (("gt", g["heatmaps"]), ("dt", hm))}
    scale = np.array([192 / 47, 256 / 63])
    kp = {n: np.stack([x["keypoints"] for x in d]) for n, d in dec.items()}
    bd = {n: np.stack([x["bound"] for x in d])[..., None] * scale for n, d in dec.items()}
    ok = np.stack([x["cond"] for x in dec["gt"]]) < 100
    ok &= np.stack([x["cond"] for x in dec["dt"]]) < 100
    tg = PR.scalar_targets(kp["gt"], kp["dt"], g["in_image"], g["annotated"], g["keypoints_visibility"], d_gt=bd["gt"], d_dt=bd["dt"])
    gb = np.where(ok | (tg["gt_oks_bound"] == 0), tg["gt_oks_bound"], 1.0)
    for name, (value, bound) in PR.scalar_losses(sc, tg, g["in_image"], g["annotated"], g["keypoints_visibility"], gb).items():
        assert abs(got[name] - value) <= bound + PR.U * abs(value), (name, got[name], value, bound)
    assert model.loss(crops, C.make_samples(g), train_cfg=dict(compute_acc=False)).keys() == set(C.LOSS_KEYS[:5])


@pytest.mark.gpu
def test_dataset_loop_with_loss(tmp_path):
    from PIL import Image

    from probpose_code_amd import apis, runner, synthetic
    from probpose_code_amd.config import Config
    from probpose_code_amd.datasets import build_dataset

    doc = json.load(open(os.path.join(HERE, "golden", "dataset_cases.json")))
    rng = np.random.default_rng(5)
    # The fixture pins dataset PARSING and leaves fields out on purpose; the evaluator reads bbox, area and iscrowd of every annotation of
    # the file. The annotation without a box is no instance of the dataset either way (12 instances, asserted below); the others get the
    # area of their box and iscrowd 0 where the file leaves them out.
    doc["annotations"]["annotations"] = [a for a in doc["annotations"]["annotations"] if "bbox" in a]
    for a in doc["annotations"]["annotations"]:
        a.setdefault("area", float(a["bbox"][2] * a["bbox"][3]))
        a.setdefault("iscrowd", 0)
        assert len(a["keypoints"]) == 51
    roots = []
    for name in ("cropcoco", "coco"):
        root = tmp_path / name
        (root / "annotations").mkdir(parents=True)
        (root / "val2017").mkdir()
        (root / "annotations" / "person_keypoints_val2017.json").write_text(json.dumps(doc["annotations"]))
        for im in doc["annotations"]["images"]:
            Image.fromarray(rng.integers(0, 255, (im["height"], im["width"], 3), dtype=np.uint8)).save(root / "val2017" / im["file_name"], quality=90)
        roots.append(str(root) + "/")
    cfg = Config.fromfile(EVAL_CONFIG)
    cfg.merge_from_dict({f"test_dataloader.dataset.datasets.{i}.data_root": r for i, r in enumerate(roots)})
    net = apis.init_model(cfg, dict(state_dict=synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device=DEV)
    dataset = build_dataset(cfg.test_dataloader.dataset)
    assert len(dataset) == 12
    runs = []
    for flag in (False, True):
        np.random.seed(0)
        runs.append(runner.test_dataset(net, dataset, runner.build_evaluator(cfg.test_evaluator, dataset, device=DEV), batch_size=8, workers=2,
                                        loss=flag))
    plain, scored = runs
    extra = {k: v for k, v in scored.items() if k.startswith("loss/")}
    assert sorted(extra) == sorted("loss/" + k for k in C.LOSS_KEYS) and not any(k.startswith("loss/") for k in plain)
    print(extra)
    assert all(math.isfinite(v) for v in extra.values()), extra
    rest = {k: v for k, v in scored.items() if k not in extra}
    assert rest.keys() == plain.keys()
    assert all(np.float64(rest[k]).tobytes() == np.float64(plain[k]).tobytes() for k in plain), "the metrics changed with loss=True"
