"""Dataset evaluation on the MI355X: the batch crop warp (pp_warp_affine_u8_batch) byte for byte against the per-image warp and
the oracle, the test loop (runner.test_dataset) against the same batches built sample by sample, and tools/test.py in a
child process. All data is generated here."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EVAL_CONFIG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_cropcoco-coco-val-256x192.py")
CANARY = 0xA5


def _random_mats(rng, shapes, crop_image, input_size=(192, 256)):
    from probpose_code_amd import transforms as T

    mats = []
    for j in crop_image:
        H, W = shapes[j]
        x0, y0 = rng.uniform(-0.3 * W, W), rng.uniform(-0.3 * H, H)
        bw, bh = rng.uniform(1, 1.2 * W + 2), rng.uniform(1, 1.2 * H + 2)
        c, s, m = T.topdown_affine_params(np.array([[x0, y0, x0 + bw, y0 + bh]], np.float32), input_size)
        rot = float(rng.choice([0.0, 0.0, rng.uniform(-45, 45)]))
        mats.append(T.get_udp_warp_matrix(c[0], s[0], rot, input_size) if rot else m[0])
    return np.stack(mats).astype(np.float64)


@pytest.mark.gpu
def test_batch_warp_is_byte_equal_to_the_per_image_warp_and_the_oracle():
    import torch

    from oracle import warp_ref
    from probpose_code_amd import _lib
    from probpose_code_amd import transforms as T

    rng = np.random.default_rng(2026)
    dev = torch.device("cuda:0")
    oh, ow = 256, 192
    checked = 0
    for case in range(12):
        C = 1 if case % 3 == 0 else 3
        m = int(rng.integers(1, 9))
        shapes = [(1, 3), (1080, 1920)][: m] if case == 0 else []
        while len(shapes) < m:
            shapes.append((int(rng.integers(1, 1081)), int(rng.integers(1, 1921))))
        imgs = [rng.integers(0, 256, (h, w, C), dtype=np.uint8) for h, w in shapes]
        n = int(rng.integers(1, 301)) if case % 4 else int(rng.integers(1, 4))
        crop_image = rng.integers(0, m, n).astype(np.int32)  # crops interleaved across the images, random order
        mats = _random_mats(rng, shapes, crop_image)
        inv = torch.as_tensor(np.stack([T.invert_affine(mm) for mm in mats]), dtype=torch.float64, device=dev)
        packed = case % 2 == 0  # images in one device buffer, or as separate device tensors
        if packed:
            offs = np.cumsum([0] + [a.size + 13 for a in imgs])  # odd offsets on purpose
            buf = torch.zeros(int(offs[-1]), dtype=torch.uint8, device=dev)
            for a, o in zip(imgs, offs):
                buf[int(o):int(o) + a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
            ptrs = [buf.data_ptr() + int(o) for o in offs[:-1]]
            dimgs = [buf[int(o):int(o) + a.size].view(a.shape) for a, o in zip(imgs, offs)]
        else:
            dimgs = [torch.from_numpy(a).to(dev) for a in imgs]
            ptrs = [t.data_ptr() for t in dimgs]
        tab_ptr = torch.tensor(ptrs, dtype=torch.int64, device=dev)
        tab_hw = torch.tensor(np.array(shapes, np.int32).reshape(-1), dtype=torch.int32, device=dev)
        tab_crop = torch.from_numpy(crop_image).to(dev)
        guard = 4096
        out = torch.full((guard + n * C * oh * ow + guard,), CANARY, dtype=torch.uint8, device=dev)
        _lib.call("pp_warp_affine_u8_batch", tab_ptr.data_ptr(), tab_hw.data_ptr(), C, tab_crop.data_ptr(), inv.data_ptr(),
                  max(h for h, _ in shapes), max(w for _, w in shapes), out.data_ptr() + guard, n, oh, ow,
                  torch.cuda.current_stream().cuda_stream)
        host = out.cpu().numpy()
        assert (host[:guard] == CANARY).all() and (host[-guard:] == CANARY).all(), f"case {case}: bytes outside the output written"
        crops = host[guard:-guard].reshape(n, C, oh, ow)
        for j in range(m):  # the single-image entry on the crops of image j
            sel = np.nonzero(crop_image == j)[0]
            if len(sel) == 0:
                continue
            ref = T.warp_affine_crops(dimgs[j], mats[sel], (ow, oh)).cpu().numpy()
            assert np.array_equal(crops[sel], ref), f"case {case}: image {j} differs from pp_warp_affine_u8"
        for i in rng.choice(n, min(n, 3), replace=False):  # and the oracle on a few
            ref = warp_ref.warp_affine_u8(imgs[crop_image[i]], mats[i], (ow, oh))
            ref = ref.reshape(oh, ow, C).transpose(2, 0, 1)
            assert np.array_equal(crops[i], ref), f"case {case}: crop {i} differs from the oracle"
            checked += 1
    assert checked >= 12


@pytest.mark.gpu
def test_transform_batch_packs_host_images_and_reads_device_images_in_place():
    """Compose.batched over boxes of several images - host arrays and device tensors mixed - equals the per-sample pipeline."""
    import torch

    from probpose_code_amd import transforms as T

    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (int(rng.integers(50, 700)), int(rng.integers(50, 900)), 3), dtype=np.uint8) for _ in range(5)]
    srcs = [imgs[0], torch.from_numpy(imgs[1]).cuda(), imgs[2], torch.from_numpy(imgs[3]).cuda(), imgs[4]]
    pipe = T.Compose([dict(type="MI355XGetBBoxCenterScale"), dict(type="MI355XTopdownAffine", input_size=(192, 256), use_udp=True)])
    data = []
    for k in rng.integers(0, 5, 40):
        H, W = imgs[k].shape[:2]
        x0, y0 = rng.uniform(-20, W - 10), rng.uniform(-20, H - 10)
        data.append(dict(img=srcs[k], bbox=np.array([[x0, y0, x0 + rng.uniform(5, W), y0 + rng.uniform(5, H)]], np.float32), k=int(k)))
    for _ in range(2):  # twice: the second batch reuses the pinned buffer
        got = pipe.batched([dict(d) for d in data])
        for d, g in zip(data, got):
            one = pipe(dict(d, img=imgs[d["k"]]))
            assert np.array_equal(g["img"].cpu().numpy(), one["img"].cpu().numpy())
            assert np.array_equal(g["input_center"], one["input_center"]) and np.array_equal(g["input_scale"], one["input_scale"])


def _write_two_datasets(tmp_path):
    from probpose_code_amd import synthetic as S

    roots = [str(tmp_path / "cropcoco") + "/", str(tmp_path / "coco") + "/"]
    n0 = S.synthetic_coco_dataset(roots[0], 19, seed=11, persons=(1, 8), id_base=1)
    n1 = S.synthetic_coco_dataset(roots[1], 21, seed=12, persons=(1, 8), id_base=2)
    return roots, n0 + n1


def _cfg_options(roots):
    return {f"test_dataloader.dataset.datasets.{i}.data_root": r for i, r in enumerate(roots)}


def _same(a, b):
    return a.keys() == b.keys() and all((isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k] for k in a)


@pytest.fixture(scope="module")
def eval_run(tmp_path_factory):
    import torch

    from probpose_code_amd import apis, runner, synthetic
    from probpose_code_amd.config import Config
    from probpose_code_amd.datasets import build_dataset

    tmp = tmp_path_factory.mktemp("dataset_eval")
    roots, n_valid = _write_two_datasets(tmp)
    cfg = Config.fromfile(EVAL_CONFIG)
    cfg.merge_from_dict(_cfg_options(roots))
    model = apis.init_model(cfg, dict(state_dict=synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device="cuda:0")
    dataset = build_dataset(cfg.test_dataloader.dataset)
    batches = []
    metrics = runner.test_dataset(model, dataset, runner.build_evaluator(cfg.test_evaluator, dataset, device="cuda:0"), batch_size=64,
                                  workers=4, sink=batches.append)
    torch.cuda.synchronize()
    return dict(tmp=tmp, roots=roots, n_valid=n_valid, cfg=cfg, model=model, dataset=dataset, batches=batches, metrics=metrics)


@pytest.mark.gpu
def test_test_dataset_equals_sample_by_sample_batches(eval_run):
    import torch

    from probpose_code_amd import runner
    from probpose_code_amd.transforms import pseudo_collate

    model, dataset, batches = eval_run["model"], eval_run["dataset"], eval_run["batches"]
    n = len(dataset)
    assert n == eval_run["n_valid"] and 120 <= n <= 200, n
    assert [len(b) for b in batches] == [min(64, n - lo) for lo in range(0, n, 64)]  # full batches, a partial last one
    infos = [dataset.get_data_info(i) for i in range(n)]
    plan = runner.plan_batches([d["img_path"] for d in infos], 64)
    assert any(set(a.images) & set(b.images) for a, b in zip(plan, plan[1:])), "no image split across two batches"
    assert any(len({infos[i]["dataset_name"] for i in b.indices}) == 2 for b in plan), "no batch crosses the dataset boundary"
    got = [s for b in batches for s in b]
    assert [s.id for s in got] == [d["id"] for d in infos] and [s.dataset_name for s in got] == [d["dataset_name"] for d in infos]
    k = 0
    fields = ("keypoints", "keypoint_scores", "keypoints_probs", "keypoints_visible", "keypoints_oks", "keypoints_error", "bboxes",
              "bbox_scores")
    for b in plan:
        ref = model.test_step(pseudo_collate([dataset.pipeline(dataset.get_data_info(i)) for i in b.indices]))
        torch.cuda.synchronize()
        for r in ref:
            g = got[k]
            k += 1
            assert g.img_id == r.img_id and g.id == r.id
            for f in fields:
                if f not in r.pred_instances:
                    continue
                a, e = np.asarray(getattr(g.pred_instances, f)), np.asarray(getattr(r.pred_instances, f))
                assert a.dtype == e.dtype and a.tobytes() == e.tobytes(), (f, g.id)
    assert k == n


@pytest.mark.gpu
def test_metrics_equal_two_coco_metrics_fed_the_same_predictions(eval_run):
    from probpose_code_amd import runner

    cfg, dataset, batches = eval_run["cfg"], eval_run["dataset"], eval_run["batches"]
    metrics = eval_run["metrics"]
    ev = runner.build_evaluator(cfg.test_evaluator, dataset, device="cuda:0")
    by_name = {}
    for s in (s for b in batches for s in b):
        d = runner.sample_to_dict(s)
        by_name.setdefault(d["dataset_name"], []).append(d)
    ref = {}
    for name, metric in ev.metrics_dict.items():
        metric.process(None, by_name[name])
        ref.update(metric.compute_metrics())
    assert any(k.startswith("CropCOCO/") for k in metrics) and any(k.startswith("COCO/") for k in metrics)
    assert "CropCOCO/Ex_AP" in metrics and "COCO/AP" in metrics
    assert _same(metrics, ref), (metrics, ref)


@pytest.mark.gpu
def test_tools_test_cli_writes_the_same_metrics(eval_run):
    out = eval_run["tmp"] / "metrics.json"
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.join(ROOT, "tools", "test.py"), EVAL_CONFIG, "synthetic",
           "--cfg-options"] + [f"{k}={v}" for k, v in _cfg_options(eval_run["roots"]).items()] + ["--out", str(out), "--workers", "4"]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "CropCOCO/AP" in r.stdout
    assert _same(json.load(open(out)), eval_run["metrics"])
