"""GPU: the device half of the split JPEG decoder (csrc/pp_jpeg.hip) bit for bit against the committed grid
(tests/golden/jpeg_cases.npz: Pillow's pixels, which tests/jpeg_ref.py restates) with canary bytes around every output image
and the plane scratch, the coefficient input compared after the launches, two calls compared and the launches counted;
then the opt-in paths built on it: ``jpeg.imread_device``, ``runner.test_dataset(decode="device")`` and
``inference_topdown`` under ``LoadImage(imdecode_backend="mi355x")``, each against the host decoder, bitwise."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import jpeg_ref as J  # noqa: E402
from make_golden_jpeg import truncations  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5
GUARD = 4096
GAP = 67  # canary bytes between two output images: odd, so the images start at every alignment
CONFIG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_cropcoco-coco-val-256x192.py")


@pytest.fixture(scope="module")
def jpeg(lib_built):
    from probpose_code_amd import jpeg

    return jpeg


@pytest.fixture(scope="module")
def coefficients(jpeg):
    """name -> JpegCoefficients of every grid file (the host half, checked against the reference by the CPU tests)."""
    g = J.golden()
    out = {}
    for name in g["names"]:
        assert jpeg.probe(g["jpg"][name]).supported == 1, name  # no grid file may take the fallback
        out[name] = jpeg.entropy_decode(g["jpg"][name])
    return out


def _align(v, a=256):
    return (v + a - 1) // a * a


def _raw_reconstruct(jpeg, coefs):
    """pp_jpeg_reconstruct_bgr_batch on buffers of this test's own: the input block (descriptors, tables, coefficients), the
    plane scratch and all output images inside canary bytes. Runs the call twice. Returns the images (numpy, BGR)."""
    _lib = jpeg._lib
    n = len(coefs)
    off, o_qt, o_coef = _align(64 * n), [], []
    for c in coefs:
        o_qt.append(off)
        off = _align(off + 384)
        o_coef.append(off)
        off = _align(off + 2 * c.coef.size)
    host = np.zeros(off, np.uint8)
    sizes = [int(np.prod(c.shape)) for c in coefs]
    o_out, p = [], GUARD
    for s in sizes:
        o_out.append(p)
        p += s + GAP
    out = torch.full((p - GAP + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    infos = (jpeg.JpegInfo * n)(*[c.info for c in coefs])
    need = int(_lib.lib.pp_jpeg_scratch_bytes(infos, n))
    assert need == sum(_align(int(c.info.coef_count)) for c in coefs)
    scratch = torch.full((need + 2 * GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    dev = torch.empty(off, dtype=torch.uint8, device=DEV)
    desc = host[:64 * n].view(jpeg._DESC)
    planes = scratch.data_ptr() + GUARD
    for i, c in enumerate(coefs):
        host[o_qt[i]:o_qt[i] + 128 * len(c.qtables)].view(np.uint16)[:] = c.qtables.reshape(-1)
        host[o_coef[i]:o_coef[i] + 2 * c.coef.size].view(np.int16)[:] = c.coef
        desc[i] = (dev.data_ptr() + o_coef[i], dev.data_ptr() + o_qt[i], planes, out.data_ptr() + o_out[i], c.info.width, c.info.height,
                   c.info.ncomp, c.info.hs, c.info.vs, c.info.mcus_x, c.info.mcus_y, 0)
        planes += _align(int(c.info.coef_count))
    dev.copy_(torch.from_numpy(host))
    args = (dev.data_ptr(), n, max(int(c.info.coef_count) // 64 for c in coefs), max(c.info.height for c in coefs),
            max(c.info.width for c in coefs), torch.cuda.current_stream().cuda_stream)
    _lib.reset_launch_counts()
    _lib.call("pp_jpeg_reconstruct_bgr_batch", *args)
    torch.cuda.synchronize()
    counts = (_lib.launch_count("jpeg_idct"), _lib.launch_count("jpeg_color"), _lib.launch_count("pp_jpeg.hip"))
    assert counts == (1, 1, 2), f"launches per call {counts} for n = {n}"
    first = out.cpu().numpy()
    out[GUARD:len(out) - GUARD] = CANARY  # (the images and the gaps between them)
    _lib.call("pp_jpeg_reconstruct_bgr_batch", *args)
    torch.cuda.synchronize()
    second = out.cpu().numpy()
    assert np.array_equal(first, second), "a second launch gives other bytes"
    assert np.array_equal(dev.cpu().numpy(), host), "the kernels changed their input"
    sc = scratch.cpu().numpy()
    assert (sc[:GUARD] == CANARY).all() and (sc[GUARD + need:] == CANARY).all(), "bytes outside the plane scratch written"
    mask = np.ones(len(first), bool)
    for o, s in zip(o_out, sizes):
        mask[o:o + s] = False
    assert (first[mask] == CANARY).all(), "bytes outside an output image written"
    return [first[o:o + s].reshape(c.shape) for o, s, c in zip(o_out, sizes, coefs)]


def _check(names, images):
    g = J.golden()
    for name, img in zip(names, images):
        ref = g["rgb"][name][:, :, ::-1]
        assert img.shape == ref.shape, name
        assert np.array_equal(img, ref), f"{name}: {int((img != ref).any(axis=2).sum())} of {ref.shape[0] * ref.shape[1]} pixels differ"


def test_mixed_batches_of_16_equal_the_golden_pixels(jpeg, coefficients):
    names = list(coefficients)
    order = np.random.default_rng(3).permutation(len(names))  # sizes and sampling mixed within every batch
    for lo in range(0, len(names), 16):
        batch = [names[i] for i in order[lo:lo + 16]]
        _check(batch, _raw_reconstruct(jpeg, [coefficients[n] for n in batch]))


def test_every_size_alone_equals_the_golden_pixels(jpeg, coefficients):
    sizes = {}
    for k, name in enumerate(coefficients):
        sizes.setdefault(name.split("_")[0], []).append(name)
    assert len(sizes) == 13
    for k, (size, group) in enumerate(sorted(sizes.items())):
        name = group[(7 * k) % len(group)]  # another sampling / quality for every size
        _check([name], _raw_reconstruct(jpeg, [coefficients[name]]))


def test_reconstruct_batch_uploads_once_and_equals_the_golden_pixels(jpeg, coefficients):
    from probpose_code_amd.transforms import BatchStaging

    names = list(coefficients)[::9]
    staging = BatchStaging()
    for _ in range(2):  # the second call reuses the pinned buffer
        before = jpeg.reconstruct_calls
        jpeg._lib.reset_launch_counts()
        imgs = jpeg.reconstruct_batch([coefficients[n] for n in names], DEV, staging)
        assert jpeg.reconstruct_calls == before + 1 and jpeg._lib.launch_count("pp_jpeg.hip") == 2
        assert all(t.is_cuda and t.dtype == torch.uint8 for t in imgs)
        _check(names, [t.cpu().numpy() for t in imgs])
    assert jpeg.reconstruct_batch([], DEV) == []


def _host_outcome(path):
    from probpose_code_amd.apis import load_image_bgr

    try:
        return torch.from_numpy(load_image_bgr(path))
    except Exception as e:  # noqa: BLE001
        return e


def test_imread_device_equals_the_host_decoder(jpeg, tmp_path):
    g = J.golden()
    names = [n for n in g["names"] if "_q75_" in n or n.endswith(("optimize", "qtables"))]
    assert len(names) >= 13 * 4
    before = jpeg.fallbacks
    for name in names:
        path = str(tmp_path / (name + ".jpg"))
        with open(path, "wb") as f:
            f.write(g["jpg"][name])
        ref = _host_outcome(path)
        assert isinstance(ref, torch.Tensor), (name, ref)
        for src in (path, g["jpg"][name]):
            got = jpeg.imread_device(src, DEV)
            assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), ref), name
    assert jpeg.fallbacks == before, "a grid file took the host decoder"


def test_imread_device_falls_back_like_the_host_decoder(jpeg, tmp_path):
    g = J.golden()
    files = dict(g["refused"])
    for kind, cut in truncations(g["jpg"]["48x64_420_q95_smooth_r0"]).items():
        files["truncated_" + kind] = cut
    files["missing"] = None
    jpeg._lib.reset_launch_counts()
    for k, (name, data) in enumerate(files.items()):
        path = str(tmp_path / (name + ".jpg"))
        if data is not None:
            with open(path, "wb") as f:
                f.write(data)
        ref = _host_outcome(path)
        before = jpeg.fallbacks
        try:
            got = jpeg.imread_device(path, DEV)
        except Exception as e:  # noqa: BLE001
            got = e
        assert jpeg.fallbacks == before + 1, name
        if isinstance(ref, Exception):
            assert type(got) is type(ref) and str(got) == str(ref), (name, got, ref)
        else:
            assert isinstance(got, torch.Tensor) and got.is_cuda and torch.equal(got.cpu(), ref), name
    assert isinstance(_host_outcome(str(tmp_path / "progressive.jpg")), torch.Tensor)  # the host decoder reads these two
    assert isinstance(_host_outcome(str(tmp_path / "cmyk.jpg")), torch.Tensor)
    assert jpeg._lib.launch_count("jpeg_idct") == 0 and jpeg._lib.launch_count("jpeg_color") == 0


@pytest.fixture(scope="module")
def small_model(tmp_path_factory):
    from probpose_code_amd import apis, synthetic
    from probpose_code_amd.config import Config
    from probpose_code_amd.datasets import build_dataset

    tmp = tmp_path_factory.mktemp("jpeg_coco")  # six JPEG images, three in each of the config's two datasets
    root = [str(tmp / "cropcoco") + "/", str(tmp / "coco") + "/"]
    n = sum(synthetic.synthetic_coco_dataset(r, 3, seed=9 + i, fmt="jpg", persons=(2, 6), invalid_image=False, id_base=i + 1) for i, r in enumerate(root))
    cfg = Config.fromfile(CONFIG)
    cfg.merge_from_dict({f"test_dataloader.dataset.datasets.{i}.data_root": r for i, r in enumerate(root)})
    model = apis.init_model(cfg, dict(state_dict=synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device=DEV)
    return model, build_dataset(cfg.test_dataloader.dataset), root, n


FIELDS = ("keypoints", "keypoint_scores", "keypoints_probs", "keypoints_visible", "keypoints_oks", "keypoints_error", "bboxes", "bbox_scores")


def _same_fields(x, y):
    checked = 0
    for f in FIELDS:
        if f in x.pred_instances or f in y.pred_instances:
            a, e = np.asarray(getattr(x.pred_instances, f)), np.asarray(getattr(y.pred_instances, f))
            assert a.dtype == e.dtype and a.tobytes() == e.tobytes(), f
            checked += 1
    assert checked >= 4


def _same_samples(a, b):
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert x.id == y.id and x.img_path == y.img_path
        _same_fields(x, y)


def test_test_dataset_with_device_decode_equals_host_decode(jpeg, small_model):
    from probpose_code_amd import runner

    model, dataset, _, n = small_model
    assert len(dataset) == n > 8
    runs = {}
    for mode in ("host", "device"):
        got = []
        calls, falls = jpeg.reconstruct_calls, jpeg.fallbacks
        jpeg._lib.reset_launch_counts()
        runner.test_dataset(model, dataset, None, batch_size=8, workers=4, sink=got.extend, decode=mode)
        torch.cuda.synchronize()
        runs[mode] = got
        plan = runner.plan_batches([dataset.get_data_info(i)["img_path"] for i in range(n)], 8)
        seen, with_new = set(), 0
        for b in plan:
            with_new += bool(set(b.images) - seen)
            seen |= set(b.images)
        assert len(plan) > 1 and len(seen) >= 5
        if mode == "device":  # one call per batch that brings new images, two launches each, no file left to the host
            assert jpeg.reconstruct_calls - calls == with_new and jpeg._lib.launch_count("pp_jpeg.hip") == 2 * with_new
            assert jpeg.fallbacks == falls
        else:
            assert jpeg.reconstruct_calls == calls and jpeg._lib.launch_count("pp_jpeg.hip") == 0
    _same_samples(runs["host"], runs["device"])
    with pytest.raises(ValueError, match="decode"):
        runner.test_dataset(model, dataset, None, decode="gpu")


def test_inference_topdown_follows_the_loadimage_backend(jpeg, small_model):
    from probpose_code_amd import apis
    from probpose_code_amd import transforms as T

    model, dataset, _, _ = small_model
    path = dataset.get_data_info(0)["img_path"]
    bb = np.array([[40, 30, 300, 400], [200, 60, 500, 470]], np.float32)
    jpeg._lib.reset_launch_counts()
    host = apis.inference_topdown(model, path, bb) + apis.inference_topdown(model, path)
    assert jpeg._lib.launch_count("pp_jpeg.hip") == 0  # the default backend decodes on the host
    apis.use_device_decode(model)
    try:
        assert [t.imdecode_backend for t in apis._val_pipeline(model).transforms if isinstance(t, T.LoadImage)] == ["mi355x"]
        device = apis.inference_topdown(model, path, bb) + apis.inference_topdown(model, path)
        assert jpeg._lib.launch_count("pp_jpeg.hip") == 4
    finally:
        apis.use_device_decode(model, False)
    assert len(host) == len(device) == 3
    for x, y in zip(host, device):
        _same_fields(x, y)
    # the transform itself, from a config dict: a device tensor with the host decoder's bytes
    one = T.Compose([dict(type="MI355XLoadImage", imdecode_backend="mi355x")])(dict(img_path=path))
    ref = T.Compose([dict(type="MI355XLoadImage")])(dict(img_path=path))
    assert one["img"].is_cuda and np.array_equal(one["img"].cpu().numpy(), ref["img"]) and tuple(one["img_shape"]) == tuple(ref["img_shape"])
