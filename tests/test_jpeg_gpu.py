"""GPU: the device half of the split JPEG decoder (csrc/pp_jpeg.hip) bit for bit against the committed grid
(tests/golden/jpeg_cases.npz: Pillow's pixels, which tests/jpeg_ref.py restates) with canary bytes around every output image
and the plane scratch, the coefficient input compared after the launches, two calls compared and the launches counted;
then the opt-in paths built on it: ``jpeg.imread_device``, ``runner.test_dataset(decode="device")`` and
``inference_topdown`` under ``LoadImage(imdecode_backend="mi355x")``, each against the host decoder, bitwise.
Beyond the grid (tests/jpeg_sources.py), judged by tests/jpeg_ref.py alone - Pillow only encodes: widths that reach the second
and third workgroup column of jpeg_color_kernel, 65 MCUs in a row and in a column, two workload-sized images, a batch whose
launch bounds come from three different images; streams of other layouts (tests/jpeg_write.py) and the streams to refuse
through ``jpeg.imread_device``; and tests/fuzz_jpeg.py for a few seconds."""
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
import jpeg_sources as S  # noqa: E402
from jpeg_harness import raw_reconstruct as _raw_reconstruct  # noqa: E402
from make_golden_jpeg import truncations  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
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


_REF = {}


def _reference_bgr(data: bytes) -> np.ndarray:
    """tests/jpeg_ref.py's pixels of a file as BGR, computed once and shared (do not modify)."""
    if data not in _REF:
        _REF[data] = np.ascontiguousarray(J.decode_rgb(data)[:, :, ::-1])
    return _REF[data]


def _host_half(jpeg, files):
    out = []
    for label, data in files:
        info = jpeg.probe(data)
        assert info.supported == 1, (label, info.reason)  # none of these may take the fallback
        out.append(jpeg.entropy_decode(data))
    return out


def _check_reference(files, images):
    assert len(files) == len(images)
    for (label, data), img in zip(files, images):
        ref = _reference_bgr(data)
        assert img.shape == ref.shape, label
        bad = (img != ref).any(axis=2)
        assert not bad.any(), f"{label}: {int(bad.sum())} of {bad.size} pixels differ, the first at (y, x) = {tuple(int(v) for v in np.argwhere(bad)[0])}"


@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_beyond_the_grid_equal_the_reference(jpeg, size):
    """5 x 257, 6 x 260, 3 x 515: pixels at x >= 256 and x >= 512 (blockIdx.x of jpeg_color_kernel 1 and 2), a tail of one
    and of three pixels behind full threads, a full last thread, row offsets where the dword stores apply and where they do
    not; 9 x 1037 and 1037 x 9: 65 MCUs in a row / in a column, tens of workgroups of jpeg_idct_kernel. Each sampling
    alone, then the four in one batch."""
    H, W = size
    files = [(f"{H}x{W}_{s}", S.size_case(H, W, s)) for s in S.SAMPLINGS]
    coefs = _host_half(jpeg, files)
    for f, c in zip(files, coefs):
        assert c.shape == (H, W, 3), f[0]
        _check_reference([f], _raw_reconstruct(jpeg, [c]))
    _check_reference(files, _raw_reconstruct(jpeg, coefs))


def test_workload_sized_images_equal_the_reference(jpeg):
    """480 x 640 4:2:0 q75 and 333 x 500 4:2:2 q90, every pixel (the dataset test compares keypoints inside the boxes)."""
    files = [(n, S.source(n)) for n in ("480x640_420", "333x500_422")]
    coefs = _host_half(jpeg, files)
    assert [c.shape for c in coefs] == [(480, 640, 3), (333, 500, 3)]
    for f, c in zip(files, coefs):
        _check_reference([f], _raw_reconstruct(jpeg, [c]))


def test_batch_whose_bounds_come_from_different_images(jpeg):
    """480 x 640 with 1 x 1 and 5 x 257 - and 1037 x 9, 9 x 1037: max_blocks, max_height and max_width of the launch each come
    from another image, so most workgroups of every image but one lie outside it."""
    files = [("480x640_420", S.source("480x640_420")), ("1x1_420", S.encoded(1, 1, "420", 75, "noise", 0)), ("5x257_444", S.size_case(5, 257, "444"))]
    _check_reference(files, _raw_reconstruct(jpeg, _host_half(jpeg, files)))
    files = [("1037x9_422", S.size_case(1037, 9, "422")), ("1x1_420", files[1][1]), ("9x1037_grey", S.size_case(9, 1037, "grey")),
             ("333x500_422", S.source("333x500_422"))]
    _check_reference(files, _raw_reconstruct(jpeg, _host_half(jpeg, files)))


def test_transcoded_layouts_decode_on_the_device(jpeg):
    """Every must-decode layout of the small sources through ``imread_device``: no fallback, the reference's pixels; then the
    twelve layouts of a source as one guarded batch."""
    before = jpeg.fallbacks
    for name in S.SMALL_SOURCES:
        files = [(f"{name} {layout}", S.transcoded(name, layout)) for layout in S.LAYOUTS]
        src = np.ascontiguousarray(J.reconstruct_rgb(S.source_parsed(name))[:, :, ::-1])
        for label, data in files:
            got = jpeg.imread_device(data, DEV)
            assert got.is_cuda and got.dtype == torch.uint8, label
            _check_reference([(label, data)], [got.cpu().numpy()])
            assert np.array_equal(_reference_bgr(data), src), label  # (and those are the source's pixels)
        assert jpeg.fallbacks == before, f"a layout of {name} took the host decoder"
        _check_reference(files, _raw_reconstruct(jpeg, _host_half(jpeg, files)))


def test_streams_outside_the_subset_take_the_host_decoder(jpeg, tmp_path):
    """Three scans, 4:4:0, 4:1:1, Adobe transform 0, ids R G B without JFIF: one fallback each, the host decoder's pixels (or
    its exception), no JPEG launch."""
    jpeg._lib.reset_launch_counts()
    for name in S.REFUSED:
        data, word = S.refused(name)
        path = str(tmp_path / (name + ".jpg"))
        with open(path, "wb") as f:
            f.write(data)
        ref = _host_outcome(path)
        for src in (path, data):
            before = jpeg.fallbacks
            try:
                got = jpeg.imread_device(src, DEV)
            except Exception as e:  # noqa: BLE001
                got = e
            assert jpeg.fallbacks == before + 1, name
            if isinstance(ref, Exception):
                assert type(got) is type(ref) and str(got) == str(ref), (name, got, ref)
            else:
                assert isinstance(got, torch.Tensor) and got.is_cuda and torch.equal(got.cpu(), ref), name
        assert word.encode() in jpeg.probe(data).reason, name
    assert jpeg._lib.launch_count("jpeg_idct") == 0 and jpeg._lib.launch_count("jpeg_color") == 0 and jpeg._lib.launch_count("pp_jpeg.hip") == 0


def test_jpeg_differential_fuzz_against_the_reference():
    """tests/fuzz_jpeg.py for a few seconds: random sizes up to 700 a side around the kernels' thresholds, sampling, quality,
    content, stream layout, batches of 1..16 - no fallback, every image equal to tests/jpeg_ref.py byte for byte."""
    import subprocess

    r = subprocess.run([sys.executable, os.path.join(HERE, "fuzz_jpeg.py"), "8"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "JPEG FUZZ OK" in r.stdout, (r.stdout[-800:], r.stderr[-800:])


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
