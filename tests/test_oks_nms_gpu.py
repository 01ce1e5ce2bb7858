"""Batched OKS-NMS on the MI355X (pp_oks_nms_batch): the kept sets are ``evaluation.oks_nms``'s index for index - the reference's
own on tests/golden/nms_cases.npz - whatever the last bits of the device's exp(); images with a pair next to the float32
rounding midpoint are reported undecided and decided on the host by ``CocoMetric``."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from oks_nms_cases import SEED, THRESHOLDS, make_batch, nearest_pair, sorted_arrays  # noqa: E402

NMS = np.load(os.path.join(HERE, "golden", "nms_cases.npz"))
CANARY = 0xA5
PAD = 4096
AREA_DTYPE = {0.5: np.float64, 0.7: np.float32, 0.9: np.float64}  # float32 areas: what bbox_scales give the metric


def _sigmas():
    from probpose_code_amd.evaluation import COCO_SIGMAS

    return COCO_SIGMAS


@pytest.fixture(scope="module")
def batches():
    """Per threshold: the seeded batch (its area dtype), the host's kept lists (computed once) and the pairs' distance to the midpoint."""
    from probpose_code_amd.evaluation import oks_nms, oks_nms_midpoint

    class Lazy(dict):
        def __missing__(self, thr):
            images = make_batch(SEED, AREA_DTYPE[thr])
            ref = [np.asarray(oks_nms([dict(keypoints=kp[i], score=sc[i], area=ar[i]) for i in range(len(kp))], thr), np.int64)
                   for kp, sc, ar in images]
            self[thr] = dict(images=images, ref=ref, near=nearest_pair(images, _sigmas(), oks_nms_midpoint(thr)))
            return self[thr]

    return Lazy()


def _launch(images, thr, guard, area_f32=False):
    """One pp_oks_nms_batch call inside canaries. Returns (kept index lists in pick order, status, raw keep / status bytes)."""
    import torch

    from probpose_code_amd import _lib

    dev = torch.device("cuda:0")
    arrays = [sorted_arrays(img) for img in images]
    off = np.cumsum([0] + [len(a[0]) for a in arrays]).astype(np.int64)
    N, n_img = int(off[-1]), len(images)
    kp_host = np.concatenate([a[0] for a in arrays]).reshape(N, 17, 3)
    ar_host = np.concatenate([a[1] for a in arrays]).astype(np.float64)
    kp, ar = torch.from_numpy(kp_host).to(dev), torch.from_numpy(ar_host).to(dev)
    sg = torch.from_numpy(np.asarray(_sigmas(), np.float64)).to(dev)
    size = _lib.lib.pp_oks_nms_workspace_bytes(off.ctypes.data, N, n_img)
    assert size > 0
    ws = torch.full((PAD + size + PAD,), CANARY, dtype=torch.uint8, device=dev)
    keep = torch.full((PAD + N + PAD,), CANARY, dtype=torch.uint8, device=dev)
    status = torch.full((PAD + n_img + PAD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    assert (ws.data_ptr() + PAD) % 8 == 0
    _lib.call("pp_oks_nms_batch", kp.data_ptr(), ar.data_ptr(), off.ctypes.data, sg.data_ptr(), N, n_img, 17, float(thr), float(guard),
              int(area_f32), ws.data_ptr() + PAD, size, keep.data_ptr() + PAD, status.data_ptr() + 4 * PAD,
              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    k, s, w = keep.cpu().numpy(), status.cpu().numpy(), ws.cpu().numpy()
    assert (k[:PAD] == CANARY).all() and (k[PAD + N:] == CANARY).all(), "bytes outside keep written"
    assert (s[:PAD] == 0x5A5A5A5A).all() and (s[PAD + n_img:] == 0x5A5A5A5A).all(), "words outside status written"
    assert (w[:PAD] == CANARY).all() and (w[PAD + size:] == CANARY).all(), "bytes outside the workspace written"
    assert np.array_equal(kp.cpu().numpy(), kp_host, equal_nan=True) and np.array_equal(ar.cpu().numpy(), ar_host), "inputs changed"
    k, s = k[PAD:PAD + N], s[PAD:PAD + n_img]
    assert set(np.unique(k)) <= {0, 1}
    kept = [a[2][k[off[n]:off[n + 1]].astype(bool)] for n, a in enumerate(arrays)]
    return kept, s, (k.tobytes(), s.tobytes())


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_seed_leaves_at_most_one_percent_of_the_images_next_to_the_midpoint(thr):
    """numpy alone: the zero-fallback assertion below leaves out images with a pair within 1e-9 of the midpoint."""
    from probpose_code_amd.evaluation import oks_nms_midpoint

    images = make_batch(SEED, AREA_DTYPE[thr])
    assert len(images) == 300 and [len(i[0]) for i in images[:8]] == [0, 1, 2, 63, 64, 65, 128, 129]
    near = nearest_pair(images, _sigmas(), oks_nms_midpoint(thr))
    assert (near <= 1e-9).sum() <= 3
    assert thr != 0.7 or (near < 5e-4).sum() >= 1, "no image for the wide-guard test (which runs at 0.7)"
    assert any(len(np.unique(sc)) < len(sc) for _, sc, _ in images) and np.isnan(images[5][0]).sum() == 1  # tied scores, the NaN


@pytest.mark.gpu
def test_golden_cases_as_one_mixed_batch():
    from probpose_code_amd import _lib

    cases = [(NMS[f"n{n}/kpts"], NMS[f"n{n}/score"], NMS[f"n{n}/area"]) for n in range(int(NMS["n_cases"]))]
    thrs = [float(NMS[f"n{n}/thr"]) for n in range(len(cases))]
    checked = 0
    for thr in sorted(set(thrs)):  # one threshold per call: the whole batch at each, the cases of that threshold held to the fixture
        kept, status, _ = _launch(cases, thr, 2.0 ** -40)
        for n, t in enumerate(thrs):
            if t == thr:
                assert status[n] == _lib.PP_OKS_NMS_DECIDED, n
                assert np.array_equal(kept[n], NMS[f"n{n}/keep"]), (n, kept[n], NMS[f"n{n}/keep"])
                checked += 1
    assert checked == len(cases) == 6


@pytest.mark.gpu
@pytest.mark.parametrize("thr", THRESHOLDS)
def test_random_batch_equals_the_host_and_needs_no_fallback(batches, thr):
    from probpose_code_amd import _lib

    b = batches[thr]
    f32 = AREA_DTYPE[thr] == np.float32
    kept, status, raw = _launch(b["images"], thr, 2.0 ** -40, f32)
    left_out = b["near"] <= 1e-9
    assert left_out.sum() <= 3
    assert (status[~left_out] == _lib.PP_OKS_NMS_DECIDED).all(), np.nonzero(status != 0)[0]
    suppressed = 0
    for n, (got, ref) in enumerate(zip(kept, b["ref"])):
        if status[n] == _lib.PP_OKS_NMS_DECIDED:
            assert np.array_equal(got, ref), (n, len(b["images"][n][0]))
            suppressed += len(b["images"][n][0]) - len(ref)
    assert suppressed > 1000  # the clusters made it a real suppression
    # a second launch on the same input: the same bytes
    assert _launch(b["images"], thr, 2.0 ** -40, f32)[2] == raw


def _metric_inputs(images, first_img_id=0):
    """The batch as ``CocoMetric.results`` entries: keypoint scores of 1 make the instance score the (tied) bbox score."""
    res, nid = [], 0
    for n, (kp, sc, ar) in enumerate(images):
        for i in range(len(kp)):
            res.append(dict(id=nid, img_id=first_img_id + n, category_id=1, keypoints=kp[i:i + 1, :, :2], keypoint_scores=np.ones((1, 17)),
                            keypoints_visible=np.ones((1, 17)), keypoint_probs=kp[i:i + 1, :, 2], bbox_scores=sc[i:i + 1], areas=ar[i:i + 1]))
            nid += 1
    return res


def _kept_ids(valid):
    return {img: [(p["id"], float(p["score"])) for p in persons] for img, persons in valid.items()}


@pytest.mark.gpu
def test_coco_metric_device_backend_equals_the_host_backend(batches):
    from probpose_code_amd.evaluation import CocoMetric

    thr = 0.7  # float32 areas, as the test loop produces them
    b = batches[thr]
    images = [img for img, near in zip(b["images"], b["near"]) if near > 1e-9]
    host, dev = CocoMetric([], nms_thr=thr), CocoMetric([], nms_thr=thr, nms_backend="device", device="cuda:0")
    host.results, dev.results = _metric_inputs(images), _metric_inputs(images)
    ref, got = host._instances(), dev._instances()
    assert list(got) == list(ref) and _kept_ids(got) == _kept_ids(ref)
    assert dev.nms_fallbacks == 0 and host.nms_fallbacks == 0
    assert sum(len(v) for v in ref.values()) < sum(len(i[0]) for i in images)


@pytest.mark.gpu
def test_wide_guard_reports_the_predicted_images_and_the_metric_falls_back(batches):
    from probpose_code_amd import _lib
    from probpose_code_amd.evaluation import CocoMetric

    thr = 0.7
    b = batches[thr]
    kept, status, _ = _launch(b["images"], thr, 1e-3, True)
    must, may = b["near"] < 5e-4, b["near"] < 2e-3
    und = status == _lib.PP_OKS_NMS_UNDECIDED
    assert und.sum() >= 1 and must.sum() >= 1
    assert (und[must]).all() and not (und[~may]).any(), (np.nonzero(must)[0], np.nonzero(und)[0])
    assert set(np.unique(status)) <= {_lib.PP_OKS_NMS_DECIDED, _lib.PP_OKS_NMS_UNDECIDED}
    for n in np.nonzero(~und)[0]:
        assert np.array_equal(kept[n], b["ref"][n]), n
    host = CocoMetric([], nms_thr=thr)
    dev = CocoMetric([], nms_thr=thr, nms_backend="device", nms_guard=1e-3, device="cuda:0")
    host.results, dev.results = _metric_inputs(b["images"]), _metric_inputs(b["images"])
    assert _kept_ids(dev._instances()) == _kept_ids(host._instances())
    assert must.sum() <= dev.nms_fallbacks <= may.sum()


@pytest.mark.gpu
def test_capacity_and_one_above():
    from probpose_code_amd import _lib
    from probpose_code_amd.evaluation import CocoMetric, oks_nms

    cap = _lib.PP_OKS_NMS_MAX_PER_IMAGE
    assert cap >= 1024
    rng = np.random.default_rng(3)
    images = []
    for n in (cap, cap + 1):  # 8 distinct poses repeated: the host check stays cheap
        poses = np.concatenate([rng.uniform(50, 400, (8, 17, 2)), rng.uniform(0, 1, (8, 17, 1))], -1)
        which = rng.integers(0, 8, n)
        images.append((poses[which], np.round(rng.uniform(0.1, 1.0, n), 3), rng.uniform(3000, 30000, 8)[which]))
    kept, status, _ = _launch(images, 0.9, 2.0 ** -40)
    assert status.tolist() == [_lib.PP_OKS_NMS_DECIDED, _lib.PP_OKS_NMS_HOST]
    ref = [np.asarray(oks_nms([dict(keypoints=kp[i], score=sc[i], area=ar[i]) for i in range(len(kp))], 0.9), np.int64) for kp, sc, ar in images]
    assert np.array_equal(kept[0], ref[0]) and len(ref[0]) == 8 and len(kept[1]) == 0
    dev = CocoMetric([], nms_thr=0.9, nms_backend="device", device="cuda:0")
    dev.results = _metric_inputs(images)
    got = dev._instances()
    assert dev.nms_fallbacks == 1
    for n in range(2):
        first = sum(len(i[0]) for i in images[:n])
        assert [p["id"] - first for p in got[n]] == ref[n].tolist()
