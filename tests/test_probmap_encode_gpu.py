"""GPU: ``pp_probmap_encode`` / ``ProbMap.encode_device`` against the reference's targets (tests/golden/loss_cases.npz) and against the
host form at other shapes, inside canaries, with unchanged inputs and bit-identical repeat launches.

Map tolerance: 1 ulp of float32 per value (the float32 rounding of a float64 exp; device and numpy exp may differ in the last place).
Share of differing values on the golden batch against the reference: measured on an MI355X, 0 of 156 672 (largest difference 0 ulp). The
cap is that measured count plus a margin of the same size; as twice nothing admits nothing, it has a floor of 1 value, so that a single
last-place difference of another device libm build does not fail the suite (README, "Loss mode")."""
import numpy as np
import pytest
import torch

import probmap_loss_cases as C

DEV = "cuda:0"
CANARY = 0xA5
MEASURED_DIFFERING = 0  # of 156 672 values, golden batch, device exp against numpy's
CAP_DIFFERING = max(2 * MEASURED_DIFFERING, 1)


def ulp_distance(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def launch_in_canaries(kp, vis, H, W, in_size=(192, 256), sigma=-1.0):
    """One raw launch with every output inside a canary-filled buffer; returns the outputs and checks the guard bytes."""
    from probpose_code_amd import _lib

    B, K = vis.shape
    pad = 256
    sizes = dict(heatmaps=B * K * H * W * 4, keypoint_weights=B * K * 4, annotated=B * K, in_image=B * K)
    bufs = {n: torch.full((s + 2 * pad,), CANARY, dtype=torch.uint8, device=DEV) for n, s in sizes.items()}
    kp_d, vis_d = torch.from_numpy(kp).to(DEV), torch.from_numpy(vis).to(DEV)
    kp0, vis0 = kp_d.clone(), vis_d.clone()
    _lib.call("pp_probmap_encode", kp_d.data_ptr(), vis_d.data_ptr(), B, K, H, W, float(in_size[0]), float(in_size[1]), float(sigma),
              *(bufs[n].data_ptr() + pad for n in sizes), _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert torch.equal(kp_d, kp0) and torch.equal(vis_d, vis0), "inputs changed"
    out = {}
    for n, s in sizes.items():
        raw = bufs[n].cpu().numpy()
        assert (raw[:pad] == CANARY).all() and (raw[pad + s:] == CANARY).all(), f"{n}: write outside the buffer"
        out[n] = raw[pad:pad + s].copy()
    return dict(heatmaps=out["heatmaps"].view(np.float32).reshape(B, K, H, W), keypoint_weights=out["keypoint_weights"].view(np.float32).reshape(B, K),
                annotated=out["annotated"].reshape(B, K).astype(bool), in_image=out["in_image"].reshape(B, K).astype(bool))


@pytest.mark.gpu
def test_golden_batch_inside_canaries():
    g = C.golden()
    got = launch_in_canaries(g["keypoints"].copy(), g["keypoints_visible"].copy(), 64, 48)
    for name in ("keypoint_weights", "annotated", "in_image"):
        assert np.array_equal(got[name], g[name]), name  # exactly the reference's, the float64 underflow pair included
    d = ulp_distance(got["heatmaps"], g["heatmaps"])
    differing = int((d != 0).sum())
    print(f"device encode: {differing} of {d.size} map values differ from the reference, largest difference {int(d.max())} ulp")
    assert d.max() <= 1 and differing <= CAP_DIFFERING
    again = launch_in_canaries(g["keypoints"].copy(), g["keypoints_visible"].copy(), 64, 48)
    assert all(got[n].tobytes() == again[n].tobytes() for n in got), "a repeat launch is not bit-identical"


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (64, 48)])
@pytest.mark.parametrize("B", [1, 3])  # B K = 17 and 51: neither a multiple of a wave nor of a workgroup
def test_shapes_against_the_host_form(H, W, B):
    import probpose_code_amd as pp

    rng = np.random.default_rng(H * 100 + W + B)
    codec = pp.KEYPOINT_CODECS.build(dict(C.CODEC, heatmap_size=(W, H)))
    kp = np.stack([rng.uniform(-40, 232, (B, 17)), rng.uniform(-40, 296, (B, 17))], -1).astype(np.float32)
    vis = (rng.random((B, 17)) < 0.8).astype(np.float32)
    kp[0, 1] = (-3000.0, 10.0)
    vis[0, 1] = 1
    with np.errstate(all="ignore"):  # (a 1-pixel axis: scale factor inf, as the reference computes it)
        want = [codec.encode(kp[b:b + 1], vis[b:b + 1]) for b in range(B)]
    got = launch_in_canaries(kp.copy(), vis.copy(), H, W)
    for name in ("keypoint_weights", "annotated", "in_image"):
        assert np.array_equal(got[name], np.concatenate([w[name] for w in want])), name
    d = ulp_distance(got["heatmaps"], np.stack([w["heatmaps"] for w in want]))
    assert d.max() <= 1 and (d != 0).sum() <= max(1, CAP_DIFFERING * d.size // 156672)
    dev = codec.encode_device(torch.from_numpy(kp).to(DEV), torch.from_numpy(vis).to(DEV))
    assert dev["in_image"].dtype == torch.bool and np.array_equal(dev["heatmaps"].cpu().numpy(), got["heatmaps"])


@pytest.mark.gpu
def test_single_map_and_fixed_sigma():
    import probpose_code_amd as pp

    codec = pp.KEYPOINT_CODECS.build(dict(C.CODEC, sigma=1.5))
    kp, vis = np.array([[[100.5, 37.25]]], np.float32), np.ones((1, 1), np.float32)  # B K = 1, legal with a positive sigma
    got = launch_in_canaries(kp, vis, 64, 48, sigma=1.5)
    want = codec.encode(kp, vis)
    assert ulp_distance(got["heatmaps"][0], want["heatmaps"]).max() <= 1 and got["keypoint_weights"][0, 0] == 1
    from probpose_code_amd import _lib

    with pytest.raises(_lib.ProbPoseLibraryError, match="K must be 17"):  # the COCO sigma table: a status, never a launch
        _lib.call("pp_probmap_encode", 8, 8, 1, 1, 64, 48, 192.0, 256.0, -1.0, 8, 8, 8, 8, None)
