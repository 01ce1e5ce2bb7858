"""Pin the loss mode - ``ProbMap.encode`` and ``ProbMapHead.loss`` - to the REFERENCE's own code.

Run in the build container only (needs the reference tree):

    python tests/golden/make_golden_loss.py     ->  tests/golden/loss_cases.npz, tests/golden/loss_target_maps.npz

What runs here is the reference's own code, imported file by file behind the stubs of ``make_golden_head.load_reference_model``
(the head, the codecs, ``to_numpy``) plus this script's own loader for what that one stubs away:

    mmpose/models/losses/heatmap_loss.py, classification_loss.py, regression_loss.py   the REAL loss modules, registered in the stub
                                                                                       ``MODELS`` registry in place of nn.Identity
    mmpose/evaluation/functional/keypoint_eval.py                                      the REAL ``pose_pck_accuracy``
    mmpose.models.utils.realnvp.RealNVP                                                -> None (RLELoss only)
    cv2.GaussianBlur                                                                   -> tests/udp_ref.blur, as make_golden_codecs.py
                                                                                          (UNPINNED there and here: cv2 is not installed
                                                                                          where this ran; it reaches gt_oks only)

The reference's ``ProbMapHead.loss`` itself runs: the head is built by its own ``__init__`` from the ProbPose config block, its
``forward`` is replaced by a function that returns the seeded maps and tower outputs of the fixture (so the fixture carries no
backbone), the samples hold what ``ProbMap.encode`` + ``PackPoseInputs`` put there. Recorded: the inputs, every target
(``ProbMap.encode``'s dictionary per instance), the intermediates (``gt_oks``, ``oks_weight``, the visibility weights, the per-map sums
of the per-pixel loss) and every entry of the loss dictionary under ``np.random.seed(0)``. Data only.

The instances hold between them: an unannotated keypoint; an annotated keypoint outside the input; a keypoint so far outside that its
float64 map is all zero (the script ASSERTS that the reference gives it weight 0, and weight 1 to one placed just inside that
distance); a keypoint on x = input width (in_image false) and one on x = 0 (true); an instance without any valid keypoint
(oks_weight 0); a predicted map that is all zero.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import make_golden_head as GH  # noqa: E402  (its loader and stubs; importing it runs nothing)
import udp_ref as R  # noqa: E402
from _ref_import import REF, _load, _shell  # noqa: E402

B, K, H, W = 3, 17, 64, 48
IN_W, IN_H = 192, 256


def load_reference_loss():
    """The reference head with its REAL loss modules and accuracy function. Returns (ProbMapHead, ProbMap codec class, head module)."""
    ns, reg, ProbMapHead, _ = GH.load_reference_model()
    cv2 = sys.modules["cv2"]

    def gaussian_blur_stub(src, ksize, sigma_x, dst=None):
        assert ksize[0] == ksize[1] and sigma_x == 0 and src.dtype == np.float32
        out = R.blur(src, ksize[0], np.float32, border="reflect")
        if dst is not None:
            dst[...] = out
            return dst
        return out

    cv2.GaussianBlur = gaussian_blur_stub
    _shell("mmpose.models.utils.realnvp").RealNVP = None
    _shell("mmpose.models.losses", os.path.join(REF, "mmpose/models/losses"))
    for f in ("heatmap_loss", "classification_loss", "regression_loss"):  # @MODELS.register_module() replaces the Identity stubs
        _load("mmpose.models.losses." + f, f"mmpose/models/losses/{f}.py")
    for name in ("OKSHeatmapLoss", "BCELoss", "MSELoss", "L1LogLoss"):
        assert isinstance(reg.MODELS.module_dict[name], type), name
    _shell("mmpose.evaluation.functional", os.path.join(REF, "mmpose/evaluation/functional"))
    ke = _load("mmpose.evaluation.functional.keypoint_eval", "mmpose/evaluation/functional/keypoint_eval.py")
    head_mod = sys.modules["mmpose.models.heads.hybrid_heads.probmap_head"]
    head_mod.pose_pck_accuracy = ke.pose_pck_accuracy
    return ProbMapHead, ns.probmap.ProbMap, head_mod


def first_all_zero_x(codec, k, y):
    """The float32 input-space x < 0 closest to the map at which keypoint k (on row y) still has weight 1, and the next float32
    steps further out until the reference gives weight 0: (inside, outside)."""
    def weight(x):
        kp = np.zeros((1, K, 2), np.float32)
        kp[0, k] = (x, y)
        vis = np.zeros((1, K), np.float32)
        vis[0, k] = 1
        return codec.encode(kp, vis)["keypoint_weights"][0, k]

    lo, hi = np.float32(-50.0), np.float32(-2000.0)  # weight 1 at lo, 0 at hi
    assert weight(lo) == 1 and weight(hi) == 0
    while True:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            break
        if weight(mid) == 1:
            lo = mid
        else:
            hi = mid
    return lo, hi


def blob(cx, cy, amp, sig):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sig * sig))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)  # the reference's fp32 sums in one fixed order
    ProbMapHead, ProbMap, head_mod = load_reference_loss()
    codec = ProbMap(input_size=(IN_W, IN_H), heatmap_size=(W, H), sigma=-1)
    rng = np.random.default_rng(20)

    # ---- keypoints, flags
    kp = np.stack([rng.uniform(8, IN_W - 8, (B, K)), rng.uniform(8, IN_H - 8, (B, K))], -1).astype(np.float32)
    visible = np.ones((B, K), np.float32)
    visibility = (rng.random((B, K)) < 0.6).astype(np.float32)
    inside_x, outside_x = first_all_zero_x(codec, 5, 128.0)
    visible[0, 3] = 0                       # unannotated
    visibility[0, 3] = 0
    kp[0, 4] = (-10.0, 100.0)               # annotated, outside the input
    kp[0, 5] = (outside_x, 128.0)           # so far outside that the float64 map is all zero
    kp[0, 6] = (IN_W, 40.0)                 # exactly on x = input width: in_image false
    kp[0, 7] = (0.0, 60.0)                  # exactly on x = 0: in_image true
    kp[1, 5] = (inside_x, 128.0)            # one float32 step inside that distance: weight 1
    kp[1, 9] = (100.0, IN_H)                # exactly on y = input height
    visible[1, 12] = 0
    for k in range(K):                      # instance 2: no valid keypoint at all - unannotated or outside
        if k % 2:
            visible[2, k] = 0
            visibility[2, k] = 0
        else:
            kp[2, k] = (IN_W + 5.0 + k, 20.0 + 10 * k)
    visibility = visibility * visible       # (COCO: v = 2 implies labelled)

    # ---- the reference's targets, one instance at a time
    enc = [codec.encode(kp[b:b + 1], visible[b:b + 1], keypoints_visibility=visibility[b:b + 1]) for b in range(B)]
    assert enc[0]["keypoint_weights"][0, 5] == 0 and enc[1]["keypoint_weights"][0, 5] == 1, "the underflow pair"
    assert not enc[0]["in_image"][0, 6] and enc[0]["in_image"][0, 7] and not enc[0]["in_image"][0, 4]
    assert not (enc[2]["in_image"][0] & enc[2]["annotated"][0]).any()
    gt_maps = np.stack([e["heatmaps"] for e in enc])
    assert gt_maps.dtype == np.float32 and not gt_maps[0, 5].any() and gt_maps[1, 5].any() is not None

    # ---- seeded predictions: blobs near the targets plus sparse noise, on a 2^-12 grid in [0, 1]; one all-zero map; tower outputs
    dt_maps = np.zeros((B, K, H, W), np.float64)
    for b in range(B):
        for k in range(K):
            cx, cy = kp[b, k, 0] / (IN_W - 1) * (W - 1), kp[b, k, 1] / (IN_H - 1) * (H - 1)
            cx, cy = np.clip(cx, 0, W - 1) + rng.normal(0, 1.0), np.clip(cy, 0, H - 1) + rng.normal(0, 1.0)
            m = blob(cx, cy, rng.uniform(0.05, 0.4), rng.uniform(0.8, 2.0))
            m = m + (rng.random((H, W)) < 0.01) * rng.uniform(0, 0.1, (H, W))
            m[m < 1e-3] = 0
            dt_maps[b, k] = m
    dt_maps[1, 2] = 0                       # a predicted map that is all zero
    dt_maps[0, 0, 10, 7] = dt_maps[0, 0].max() * 0 + 0.5  # ties for the argmax: the same maximum at two pixels
    dt_maps[0, 0, 40, 30] = 0.5
    dt_maps = (np.round(np.clip(dt_maps, 0, 1) * 4096) / 4096).astype(np.float32)
    scalars = np.stack([rng.uniform(0.02, 0.98, (B, K)), rng.uniform(0.02, 0.98, (B, K)), rng.uniform(0.02, 0.98, (B, K)),
                        rng.uniform(0.0, 5.0, (B, K))]).astype(np.float32)

    # ---- the reference head: its own __init__ (real loss modules), its own loss()
    cfg = dict(GH.HEAD_CFG)
    cfg.pop("type")
    head = ProbMapHead(**cfg).eval()
    assert type(head.keypoint_loss_module).__name__ == "OKSHeatmapLoss" and type(head.error_loss_module).__name__ == "L1LogLoss"
    outs = tuple([torch.from_numpy(dt_maps)] + [torch.from_numpy(scalars[i]).reshape(B, K, 1, 1) for i in range(4)])
    head.forward = lambda feats: outs
    samples = []
    for b in range(B):
        ds = GH.PoseDataSample()
        ds.gt_fields = GH.PixelData(heatmaps=torch.from_numpy(enc[b]["heatmaps"]))
        ds.gt_instances = GH.InstanceData(in_image=enc[b]["in_image"], keypoints_visible=visible[b:b + 1], keypoints_visibility=visibility[b:b + 1])
        ds.gt_instance_labels = GH.InstanceData(keypoint_weights=torch.from_numpy(enc[b]["keypoint_weights"]))
        samples.append(ds)
    seen = {}
    oks_from = head._oks_from_heatmaps

    def oks_spy(gt, dt, weight):
        seen["gt_oks"], seen["oks_weight"] = oks_from(gt, dt, weight)
        return seen["gt_oks"], seen["oks_weight"]

    head._oks_from_heatmaps = oks_spy
    head.visibility_loss_module.register_forward_pre_hook(lambda m, a: seen.__setitem__("vis_weights", a[2].detach().clone()))
    head.keypoint_loss_module.register_forward_hook(lambda m, a, o: seen.__setitem__("pixel_loss", o.detach().clone()))
    np.random.seed(0)
    with torch.no_grad():
        losses = head.loss(None, samples)
    assert float(seen["oks_weight"][2]) == 0 and float(seen["oks_weight"][0]) == 1

    out = dict(keypoints=kp, keypoints_visible=visible, keypoints_visibility=visibility, pred_maps_q12=np.round(dt_maps * 4096).astype(np.int16),
               pred_scalars=scalars, keypoint_weights=np.concatenate([e["keypoint_weights"] for e in enc]),
               annotated=np.concatenate([e["annotated"] for e in enc]), in_image=np.concatenate([e["in_image"] for e in enc]),
               keypoints_scaled=np.concatenate([e["keypoints_scaled"] for e in enc]),
               heatmap_keypoints=np.concatenate([e["heatmap_keypoints"] for e in enc]),
               encode_keys=np.array(sorted(enc[0].keys())), encode_dtypes=np.array([str(np.asarray(enc[0][k]).dtype) for k in sorted(enc[0].keys())]),
               identification_similarity=np.array(enc[0]["identification_similarity"]),
               underflow_x=np.array([inside_x, outside_x], np.float32),
               gt_oks=seen["gt_oks"].numpy(), oks_weight=seen["oks_weight"].numpy(), vis_weights=seen["vis_weights"].numpy(),
               pixel_loss_map_sums=seen["pixel_loss"].double().sum((2, 3)).numpy(), pixel_loss_dtype=np.array(str(seen["pixel_loss"].dtype)),
               seed=np.array(0))
    for name, v in losses.items():
        out["loss_" + name] = v.detach().cpu().numpy()
        out["lossdtype_" + name] = np.array(str(v.dtype))
    out["loss_keys"] = np.array(list(losses.keys()))
    np.savez_compressed(os.path.join(HERE, "loss_cases.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "loss_target_maps.npz"), heatmaps=gt_maps)
    for f in ("loss_cases.npz", "loss_target_maps.npz"):
        print(f"wrote tests/golden/{f}: {os.path.getsize(os.path.join(HERE, f)) / 1024:.0f} KiB")
    print({k: (float(np.ravel(v.detach().numpy())[0])) for k, v in losses.items()})
    print("underflow pair (inside, outside):", inside_x, outside_x)


if __name__ == "__main__":
    main()
