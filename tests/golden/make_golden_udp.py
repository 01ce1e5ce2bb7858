"""Generates tests/golden/udp_decode_cases.npz from the REFERENCE's own ``get_heatmap_maximum``, ``gaussian_blur``,
``refine_keypoints_dark_udp`` (mmpose/codecs/utils), ``UDPHeatmap.decode`` (mmpose/codecs/udp_heatmap.py) and ``flip_heatmaps``
(mmpose/models/utils/tta.py), loaded file by file behind stubs of this script's own. Inputs and outputs only. Run in the build
container (the reference does not travel):
    python tests/golden/make_golden_udp.py

UNPINNED: ``cv2`` is not installed where this ran. The reference's ``gaussian_blur`` calls ``cv2.GaussianBlur(padded, (ks, ks),
0)``; the stub below supplies it as tests/udp_ref.blur with cv2's default border (BORDER_REFLECT_101) on the padded array - a
separable fp32 blur, taps from sigma = 0.3 ((ks - 1) / 2 - 1) + 0.8 normalised in double and rounded to fp32, rows first, taps
ascending, one rounding per operator. The reference pads by (ks - 1) / 2 zeros first, so no border mode reaches the kept region;
what is NOT pinned is the order of cv2's own fp32 sums (its vectorised filters pair the symmetric taps). On a box with cv2:
drop the stub (``import cv2`` first), re-run this script, and run tests/test_udp_references.py - the bit-for-bit comparison of
the stepwise form then shows whether udp_ref.blur has to follow cv2's summation order; the error bound has room for either.
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import udp_ref as R  # noqa: E402

REF = os.environ.get("PROBPOSE_REFERENCE", "/root/reference")


def _shell(name, path=None):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    sys.modules[name] = m
    return m


def _load(name, relpath):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class _Registry:
    def register_module(self, name=None, force=False, module=None):
        return (lambda cls: cls) if module is None else module


def load_reference():
    cv2 = _shell("cv2")

    def gaussian_blur_stub(src, ksize, sigma_x, dst=None):
        assert ksize[0] == ksize[1] and sigma_x == 0 and src.dtype == np.float32
        out = R.blur(src, ksize[0], np.float32, border="reflect")
        if dst is not None:
            dst[...] = out
            return dst
        return out

    cv2.GaussianBlur = gaussian_blur_stub
    _shell("mmpose", os.path.join(REF, "mmpose"))
    _shell("mmpose.codecs", os.path.join(REF, "mmpose/codecs"))
    mmengine = _shell("mmengine")
    mmengine.utils = _shell("mmengine.utils")
    mmengine.utils.is_method_overridden = lambda method, base, derived: getattr(
        derived if isinstance(derived, type) else derived.__class__, method) != getattr(base, method)
    _shell("mmpose.registry").KEYPOINT_CODECS = _Registry()
    ns = types.SimpleNamespace()
    ns.utils = importlib.import_module("mmpose.codecs.utils")
    _load("mmpose.codecs.base", "mmpose/codecs/base.py")
    ns.UDPHeatmap = _load("mmpose.codecs.udp_heatmap", "mmpose/codecs/udp_heatmap.py").UDPHeatmap
    ns.flip_heatmaps = _load("_ref_tta_udp", "mmpose/models/utils/tta.py").flip_heatmaps
    return ns


def blob(H, W, cx, cy, amp=1.0, sig=2.0):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sig * sig))


def build_cases(rng):
    cases = {}
    H, W = 16, 12
    # blobs inside, on and up to two pixels beyond every border and corner
    centres = [(5.3, 7.6), (0.0, 8.2), (W - 1.0, 3.1), (4.4, 0.0), (6.6, H - 1.0), (-1.0, 5.5), (W + 0.0, 9.5), (3.5, -2.0),
               (7.5, H + 1.0), (-2.0, -2.0), (W + 1.0, H + 1.0), (-1.5, H + 0.5), (W + 0.5, -1.0), (0.4, 0.3), (W - 1.4, H - 1.2),
               (5.0, 5.0), (6.5, 8.5)]
    m = np.stack([blob(H, W, cx, cy, rng.uniform(0.5, 1.0)) for cx, cy in centres]) + rng.normal(0, 0.005, (len(centres), H, W))
    cases["blobs_16x12"] = (m, 11)
    cases["blobs_16x12_ks17"] = (m + rng.normal(0, 0.005, m.shape), 17)
    # two near-equal peaks, exact ties (first index wins), a flat map, a single hot pixel in every corner
    tp = [blob(H, W, 3, 4, 0.8) + blob(H, W, 8, 11, 0.8 * s) for s in (1.0, 1 + 1e-6, 1 - 1e-6)]
    tie = np.zeros((H, W))
    tie[[2, 9, 13], [7, 3, 10]] = 0.75
    quant = np.round(rng.random((H, W)) * 4) / 4
    corners = []
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        c = np.zeros((H, W))
        c[y, x] = 0.9
        corners.append(c)
    cases["peaks_ties_flat_16x12"] = (np.stack(tp + [tie, quant, np.full((H, W), 0.3)] + corners), 11)
    # the reference's read outside the map (loc = (-1, -1)): non-positive maps next to maps with mass in the bottom-right corner, also
    # at k = 0 (the negative index reads the LAST map)
    br = blob(H, W, W - 1.2, H - 1.4, 0.9)
    cases["nonpositive_16x12"] = (np.stack([np.full((H, W), -0.1), blob(H, W, 4, 6, 0.7), np.zeros((H, W)), br,
                                           -np.abs(rng.normal(0, 0.1, (H, W))), br * 0.6 + rng.normal(0, 0.005, (H, W))]), 11)
    cases["nonpositive_three_16x12"] = (np.stack([np.full((H, W), -0.1), np.zeros((H, W)), br]), 11)
    cases["nonpositive_empty_corner_16x12"] = (np.stack([np.full((H, W), -0.1), np.zeros((H, W)), blob(H, W, 3, 3, 0.9)]), 11)
    cases["nonpositive_single_map_16x12"] = (np.stack([-br]), 11)
    cases["nonpositive_16x12_ks17"] = (np.stack([br, np.full((H, W), -0.2), np.zeros((H, W))]), 17)
    # the two model sizes
    for (h, w, k, ks) in ((64, 48, 8, 11), (96, 72, 3, 17)):
        mm = np.stack([blob(h, w, rng.uniform(-2, w + 1), rng.uniform(-2, h + 1), rng.uniform(0.5, 1.0)) for _ in range(k)])
        mm = mm + rng.normal(0, 0.01, mm.shape)
        mm[k - 1] = -np.abs(mm[k - 1]) * 0.1  # (its neighbour k - 2 may or may not reach the corner)
        mm[k - 2] = blob(h, w, w - 1.5, h - 1.0, 0.8) + rng.normal(0, 0.01, (h, w))
        cases[f"model_{h}x{w}"] = (mm, ks)
    return {n: (np.ascontiguousarray(m, np.float32), ks) for n, (m, ks) in cases.items()}


def main():
    ref = load_reference()
    rng = np.random.default_rng(20261016)
    out = {}
    names = []
    for name, (maps, ks) in build_cases(rng).items():
        K, H, W = maps.shape
        input_size = (4 * W, 4 * H)
        codec = ref.UDPHeatmap(input_size=input_size, heatmap_size=(W, H), sigma=2 if ks == 11 else 3, blur_kernel_size=ks)
        kp, sc = codec.decode(maps.copy())
        locs, vals = ref.utils.get_heatmap_maximum(maps.copy())
        refined = ref.utils.refine_keypoints_dark_udp(locs.copy()[None], maps.copy(), ks)
        assert refined.dtype == np.float32 and kp.dtype == np.float64 and sc.dtype == np.float32
        names.append(name)
        out.update({f"{name}.maps": maps, f"{name}.ks": np.int32(ks), f"{name}.input_size": np.array(input_size), f"{name}.keypoints": kp,
                    f"{name}.scores": sc, f"{name}.locs": locs, f"{name}.refined": refined})
        if H * W <= 192:  # (the modulated maps of the small cases only: the fixture stays a few hundred KiB)
            out[f"{name}.blurred"] = ref.utils.gaussian_blur(maps.copy(), ks)
    # what the issue states for three 16 x 12 maps (map 0 at -0.1, a blob in the last map's bottom-right corner): keypoint 0 leaves (-1, -1)
    print("nonpositive_three_16x12 keypoint 0 (heatmap px):", out["nonpositive_three_16x12.refined"][0, 0],
          " empty corner:", out["nonpositive_empty_corner_16x12.refined"][0, 0])
    # the flip-test average of HeatmapHead.predict (heatmap_head.py:246-258), with and without shift_heatmap
    flip_indices = [0, 2, 1, 4, 3, 6, 5]
    a = np.stack([[blob(16, 12, rng.uniform(0, 11), rng.uniform(0, 15), 0.8) for _ in range(7)] for _ in range(2)]).astype(np.float32)
    b = (a[:, flip_indices][..., ::-1] + rng.normal(0, 0.01, a.shape)).astype(np.float32)
    out.update({"flip.a": a, "flip.b": np.ascontiguousarray(b), "flip.flip_indices": np.array(flip_indices), "flip.ks": np.int32(11),
                "flip.input_size": np.array((48, 64))})
    codec = ref.UDPHeatmap(input_size=(48, 64), heatmap_size=(12, 16), sigma=2, blur_kernel_size=11)
    for shift in (False, True):
        fb = ref.flip_heatmaps(torch.from_numpy(b.copy()), flip_mode="heatmap", flip_indices=flip_indices, shift_heatmap=shift)
        avg = ((torch.from_numpy(a) + fb) * 0.5).numpy()
        dec = [codec.decode(avg[i]) for i in range(2)]
        tag = "flip.shift" if shift else "flip.plain"
        out.update({f"{tag}.avg": avg, f"{tag}.keypoints": np.concatenate([d[0] for d in dec]), f"{tag}.scores": np.concatenate([d[1] for d in dec])})
    out["names"] = np.array(names)
    path = os.path.join(HERE, "udp_decode_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
