"""Generates tests/golden/codec_swap_cases.npz from the REFERENCE's own ``UDPExpMaxHeatmap.decode``
(mmpose/codecs/udp_expmax_heatmap.py), ``ArgMaxProbMap.decode`` (mmpose/codecs/argmax_probmap.py) and ``flip_heatmaps``
(mmpose/models/utils/tta.py), loaded file by file behind stubs of this script's own. Inputs, outputs and the two classes' constructor
defaults only. Run in the build container (the reference does not travel):
    python tests/golden/make_golden_codecs.py

UNPINNED (as tests/golden/make_golden_udp.py): ``cv2`` is not installed where this ran. The reference's ``gaussian_blur`` calls
``cv2.GaussianBlur(padded, (ks, ks), 0)``; the stub below supplies it as tests/udp_ref.blur with cv2's default border
(BORDER_REFLECT_101) on the padded array - a separable fp32 blur, taps from sigma = 0.3 ((ks - 1) / 2 - 1) + 0.8 normalised in double
and rounded to fp32, rows first, taps ascending, one rounding per operator. The reference pads by (ks - 1) / 2 zeros first, so no
border mode reaches the kept region; what is NOT pinned is the order of cv2's own fp32 sums. On a box with cv2: drop the stub, re-run
this script and the tests that read the fixture - the keypoint bound of the ArgMax cases has room for either order.

The ExpMax half is pinned: the generator asserts, for every case it writes, that ``oracle.decode_ref.probmap_decode`` (both
backends) equals the reference class bit for bit. A mismatch is a finding about the oracle.

The values are quantised (maps to 2^-9, logits to 2^-8) and stored as int16 steps, so that the compressed fixture stays a few hundred
KiB; they are inputs like any other.
"""
import importlib
import importlib.util
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import udp_ref as R  # noqa: E402
from oracle import decode_ref  # noqa: E402

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
    ns.UDPExpMaxHeatmap = _load("mmpose.codecs.udp_expmax_heatmap", "mmpose/codecs/udp_expmax_heatmap.py").UDPExpMaxHeatmap
    ns.ArgMaxProbMap = _load("mmpose.codecs.argmax_probmap", "mmpose/codecs/argmax_probmap.py").ArgMaxProbMap
    ns.flip_heatmaps = _load("_ref_tta_codecs", "mmpose/models/utils/tta.py").flip_heatmaps
    return ns


def blob(H, W, cx, cy, amp=1.0, sig=2.0):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sig * sig))


def quant(a, bits):
    return (np.round(np.asarray(a, np.float64) * 2.0 ** bits) / 2.0 ** bits + 0.0).astype(np.float32)  # (+ 0.0: no negative zeros)


def sparsemax(z):
    """Sparsemax over the last axis (Martins & Astudillo 2016, sort form), fp64 -> fp32."""
    z = np.asarray(z, np.float64)
    s = -np.sort(-z, axis=-1)
    cs = np.cumsum(s, axis=-1)
    k = np.arange(1, z.shape[-1] + 1)
    supp = (1 + k * s > cs).sum(-1, keepdims=True)
    tau = (np.take_along_axis(cs, supp - 1, -1) - 1) / supp
    return np.clip(z - tau, 0, None).astype(np.float32)


def pack(out, key, arr, bits):
    """A quantised array as int16 steps of 2^-bits (exact; ``unpack`` of tests/test_codec_swap_host.py gives the fp32 values back)."""
    q = np.round(np.asarray(arr, np.float64) * 2.0 ** bits)
    assert np.array_equal((q / 2.0 ** bits + 0.0).astype(np.float32).view(np.int32), arr.view(np.int32)) and np.abs(q).max() < 2 ** 15
    out[key] = q.astype(np.int16)
    out[key + ".scale"] = np.float32(2.0 ** bits)


FLIP17 = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]


def defaults_of(cls):
    return {n: p.default for n, p in inspect.signature(cls.__init__).parameters.items() if p.default is not inspect.Parameter.empty}


def expmax_cases(ref, rng, out):
    """Seventeen blobs (sigma 2, amplitude 0.3 - 1.6, centres from 2 px outside to inside every border) + N(0, 0.02) - 0.01: values
    below 0 and above 1 occur. Per size: the plain pass, the flipped pass, and their average with and without shift."""
    names, n_kpts = [], 0
    for (H, W) in ((16, 16), (16, 12), (64, 48), (96, 72)):
        centres = [(rng.uniform(2, W - 3), rng.uniform(2, H - 3)) for _ in range(5)]
        centres += [(-2.0, rng.uniform(0, H - 1)), (W + 1.0, rng.uniform(0, H - 1)), (rng.uniform(0, W - 1), -2.0), (rng.uniform(0, W - 1), H + 1.0),
                    (0.0, rng.uniform(0, H - 1)), (W - 1.0, rng.uniform(0, H - 1)), (rng.uniform(0, W - 1), 0.0), (rng.uniform(0, W - 1), H - 1.0),
                    (-1.0, -1.0), (W + 0.0, H + 0.0), (0.6, H - 1.4), (W - 1.3, 0.4)]
        assert len(centres) == 17
        amps = rng.uniform(0.3, 1.6, 17)
        amps[:3] = (1.6, 0.3, 1.3)
        a = quant(np.stack([blob(H, W, cx, cy, am) for (cx, cy), am in zip(centres, amps)]) + rng.normal(0, 0.02, (17, H, W)) - 0.01, 9)
        b = quant(a[FLIP17][..., ::-1] + rng.normal(0, 0.02, a.shape), 9)
        b = np.ascontiguousarray(b)
        assert a.min() < 0 and a.max() > 1
        input_size = (4 * W, 4 * H)
        codec = ref.UDPExpMaxHeatmap(input_size=input_size, heatmap_size=(W, H))
        name = f"expmax_{H}x{W}"
        names.append(name)
        pack(out, f"{name}.a", a, 9)
        pack(out, f"{name}.b", b, 9)
        out[f"{name}.input_size"] = np.array(input_size)
        variants = {"a": a, "b": b}
        for shift in (False, True):
            fb = ref.flip_heatmaps(torch.from_numpy(b.copy())[None], flip_mode="heatmap", flip_indices=FLIP17, shift_heatmap=shift)
            variants["shift" if shift else "plain"] = ((torch.from_numpy(a)[None] + fb) * 0.5).numpy()[0]
        for tag, maps in variants.items():
            kp, sc = codec.decode(maps.copy())
            assert kp.dtype == np.float64 and sc.dtype == np.float32 and kp.shape == (1, 17, 2)
            for backend in ("symmetric_f64", "scipy"):
                okp, osc = decode_ref.probmap_decode(maps.copy(), input_size=input_size, heatmap_size=(W, H), backend=backend)
                assert np.array_equal(okp.view(np.int64), kp.view(np.int64)) and np.array_equal(osc.view(np.int32), sc.view(np.int32)), \
                    f"oracle ({backend}) differs from the reference's UDPExpMaxHeatmap.decode on {name}.{tag}"
            n_kpts += 17
            out.update({f"{name}.{tag}.keypoints": kp, f"{name}.{tag}.scores": sc})
            if H * W <= 256:  # (the averaged maps of the small cases only)
                out[f"{name}.{tag}.maps"] = maps
    out["expmax.names"] = np.array(names)
    print(f"ExpMax: oracle == reference bit for bit on {n_kpts} of {n_kpts} keypoints, both backends")


def argmax_cases(ref, rng, out):
    """Sparsemax over the H*W logits of one blob (amplitude 2, 8 or 30, sigma 1 - 2.5, centre from -1 to W / H) + N(0, 0.3)."""
    names = []
    conds = []
    for (H, W, n, ks) in ((16, 12, 136, 11), (16, 16, 85, 11), (16, 12, 34, 17), (64, 48, 17, 11)):
        amp = rng.choice([2.0, 8.0, 30.0], n)
        z = np.stack([blob(H, W, rng.uniform(-1, W), rng.uniform(-1, H), am, rng.uniform(1.0, 2.5)) for am in amp]) + rng.normal(0, 0.3, (n, H, W))
        z = quant(z, 8)
        maps = sparsemax(z.reshape(n, -1)).reshape(n, H, W)
        input_size = (4 * W, 4 * H)
        codec = ref.ArgMaxProbMap(input_size=input_size, heatmap_size=(W, H), blur_kernel_size=ks)
        name = f"argmax_{H}x{W}_ks{ks}"
        names.append(name)
        kps, scs, locs = [], [], []
        for i in range(0, n, 17):
            kp, sc = codec.decode(maps[i:i + 17].copy())
            lc, _ = ref.utils.get_heatmap_maximum(maps[i:i + 17].copy())
            assert kp.dtype == np.float64 and sc.dtype == np.float32
            kps.append(kp[0]); scs.append(sc[0]); locs.append(lc)
            conds.append(R.decode_f64(maps[i:i + 17], ks, input_size)["cond"])
        pack(out, f"{name}.logits", z, 8)
        out.update({f"{name}.maps": maps, f"{name}.ks": np.int32(ks), f"{name}.input_size": np.array(input_size),
                    f"{name}.keypoints": np.stack(kps), f"{name}.scores": np.stack(scs), f"{name}.locs": np.stack(locs)})
    # the flip-test average of ProbMapHead.predict (probmap_head.py:757-763) on Sparsemax maps, with and without shift
    H, W = 16, 12
    za = quant(np.stack([[blob(H, W, rng.uniform(0, W - 1), rng.uniform(0, H - 1), 8.0, 1.5) for _ in range(17)] for _ in range(2)])
               + rng.normal(0, 0.3, (2, 17, H, W)), 8)
    zb = np.ascontiguousarray(quant(za[:, FLIP17][..., ::-1] + rng.normal(0, 0.3, za.shape), 8))
    a = sparsemax(za.reshape(2, 17, -1)).reshape(za.shape)
    b = sparsemax(zb.reshape(2, 17, -1)).reshape(zb.shape)
    codec = ref.ArgMaxProbMap(input_size=(48, 64), heatmap_size=(12, 16), blur_kernel_size=11)
    pack(out, "argmax_flip.logits_a", za, 8)
    pack(out, "argmax_flip.logits_b", zb, 8)
    out.update({"argmax_flip.a": a, "argmax_flip.b": b,
                "argmax_flip.ks": np.int32(11), "argmax_flip.input_size": np.array((48, 64))})
    for shift in (False, True):
        fb = ref.flip_heatmaps(torch.from_numpy(b.copy()), flip_mode="heatmap", flip_indices=FLIP17, shift_heatmap=shift)
        avg = ((torch.from_numpy(a) + fb) * 0.5).numpy()
        dec = [codec.decode(avg[i]) for i in range(2)]
        tag = "argmax_flip.shift" if shift else "argmax_flip.plain"
        out.update({f"{tag}.avg": avg, f"{tag}.keypoints": np.concatenate([d[0] for d in dec]), f"{tag}.scores": np.concatenate([d[1] for d in dec]),
                    f"{tag}.locs": np.stack([ref.utils.get_heatmap_maximum(avg[i].copy())[0] for i in range(2)])})
        conds += [R.decode_f64(avg[i], 11, (48, 64))["cond"] for i in range(2)]
    out["argmax.names"] = np.array(names)
    conds = np.concatenate(conds)
    good = float((conds < 100).mean())
    print(f"ArgMax: {conds.size} keypoints, {100 * good:.2f} % well-conditioned (cond < 100)")
    assert good >= 0.99, "the fixture's inputs must stay inside the 1 % cap for the reference alone"


def main():
    ref = load_reference()
    rng = np.random.default_rng(20261017)
    out = {"flip_indices": np.array(FLIP17)}
    out["defaults"] = np.array(json.dumps({"UDPExpMaxHeatmap": defaults_of(ref.UDPExpMaxHeatmap), "ArgMaxProbMap": defaults_of(ref.ArgMaxProbMap)}))
    expmax_cases(ref, rng, out)
    argmax_cases(ref, rng, out)
    path = os.path.join(HERE, "codec_swap_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
