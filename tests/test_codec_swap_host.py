"""CPU: the host side of the codec swap - ``ArgMaxProbMap`` and ``UDPExpMaxHeatmap`` in the registry, their constructor defaults
against the reference's (recorded in tests/golden/codec_swap_cases.npz), their refusals, the ``decode`` a ``TopdownPoseEstimator``
hands its engine for each of the four head x codec pairs, and the fixture itself: the oracle reproduces its ExpMax half bit for bit,
and ``udp_ref.decode_f64`` judges at least 99 % of its ArgMax keypoints well-conditioned. No engine, no GPU."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_PM = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")
CFG_HM = os.path.join(ROOT, "configs", "td-hm_ViTPose-small_mi355x_coco-256x192.py")
SIZES = dict(input_size=(192, 256), heatmap_size=(48, 64))


def load_fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "codec_swap_cases.npz"))


def unpack(d, key):
    """A quantised input of the fixture (int16 steps) as the fp32 array it stands for."""
    return (d[key].astype(np.float64) / float(d[key + ".scale"])).astype(np.float32)


def test_registration_and_constructor_defaults(golden_dir):
    import probpose_code_amd as pp

    for name in ("ArgMaxProbMap", "ArgMaxProbMapMI355X"):
        assert pp.KEYPOINT_CODECS.get(name) is pp.ArgMaxProbMap, name
    for name in ("UDPExpMaxHeatmap", "UDPExpMaxHeatmapMI355X"):
        assert pp.KEYPOINT_CODECS.get(name) is pp.UDPExpMaxHeatmap, name
    recorded = json.loads(str(load_fixture(golden_dir)["defaults"]))
    for cls in (pp.ArgMaxProbMap, pp.UDPExpMaxHeatmap):
        sig = inspect.signature(cls.__init__)
        mine = {n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
        assert mine == recorded[cls.__name__], cls.__name__
        assert list(sig.parameters)[1:3] == ["input_size", "heatmap_size"]
    a = pp.KEYPOINT_CODECS.build(dict(type="ArgMaxProbMap", **SIZES))
    assert (a.sigma, a.blur_kernel_size, a.heatmap_type, a.increase_sigma_with_padding) == (-1, 11, "gaussian", False)
    e = pp.KEYPOINT_CODECS.build(dict(type="UDPExpMaxHeatmap", normalize=True, parzen_size=0.25, **SIZES))
    assert (e.sigma, e.blur_kernel_size, e.normalize, e.parzen_size) == (2.0, 11, True, 0.25)
    for c in (a, e):
        assert c.support_batch_decoding and tuple(c.heatmap_size) == (48, 64)
        assert np.array_equal(c.scale_factor, np.array([191 / 47, 255 / 63], np.float32))
    assert pp.ProbMap.decode_kind == "expmax" and pp.UDPExpMaxHeatmap.decode_kind == "expmax"
    assert pp.UDPHeatmap.decode_kind == "dark" and pp.ArgMaxProbMap.decode_kind == "dark"


@pytest.mark.parametrize("name", ["ArgMaxProbMap", "UDPExpMaxHeatmap"])
def test_refusals(name):
    import probpose_code_amd as pp

    cfg = dict(type=name, **SIZES)
    with pytest.raises(NotImplementedError, match="combined"):
        pp.KEYPOINT_CODECS.build(dict(cfg, heatmap_type="combined"))
    with pytest.raises(ValueError, match="heatmap_type"):
        pp.KEYPOINT_CODECS.build(dict(cfg, heatmap_type="offset"))
    codec = pp.KEYPOINT_CODECS.build(cfg)
    with pytest.raises(NotImplementedError, match="training"):
        codec.encode(np.zeros((1, 17, 2)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.decode_device(torch.zeros(1, 17, 64, 48))
    if name == "ArgMaxProbMap":  # the DARK blur's kernel size, validated like UDPHeatmap's
        for ks in (10, 21, 0):
            with pytest.raises(ValueError, match="blur_kernel_size"):
                pp.KEYPOINT_CODECS.build(dict(cfg, blur_kernel_size=ks))
        assert pp.KEYPOINT_CODECS.build(dict(cfg, blur_kernel_size=17)).blur_kernel_size == 17


@pytest.mark.parametrize("cfg,codec,head_kind,decode,ks", [
    (CFG_PM, None, "probmap", "expmax", 11), (CFG_PM, "ArgMaxProbMap", "probmap", "dark", 17),
    (CFG_HM, None, "heatmap", "dark", 17), (CFG_HM, "UDPExpMaxHeatmap", "heatmap", "expmax", 11)])
def test_estimator_hands_the_engine_its_codecs_decode(cfg, codec, head_kind, decode, ks):
    """(blur_kernel_size 17 on the codec: it reaches the engine for a DARK decode and stays 11 - unused - otherwise)"""
    import probpose_code_amd as pp

    c = pp.Config.fromfile(cfg)
    opts = {"model.head.decoder.blur_kernel_size": 17}
    if codec is not None:
        opts["model.head.decoder.type"] = codec
    c.merge_from_dict(opts)
    m = dict(c.model)
    m.pop("train_cfg", None)
    model = pp.build_pose_estimator(m)
    assert type(model.head.decoder).__name__ == (codec or ("ProbMap" if head_kind == "probmap" else "UDPHeatmap"))
    o = model._engine_options()
    assert (o["head_kind"], o["decode"], o["blur_kernel_size"]) == (head_kind, decode, ks)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.engine


def test_abi_argument_checks_without_gpu(lib_built):
    """Refusals that need no device: unknown flags, K > 17 on the ExpMax path, an even blur kernel, a map too large for LDS."""
    from probpose_code_amd import _lib

    L = _lib.lib
    assert L.pp_expmax_heatmap_decode(None, None, None, None, None, 1, 17, 64, 48, 192.0, 256.0, None, None, None, None, None, 1, None) == _lib.PP_ERR_INVALID_ARG
    assert b"unknown flag" in L.pp_last_error()
    assert L.pp_expmax_heatmap_decode(None, None, None, None, None, 1, 18, 64, 48, 192.0, 256.0, None, None, None, None, None, 0, None) == _lib.PP_ERR_UNSUPPORTED
    assert b"17 sigmas" in L.pp_last_error()
    assert L.pp_expmax_heatmap_decode(None, None, None, None, None, 1, 17, 64, 48, 192.0, 256.0, None, None, None, None, None, 0, None) == _lib.PP_ERR_INVALID_ARG
    assert b"non-NULL" in L.pp_last_error()

    def argmax(H=64, W=48, T=0.5, ks=11, flags=0):
        return L.pp_argmax_probmap_decode(None, None, None, 1, 17, H, W, 192.0, 256.0, T, 1.0, ks, None, None, None, None, flags, None)

    assert argmax(flags=1) == _lib.PP_ERR_INVALID_ARG and b"unknown flag" in L.pp_last_error()  # (PP_DECODE_LOGITS is implied, not a flag here)
    assert argmax(flags=8) == _lib.PP_ERR_INVALID_ARG and b"unknown flag" in L.pp_last_error()
    assert argmax(ks=10) == _lib.PP_ERR_INVALID_ARG and b"odd" in L.pp_last_error()
    assert argmax(ks=21) == _lib.PP_ERR_UNSUPPORTED and b"above 19" in L.pp_last_error()
    assert argmax(T=0.0) == _lib.PP_ERR_INVALID_ARG and b"temperature" in L.pp_last_error()
    assert argmax(W=50) == _lib.PP_ERR_UNSUPPORTED and b"multiple of 4" in L.pp_last_error()
    assert argmax(H=63, flags=2) == _lib.PP_ERR_UNSUPPORTED and b"PP_DECODE_PHASED" in L.pp_last_error()
    assert argmax(H=3072, W=4) == _lib.PP_ERR_UNSUPPORTED and b"LDS" in L.pp_last_error()  # 12 288 pixels, but 3072 x (4 + 24) padded floats: 336 KiB
    assert argmax(H=128, W=100) == _lib.PP_ERR_UNSUPPORTED and b"12288" in L.pp_last_error()
    assert argmax() == _lib.PP_ERR_INVALID_ARG and b"non-NULL" in L.pp_last_error()  # every shape check passed


def test_oracle_reproduces_the_expmax_fixture_bit_for_bit(golden_dir):
    from oracle import decode_ref

    d = load_fixture(golden_dir)
    fi = [int(i) for i in d["flip_indices"]]
    n = 0
    for name in d["expmax.names"]:
        a, b = unpack(d, f"{name}.a"), unpack(d, f"{name}.b")
        K, H, W = a.shape
        assert K == 17 and a.min() < 0 and a.max() > 1, "the input class holds negatives and values above 1"
        size = tuple(int(v) for v in d[f"{name}.input_size"])
        variants = dict(a=a, b=b, plain=decode_ref.tta_average(a[None], b[None], fi)[0], shift=decode_ref.tta_average(a[None], b[None], fi, True)[0])
        for tag, maps in variants.items():
            if f"{name}.{tag}.maps" in d.files:  # the reference's own flip_heatmaps average
                assert np.array_equal(maps.view(np.int32), d[f"{name}.{tag}.maps"].view(np.int32)), (name, tag)
            for backend in ("symmetric_f64", "scipy"):
                kp, sc = decode_ref.probmap_decode(maps, input_size=size, heatmap_size=(W, H), backend=backend)
                assert np.array_equal(kp.view(np.int64), d[f"{name}.{tag}.keypoints"].view(np.int64)), (name, tag, backend)
                assert np.array_equal(sc.view(np.int32), d[f"{name}.{tag}.scores"].view(np.int32)), (name, tag, backend)
            n += K
    assert n == 272


def test_argmax_fixture_is_well_conditioned(golden_dir):
    """At most 1 % of the ArgMax fixture's keypoints are ill-conditioned (cond >= 100) for the fp64 form alone - the GPU test's cap on
    left-out keypoints has room for the fixture's inputs. Also: the maps are the Sparsemax of the stored logits."""
    import udp_ref as R

    d = load_fixture(golden_dir)
    conds = []
    for name in d["argmax.names"]:
        maps, z = d[f"{name}.maps"], unpack(d, f"{name}.logits")
        assert maps.shape == z.shape and maps.min() >= 0 and np.allclose(maps.reshape(len(maps), -1).sum(1), 1, atol=1e-5)
        assert ((maps > 0) <= (z > z.reshape(len(z), -1).max(1)[:, None, None] - 1)).all()  # support within one unit of the maximum
        size = tuple(int(v) for v in d[f"{name}.input_size"])
        for i in range(0, len(maps), 17):
            conds.append(R.decode_f64(maps[i:i + 17], int(d[f"{name}.ks"]), size)["cond"])
    for tag in ("plain", "shift"):
        conds += [R.decode_f64(m, 11, (48, 64))["cond"] for m in d[f"argmax_flip.{tag}.avg"]]
    conds = np.concatenate(conds)
    good = float((conds < 100).mean())
    print(f"{conds.size} keypoints, {100 * good:.2f} % with cond < 100")
    assert conds.size >= 200 and good >= 0.99
