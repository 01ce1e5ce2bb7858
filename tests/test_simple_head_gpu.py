"""GPU: the ViTPose ``-simple`` variants - csrc/pp_simple_head.hip alone and the small-simple config end to end.

pp_relu_operand: bit for bit the helper's rule (tests/simple_head_ref.py) in the three operand formats, with canaries around the output.
pp_taps_upsample4_conv3x3: against the formula in fp64 under ``41 * 2^-24 * S`` (the bound and the faults it rejects:
tests/test_simple_head_references.py) on random taps, corner impulses and constant planes.
End to end (f16x3, ``calibrated_state_dict(0)``): the heatmaps against the reference's order of operations in fp32 on
oracle.model_ref.vit_forward features, under the project's bar ``1e-3 * max(1, max |ref|)``; keypoints, maxima and scores against the fp64
decode (tests/udp_ref.py) of THE MAPS THE GPU RETURNED under that decode's bound, keypoints whose fp64 Hessian has condition number >= 100
left out of the coordinate comparison only (the share the reference's own maps leave out: tests/test_simple_head_references.py).
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_head_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0x7FA5A5A5  # a NaN pattern no kernel writes
FMT = {"f32": 0, "bf16": 1, "split": 2}  # PP_OUT_*


def _cfg(size="small"):
    return os.path.join(ROOT, "configs", f"td-hm_ViTPose-{size}-simple_mi355x_coco-256x192.py")


def _model(flip=True, sd=None, size="small", **opts):
    from probpose_code_amd import apis

    o = {"model.test_cfg.flip_test": flip}
    o.update(opts)
    return apis.init_model(_cfg(size), dict(state_dict=R.calibrated_state_dict(0) if sd is None else sd), device="cuda:0", cfg_options=o)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n_words):
    """int32 buffer of n_words behind and in front of 64 canary words (16-byte aligned payload)."""
    buf = torch.full((n_words + 128,), CANARY, dtype=torch.int32, device="cuda")
    return buf, buf[64:64 + n_words]


def _canaries_intact(buf, n_words):
    return bool((buf[:64] == CANARY).all()) and bool((buf[64 + n_words:] == CANARY).all())


# ------------------------------------------------------------------------------------------------------------ pp_relu_operand
def _relu_input(fmt, n_rows, row_len, rng):
    """Bit patterns of n_rows x row_len elements: random values of either sign, +-0, tiny negatives whose hi half is zero, NaN, +-Inf."""
    n = n_rows * row_len
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -1e-9, 1e-9, -6e-8, 6e-8, -65504.0, 65504.0], np.float32)
    pos = rng.permutation(n)[: min(n, 4 * special.size)]
    x[pos] = np.resize(special, pos.size)
    if fmt == "f32":
        return x.view(np.uint32).copy()
    if fmt == "bf16":
        return (x.view(np.uint32) >> 16).astype(np.uint16)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    # tiny negatives whose hi half is ZERO (either sign) and whose lo half alone carries the value; and a pair that cancels exactly
    hi_u, lo_u = hi.view(np.uint16).copy(), lo.view(np.uint16).copy()
    for j, (h, l) in enumerate(((0x0000, 0x8001), (0x8000, 0x8001), (0x0000, 0x0001), (0x8000, 0x0001), (0x3C00, 0xBC00), (0x7C00, 0xFC00))):
        hi_u[(7 * j + 3) % n], lo_u[(7 * j + 3) % n] = h, l
    blocks = np.stack([hi_u.reshape(-1, 32), lo_u.reshape(-1, 32)], axis=1)  # (n / 32, 2, 32): 32 hi halves then 32 lo halves
    return blocks.reshape(-1).copy()


@pytest.mark.parametrize("n_rows", [1, 385])
@pytest.mark.parametrize("row_len", [32, 64, 384])
@pytest.mark.parametrize("fmt", ["f32", "bf16", "split"])
def test_relu_operand_is_bit_exact(fmt, row_len, n_rows):
    from probpose_code_amd import _lib

    rng = np.random.default_rng(row_len + n_rows)
    bits = _relu_input(fmt, n_rows, row_len, rng)
    want = {"f32": R.relu_f32_bits, "bf16": R.relu_bf16_bits, "split": R.relu_split_bits}[fmt](bits)
    words = torch.from_numpy(bits.view(np.int32).copy()).cuda()
    keep = words.clone()
    buf, out = _guarded(words.numel())
    _lib.reset_launch_counts()
    _lib.call("pp_relu_operand", FMT[fmt], words.data_ptr(), out.data_ptr(), n_rows, row_len, _stream())
    torch.cuda.synchronize()
    assert _lib.launch_count("pp_simple_head.hip") == 1
    got = out.cpu().numpy().view(bits.dtype)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} elements differ"
    assert _canaries_intact(buf, words.numel()) and torch.equal(words, keep)
    changed = int((want != bits).sum())
    assert 0 < changed < bits.size  # (the input has elements of either kind)


def test_relu_operand_refusals():
    from probpose_code_amd import _lib

    x = torch.zeros(64, dtype=torch.float32, device="cuda")
    y = torch.full((64,), 7.0, device="cuda")
    L, st = _lib.lib, _stream()
    _lib.reset_launch_counts()
    assert L.pp_relu_operand(3, x.data_ptr(), y.data_ptr(), 1, 32, st) == _lib.PP_ERR_INVALID_ARG
    assert L.pp_relu_operand(0, None, y.data_ptr(), 1, 32, st) == _lib.PP_ERR_INVALID_ARG
    assert L.pp_relu_operand(0, x.data_ptr(), None, 1, 32, st) == _lib.PP_ERR_INVALID_ARG
    assert L.pp_relu_operand(0, x.data_ptr(), y.data_ptr(), -1, 32, st) == _lib.PP_ERR_INVALID_ARG
    assert L.pp_relu_operand(0, x.data_ptr(), y.data_ptr(), 1, 0, st) == _lib.PP_ERR_INVALID_ARG
    assert L.pp_relu_operand(2, x.data_ptr(), y.data_ptr(), 1, 48, st) == _lib.PP_ERR_UNSUPPORTED
    assert L.pp_relu_operand(0, None, None, 0, 32, st) == _lib.PP_OK  # no rows: returns at once
    torch.cuda.synchronize()
    assert _lib.launch_count("pp_simple_head.hip") == 0 and bool((y == 7.0).all())


# ------------------------------------------------------------------------------------------------------------ pp_taps_upsample4_conv3x3
@pytest.mark.parametrize("shape", R.GATHER_SHAPES)
def test_taps_upsample4_conv3x3_against_the_fp64_formula(shape):
    from probpose_code_amd import _lib

    n, K, h, w = shape
    n_out = n * K * 16 * h * w
    for name, taps, bias in R.gather_inputs(*shape):
        ref, S = R.composed(taps, bias, K, h, w, np.float64)
        t = torch.from_numpy(taps).cuda()
        keep = t.clone()
        b = torch.from_numpy(bias).cuda()
        buf, out = _guarded(n_out)
        _lib.reset_launch_counts()
        _lib.call("pp_taps_upsample4_conv3x3", t.data_ptr(), b.data_ptr(), out.data_ptr(), n, K, h, w, _stream())
        torch.cuda.synchronize()
        assert _lib.launch_count("pp_simple_head.hip") == 1
        assert not bool((out == CANARY).any()), f"{shape} {name}: an output element was not written"
        got = out.view(torch.float32).cpu().numpy().reshape(n, K, 4 * h, 4 * w)
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= R.BOUND * S).all(), f"{shape} {name}: off by {(err / np.maximum(S, 1e-300)).max() / 2.0 ** -24:.2f} x 2^-24 S (bound 41)"
        if name == "constant":
            assert set(np.unique(got).tolist()) <= {4.0, 6.0, 9.0} and got[0, 0, 0, 0] == 4 and got[0, 0, 1, 1] == 9
        assert _canaries_intact(buf, n_out) and torch.equal(t, keep)
        # a second launch is bit-identical; so is one into a buffer that is only 4-byte aligned (scalar stores)
        buf2, out2 = _guarded(n_out + 1)
        _lib.call("pp_taps_upsample4_conv3x3", t.data_ptr(), b.data_ptr(), out.data_ptr(), n, K, h, w, _stream())
        _lib.call("pp_taps_upsample4_conv3x3", t.data_ptr(), b.data_ptr(), out2[1:].data_ptr(), n, K, h, w, _stream())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), got.view(np.int32).reshape(-1)) and torch.equal(out2[1:], out)
        assert int(out2[0]) == CANARY and _canaries_intact(buf2, n_out + 1)


def test_taps_upsample4_conv3x3_refusals_and_nan_containment():
    from probpose_code_amd import _lib

    L, st = _lib.lib, _stream()
    t = torch.zeros(9 * 4, dtype=torch.float32, device="cuda")
    b = torch.zeros(1, dtype=torch.float32, device="cuda")
    o = torch.full((64,), 7.0, device="cuda")
    _lib.reset_launch_counts()
    for args in ((None, b.data_ptr(), o.data_ptr(), 1, 1, 2, 2), (t.data_ptr(), None, o.data_ptr(), 1, 1, 2, 2), (t.data_ptr(), b.data_ptr(), None, 1, 1, 2, 2),
                 (t.data_ptr(), b.data_ptr(), o.data_ptr(), -1, 1, 2, 2), (t.data_ptr(), b.data_ptr(), o.data_ptr(), 1, 0, 2, 2),
                 (t.data_ptr(), b.data_ptr(), o.data_ptr(), 1, 1, 0, 2), (t.data_ptr(), b.data_ptr(), o.data_ptr(), 1, 1, 2, -3)):
        assert L.pp_taps_upsample4_conv3x3(*args, st) == _lib.PP_ERR_INVALID_ARG, args
    assert L.pp_taps_upsample4_conv3x3(t.data_ptr(), b.data_ptr(), o.data_ptr(), 1, 1, 1 << 21, 1, st) == _lib.PP_ERR_UNSUPPORTED
    assert L.pp_taps_upsample4_conv3x3(None, None, None, 0, 17, 16, 12, st) == _lib.PP_OK  # empty batch: returns at once
    torch.cuda.synchronize()
    assert _lib.launch_count("pp_simple_head.hip") == 0 and bool((o == 7.0).all())
    # out-of-map taps are left out by selection: a NaN at a corner sample reaches exactly the outputs whose in-map taps sample it
    h, w, K = 3, 5, 2
    taps = np.ones((1, 9 * K, h * w), np.float32)
    taps[0, 4 * K + 1, 0] = np.nan  # centre tap of keypoint 1, sample (0, 0)
    ref, _ = R.composed(taps, np.zeros(K, np.float32), K, h, w)
    out = torch.empty(K * 16 * h * w, dtype=torch.float32, device="cuda")
    _lib.call("pp_taps_upsample4_conv3x3", torch.from_numpy(taps).cuda().data_ptr(), torch.zeros(K, device="cuda").data_ptr(), out.data_ptr(), 1, K, h, w, st)
    got = out.cpu().numpy().reshape(1, K, 4 * h, 4 * w)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got[0, 1]).any() and not np.isnan(got[0, 0]).any()


# ------------------------------------------------------------------------------------------------------------ end to end
def _check_against_references(eng, out, sd, crops, B, flip, coord_check=True):
    import udp_ref as U

    hm = out["heatmaps"].cpu().numpy()
    kp, sc, locs = out["keypoints"].cpu().numpy(), out["scores"].cpu().numpy(), out["locs"].cpu().numpy()
    ref = R.reference_heatmaps(sd, crops, flip, eng.heads)
    bar = 1e-3 * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(hm - ref).max())
    print(f"B {B} flip {flip} {eng.precision}: heatmaps L_inf {err:.3e} (bar {bar:.3e}, largest |value| {np.abs(ref).max():.2f})")
    assert err <= bar, f"heatmaps off by {err:.3e} (bar {bar:.3e})"
    if not coord_check:
        return
    assert (ref.reshape(B, 17, -1).max(-1) > 0).all(), "a synthetic map without a positive maximum"
    ref_out = int(sum((~(U.decode_f64(m, 11, (192, 256))["cond"] < 100)).sum() for m in ref))
    assert ref_out <= max(1, int(0.05 * B * 17)), f"the reference's own maps leave out {ref_out} of {B * 17} keypoints"
    scale = np.array([192 / 47, 256 / 63])
    n_out = 0
    for b in range(B):
        d = U.decode_f64(hm[b], 11, (192, 256))
        assert np.array_equal(locs[b], d["locs"]) and np.array_equal(sc[b], d["scores"]), b
        ok = d["cond"] < 100
        n_out += int((~ok).sum())
        e = (np.abs(kp[b] - d["keypoints"]) / scale).max(1)
        assert (e[ok] <= d["bound"][ok]).all(), (b, e[ok].max(), d["bound"][ok])
    print(f"    left out of the coordinate comparison: {n_out} of {B * 17} on the GPU's maps, {ref_out} on the reference's")
    assert n_out <= ref_out + 2


@pytest.mark.parametrize("B,flip", [(1, True), (1, False), (8, True), (8, False), (20, True)])
def test_heatmaps_against_the_reference_order_and_keypoints_against_the_fp64_decode(B, flip):
    from probpose_code_amd import _lib
    from probpose_code_amd import synthetic as S

    sd = R.calibrated_state_dict(0)
    model = _model(flip)
    eng = model.engine
    assert eng.head_kind == "heatmap" and eng.simple_head and (eng.Hh, eng.Wh) == (64, 48) and not eng.tower_hw
    assert (B * (2 if flip else 1) * eng.Np >= eng.small_rows_below) == (B == 20)  # B 20 with flip: 7 680 token rows, beyond the small-batch plan
    crops = S.synthetic_crops(B, seed=100)
    eng.forward(crops.cuda(), flip, S.COCO_FLIP_INDICES, return_heatmaps=True)  # (kernel attributes set before the launches are counted)
    _lib.reset_launch_counts()
    out = eng.forward(crops.cuda(), flip, S.COCO_FLIP_INDICES, return_heatmaps=True)
    torch.cuda.synchronize()
    assert _lib.launch_count("pp_simple_head.hip") == 2 and _lib.launch_count("pp_udp_decode.hip") == 1 and _lib.launch_count("pp_decode.hip") == 0
    for other in ("pp_panel_split.hip", "skinny_deconv", "skinny_conv1x1", "pp_winograd.hip", "pp_conv_halo.hip", "pp_head.hip"):
        assert _lib.launch_count(other) == 0, f"{other} launched for the -simple head"
    assert not eng._logits_phased
    _check_against_references(eng, out, sd, crops, B, flip)


def test_fp32_meets_the_bar_and_bf16_runs():
    from probpose_code_amd import synthetic as S

    sd = R.calibrated_state_dict(0)
    crops = S.synthetic_crops(1, seed=100)
    m32 = _model(True, **{"model.precision": "f32"})
    out = m32.engine.forward(crops.cuda(), True, S.COCO_FLIP_INDICES, return_heatmaps=True)
    torch.cuda.synchronize()
    _check_against_references(m32.engine, out, sd, crops, 1, True)
    mbf = _model(True, **{"model.precision": "bf16"})
    out = mbf.engine.forward(crops.cuda(), True, S.COCO_FLIP_INDICES, return_heatmaps=True)
    torch.cuda.synchronize()
    hm = out["heatmaps"].cpu().numpy()
    assert np.isfinite(hm).all() and bool(torch.isfinite(out["keypoints"]).all()) and bool(torch.isfinite(out["scores"]).all())
    ref = R.reference_heatmaps(sd, crops, True)
    print(f"bf16 B 1 flip: heatmaps L_inf {np.abs(hm - ref).max():.3e} (largest |value| {np.abs(ref).max():.2f}) - printed, not asserted")


def test_apply_relu_false_leaves_the_relu_launch_out():
    from probpose_code_amd import _lib
    from probpose_code_amd import synthetic as S

    sd = R.calibrated_state_dict(0)
    model = _model(False, **{"model.neck.apply_relu": False})
    eng = model.engine
    crops = S.synthetic_crops(2, seed=100)
    eng.forward(crops.cuda(), False, None, return_heatmaps=True)
    _lib.reset_launch_counts()
    out = eng.forward(crops.cuda(), False, None, return_heatmaps=True)
    torch.cuda.synchronize()
    assert _lib.launch_count("pp_simple_head.hip") == 1
    with torch.no_grad():
        ref = R.reference_order(R.features(sd, crops), sd["head.final_layer.weight"], sd["head.final_layer.bias"], apply_relu=False).numpy()
    bar = 1e-3 * max(1.0, float(np.abs(ref).max()))
    assert np.abs(out["heatmaps"].cpu().numpy() - ref).max() <= bar


def test_graph_replay_stream_full_image_codec_swap_and_output_heatmaps():
    from probpose_code_amd import _lib, apis
    from probpose_code_amd import synthetic as S

    model = _model(True)
    eng = model.engine
    crops = S.synthetic_crops(8, seed=7).cuda()
    plain = {k: v.clone() for k, v in eng.forward(crops, True, S.COCO_FLIP_INDICES, return_heatmaps=True).items() if v is not None}
    graph = eng.forward_graph(crops, True, S.COCO_FLIP_INDICES, return_heatmaps=True)
    torch.cuda.synchronize()
    for k in ("keypoints", "scores", "locs", "heatmaps"):
        assert torch.equal(plain[k], graph[k]), k
    assert torch.count_nonzero(graph["scalars"]) == 0
    # test_step_stream == test_step (batches of different sizes)
    rng = np.random.default_rng(3)
    batches = []
    for n, seed in ((8, 1), (3, 2), (8, 3)):
        c = S.synthetic_crops(n, seed=seed)
        center = np.stack([rng.uniform(80, 400, n), rng.uniform(100, 500, n)], -1).astype(np.float32)
        scale = (np.array([192, 256], np.float32) * rng.uniform(0.8, 2.5, (n, 1)).astype(np.float32) * 1.25).astype(np.float32)
        batches.append((c, center, scale))
    steps = [model.test_step(apis.pack_crops(c, ce, s, model.dataset_meta)) for c, ce, s in batches]
    streamed = list(model.test_step_stream([apis.pack_crops(c, ce, s, model.dataset_meta) for c, ce, s in batches], depth=2, max_batch=8))
    for a, b in zip(steps, streamed):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            for f in ("keypoints", "keypoint_scores", "keypoints_visible", "bboxes"):
                assert np.array_equal(getattr(x.pred_instances, f), getattr(y.pred_instances, f)), f
            assert "keypoints_probs" not in x.pred_instances
    # inference_topdown on the full image == the crops it cuts, through pack_crops
    img_path = os.path.join(ROOT, "demo", "resources", "synthetic_person.png")
    bb = np.array([[40, 30, 200, 400], [100, 60, 300, 420]], np.float32)
    res = apis.inference_topdown(model, img_path, bb)
    batch = apis._frame_batch(model, img_path, bb, "xyxy")
    crops2 = torch.stack(list(batch["inputs"]))
    center = np.stack([np.asarray(s.metainfo["input_center"]) for s in batch["data_samples"]])
    scale = np.stack([np.asarray(s.metainfo["input_scale"]) for s in batch["data_samples"]])
    res2 = model.test_step(apis.pack_crops(crops2, center, scale, model.dataset_meta))
    assert len(res) == len(res2) == 2
    for x, y in zip(res, res2):
        assert np.array_equal(x.pred_instances.keypoints, y.pred_instances.keypoints)
        assert np.array_equal(x.pred_instances.keypoint_scores, y.pred_instances.keypoint_scores)
    # extract_feat keeps returning the backbone's maps; _forward gives the (B, K, 64, 48) maps
    x = crops[:2]
    feats = model.extract_feat(x)
    assert tuple(feats[0].shape) == (2, 384, 16, 12)
    assert tuple(model._forward(x).shape) == (2, 17, 64, 48)
    # output_heatmaps through test_step
    m2 = _model(True, **{"model.test_cfg.output_heatmaps": True})
    r = m2.test_step(apis.pack_crops(batches[1][0], batches[1][1], batches[1][2], m2.dataset_meta))
    assert tuple(r[0].pred_fields.heatmaps.shape) == (17, 64, 48)
    # the swapped codec: the expected-OKS decode on the same logits
    m3 = _model(True, **{"model.head.decoder.type": "UDPExpMaxHeatmap"})
    e3 = m3.engine
    e3.forward(crops, True, S.COCO_FLIP_INDICES, return_heatmaps=True)
    _lib.reset_launch_counts()
    o3 = e3.forward(crops, True, S.COCO_FLIP_INDICES, return_heatmaps=True)
    torch.cuda.synchronize()
    assert _lib.launch_count("pp_expmax_heatmap_decode") == 1 and _lib.launch_count("pp_udp_decode.hip") == 0 and _lib.launch_count("pp_simple_head.hip") == 2
    assert torch.equal(o3["heatmaps"], plain["heatmaps"]) and bool(torch.isfinite(o3["keypoints"]).all())


def test_a_poisoned_crop_is_reported_and_leaves_the_others_alone():
    from probpose_code_amd import synthetic as S

    model = _model(False)
    eng = model.engine
    crops = S.synthetic_crops(4, seed=11).cuda()
    feat32 = eng.export_features(eng.run_backbone(crops, False))  # (4, 16, 12, 384) fp32, the caller's copy
    clean = {k: v.clone() for k, v in eng.run_head(eng.import_features(feat32), False, None, return_heatmaps=True).items()}
    model.head.pack_predictions(clean, {})  # finite: no error
    bad = feat32.clone()
    bad[2, 5, 7, 100] = float("nan")
    out = eng.run_head(eng.import_features(bad), False, None, return_heatmaps=True)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(out["keypoints"][2]).any()) and not bool(torch.isfinite(out["scores"][2]).any())
    with pytest.raises(FloatingPointError, match=r"crop\(s\) \[2\]"):
        model.head.pack_predictions(out, {})
    for b in (0, 1, 3):
        for k in ("keypoints", "scores", "locs", "heatmaps"):
            assert torch.equal(out[k][b], clean[k][b]), (b, k)


@pytest.mark.parametrize("size", ["base", "huge"])
def test_larger_archs_meet_the_heatmap_bar(size):
    from probpose_code_amd import synthetic as S

    sd = S.synthetic_state_dict(size, seed=0, logit_scale=2.0, head="heatmap-simple")
    model = _model(True, sd=sd, size=size)
    eng = model.engine
    assert eng.simple_head and eng.E == {"base": 768, "huge": 1280}[size]
    crops = S.synthetic_crops(1, seed=100)
    out = eng.forward(crops.cuda(), True, S.COCO_FLIP_INDICES, return_heatmaps=True)
    torch.cuda.synchronize()
    _check_against_references(eng, out, sd, crops, 1, True, coord_check=False)
