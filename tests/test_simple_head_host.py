"""CPU: the host side of the ViTPose ``-simple`` variants - FeatureMapProcessor(scale_factor=4.0, apply_relu=True) in front of
HeatmapHead(deconv_out_channels=[], final_layer=dict(kernel_size=3, padding=1)): the four configs build, every other pairing is refused
by name, checkpoints load under the reference's key names, weights.pack recognises the head and packs its tap matrix, the synthetic
weights leave the other heads' tensors alone - and tests/simple_head_ref.py equals the REFERENCE's own classes (tests/golden/
simple_head.npz, written by tests/golden/make_golden_simple_head.py)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_head_ref as R  # noqa: E402

SIZES = {"small": 384, "base": 768, "large": 1024, "huge": 1280}
GOLDEN = os.path.join(ROOT, "tests", "golden", "simple_head.npz")


def _cfg(size):
    import probpose_code_amd as pp

    return pp.Config.fromfile(os.path.join(ROOT, "configs", f"td-hm_ViTPose-{size}-simple_mi355x_coco-256x192.py"))


def _model_cfg(size="small", **over):
    m = dict(_cfg(size).model)
    m.pop("train_cfg", None)
    m.update(over)
    return m


@pytest.mark.parametrize("size", list(SIZES))
def test_the_four_configs_build(size):
    import probpose_code_amd as pp
    from probpose_code_amd import synthetic as S

    cfg = _cfg(size)
    model = pp.build_pose_estimator(_model_cfg(size))
    assert isinstance(model.neck, pp.FeatureMapProcessor) and model.with_neck and model.with_head
    assert model.neck.scale_factor == 4.0 and model.neck.apply_relu and not list(model.neck.parameters())
    fl = model.head.final_layer
    assert isinstance(fl, torch.nn.Conv2d) and fl.kernel_size == (3, 3) and fl.padding == (1, 1) and fl.stride == (1, 1)
    assert (fl.in_channels, fl.out_channels) == (SIZES[size], 17) and model.head.upsampled_input == 4
    assert not any(k.startswith("head.deconv_layers.") for k in model.state_dict())
    assert S.head_kind_of(cfg) == "heatmap-simple"
    opts = model._engine_options()
    assert opts["head_kind"] == "heatmap" and opts["decode"] == "dark" and opts["neck_relu"] is True
    # the classic config of the same size keeps its head kind, and has no neck
    classic = pp.Config.fromfile(os.path.join(ROOT, "configs", f"td-hm_ViTPose-{size}_mi355x_coco-256x192.py"))
    assert S.head_kind_of(classic) == "heatmap"
    if size == "small":
        m = dict(classic.model)
        m.pop("train_cfg", None)
        assert not pp.build_pose_estimator(m).with_neck


def test_refusals_name_their_argument_and_the_pairing_that_runs():
    import probpose_code_amd as pp

    neck = dict(type="FeatureMapProcessor", scale_factor=4.0, apply_relu=True)
    for kw, name in ((dict(select_index=0), "select_index"), (dict(concat=True), "concat"), (dict(scale_factor=2.0), "scale_factor"),
                     (dict(scale_factor=1.0), "scale_factor"), (dict(align_corners=True), "align_corners")):
        with pytest.raises(NotImplementedError, match=name):
            pp.MODELS.build(dict(neck, **kw))
    assert pp.MODELS.build(dict(neck, apply_relu=False)).apply_relu is False  # runnable either way
    with pytest.raises(NotImplementedError, match="GlobalAveragePooling"):  # any other neck
        pp.build_pose_estimator(_model_cfg(neck=dict(type="GlobalAveragePooling")))
    simple_head = dict(_model_cfg()["head"])
    classic_head = dict(simple_head, deconv_out_channels=(256, 256), deconv_kernel_sizes=(4, 4), final_layer=dict(kernel_size=1))
    with pytest.raises(NotImplementedError, match="without a neck.*pairing that runs"):  # the no-deconv head under an estimator without the neck
        pp.build_pose_estimator(_model_cfg(neck=None))
    with pytest.raises(NotImplementedError, match="upsampled_input.*pairing that runs"):  # the estimator's keyword without the estimator's neck
        pp.build_pose_estimator(_model_cfg(neck=None, head=dict(simple_head, upsampled_input=4)))
    with pytest.raises(NotImplementedError, match="deconv_out_channels.*pairing that runs"):  # the neck in front of the classic head
        pp.build_pose_estimator(_model_cfg(head=classic_head))
    with pytest.raises(NotImplementedError, match="final_layer.*pairing that runs"):
        pp.build_pose_estimator(_model_cfg(head=dict(simple_head, final_layer=dict(kernel_size=1))))
    with pytest.raises(NotImplementedError, match="final_layer"):
        pp.build_pose_estimator(_model_cfg(head=dict(simple_head, final_layer=dict(kernel_size=3, padding=1, stride=2))))
    with pytest.raises(NotImplementedError, match="conv_out_channels"):
        pp.build_pose_estimator(_model_cfg(head=dict(simple_head, conv_out_channels=(64,), conv_kernel_sizes=(1,))))
    with pytest.raises(NotImplementedError, match="upsampled_input"):
        pp.MODELS.build(dict(simple_head, upsampled_input=2))
    probmap = dict(pp.Config.fromfile(os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")).model)["head"]
    with pytest.raises(NotImplementedError, match="ProbMapHead.*pairing that runs"):
        pp.build_pose_estimator(_model_cfg(head=dict(probmap)))
    # built on its own, without the estimator's keyword, the head is refused as before (pinned in tests/test_heatmap_head_host.py)
    with pytest.raises(NotImplementedError, match="deconv"):
        pp.MODELS.build(simple_head)
    for empty in (None, [], ()):
        assert pp.MODELS.build(dict(simple_head, deconv_out_channels=empty, deconv_kernel_sizes=empty, upsampled_input=4)).final_layer.kernel_size == (3, 3)


def test_checkpoint_keys_load_strictly_and_pack_recognises_the_head():
    import probpose_code_amd as pp
    from probpose_code_amd import synthetic as S
    from probpose_code_amd import weights

    model = pp.build_pose_estimator(_model_cfg())
    ref_keys = ["head." + k for k in np.load(GOLDEN)["state_keys"].tolist()]  # the reference head's own state_dict keys
    assert sorted(ref_keys) == sorted(k for k in model.state_dict() if k.startswith("head."))
    sd = S.synthetic_state_dict("small", seed=0, logit_scale=2.0, head="heatmap-simple")
    assert sorted(sd) == sorted(model.state_dict())
    model.load_state_dict(sd, strict=True)
    assert torch.equal(model.head.final_layer.weight, sd["head.final_layer.weight"])
    W = sd["head.final_layer.weight"]
    K, E = W.shape[:2]
    want = torch.stack([W[:, :, t // 3, t % 3] for t in range(9)]).reshape(9 * K, E)  # row t K + k, t = 3 (dy + 1) + (dx + 1)
    w32 = weights.pack(sd, torch.float32, "cpu", num_heads=12)
    assert w32.head_kind == "heatmap" and w32.deconv_channels == [] and w32.final_upsample == 4 and not w32.has("final.w")
    assert torch.equal(w32["final.taps"], want) and w32.inv("final.taps") == 1.0 and torch.equal(w32["final.b"], sd["head.final_layer.bias"])
    ws = weights.pack(sd, torch.float32, "cpu", split=True, num_heads=12)
    inv = ws.inv("final.taps")
    assert ws.final_upsample == 4 and np.log2(inv) == round(np.log2(inv)) and inv < 1  # a power-of-two scale, undone through w_inv_scale
    got = weights.from_split(ws["final.taps"]) * inv
    assert (got - want).abs().max() <= 2.0 ** -21 * want.abs().max()
    assert 2.0 ** 12 <= float(weights.from_split(ws["final.taps"]).abs().max()) < 2.0 ** 13
    assert weights.pack(sd, torch.bfloat16, "cpu", num_heads=12)["final.taps"].dtype == torch.bfloat16
    # the classic head is packed as before; a 3x3 final layer behind deconvolutions stays refused
    wc = weights.pack(S.synthetic_state_dict("small", seed=0, head="heatmap"), torch.float32, "cpu", num_heads=12)
    assert wc.final_upsample == 0 and wc.deconv_channels == [256, 256] and wc.has("final.w") and not wc.has("final.taps")
    mixed = S.synthetic_state_dict("small", seed=0, head="heatmap")
    mixed["head.final_layer.weight"] = torch.zeros(17, 256, 3, 3)
    with pytest.raises(NotImplementedError, match="3x3 final layer behind deconvolutions"):
        weights.pack(mixed, torch.float32, "cpu", num_heads=12)


def test_synthetic_simple_head_leaves_the_other_tensors_alone():
    from probpose_code_amd import synthetic as S

    simple = S.synthetic_state_dict("small", seed=3, logit_scale=2.0, head="heatmap-simple")
    classic = S.synthetic_state_dict("small", seed=3, logit_scale=2.0, head="heatmap")
    backbone = [k for k in classic if k.startswith("backbone.")]
    assert backbone and all(torch.equal(simple[k], classic[k]) for k in backbone)
    assert torch.equal(simple["head.final_layer.bias"], classic["head.final_layer.bias"])
    assert sorted(k for k in simple if k.startswith("head.")) == ["head.final_layer.bias", "head.final_layer.weight"]
    W = simple["head.final_layer.weight"]
    assert tuple(W.shape) == (17, 384, 3, 3)
    assert W.mean(dim=(1, 2, 3)).abs().max() < 1e-6 and abs(float(W.std()) / (2.0 / np.sqrt(9 * 384)) - 1) < 0.05
    with pytest.raises(ValueError, match="heatmap-simple"):
        S.synthetic_state_dict("small", head="simple")


def test_the_helper_equals_the_reference_classes_fixture():
    import probpose_code_amd as pp

    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 500_000
    assert dict(zip(g["state_keys"].tolist(), g["state_shapes"].tolist())) == {"final_layer.bias": "(17,)", "final_layer.weight": "(17, 64, 3, 3)"}
    W, b = torch.from_numpy(g["weight"].astype(np.float32)), torch.from_numpy(g["bias"].astype(np.float32))
    neck = pp.MODELS.build(dict(type="FeatureMapProcessor", scale_factor=4.0, apply_relu=True))
    for name, hw in (("small", (4, 3)), ("full", (16, 12))):
        x = torch.from_numpy(g[f"x_{name}"].astype(np.float32))
        want = g[f"y_{name}"]
        assert x.shape == (2, 64) + hw and want.shape == (2, 17, 4 * hw[0], 4 * hw[1]) and want.dtype == np.float32
        tol = 1e-6 * np.abs(want).max()
        got = R.reference_order(x, W, b).numpy()
        assert np.abs(got - want).max() <= tol, (name, np.abs(got - want).max() / np.abs(want).max())
        # FeatureMapProcessor.forward (for a caller of model.neck(x)): tuple in, list out; tensor in, tensor out
        up = neck((x,))
        assert isinstance(up, list) and len(up) == 1 and torch.equal(up[0], neck(x))
        got2 = torch.nn.functional.conv2d(up[0], W, b, padding=1).numpy()
        assert np.abs(got2 - want).max() <= tol
        # ... and the composed form, from fp32 taps, within its own bound plus the fixture's fp32 rounding
        out, S = R.composed(R.taps_of(x, W, torch.float64).astype(np.float32), b.numpy(), 17, hw[0], hw[1])
        assert np.abs(out - want).max() <= 1e-5 * np.abs(want).max()
