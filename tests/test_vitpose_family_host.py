"""CPU: the host side of ViTPose-B / -L / -H - the ``huge`` arch in both arch tables, the three configs next to the ViTPose-S one,
their synthetic state dicts, the checked loader, the ``bbox_file`` refusal and the arch a ``synthetic`` checkpoint takes from a
config. No engine, no GPU."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCHS = {"base": (768, 12, 12, 3072), "large": (1024, 24, 16, 4096), "huge": (1280, 32, 16, 5120)}


def _cfg_path(arch):
    return os.path.join(ROOT, "configs", f"td-hm_ViTPose-{arch}_mi355x_coco-256x192.py")


def test_huge_is_in_both_arch_tables():
    from probpose_code_amd import pose_estimators, synthetic

    want = dict(embed_dims=1280, num_layers=32, num_heads=16, feedforward_channels=5120)
    assert pose_estimators._VIT_ARCHS["huge"] == want and pose_estimators._VIT_ARCHS["h"] == want
    assert synthetic.ARCHS["huge"] == want
    for name, (e, n, h, f) in ARCHS.items():  # the two tables agree on the ViTPose family
        want = dict(embed_dims=e, num_layers=n, num_heads=h, feedforward_channels=f)
        assert pose_estimators._VIT_ARCHS[name] == want and synthetic.ARCHS[name] == want, name


@pytest.mark.parametrize("arch", list(ARCHS))
def test_config_builds_and_matches_the_synthetic_state_dict(arch):
    import probpose_code_amd as pp
    from probpose_code_amd import apis, synthetic
    from probpose_code_amd.datasets import build_dataset

    E, L, H, Fd = ARCHS[arch]
    cfg = pp.Config.fromfile(_cfg_path(arch))
    assert cfg.model["backbone"]["arch"] == arch and cfg.model["head"]["in_channels"] == E and cfg.model["precision"] == "f16x3"
    assert synthetic.arch_of(cfg) == dict(embed_dims=E, num_layers=L, num_heads=H, feedforward_channels=Fd)
    assert synthetic.head_kind_of(cfg) == "heatmap"
    m = dict(cfg.model)
    m.pop("train_cfg", None)
    model = pp.build_pose_estimator(m)
    assert isinstance(model.head, pp.HeatmapHead) and isinstance(model.head.decoder, pp.UDPHeatmap)
    bb = model.backbone
    assert (bb.embed_dims, bb.num_layers, bb.num_heads, bb.ffn_dims) == (E, L, H, Fd) and bb.patch_resolution == (16, 12) and bb.patch_padding == 2
    assert model.test_cfg == dict(flip_test=True, flip_mode="heatmap", shift_heatmap=False)
    # parameter / buffer names and shapes == the synthetic state dict's
    sd = synthetic.synthetic_state_dict(arch, seed=0, logit_scale=2.0, head="heatmap")
    own = model.state_dict()
    assert set(own) == set(sd)
    for k, v in sd.items():
        assert tuple(own[k].shape) == tuple(v.shape), k
    assert sd["backbone.layers.0.attn.qkv.weight"].shape == (3 * E, E) and sd["head.deconv_layers.0.weight"].shape == (E, 256, 4, 4)
    assert f"backbone.layers.{L - 1}.ffn.layers.1.weight" in sd and f"backbone.layers.{L}.ln1.weight" not in sd
    apis.load_state_dict_checked(model, sd)
    short = dict(sd)
    short.pop(f"backbone.layers.{L - 1}.attn.proj.weight")
    with pytest.raises(Exception, match="proj"):
        apis.load_state_dict_checked(model, short)
    # ground-truth boxes; the reference config's detector boxes stay refused
    assert cfg.test_evaluator["type"] == "CocoMetric" and "bbox_file" not in cfg.test_dataloader.dataset
    with pytest.raises(NotImplementedError, match="bbox_file"):
        build_dataset(dict(cfg.test_dataloader.dataset, bbox_file="person_detection_results/COCO_val2017_detections_AP_H_56_person.json"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.engine


def test_trained_statistics_of_the_huge_state_dict():
    """stats="trained" re-parametrises per head dimension (q / k and v / proj rows of 16 heads of 80): same keys and shapes, other values."""
    import torch
    from probpose_code_amd import synthetic

    unit = synthetic.synthetic_state_dict("huge", seed=0, logit_scale=2.0, head="heatmap")
    trained = synthetic.synthetic_state_dict("huge", seed=0, logit_scale=2.0, head="heatmap", stats="trained")
    assert set(unit) == set(trained) and all(unit[k].shape == trained[k].shape for k in unit)
    assert not torch.equal(unit["backbone.layers.3.attn.qkv.weight"], trained["backbone.layers.3.attn.qkv.weight"])
    assert all(bool(torch.isfinite(v.float()).all()) for v in trained.values())


def test_synthetic_arch_of_the_existing_configs_is_unchanged():
    """``CHECKPOINT = synthetic`` takes the arch from the config: for the ViTPose-S / ProbPose-S configs that is the "small" table entry."""
    import probpose_code_amd as pp
    from probpose_code_amd import synthetic

    for name in ("td-hm_ViTPose-small_mi355x_coco-256x192.py", "td-pm_ProbPose-small_mi355x_coco-256x192.py"):
        assert synthetic.arch_of(pp.Config.fromfile(os.path.join(ROOT, "configs", name))) == synthetic.ARCHS["small"], name
    with pytest.raises(ValueError, match="default archs"):
        synthetic.arch_of(dict(model=dict(backbone=dict(arch="giant"))))
