"""CPU: the host side of the ViTPose baseline - ``HeatmapHead``, the ``UDPHeatmap`` codec, the config, the synthetic state dict of
a head without towers, the C ABI's argument checks for ``pp_udp_heatmap_decode`` and ``CocoMetric`` on samples that carry no
presence probabilities. No engine, no GPU."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "td-hm_ViTPose-small_mi355x_coco-256x192.py")
HEAD = dict(type="HeatmapHead", in_channels=384, out_channels=17, deconv_out_channels=(256, 256), deconv_kernel_sizes=(4, 4),
            loss=dict(type="KeypointMSELoss", use_target_weight=True),
            decoder=dict(type="UDPHeatmap", input_size=(192, 256), heatmap_size=(48, 64), sigma=2))


def test_registry_names():
    import probpose_code_amd as pp

    for name in ("HeatmapHead", "HeatmapHeadMI355X", "mmpose.HeatmapHead"):
        assert pp.MODELS.get(name) is pp.HeatmapHead, name
    for name in ("UDPHeatmap", "UDPHeatmapMI355X"):
        assert pp.KEYPOINT_CODECS.get(name) is pp.UDPHeatmap, name
    codec = pp.KEYPOINT_CODECS.build(HEAD["decoder"])
    assert codec.blur_kernel_size == 11 and codec.support_batch_decoding and tuple(codec.heatmap_size) == (48, 64)
    assert np.array_equal(codec.scale_factor, np.array([191 / 47, 255 / 63], np.float32))


def test_codec_refusals():
    import probpose_code_amd as pp

    with pytest.raises(NotImplementedError, match="combined"):
        pp.KEYPOINT_CODECS.build(dict(HEAD["decoder"], heatmap_type="combined"))
    with pytest.raises(ValueError, match="heatmap_type"):
        pp.KEYPOINT_CODECS.build(dict(HEAD["decoder"], heatmap_type="offset"))
    with pytest.raises(ValueError, match="blur_kernel_size"):
        pp.KEYPOINT_CODECS.build(dict(HEAD["decoder"], blur_kernel_size=10))
    with pytest.raises(ValueError, match="blur_kernel_size"):
        pp.KEYPOINT_CODECS.build(dict(HEAD["decoder"], blur_kernel_size=21))
    codec = pp.KEYPOINT_CODECS.build(HEAD["decoder"])
    with pytest.raises(NotImplementedError, match="training"):
        codec.encode(np.zeros((1, 17, 2)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.decode_device(torch.zeros(1, 17, 64, 48))


def test_head_refusals():
    import probpose_code_amd as pp

    def build(**kw):
        return pp.MODELS.build(dict(HEAD, **kw))

    for ks in (3, 2):
        with pytest.raises(NotImplementedError, match="kernel 4"):
            build(deconv_kernel_sizes=(4, ks))
    with pytest.raises(ValueError, match="Unsupported kernel size"):
        build(deconv_kernel_sizes=(4, 5))
    with pytest.raises(ValueError, match="same length"):
        build(deconv_kernel_sizes=(4,))
    with pytest.raises(NotImplementedError, match="conv_out_channels"):
        build(conv_out_channels=(256,), conv_kernel_sizes=(1,))
    with pytest.raises(NotImplementedError, match="1x1"):  # the '-simple' ViTPose heads: no deconvolution, a 3x3 final layer
        build(final_layer=dict(kernel_size=3, padding=1))
    with pytest.raises(NotImplementedError, match="deconv"):
        build(deconv_out_channels=None, deconv_kernel_sizes=None, final_layer=dict(kernel_size=3, padding=1))
    with pytest.raises(NotImplementedError, match="1x1"):
        build(final_layer=None)
    head = build()
    with pytest.raises(NotImplementedError, match="training"):
        head.loss(None, None)
    with pytest.raises(RuntimeError, match="TopdownPoseEstimator"):
        head.forward((torch.zeros(1, 384, 16, 12),))


def _model():
    from probpose_code_amd import Config, build_pose_estimator

    m = dict(Config.fromfile(CFG).model)
    m.pop("train_cfg", None)
    return build_pose_estimator(m)


def test_config_builds_the_baseline_and_keeps_ground_truth_boxes():
    import probpose_code_amd as pp
    from probpose_code_amd.datasets import build_dataset

    cfg = pp.Config.fromfile(CFG)
    model = _model()
    assert isinstance(model.head, pp.HeatmapHead) and isinstance(model.head.decoder, pp.UDPHeatmap)
    assert model.test_cfg == dict(flip_test=True, flip_mode="heatmap", shift_heatmap=False)
    assert cfg.test_evaluator["type"] == "CocoMetric" and "bbox_file" not in cfg.test_dataloader.dataset
    with pytest.raises(NotImplementedError, match="bbox_file"):  # the reference config's detector boxes stay refused
        build_dataset(dict(cfg.test_dataloader.dataset, bbox_file="person_detection_results/COCO_val2017_detections_AP_H_56_person.json"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.engine
    model.test_cfg["flip_mode"] = "udp_combined"
    with pytest.raises(NotImplementedError, match="udp_combined"):
        model._check_flip_cfg()


def test_state_dict_keys_round_trip_and_old_checkpoints():
    from probpose_code_amd import apis, synthetic

    model = _model()
    sd = synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0, head="heatmap")
    head_keys = sorted(k for k in sd if k.startswith("head."))
    assert head_keys == sorted(f"head.{k}" for k in model.head.state_dict())  # head.deconv_layers.{0,1,3,4}.*, head.final_layer.*
    assert {k.split(".")[2] for k in head_keys if "deconv_layers" in k} == {"0", "1", "3", "4"}
    assert not any("_layers." in k and "deconv" not in k for k in head_keys), "tower keys in a heatmap state dict"
    apis.load_state_dict_checked(model, sd)
    back = model.state_dict()
    for k, v in sd.items():
        assert torch.equal(back[k], v), k
    # equal seeds: the backbone and the deconvolutions are the ProbPose model's tensors; the final layer's weights are centred per keypoint
    full = synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0)
    assert set(sd) < set(full) and all(torch.equal(full[k], v) for k, v in sd.items() if k != "head.final_layer.weight")
    fw = full["head.final_layer.weight"]
    assert torch.equal(sd["head.final_layer.weight"], fw - fw.mean(dim=1, keepdim=True))
    assert sd["head.final_layer.weight"].sum(dim=1).abs().max() < 1e-4
    with pytest.raises(ValueError, match="head must be"):
        synthetic.synthetic_state_dict("small", head="simcc")
    # a checkpoint written before MMPose 1.0: `keypoint_head.` prefix, preprocessor statistics, no version
    old = {k.replace("head.", "keypoint_head.", 1) if k.startswith("head.") else k: v for k, v in sd.items()}
    old["data_preprocessor.mean"] = torch.zeros(3)
    model2 = _model()
    apis.load_state_dict_checked(model2, old)
    assert all(torch.equal(model2.state_dict()[k], v) for k, v in sd.items())
    # `final_layer.n.*` belongs to a head with intermediate conv layers: refused as the reference's hook refuses it
    bad = dict(sd)
    bad["head.final_layer.0.weight"] = bad.pop("head.final_layer.weight")
    with pytest.raises(AssertionError, match="intermediate conv"):
        _model().load_state_dict(bad, strict=False)
    # a ProbPose checkpoint does not load silently into the baseline, nor the other way round
    with pytest.warns(RuntimeWarning, match="unexpected key"):
        apis.load_state_dict_checked(_model(), full)
    from probpose_code_amd import Config, build_pose_estimator

    pm = dict(Config.fromfile(os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")).model)
    with pytest.raises(RuntimeError, match="does not provide"):
        apis.load_state_dict_checked(build_pose_estimator(pm), sd)


def test_head_kind_of_a_config():
    from probpose_code_amd import Config, synthetic

    assert synthetic.head_kind_of(Config.fromfile(CFG)) == "heatmap"
    assert synthetic.head_kind_of(Config.fromfile(os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py"))) == "probmap"
    assert synthetic.head_kind_of(dict(model=dict(head=dict(type="mmpose.HeatmapHead")))) == "heatmap"
    assert synthetic.head_kind_of(dict(model=dict(head=None))) == "probmap"


def test_pack_records_and_datasample_fields():
    from probpose_code_amd import apis

    model = _model()
    rng = np.random.default_rng(0)
    B, K = 4, 17
    rec = np.zeros((B, K, 7))
    rec[..., :2] = rng.uniform(0, 255, (B, K, 2))
    rec[..., 2] = rng.random((B, K)).astype(np.float32)
    preds = model.head.pack_records(rec.copy(), model.test_cfg)
    assert len(preds) == B
    for b, p in enumerate(preds):
        assert p.keypoints.dtype == np.float64 and np.array_equal(p.keypoints, rec[b:b + 1, :, :2])
        assert p.keypoint_scores.dtype == np.float32 and np.array_equal(p.keypoint_scores, rec[b:b + 1, :, 2].astype(np.float32))
        assert "keypoints_probs" not in p and "keypoints_visible" not in p
    c = rng.uniform(50, 500, (B, 2)).astype(np.float32)
    s = rng.uniform(100, 700, (B, 2)).astype(np.float32)
    batch = apis.pack_crops(torch.zeros(B, 3, 256, 192, dtype=torch.uint8), c, s, apis.coco_dataset_meta())
    out = model.add_pred_to_datasample(preds, None, batch["data_samples"])
    for b, ds in enumerate(out):
        m = ds.metainfo
        want = rec[b:b + 1, :, :2] / m["input_size"] * m["input_scale"] + m["input_center"] - 0.5 * m["input_scale"]
        assert np.array_equal(ds.pred_instances.keypoints, want)
        # topdown.py:168-169: a head without a visibility output
        assert np.array_equal(ds.pred_instances.keypoints_visible, ds.pred_instances.keypoint_scores)
    bad = rec.copy()
    bad[2, 5, 0] = np.nan

    class _E:
        precision = "f16x3"

    model._engine = _E()
    with pytest.raises(FloatingPointError, match=r"crop\(s\) \[2\]"):
        model.head.pack_records(bad, model.test_cfg)


def test_coco_metric_on_samples_without_probabilities():
    """Samples as a HeatmapHead model's test step leaves them: no ``keypoints_probs``."""
    from probpose_code_amd.evaluation import CocoMetric

    rng = np.random.default_rng(1)
    anns, imgs, samples = [], [], []
    for i in range(6):
        imgs.append(dict(id=i + 1, width=640, height=480, file_name=f"{i}.png"))
        kp = np.concatenate([rng.uniform(100, 300, (17, 2)), np.full((17, 1), 2.0)], 1)
        x0, y0, x1, y1 = kp[:, 0].min() - 10, kp[:, 1].min() - 10, kp[:, 0].max() + 10, kp[:, 1].max() + 10
        anns.append(dict(id=100 + i, image_id=i + 1, category_id=1, keypoints=kp.reshape(-1).tolist(), num_keypoints=17, iscrowd=0,
                         bbox=[x0, y0, x1 - x0, y1 - y0], area=float((x1 - x0) * (y1 - y0))))
        samples.append(dict(id=100 + i, img_id=i + 1, category_id=1,
                            pred_instances=dict(keypoints=kp[None, :, :2], keypoint_scores=np.full((1, 17), 0.9, np.float32),
                                                bboxes=np.array([[x0, y0, x1, y1]], np.float32)),
                            gt_instances=dict(bbox_scores=np.ones(1, np.float32), bbox_scales=np.array([[x1 - x0, y1 - y0]], np.float32))))
    gt = dict(images=imgs, annotations=anns, categories=[dict(id=1, name="person")])
    metric = CocoMetric(gt)
    metric.process(None, samples)
    assert metric.has_probability is False  # the `score_acc` / `score_thr` branch of compute_metrics (the Ex-OKS evaluation itself is a GPU kernel)
    assert len(metric.results) == 6
    for pred, smp in zip(metric.results, samples):
        # what the evaluator reads as visibility and probability falls back to the keypoint scores (coco_metric.py:262-266)
        assert np.array_equal(pred["keypoints_visible"], smp["pred_instances"]["keypoint_scores"])
        assert np.array_equal(pred["keypoint_probs"], smp["pred_instances"]["keypoint_scores"])
        assert pred["areas"].shape == (1,)


def test_udp_decode_argument_validation_without_gpu(lib_built):
    from probpose_code_amd import _lib

    f = _lib.lib.pp_udp_heatmap_decode
    one = torch.zeros(4)
    p = one.data_ptr()
    assert f(None, None, None, 1, 17, 64, 48, 192.0, 256.0, 11, None, None, None, None, 0, None) == _lib.PP_ERR_INVALID_ARG
    assert b"non-NULL" in _lib.lib.pp_last_error()
    assert f(p, None, None, 0, 17, 64, 48, 192.0, 256.0, 11, None, p, p, p, 0, None) == _lib.PP_OK  # an empty batch launches nothing
    assert f(p, None, None, 1, 17, 64, 48, 192.0, 256.0, 10, None, p, p, p, 0, None) == _lib.PP_ERR_INVALID_ARG  # even kernel size
    assert f(p, None, None, 1, 17, 64, 48, 192.0, 256.0, 21, None, p, p, p, 0, None) == _lib.PP_ERR_UNSUPPORTED
    assert f(p, None, None, 1, 17, 64, 48, 192.0, 256.0, 11, None, p, p, p, 1, None) == _lib.PP_ERR_INVALID_ARG  # PP_DECODE_LOGITS: not this decode's
    assert f(p, None, None, 1, 17, 63, 48, 192.0, 256.0, 11, None, p, p, p, 2, None) == _lib.PP_ERR_UNSUPPORTED  # phased: even sizes
    assert f(p, p, None, 1, 17, 64, 48, 192.0, 256.0, 11, None, p, p, p, 0, None) == _lib.PP_ERR_INVALID_ARG
    assert b"flip_indices" in _lib.lib.pp_last_error()
    assert f(p, None, None, 1, 17, 128, 128, 192.0, 256.0, 11, None, p, p, p, 0, None) == _lib.PP_ERR_UNSUPPORTED  # 16 384 pixels
    assert f(p, None, None, 1, 17, 8, 1536, 192.0, 256.0, 19, None, p, p, p, 0, None) == _lib.PP_ERR_UNSUPPORTED  # LDS images beyond 160 KiB
    assert f(p, None, None, 1, 17, 1, 48, 192.0, 256.0, 11, None, p, p, p, 0, None) == _lib.PP_ERR_INVALID_ARG
    assert _lib.lib.pp_abi_version() == 4
