"""CPU: the references of the ViTPose ``-simple`` head tests (tests/simple_head_ref.py) checked against each other, before any GPU run.

(a) the composed form - the 3x3 convolution as nine taps at low resolution, then the bilinear x4 gather - equals the reference's order
    ``conv2d(interpolate(relu(x)))`` in fp64 to 1e-12 relative;
(b) the bound the GPU test holds pp_taps_upsample4_conv3x3 to, ``41 * 2^-24 * S``, holds for an fp32 emulation of the formula (every
    product, nested weight and addition rounded: at most 40 roundings on any path, plus one for the second-order term) on the inputs the
    GPU test uses - and rejects each single fault a kernel of this kind can have, on those same inputs;
(c) the synthetic model of the end-to-end GPU test (``calibrated_state_dict(0)``, crop seed 100): every flip-averaged / plain reference map
    has a positive maximum, and the share of keypoints the fp64 DARK decode leaves out of the coordinate comparison (Hessian condition
    number >= 100) stays under the GPU test's cap. Measured (with flip test / without): B 1: 1 of 17 / 1 of 17; B 8: 2 of 136 / 2 of 136;
    B 20: 6 of 340 (1.8 %) / 4 of 340 (1.2 %); B 64: 12 of 1088 / 13 of 1088; smallest maximum over the eight cases 0.030. B 1 and 8 are
    re-measured here; this docstring is the record of the other two batch sizes.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_head_ref as R  # noqa: E402


@pytest.mark.parametrize("K", [1, 17])
@pytest.mark.parametrize("hw", [(1, 1), (1, 3), (2, 2), (3, 5), (16, 12)])
def test_composed_form_equals_the_reference_order_in_fp64(hw, K):
    h, w = hw
    g = torch.Generator().manual_seed(17 * h + w + K)
    x = torch.randn(2, 64, h, w, generator=g, dtype=torch.float64) * 3
    W = torch.randn(K, 64, 3, 3, generator=g, dtype=torch.float64) * 0.05
    b = torch.randn(K, generator=g, dtype=torch.float64)
    ref = R.reference_order(x, W, b, torch.float64).numpy()
    out, _ = R.composed(R.taps_of(x, W, torch.float64), b.numpy(), K, h, w, np.float64)
    err = np.abs(out - ref).max() / np.abs(ref).max()
    assert err <= 1e-12, f"{h}x{w} K {K}: composed form off by {err:.2e} relative"


@pytest.mark.parametrize("shape", R.GATHER_SHAPES)
def test_bound_holds_for_an_fp32_emulation_and_rejects_single_faults(shape):
    n, K, h, w = shape
    worst = {f: 0.0 for f in R.FAULTS}
    for name, taps, bias in R.gather_inputs(*shape):
        ref, S = R.composed(taps, bias, K, h, w, np.float64)
        emu, _ = R.composed(taps, bias, K, h, w, np.float32)
        assert (np.abs(emu - ref) <= R.BOUND * S).all(), f"{shape} {name}: the fp32 emulation misses the bound by {(np.abs(emu - ref) / np.maximum(S, 1e-300)).max() / R.BOUND:.2f}x"
        if name == "constant":  # the count of in-map taps: corners 4, edges 6, inside 9
            counts = set(np.unique(ref).tolist())
            assert counts <= {4.0, 6.0, 9.0} and 4.0 in counts, counts
            assert ref[0, 0, 0, 0] == 4 and ref[0, 0, -1, -1] == 4 and ref[0, 0, 1, 0] == 6 and ref[0, 0, 1, 1] == 9
        for f in R.FAULTS:
            bad, _ = R.composed(taps, bias, K, h, w, np.float64, fault=f)
            with np.errstate(divide="ignore", invalid="ignore"):
                over = np.where(S > 0, np.abs(bad - ref) / (R.BOUND * S), np.where(bad != ref, np.inf, 0.0))
            worst[f] = max(worst[f], float(over.max()))
    for f in R.FAULTS:
        if (h, w) == (1, 1) and f in ("align_corners", "no_clamp0"):
            continue  # (a plane of one sample: every sampling rule reads that sample with weight 1 - these two are no faults there)
        assert worst[f] > 1.0, f"{shape}: the bound does not reject the fault {f!r} (largest deviation {worst[f]:.3g} x bound)"


@pytest.mark.parametrize("B", [1, 8])
def test_the_calibrated_synthetic_model_has_decodable_maps(B):
    import udp_ref as U
    from probpose_code_amd import synthetic as S

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = R.calibrated_state_dict(0)
    assert tuple(sd["head.final_layer.weight"].shape) == (17, 384, 3, 3) and not any(k.startswith("head.deconv_layers.") for k in sd)
    crops = S.synthetic_crops(B, seed=100)
    for flip in (True, False):
        ref = R.reference_heatmaps(sd, crops, flip)
        assert ref.shape == (B, 17, 64, 48)
        maxima = ref.reshape(B, 17, -1).max(-1)
        conds = np.concatenate([U.decode_f64(m, 11, (192, 256))["cond"] for m in ref])
        left_out = int((~(conds < 100)).sum())
        print(f"B {B} flip {flip}: smallest maximum {maxima.min():.3f}, left out {left_out} of {conds.size}, largest |value| {np.abs(ref).max():.2f}")
        assert (maxima > 0).all(), "a synthetic map without a positive maximum"
        assert left_out <= max(1, int(0.05 * conds.size)), f"{left_out} of {conds.size} keypoints left out on the reference's own maps"
