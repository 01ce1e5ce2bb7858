"""The engine's launch plans, pinned call by call.

``tests/golden/launch_plans.json`` holds, for every case of ``launch_trace.CASES``, the C-ABI calls of one eager forward with their arguments
(pointers as buffer names + offsets), the ``layer_plan`` string and the workspace buffers that exist - recorded from the engine as it was
when this test was added. The engine under test must issue the same calls, entry for entry; its workspace may have lost buffers that no
recorded launch names and gained none. The golden file is never regenerated from later code: a host-side rewrite of the engine (where the
plan is decided, how the launch code reads) that changes a trace has changed behaviour.

Host part (no GPU): the recorded traces themselves reach the branch each case is there for.
"""
import json

import pytest
import torch

import launch_trace as LT

gpu = pytest.mark.gpu
RESULT_KEYS = {"keypoints", "scores", "locs", "scalars", "heatmaps"}


@pytest.fixture(scope="module")
def golden():
    with open(LT.GOLDEN_FILE) as f:
        return json.load(f)


def _names(trace):
    return [c.split("(", 1)[0] for c in trace]


# case -> (functions its recorded trace must contain, functions it must not contain)
REACHES = {
    "s3_b1": (["pp_skinny_linear", "pp_qkv_attention_split_ws", "pp_skinny_deconv", "pp_skinny_conv1x1_planar", "pp_conv3x3_splitk"],
              ["pp_conv_gemm", "pp_gemm_ws", "pp_conv3x3_winograd_maxpool_relu"]),
    "s3_b4": (["pp_skinny_linear", "pp_skinny_deconv", "pp_conv_gemm"], []),
    "s3_b17": (["pp_skinny_linear"], ["pp_proj_ffn_split_folded"]),
    "s3_b18": (["pp_qkv_attention_split_folded", "pp_proj_ffn_split_folded", "pp_deconv_head_split", "pp_conv3x3_winograd_maxpool_relu",
                "pp_conv3x3_splitk"], ["pp_skinny_linear", "pp_layernorm"]),
    "s3_b18_no_ln_fold": (["pp_proj_ffn_split_residual_layernorm_ws"], ["pp_proj_ffn_split_folded", "pp_qkv_attention_split_folded"]),
    "s3_b18_no_fuse_qkv_attn": (["pp_gemm_ws", "pp_attention", "pp_proj_ffn_split_residual_layernorm_ws"], ["pp_qkv_attention_split_ws"]),
    "s3_b18_no_fuse_proj": (["pp_qkv_attention_split_ws", "pp_gemm_residual_layernorm_ws", "pp_ffn_split_residual_layernorm_ws"], []),
    "s3_b18_no_fuse_mlp": (["pp_qkv_attention_split_ws", "pp_gemm_residual_layernorm_ws", "pp_gemm_ws"],
                           ["pp_ffn_split_residual_layernorm_ws", "pp_proj_ffn_split_folded"]),
    "s3_b18_no_winograd": (["pp_conv3x3_maxpool_relu"], ["pp_conv3x3_winograd_maxpool_relu"]),
    "s3_b18_no_fuse_pool_no_winograd": (["pp_conv_gemm", "pp_maxpool_relu_nhwc"], ["pp_conv3x3_maxpool_relu"]),
    "s3_b18_no_split_k": ([], ["pp_conv3x3_splitk"]),
    "s3_b18_no_fuse_head": (["pp_conv_gemm", "pp_gemm_ws"], ["pp_deconv_head_split"]),
    "s3_b1_no_small_plan": (["pp_proj_ffn_split_folded"], ["pp_skinny_linear", "pp_skinny_deconv", "pp_skinny_conv1x1_planar"]),
    "s3_384x288_b2_no_small_plan": (["pp_gemm_ws", "pp_attention", "pp_proj_ffn_split_residual_layernorm_ws"], ["pp_qkv_attention_split_ws"]),
    "b3_b18": (["pp_gemm_ws", "pp_layernorm", "pp_attention"], ["pp_skinny_linear", "pp_linear_ln_folded_ws"]),
    "b3_b64": (["pp_linear_ln_folded_ws", "pp_attention", "pp_layernorm"], ["pp_skinny_linear"]),
    "b3_b2_no_small_plan": (["pp_gemm_ws", "pp_layernorm", "pp_attention"], ["pp_linear_ln_folded_ws", "pp_gemm_residual_layernorm_ws"]),
    "b3_b2": (["pp_skinny_linear", "pp_attention"], []),
    "b3_b2_no_small_plan_resln": (["pp_gemm_residual_layernorm_ws"], ["pp_layernorm"]),
    "l2_b1": (["pp_skinny_linear"], []),
    "h2_b1": (["pp_gemm_ws", "pp_attention"], ["pp_skinny_linear"]),
    "bf16_s3_b8": (["pp_vit_layer", "pp_deconv_head"], ["pp_attention", "pp_proj_mlp_residual_layernorm"]),
    "bf16_s3_b8_no_fuse_attn": (["pp_attention", "pp_proj_mlp_residual_layernorm"], ["pp_vit_layer"]),
    "bf16_s3_b8_no_fuse_proj": (["pp_mlp_residual_layernorm"], ["pp_vit_layer", "pp_proj_mlp_residual_layernorm"]),
    "bf16_s3_b8_no_fuse_mlp": (["pp_gemm_ws"], ["pp_vit_layer", "pp_mlp_residual_layernorm"]),
    "bf16_s3_b8_no_fuse_head": (["pp_conv_gemm"], ["pp_deconv_head"]),
    "bf16_s3_b8_no_fuse_resln": (["pp_layernorm"], ["pp_gemm_residual_layernorm_ws", "pp_vit_layer"]),
    "s3_b2_heatmap": (["pp_udp_heatmap_decode"], ["pp_tower_final"]),
    "s3_b2_heatmap_expmax": (["pp_expmax_heatmap_decode"], ["pp_tower_final"]),
    "s3_b2_probmap_dark": (["pp_argmax_probmap_decode", "pp_tower_final"], []),
    "s3_b2_return_heatmaps": (["pp_probmap_decode_flags"], []),
}


def test_golden_covers_the_cases(golden):
    assert sorted(golden) == sorted(c["name"] for c in LT.CASES)
    for c in LT.CASES:
        assert golden[c["name"]]["warned"] == c["warns"], c["name"]


@pytest.mark.parametrize("name", sorted(REACHES))
def test_golden_reaches_its_branch(golden, name):
    names = set(_names(golden[name]["trace"]))
    has, has_not = REACHES[name]
    assert not [f for f in has if f not in names], (name, sorted(names))
    assert not [f for f in has_not if f in names], (name, sorted(names))


def test_golden_streams_and_flags(golden):
    side = lambda n: any(c.endswith(", side)") for c in golden[n]["trace"])  # noqa: E731
    assert side("s3_b1") and side("s3_b17") and not side("s3_b18") and not side("s3_b1_one_stream") and not side("s3_b1_no_small_plan")
    assert golden["s3_b18"]["logits_phased"] and not golden["s3_b1"]["logits_phased"] and golden["bf16_s3_b8"]["logits_phased"]
    assert any("ws:heatmaps+0" in c for c in golden["s3_b2_return_heatmaps"]["trace"])
    assert not any("ws:heatmaps+0" in c for c in golden["s3_b2_shift_heatmap"]["trace"])
    assert not any("flip_indices" in c for c in golden["s3_b2_no_flip"]["trace"])


@gpu
@pytest.mark.parametrize("case", LT.CASES, ids=[c["name"] for c in LT.CASES])
def test_launch_trace_equals_recorded(golden, case):
    want = golden[case["name"]]
    eng, warned = LT.build_engine(case)
    assert warned == case["warns"]
    assert eng.layer_plan == want["layer_plan"]
    if case["arch"] == "B3":  # the folded-Linear plan engages between these two
        assert eng._ln_fold_at(case["B"] * 2 * eng.Np) == (case["name"] == "b3_b64")
    imgs, flip = LT.case_inputs(case)
    got, _ = LT.trace_forward(eng, imgs, case, flip)
    assert len(got) == len(want["trace"]), (_names(got), _names(want["trace"]))
    for k, (g, w) in enumerate(zip(got, want["trace"])):
        assert g == w, f"call {k} differs:\n  got      {g}\n  recorded {w}"
    assert bool(eng._logits_phased) == want["logits_phased"]
    keys = {k for k, v in eng._workspace(case["B"], 2 if case["flip_test"] else 1, 0).items() if v is not None}
    assert keys <= set(want["ws_keys"]), f"workspace gained {sorted(keys - set(want['ws_keys']))}"
    for lost in set(want["ws_keys"]) - keys:
        assert lost not in RESULT_KEYS and not any(f"ws:{lost}+" in c for c in want["trace"]), f"workspace lost {lost}, which a recorded launch names"


@gpu
@pytest.mark.parametrize("B", [1, 18])
def test_replayed_graph_equals_eager(B):
    """``capture`` (its key, the fork / join inside the capture at B = 1) against the launches one by one: bit for bit."""
    case = next(c for c in LT.CASES if c["name"] == f"s3_b{B}")
    eng, _ = LT.build_engine(case)
    imgs, flip = LT.case_inputs(case)
    eager = {k: v.clone() for k, v in eng.forward(imgs, True, flip).items()}
    torch.cuda.synchronize()
    replayed = eng.forward_graph(imgs, True, flip)
    torch.cuda.synchronize()
    assert eng.has_graph(B, True, flip) and eng.graph_captures == 1
    assert sorted(replayed) == sorted(eager)
    for k in eager:
        assert torch.equal(replayed[k].view(torch.uint8), eager[k].view(torch.uint8)), k
