"""tests/fuzz_wide.py on the CPU: its row-sampled fp64 reference equals the full product, its restatement of pp_gemm's dispatch gives the
thresholds the kernels' sources state (csrc/pp_linear_dma.hip: 512 tiles of 192 x 192; csrc/pp_panel_split.hip: 192 wide tiles), the
deconvolution reference it borrows from tests/fuzz_conv.py equals torch's conv_transpose2d in fp64, and its tolerances reject a Linear layer
computed from fp16 operands (the low halves of the split format dropped) at the deepest K while the split format's own rounding passes."""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fuzz_wide as W  # noqa: E402
from fuzz_layer import TOL, error_ratio, magnitude_factor, sample_rows  # noqa: E402


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def test_row_sampled_reference_equals_the_full_product():
    M, N, K, res_mod = 1500, 96, 160, 192
    x, w, b = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=K ** -0.5), _rand(N, seed=3).float()
    table, r = _rand(res_mod, N, seed=4), _rand(M, N, seed=5)
    rows = sample_rows(M, 256, np.random.default_rng(0))
    assert 2 * 256 < len(rows) < M and int(rows[0]) == 0 and int(rows[-1]) == M - 1
    assert set(range(256)) <= set(rows.tolist()) and set(range(M - 256, M)) <= set(rows.tolist())
    assert all(any(lo <= v < lo + 256 for v in rows.tolist()) for lo in range(0, M, 256)), "a row of every block"
    full = F.linear(x, w, b.double())
    torch.testing.assert_close(W.linear_ref64(x[rows], w, b, W.ACT_NONE, None), full[rows], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(W.linear_ref64(x[rows], w, b, W.ACT_GELU, None), F.gelu(full)[rows], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(W.linear_ref64(x[rows], w, None, W.ACT_RELU, r[rows]), (torch.relu(F.linear(x, w)) + r)[rows], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(W.linear_ref64(x[rows], w, b, W.ACT_NONE, table[rows % res_mod]), (full + table[torch.arange(M) % res_mod])[rows],
                               rtol=1e-12, atol=1e-12)


def test_restated_dispatch_thresholds():
    assert W.dma_threshold(3072) == 5953 and W.dma_threshold(3840) == 4801
    for N, K in ((3072, 1024), (3840, 1280)):
        t = W.dma_threshold(N)
        assert W.gemm_kernel(W.F16X3, t, N, K, 2, False) == "linear_dma_tile" and W.gemm_kernel(W.F16X3, t - 1, N, K, 2, False) == "pp_panel_split.hip"
        assert (N // 192) * math.ceil(t / 192) >= 512 > (N // 192) * math.ceil((t - 1) / 192)
        w = W.wide_threshold(N)
        assert W.gemm_kernel(W.F16X3, w, N, K, 2, False) == "pp_panel_split.hip" and W.gemm_kernel(W.F16X3, w - 1, N, K, 2, False) == "pp_gemm.hip"
        assert W.wide_tiles(w, N) >= 192 > W.wide_tiles(w - 1, N)
    # one round of the chip either way: the 192-row tile (three quarters of the area) wins, and 192 tiles of it are twelve / ten tile rows
    assert W.wide_threshold(3072) == 192 * 11 + 1 and W.wide_threshold(3840) == 192 * 9 + 1
    # every other Linear width of ViT-L / -H is no multiple of 192: the 128 x 128 kernel at every M, in every precision
    for (arch, layer), (N, K) in W.TABLE.items():
        if layer != "qkv":
            for prec in (W.F16X3, W.BF16, W.F32):
                assert {W.gemm_kernel(prec, M, N, K, W.engine_epilogue(layer, prec)["fmt"], True) for M in (1, 385, 4801, 24576)} == {"pp_gemm.hip"}
    # bf16: the wide-tile kernel from K = 768 (fp32 rows out) / 1536 (bf16 rows out) on; f32: never
    assert W.gemm_kernel(W.BF16, 24576, 3072, 1024, 1, False) == "pp_gemm.hip" and W.gemm_kernel(W.BF16, 24576, 3072, 1024, 0, False) == "pp_panel_split.hip"
    assert W.gemm_kernel(W.F32, 24576, 3072, 1024, 0, False) == "pp_gemm.hip"
    # the engine's rows at B = 64 with flip test (49 152): qkv on the twelve-wave kernel
    assert W.gemm_kernel(W.F16X3, 128 * 384, 3072, 1024, 2, False) == W.gemm_kernel(W.F16X3, 128 * 384, 3840, 1280, 2, False) == "linear_dma_tile"


def test_deconvolution_tile_boundary():
    # 16 x 12 = 192 input pixels an image = one 192-pixel tile; 256 output channels = one 256-column tile; four phases in one launch
    assert W.deconv_tiles(47, -1) == 188 and W.deconv_tiles(48, -1) == 192 and W.deconv_threshold(-1) == 48
    assert W.deconv_tiles(191, 0) == 191 and W.deconv_threshold(0) == W.deconv_threshold(3) == 192
    import fuzz_conv as FC

    for nb, phase, want in ((47, -1, "pp_gemm.hip"), (48, -1, "pp_panel_split.hip"), (191, 2, "pp_gemm.hip"), (192, 2, "pp_panel_split.hip")):
        for cin in W.DECONV_CIN:
            assert FC.conv_kernel(W.F16X3, W.DECONV, nb, 16, 12, cin, 256, 4 if phase < 0 else 1, 2, W.ACT_RELU, FC.DEFAULT_OPTIONS) == want
    # a phase's weight set against the 3 MiB at which the wide-tile kernel gives up the weight-major order: only Cin = 768 stays inside
    assert [4 * cin * 256 * 4 > 3 * 1024 * 1024 for cin in W.DECONV_CIN] == [False, True, True]


def test_deconvolution_reference_equals_conv_transpose2d():
    B, Cin, Cout, H, Wd = 2, 24, 16, 5, 4
    x, w, b = _rand(B, Cin, H, Wd, seed=10), _rand(Cin, Cout, 4, 4, seed=11, scale=0.2), _rand(Cout, seed=12)
    want = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    torch.testing.assert_close(W.deconv64(x, w, b), want, rtol=1e-12, atol=1e-12)
    # ... and the phase matrices the kernels are handed stand for the same weights
    ph = W.deconv_phases(w)
    xp = F.pad(x, (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            cols = torch.cat([xp[:, :, py + ty:py + ty + H, px + tx:px + tx + Wd] for ty in range(2) for tx in range(2)], dim=1)
            got = torch.einsum("bkhw,ok->bohw", cols, ph[py, px]) + b.view(1, -1, 1, 1)
            torch.testing.assert_close(got, want[:, :, py::2, px::2], rtol=1e-12, atol=1e-12)


def test_tolerance_at_the_deepest_k_rejects_fp16_operands_and_passes_the_split_format():
    """K = 5120 (fc2 of ViT-H), unit-normal rows: the split format's rounding (hi + lo of both operands, exact products, fp64 sums) sits far
    inside TOL["linear_long"]; operands rounded to fp16 - a kernel that dropped the low halves - are rejected."""
    from probpose_code_amd.weights import from_split, to_split

    M, N, K = 24, 64, 5120
    x, w = _rand(M, K, seed=20).float(), _rand(N, K, seed=21, scale=K ** -0.5).float()
    ref = x.double() @ w.double().t()
    tol = TOL["linear_long"] * magnitude_factor(x) * W.weight_factor(w.double(), K)
    split = from_split(to_split(x)).double() @ from_split(to_split(w * 4096.0)).double().t() / 4096.0
    assert error_ratio(split, ref, tol, tol) < 0.1
    half = x.half().double() @ w.half().double().t()
    assert error_ratio(half, ref, tol, tol) > 1.0
