"""GPU: the Linear and deconvolution kernels at the ViT-L / ViT-H widths against fp64 (tests/fuzz_wide.py's single cases on a fixed grid, then
the fuzzer for a few seconds).

  * pp_gemm_ws at the ten layer shapes of fuzz_wide.TABLE x three precisions, each with the epilogue the engine sends with it. The qkv shapes
    (N = 3072 / 3840, the only multiples of 192) at M = 1, 385, the last row count below the twelve-wave kernel's threshold (5952 / 4800: the
    wide-tile kernel in f16x3) and a ragged tile above it (the twelve-wave kernel at K = 1024 / 1280: 32 / 40 K-steps on its ring of three
    stages); the others (the 128 x 128 kernel at every M, K up to 5120) at M = 1, 385, 4801.
  * the first head deconvolution, Cin = 768 / 1024 / 1280 -> 256 on the 16 x 12 map, three precisions: two images phase by phase (the 128 x 128
    kernel) and 64 images in one launch (256 wide tiles); in f16x3 also with the weight-major tile order asked for, which the wide-tile kernel
    honours at Cin = 768 and drops above (a phase's weight set over 3 MiB); pp_skinny_deconv on one and eight images.
  * pp_skinny_linear at the five ViT-L small-batch shapes, M = 1, 1536, 6911, every tile shape that divides N forced in turn.
Every case: canaries, every element written, inputs unchanged, a repeat launch bit-identical, the kernel the restated dispatcher predicts, and
error / tolerance <= 1 under the tolerances fuzz_wide.py's docstring derives from the project's fixed ones.
  * the regression the fuzzer found: bf16 rows out with an fp32 residual were rounded twice by the 128 x 128 kernel."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fuzz_wide as W  # noqa: E402

pytestmark = pytest.mark.gpu

PRECS = {"f16x3": W.F16X3, "bf16": W.BF16, "f32": W.F32}


def _gemm_grid():
    for (arch, layer), (N, _) in W.TABLE.items():
        t = W.dma_threshold(N) if layer == "qkv" else None
        for M in ([1, 385, t - 1, t + 100] if layer == "qkv" else [1, 385, 4801]):
            yield pytest.param(arch, layer, M, id=f"{arch}-{layer}-M{M}")


def _report(faults, ratio, info):
    print(f"{info}: error / tolerance {ratio:.3g}")
    assert not faults, (info, faults)
    assert ratio <= 1.0, f"{info}: error / tolerance {ratio:.3g}"


@pytest.mark.parametrize("arch,layer,M", list(_gemm_grid()))
@pytest.mark.parametrize("precision", list(PRECS))
def test_linear_layer_of_large_and_huge_against_fp64(precision, arch, layer, M):
    prec = PRECS[precision]
    N, K = W.TABLE[(arch, layer)]
    seed = 7000 + 97 * list(W.TABLE).index((arch, layer)) + M % 89 + 13 * prec
    cls_a, cls_w = W.CLASSES[seed % 3], W.CLASSES[(seed // 3) % 3]
    if cls_a == cls_w == "offset":
        cls_w = "massive"
    ran = []
    faults, ratio, info = W.gemm_case(prec, M, N, K, W.engine_epilogue(layer, prec), seed, cls_a, cls_w, e=None, ran=ran, must_accept=True)
    _report(faults, ratio, f"{arch} {layer}: {info}")
    if layer == "qkv" and prec == W.F16X3:
        t = W.dma_threshold(N)
        assert ran == ["linear_dma_tile" if M >= t else "pp_panel_split.hip" if M == t - 1 else "pp_gemm.hip"], ran
    elif layer != "qkv":
        assert ran == ["pp_gemm.hip"], ran


@pytest.mark.parametrize("nb,phase", [(2, 1), (64, -1)])
@pytest.mark.parametrize("cin", W.DECONV_CIN)
@pytest.mark.parametrize("precision", list(PRECS))
def test_first_head_deconvolution_against_fp64(precision, cin, nb, phase):
    prec = PRECS[precision]
    ran = []
    _report(*W.deconv_case(prec, cin, nb, phase, 8000 + cin + nb + prec, cls="massive" if nb == 2 else "normal", ran=ran))
    wide = {W.F16X3: "pp_panel_split.hip", W.BF16: "pp_panel_gemm.hip", W.F32: "pp_gemm.hip"}[prec]
    assert ran == [wide if nb == 64 else "pp_gemm.hip"], ran


@pytest.mark.parametrize("cin", W.DECONV_CIN)
def test_deconvolution_with_the_weight_major_order_asked_for(cin):
    """Option "psplit_deconv_weight_major": the tile order the wide-tile kernel keeps while a phase's weight set (4 Cin x 256 x 4 bytes) is at
    most 3 MiB - Cin = 768 - and drops for the row-major one above it. The result is the same deconvolution either way."""
    ran = []
    _report(*W.deconv_case(W.F16X3, cin, 64, -1, 8100 + cin, cls="massive", weight_major=1, ran=ran))
    assert ran == ["pp_panel_split.hip"], ran


@pytest.mark.parametrize("nb", [1, 8])
@pytest.mark.parametrize("cin", W.DECONV_CIN)
def test_skinny_deconvolution_against_fp64(cin, nb):
    for code in W.SKINNY_DECONV_CODES:
        _report(*W.skinny_deconv_case(cin, nb, code, 8200 + cin + nb, cls="border" if nb == 1 else "normal"))


@pytest.mark.parametrize("M", [1, 1536, 6911])
@pytest.mark.parametrize("shape", W.SKINNY_SHAPES, ids=[f"{s[2]}-{s[0]}x{s[1]}" for s in W.SKINNY_SHAPES])
def test_skinny_linear_at_the_large_shapes_against_fp64(shape, M):
    codes = W.skinny_codes(shape[0])
    assert len(codes) == (7 if shape[0] % 96 == 0 else 4)
    for xcd in (0, 1):
        _report(*W.skinny_case(shape, M, codes, xcd, 8300 + M + shape[0] + shape[1] + xcd, e=None))


# ------------------------------------------------------------------------------------------------- regression: found by tests/fuzz_wide.py
@pytest.mark.parametrize("M,N,K,res_mod,kernel", [(385, 104, 64, 0, "pp_gemm.hip"), (3662, 64, 896, 7, "pp_gemm.hip"), (6144, 1536, 1536, 192, "pp_panel_split.hip")],
                         ids=["M385-N104-K64", "M3662-N64-K896-table7", "M6144-N1536-K1536-wide"])
def test_bf16_rows_out_with_an_fp32_residual_are_rounded_once(M, N, K, res_mod, kernel):
    """pp_gemm in bf16 with bf16 rows out and an fp32 residual. The 128 x 128 kernel rounded the product to bf16 where it staged its tile and
    once more behind the residual: up to 1.54 of 2^-8 |ref| + 2e-3 in the first 60-second run of fuzz_wide.py (twenty cases, all of this
    epilogue, e.g. seed 130293: M 3662 N 64 K 896, fp32 residual; seed 130056: M 3871 N 1024 K 3584, table of 7 rows). Now the residual is
    added in fp32 in front of the one rounding, as the wide-tile kernel always did. Operands chosen so that every product and sum is exact in
    fp32 - small integers, times 2^-8 for the weights and 2^-10 for the residual - make the correct output unique: the fp32 value rounded to
    nearest even, bit for bit."""
    import torch

    from probpose_code_amd import _lib as L

    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-32, 33, (M, K), generator=g).float()
    w = torch.randint(-4, 5, (N, K), generator=g).float() * 2.0 ** -8
    r = torch.randint(-64, 65, (res_mod if res_mod else M, N), generator=g).float() * 2.0 ** -10
    exact = a.double() @ w.double().t() + (r.double()[torch.arange(M) % res_mod] if res_mod else r.double())
    assert torch.equal(exact.float().double(), exact) and float(exact.abs().max()) < 2.0 ** 10  # (an fp32 number: fp32 accumulation is exact as well)
    want = exact.float().bfloat16()
    twice = (((a.double() @ w.double().t()).float().bfloat16().float() + (r[torch.arange(M) % res_mod] if res_mod else r))).bfloat16()
    assert int((twice.view(torch.int16) != want.view(torch.int16)).sum()) > M * N // 100, "the operands do not tell one rounding from two"
    ad, wd, rd = a.bfloat16().cuda(), w.bfloat16().cuda(), r.cuda()
    out = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    L.reset_launch_counts()
    L.call("pp_gemm_ws", W.BF16, ad.data_ptr(), wd.data_ptr(), None, rd.data_ptr(), res_mod, out.data_ptr(), M, N, K, K, K, N, W.ACT_NONE, 1, 0, 1.0, None)
    torch.cuda.synchronize()
    assert L.launch_count(kernel) > 0 and W.gemm_kernel(W.BF16, M, N, K, 1, True) == kernel
    wrong = int((out.cpu().view(torch.int16) != want.view(torch.int16)).sum())
    print(f"bf16 rows + fp32 residual M {M} N {N} K {K} res_mod {res_mod} on {kernel}: {wrong} of {M * N} elements differ from the once-rounded value")
    assert wrong == 0


@pytest.mark.parametrize("seed", [130056, 130293, 130775])
def test_bf16_residual_cases_the_fuzzer_found(seed):
    """Three of the shapes and epilogues of the mismatches named above (classes as drawn there), under the fuzzer's tolerance."""
    M, N, K, epi, cls = {130056: (3871, 1024, 3584, dict(bias=True, act=0, fmt=1, res="table", res_mod=7), ("massive", "normal")),
                         130293: (3662, 64, 896, dict(bias=True, act=0, fmt=1, res="f32", res_mod=0), ("massive", "normal")),
                         130775: (6100, 3072, 1024, dict(bias=True, act=1, fmt=1, res="table", res_mod=1), ("massive", "normal"))}[seed]
    _report(*W.gemm_case(W.BF16, M, N, K, epi, seed, *cls))


def test_fuzz_of_the_wide_shapes():
    r = subprocess.run([sys.executable, os.path.join(HERE, "fuzz_wide.py"), "10"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "WIDE FUZZ OK" in r.stdout, (r.stdout[-3000:], r.stderr[-800:])
