"""GPU: the matrix entry points at the edges of what their argument checks admit, against fp64 (tests/fuzz_edges.py's grids case by case, then
its random draw for a few seconds). The other fuzzers draw their widths from the shipped models; here K is one K-tile, Cin one or three channel
blocks, maps 1 x 1, rows pitched - the narrow heads a config may ask for (deconv_out_channels is free).

  * pp_gemm_ws: the 128 x 128 kernel at K = 32 / 96 (f32, f16x3) and 64 / 192 (bf16), N = 32 and 17 (fp32 rows on a padded pitch), M = 1 and
    129, every epilogue kind; f16x3 on the wide-tile kernel at N = 192, K = 32 / 64 (fewer K-steps than ring stages) at its threshold and a
    row below; the twelve-wave kernel at K = 64; row pitches lda / ldw / ldc with the smallest padding each check admits (operand gaps hold
    NaN, output gaps are canaries).
  * pp_conv_gemm, 3x3 and deconvolution: f32 / f16x3 at Cin = 32 / 96, bf16 at Cin = 64, Cout 32 / 96, maps 1 x 1, 2 x 3, 16 x 12, groups 1 / 2,
    phases one at a time and all four; f16x3 on the wide-tile kernel at Cin = 32; bf16 rows out at Cin = 64 .. 160 on exactly 192 tiles.
  * pp_deconv_head / pp_deconv_head_split at Cin = 32 .. 160, 1 / 17 / 28 maps, 4 x 4 and 16 x 12 inputs.
  * pp_skinny_deconv at Cin = 32 .. 160, Cout = 32 / 96 / 256, maps 2 x 2, 3 x 5, 16 x 12, 1 and 8 images, every tile code that divides Cout.
  * pp_conv3x3_splitk with channel-range slices of one K-block; pp_skinny_linear / pp_skinny_conv1x1_planar at their smallest shapes.
Every case: canaries, every element written, inputs unchanged, a repeat launch bit-identical, the kernel the restated dispatcher predicts, and
error / tolerance <= 1 under the tolerances the other fuzzers already use. A refused shape is never skipped: it must be one fuzz_edges.REFUSED
lists (shapes the header puts outside the contract), refused with PP_ERR_UNSUPPORTED, with every buffer untouched."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fuzz_edges as E  # noqa: E402
import fuzz_wide as W  # noqa: E402

pytestmark = pytest.mark.gpu

P = E.PREC_NAME


def _report(faults, ratio, info):
    print(f"{info}: error / tolerance {ratio:.3g}")
    assert not faults, (info, faults)
    assert ratio <= 1.0, f"{info}: error / tolerance {ratio:.3g}"


# ------------------------------------------------------------------------------------------------- pp_gemm_ws
@pytest.mark.parametrize("i,case", list(enumerate(E.gemm_small_grid())),
                         ids=[f"{P[c[0]]}-M{c[1]}-N{c[2]}-K{c[3]}-{c[4]['res']}-act{c[4]['act']}-fmt{c[4]['fmt']}{'-planar' if c[6] else ''}"
                              for c in E.gemm_small_grid()])
def test_gemm_128_kernel_at_the_smallest_shapes(i, case):
    prec, M, N, K, epi, pad_c, planar = case
    _report(*E.gemm_edge_case(prec, M, N, K, epi, 9200 + i, pad_c=pad_c, planar_P=planar, kernel="pp_gemm.hip"))


def test_every_epilogue_kind_is_in_the_small_grid():
    for prec in (W.F32, W.F16X3, W.BF16):
        seen = {(c[4]["res"], c[4]["act"], bool(c[4]["bias"])) for c in E.gemm_small_grid() if c[0] == prec}
        assert {r for r, _, _ in seen} == {"none", "in_place", "f32", "table"} and {a for _, a, _ in seen} == {0, 1, 2} and {b for _, _, b in seen} == {True, False}
        assert {c[4]["fmt"] for c in E.gemm_small_grid() if c[0] == prec} == {0, W.OPERAND_FMT[prec]} and any(c[6] for c in E.gemm_small_grid() if c[0] == prec)


@pytest.mark.parametrize("M,N,K,kernel", E.gemm_wide_grid(), ids=[f"M{c[0]}-K{c[2]}-{c[3][:-4]}" for c in E.gemm_wide_grid()])
@pytest.mark.parametrize("fmt", [0, 2])
def test_gemm_wide_tile_kernel_with_fewer_k_steps_than_stages(fmt, M, N, K, kernel):
    epi = dict(bias=True, act=W.ACT_GELU if fmt else W.ACT_NONE, fmt=fmt, res="none" if fmt else "in_place", res_mod=0)
    _report(*E.gemm_edge_case(W.F16X3, M, N, K, epi, 9300 + K + fmt + M % 7, kernel=kernel))


@pytest.mark.parametrize("nst", [2, 3])
@pytest.mark.parametrize("K", [32, 64])
def test_gemm_wide_tile_kernel_ring_of_two_and_three_stages(K, nst):
    """Option "psplit_nst" pins the ring: 2 stages (256 x 192 tiles) or 3 (192 x 192). One and two K-steps on either."""
    from probpose_code_amd import _lib as L

    L.set_option("psplit_nst", nst)
    try:
        M = 256 * 191 + 1 if nst == 2 else 192 * 191 + 1  # 192 tiles of the pinned form
        epi = dict(bias=True, act=W.ACT_NONE, fmt=2, res="none", res_mod=0)
        ran = []
        faults, ratio, info = W.gemm_case(W.F16X3, M, 192, K, epi, 9350 + K + nst, e=None, ran=ran)
        faults = [f for f in faults if "restated dispatcher" not in f]  # (it restates the default options)
        _report(faults, ratio, f"psplit_nst {nst}: {info}")
        assert ran == ["pp_panel_split.hip"], ran
    finally:
        L.restore_options()


@pytest.mark.parametrize("M,N,K", E.gemm_dma_grid(), ids=[f"M{c[0]}" for c in E.gemm_dma_grid()])
@pytest.mark.parametrize("fmt", [0, 2])
def test_gemm_twelve_wave_kernel_at_two_k_steps(fmt, M, N, K):
    epi = dict(bias=True, act=W.ACT_GELU if fmt else W.ACT_NONE, fmt=fmt, res="none" if fmt else "in_place", res_mod=0)
    _report(*E.gemm_edge_case(W.F16X3, M, N, K, epi, 9400 + fmt + M % 7, kernel="linear_dma_tile"))


@pytest.mark.parametrize("i,case", list(enumerate(E.pitch_grid())),
                         ids=[f"{P[c[0]]}-M{c[1]}-N{c[2]}-K{c[3]}-fmt{c[4]}-lda+{c[5]}-ldw+{c[6]}-ldc+{c[7]}-{c[8]}-{c[9].replace('.hip', '')}" for c in E.pitch_grid()])
def test_gemm_row_pitches(i, case):
    prec, M, N, K, fmt, pa, pw, pc, res, kernel = case
    epi = dict(bias=True, act=W.ACT_NONE, fmt=fmt, res=res, res_mod=7 if res == "table" else 0)
    _report(*E.gemm_edge_case(prec, M, N, K, epi, 9500 + i, pa, pw, pc, kernel=kernel))


# ------------------------------------------------------------------------------------------------- pp_conv_gemm
@pytest.mark.parametrize("kind", [E.CONV3X3, E.DECONV], ids=["conv3x3", "deconv"])
@pytest.mark.parametrize("prec,cin", E.CONV_WIDTHS, ids=[f"{P[p]}-cin{c}" for p, c in E.CONV_WIDTHS])
def test_conv_gemm_at_narrow_widths_and_small_maps(prec, cin, kind):
    grid = E.conv_grid(prec, cin, kind)
    assert {c[3] for c in grid} == set(E.CONV_COUT) and {(c[1], c[2]) for c in grid} == set(E.CONV_MAPS)
    assert ({c[4] for c in grid} == {1, 2}) if kind == E.CONV3X3 else ({c[9] < 0 for c in grid} == {True, False})
    for i, (B, H, Wd, Cout, groups, fmt, act, bias, shared, phase, cls) in enumerate(grid):
        _report(*E.conv_edge_case(prec, kind, B, H, Wd, cin, Cout, groups, fmt, act, bias, shared, phase, cls, 9600 + 50 * kind + i + cin + prec,
                                  kernel="pp_gemm.hip"))


@pytest.mark.parametrize("kind,B,cout,groups,phase", E.conv_wide_grid(), ids=["conv3x3", "deconv"])
@pytest.mark.parametrize("fmt", [0, 2])
def test_conv_gemm_wide_tile_kernel_at_one_channel_block(fmt, kind, B, cout, groups, phase):
    _report(*E.conv_edge_case(W.F16X3, kind, B, 16, 12, 32, cout, groups, fmt, W.ACT_RELU, True, False, phase, "normal", 9700 + kind + fmt,
                              kernel="pp_panel_split.hip"))


@pytest.mark.parametrize("cin", E.BF16_DECONV_CIN)
def test_bf16_deconvolution_on_exactly_192_tiles(cin):
    """48 maps of 16 x 12, 256 channels out, four phases: pp_panel_gemm.hip takes Cin % 64 == 0; the widths between (a K-tile of 64 channels
    would straddle two taps) are refused by every bf16 kernel."""
    assert E.listed_refused("pp_conv_gemm", prec=W.BF16, Cin=cin) == (cin % 64 != 0)
    _report(*E.bf16_deconv_case(cin, 9800 + cin))


# ------------------------------------------------------------------------------------------------- the fused heads
@pytest.mark.parametrize("H,Wd", E.HEAD_MAPS, ids=["4x4", "16x12"])
@pytest.mark.parametrize("cin", E.HEAD_CIN)
def test_deconv_head_bf16_at_narrow_widths(cin, H, Wd):
    assert E.listed_refused("pp_deconv_head", Cin=cin) == (cin % 64 != 0)
    for K in E.HEAD_K:
        _report(*E.deconv_head_edge_case(False, cin, K, H, Wd, 9900 + cin + K + H))


@pytest.mark.parametrize("H,Wd", E.HEAD_MAPS, ids=["4x4", "16x12"])
@pytest.mark.parametrize("cin", E.HEAD_CIN)
def test_deconv_head_split_at_narrow_widths(cin, H, Wd):
    B = E.head_split_images(H, Wd)
    assert 4 * -(-B * H * Wd // 192) >= 192 > 4 * -(-(B - 1) * H * Wd // 192)
    for K in E.HEAD_K:
        _report(*E.deconv_head_edge_case(True, cin, K, H, Wd, 10000 + cin + K + H))


# ------------------------------------------------------------------------------------------------- the column-parallel kernels
@pytest.mark.parametrize("cout", E.SKINNY_DECONV_COUT)
@pytest.mark.parametrize("cin", E.SKINNY_DECONV_CIN)
def test_skinny_deconv_at_narrow_widths(cin, cout):
    codes = W.skinny_codes(cout, W.SKINNY_DECONV_CODES)
    assert codes == {32: [0, 11], 96: [0, 11], 256: [0, 11, 22, 12, 32]}[cout]
    assert E.listed_refused("pp_skinny_deconv", Cin=cin) == (cin == 32)
    for H, Wd in E.SKINNY_DECONV_MAPS:
        for nb in (1, 8):
            for code in codes:
                _report(*E.skinny_deconv_edge_case(cin, cout, H, Wd, nb, code, 10100 + cin + cout + H + nb))


@pytest.mark.parametrize("B,H,Wd,cin,cout,G,ks", E.splitk_grid(), ids=["cin64-2-slices", "cin128-4-slices"])
def test_splitk_channel_range_slices_of_one_k_block(B, H, Wd, cin, cout, G, ks):
    assert cin // ks == 32 and (cout // 192) * -(-B * H * Wd // 256) * G * ks >= 192 > (cout // 192) * -(-(B - 1) * H * Wd // 256) * G * ks
    _report(*E.splitk_edge_case(B, H, Wd, cin, cout, G, ks, 10200 + cin))


@pytest.mark.parametrize("name,case", E.skinny_pins(), ids=[n for n, _ in E.skinny_pins()])
def test_skinny_linear_and_conv1x1_at_their_smallest_shapes(name, case):
    _report(*case())


def test_fuzz_of_the_contract_edges():
    r = subprocess.run([sys.executable, os.path.join(HERE, "fuzz_edges.py"), "10"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "EDGES FUZZ OK" in r.stdout, (r.stdout[-3000:], r.stderr[-800:])
