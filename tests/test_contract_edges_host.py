"""CPU: the shapes tests/fuzz_edges.py lists as refused are refused by the real library with PP_ERR_UNSUPPORTED (the argument checks run in front
of every HIP call: dummy non-NULL pointers are never dereferenced), the header says so, and the restated dispatchers of tests/fuzz_conv.py and
tests/fuzz_wide.py agree with the checks of csrc/: pp_skinny_deconv needs a stage of two 32-channel blocks within one tap's Cin / 32 blocks
(Cin >= 64), the wide-tile bf16 kernel of pp_panel_gemm.hip - and pp_deconv_head, which is that kernel - stages of 64 channels of one tap
(Cin % 64 == 0), and no bf16 kernel takes a convolution whose Cin is no multiple of its K-tile of 64 channels."""
import ctypes
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import fuzz_conv as FC  # noqa: E402
import fuzz_edges as E  # noqa: E402
import fuzz_wide as W  # noqa: E402


@pytest.fixture()
def lib(lib_built):
    from probpose_code_amd import _lib

    buf = ctypes.create_string_buffer(64)
    return _lib, ctypes.addressof(buf), buf  # (buf keeps the address alive; it is never dereferenced: the checks fail first)


def _unsupported(_lib, status, word):
    assert status == _lib.PP_ERR_UNSUPPORTED, (status, _lib.lib.pp_last_error())
    assert word.encode() in _lib.lib.pp_last_error(), _lib.lib.pp_last_error()


@pytest.mark.parametrize("B,H,W,cout", [(1, 32, 24, 256), (1, 2, 2, 32), (8, 16, 12, 96)])
def test_skinny_deconv_refuses_one_channel_block(lib, B, H, W, cout):
    _lib, p, _ = lib
    _unsupported(_lib, _lib.lib.pp_skinny_deconv(p, p, p, p, B, H, W, 32, cout, None), "Cin >= 64")
    # a multiple of 32 is still required
    _unsupported(_lib, _lib.lib.pp_skinny_deconv(p, p, p, p, B, H, W, 80, cout, None), "Cin % 32 == 0")


@pytest.mark.parametrize("cin", [32, 96, 160])
@pytest.mark.parametrize("B,H,W,K", [(2, 4, 4, 1), (8, 32, 24, 17), (48, 16, 12, 28)])
def test_deconv_head_refuses_half_stages(lib, cin, B, H, W, K):
    _lib, p, _ = lib
    _unsupported(_lib, _lib.lib.pp_deconv_head(p, p, p, p, p, p, B, H, W, cin, 256, K, None), "Cin % 64 == 0")


@pytest.mark.parametrize("cin", [96, 160])
@pytest.mark.parametrize("B,py", [(48, -1), (192, 0), (1, -1)])
def test_bf16_deconvolution_refuses_half_k_tiles_at_every_tile_count(lib, cin, B, py):
    """48 maps x four phases (192 one-phase maps) are the 192 tiles from which pp_panel_gemm.hip took bf16 rows out; below, the 128 x 128 kernel
    always refused a Cin that is no multiple of its K-tile. Now every tile count answers alike."""
    _lib, p, _ = lib
    st = _lib.lib.pp_conv_gemm(W.BF16, W.DECONV, p, p, p, p, B, 16, 12, cin, 256, py, 0, 1, 0, 0, 0, 0, 256, W.ACT_RELU, 1, None)
    _unsupported(_lib, st, "K-tile")
    assert FC.conv_kernel(W.BF16, W.DECONV, B, 16, 12, cin, 256, 4 if py < 0 else 1, 1, W.ACT_RELU, FC.DEFAULT_OPTIONS) == "refused"


def test_every_listed_refusal_is_in_the_header_and_in_the_library(lib):
    _lib, p, _ = lib
    header = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "probpose_mi355x.h")).read())
    for phrase in ("Cin % 32 == 0 and Cin >= 64", "Cin % 64 == 0 (the kernel's stages are 64 channels of one tap)",
                   "precision's K-tile - 64 channels (bf16), 32 (fp32, split fp16)"):
        assert phrase in header, phrase
    for entry, shape, _ in E.REFUSED:
        cin = shape["Cin"]
        if entry == "pp_skinny_deconv":
            st = _lib.lib.pp_skinny_deconv(p, p, p, p, 1, 16, 12, cin, 256, None)
        elif entry == "pp_deconv_head":
            st = _lib.lib.pp_deconv_head(p, p, p, p, p, p, 2, 16, 12, cin, 256, 17, None)
        else:
            assert entry == "pp_conv_gemm" and shape["prec"] == W.BF16
            st = _lib.lib.pp_conv_gemm(W.BF16, W.DECONV, p, p, p, p, 48, 16, 12, cin, 256, -1, 0, 1, 0, 0, 0, 0, 256, W.ACT_RELU, 1, None)
        assert st == _lib.PP_ERR_UNSUPPORTED, (entry, shape, _lib.lib.pp_last_error())
    # ... and the list names nothing the grids do not hold, and no width the checks admit
    assert {s["Cin"] for e, s, _ in E.REFUSED if e == "pp_skinny_deconv"} == {c for c in E.SKINNY_DECONV_CIN if c < 64}
    assert {s["Cin"] for e, s, _ in E.REFUSED if e == "pp_deconv_head"} == {c for c in E.HEAD_CIN if c % 64}
    assert {s["Cin"] for e, s, _ in E.REFUSED if e == "pp_conv_gemm"} == {c for c in E.BF16_DECONV_CIN if c % 64}
    assert not any(E.listed_refused("pp_conv_gemm", prec=prec, Cin=cin) for prec, cin in E.CONV_WIDTHS)
    assert not any(E.listed_refused("pp_deconv_head_split", Cin=cin) for cin in E.HEAD_CIN)


def test_restated_conv_dispatchers_follow_the_tightened_checks():
    opt = FC.DEFAULT_OPTIONS
    for cin, want in ((64, "pp_panel_gemm.hip"), (128, "pp_panel_gemm.hip"), (96, "refused"), (160, "refused")):
        assert FC.conv_kernel(W.BF16, W.DECONV, 48, 16, 12, cin, 256, 4, 1, W.ACT_RELU, opt) == want
        assert FC.conv_kernel(W.BF16, W.DECONV, 47, 16, 12, cin, 256, 4, 1, W.ACT_RELU, opt) == ("refused" if cin % 64 else "pp_gemm.hip")
    # f32 / f16x3: one K-tile of 32 channels; the wide-tile split kernel from 192 tiles on at Cin = 32
    assert FC.conv_kernel(W.F32, W.DECONV, 48, 16, 12, 32, 256, 4, 0, W.ACT_RELU, opt) == "pp_gemm.hip"
    assert FC.conv_kernel(W.F16X3, W.DECONV, 48, 16, 12, 32, 256, 4, 2, W.ACT_RELU, opt) == "pp_panel_split.hip"
    assert FC.conv_kernel(W.F16X3, W.DECONV, 47, 16, 12, 32, 256, 4, 2, W.ACT_RELU, opt) == "pp_gemm.hip"
    assert FC.conv_kernel(W.F16X3, FC.CONV3X3, 63, 16, 12, 32, 192, 4, 2, W.ACT_RELU, opt) == "pp_panel_split.hip"
    assert FC.conv_kernel(W.F16X3, FC.CONV3X3, 62, 16, 12, 32, 192, 4, 2, W.ACT_RELU, opt) == "pp_gemm.hip"
    assert FC.conv_kernel(W.F16X3, W.DECONV, 48, 16, 12, 48, 256, 4, 2, W.ACT_RELU, opt) == "refused"
    # whole-tap split-K on the wide-tile bf16 kernel: stages of 64 channels as well (9 Cin / ks % 128 == 0 implies it for ks = 1, 3, 9)
    assert FC.splitk_kernel(W.BF16, 128, 4, 4, 384, 384, 4, 3, opt) == "pp_panel_gemm.hip"
    assert FC.splitk_kernel(W.BF16, 512, 4, 4, 96, 192, 4, 3, opt) == "pp_gemm.hip"


def test_restated_linear_dispatcher_knows_the_row_pitches():
    t, d = W.wide_threshold(192, K=64), W.dma_threshold(192)
    assert (t, W.wide_threshold(192, K=32), d) == (192 * 191 + 1, 192 * 191 + 1, 192 * 511 + 1)
    assert W.gemm_kernel(W.F16X3, t, 192, 64, 0, True) == W.gemm_kernel(W.F16X3, t, 192, 64, 0, True, lda=96, ldw=96, ldc=224) == "pp_panel_split.hip"
    assert W.gemm_kernel(W.F16X3, t - 1, 192, 64, 0, True, lda=96, ldw=96, ldc=224) == "pp_gemm.hip"
    assert W.gemm_kernel(W.F16X3, t, 192, 64, 0, False, ldc=196) == "pp_gemm.hip"      # the wide-tile kernel wants ldc % 32 == 0
    assert W.gemm_kernel(W.F16X3, t, 192, 32, 2, False) == "pp_panel_split.hip"       # one K-step
    assert W.gemm_kernel(W.F16X3, d, 192, 64, 2, False) == "linear_dma_tile" and W.gemm_kernel(W.F16X3, d, 192, 32, 2, False) == "pp_panel_split.hip"
    for pitched in (dict(lda=96), dict(ldw=96), dict(ldc=224)):                        # the twelve-wave kernel takes dense operands only
        assert W.gemm_kernel(W.F16X3, d, 192, 64, 2, False, **pitched) == "pp_panel_split.hip"
    tb = W.wide_threshold(192, W.BF16, 768, 0)
    assert W.gemm_kernel(W.BF16, tb, 192, 768, 0, True, lda=776, ldw=776, ldc=200) == "pp_panel_split.hip"
    # the grids name the kernel each pitched case lands on; the restatement must agree with them
    for prec, M, N, K, fmt, pa, pw, pc, res, kernel in E.pitch_grid():
        assert W.gemm_kernel(prec, M, N, K, fmt, res != "none", False, K + pa, K + pw, N + pc) == kernel, (prec, M, N, K, fmt, pa, pw, pc)
    for M, N, K, kernel in E.gemm_wide_grid():
        assert W.gemm_kernel(W.F16X3, M, N, K, 2, False) == W.gemm_kernel(W.F16X3, M, N, K, 0, True) == kernel
    for M, N, K in E.gemm_dma_grid():
        assert W.gemm_kernel(W.F16X3, M, N, K, 2, False) == W.gemm_kernel(W.F16X3, M, N, K, 0, True) == "linear_dma_tile"
    for prec, M, N, K, epi, pad_c, planar in E.gemm_small_grid():
        assert W.gemm_kernel(prec, M, N, K, epi["fmt"], epi["res"] != "none", bool(planar), ldc=N + pad_c) == "pp_gemm.hip"
