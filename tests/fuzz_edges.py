#!/usr/bin/env python
"""The matrix entry points at the EDGES of what their argument checks admit, against torch fp64: the smallest and most awkward shapes each check
in csrc/ lets through - one K-tile, Cin of one or three channel blocks, 1 x 1 maps, one output map, padded row pitches - where the other fuzzers
draw their widths from the shipped models (64 .. 1280 channels, K >= 64, dense rows). The single cases and every tolerance are the other
fuzzers' own (fuzz_wide.gemm_case / skinny_case / deconv_case / skinny_deconv_case, fuzz_conv.conv_gemm_case / deconv_head_case,
fuzz_head.deconv_head_split_case / splitk_case; bars scaled by magnitude_factor as fuzz_wide.py documents); each asserts canaries bit for bit,
every element written, inputs unchanged, a repeat launch bit-identical, pp_launch_count naming the kernel the restated dispatcher predicts, and
error / tolerance <= 1. The grids below are what tests/test_contract_edges_gpu.py runs case by case; ``python tests/fuzz_edges.py [seconds]``
draws random combinations from the same sets.

A shape the library refuses passes only if REFUSED names it - shapes include/probpose_mi355x.h puts outside the contract - and then the
refusal must be PP_ERR_UNSUPPORTED with every canary, output element and input untouched (``checked``). A shape REFUSED names that is
accepted fails as well."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuzz_conv as FC  # noqa: E402
import fuzz_head as FH  # noqa: E402
import fuzz_wide as W  # noqa: E402
from fuzz_layer import BF16, F16X3, F32, TOL, Guard, Refused, cpu_rand, error_ratio, run_entries, run_twice  # noqa: E402

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
CONV3X3, DECONV = FC.CONV3X3, FC.DECONV
PREC_NAME = W.PREC_NAME
OPERAND_FMT = W.OPERAND_FMT

# (entry point, what names the shape, the sentence of include/probpose_mi355x.h that puts it outside the contract)
REFUSED = [
    ("pp_skinny_deconv", dict(Cin=32), "pp_skinny_deconv: Cin % 32 == 0 and Cin >= 64"),
    ("pp_deconv_head", dict(Cin=32), "pp_deconv_head: Cin % 64 == 0"),
    ("pp_deconv_head", dict(Cin=96), "pp_deconv_head: Cin % 64 == 0"),
    ("pp_deconv_head", dict(Cin=160), "pp_deconv_head: Cin % 64 == 0"),
    ("pp_conv_gemm", dict(prec=BF16, Cin=96), "pp_conv_gemm: Cin a multiple of the K-tile, 64 channels in bf16"),
    ("pp_conv_gemm", dict(prec=BF16, Cin=160), "pp_conv_gemm: Cin a multiple of the K-tile, 64 channels in bf16"),
]


def listed_refused(entry, **shape):
    return any(e == entry and all(shape.get(k) == v for k, v in want.items()) for e, want, _ in REFUSED)


def checked(entry, shape, fn):
    """fn() -> (faults, error / tolerance, description). A refusal is a fault unless REFUSED lists the shape; a listed shape must be refused with
    PP_ERR_UNSUPPORTED and leave every buffer as it was."""
    listed = listed_refused(entry, **shape)
    try:
        faults, ratio, info = fn()
    except Refused as exc:
        info = f"{entry} {shape}: refused"
        if not listed:
            return [f"refused, and REFUSED does not list the shape: {exc}"], 0.0, info
        faults = list(getattr(exc, "faults", ["the refusing case did not check its buffers"]))
        if "UNSUPPORTED" not in str(exc):
            faults.append(f"refused, but not with PP_ERR_UNSUPPORTED: {exc}")
        return faults, 0.0, info + " as listed"
    return (faults + ["accepted, though REFUSED lists the shape"]) if listed else faults, ratio, info


# ----------------------------------------------------------------------------------------------------- pp_gemm_ws
def epilogues(prec):
    """Every epilogue kind once: bias or none, the three activations, no residual / in place / separate rows / broadcast table, fp32 or
    operand-format rows out."""
    op = OPERAND_FMT[prec]
    return [dict(bias=True, act=ACT_NONE, fmt=op, res="none", res_mod=0), dict(bias=False, act=ACT_GELU, fmt=0, res="none", res_mod=0),
            dict(bias=True, act=ACT_RELU, fmt=0, res="in_place", res_mod=0), dict(bias=True, act=ACT_NONE, fmt=op, res="f32", res_mod=0),
            dict(bias=True, act=ACT_GELU, fmt=0, res="table", res_mod=7), dict(bias=False, act=ACT_NONE, fmt=0, res="f32", res_mod=0)]


GEMM_K = {F32: (32, 96), F16X3: (32, 96), BF16: (64, 192)}  # one K-tile (the double buffer's prologue is its last step), and three


def gemm_small_grid():
    """The 128 x 128 kernel: (precision, M, N, K, epilogue, pad_c, planar_P). N = 17: fp32 rows out on the smallest pitch the check admits (20)."""
    out = []
    for prec in (F32, F16X3, BF16):
        i = 0
        for K in GEMM_K[prec]:
            for N in (32, 17):
                for M in (1, 129):
                    epi = dict(epilogues(prec)[i % 6])
                    i += 1
                    if N == 17:
                        epi["fmt"] = 0
                    out.append((prec, M, N, K, epi, 3 if N == 17 else 0, 0))
        # the epilogues the eight cases above did not reach, and planar planes (the final 1x1 convolution's layout: fp32 only)
        out.append((prec, 129, 32, GEMM_K[prec][0], epilogues(prec)[2], 0, 0))
        out.append((prec, 129, 32, GEMM_K[prec][1], epilogues(prec)[3], 0, 0))
        out.append((prec, 129, 17, GEMM_K[prec][0], dict(bias=True, act=ACT_NONE, fmt=0, res="none", res_mod=0), 0, 43))
    return out


def gemm_wide_grid():
    """f16x3 on the wide-tile kernel with fewer K-steps than its ring has stages (K = 32, 64 on 2 / 3 stages), M at the kernel's threshold and
    one row below it (the 128 x 128 kernel): (M, N, K, kernel)."""
    out = []
    for K in (32, 64):
        t = W.wide_threshold(192, K=K)
        out += [(t, 192, K, "pp_panel_split.hip"), (t - 1, 192, K, "pp_gemm.hip")]
    return out


def gemm_dma_grid():
    """The twelve-wave kernel at K = 64 - two stages, its stated minimum, on a ring of three: (M, N, K)."""
    t = W.dma_threshold(192)
    return [(t, 192, 64), (t + 100, 192, 64)]


def pitch_grid():
    """Row pitches lda = K + a, ldw = K + a, ldc = N + a with the smallest a each check admits: (precision, M, N, K, fmt, pad_a, pad_w, pad_c,
    residual kind, kernel). The operands' gap columns hold NaN, the output's are canaries."""
    out = []
    for prec, K, pa in ((F32, 96, 8), (F16X3, 96, 32), (BF16, 192, 8)):
        op = OPERAND_FMT[prec]
        pc_op = {0: 4, 1: 8, 2: 32}[op]
        out += [(prec, 129, 96, K, 0, pa, pa, 4, "none", "pp_gemm.hip"), (prec, 129, 96, K, op, pa, pa, pc_op, "none", "pp_gemm.hip"),
                (prec, 129, 96, K, 0, pa, 0, 0, "none", "pp_gemm.hip"), (prec, 129, 96, K, 0, 0, pa, 4, "in_place", "pp_gemm.hip"),
                (prec, 1, 17, K, 0, pa, pa, 3, "table", "pp_gemm.hip")]
    t = W.wide_threshold(192, K=64)
    out += [(F16X3, t, 192, 64, 0, 32, 32, 32, "in_place", "pp_panel_split.hip"), (F16X3, t, 192, 64, 2, 32, 32, 32, "none", "pp_panel_split.hip"),
            # fp32 rows on a pitch the wide-tile kernel does not take (ldc % 32 != 0): the 128 x 128 kernel
            (F16X3, t, 192, 64, 0, 32, 32, 4, "none", "pp_gemm.hip"),
            # enough tiles for the twelve-wave kernel, which takes dense operands only: the wide-tile kernel
            (F16X3, W.dma_threshold(192), 192, 64, 2, 32, 0, 0, "none", "pp_panel_split.hip")]
    tb = W.wide_threshold(192, BF16, 768, 0)
    out += [(BF16, tb, 192, 768, 0, 8, 8, 8, "f32", "pp_panel_split.hip")]
    return out


def gemm_edge_case(prec, M, N, K, epi, seed, pad_a=0, pad_w=0, pad_c=0, planar_P=0, kernel=None):
    ran = []
    cls = W.CLASSES[seed % 3], W.CLASSES[(seed // 3) % 3]
    cls = (cls[0], "massive") if cls == ("offset", "offset") else cls
    faults, ratio, info = checked("pp_gemm_ws", dict(prec=prec, M=M, N=N, K=K), lambda: W.gemm_case(
        prec, M, N, K, epi, seed, cls[0], cls[1], e=None, planar_P=planar_P, ran=ran, pad_a=pad_a, pad_w=pad_w, pad_c=pad_c))
    if kernel is not None and ran != [kernel]:
        faults = faults + [f"kernel {ran}, the grid names {kernel}"]
    return faults, ratio, info


# ----------------------------------------------------------------------------------------------------- pp_conv_gemm
CONV_WIDTHS = [(F32, 32), (F32, 96), (F16X3, 32), (F16X3, 96), (BF16, 64)]
CONV_COUT = (32, 96)
CONV_MAPS = ((1, 1), (2, 3), (16, 12))


def conv_grid(prec, Cin, kind):
    """(B, H, W, Cout, groups, fmt, act, bias, shared, phase, class) over Cout x maps x (groups 1 and 2 | phases one at a time and all four)."""
    fmts = {BF16: [0, 1], F32: [0], F16X3: [0, 2]}[prec]
    out, i = [], 0
    for Cout in CONV_COUT:
        for H, Wd in CONV_MAPS:
            for v in (0, 1):
                i += 1
                cls = ("normal", "massive", "border")[i % 3] if H * Wd > 1 else "normal"
                groups, phase = (1 + v, 0) if kind == CONV3X3 else (1, (i % 4) if v == 0 else -1)
                out.append((2, H, Wd, Cout, groups, fmts[i % len(fmts)], i % 3, i % 4 != 0, kind == CONV3X3 and groups == 2 and i % 2 == 0, phase, cls))
    return out


def conv_edge_case(prec, kind, B, H, Wd, Cin, Cout, groups, fmt, act, bias, shared, phase, cls, seed, kernel=None):
    rng, g = np.random.default_rng(seed), torch.Generator().manual_seed(seed)
    ran = []
    faults, ratio, info = checked("pp_conv_gemm", dict(prec=prec, Cin=Cin), lambda: FC.conv_gemm_case(
        prec, kind, B, H, Wd, Cin, Cout, groups, fmt, act, bias, shared, phase, cls, dict(FC.DEFAULT_OPTIONS), "none", rng, g, kernels=ran))
    if kernel is not None and ran and ran != [kernel]:
        faults = faults + [f"kernel {ran}, the grid names {kernel}"]
    return faults, ratio, info


def conv_wide_grid():
    """f16x3 on the wide-tile kernel at Cin = 32 with just enough pixels for 192 tiles: (kind, B, Cout, groups, phase). 3x3: four problems of
    63 maps of 16 x 12 (48 tiles of 256 pixels each); deconvolution: the four phases of 48 maps (48 tiles of 192 pixels each)."""
    return [(CONV3X3, 63, 192, 4, 0), (DECONV, 48, 256, 1, -1)]


BF16_DECONV_CIN = (64, 96, 128, 160)  # bf16 rows out, Cout 256, 48 maps of 16 x 12, four phases: exactly 192 tiles for pp_panel_gemm.hip


def bf16_deconv_case(Cin, seed):
    ran = []
    faults, ratio, info = checked("pp_conv_gemm", dict(prec=BF16, Cin=Cin), lambda: W.deconv_case(BF16, Cin, 48, -1, seed, fmt=1, ran=ran))
    if ran and ran != ["pp_panel_gemm.hip"]:
        faults = faults + [f"kernel {ran}, the grid names pp_panel_gemm.hip"]
    return faults, ratio, info


# ----------------------------------------------------------------------------------------------------- the fused heads
HEAD_CIN = (32, 64, 96, 128, 160)
HEAD_K = (1, 17, 28)
HEAD_MAPS = ((4, 4), (16, 12))


def head_split_images(H, Wd):
    """Smallest image count at which pp_deconv_head_split has its 192 tiles: 4 ceil(B H W / 192) >= 192."""
    return math.ceil((47 * 192 + 1) / (H * Wd))


def deconv_head_edge_case(split, Cin, K, H, Wd, seed):
    rng, g = np.random.default_rng(seed), torch.Generator().manual_seed(seed)
    if split:
        return checked("pp_deconv_head_split", dict(Cin=Cin), lambda: FH.deconv_head_split_case(head_split_images(H, Wd), H, Wd, Cin, K, rng, g))
    cls = ("normal", "massive", "border")[seed % 3]
    return checked("pp_deconv_head", dict(Cin=Cin), lambda: FC.deconv_head_case(2, H, Wd, Cin, K, cls, rng, g))


# ----------------------------------------------------------------------------------------------------- the column-parallel kernels
SKINNY_DECONV_CIN = (32, 64, 96, 160)
SKINNY_DECONV_COUT = (32, 96, 256)
SKINNY_DECONV_MAPS = ((2, 2), (3, 5), (16, 12))


def skinny_deconv_edge_case(Cin, Cout, H, Wd, nb, code, seed):
    cls = ("normal", "border", "massive")[seed % 3]
    return checked("pp_skinny_deconv", dict(Cin=Cin), lambda: W.skinny_deconv_case(Cin, nb, code, seed, cls=cls, H=H, W=Wd, cout=Cout))


def splitk_grid():
    """Channel-range slices of ONE K-block each (f16x3, the wide-tile kernel only): (B, H, W, Cin, Cout, towers, slices), B the smallest batch with
    192 tiles of 256 pixels x 192 channels over towers x slices."""
    return [(369, 4, 4, 64, 192, 4, 2), (177, 4, 4, 128, 192, 4, 4)]


def splitk_edge_case(B, H, Wd, Cin, Cout, G, ks, seed):
    from probpose_code_amd import _lib as L

    rng, g = np.random.default_rng(seed), torch.Generator().manual_seed(seed)
    L.reset_launch_counts()
    faults, ratio, info = checked("pp_conv3x3_splitk", dict(Cin=Cin, ks=ks), lambda: FH.splitk_case(B, H, Wd, Cin, Cout, G, ks, rng, g))
    got = [k for k in FC.KERNELS if L.launch_count(k) > 0]
    if got != ["pp_panel_split.hip", "pp_head.hip"]:
        faults = faults + [f"kernels {got}: channel-range slices belong to pp_panel_split.hip"]
    return faults, ratio, info


def conv1x1_planar_case(n_img, P, K, nv, seed):
    """pp_skinny_conv1x1_planar against fp64 under tests/fuzz_skinny.py's bar for it (3e-5 = TOL["linear_long"], unit-normal rows)."""
    from probpose_code_amd import _lib as L
    from probpose_code_amd.weights import to_split

    g = torch.Generator().manual_seed(seed)
    x, wt, b = cpu_rand(n_img * P, K, g=g), cpu_rand(nv, K, g=g, scale=1 / math.sqrt(K)), cpu_rand(nv, g=g, scale=0.3)
    rows = 32 * ((nv + 31) // 32)
    wp, bp = torch.zeros(rows, K), torch.zeros(rows)
    wp[:nv], bp[:nv] = wt, b
    guard = Guard()
    xd, wd, bd = guard.inp("act", to_split(x)), guard.inp("weight", to_split(wp)), guard.inp("bias", bp)
    out = guard.out("out", (n_img, nv, P))

    def go():
        W._launch(L, "pp_skinny_conv1x1_planar", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), n_img, P, K, nv, 1.0, None)

    L.reset_launch_counts()
    faults, snap = run_twice(guard, go)
    if L.launch_count("skinny_conv1x1") != 2:
        faults.append(f"pp_launch_count('skinny_conv1x1') = {L.launch_count('skinny_conv1x1')} after two launches")
    ref = (x.double() @ wt.double().t() + b.double()).view(n_img, P, nv).permute(0, 2, 1)
    return faults, error_ratio(snap[0].cpu(), ref, TOL["linear_long"], TOL["linear_long"]), f"conv1x1 planar n_img {n_img} P {P} K {K} n_valid {nv}"


def skinny_pins():
    """Shapes of tests/fuzz_skinny.py's random draw, pinned: the smallest Linear layer, the LayerNorm tail at its narrowest, one output map of one pixel."""
    return [("linear", lambda: W.skinny_case((32, 64, "qkv"), 1, W.skinny_codes(32), 0, 9101, e=None)),
            ("linear-gelu", lambda: W.skinny_case((32, 64, "fc1"), 33, W.skinny_codes(32), 1, 9102, e=None)),
            ("ln-tail-n64", lambda: W.skinny_case((64, 64, "proj"), 1, W.skinny_codes(64), 0, 9103, e=None)),
            ("ln-tail-n64-table", lambda: W.skinny_case((64, 64, "patch"), 33, W.skinny_codes(64), 1, 9104, e=None)),
            ("conv1x1-one-map-one-pixel", lambda: conv1x1_planar_case(1, 1, 64, 1, 9105)),
            ("conv1x1-17-maps", lambda: conv1x1_planar_case(2, 5, 64, 17, 9106))]


# ----------------------------------------------------------------------------------------------------- the fuzzer
def _main(seconds):
    from probpose_code_amd import _lib as L

    def one(seq, rng):
        return seq[int(rng.integers(0, len(seq)))]

    def case_gemm(rng, g):
        prec = one((F32, F16X3, BF16), rng)
        epi = dict(one(epilogues(prec), rng))
        M, N, K = one((1, 2, 127, 128, 129, 257), rng), one((32, 17, 96, 8), rng), one(GEMM_K[prec], rng)
        pa = {F32: 8, F16X3: 32, BF16: 8}[prec] * int(rng.integers(0, 2))
        pw = {F32: 8, F16X3: 32, BF16: 8}[prec] * int(rng.integers(0, 2))
        if N % 32 != 0 and epi["fmt"] == 2 or N % 8 != 0 and epi["fmt"] == 1:
            epi["fmt"] = 0
        unit = {0: 4, 1: 8, 2: 32}[epi["fmt"]]
        pc = (-N) % unit + unit * int(rng.integers(0, 2))
        return gemm_edge_case(prec, M, N, K, epi, int(rng.integers(1 << 30)), pa, pw, pc)

    def case_gemm_wide(rng, g):
        K = one((32, 64), rng)
        fmt = one((0, 2), rng)
        pad = 32 * int(rng.integers(0, 2))
        M = W.wide_threshold(192, K=K) - int(rng.integers(0, 2))
        epi = dict(bias=rng.random() < 0.7, act=int(rng.integers(0, 3)), fmt=fmt, res="none" if fmt else one(("none", "in_place", "table"), rng), res_mod=0)
        epi["res_mod"] = 7 if epi["res"] == "table" else 0
        return gemm_edge_case(F16X3, M, 192, K, epi, int(rng.integers(1 << 30)), pad, pad, pad)

    def case_conv(rng, g):
        prec, Cin = one(CONV_WIDTHS + [(BF16, 96)], rng)
        kind = one((CONV3X3, DECONV), rng)
        grid = conv_grid(prec, 64 if (prec, Cin) == (BF16, 96) else Cin, kind)
        B, H, Wd, Cout, groups, fmt, act, bias, shared, phase, cls = one(grid, rng)
        return conv_edge_case(prec, kind, int(rng.integers(1, 4)), H, Wd, Cin, Cout, groups, fmt, int(rng.integers(0, 3)), bias, shared, phase, cls,
                              int(rng.integers(1 << 30)))

    def case_head(split):
        def run(rng, g):
            H, Wd = one(HEAD_MAPS, rng)
            return deconv_head_edge_case(split, one(HEAD_CIN, rng), one(HEAD_K, rng), H, Wd, int(rng.integers(1 << 30)))
        return run

    def case_skinny_deconv(rng, g):
        Cin, Cout = one(SKINNY_DECONV_CIN, rng), one(SKINNY_DECONV_COUT, rng)
        H, Wd = one(SKINNY_DECONV_MAPS, rng)
        return skinny_deconv_edge_case(Cin, Cout, H, Wd, one((1, 8), rng), one(W.skinny_codes(Cout, W.SKINNY_DECONV_CODES), rng), int(rng.integers(1 << 30)))

    def case_pins(rng, g):
        return one(skinny_pins(), rng)[1]()

    entries = [("pp_gemm_ws (128 x 128, pitches)", case_gemm), ("pp_gemm_ws (wide tile, K = 32 / 64)", case_gemm_wide), ("pp_conv_gemm", case_conv),
               ("pp_deconv_head", case_head(False)), ("pp_deconv_head_split", case_head(True)), ("pp_skinny_deconv", case_skinny_deconv),
               ("pp_skinny_linear / conv1x1 (pins)", case_pins)]
    return run_entries(entries, seconds, 150000, "EDGES", L)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sys.exit(_main(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0))


if __name__ == "__main__":
    main()
