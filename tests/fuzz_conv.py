#!/usr/bin/env python
"""Fuzz of the convolution, pooling and elementwise kernels of the heatmap branch and the scalar towers against torch fp64, visited round robin:
pp_conv_gemm (PP_CONV3X3 with groups 1 - 4, shared or separate inputs, bias / none, act none / ReLU / GELU, every admitted output format;
PP_DECONV4X4S2 as the four single phases and as all four in one launch) in bf16 / fp32 / f16x3, pp_conv3x3_splitk (slices 1 / 3 / 9) +
pp_sum_maxpool_relu_nhwc in bf16 / fp32, the bf16 pp_conv3x3_maxpool_relu and pp_deconv_head, pp_maxpool_relu_nhwc (every admitted format pair,
windows that do not divide the map), pp_preproc_im2col (uint8 / fp32 input, pad 0 - 3, one or two passes, three output formats) and
pp_layernorm (E 384 / 768 / 1024 / 1280, the row classes of tests/fuzz_layer.py).

Shapes: the engine's own maps (ViT-S 16 x 12 x 384, ViT-B 24 x 18 x 768, the tower stages 4 x 4, 6 x 6, 3 x 3, 2 x 2) and random ones down to 1 x 1.
The dispatcher's predicates (panel_split_supported, conv_halo_supported, panel_gemm_supported, then the 128 x 128 kernel) are mirrored below;
B is drawn so that the tile count lands on both sides of 192 for each kernel, one of the steering options is set per case, and the launch
counters (pp_launch_count) record which kernel really ran: a kernel other than the mirror's prediction is a mismatch, and a cell of the
(entry, precision, kind) x kernel table the chosen shapes must reach that stays empty fails the run.

Values: unit normal; massive channels (tests/fuzz_layer.py MASSIVE); border impulses (every image zero but a few pixels on its first / last rows
and columns, of about 8: a read across an image boundary or a missing zero pad is off by orders of magnitude more than the tolerance); and, for
the pooling entries, non-finite poison (+inf, -inf, canonical NaN; the contract and its checks: tests/fuzz_head.py, poison_ratio).
Every case: outputs and partial sums between canaries (bit for bit), every element written, inputs bit-identical after the launch, a repeat
launch bit-identical, fp64 accuracy:
  * f16x3: tests/fuzz_head.py TOL, scaled by the operands' magnitude (tests/fuzz_layer.py magnitude_factor);
  * fp32: 2e-4 (tests/fuzz_gemm.py);
  * bf16: against fp64 on the bf16-rounded operands, 2e-3 for fp32 output, 2^-8 |ref| + 2e-3 for bf16 output (one rounding of the result);
  * im2col: fp32 output within 2 ulp of the fp64 (x - mean) / std; bf16 and split output the correctly rounded value of the fp32 result;
  * LayerNorm: fuzz_layer.TOL["gemm_ln"] for fp32 / split output (times ln_factor of the rows), the bf16 rule for bf16 output.
Refusals (UNSUPPORTED / INVALID_ARG) are counted; shapes stay inside the documented constraints and MEM_CAP.   python tests/fuzz_conv.py [seconds]"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from fuzz_head import TOL as HEAD_TOL  # noqa: E402
from fuzz_head import bad_pixels, conv3x3_64, conv_reach, deconv_phases, poison_, poison_ratio, run_guarded  # noqa: E402
from fuzz_layer import (BF16, F16X3, F32, MASSIVE, MEM_CAP, SPLIT, Guard, Refused, cpu_rand, error_ratio, gelu64, layernorm64,  # noqa: E402
                        ln_factor, magnitude_factor, rows_of_class, run_entries, run_twice)
from fuzz_layer import TOL as LAYER_TOL  # noqa: E402

CONV3X3, DECONV = 1, 2  # PP_CONV3X3, PP_DECONV4X4S2
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
F32_TOL = 2e-4           # tests/fuzz_gemm.py
BF16_F32OUT_TOL = 2e-3
BF16_OUT_RTOL, BF16_OUT_ATOL = 2.0 ** -8, 2e-3
ENGINE_MAPS = [(16, 12, 384), (24, 18, 768), (4, 4, 384), (6, 6, 768), (3, 3, 384), (2, 2, 768)]
KERNELS = ("pp_gemm.hip", "pp_panel_split.hip", "pp_panel_gemm.hip", "pp_conv_halo.hip", "pp_head.hip")
# (entry, precision, kind) -> kernels the chosen shapes must reach
EXPECTED = {
    ("pp_conv_gemm", "bf16", "conv3x3"): {"pp_gemm.hip", "pp_panel_split.hip", "pp_panel_gemm.hip", "pp_conv_halo.hip"},
    ("pp_conv_gemm", "bf16", "deconv"): {"pp_gemm.hip", "pp_panel_split.hip", "pp_panel_gemm.hip"},
    ("pp_conv_gemm", "f32", "conv3x3"): {"pp_gemm.hip"},
    ("pp_conv_gemm", "f32", "deconv"): {"pp_gemm.hip"},
    ("pp_conv_gemm", "f16x3", "conv3x3"): {"pp_gemm.hip", "pp_panel_split.hip"},
    ("pp_conv_gemm", "f16x3", "deconv"): {"pp_gemm.hip", "pp_panel_split.hip"},
    ("pp_conv3x3_splitk", "bf16", "conv3x3"): {"pp_gemm.hip", "pp_panel_gemm.hip"},
    ("pp_conv3x3_splitk", "f32", "conv3x3"): {"pp_gemm.hip"},
    ("pp_conv3x3_maxpool_relu", "bf16", "conv3x3"): {"pp_conv_halo.hip", "pp_panel_gemm.hip", "pp_gemm.hip"},
    ("pp_deconv_head", "bf16", "deconv"): {"pp_panel_gemm.hip"},
}
PREC_NAME = {BF16: "bf16", F32: "f32", F16X3: "f16x3"}
DEFAULT_OPTIONS = dict(panel=1, conv_halo=1, psplit_nst=0, psplit_bf16_conv=0, psplit_tap_inner=1, psplit_conv_weight_major=1,
                       psplit_deconv_weight_major=0)


# ----------------------------------------------------------------------------------------------------- fp64 references (checked by the CPU test)
def act64(y, act):
    return gelu64(y) if act == ACT_GELU else torch.relu(y) if act == ACT_RELU else y


def deconv64(x, w, b=None):
    """ConvTranspose2d(k4, s2, p1): x (B, Cin, H, W), w (Cin, Cout, 4, 4) -> (B, Cout, 2H, 2W), written out as its four output phases."""
    B, Cin, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.empty((B, w.shape[1], 2 * H, 2 * W), dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            out[:, :, py::2, px::2] = sum(torch.einsum("bchw,co->bohw", xp[:, :, py + ty:py + ty + H, px + tx:px + tx + W], w[:, :, 3 - 2 * ty - py, 3 - 2 * tx - px])
                                          for ty in range(2) for tx in range(2))
    return out + b.view(1, -1, 1, 1) if b is not None else out


def pool_relu_floor64(y, ph, pw):
    """MaxPool2d(kernel = stride = (ph, pw), floor: the last rows / columns a window does not fill are dropped) + ReLU; a NaN in a window gives NaN."""
    B, C, H, W = y.shape
    Ho, Wo = H // ph, W // pw
    return torch.relu(y[:, :, :Ho * ph, :Wo * pw].reshape(B, C, Ho, ph, Wo, pw).amax(dim=(3, 5)))


def im2col64(img, mean, std, pad, passes, bgr_to_rgb):
    """(B, 3, H, W) uint8 / float -> (passes * B * Hp * Wp, 768) fp64 rows of 16 x 16 patches, channel-major (F.unfold's order): (x - mean) / std of
    the RGB image (channels reversed first when bgr_to_rgb), the second pass mirrored left-right, zero padding `pad` on every side."""
    x = img.double()
    if bgr_to_rgb:
        x = x.flip(1)
    x = (x - torch.as_tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.as_tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    if passes == 2:
        x = torch.cat([x, x.flip(-1)])
    B, _, H, W = x.shape
    Hp, Wp = (H + 2 * pad - 16) // 16 + 1, (W + 2 * pad - 16) // 16 + 1
    xp = F.pad(x, (pad, pad, pad, pad))
    rows = []
    for py in range(Hp):
        for px in range(Wp):
            rows.append(xp[:, :, 16 * py:16 * py + 16, 16 * px:16 * px + 16].reshape(B, 768))
    return torch.stack(rows, dim=1).reshape(B * Hp * Wp, 768)


def bf16_out_ratio(got, ref):
    """bf16 output: one rounding of the result (2^-8 relative) on top of the fp32 accumulation's 2e-3."""
    return error_ratio(got, ref, BF16_OUT_RTOL, BF16_OUT_ATOL)


def ulp32(x):
    """fp32 unit in the last place of |x| (fp64 tensor)."""
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).double()


def border_impulses(B, H, W, C, g, n=2):
    """(B, H, W, C) fp32, zero but n pixels on each of the first / last rows and columns of every image, values +-8 (1 +- 0.25)."""
    x = torch.zeros(B, H, W, C)
    for i in range(B):
        for _ in range(n):
            for y, xx in ((0, None), (H - 1, None), (None, 0), (None, W - 1)):
                yy = int(torch.randint(0, H, (1,), generator=g)) if y is None else y
                xc = int(torch.randint(0, W, (1,), generator=g)) if xx is None else xx
                x[i, yy, xc] = 8.0 * (1 + 0.25 * torch.randn(C, generator=g)) * torch.sign(torch.randn(C, generator=g))
    return x


def input_of_class(cls, B, H, W, C, g):
    """NHWC activations (CPU fp32) of a value class: normal, massive (three channels at 60 .. 250), border."""
    if cls == "border":
        return border_impulses(B, H, W, C, g)
    x = torch.randn(B, H, W, C, generator=g)
    if cls == "massive":
        for c, m in zip(torch.randperm(C, generator=g)[:3].tolist(), MASSIVE):
            x[..., c] = m * (0.5 + 0.5 * torch.rand(B, H, W, generator=g))
    return x


# ----------------------------------------------------------------------------------------------------- the dispatcher, mirrored
def conv_kernel(prec, kind, B, H, W, Cin, Cout, groups, fmt, act, opt):
    """Which kernel pp_conv_gemm launches (pp_gemm.hip: panel_split_supported, conv_halo_supported, panel_gemm_supported, else gemm); "refused":
    Cin is no multiple of the precision's K-tile (64 channels in bf16, 32 in fp32 and f16x3), PP_ERR_UNSUPPORTED from every kernel."""
    M, K = B * H * W, (9 if kind == CONV3X3 else 4) * Cin
    if Cin % (64 if prec == BF16 else 32) != 0:
        return "refused"

    def tiles(bm, bn):
        return (Cout // bn) * ((M + bm - 1) // bm) * groups

    if opt["panel"]:
        ok = False
        if prec == F16X3 and fmt in (0, 2) and Cin % 32 == 0 and Cout % 32 == 0 and K % 32 == 0:
            ok = True
        elif prec == BF16 and opt["psplit_bf16_conv"] and K % 128 == 0 and Cin % 64 == 0 and fmt in (0, 1) and Cout % 8 == 0:
            ok = True
        if ok:
            if kind == DECONV:
                bm, bn = (128, 256) if (opt["psplit_nst"] == 3) else (192, 256)
            else:
                bm, bn = (192, 192) if opt["psplit_nst"] == 3 else (256, 192)
            if Cout % bn == 0 and tiles(bm, bn) >= 192:
                return "pp_panel_split.hip"
        if (opt["conv_halo"] and prec == BF16 and kind == CONV3X3 and fmt == 1 and act in (ACT_NONE, ACT_RELU) and H * W == 192
                and (H + 2) * (W + 2) == 252 and Cin % 128 == 0 and Cout % 128 == 0 and tiles(384, 128) >= 192):
            return "pp_conv_halo.hip"
        if prec == BF16 and fmt == 1 and act in (ACT_NONE, ACT_RELU) and Cin % 64 == 0 and K % 128 == 0:
            bm, bn = (192, 256) if kind == DECONV else (256, 192)
            if Cout % bn == 0 and tiles(bm, bn) >= 192:
                return "pp_panel_gemm.hip"
    return "pp_gemm.hip"


def splitk_kernel(prec, B, H, W, Cin, Cout, groups, ks, opt):
    """pp_conv3x3_splitk for whole-tap slices: the wide-tile bf16 kernel (fp32 partials) with enough tiles, else the 128 x 128 kernel."""
    M = B * H * W
    if opt["panel"] and prec == BF16 and Cin % 64 == 0 and (9 * Cin // ks) % 128 == 0 and Cout % 192 == 0 and ks > 1:
        if (Cout // 192) * ((M + 255) // 256) * groups * ks >= 192:
            return "pp_panel_gemm.hip"
    return "pp_gemm.hip"


def b_around(tiles_per_img, rng, lo=1, hi=None):
    """B with the tile count (tiles_per_img images per tile count, as a float) just below, at and above 192, or random."""
    b0 = max(1, math.ceil(192 / tiles_per_img))
    c = [b0 - 1, b0, b0 + 1, int(rng.integers(1, 2 * b0 + 2)), int(rng.integers(1, 9))]
    B = int(rng.choice(c))
    B = max(lo, B)
    return min(B, hi) if hi else B


# ----------------------------------------------------------------------------------------------------- GPU helpers and single cases
def sp(x):
    from probpose_code_amd.weights import to_split

    return to_split(x.float()).cuda()


def unsp(c):
    from probpose_code_amd.weights import from_split

    return from_split(c.float().cpu()).double()


def launch(fn, *args):
    from probpose_code_amd import _lib as L

    try:
        L.call(fn, *args)
    except L.ProbPoseLibraryError as exc:
        if "UNSUPPORTED" in str(exc) or "INVALID" in str(exc):
            raise Refused(str(exc)) from None
        raise
    torch.cuda.synchronize()


def ran():
    from probpose_code_amd import _lib as L

    return [k for k in KERNELS if L.launch_count(k) > 0]


def apply_options(opt):
    from probpose_code_amd import _lib as L

    for k, v in opt.items():
        if L.get_option(k) != v:
            L.set_option(k, v)


def dev(x, prec):
    """CPU fp32 -> device operand of the precision; and the fp64 values the kernel multiplies (bf16-rounded for bf16)."""
    if prec == F16X3:
        return sp(x), x.double()
    if prec == BF16:
        return x.bfloat16().cuda(), x.bfloat16().double()
    return x.cuda(), x.double()


def out_of(snap_t, fmt):
    return unsp(snap_t) if fmt == SPLIT else snap_t.cpu().double()


def tol_ratio(got, ref, prec, fmt, fac):
    if prec == F16X3:
        return error_ratio(got, ref, fac[0] * fac[1], fac[0] * fac[1])
    if prec == F32:
        return error_ratio(got, ref, F32_TOL, F32_TOL)
    return bf16_out_ratio(got, ref) if fmt == 1 else error_ratio(got, ref, BF16_F32OUT_TOL, BF16_F32OUT_TOL)


def pick(n, rng, k):
    return torch.unique(torch.tensor([0, n - 1] + rng.integers(0, n, k).tolist())) if n > k + 2 else torch.arange(n)


def conv_gemm_case(prec, kind, B, H, W, Cin, Cout, groups, fmt, act, bias, shared, phase, cls, opt, oname, rng, g, record=None, kernels=None):
    """One guarded launch pair of pp_conv_gemm -> (faults, error / tolerance, description). PP_CONV3X3 with `groups` problems on shared or
    separate inputs; PP_DECONV4X4S2 with all four phases in one launch (phase < 0) or one launch each, `phase` first. ``opt``: the steering
    options to run under (``oname``: the one that differs from the defaults, for the description). The kernels that ran are handed to
    ``record`` and appended to ``kernels``."""
    from probpose_code_amd import _lib as L

    kname = "conv3x3" if kind == CONV3X3 else "deconv"
    want = conv_kernel(prec, kind, B, H, W, Cin, Cout, groups if kind == CONV3X3 else (4 if phase < 0 else 1), fmt, act, opt)
    apply_options(opt)
    ng = 1 if shared else groups
    x = torch.stack([input_of_class(cls, B, H, W, Cin, g) for _ in range(ng)])
    if kind == CONV3X3:
        w = cpu_rand(groups, Cout, Cin, 3, 3, g=g, scale=1 / math.sqrt(9 * Cin))
        wk = w.permute(0, 1, 3, 4, 2).reshape(groups, Cout, 9 * Cin)
    else:
        w = cpu_rand(1, Cin, Cout, 4, 4, g=g, scale=1 / math.sqrt(4 * Cin))
        wk = deconv_phases(w[0]).reshape(1, 4, Cout, 4 * Cin)
    b = cpu_rand(groups, Cout, g=g, scale=0.3)
    guard = Guard()
    xd, xq = dev(x, prec)
    wd, wq = dev(wk, prec)
    xd, wd = guard.inp("act", xd), guard.inp("weight", wd)
    bd = guard.inp("bias", b) if bias else None
    odt = torch.bfloat16 if fmt == 1 else torch.float32
    oh, ow = (H, W) if kind == CONV3X3 else (2 * H, 2 * W)
    out = guard.out("out", (groups, B, oh, ow, Cout), dtype=odt)
    sa = 0 if shared else B * H * W * Cin

    def go():
        if kind == CONV3X3:
            launch("pp_conv_gemm", prec, CONV3X3, xd.data_ptr(), wd.data_ptr(), L.ptr(bd), out.data_ptr(), B, H, W, Cin, Cout, 0, 0, groups, sa,
                   Cout * 9 * Cin, B * H * W * Cout, Cout if bias else 0, Cout, act, fmt, None)
        elif phase < 0:
            launch("pp_conv_gemm", prec, DECONV, xd.data_ptr(), wd.data_ptr(), L.ptr(bd), out.data_ptr(), B, H, W, Cin, Cout, -1, 0, 1, 0, 0, 0, 0,
                   Cout, act, fmt, None)
        else:  # the four phases, one launch each, `phase` first
            for k in range(4):
                py, px = divmod((phase + k) % 4, 2)
                launch("pp_conv_gemm", prec, DECONV, xd.data_ptr(), wd[0, 2 * py + px].data_ptr(), L.ptr(bd), out.data_ptr(), B, H, W, Cin, Cout,
                       py, px, 1, 0, 0, 0, 0, Cout, act, fmt, None)
    L.reset_launch_counts()
    faults, snap = run_guarded(guard, go)
    got_k = ran()
    if kernels is not None:
        kernels += got_k
    if record is not None:
        record("pp_conv_gemm", prec, kname, got_k)
    if got_k != [want]:
        faults.append(f"kernel {got_k}, the mirrored dispatcher predicts {want}")
    imgs = pick(B, rng, 1)
    ratio = 0.0
    fac = (HEAD_TOL["conv_pool"] if kind == CONV3X3 else HEAD_TOL["deconv_head"], magnitude_factor(xq[:, imgs].reshape(-1, Cin)))
    for k in range(groups):
        xi = xq[0 if shared or kind == DECONV else k][imgs].permute(0, 3, 1, 2)
        if kind == CONV3X3:
            ch = torch.from_numpy(rng.choice(Cout, min(Cout, 48), replace=False))
            wt = wq[k].reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)[ch]
            ref = act64(conv3x3_64(xi, wt, b[k][ch].double() if bias else None), act)
        else:
            ch = torch.arange(Cout)
            ph = wq[0].reshape(2, 2, Cout, 4 * Cin)
            wt = torch.empty(Cin, Cout, 4, 4, dtype=torch.float64)  # the torch weight the (rounded) phase matrices stand for
            for py in range(2):
                for px in range(2):
                    for ty in range(2):
                        for tx in range(2):
                            t = ty * 2 + tx
                            wt[:, :, 3 - 2 * ty - py, 3 - 2 * tx - px] = ph[py, px, :, t * Cin:(t + 1) * Cin].t()
            ref = act64(deconv64(xi, wt, b[0].double() if bias else None), act)
        got = out_of(snap[0][k][imgs], fmt)[..., ch].permute(0, 3, 1, 2)
        ratio = max(ratio, tol_ratio(got, ref, prec, fmt, fac))
    info = (f"{PREC_NAME[prec]} {kname} B {B} {H}x{W} Cin {Cin} Cout {Cout} groups {groups} shared {shared} phase {phase} bias {bias} act {act} "
            f"fmt {fmt} class {cls} option {oname}={opt.get(oname)} kernel {want}")
    return faults, ratio, info


def deconv_head_case(B, H, W, Cin, K, cls, rng, g, record=None):
    """One guarded launch pair of pp_deconv_head (bf16: the last deconvolution to 256 channels + ReLU + the 1x1 convolution to K maps, logits in
    the phase-separated layout) -> (faults, error / tolerance, description)."""
    from probpose_code_amd import _lib as L

    Cout = 256
    x = input_of_class(cls, B, H, W, Cin, g)
    w = cpu_rand(Cin, Cout, 4, 4, g=g, scale=1 / math.sqrt(4 * Cin))
    b = cpu_rand(Cout, g=g, scale=0.2)
    wf, bf = cpu_rand(K, Cout, g=g, scale=4 / math.sqrt(Cout)), cpu_rand(K, g=g)
    wpad = torch.zeros(32, Cout)
    wpad[:K] = wf
    guard = Guard()
    xd, phd = guard.inp("act", x.bfloat16().cuda()), guard.inp("weight", deconv_phases(w).bfloat16().cuda())
    bd, hwd, bfd = guard.inp("bias", b), guard.inp("head_w", wpad.bfloat16().cuda()), guard.inp("head_b", bf)
    lg = guard.out("logits", (B, K, 4, H * W))

    def go():
        launch("pp_deconv_head", xd.data_ptr(), phd.data_ptr(), bd.data_ptr(), hwd.data_ptr(), bfd.data_ptr(), lg.data_ptr(), B, H, W, Cin, Cout, K,
               None)
    L.reset_launch_counts()
    faults, snap = run_guarded(guard, go)
    got_k = ran()
    if record is not None:
        record("pp_deconv_head", BF16, "deconv", got_k)
    if got_k != ["pp_panel_gemm.hip"]:
        faults.append(f"kernels {got_k}")
    imgs = pick(B, rng, 1)
    xi = x[imgs].bfloat16().double().permute(0, 3, 1, 2)
    wq, wfq = w.bfloat16().double(), wf.bfloat16().double()
    mid = torch.relu(deconv64(xi, wq, b.double())).float().bfloat16().double()  # the kernel hands the 1x1 bf16 activations
    ref = torch.einsum("bchw,kc->bkhw", mid, wfq) + bf.double().view(1, -1, 1, 1)
    got = snap[0][imgs].cpu().double().reshape(len(imgs), K, 2, 2, H, W).permute(0, 1, 4, 2, 5, 3).reshape(len(imgs), K, 2 * H, 2 * W)
    # a mid value at a rounding boundary may round the other way from fp32 than from fp64: one bf16 step of the largest product
    flip = 2.0 ** -8 * float(mid.abs().max()) * float(wfq.abs().max())
    return faults, error_ratio(got, ref, BF16_F32OUT_TOL, BF16_F32OUT_TOL + flip), f"B {B} {H}x{W} Cin {Cin} K {K} class {cls}"


def _main(seconds):
    from probpose_code_amd import _lib as L
    from probpose_code_amd.weights import from_split, to_split

    table = {}  # (entry, prec, kind) -> {kernel: cases}

    def draw_options(rng):
        """The defaults with one steering option changed (set by apply_options; the standalone run restores them through run_entries, the suite's
        fixture as well)."""
        opt = dict(DEFAULT_OPTIONS)
        name = str(rng.choice(["none", "panel", "conv_halo", "psplit_nst", "psplit_bf16_conv", "psplit_tap_inner", "psplit_conv_weight_major",
                               "psplit_deconv_weight_major"]))
        if name != "none":
            opt[name] = {"panel": 0, "conv_halo": 0, "psplit_nst": int(rng.choice([2, 3])), "psplit_bf16_conv": 1, "psplit_tap_inner": int(rng.choice([0, 2])),
                         "psplit_conv_weight_major": 0, "psplit_deconv_weight_major": 1}[name]
        return opt, name

    visits = {}

    def next_target(entry):
        """The (precision, kind, kernel) cell a visit must land in: every expected cell of the entry in turn on its first visits (so that a run of
        a few seconds fills the table), then every other visit; None: a free draw."""
        cells = sorted((p, k, kern) for (e, p, k), kerns in EXPECTED.items() if e == entry for kern in kerns)
        v = visits[entry] = visits.get(entry, -1) + 1
        if v < len(cells):
            return cells[v]
        return cells[(v // 2) % len(cells)] if v % 2 == 0 else None

    def record(entry, prec, kind, kernels):
        cell = table.setdefault((entry, PREC_NAME[prec], kind), {})
        for k in kernels:
            cell[k] = cell.get(k, 0) + 1

    # ------------------------------------------------------------------------------------------------- pp_conv_gemm
    def case_conv_gemm(rng, g):
        target = next_target("pp_conv_gemm")
        for _ in range(100000):  # (parameters only: a draw costs microseconds)
            prec = int(rng.choice([BF16, F32, F16X3]))
            kind = int(rng.choice([CONV3X3, DECONV]))
            opt, oname = draw_options(rng)
            if rng.random() < 0.6:
                H, W, Cin = ENGINE_MAPS[int(rng.integers(0, len(ENGINE_MAPS)))]
                if kind == DECONV and rng.random() < 0.4:
                    H, W, Cin = 32, 24, 256  # the second heatmap deconvolution
            else:
                H, W = int(rng.integers(1, 25)), int(rng.integers(1, 25))
                Cin = int(rng.choice([64, 128, 192, 256, 384]))
                if kind == DECONV:  # the widths between the K-tiles' multiples too (bf16: refused unless Cin % 64 == 0)
                    Cin = int(rng.choice([64, 96, 128, 160, 192, 256, 384] + ([] if prec == BF16 else [32])))
            if kind == CONV3X3:
                Cout = int(rng.choice([Cin, Cin, 192, 384, 128, 96, 64]))
                groups = int(rng.integers(1, 5))
            else:
                Cout = int(rng.choice([256, 256, 512, 128, 64]))
                groups = 1
            fmts = {BF16: [0, 1], F32: [0], F16X3: [0, SPLIT]}[prec]
            fmt = int(rng.choice(fmts))
            act = int(rng.integers(0, 3))
            bias = rng.random() < 0.7
            shared = kind == CONV3X3 and rng.random() < 0.5
            phase = int(rng.integers(-1, 4)) if kind == DECONV else 0  # -1: all four in one launch; 0 - 3: the four phases one launch each
            # B: tile counts on both sides of 192 for the kernel the options favour
            M1 = H * W
            if kind == CONV3X3:
                bm, bn = (384, 128) if (prec == BF16 and M1 == 192 and fmt == 1 and rng.random() < 0.5) else (256, 192)
            else:
                bm, bn = 192, 256
            per_img = (max(1, Cout // bn) * (groups if kind == CONV3X3 else (4 if phase < 0 else 1))) * M1 / bm
            esz = 2 if prec == BF16 else 4
            cap = max(1, int(MEM_CAP // (M1 * (Cin * esz * (1 if shared else groups) + Cout * 4 * groups * (4 if kind == DECONV else 1)) * 2)))
            B = b_around(per_img, rng, hi=min(cap, 2048))
            cls = str(rng.choice(["normal", "massive", "border"]))
            kname = "conv3x3" if kind == CONV3X3 else "deconv"
            want = conv_kernel(prec, kind, B, H, W, Cin, Cout, groups if kind == CONV3X3 else (4 if phase < 0 else 1), fmt, act, opt)
            if target is None or target == (PREC_NAME[prec], kname, want):
                break
        return conv_gemm_case(prec, kind, B, H, W, Cin, Cout, groups, fmt, act, bias, shared, phase, cls, opt, oname, rng, g, record)

    # ------------------------------------------------------------------------------------------------- split-K + sum-pool
    def case_splitk(rng, g):
        target = next_target("pp_conv3x3_splitk")
        for _ in range(100000):
            prec = int(rng.choice([BF16, F32]))
            opt, oname = draw_options(rng)
            H, W, C = [(4, 4, 384), (6, 6, 768), (3, 3, 384), (2, 2, 768), (8, 6, 384), (16, 12, 384)][int(rng.integers(0, 6))]
            G = int(rng.integers(1, 5))
            ks = int(rng.choice([1, 3, 9]))
            per_img = (C // 192) * G * ks * H * W / 256
            B = b_around(per_img, rng, hi=max(1, int(MEM_CAP // (G * H * W * C * 4 * (ks + 2)))))
            want = splitk_kernel(prec, B, H, W, C, C, G, ks, opt)
            if target is None or target == (PREC_NAME[prec], "conv3x3", want):
                break
        apply_options(opt)
        ph, pw = [(2, 2), (4, 3), (3, 3), (2, 3)][int(rng.integers(0, 4))]
        ph, pw = min(ph, H), min(pw, W)
        cls = str(rng.choice(["normal", "massive", "border", "poison", "poison"]))
        shared = rng.random() < 0.5
        x = torch.stack([input_of_class("normal" if cls == "poison" else cls, B, H, W, C, g) for _ in range(1 if shared else G)])
        if cls == "poison":
            for k in range(x.shape[0]):
                for i in {0, B - 1}:
                    poison_(x[k, i], g, int(rng.integers(1, 3)))
        w = cpu_rand(G, C, C, 3, 3, g=g, scale=1 / math.sqrt(9 * C))
        b = cpu_rand(G, C, g=g)
        fmt = int(rng.choice([0, 1])) if prec == BF16 else 0
        guard = Guard()
        xd, xq = dev(x, prec)
        wd, wq = dev(w.permute(0, 1, 3, 4, 2).reshape(G, C, 9 * C), prec)
        xd, wd, bd = guard.inp("act", xd), guard.inp("weight", wd), guard.inp("bias", b)
        part = guard.out("partials", (ks, G, B, H, W, C))
        pooled = guard.out("pooled", (G * B, H // ph, W // pw, C), dtype=torch.bfloat16 if fmt == 1 else torch.float32)

        def go():
            launch("pp_conv3x3_splitk", prec, xd.data_ptr(), wd.data_ptr(), part.data_ptr(), B, H, W, C, C, G, 0 if shared else B * H * W * C, C * 9 * C,
                   ks, None)
            launch("pp_sum_maxpool_relu_nhwc", part.data_ptr(), ks, G * B * H * W * C, bd.data_ptr(), B, pooled.data_ptr(), fmt, G * B, H, W, C, ph, pw,
                   None)
        L.reset_launch_counts()
        faults, snap = run_twice(guard, go)
        got_k = ran()
        record("pp_conv3x3_splitk", prec, "conv3x3", [k for k in got_k if k != "pp_head.hip"])
        if got_k != sorted({want, "pp_head.hip"}, key=KERNELS.index):
            faults.append(f"kernels {got_k}, the mirrored dispatcher predicts {want} + pp_head.hip")
        imgs, ch = pick(B, rng, 1), torch.from_numpy(rng.choice(C, 48, replace=False))
        ratio = 0.0
        ptol = F32_TOL if prec == F32 else BF16_F32OUT_TOL
        for k in range(G):
            xk = xq[0 if shared else k][imgs]
            conv = conv3x3_64(xk.permute(0, 3, 1, 2), wq[k].reshape(C, 3, 3, C).permute(0, 3, 1, 2)[ch])
            psum = snap[0][:, k][:, imgs][..., ch].cpu().double().sum(0).permute(0, 3, 1, 2)
            pref = pool_relu_floor64(conv + b[k][ch].double().view(1, -1, 1, 1), ph, pw)
            pg = snap[1].view(G, B, H // ph, W // pw, C)[k][imgs][..., ch].cpu().double().permute(0, 3, 1, 2)
            rt = (BF16_OUT_RTOL, BF16_OUT_ATOL) if fmt == 1 else (ptol, ptol)
            if cls == "poison":
                bad = bad_pixels(xk)
                ratio = max(ratio, poison_ratio(psum, conv, conv_reach(bad), ptol, ptol), poison_ratio(pg, pref, conv_reach(bad, ph, pw), *rt))
            else:
                ratio = max(ratio, error_ratio(psum, conv, ptol, ptol), error_ratio(pg, pref, *rt))
        return faults, ratio, f"{PREC_NAME[prec]} B {B} {H}x{W} C {C} G {G} slices {ks} pool {ph}x{pw} fmt {fmt} shared {shared} class {cls} option {oname}"

    # ------------------------------------------------------------------------------------------------- bf16 conv + pool (halo kernel or two launches)
    def case_conv_pool(rng, g):
        target = next_target("pp_conv3x3_maxpool_relu")
        for _ in range(100000):
            opt, oname = draw_options(rng)
            H, W, C = [(16, 12, 384), (16, 12, 384), (8, 6, 384), (24, 18, 768)][int(rng.integers(0, 4))]
            ph, pw = (4, 3) if (H, W) == (16, 12) else (2, 2) if (H, W) == (8, 6) else (6, 6)
            G = int(rng.integers(1, 5))
            B = b_around((C // 128) * G * H * W / 384, rng, hi=max(1, int(MEM_CAP // (G * H * W * C * 2 * 3))))
            halo = (opt["conv_halo"] and (H, W) == (16, 12) and (C // 128) * ((B * 192 + 383) // 384) * G >= 192)
            want = ["pp_conv_halo.hip"] if halo else sorted({conv_kernel(BF16, CONV3X3, B, H, W, C, C, G, 1, ACT_NONE, opt), "pp_head.hip"}, key=KERNELS.index)
            if target is None or target[2] in want:
                break
        apply_options(opt)
        cls = str(rng.choice(["normal", "massive", "border", "poison", "poison"]))
        x = input_of_class("normal" if cls == "poison" else cls, B, H, W, C, g)
        if cls == "poison":
            for i in {0, B - 1}:
                poison_(x[i], g, int(rng.integers(1, 4)))
        w = cpu_rand(G, C, C, 3, 3, g=g, scale=1 / math.sqrt(9 * C))
        b = cpu_rand(G, C, g=g)
        guard = Guard()
        xd, xq = dev(x, BF16)
        wd, wq = dev(w.permute(0, 1, 3, 4, 2).reshape(G, C, 9 * C), BF16)
        xd, wd, bd = guard.inp("act", xd), guard.inp("weight", wd), guard.inp("bias", b)
        pooled = guard.out("pooled", (G, B, H // ph, W // pw, C), dtype=torch.bfloat16)
        scratch = guard.out("scratch", (G, B, H, W, C), dtype=torch.bfloat16, must_write=False)

        def go():
            launch("pp_conv3x3_maxpool_relu", BF16, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), pooled.data_ptr(), scratch.data_ptr(), B, H, W, C, C,
                   ph, pw, G, 0, C * 9 * C, C, 1, None)
        L.reset_launch_counts()
        faults, snap = run_twice(guard, go)
        got_k = ran()
        record("pp_conv3x3_maxpool_relu", BF16, "conv3x3", [k for k in got_k if k != "pp_head.hip"])
        if got_k != want:
            faults.append(f"kernels {got_k}, the mirrored dispatcher predicts {want}")
        imgs, ch = pick(B, rng, 1), torch.from_numpy(rng.choice(C, 48, replace=False))
        ratio = 0.0
        for k in range(G):
            ref = pool_relu_floor64(conv3x3_64(xq[imgs].permute(0, 3, 1, 2), wq[k].reshape(C, 3, 3, C).permute(0, 3, 1, 2)[ch], b[k][ch].double()), ph, pw)
            got = snap[0][k][imgs][..., ch].cpu().double().permute(0, 3, 1, 2)
            if cls == "poison":
                ratio = max(ratio, poison_ratio(got, ref, conv_reach(bad_pixels(xq[imgs]), ph, pw), BF16_OUT_RTOL, BF16_OUT_ATOL))
            else:
                ratio = max(ratio, bf16_out_ratio(got, ref))
        return faults, ratio, f"B {B} {H}x{W} C {C} G {G} class {cls} option {oname} kernels {want}"

    # ------------------------------------------------------------------------------------------------- bf16 deconvolution + 1x1 head
    def case_deconv_head(rng, g):
        H, W, Cin = [(32, 24, 256), (16, 12, 384), (48, 36, 256), (4, 4, 128)][int(rng.integers(0, 4))]
        Cout, K = 256, int(rng.integers(1, 29))
        B = int(rng.choice([1, 2, 5, 16, 64, int(rng.integers(1, 129))]))
        B = max(1, min(B, int(MEM_CAP // (H * W * (Cin * 2 + 28 * 16) * 2))))
        cls = str(rng.choice(["normal", "massive", "border"]))
        return deconv_head_case(B, H, W, Cin, K, cls, rng, g, record)

    # ------------------------------------------------------------------------------------------------- pooling alone
    def case_maxpool(rng, g):
        fin, fout = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 2), (2, 0), (0, 2)][int(rng.integers(0, 7))]
        if rng.random() < 0.5:
            H, W, C = ENGINE_MAPS[int(rng.integers(0, len(ENGINE_MAPS)))]
        else:
            H, W, C = int(rng.integers(1, 30)), int(rng.integers(1, 30)), 32 * int(rng.integers(1, 25))
        if fin != 2 and fout != 2 and rng.random() < 0.3:
            C = 4 * int(rng.integers(1, 200))
        ph, pw = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        if rng.random() < 0.5:
            ph, pw = min(int(rng.choice([2, 3, 4])), H), min(int(rng.choice([2, 3, 4])), W)
        N = int(rng.choice([1, 3, 64, 4 * 128, int(rng.integers(1, 1000))]))
        N = max(1, min(N, int(MEM_CAP // (H * W * C * 4 * 4))))
        cls = str(rng.choice(["normal", "massive", "poison", "poison"]))
        x = input_of_class("normal" if cls == "poison" else cls, N, H, W, C, g)
        if cls == "poison":
            for i in {0, N - 1}:
                poison_(x[i], g, int(rng.integers(1, 6)))
        guard = Guard()
        if fin == SPLIT:
            xd, xq = sp(x), from_split(to_split(x)).double()
        elif fin == 1:
            xd, xq = x.bfloat16().cuda(), x.bfloat16().double()
        else:
            xd, xq = x.cuda(), x.double()
        xd = guard.inp("in", xd)
        out = guard.out("out", (N, H // ph, W // pw, C), dtype=torch.bfloat16 if fout == 1 else torch.float32)

        def go():
            launch("pp_maxpool_relu_nhwc", xd.data_ptr(), fin, out.data_ptr(), fout, N, H, W, C, ph, pw, None)
        L.reset_launch_counts()
        faults, snap = run_twice(guard, go)
        record("pp_maxpool_relu_nhwc", F32, f"{fin}->{fout}", ran())
        imgs = pick(N, rng, 3)
        ref = pool_relu_floor64(xq[imgs].permute(0, 3, 1, 2), ph, pw)
        if fout != fin:  # one rounding of the exact max into the output format
            ref = (ref.float().bfloat16().double() if fout == 1 else from_split(to_split(ref.permute(0, 2, 3, 1).float())).double().permute(0, 3, 1, 2)
                   if fout == SPLIT else ref)
        got = out_of(snap[0][imgs], fout).permute(0, 3, 1, 2)
        # a max of stored values is exact: the output must equal the reference's rounding bit for bit where both are finite
        if cls == "poison":
            bad = bad_pixels(xq[imgs])
            reach = F.max_pool2d(bad.double()[:, None][:, :, :H // ph * ph, :W // pw * pw], (ph, pw)) > 0
            ratio = poison_ratio(got, ref, reach, 0.0, 1e-300)
        else:
            ratio = error_ratio(got, ref, 0.0, 1e-300)
        return faults, ratio, f"in {fin} out {fout} N {N} {H}x{W} C {C} window {ph}x{pw} class {cls}"

    # ------------------------------------------------------------------------------------------------- preprocessing + im2col
    def case_im2col(rng, g):
        prec = int(rng.choice([BF16, F32, F16X3]))
        f32_in = rng.random() < 0.3
        if rng.random() < 0.3:
            H, W = [(256, 192), (384, 288)][int(rng.integers(0, 2))]
        else:
            H, W = int(rng.integers(max(1, 16 - 6), 300)), int(rng.integers(max(1, 16 - 6), 300))
        pad = int(rng.integers(0, 4))
        H, W = max(H, 16 - 2 * pad), max(W, 16 - 2 * pad)
        passes = int(rng.integers(1, 3))
        bgr = int(rng.integers(0, 2))
        B = int(rng.choice([1, 2, 7, 64, int(rng.integers(1, 100))]))
        Hp, Wp = (H + 2 * pad - 16) // 16 + 1, (W + 2 * pad - 16) // 16 + 1
        B = max(1, min(B, 6000 // (passes * Hp * Wp)))  # (the fp64 reference is computed on every row)
        if f32_in:
            img = torch.randn(B, 3, H, W, generator=g) * 2
            mean, std = np.zeros(3, np.float32), np.ones(3, np.float32)
        else:
            img = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
            mean = np.array([123.675, 116.28, 103.53], np.float32) + rng.normal(0, 5, 3).astype(np.float32)
            std = np.array([58.395, 57.12, 57.375], np.float32) * rng.uniform(0.8, 1.2, 3).astype(np.float32)
        guard = Guard()
        imd = guard.inp("img", img)
        rows = passes * B * Hp * Wp
        out = guard.out("patches", (rows, 768), dtype=torch.bfloat16 if prec == BF16 else torch.float32)
        out32 = torch.empty((rows, 768), device="cuda")

        def go():
            launch("pp_preproc_im2col", prec, imd.data_ptr(), int(f32_in), out.data_ptr(), B, passes, H, W, 16, pad, None if f32_in else mean.ctypes.data,
                   None if f32_in else std.ctypes.data, bgr, None)
        faults, snap = run_twice(guard, go)
        ref = im2col64(img, mean.astype(np.float64), std.astype(np.float64), pad, passes, bool(bgr) and not f32_in)
        if prec == F32:
            got = snap[0].cpu().double()
            ratio = float(((got - ref).abs() / (2 * ulp32(ref)).clamp_min(1e-300)).max())
        else:
            launch("pp_preproc_im2col", F32, imd.data_ptr(), int(f32_in), out32.data_ptr(), B, passes, H, W, 16, pad, None if f32_in else mean.ctypes.data,
                   None if f32_in else std.ctypes.data, bgr, None)
            r32 = out32.cpu()
            ratio = float(((r32.double() - ref).abs() / (2 * ulp32(ref)).clamp_min(1e-300)).max())
            same = torch.equal(snap[0].cpu().view(torch.int16), r32.bfloat16().view(torch.int16)) if prec == BF16 else \
                torch.equal(snap[0].cpu().view(torch.int32), to_split(r32).view(torch.int32))
            if not same:
                faults.append("not the correctly rounded value of the fp32 result")
        return faults, ratio, f"{PREC_NAME[prec]} B {B} {H}x{W} pad {pad} passes {passes} bgr {bgr} f32_in {f32_in}"

    # ------------------------------------------------------------------------------------------------- LayerNorm
    def case_layernorm(rng, g):
        E = int(rng.choice([384, 768, 1024, 1280]))
        fmt = int(rng.choice([0, 1, SPLIT]))
        M = int(rng.choice([1, 3, 4, 5, 192, 203, 12288, int(rng.integers(1, 30000))]))
        cls = str(rng.choice(["normal", "offset", "massive"]))
        x = rows_of_class(M, E, cls, g, device="cpu")
        gam, bet = 1 + 0.1 * cpu_rand(E, g=g), cpu_rand(E, g=g, scale=0.1)
        guard = Guard()
        xd, gd, bd = guard.inp("x", x), guard.inp("gamma", gam), guard.inp("beta", bet)
        y = guard.out("y", (M, E), dtype=torch.bfloat16 if fmt == 1 else torch.float32)

        def go():
            launch("pp_layernorm", xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), M, E, 1e-6, fmt, None)
        faults, snap = run_twice(guard, go)
        rows = pick(M, rng, 64)
        ref = layernorm64(x[rows].double(), gam.double(), bet.double())
        got = out_of(snap[0][rows], fmt)
        base = LAYER_TOL["gemm_ln"] * ln_factor(x[rows])
        ratio = bf16_out_ratio(got, ref) if fmt == 1 else error_ratio(got, ref, base, base)
        return faults, ratio, f"M {M} E {E} fmt {fmt} class {cls}"

    entries = [
        ("pp_conv_gemm", case_conv_gemm),
        ("pp_conv3x3_splitk + pp_sum_maxpool_relu_nhwc", case_splitk),
        ("pp_conv3x3_maxpool_relu (bf16)", case_conv_pool),
        ("pp_deconv_head (bf16)", case_deconv_head),
        ("pp_maxpool_relu_nhwc", case_maxpool),
        ("pp_preproc_im2col", case_im2col),
        ("pp_layernorm", case_layernorm),
    ]

    def summary():
        """The (entry, precision, kind) x kernel table; a cell the chosen shapes must reach that stayed empty fails the run."""
        print(f"{'entry, precision, kind':52s} " + " ".join(f"{k[:-4]:>15s}" for k in KERNELS))
        empty = []
        for key in sorted(set(table) | set(EXPECTED)):
            cell = table.get(key, {})
            print(f"{', '.join(key):52s} " + " ".join(f"{cell.get(k, 0):15d}" for k in KERNELS))
            empty += [f"{', '.join(key)} -> {k}" for k in sorted(EXPECTED.get(key, ())) if not cell.get(k)]
        for e in empty:
            print(f"EMPTY CELL {e}")
        return empty

    return run_entries(entries, seconds, 110000, "CONV", L, summary=summary)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sys.exit(_main(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0))


if __name__ == "__main__":
    main()
