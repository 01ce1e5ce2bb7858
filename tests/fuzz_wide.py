#!/usr/bin/env python
"""Fuzz of the Linear and deconvolution kernels at the ViT-L / ViT-H widths (E = 1024 / 1280, FFN 4096 / 5120, qkv 3072 / 3840, first head
deconvolution Cin 768 / 1024 / 1280 -> K per phase 3072 / 4096 / 5120) against torch fp64, entry points visited round robin:
  * pp_gemm_ws in f16x3, bf16 and f32: half the draws one of the ten layer shapes of TABLE with the epilogue engine.py's _gemm sends with it (qkv:
    operand-format rows out; fc1: GELU + operand-format rows; proj / fc2: fp32 residual stream updated in place; patch embedding: position table
    as a residual with res_mod = 192), half K = 32 j <= 5120 (128 j for bf16), N over multiples of 32 and the epilogues of tests/fuzz_gemm.py
    (bias or none, GELU / ReLU, residual in place / separate / broadcast table, every output format, planar planes);
  * pp_skinny_linear at the five ViT-L small-batch shapes (SKINNY_SHAPES; its LayerNorm tail ends at 1024 columns), every tile shape that divides
    N forced in turn, both tile orders, the arrival counters back at zero;
  * pp_conv_gemm PP_DECONV4X4S2 at the first head deconvolution (16 x 12 x Cin -> 256 channels) in the three precisions, all four phases in one
    launch or one launch each, and pp_skinny_deconv on at most 1 536 input pixels.
M (and the image count of the deconvolutions) straddles the dispatch thresholds, restated below from csrc/pp_linear_dma.hip and
csrc/pp_panel_split.hip and checked on the CPU by tests/test_wide_references.py: the twelve-wave kernel takes a split-fp16 Linear layer with
N % 192 == 0 from 512 tiles of 192 x 192 on (M >= 5953 at N = 3072, 4801 at N = 3840), the wide-tile kernel from 192 tiles on, the 128 x 128
kernel the rest - every N that is no multiple of 192 (proj, fc1, fc2 and the patch embedding of ViT-L / -H). pp_launch_count tells which kernel
ran: another one than the restated dispatcher predicts is a mismatch, and the run fails unless each of the three kernels accepted an f16x3 case
at (3072, 1024) and at (3840, 1280), and the 128 x 128 kernel all eight other table shapes in each precision. A table shape at a row count the
engine sends (384 B rows, B = 1 .. 64) is never refused.

Values: activations and weights of the classes of tests/fuzz_layer.py rows_of_class (normal, offset, massive; weights divided by sqrt(K); not both
"offset": the dot products of two offset operands at K = 5120 leave the fp16 range of operand-format output rows), weight scale 2^e from draw_e in
f16x3. Every case: outputs between canaries (bit for bit), every element written, inputs bit-identical after the launch, a repeat launch
bit-identical, fp64 accuracy on sample_rows (first and last blocks whole, one row of every block).

Tolerances are the project's own, scaled by the operands' magnitude - a dot product's error is relative to |a_r| |w_n|, and the fixed bars hold
for unit-normal activation rows and weight rows of unit norm: fac = magnitude_factor(activation rows) * magnitude_factor(weight rows * sqrt(K)).
  * f16x3: TOL["linear_long"] * fac (Linear; fuzz_layer.case_linear), fuzz_head TOL["deconv_head"] * fac (deconvolution; fuzz_conv), 1e-4 on the
    LayerNorm tail's rows (tests/fuzz_skinny.py);
  * f32: fuzz_conv.F32_TOL * fac; bf16: fuzz_conv.BF16_F32OUT_TOL * fac for fp32 output, bf16_out_ratio on values divided by fac for bf16 output.
No K-dependent term was needed: the K = 4096 / 5120 cases stay below a quarter of these bars in f16x3 and a tenth in f32. The bf16-output bar is
one rounding of the result, which the 128 x 128 kernel missed with an fp32 residual (it rounded in front of the residual and again behind it: up
to 1.54 of the bar) until csrc/pp_gemm.hip added the residual first; tests/test_wide_widths_gpu.py keeps those cases.
``gemm_case``, ``skinny_case``, ``deconv_case`` and ``skinny_deconv_case`` are the single cases tests/test_wide_widths_gpu.py runs on its grid;
tests/fuzz_edges.py runs them at the smallest shapes the argument checks admit, through their optional parameters (row pitches of pp_gemm_ws;
map size and output width of the deconvolutions), whose defaults are the shapes above.
python tests/fuzz_wide.py [seconds]"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuzz_conv as FC  # noqa: E402
from fuzz_conv import BF16_F32OUT_TOL, F32_TOL, bf16_out_ratio, deconv64  # noqa: E402
from fuzz_head import TOL as HEAD_TOL  # noqa: E402
from fuzz_head import deconv_phases  # noqa: E402
from fuzz_layer import (BF16, F16X3, F32, MEM_CAP, PATTERN, TOL, Guard, Refused, cpu_rand, draw_e, error_ratio, gelu64, layernorm64,  # noqa: E402
                        magnitude_factor, rows_of_class, run_entries, run_twice, sample_rows)

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
DECONV = 2  # PP_DECONV4X4S2
PREC_NAME = {BF16: "bf16", F32: "f32", F16X3: "f16x3"}
OPERAND_FMT = {BF16: 1, F32: 0, F16X3: 2}  # PP_OUT_* of a precision's operand format
CLASSES = ("normal", "offset", "massive")
LN_TAIL_TOL = 1e-4  # tests/fuzz_skinny.py
GEMM_KERNELS = ("linear_dma_tile", "pp_panel_split.hip", "pp_gemm.hip")
# (arch, layer) -> (N, K) of the Linear layers the generic plan sends through pp_gemm_ws
TABLE = {
    ("large", "qkv"): (3072, 1024), ("large", "proj"): (1024, 1024), ("large", "fc1"): (4096, 1024), ("large", "fc2"): (1024, 4096),
    ("large", "patch"): (1024, 768),
    ("huge", "qkv"): (3840, 1280), ("huge", "proj"): (1280, 1280), ("huge", "fc1"): (5120, 1280), ("huge", "fc2"): (1280, 5120),
    ("huge", "patch"): (1280, 768),
}
# pp_skinny_linear at the ViT-L small-batch plan: (N, K, layer)
SKINNY_SHAPES = [(3072, 1024, "qkv"), (4096, 1024, "fc1"), (1024, 1024, "proj"), (1024, 4096, "fc2"), (1024, 768, "patch")]
SKINNY_M = [1, 2, 31, 32, 33, 63, 95, 96, 97, 191, 384, 385, 767, 1536, 2047, 2048, 3071, 3072, 6911]  # tests/fuzz_skinny.py
SKINNY_CODES = (0, 11, 22, 33, 13, 12, 23)         # option "skinny_tile": 10 x (rows / 32) + columns / 32; 0: the cost model's choice
SKINNY_DECONV_CODES = (0, 11, 22, 12, 32)
DECONV_CIN = (768, 1024, 1280)
MAP_H, MAP_W, DECONV_COUT = 16, 12, 256


# ----------------------------------------------------------------------------------------------------- the dispatcher, restated (CPU-checked)
def engine_epilogue(layer, prec):
    """The epilogue engine.py sends with a layer's pp_gemm_ws launch (backbone(): _gemm / res_ln)."""
    if layer == "qkv":
        return dict(bias=True, act=ACT_NONE, fmt=OPERAND_FMT[prec], res="none", res_mod=0)
    if layer == "fc1":
        return dict(bias=True, act=ACT_GELU, fmt=OPERAND_FMT[prec], res="none", res_mod=0)
    if layer in ("proj", "fc2"):
        return dict(bias=True, act=ACT_NONE, fmt=0, res="in_place", res_mod=0)
    if layer == "patch":
        return dict(bias=True, act=ACT_NONE, fmt=0, res="table", res_mod=192)
    raise ValueError(layer)


def dma_threshold(N):
    """Smallest M at which pp_gemm hands a split-fp16 Linear layer of N columns (N % 192 == 0) to the twelve-wave kernel: 512 tiles of 192 x 192."""
    return 192 * math.ceil(512 / (N // 192)) - 191


def wide_tile_rows(M, N):
    """Row count of the wide tile a Linear layer gets (panel_split_shape, default options): 192 where the 192 x 192 form needs at least 10 % less
    tile area over whole rounds of 256 workgroups than the 256 x 192 form, else 256."""
    t2, t4 = (N // 192) * ((M + 255) // 256), (N // 192) * ((M + 191) // 192)
    c2, c4 = ((t2 + 255) // 256) * 256 * 192, ((t4 + 255) // 256) * 192 * 192
    return 192 if c4 * 10 < c2 * 9 else 256


def wide_tiles(M, N):
    bm = wide_tile_rows(M, N)
    return (N // 192) * ((M + bm - 1) // bm)


def gemm_kernel(prec, M, N, K, fmt, residual, planar=False, lda=None, ldw=None, ldc=None):
    """Which kernel pp_gemm_ws launches for row-major operands (row pitches lda, ldw, ldc in elements; None: dense, lda = ldw = K, ldc = N),
    default options: linear_dma_supported (dense operands only), then panel_split_supported (pitches that are multiples of 32 elements in f16x3,
    of 8 in bf16), else the 128 x 128 kernel."""
    lda, ldw, ldc = K if lda is None else lda, K if ldw is None else ldw, N if ldc is None else ldc
    if planar or N % 192 != 0:
        return "pp_gemm.hip"
    if prec == F16X3:
        if fmt not in (0, 2) or K % 32 != 0 or N % 32 != 0 or (residual and fmt == 2) or lda % 32 or ldw % 32 or ldc % 32:
            return "pp_gemm.hip"
        if K >= 64 and (N // 192) * ((M + 191) // 192) >= 512 and (lda, ldw, ldc) == (K, K, N):
            return "linear_dma_tile"
    elif prec == BF16:
        if K < (1536 if fmt else 768) or K % 128 != 0 or fmt not in (0, 1) or N % 8 != 0 or lda % 8 or ldw % 8 or ldc % 8:
            return "pp_gemm.hip"
    else:
        return "pp_gemm.hip"
    return "pp_panel_split.hip" if wide_tiles(M, N) >= 192 else "pp_gemm.hip"


def wide_threshold(N, prec=F16X3, K=1024, fmt=0, hi=40000):
    """Smallest M at which the wide-tile kernel takes a Linear layer (tile counts change only where M - 1 is a multiple of 64); None: never."""
    for M in range(1, hi, 64):
        if gemm_kernel(prec, M, N, K, fmt, False) != "pp_gemm.hip":
            return M
    return None


def deconv_tiles(nb, phase):
    """Wide tiles (192 pixels x 256 channels) of the first head deconvolution of nb images: 16 x 12 = 192 input pixels an image, 256 output
    channels, times the four phases when one launch does them all (phase < 0). The wide-tile kernels take it from 192 tiles on."""
    return (4 if phase < 0 else 1) * math.ceil(MAP_H * MAP_W * nb / 192) * (DECONV_COUT // 256)


def deconv_threshold(phase):
    """Smallest image count at which the first head deconvolution reaches 192 wide tiles."""
    return next(nb for nb in range(1, 1000) if deconv_tiles(nb, phase) >= 192)


def linear_ref64(xq, wq, bias, act, res_rows):
    """fp64 Linear layer on the sampled rows: act(x W^T + b) + residual rows."""
    ref = xq @ wq.t()
    if bias is not None:
        ref = ref + bias.double()
    ref = gelu64(ref) if act == ACT_GELU else torch.relu(ref) if act == ACT_RELU else ref
    return ref + res_rows if res_rows is not None else ref


def weight_factor(wq, K):
    """max(1, largest row norm of the weights): magnitude_factor of the rows times sqrt(K) (N(0, 1 / K) rows have norm 1)."""
    return magnitude_factor(wq * math.sqrt(K))


def draw_classes(rng):
    ca, cw = str(rng.choice(CLASSES)), str(rng.choice(CLASSES))
    if ca == "offset" and cw == "offset":  # (outside the fp16 range of operand-format output rows at K = 5120)
        cw = str(rng.choice(["normal", "massive"]))
    return ca, cw


# ----------------------------------------------------------------------------------------------------- GPU cases
def _launch(L, fn, *args):
    try:
        L.call(fn, *args)
    except L.ProbPoseLibraryError as exc:
        if "UNSUPPORTED" in str(exc) or "INVALID" in str(exc):
            raise Refused(str(exc)) from None
        raise
    torch.cuda.synchronize()


_run_twice = FC.run_guarded  # (run_twice; a refusal carries the state of the buffers: exc.faults)


def _pitched(t, pad, fill=float("nan")):
    """(rows, cols) -> (rows, cols + pad) with `fill` in the gap columns (NaN: a kernel that reads them poisons its sums)."""
    return t if not pad else torch.cat([t, torch.full((t.shape[0], pad), fill, dtype=t.dtype, device=t.device)], dim=1)


def _gap_faults(name, snap_t, N):
    """A pitched output (rows, ldc): the gap columns N .. ldc are canaries and every element left of them was written."""
    pat = PATTERN[snap_t.dtype]
    bits = snap_t.contiguous().view({torch.float32: torch.int32, torch.bfloat16: torch.int16}[snap_t.dtype])
    f = []
    if bits.shape[1] > N and not bool((bits[:, N:] == pat).all()):
        f.append(f"{name}: gap columns overwritten")
    if bool((bits[:, :N] == pat).any()):
        f.append(f"{name}: elements left unwritten")
    return f


def _unsplit(t):
    from probpose_code_amd.weights import from_split

    return from_split(t.float().cpu()).double()


def gemm_case(prec, M, N, K, epi, seed, cls_a="normal", cls_w="normal", e=0, planar_P=0, rng=None, ran=None, must_accept=False, pad_a=0, pad_w=0,
              pad_c=0):
    """One guarded launch pair of pp_gemm_ws -> (faults, error / tolerance, description); the kernels that ran are appended to ``ran``.
    ``e``: the weights are stored times 2^e (f16x3 only); None: drawn by draw_e from the weights. ``pad_a`` / ``pad_w`` / ``pad_c``: row pitches
    lda = K + pad_a, ldw = K + pad_w, ldc = N + pad_c (row-major output only); the gap columns of the operands hold NaN, those of the output
    (and of an in-place residual) are canaries that must stay untouched."""
    from probpose_code_amd import _lib as L
    from probpose_code_amd.weights import to_split

    rng = rng if rng is not None else np.random.default_rng(seed)
    g = torch.Generator().manual_seed(int(seed))
    gd = torch.Generator(device="cuda").manual_seed(int(seed))
    fmt, act, res_kind, res_mod = epi["fmt"], epi["act"], epi["res"], epi["res_mod"]
    w = rows_of_class(N, K, cls_w, g, device="cpu") / math.sqrt(K)
    bias = cpu_rand(N, g=g, scale=0.3) if epi["bias"] else None
    x = rows_of_class(M, K, cls_a, gd)
    rows = sample_rows(M, 256, rng)
    e = (draw_e(rng, w) if prec == F16X3 else 0) if e is None else e
    guard = Guard()
    assert not (planar_P and pad_c)
    lda, ldw, ldc = K + pad_a, K + pad_w, N + pad_c
    if prec == F16X3:
        ad, wd = to_split(_pitched(x, pad_a)), to_split(_pitched((w * 2.0 ** e).cuda(), pad_w))
        xq, wq = x[rows].cpu().double(), w.double()
    elif prec == BF16:
        ad, wd = _pitched(x.bfloat16(), pad_a), _pitched(w.bfloat16().cuda(), pad_w)
        xq, wq = ad[rows][:, :K].cpu().double(), w.bfloat16().double()
    else:
        ad, wd = _pitched(x, pad_a), _pitched(w.cuda(), pad_w)
        xq, wq = x[rows].cpu().double(), w.double()
    del x
    ad, wd = guard.inp("act", ad), guard.inp("weight", wd)
    bd = guard.inp("bias", bias) if bias is not None else None
    odt = torch.bfloat16 if fmt == 1 else torch.float32
    oshape = (M // planar_P, N, planar_P) if planar_P else (M, ldc)
    res = rr = None
    if res_kind != "none":
        r = torch.randn(res_mod if res_kind == "table" else M, N, generator=gd, device="cuda")
        rr = r.cpu().double()[rows % res_mod] if res_kind == "table" else r[rows].cpu().double()
        if res_kind == "in_place":
            assert fmt == 0 and not planar_P
            # (the gap columns of a pitched stream start as the canary's NaN payload: they are compared bit for bit below)
            res = out = guard.out("residual/out", oshape, init=_pitched(r, pad_c).view(torch.int32).masked_fill_(
                (torch.arange(ldc, device="cuda") >= N)[None], PATTERN[torch.float32]).view(torch.float32) if pad_c else r)
        else:
            res = guard.inp("residual", _pitched(r, pad_c))  # (the residual's pitch is the output's)
    if res_kind != "in_place":
        out = guard.out("out", oshape, dtype=odt, must_write=not pad_c)
    ref = linear_ref64(xq, wq, bias, act, rr)

    def go():
        _launch(L, "pp_gemm_ws", prec, ad.data_ptr(), wd.data_ptr(), L.ptr(bd), L.ptr(res), res_mod, out.data_ptr(), M, N, K, lda, ldw, ldc, act, fmt,
                planar_P, 2.0 ** -e, None)

    info = (f"{PREC_NAME[prec]} M {M} N {N} K {K} bias {bias is not None} act {act} fmt {fmt} res {res_kind}/{res_mod} planar {planar_P} e {e} "
            f"classes {cls_a} / {cls_w}" + (f" lda {lda} ldw {ldw} ldc {ldc}" if pad_a or pad_w or pad_c else ""))
    L.reset_launch_counts()
    try:
        faults, snap = _run_twice(guard, go)
    except Refused as exc:
        if must_accept:
            return [f"a shape the engine sends was refused: {exc}"], 0.0, info
        raise
    got_k = [k for k in GEMM_KERNELS if L.launch_count(k) > 0]
    want = gemm_kernel(prec, M, N, K, fmt, res is not None, bool(planar_P), lda, ldw, ldc)
    if ran is not None:
        ran += got_k
    if got_k != [want]:
        faults.append(f"kernel {got_k}, the restated dispatcher predicts {want}")
    o = snap[0]
    if planar_P:
        o = o.permute(0, 2, 1).reshape(M, N)
    elif pad_c:
        faults += _gap_faults("out", o, N)
        o = o[:, :N]
    got = _unsplit(o[rows]) if fmt == 2 else o[rows].cpu().double()
    fac = magnitude_factor(xq) * weight_factor(wq, K)
    if prec == F16X3:
        ratio = error_ratio(got, ref, TOL["linear_long"] * fac, TOL["linear_long"] * fac)
    elif prec == F32:
        ratio = error_ratio(got, ref, F32_TOL * fac, F32_TOL * fac)
    elif fmt == 1:
        ratio = bf16_out_ratio(got / fac, ref / fac)  # (2^-8 |ref| + 2e-3 fac)
    else:
        ratio = error_ratio(got, ref, BF16_F32OUT_TOL * fac, BF16_F32OUT_TOL * fac)
    return faults, ratio, f"{info} kernel {want}"


def skinny_codes(N, codes=SKINNY_CODES):
    """The tile codes pp_skinny_linear / pp_skinny_deconv can be forced to at N columns (the tile's columns divide N)."""
    return [c for c in codes if c == 0 or N % (32 * (c % 10)) == 0]


def skinny_case(shape, M, codes, xcd, seed, e=0, rng=None):  # (e: as in gemm_case)
    """pp_skinny_linear at one of SKINNY_SHAPES with the epilogue _layers_small sends (qkv: split rows out; fc1: GELU + split rows; proj / fc2:
    fp32 residual in place + LayerNorm tail; patch: position table + LayerNorm tail): a guarded launch pair per forced tile code ->
    (faults, worst error / tolerance over out and ln_out, description)."""
    from probpose_code_amd import _lib as L
    from probpose_code_amd.weights import to_split

    N, K, layer = shape
    rng = rng if rng is not None else np.random.default_rng(seed)
    g = torch.Generator().manual_seed(int(seed))
    gd = torch.Generator(device="cuda").manual_seed(int(seed))
    ln = layer in ("proj", "fc2", "patch")
    act = ACT_GELU if layer == "fc1" else ACT_NONE
    res_mod = 192 if layer == "patch" else 0
    w, bias = cpu_rand(N, K, g=g, scale=1 / math.sqrt(K)), cpu_rand(N, g=g, scale=0.3)
    x = torch.randn(M, K, generator=gd, device="cuda")
    rows = sample_rows(M, 96, rng)
    xq = x[rows].cpu().double()
    e = draw_e(rng, w) if e is None else e
    guard = Guard()
    ad, wd, bd = guard.inp("act", to_split(x)), guard.inp("weight", to_split((w * 2.0 ** e).cuda())), guard.inp("bias", bias)
    rr = res = gam = bet = ln_out = cnt = None
    if ln:
        gam, bet = guard.inp("gamma", torch.rand(N, generator=g) + 0.5), guard.inp("beta", cpu_rand(N, g=g, scale=0.1))
        r = torch.randn(res_mod if res_mod else M, N, generator=gd, device="cuda")
        rr = r.cpu().double()[rows % res_mod] if res_mod else r[rows].cpu().double()
        if res_mod:
            res, out = guard.inp("residual", r), guard.out("out", (M, N))
        else:
            res = out = guard.out("residual/out", (M, N), init=r)
        ln_out = guard.out("ln_out", (M, N))
        cnt = torch.zeros((M + 31) // 32, dtype=torch.int32, device="cuda")
    else:
        out = guard.out("out", (M, N))
    ref = linear_ref64(xq, w.double(), bias, act, rr)
    ref_h = layernorm64(ref, gam.cpu().double(), bet.cpu().double()) if ln else None
    tol = TOL["linear_long"] * magnitude_factor(xq)

    def go():
        _launch(L, "pp_skinny_linear", ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), L.ptr(res), res_mod, out.data_ptr(), 0 if ln else 2, M, N, K, act,
                2.0 ** -e, L.ptr(gam), L.ptr(bet), 1e-6, L.ptr(ln_out), L.ptr(cnt), None)

    faults, ratio, parts = [], 0.0, []
    for code in codes:
        L.set_option("skinny_tile", code)
        L.set_option("skinny_xcd_order", xcd)
        guard.rearm()
        f, snap = run_twice(guard, go)
        outs = {id(o[5]): s for o, s in zip(guard.outs, snap)}
        if cnt is not None and int(cnt.abs().sum()) != 0:
            f.append("arrival counters not back at zero")
            cnt.zero_()
        o = outs[id(out)][rows]
        r_out = error_ratio(o.cpu().double() if ln else _unsplit(o), ref, tol, tol)
        r_ln = error_ratio(_unsplit(outs[id(ln_out)][rows]), ref_h, LN_TAIL_TOL, LN_TAIL_TOL) if ln else 0.0
        parts.append(f"{code}: {r_out:.3g}" + (f" / {r_ln:.3g}" if ln else ""))
        ratio = max(ratio, r_out, r_ln)
        faults += [f"tile {code}: {x_}" for x_ in f]
    return faults, ratio, f"{layer} M {M} N {N} K {K} xcd_order {xcd} e {e} (tile: out{' / ln_out' if ln else ''} {', '.join(parts)})"


def _deconv_operands(prec, Cin, nb, cls, seed, rng, H=MAP_H, W=MAP_W, cout=DECONV_COUT):
    """Activations (nb, H, W, Cin) on the GPU (16 x 12 unless given), phase matrices, shift; and the fp64 values of two or three images and of
    the torch weight the kernel multiplies (bf16-rounded for bf16)."""
    from probpose_code_amd.weights import to_split

    g = torch.Generator().manual_seed(int(seed))
    gd = torch.Generator(device="cuda").manual_seed(int(seed))
    if cls == "border":
        x = FC.border_impulses(nb, H, W, Cin, g).cuda()
    else:
        x = rows_of_class(nb * H * W, Cin, cls, gd).reshape(nb, H, W, Cin)
    w = cpu_rand(Cin, cout, 4, 4, g=g, scale=1 / math.sqrt(4 * Cin))
    shift = cpu_rand(cout, g=g, scale=0.3)
    ph = deconv_phases(w)  # (2, 2, Cout, 4 Cin)
    imgs = torch.unique(torch.tensor([0, nb - 1, int(rng.integers(0, nb))]))
    if prec == F16X3:
        xd, wd, xq, wq = to_split(x), to_split(ph.cuda()), x[imgs].cpu().double(), w.double()
    elif prec == BF16:
        xd, wd = x.bfloat16(), ph.bfloat16().cuda()
        xq, wq = xd[imgs].cpu().double(), w.bfloat16().double()
    else:
        xd, wd, xq, wq = x, ph.cuda(), x[imgs].cpu().double(), w.double()
    return xd, wd, shift, imgs, xq, wq


def deconv_case(prec, Cin, nb, phase, seed, act=ACT_RELU, fmt=None, bias=True, cls="normal", weight_major=0, rng=None, ran=None, H=MAP_H, W=MAP_W,
                cout=DECONV_COUT, only_phase=False):
    """pp_conv_gemm PP_DECONV4X4S2 at the first head deconvolution (nb, 16, 12, Cin) -> (nb, 32, 24, 256) - or at the map ``H`` x ``W`` and the
    ``cout`` output channels given: all four phases in one launch (phase < 0) or one launch each, `phase` first (``only_phase``: that one phase
    alone; the pixels of the three others are canaries that must stay untouched). ``weight_major``: option "psplit_deconv_weight_major" -
    honoured only while a phase's weight set (4 Cin x 256 x 4 bytes) is at most 3 MiB, Cin = 768; above, the wide-tile kernel falls back to
    its row-major tile order."""
    from probpose_code_amd import _lib as L

    rng = rng if rng is not None else np.random.default_rng(seed)
    fmt = OPERAND_FMT[prec] if fmt is None else fmt
    MAP_H, MAP_W, DECONV_COUT = H, W, cout  # (the names the body below was written with)
    xd, wd, shift, imgs, xq, wq = _deconv_operands(prec, Cin, nb, cls, seed, rng, H, W, cout)
    guard = Guard()
    xd, wd = guard.inp("act", xd), guard.inp("weight", wd)
    bd = guard.inp("bias", shift) if bias else None
    out = guard.out("out", (nb, 2 * MAP_H, 2 * MAP_W, DECONV_COUT), dtype=torch.bfloat16 if fmt == 1 else torch.float32, must_write=not only_phase)
    wflat = wd.reshape(4, DECONV_COUT, -1)

    def go():
        if phase < 0:
            _launch(L, "pp_conv_gemm", prec, DECONV, xd.data_ptr(), wd.data_ptr(), L.ptr(bd), out.data_ptr(), nb, MAP_H, MAP_W, Cin, DECONV_COUT, -1, 0,
                    1, 0, 0, 0, 0, DECONV_COUT, act, fmt, None)
        else:
            for k in range(1 if only_phase else 4):
                py, px = divmod((phase + k) % 4, 2)
                _launch(L, "pp_conv_gemm", prec, DECONV, xd.data_ptr(), wflat[2 * py + px].data_ptr(), L.ptr(bd), out.data_ptr(), nb, MAP_H, MAP_W, Cin,
                        DECONV_COUT, py, px, 1, 0, 0, 0, 0, DECONV_COUT, act, fmt, None)

    if weight_major:
        L.set_option("psplit_deconv_weight_major", 1)
    L.reset_launch_counts()
    faults, snap = _run_twice(guard, go)
    got_k = [k for k in FC.KERNELS if L.launch_count(k) > 0]
    want = FC.conv_kernel(prec, DECONV, nb, MAP_H, MAP_W, Cin, DECONV_COUT, 4 if phase < 0 else 1, fmt, act, FC.DEFAULT_OPTIONS)
    if ran is not None:
        ran += got_k
    if got_k != [want]:
        faults.append(f"kernel {got_k}, the mirrored dispatcher predicts {want}")
    ref = FC.act64(deconv64(xq.permute(0, 3, 1, 2), wq, shift.double() if bias else None), act)
    got = (_unsplit(snap[0][imgs]) if fmt == 2 else snap[0][imgs].cpu().double()).permute(0, 3, 1, 2)
    if only_phase:  # the one phase written whole, the three others still canaries (bit for bit, the whole batch)
        py, px = divmod(phase, 2)
        pat = PATTERN[snap[0].dtype]
        bits = snap[0].view(torch.int16 if fmt == 1 else torch.int32)
        mine = torch.zeros(2 * MAP_H, 2 * MAP_W, dtype=torch.bool, device="cuda")
        mine[py::2, px::2] = True
        if bool((bits[:, mine] == pat).any()):
            faults.append("out: elements of the phase left unwritten")
        if not bool((bits[:, ~mine] == pat).all()):
            faults.append("out: pixels of another phase overwritten")
        got, ref = got[:, :, py::2, px::2], ref[:, :, py::2, px::2]
    fac = magnitude_factor(xq.reshape(-1, Cin))
    if prec == F16X3:
        ratio = error_ratio(got, ref, HEAD_TOL["deconv_head"] * fac, HEAD_TOL["deconv_head"] * fac)
    elif prec == F32:
        ratio = error_ratio(got, ref, F32_TOL * fac, F32_TOL * fac)
    elif fmt == 1:
        ratio = bf16_out_ratio(got / fac, ref / fac)
    else:
        ratio = error_ratio(got, ref, BF16_F32OUT_TOL * fac, BF16_F32OUT_TOL * fac)
    return faults, ratio, (f"{PREC_NAME[prec]} deconv nb {nb} {MAP_H}x{MAP_W} Cin {Cin} Cout {DECONV_COUT} phase {phase}{' alone' if only_phase else ''} "
                           f"bias {bias} act {act} fmt {fmt} class {cls} weight_major {weight_major} kernel {want}")


def skinny_deconv_case(Cin, nb, code, seed, cls="normal", rng=None, H=MAP_H, W=MAP_W, cout=DECONV_COUT):
    """pp_skinny_deconv (f16x3, shift + ReLU, split rows out) on nb x 192 <= 1 536 input pixels (or nb maps of ``H`` x ``W``, ``cout`` output
    channels), tile code forced (0: the cost model's)."""
    from probpose_code_amd import _lib as L

    rng = rng if rng is not None else np.random.default_rng(seed)
    MAP_H, MAP_W, DECONV_COUT = H, W, cout
    xd, wd, shift, imgs, xq, wq = _deconv_operands(F16X3, Cin, nb, cls, seed, rng, H, W, cout)
    guard = Guard()
    xd, wd, bd = guard.inp("act", xd), guard.inp("weight", wd), guard.inp("bias", shift)
    out = guard.out("out", (nb, 2 * MAP_H, 2 * MAP_W, DECONV_COUT))

    def go():
        _launch(L, "pp_skinny_deconv", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), nb, MAP_H, MAP_W, Cin, DECONV_COUT, None)

    L.set_option("skinny_tile", code)
    L.reset_launch_counts()
    faults, snap = _run_twice(guard, go)
    if L.launch_count("skinny_deconv") != 2:
        faults.append(f"pp_launch_count('skinny_deconv') = {L.launch_count('skinny_deconv')} after two launches")
    ref = torch.relu(deconv64(xq.permute(0, 3, 1, 2), wq, shift.double()))
    got = _unsplit(snap[0][imgs]).permute(0, 3, 1, 2)
    tol = HEAD_TOL["deconv_head"] * magnitude_factor(xq.reshape(-1, Cin))
    return faults, error_ratio(got, ref, tol, tol), f"skinny deconv nb {nb} {MAP_H}x{MAP_W} Cin {Cin} Cout {DECONV_COUT} tile {code} class {cls}"


# ----------------------------------------------------------------------------------------------------- the fuzzer
def draw_m(rng, N, CU, cap):
    """M on both sides of each dispatch threshold of N columns, tile counts around multiples of the CU count, M = 1, ragged against 128 / 192 /
    256, a row count the engine sends, or random."""
    c = [1, int(rng.integers(1, 30000)), 384 * int(rng.integers(1, 65))]
    for bm in (128, 192, 256):
        t = int(rng.integers(1, 40))
        c += [bm * t - int(rng.integers(0, 3)), bm * t + int(rng.integers(1, bm))]
    ct = N // 192 if N % 192 == 0 else (N + 127) // 128
    bm = 192 if N % 192 == 0 else 128
    rt = max(1, (int(rng.integers(1, 6)) * CU + int(rng.integers(-3, 4))) // ct)
    c += [bm * rt - int(rng.integers(0, bm)), bm * rt + int(rng.integers(1, bm))]
    if N % 192 == 0:
        for t in (dma_threshold(N), wide_threshold(N)):
            c += [t - 1 - int(rng.integers(0, 192)), t - 1, t, t + int(rng.integers(1, 192))] * 2
    return max(1, min(int(rng.choice(c)), cap))


def m_for_kernel(kernel, N, rng):
    """A row count that lands an f16x3 qkv shape (N % 192 == 0) on the named kernel."""
    d, w = dma_threshold(N), wide_threshold(N)
    if kernel == "linear_dma_tile":
        return d + int(rng.integers(0, 400))
    if kernel == "pp_panel_split.hip":
        return int(rng.integers(w, d))
    return int(rng.choice([1, 385, w - 1, int(rng.integers(1, w))]))


def _main(seconds):
    from probpose_code_amd import _lib as L

    CU = int(L.lib.pp_device_cu_count())
    names = list(TABLE)
    table = {}  # (precision, (arch, layer), kernel) -> accepted cases
    visits = {}

    def case_gemm(prec):
        def run(rng, g):
            v = visits[prec] = visits.get(prec, -1) + 1
            # the cells the summary asks for first (a run of a few seconds fills them), then every other visit; in between free draws
            cells = [(n, "pp_gemm.hip") for n in names if n[1] != "qkv"]
            if prec == F16X3:
                cells = [(n, k) for n in names if n[1] == "qkv" for k in GEMM_KERNELS] + cells
            target = cells[v] if v < len(cells) else (cells[(v // 2) % len(cells)] if v % 2 == 0 else None)
            name = None
            cls_a, cls_w = draw_classes(rng)
            planar = 0
            if target is not None or rng.random() < 0.5:
                name = target[0] if target is not None else names[int(rng.integers(0, len(names)))]
                N, K = TABLE[name]
                epi = engine_epilogue(name[1], prec)
                cap = int(MEM_CAP // (4 * (2 * N + K) * 3))
                if target is not None and name[1] == "qkv":
                    M = m_for_kernel(target[1], N, rng)
                elif target is not None:
                    M = int(rng.choice([1, 385, 384 * int(rng.integers(1, 9)), int(rng.integers(1, 2000))]))
                else:
                    M = draw_m(rng, N, CU, cap)
            else:
                K = 128 * int(rng.integers(1, 41)) if prec == BF16 else 32 * int(rng.integers(2, 161))
                N = 32 * int(rng.choice([1, 2, 6, 12, 18, 24, 32, 36, 40, 48, 72, 96, 120, 128, 160, int(rng.integers(1, 161))]))
                fmt = 0 if rng.random() < 0.5 else OPERAND_FMT[prec]
                kind = int(rng.integers(0, 3))  # tests/fuzz_gemm.py: none; fp32 rows (in place where the output is fp32 too); broadcast table
                epi = dict(bias=rng.random() < 0.8, act=int(rng.integers(0, 3)), fmt=fmt,
                           res=("none", "in_place" if fmt == 0 else "f32", "table")[kind], res_mod=int(rng.choice([1, 7, 192])) if kind == 2 else 0)
                if kind == 1 and fmt == 0 and rng.random() < 0.3:
                    epi["res"] = "f32"  # (a separate residual tensor with fp32 output)
                cap = int(MEM_CAP // (4 * (2 * N + K) * 3))
                M = draw_m(rng, N, CU, cap)
                if rng.random() < 0.1:  # planar planes: the final 1x1 convolution's layout, fp32 only
                    N, planar = 17, int(rng.choice([64, 3072]))
                    M = planar * max(1, min(M, 20000) // planar)
                    epi = dict(bias=epi["bias"], act=epi["act"], fmt=0, res="none", res_mod=0)
            engine_m = name is not None and M % 384 == 0 and M <= 64 * 384
            ran = []
            faults, ratio, info = gemm_case(prec, M, N, K, epi, int(rng.integers(1 << 30)), cls_a, cls_w, None, planar, rng, ran, must_accept=engine_m)
            if name is not None and not faults:
                for k in ran:
                    table[(PREC_NAME[prec], name, k)] = table.get((PREC_NAME[prec], name, k), 0) + 1
            return faults, ratio, (f"{name[0]} {name[1]}: " if name else "") + info
        return run

    def case_skinny(rng, g):
        v = visits["skinny"] = visits.get("skinny", -1) + 1
        shape = SKINNY_SHAPES[v % len(SKINNY_SHAPES)]
        codes = skinny_codes(shape[0])
        code = codes[(v // len(SKINNY_SHAPES)) % len(codes)]
        M = int(rng.choice(SKINNY_M + [int(rng.integers(1, 7000))]))
        return skinny_case(shape, M, [code], int(rng.integers(0, 2)), int(rng.integers(1 << 30)), None, rng)

    def case_deconv(prec):
        def run(rng, g):
            Cin = int(rng.choice(DECONV_CIN))
            phase = int(rng.integers(-1, 4))
            t = deconv_threshold(phase)
            nb = int(rng.choice([1, 2, t - 1, t, t + 1, int(rng.integers(1, t + 2)), int(rng.integers(1, 9))]))
            fmt = int(rng.choice({BF16: [0, 1], F32: [0], F16X3: [0, 2]}[prec]))
            cls = str(rng.choice(["normal", "massive", "border"] if nb <= 8 else ["normal", "massive"]))
            return deconv_case(prec, Cin, nb, phase, int(rng.integers(1 << 30)), act=int(rng.integers(0, 3)), fmt=fmt, bias=rng.random() < 0.7, cls=cls,
                               weight_major=int(rng.integers(0, 2)) if prec != F32 else 0, rng=rng)
        return run

    def case_skinny_deconv(rng, g):
        v = visits["skinny_deconv"] = visits.get("skinny_deconv", -1) + 1
        return skinny_deconv_case(int(rng.choice(DECONV_CIN)), int(rng.integers(1, 9)), SKINNY_DECONV_CODES[v % len(SKINNY_DECONV_CODES)],
                                  int(rng.integers(1 << 30)), cls=str(rng.choice(["normal", "massive", "border"])), rng=rng)

    gemm = {p: (f"pp_gemm_ws {PREC_NAME[p]}", case_gemm(p)) for p in (F16X3, BF16, F32)}
    others = [("pp_skinny_linear (ViT-L shapes)", case_skinny), ("pp_conv_gemm deconv f16x3", case_deconv(F16X3)), ("pp_conv_gemm deconv bf16", case_deconv(BF16)),
              ("pp_conv_gemm deconv f32", case_deconv(F32)), ("pp_skinny_deconv", case_skinny_deconv)]
    # run_entries visits every list element once whatever the time: the pp_gemm_ws entries are listed as often as the summary has cells to fill
    entries = []
    for i in range(14):
        entries += [gemm[F16X3]] + ([gemm[BF16], gemm[F32]] if i < 8 else []) + ([others[i]] if i < len(others) else [])

    def summary():
        """(precision, table shape) x kernel; fails unless every kernel accepted an f16x3 case at both qkv shapes and the 128 x 128 kernel every
        other table shape in each precision."""
        print(f"{'precision, table shape':36s} " + " ".join(f"{k:>20s}" for k in GEMM_KERNELS))
        empty = []
        for p in ("f16x3", "bf16", "f32"):
            for n in names:
                print(f"{p + ', ' + n[0] + ' ' + n[1] + ' ' + str(TABLE[n]):36s} " + " ".join(f"{table.get((p, n, k), 0):20d}" for k in GEMM_KERNELS))
                need = GEMM_KERNELS if (p == "f16x3" and n[1] == "qkv") else () if n[1] == "qkv" else ("pp_gemm.hip",)
                empty += [f"{p}, {n[0]} {n[1]} -> {k}" for k in need if not table.get((p, n, k))]
        for e_ in empty:
            print(f"EMPTY CELL {e_}")
        return empty

    return run_entries(entries, seconds, 130000, "WIDE", L, summary=summary)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sys.exit(_main(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0))


if __name__ == "__main__":
    main()
