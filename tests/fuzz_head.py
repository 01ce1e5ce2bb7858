#!/usr/bin/env python
"""Fuzz of the heatmap-head and scalar-tower kernels of the split-fp16 (f16x3) plans against torch fp64 on the unrounded inputs, visited round robin:
pp_deconv_head_split (32 x 24 and 48 x 36 inputs, B from the 192-tile minimum up, 1 - 28 maps), pp_conv3x3_winograd_maxpool_relu (16 x 12 / 24 x 18
maps, 384 / 768 channels, 1 - 4 towers, option wino_order), pp_conv3x3_splitk + pp_sum_maxpool_relu_nhwc (the library's slice count and 1 / 3 / 9,
option ksplit_channels), pp_conv3x3_maxpool_relu (option conv_pool_split) and pp_tower_final (one / two passes, every feature format, err_div).
Every case: outputs, partial sums and scratch buffers between canaries (compared bit for bit), every output element written, inputs bit-identical
after the launch, a repeat launch bit-identical, fp64 accuracy with the fixed-shape tests' tolerances (tests/test_split_fp16.py) - on a sample of
images and output channels where the fp64 convolution of the whole batch would take minutes; the device side is checked whole.
Refusals are counted; a shape the engine sends is never refused.   python tests/fuzz_head.py [seconds]"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from fuzz_layer import (F16X3, MEM_CAP, SPLIT, Guard, Refused, bits_equal, cpu_rand, error_ratio, magnitude_factor,  # noqa: E402
                        run_entries)

# tolerances (rtol = atol) of the fixed-shape tests, tests/test_split_fp16.py
TOL = dict(deconv_head=3e-5, winograd=5e-5, splitk=2e-5, conv_pool=2e-5, tower_final=1e-5, tower_final_atol=1e-6)


# ----------------------------------------------------------------------------------------------------- fp64 references (imported by the CPU test)
def deconv_phases(w):
    """ConvTranspose2d(k4, s2, p1) weights (Cin, Cout, 4, 4) -> the four phase matrices (2, 2, Cout, 4 Cin) of PP_DECONV4X4S2: output pixel
    (2y + py, 2x + px) = sum over taps (ty, tx) of x[y + py - 1 + ty ... ] - the layout of tests/test_split_fp16.py."""
    Cin, Cout = w.shape[:2]
    ph = torch.empty((2, 2, Cout, 4 * Cin), dtype=w.dtype)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    t = ty * 2 + tx
                    ph[py, px, :, t * Cin:(t + 1) * Cin] = w[:, :, 3 - 2 * ty - py, 3 - 2 * tx - px].t()
    return ph


def deconv_head64(x, w, b, wf, bf):
    """x (B, Cin, H, W); ConvTranspose2d(k4, s2, p1) + bias + ReLU, then the 1x1 convolution wf (K, Cout) + bf -> (B, K, 2H, 2W). Written out as
    its four output phases, each a 2 x 2 convolution over the zero-padded input."""
    B, Cin, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    mid = torch.empty((B, w.shape[1], 2 * H, 2 * W), dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            acc = 0
            for ty in range(2):
                for tx in range(2):
                    ky, kx = 3 - 2 * ty - py, 3 - 2 * tx - px
                    patch = xp[:, :, py + ty:py + ty + H, px + tx:px + tx + W]
                    acc = acc + torch.einsum("bchw,co->bohw", patch, w[:, :, ky, kx])
            mid[:, :, py::2, px::2] = acc
    mid = torch.relu(mid + b.view(1, -1, 1, 1))
    return torch.einsum("bchw,kc->bkhw", mid, wf) + bf.view(1, -1, 1, 1)


def conv3x3_64(x, w, b=None):
    """x (B, Cin, H, W), w (Cout, Cin, 3, 3), zero padding 1 -> (B, Cout, H, W), written out as nine shifted products."""
    B, Cin, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = sum(torch.einsum("bchw,oc->bohw", xp[:, :, i:i + H, j:j + W], w[:, :, i, j]) for i in range(3) for j in range(3))
    return out + b.view(1, -1, 1, 1) if b is not None else out


def pool_relu64(y, ph, pw):
    B, C, H, W = y.shape
    return torch.relu(y.reshape(B, C, H // ph, ph, W // pw, pw).amax(dim=(3, 5)))


def tower_final64(feat, w, bias, flip_indices, B, passes, err_div):
    """feat (4, passes * B, C), w (4, K, C), bias (4, K) -> (4, B, K): sigmoid for the first three towers, ReLU for the error tower (divided by
    err_div), the flip pass mapped back through flip_indices and averaged."""
    z = torch.einsum("tbc,tkc->tbk", feat, w) + bias[:, None]
    a = torch.cat([torch.sigmoid(z[:3]), torch.relu(z[3:]) / err_div])
    return a if passes == 1 else (a[:, :B] + a[:, B:][:, :, flip_indices]) * 0.5


# ----------------------------------------------------------------------------------------------------- non-finite poison (imported by tests/fuzz_conv.py)
# The NaN contract of the towers (include/probpose_mi355x.h, numeric domain): a value out of range must come out as NaN / inf, never be pooled
# away. Poisoned inputs hold a few +inf, -inf or canonical NaN elements (never the canary payloads). What a case then asserts:
#   * every output whose fp64 reference is non-finite is non-finite;
#   * an output may be non-finite where the reference is finite only inside the poison's REACH: the outputs whose receptive field holds a
#     poisoned input (a split-fp16 operand of +-inf is hi = inf, lo = NaN, so the kernel's product is NaN where fp64 has +-inf, which a max
#     may discard). For a 3x3 convolution the reach is the 3x3 neighbourhood of the poisoned pixels; for the Winograd F(2x2, 3x3) form it is
#     every 2 x 2 output tile whose 4 x 4 input tile holds one (the input transform mixes the whole tile); pooling then takes the windows
#     that hold a reached output;
#   * every output finite on both sides meets the normal tolerance.
def poison_(x, g, n):
    """In place: n random elements of x set to +inf, -inf and canonical NaN in turn."""
    for i in range(n):
        idx = tuple(int(torch.randint(0, d, (1,), generator=g)) for d in x.shape)
        x[idx] = (math.inf, -math.inf, math.nan)[i % 3]
    return x


def bad_pixels(x):
    """(B, H, W, C) NHWC -> (B, H, W) bool: pixels with a non-finite channel."""
    return ~torch.isfinite(x.double()).all(dim=-1)


def conv_reach(bad, ph=1, pw=1, winograd=False):
    """bad (B, H, W) -> (B, 1, H // ph, W // pw) bool: pooled 3x3-convolution outputs a poisoned pixel can reach (ph = pw = 1: no pooling)."""
    i = bad.double()[:, None]
    if winograd:  # output tile (ty, tx) reads input rows 2 ty - 1 .. 2 ty + 2 (and the columns alike)
        H, W = bad.shape[1:]
        t = F.max_pool2d(F.pad(i, (1, 1, 1, 1)), 4, 2)[:, :, :H // 2, :W // 2]
        r = t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    else:
        r = F.max_pool2d(i, 3, 1, 1)
    B, _, H, W = r.shape
    r = r[:, :, :H // ph * ph, :W // pw * pw].reshape(B, 1, H // ph, ph, W // pw, pw).amax(dim=(3, 5))
    return r > 0


def poison_ratio(got, ref, reach, rtol, atol):
    """error / tolerance of a poisoned case (inf when a non-finite reference came out finite, or a non-finite output lies outside the reach)."""
    got, ref = got.double(), ref.double()
    fg, fr = torch.isfinite(got), torch.isfinite(ref)
    reach = reach.expand_as(got)
    if bool((~fr & fg).any()) or bool((~fg & ~reach).any()):
        return math.inf
    both = fg & fr
    return error_ratio(got[both], ref[both], rtol, atol)


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


def run_twice(guard, go):
    go()
    faults = guard.faults()
    first = guard.snapshot()
    guard.rearm()
    go()
    if not bits_equal(first, guard.snapshot()):
        faults.append("repeat launch differs")
    faults += [f for f in guard.faults() if f not in faults]
    return faults, first


def pick(n, rng, k):
    return torch.unique(torch.tensor([0, n - 1] + rng.integers(0, n, k).tolist())) if n > k + 2 else torch.arange(n)


def run_guarded(guard, go):
    """run_twice; a refusal (Refused) carries what the buffers show at that moment: exc.faults names every canary, output element or input that
    changed although the library refused the launch."""
    try:
        return run_twice(guard, go)
    except Refused as exc:
        torch.cuda.synchronize()
        f = [x for x in guard.faults() if not x.endswith("elements left unwritten")]
        for name, full, n, init, _, _, pat in guard.outs:
            if init is None and bool((full != pat).any()):
                f.append(f"{name}: written by a refused launch")
        exc.faults = f
        raise


def deconv_head_split_case(B, H, W, Cin, K, rng, g, must_accept=False):
    """One guarded launch pair of pp_deconv_head_split (f16x3: the last deconvolution to 256 channels + ReLU + the 1x1 convolution to K maps,
    logits in the phase-separated layout) -> (faults, error / tolerance, description). ``must_accept``: a refusal is a fault."""
    from probpose_code_amd.weights import pack_head_split

    Cout = 256
    gd = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
    x = torch.randn(B, H, W, Cin, generator=gd, device="cuda")
    w = cpu_rand(Cin, Cout, 4, 4, g=g, scale=1 / math.sqrt(4 * Cin))
    b = cpu_rand(Cout, g=g, scale=0.2)
    wf, bf = cpu_rand(K, Cout, g=g, scale=4 / math.sqrt(Cout)), cpu_rand(K, g=g)
    wpad = torch.zeros(32, Cout)
    wpad[:K] = wf
    guard = Guard()
    xd, phd, bd = guard.inp("act", sp(x)), guard.inp("weight", sp(deconv_phases(w))), guard.inp("bias", b)
    hwd, bfd = guard.inp("head_w", pack_head_split(wpad)), guard.inp("head_b", bf)
    lg = guard.out("logits", (B, K, 4, H * W))

    def go():
        launch("pp_deconv_head_split", xd.data_ptr(), phd.data_ptr(), bd.data_ptr(), hwd.data_ptr(), bfd.data_ptr(), lg.data_ptr(), B, H, W, Cin,
               Cout, K, None)
    try:
        faults, snap = run_guarded(guard, go)
    except Refused:
        if must_accept:
            return ["a shape with enough tiles was refused"], 0.0, f"B {B} {H}x{W} K {K}"
        raise
    imgs = pick(B, rng, 1)
    ref = deconv_head64(x[imgs].permute(0, 3, 1, 2).cpu().double(), w.double(), b.double(), wf.double(), bf.double())
    got = snap[0][imgs].cpu().reshape(len(imgs), K, 2, 2, H, W).permute(0, 1, 4, 2, 5, 3).reshape(len(imgs), K, 2 * H, 2 * W)
    return faults, error_ratio(got, ref, TOL["deconv_head"], TOL["deconv_head"]), f"B {B} {H}x{W} K {K}"


def splitk_case(B, H, W, Cin, C, G, ks, rng, g, lib_s=None, chans=None):
    """One guarded launch pair of pp_conv3x3_splitk (f16x3, Cin -> C channels, G towers, ks slices) + pp_sum_maxpool_relu_nhwc (2 x 2 windows)
    -> (faults, error / tolerance, description). ``lib_s``: the library's own slice count (refusing it is a fault); ``chans``: the
    "ksplit_channels" option the caller has set, for the description."""
    gd = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
    x = torch.randn(G, B, H, W, Cin, generator=gd, device="cuda")
    shared = rng.random() < 0.5  # the four towers on one input (stride 0) or each on its own
    poisoned = rng.random() < 0.25
    if poisoned:
        for k in range(G):
            for i in {0, B - 1}:
                poison_(x[k, i], g, int(rng.integers(1, 3)))
    w = cpu_rand(G, C, Cin, 3, 3, g=g, scale=1 / math.sqrt(9 * Cin))
    b = cpu_rand(G, C, g=g)
    guard = Guard()
    xd = guard.inp("act", sp(x[0] if shared else x))
    wd = guard.inp("weight", sp(w.permute(0, 1, 3, 4, 2).reshape(G, C, 9 * Cin)))
    bd = guard.inp("bias", b)
    part = guard.out("partials", (ks, G, B, H, W, C))
    pooled = guard.out("pooled", (G * B, H // 2, W // 2, C))

    def go():
        launch("pp_conv3x3_splitk", F16X3, xd.data_ptr(), wd.data_ptr(), part.data_ptr(), B, H, W, Cin, C, G, 0 if shared else B * H * W * Cin,
               C * 9 * Cin, ks, None)
        launch("pp_sum_maxpool_relu_nhwc", part.data_ptr(), ks, G * B * H * W * C, bd.data_ptr(), B, pooled.data_ptr(), SPLIT, G * B, H, W, C, 2, 2,
               None)
    try:
        faults, snap = run_guarded(guard, go)
    except Refused:
        if ks == lib_s:
            return ["the library's own slice count was refused"], 0.0, f"B {B} {H}x{W} C {C} slices {ks}"
        raise
    imgs, ch = pick(B, rng, 2), torch.from_numpy(rng.choice(C, min(C, 64), replace=False))
    ratio = 0.0
    for k in range(G):
        xk = (x[0] if shared else x[k])[imgs].cpu()
        xi = xk.permute(0, 3, 1, 2).double()
        conv = conv3x3_64(xi, w[k][ch].double())
        psum = snap[0][:, k][:, imgs][..., ch].cpu().double().sum(0).permute(0, 3, 1, 2)
        pref = pool_relu64(conv + b[k][ch].double().view(1, -1, 1, 1), 2, 2)
        pg = unsp(snap[1].view(G, B, H // 2, W // 2, C)[k][imgs])[..., ch].permute(0, 3, 1, 2)
        if poisoned:
            bad = bad_pixels(xk)
            ratio = max(ratio, poison_ratio(psum, conv, conv_reach(bad), TOL["splitk"], TOL["splitk"]),
                        poison_ratio(pg, pref, conv_reach(bad, 2, 2), TOL["splitk"], TOL["splitk"]))
        else:
            ratio = max(ratio, error_ratio(psum, conv, TOL["splitk"], TOL["splitk"]), error_ratio(pg, pref, TOL["splitk"], TOL["splitk"]))
    return faults, ratio, f"B {B} {H}x{W} C {C}{'' if Cin == C else f' Cin {Cin}'} slices {ks} (library {lib_s}) ksplit_channels {chans} shared {shared} poison {poisoned}"


def _main(seconds):
    from probpose_code_amd import _lib as L
    from probpose_code_amd.weights import from_split, pack_head_split, to_split, winograd_weights

    # ------------------------------------------------------------------------------------------------- deconvolution + 1x1 head
    def case_deconv_head(rng, g):
        H, W = [(32, 24), (48, 36)][int(rng.integers(0, 2))]
        Cin, Cout = 256, 256
        tiles_per_img = H * W / 192.0
        b_min = math.ceil(48 / tiles_per_img)  # 4 * ceil(B H W / 192) >= 192
        B = int(rng.choice([b_min - 1, b_min, b_min + 1, 64, 128, int(rng.integers(b_min, 301))]))
        B = max(1, min(B, int(MEM_CAP // (H * W * (Cin * 4 + 28 * 16) * 2))))
        K = int(rng.integers(1, 29))
        return deconv_head_split_case(B, H, W, Cin, K, rng, g, must_accept=B >= b_min)

    # ------------------------------------------------------------------------------------------------- first tower stage, Winograd form
    def case_winograd(rng, g):
        H, W = [(16, 12), (24, 18)][int(rng.integers(0, 2))]
        C = int(rng.choice([384, 768]))
        G = int(rng.integers(1, 5))
        B = int(rng.choice([1, 2, 5, 6, 7, 8, 64, 128, int(rng.integers(1, 301))]))
        per_img = H * W * C * 4 * (1 + 4) + (H // 2) * (W // 2) * C * 64
        B = max(1, min(B, int(MEM_CAP // per_img)))
        order = int(rng.choice([-1, 0]))
        gd = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
        x = torch.randn(B, H, W, C, generator=gd, device="cuda")
        poisoned = rng.random() < 0.25
        if poisoned:  # first and last image: both are in the sample the reference is computed on
            for i in {0, B - 1}:
                poison_(x[i], g, int(rng.integers(1, 4)))
        w = cpu_rand(G, C, C, 3, 3, g=g, scale=1 / math.sqrt(9 * C))
        b = cpu_rand(G, C, g=g, scale=0.3)
        guard = Guard()
        xd = guard.inp("act", sp(x))
        ud = guard.inp("u", sp(torch.stack([winograd_weights(w[k]) for k in range(G)])))
        bd = guard.inp("bias", b)
        nbytes = int(L.lib.pp_winograd_scratch_bytes(B, H, W, C))
        scratch = guard.out("scratch", (nbytes // 4,), must_write=False)
        out = guard.out("out", (G, B, H // 4, W // 3, C))

        def go():
            launch("pp_conv3x3_winograd_maxpool_relu", xd.data_ptr(), ud.data_ptr(), bd.data_ptr(), scratch.data_ptr(), out.data_ptr(), B, H, W, C, C,
                   4, 3, G, None)
        if order == 0:
            L.set_option("wino_order", 0)
        faults, snap = run_twice(guard, go)
        imgs, ch = pick(B, rng, 1), torch.from_numpy(rng.choice(C, 48, replace=False))
        xi = x[imgs].permute(0, 3, 1, 2).cpu().double()
        ref = torch.stack([pool_relu64(conv3x3_64(xi, w[k][ch].double(), b[k][ch].double()), 4, 3) for k in range(G)])
        got = unsp(snap[1])[:, imgs][..., ch].permute(0, 1, 4, 2, 3)
        if poisoned:
            ratio = poison_ratio(got, ref, conv_reach(bad_pixels(x[imgs].cpu()), 4, 3, winograd=True)[None], TOL["winograd"], TOL["winograd"])
        else:
            ratio = error_ratio(got, ref, TOL["winograd"], TOL["winograd"])
        return faults, ratio, f"B {B} {H}x{W} C {C} G {G} wino_order {'default' if order else 0} poison {poisoned}"

    # ------------------------------------------------------------------------------------------------- split-K tower stages
    def case_splitk(rng, g):
        H, W = [(4, 4), (2, 2), (8, 6)][int(rng.integers(0, 3))]
        C = int(rng.choice([384, 768]))
        G = 4
        B = int(rng.choice([1, 8, 64, 128, 272, int(rng.integers(1, 301))]))
        chans = int(rng.integers(0, 2))
        L.set_option("ksplit_channels", chans)
        lib_s = int(L.lib.pp_conv3x3_splitk_slices(F16X3, B, H, W, C, C, G))
        ks = int(rng.choice([lib_s, lib_s, 1, 3, 9]))
        B = max(1, min(B, int(MEM_CAP // (G * H * W * C * 4 * (ks + 2)))))
        return splitk_case(B, H, W, C, C, G, ks, rng, g, lib_s=lib_s, chans=chans)

    # ------------------------------------------------------------------------------------------------- fused conv + pool, implicit GEMM
    def case_conv_pool(rng, g):
        H, W, C, G = 16, 12, 384, 4
        B = int(rng.choice([1, 6, 23, 24, 25, 33, 64, int(rng.integers(1, 129))]))
        fused = int(rng.integers(0, 2))
        gd = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
        x = torch.randn(B, H, W, C, generator=gd, device="cuda")
        poisoned = rng.random() < 0.25
        if poisoned:
            for i in {0, B - 1}:
                poison_(x[i], g, int(rng.integers(1, 4)))
        w = cpu_rand(G, C, C, 3, 3, g=g, scale=1 / math.sqrt(9 * C))
        b = cpu_rand(G, C, g=g)
        guard = Guard()
        xd = guard.inp("act", sp(x))
        wd = guard.inp("weight", sp(w.permute(0, 1, 3, 4, 2).reshape(G, C, 9 * C)))
        bd = guard.inp("bias", b)
        pooled = guard.out("pooled", (G, B, H // 4, W // 3, C))
        scratch = guard.out("scratch", (G, B, H, W, C), must_write=False)

        def go():
            launch("pp_conv3x3_maxpool_relu", F16X3, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), pooled.data_ptr(), scratch.data_ptr(), B, H, W, C, C,
                   4, 3, G, 0, C * 9 * C, C, SPLIT, None)
        L.set_option("conv_pool_split", fused)
        faults, snap = run_twice(guard, go)
        if fused and B >= 24 and not bool((guard.outs[1][1] == guard.outs[1][6]).all()):  # 192 tiles and more: one launch, no scratch
            faults.append("the one-launch form wrote to the scratch tensor")
        imgs, ch = pick(B, rng, 1), torch.from_numpy(rng.choice(C, 48, replace=False))
        xi = x[imgs].permute(0, 3, 1, 2).cpu().double()
        ref = torch.stack([pool_relu64(conv3x3_64(xi, w[k][ch].double(), b[k][ch].double()), 4, 3) for k in range(G)])
        got = unsp(snap[0])[:, imgs][..., ch].permute(0, 1, 4, 2, 3)
        if poisoned:
            ratio = poison_ratio(got, ref, conv_reach(bad_pixels(x[imgs].cpu()), 4, 3)[None], TOL["conv_pool"], TOL["conv_pool"])
        else:
            ratio = error_ratio(got, ref, TOL["conv_pool"], TOL["conv_pool"])
        return faults, ratio, f"B {B} conv_pool_split {fused} poison {poisoned}"

    # ------------------------------------------------------------------------------------------------- last tower layer + flip average
    def case_tower_final(rng, g):
        fmt = int(rng.integers(0, 3))  # fp32, bf16, split
        passes = int(rng.integers(1, 3))
        B = int(rng.choice([1, 2, 3, 64, int(rng.integers(1, 600))]))
        C = 32 * int(rng.integers(1, 25)) if fmt == 2 else 4 * int(rng.integers(1, 193))
        K = int(rng.integers(1, 40))
        err_div = float(rng.choice([1.0, 2.0, 7.3, 100.0]))
        feat = cpu_rand(4, passes * B, C, g=g)
        poisoned = rng.random() < 0.25
        if poisoned:
            poison_(feat, g, int(rng.integers(1, 6)))
        w = cpu_rand(4, K, C, g=g, scale=1 / math.sqrt(C))
        bias = cpu_rand(4, K, g=g, scale=0.3)
        fi = torch.randperm(K, generator=g)
        guard = Guard()
        if fmt == 2:
            fd, fq = sp(feat), feat.double()
        elif fmt == 1:
            fd, fq = feat.bfloat16().cuda(), feat.bfloat16().double()
        else:
            fd, fq = feat.cuda(), feat.double()
        fd, wd, bd = guard.inp("feat", fd), guard.inp("w", w), guard.inp("bias", bias)
        fid = guard.inp("flip_indices", fi.to(torch.int32))
        out = guard.out("out", (4, B, K))

        def go():
            launch("pp_tower_final", fd.data_ptr(), fmt, wd.data_ptr(), bd.data_ptr(), fid.data_ptr() if passes == 2 else None, out.data_ptr(), B,
                   passes, C, K, err_div, None)
        faults, snap = run_twice(guard, go)
        ref = tower_final64(fq, w.double(), bias.double(), fi, B, passes, err_div)
        if poisoned:  # a feature row with a non-finite element reaches every keypoint of its (tower, crop); the flip pass's row the same crop
            bad = ~torch.isfinite(fq).all(dim=-1)
            reach = (bad[:, :B] | bad[:, B:]) if passes == 2 else bad
            fac = magnitude_factor(fq.nan_to_num(0.0, 0.0, 0.0).reshape(-1, C))
            ratio = poison_ratio(snap[0].cpu(), ref, reach[..., None], TOL["tower_final"] * fac, TOL["tower_final_atol"] * fac)
        else:
            fac = magnitude_factor(fq.reshape(-1, C))
            ratio = error_ratio(snap[0].cpu(), ref, TOL["tower_final"] * fac, TOL["tower_final_atol"] * fac)
        return faults, ratio, f"fmt {fmt} passes {passes} B {B} C {C} K {K} err_div {err_div} poison {poisoned}"

    entries = [
        ("pp_deconv_head_split", case_deconv_head),
        ("pp_conv3x3_winograd_maxpool_relu", case_winograd),
        ("pp_conv3x3_splitk + pp_sum_maxpool_relu_nhwc", case_splitk),
        ("pp_conv3x3_maxpool_relu", case_conv_pool),
        ("pp_tower_final", case_tower_final),
    ]
    return run_entries(entries, seconds, 90000, "HEAD", L)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sys.exit(_main(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0))


if __name__ == "__main__":
    main()
