#!/usr/bin/env python
"""Fuzz of the ViT-layer kernels of the split-fp16 (f16x3) plans against torch fp64 on the unrounded inputs: pp_qkv_attention_split (plain / _ws /
_folded), pp_proj_ffn_split_folded, pp_proj_ffn_split_residual_layernorm_ws, pp_ffn_split_residual_layernorm_ws, pp_linear_ln_folded_ws,
pp_gemm_residual_layernorm_ws (three precisions) and pp_attention (every instantiated precision / sequence / head size), visited round robin.
Shapes straddle the dispatch thresholds, computed from pp_device_cu_count(): the deep ring and query split of the fused attention, the XCD remap,
tile counts around multiples of the CU count, ragged 96- / 192-row blocks. Values: unit normal rows, rows with large offsets, massive-activation
channels, peaked attention (max |logit| 30 - 60, arg-max key in the first or the last key stage).
Every case: outputs, statistics and scratch buffers between canaries (a bit pattern compared bit for bit), every element written, inputs
bit-identical after the launch (but the buffer the ABI updates in place), a repeat launch bit-identical, fp64 accuracy, and the exact equalities
the code claims (query split on / off, in place / out of place, centered residual + means == the plain launch on (hi + lo) + mean).

Tolerances are the fixed-shape tests' (tests/test_split_fp16.py, tests/test_kernels_gpu.py), scaled by the operands' magnitude: the split format's
error is 2^-22 relative to an OPERAND, so a dot product's error is ~ 2^-22 |a_r| |w_n| (independent roundings add in quadrature); those tests hold
for unit-normal rows (rms 1), so a case whose largest MFMA operand row has rms s gets base * max(1, s) (LayerNorm outputs keep rms ~ 1 whatever
their input). Two classes add a documented error of their own:
  * raw rows through pp_linear_ln_folded with statistics in lose log2(1 + |mean| / std) bits (include/probpose_mi355x.h, numeric domain):
    base * (1 + max |mean| / std);
  * a LayerNorm output of rows with an offset: an fp32 row carries an error relative to |mean| + std, the LayerNorm divides it by std:
    base * (1 + max |mean| / std) of the LayerNorm's input rows (1 - 2 for unit-normal and trained rows);
  * peaked attention: a logit l carries ~ 2^-22 |l| from each of q and k, the fp32 accumulation and the exp argument - at most 2^-20 |l| - and
    that error scales the softmax weights and hence the output, which is bounded by max |v|: + 2^-20 * max |logit| * max |v| (absolute).
Refusals (UNSUPPORTED / INVALID_ARG) are counted; a shape the engine sends is never refused.   python tests/fuzz_layer.py [seconds]"""
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16, F32, F16X3 = 0, 1, 2  # PP_PREC_*
SPLIT = 2                   # PP_OUT_SPLIT
EPS = 1e-6
CAN = 2048                  # canary elements on each side of every guarded buffer
PATTERN = {torch.float32: 0x7FC0DEAD, torch.bfloat16: 0x7FAD, torch.float64: 0x7FF8DEAD0BADF00D}  # NaN payloads no kernel writes
MASSIVE = (250.0, -120.0, 60.0)  # synthetic.TRAINED_MASSIVE: residual-stream values of the massive-activation channels
MEM_CAP = 2 << 30
# base tolerances (rtol = atol) of the fixed-shape tests, per kernel output (tests/test_split_fp16.py, tests/test_kernels_gpu.py)
TOL = dict(qkv=2e-5, qkv_folded=1e-5, ffn=2e-5, proj_ffn=3e-5, ln2_rows=2e-5, row_stats=2e-5, linear=2e-5, linear_long=3e-5, part_stats=1e-4,
           gemm_ln=2e-5, gemm_ln_bf16_x=2e-2, gemm_ln_bf16_h=3e-2, attention=2e-5, attention_bf16=3e-2)


# ----------------------------------------------------------------------------------------------------- fp64 references (imported by the CPU test)
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def layernorm64(x, gamma, beta, eps=EPS):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def attention64(qkv, n_seq, S, heads, hd, scale):
    """(n_seq * S, 3 * heads * hd) rows [q | k | v], head-major inside each (mmpretrain MultiheadAttention) -> (n_seq * S, heads * hd)."""
    q, k, v = qkv.reshape(n_seq, S, 3, heads, hd).permute(2, 0, 3, 1, 4)
    logits = (q @ k.transpose(-1, -2)) * scale
    p = torch.exp(logits - logits.amax(dim=-1, keepdim=True))
    p = p / p.sum(dim=-1, keepdim=True)
    return (p @ v).transpose(1, 2).reshape(n_seq * S, heads * hd)


def max_logit64(qkv, n_seq, S, heads, hd, scale):
    q, k, _ = qkv.reshape(n_seq, S, 3, heads, hd).permute(2, 0, 3, 1, 4)
    return float(((q @ k.transpose(-1, -2)) * scale).abs().max())


def ffn64(h, w1, b1, w2, b2):
    return gelu64(h @ w1.t() + b1) @ w2.t() + b2


def proj_ffn64(att, r, wp, bp, g2, be2, w1, b1, w2, b2):
    """-> (x_mid, h_mid, x_out): x_mid = r + att Wp^T + bp, h_mid = ln2(x_mid), x_out = x_mid + ffn(h_mid)."""
    x_mid = r + att @ wp.t() + bp
    h_mid = layernorm64(x_mid, g2, be2)
    return x_mid, h_mid, x_mid + ffn64(h_mid, w1, b1, w2, b2)


def row_part_stats64(y):
    """(M, N) -> (M, N / 96, 2): per row and 96-column part (mean, sum of squared deviations from it) - pp_linear_ln_folded's stats_out."""
    p = y.reshape(y.shape[0], -1, 96)
    mean = p.mean(dim=2)
    return torch.stack([mean, ((p - mean[..., None]) ** 2).sum(dim=2)], dim=2)


def row_stats64(x, eps=EPS):
    """(M, E) -> (M, 2): (mean, rstd) of every row, biased variance (nn.LayerNorm)."""
    mean = x.mean(dim=1)
    return torch.stack([mean, 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(dim=1) + eps)], dim=1)


def error_ratio(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|): <= 1 passes (torch.allclose's bound); NaN / inf anywhere -> inf."""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max()) if got.numel() else 0.0


def peaked_atol(max_logit, max_v):
    return 2.0 ** -20 * max_logit * max_v


# ----------------------------------------------------------------------------------------------------- GPU helpers
class Refused(Exception):
    pass


class Guard:
    """Buffers of one case: outputs between canaries (refilled by rearm() for a repeat launch), inputs with a copy to compare against."""

    def __init__(self):
        self.outs, self.ins = [], []

    def out(self, name, shape, dtype=torch.float32, init=None, must_write=True):
        n = int(np.prod(shape))
        idt = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}[dtype]
        full = torch.full((n + 2 * CAN,), PATTERN[dtype], dtype=idt, device="cuda")
        view = full[CAN:CAN + n].view(dtype).view(*shape)
        init = init.to(device="cuda", dtype=dtype).reshape(shape).clone() if init is not None else None
        if init is not None:
            view.copy_(init)
        self.outs.append((name, full, n, init, must_write and init is None, view, PATTERN[dtype]))
        return view

    def inp(self, name, t):
        t = t.contiguous().cuda()
        self.ins.append((name, t, t.clone()))
        return t

    def rearm(self):
        for _, full, n, init, _, view, pat in self.outs:
            full.fill_(pat)
            if init is not None:
                view.copy_(init)

    def faults(self):
        f = []
        for name, full, n, _, must_write, _, pat in self.outs:
            if not (bool((full[:CAN] == pat).all()) and bool((full[CAN + n:] == pat).all())):
                f.append(f"{name}: canary overwritten")
            if must_write and bool((full[CAN:CAN + n] == pat).any()):
                f.append(f"{name}: elements left unwritten")
        for name, t, c in self.ins:
            if not torch.equal(t.reshape(-1).view(torch.uint8), c.reshape(-1).view(torch.uint8)):
                f.append(f"{name}: input modified")
        return f

    def snapshot(self):
        return [o[5].clone() for o in self.outs]


def bits_equal(a, b):
    return all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(a, b))


def run_twice(guard, go):
    """launch, check buffers, snapshot; rearm, launch again: the same bits."""
    go()
    faults = guard.faults()
    first = guard.snapshot()
    guard.rearm()
    go()
    if not bits_equal(first, guard.snapshot()):
        faults.append("repeat launch differs")
    faults += [f for f in guard.faults() if f not in faults]
    return faults, first


def sample_rows(M, block, rng, extra=0):
    """Rows the fp64 reference is computed on: all of them for small M, else the first and last block whole plus one random row of every block."""
    if M <= 4 * block + extra:
        return torch.arange(M)
    nb = (M + block - 1) // block
    pick = torch.from_numpy(np.minimum(np.arange(nb) * block + rng.integers(0, block, nb), M - 1))
    return torch.unique(torch.cat([torch.arange(block), torch.arange(max(0, M - 2 * block), M), pick]))


def rows_of_class(M, E, cls, g, device="cuda"):
    """Activation rows of a value class: "normal", "offset" (row means up to 16 std), "massive" (three channels at 60 .. 250)."""
    x = torch.randn(M, E, generator=g, device=device)
    if cls == "offset":
        std = torch.rand(M, 1, generator=g, device=device) * 1.5 + 0.5
        x = x * std + (torch.rand(M, 1, generator=g, device=device) * 32 - 16) * std
    elif cls == "massive":
        chans = torch.randperm(E, generator=torch.Generator().manual_seed(int(torch.randint(0, 1 << 30, (1,), generator=g, device=device))))[:3]
        for c, m in zip(chans.tolist(), MASSIVE):
            x[:, c] = m * (0.5 + 0.5 * torch.rand(M, generator=g, device=device))
    return x


def magnitude_factor(*xs):
    """max(1, largest row rms of the MFMA operands): a dot product's error is ~ 2^-22 |a_r| |w_n| (independent roundings add in quadrature), and
    the fixed-shape tolerances hold for unit-normal rows (rms 1). LayerNorm outputs have rms ~ 1 whatever their input."""
    return max([1.0] + [float(x.double().pow(2).mean(dim=-1).sqrt().max()) for x in xs if x is not None and x.numel()])


def ln_factor(x):
    """max over rows of 1 + |mean| / std: an fp32 row carries an error relative to its magnitude (|mean| + std), and a LayerNorm divides it by
    std - the factor by which a LayerNorm output's error grows with the row offset of its input."""
    x = x.double()
    return float((1.0 + x.mean(dim=-1).abs() / x.std(dim=-1, unbiased=False).clamp_min(1e-30)).max()) if x.numel() else 1.0


def chunked(fn, x, rows=8192):
    """fn over row chunks of x (device fp64 temporaries stay small), results concatenated."""
    return torch.cat([fn(x[i:i + rows]) for i in range(0, x.shape[0], rows)])


def draw_e(rng, w):
    """a weight scale 2^e from 1 (the fixed-shape tests' unscaled weights) up to the scaled tensor's largest element in [2^13, 2^14)
    (weights.weight_scale_exponent, the stored form, puts it in [2^12, 2^13))."""
    from probpose_code_amd.weights import weight_scale_exponent

    return int(rng.integers(0, weight_scale_exponent(w) + 2))


def cpu_rand(*shape, g, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _main(seconds):
    from probpose_code_amd import _lib as L
    from probpose_code_amd.weights import fold_layernorm, from_split, to_split, weight_scale_exponent

    CU = int(L.lib.pp_device_cu_count())
    QKV_DEEP_MAX = 2 * CU // 12        # n_seq * 12 <= 2 CUs: deep ring
    QKV_QSPLIT_MAX = 4 * CU // 120     # 10 * n_seq * 12 <= 4 CUs: query split

    def sp(x):
        return to_split(x.float()).cuda()

    def unsp(c):
        return from_split(c.float().cpu()).double()

    def launch(fn, *args):
        try:
            L.call(fn, *args, None)
        except L.ProbPoseLibraryError as exc:
            if "UNSUPPORTED" in str(exc) or "INVALID" in str(exc):
                raise Refused(str(exc)) from None
            raise
        torch.cuda.synchronize()

    # ------------------------------------------------------------------------------------------------- fused qkv + attention
    def case_qkv(form, rng, g):
        S, E, H, hd = 192, 384, 12, 32
        thr = [QKV_DEEP_MAX, QKV_QSPLIT_MAX]
        choices = list(range(1, 10)) + [t + d for t in thr for d in (-1, 0, 1) if t + d > 0] + list(range(36, 45)) + [127, 128, 129, 511, 512, 513]
        n_seq = int(rng.choice(choices)) if rng.random() < 0.8 else int(rng.integers(1, 1400))
        M = n_seq * S
        deep, qsplit = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        # the plain forms take LayerNorm outputs (rms ~ 1); raw residual rows - offsets, massive channels - reach the folded form only
        cls = str(rng.choice(["offset", "massive", "peaked"] if form == "folded" else ["normal", "peaked"]))
        bias = form == "folded" or rng.random() < 0.7
        w = cpu_rand(3 * E, E, g=g, scale=1 / math.sqrt(E))
        b = cpu_rand(3 * E, g=g, scale=0.3)
        if cls == "peaked":  # Wk = c Wq: a query's largest logit is its own key, in every key stage
            c = float(rng.uniform(30, 60)) / (2.5 * hd * hd ** -0.5)
            w[E:2 * E] = w[:E] * c
            b[E:2 * E] = b[:E] * c
        gd = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
        idx_seq = torch.unique(torch.tensor([0, n_seq - 1] + rng.integers(0, n_seq, 6).tolist())) if n_seq > 8 else torch.arange(n_seq)
        rows = (idx_seq[:, None] * S + torch.arange(S)).reshape(-1)
        guard = Guard()
        out = guard.out("out", (M, E))
        e = 0
        if form == "folded":
            x = rows_of_class(M, E, "massive" if cls == "massive" else "offset", gd)
            g1, be1 = 1.0 + 0.2 * cpu_rand(E, g=g), 0.2 * cpu_rand(E, g=g)
            mean = x.mean(dim=1, keepdim=True)
            xs = guard.inp("x_centered", sp(x - mean))
            xq = (from_split(xs[rows].cpu()).double() + mean[rows].cpu().double())  # the values the centered rows stand for
            xc = torch.cat([xs, mean], dim=1)
            stats = guard.inp("ln_stats", chunked(lambda c: row_stats64(from_split(c[:, :E]).double() + c[:, E:].double()).float(), xc))
            del xc
            hn = layernorm64(xq, g1.double(), be1.double())
            e = draw_e(rng, w * g1[None, :])
            wf, _, bf = fold_layernorm(w, b, g1, be1, scale_exp=e)
            wd, bd = guard.inp("w", wf), guard.inp("b", bf)
            qkv = hn @ w.double().t() + b.double()
            base, operands = TOL["qkv_folded"], (hn,)

            def go():
                launch("pp_qkv_attention_split_folded", xs.data_ptr(), wd.data_ptr(), bd.data_ptr(), stats.data_ptr(), out.data_ptr(), n_seq, S, H,
                       hd, hd ** -0.5, 2.0 ** -e)
        else:
            h = rows_of_class(M, E, "normal", gd)
            hs = guard.inp("h", sp(h))
            hq = h[rows].cpu().double()
            e = draw_e(rng, w) if form == "ws" else 0
            wd = guard.inp("w", sp(w * 2.0 ** e))
            bd = guard.inp("b", b) if bias else None
            qkv = hq @ w.double().t() + (b.double() if bias else 0.0)
            base, operands = TOL["qkv"], (hq,)

            def go():
                if form == "plain":
                    launch("pp_qkv_attention_split", hs.data_ptr(), wd.data_ptr(), L.ptr(bd), out.data_ptr(), n_seq, S, H, hd, hd ** -0.5)
                else:
                    launch("pp_qkv_attention_split_ws", hs.data_ptr(), wd.data_ptr(), L.ptr(bd), out.data_ptr(), n_seq, S, H, hd, hd ** -0.5, 2.0 ** -e)
        ns = len(idx_seq)
        ref = attention64(qkv, ns, S, H, hd, hd ** -0.5)
        ml = max_logit64(qkv, ns, S, H, hd, hd ** -0.5)
        mv = float(qkv.reshape(ns, S, 3, E)[:, :, 2].abs().max())
        fac = magnitude_factor(*operands)
        L.set_option("qkv_attn_deep", deep)
        L.set_option("qkv_attn_qsplit", qsplit)
        faults, first = run_twice(guard, go)
        if form != "folded" and deep and n_seq * H <= 2 * CU:  # the query split gives the same bits
            L.set_option("qkv_attn_qsplit", 1 - qsplit)
            guard.rearm()
            go()
            if not bits_equal(first, guard.snapshot()):
                faults.append("qkv_attn_qsplit on / off differ")
        got = unsp(first[0][rows])
        ratio = error_ratio(got, ref, base * fac, base * fac + peaked_atol(ml, mv))
        return faults, ratio, f"n_seq {n_seq} deep {deep} qsplit {qsplit} bias {bias} e {e} class {cls} max|logit| {ml:.1f}"

    # ------------------------------------------------------------------------------------------------- fused projection + FFN
    def ffn_weights(E, F_, g, rng):
        w1, b1 = cpu_rand(F_, E, g=g, scale=1 / math.sqrt(E)), cpu_rand(F_, g=g, scale=0.2)
        w2, b2 = cpu_rand(E, F_, g=g, scale=1 / math.sqrt(F_)), cpu_rand(E, g=g, scale=0.2)
        g_, be = 1 + 0.1 * cpu_rand(E, g=g), cpu_rand(E, g=g, scale=0.1)
        return w1, b1, w2, b2, g_, be

    def pack_ffn(w1, w2, e1, e2, E, F_):
        nbytes = L.lib.pp_ffn_split_packed_bytes(E, F_)
        if nbytes <= 0:
            raise Refused("pp_ffn_split_packed_bytes")
        packed = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
        w1s, w2s = sp(w1 * 2.0 ** e1), sp(w2 * 2.0 ** e2)
        L.call("pp_ffn_split_pack_weights", w1s.data_ptr(), w2s.data_ptr(), packed.data_ptr(), E, F_, None)
        torch.cuda.synchronize()  # the sources stay alive until the packing kernel has read them
        return packed

    def pack_proj(wp, ep, E):
        wpp = torch.empty(E * E, dtype=torch.float32, device="cuda")
        wps = sp(wp * 2.0 ** ep)
        L.call("pp_proj_split_pack_weights", wps.data_ptr(), wpp.data_ptr(), E, None)
        torch.cuda.synchronize()
        return wpp

    def draw_m(rng, hi):
        return int(rng.choice([1, 2, 95, 96, 97, 191, 192, 193, 96 * 7 + 40, 24576, 24576 + 96, int(rng.integers(1, hi)), int(rng.integers(1, hi // 8)),
                               192 * int(rng.integers(1, hi // 192))]))

    def case_ffn(kind, rng, g):
        E = 384
        F_ = 1536 if rng.random() < 0.3 else 128 * int(rng.integers(1, 25))
        M = draw_m(rng, 100000)
        M = max(1, min(M, int(MEM_CAP // (4 * E * 4 * 4))))
        pair = int(rng.integers(0, 2))
        cls = str(rng.choice(["normal", "offset", "massive"]))
        gd = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
        w1, b1, w2, b2, g_, be = ffn_weights(E, F_, g, rng)
        e1, e2 = draw_e(rng, w1), draw_e(rng, w2)
        packed = pack_ffn(w1, w2, e1, e2, E, F_)
        rows = sample_rows(M, 96, rng)
        guard = Guard()
        guard.inp("w_packed", packed)
        r = rows_of_class(M, E, cls, gd)
        h = rows_of_class(M, E, "normal", gd)  # LayerNorm output / attention rows
        dev = [guard.inp(n, t) for n, t in (("b1", b1), ("b2", b2), ("gamma", g_), ("beta", be))]
        in_place = rng.random() < 0.5
        if kind == "ffn":
            hs = sp(h)
            x_ref = r[rows].cpu().double() + ffn64(h[rows].cpu().double(), w1.double(), b1.double(), w2.double(), b2.double())
            operands = (h[rows],)
            if in_place:  # how the engine calls it: residual aliases x_out, h_in aliases h_out
                xo = guard.out("x_out", (M, E), init=r)
                ho = guard.out("h_in/h_out", (M, E), init=hs)
                hin, res = ho, xo
            else:
                hin, res = guard.inp("h_in", hs), guard.inp("residual", r)
                xo, ho = guard.out("x_out", (M, E)), guard.out("h_out", (M, E))

            def go():
                launch("pp_ffn_split_residual_layernorm_ws", hin.data_ptr(), packed.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), res.data_ptr(),
                       xo.data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), EPS, ho.data_ptr(), M, E, F_, 2.0 ** -e1, 2.0 ** -e2)
            base_x, base_h, checks = TOL["ffn"], TOL["ffn"], []
        else:
            wp, bp = cpu_rand(E, E, g=g, scale=1 / math.sqrt(E)), cpu_rand(E, g=g, scale=0.2)
            g2, be2 = 1 + 0.1 * cpu_rand(E, g=g), cpu_rand(E, g=g, scale=0.1)
            ep = draw_e(rng, wp)
            wpp = guard.inp("wproj_packed", pack_proj(wp, ep, E))
            dp = [guard.inp(n, t) for n, t in (("bproj", bp), ("gamma2", g2), ("beta2", be2))]
            att_s = sp(h)
            x_mid, h_mid, x_ref = proj_ffn64(h[rows].cpu().double(), r[rows].cpu().double(), wp.double(), bp.double(), g2.double(), be2.double(),
                                            w1.double(), b1.double(), w2.double(), b2.double())
            operands = (h[rows], h_mid)
            scratch = guard.out("h_scratch", (M, E))
            if in_place:  # residual aliases x_out, att aliases h_out
                xo = guard.out("x_out", (M, E), init=r)
                ho = guard.out("att/h_out", (M, E), init=att_s)
                att, res = ho, xo
            else:
                att, res = guard.inp("att", att_s), guard.inp("residual", r)
                xo, ho = guard.out("x_out", (M, E)), guard.out("h_out", (M, E))

            def go():
                launch("pp_proj_ffn_split_residual_layernorm_ws", att.data_ptr(), wpp.data_ptr(), dp[0].data_ptr(), dp[1].data_ptr(), dp[2].data_ptr(),
                       scratch.data_ptr(), packed.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), res.data_ptr(), xo.data_ptr(), dev[2].data_ptr(),
                       dev[3].data_ptr(), EPS, ho.data_ptr(), M, E, F_, 2.0 ** -ep, 2.0 ** -e1, 2.0 ** -e2)
            base_x, base_h = TOL["proj_ffn"], TOL["proj_ffn"]
            checks = [(lambda snap: unsp(snap[0][rows]), h_mid, TOL["ln2_rows"], x_mid)]
        h_ref = layernorm64(x_ref, g_.double(), be.double())
        L.set_option("ffn_pair", pair)
        faults, snap = run_twice(guard, go)
        fac = magnitude_factor(*operands)
        outs = {id(o[5]): s for o, s in zip(guard.outs, snap)}
        fh = fac * ln_factor(x_ref)
        parts = [error_ratio(outs[id(xo)][rows].cpu(), x_ref, base_x * fac, base_x * fac),
                 error_ratio(unsp(outs[id(ho)][rows]), h_ref, base_h * fh, base_h * fh)]
        parts += [error_ratio(getter(snap), ref, tol * fac * ln_factor(src), tol * fac * ln_factor(src)) for getter, ref, tol, src in checks]
        return faults, max(parts), f"M {M} F {F_} pair {pair} in_place {in_place} class {cls} (x, h, ln2: {', '.join(f'{p:.3g}' for p in parts)})"

    def case_proj_folded(rng, g):
        """pp_proj_ffn_split_folded in the forms the engine uses: first layer (fp32 residual in, folded out), layers in between (centered split
        residual + means in, folded out, in place), last layer (centered split in, LayerNorm out); weight scales."""
        E = 384
        F_ = 1536 if rng.random() < 0.5 else 256 * int(rng.integers(1, 13))
        if rng.random() < 0.05:
            F_ = 384  # an odd chunk count: refused (the paired kernel only)
        M = max(1, min(draw_m(rng, 100000), int(MEM_CAP // (4 * E * 4 * 5))))
        cls = str(rng.choice(["normal", "offset", "massive"]))
        form = str(rng.choice(["first", "middle", "last"]))
        gd = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
        w1, b1, w2, b2, g_, be = ffn_weights(E, F_, g, rng)
        wp, bp = cpu_rand(E, E, g=g, scale=1 / math.sqrt(E)), cpu_rand(E, g=g, scale=0.2)
        g2, be2 = 1 + 0.1 * cpu_rand(E, g=g), cpu_rand(E, g=g, scale=0.1)
        e1, e2, ep = (draw_e(rng, w1), draw_e(rng, w2), draw_e(rng, wp)) if rng.random() < 0.7 else (0, 0, 0)
        packed, wpp = pack_ffn(w1, w2, e1, e2, E, F_), pack_proj(wp, ep, E)
        rows = sample_rows(M, 96, rng)
        guard = Guard()
        guard.inp("w_packed", packed), guard.inp("wproj_packed", wpp)
        dev = [guard.inp(n, t) for n, t in (("bproj", bp), ("gamma2", g2), ("beta2", be2), ("b1", b1), ("b2", b2), ("gamma", g_), ("beta", be))]
        r = rows_of_class(M, E, cls, gd)
        att = guard.inp("att", sp(rows_of_class(M, E, "normal", gd)))
        rmean = r.mean(dim=1, keepdim=True)
        rs = sp(r - rmean)
        rst = torch.cat([rmean, torch.ones_like(rmean)], dim=1).contiguous()
        rq = from_split(rs) + rmean  # the fp32 rows the centered ones stand for: (hi + lo) + mean, one rounding
        res_split = form != "first"
        fold_out = form != "last"
        in_place = form == "middle" and rng.random() < 0.7
        scratch = guard.out("h_scratch", (M, E))
        if in_place:
            res = guard.out("residual/h_out", (M, E), init=rs)
            rstats = guard.out("residual_stats/stats_out", (M, 2), init=rst)
            ho, st = res, rstats
        else:
            res = guard.inp("residual", rs if res_split else r)
            rstats = guard.inp("residual_stats", rst) if res_split else None
            ho = guard.out("h_out", (M, E))
            st = guard.out("stats_out", (M, 2)) if fold_out else None
        xo = None if fold_out else guard.out("x_out", (M, E))
        sc = (2.0 ** -ep, 2.0 ** -e1, 2.0 ** -e2)

        def folded(res_, rstats_, ho_, st_, xo_, scratch_):
            launch("pp_proj_ffn_split_folded", att.data_ptr(), wpp.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                   scratch_.data_ptr(), packed.data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(), res_.data_ptr(), SPLIT if res_split else 0,
                   L.ptr(rstats_), int(fold_out), L.ptr(xo_), None if fold_out else dev[5].data_ptr(), None if fold_out else dev[6].data_ptr(), EPS,
                   ho_.data_ptr(), L.ptr(st_), M, E, F_, *sc)

        def go():
            folded(res, rstats, ho, st, xo, scratch)
        L.set_option("ffn_pair", 1)
        faults, snap = run_twice(guard, go)
        outs = {id(o[5]): s for o, s in zip(guard.outs, snap)}
        rq_rows = rq[rows].cpu().double() if res_split else r[rows].cpu().double()
        x_mid, h_mid, x_ref = proj_ffn64(from_split(att[rows].cpu()).double(), rq_rows, wp.double(), bp.double(), g2.double(), be2.double(), w1.double(),
                                         b1.double(), w2.double(), b2.double())
        fac = magnitude_factor(from_split(att[rows].cpu()), h_mid)
        tol = TOL["proj_ffn"] * fac
        f2 = fac * ln_factor(x_mid)
        ratio = error_ratio(unsp(outs[id(scratch)][rows]), h_mid, TOL["ln2_rows"] * f2, TOL["ln2_rows"] * f2)
        fo = fac * ln_factor(x_ref)
        if fold_out:
            st_got = outs[id(st)][rows].cpu().double()
            ref_st = row_stats64(x_ref)
            ratio = max(ratio, error_ratio(st_got, ref_st, TOL["row_stats"] * fo, TOL["row_stats"] * fo))
            ratio = max(ratio, error_ratio(unsp(outs[id(ho)][rows]) + st_got[:, :1], x_ref, tol, tol))
        else:
            ratio = max(ratio, error_ratio(outs[id(xo)][rows].cpu(), x_ref, tol, tol),
                        error_ratio(unsp(outs[id(ho)][rows]), layernorm64(x_ref, g_.double(), be.double()), tol * fo / fac, tol * fo / fac))
        # exact equalities: out of place == in place; centered split residual + means == the plain launch on (hi + lo) + mean
        if res_split and fold_out:
            other = [torch.full((M, E), float("nan"), device="cuda") for _ in range(2)] + [torch.full((M, 2), float("nan"), device="cuda")]
            if in_place:
                folded(rs.clone(), rst.clone(), other[0], other[2], None, other[1])
            else:
                r2, s2 = rs.clone(), rst.clone()
                folded(r2, s2, r2, s2, None, other[1])
                other[0], other[2] = r2, s2
            if not (bits_equal([outs[id(ho)]], [other[0]]) and bits_equal([outs[id(st)]], [other[2]])):
                faults.append("in place and out of place differ")
        if res_split and not fold_out:
            pxo, pho, psc = (torch.full((M, E), float("nan"), device="cuda") for _ in range(3))
            launch("pp_proj_ffn_split_residual_layernorm_ws", att.data_ptr(), wpp.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                   psc.data_ptr(), packed.data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(), rq.contiguous().data_ptr(), pxo.data_ptr(),
                   dev[5].data_ptr(), dev[6].data_ptr(), EPS, pho.data_ptr(), M, E, F_, *sc)
            if not bits_equal([outs[id(xo)], outs[id(ho)]], [pxo, pho]):
                faults.append("centered residual + means != the plain launch on (hi + lo) + mean")
        return faults, ratio, f"M {M} F {F_} form {form} in_place {in_place} scales {(ep, e1, e2)} class {cls}"

    # ------------------------------------------------------------------------------------------------- ViT-B Linear layers
    def case_linear(rng, g):
        N = int(rng.choice([192, 384, 576, 768, 1152, 1536, 2304, 3072]))
        with_ln = rng.random() < 0.4
        K = 192 * int(rng.integers(1, 17)) if with_ln else 32 * int(rng.integers(2, 97))
        if rng.random() < 0.4:
            N, K = [(768, 768), (2304, 768), (3072, 768), (768, 3072)][int(rng.integers(0, 4))]
            K = K if (not with_ln or K % 192 == 0) else 768
        # M with the tile count (ceil(M / 192) * N / 192) on either side of a multiple of the CU count
        ct = N // 192
        j = int(rng.integers(1, 6))
        rt = max(1, (j * CU + int(rng.integers(-3, 4))) // ct)
        M = int(rng.choice([1, 77, 192 * rt - int(rng.integers(0, 192)), 192 * rt + int(rng.integers(1, 192)), int(rng.integers(1, 60000))]))
        M = max(1, min(M, int(MEM_CAP // (4 * (2 * N + K) * 3))))
        act = int(rng.choice([0, 1])) if with_ln else int(rng.choice([0, 0, 1]))
        res_kind = "none" if with_ln else str(rng.choice(["none", "f32", "split", "split_in_place"]))
        out_split = res_kind == "split_in_place" or (res_kind != "split_in_place" and rng.random() < 0.5)
        stats_out = (not with_ln) and N % 96 == 0 and rng.random() < 0.5
        loop = int(rng.integers(0, 2))
        cls = str(rng.choice(["normal", "offset", "massive"]))
        gd = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
        w, b = cpu_rand(N, K, g=g, scale=1 / math.sqrt(K)), cpu_rand(N, g=g, scale=0.1)
        e = draw_e(rng, w)
        x = rows_of_class(M, K, cls, gd)
        rows = sample_rows(M, 192, rng)
        guard = Guard()
        xs = guard.inp("act", sp(x))
        xq = from_split(xs[rows].cpu()).double() if with_ln else x[rows].cpu().double()
        fac = magnitude_factor(xq)
        lnst = cs = None
        if with_ln:
            g1, be1 = 1.0 + 0.2 * cpu_rand(K, g=g), 0.2 * cpu_rand(K, g=g)
            e = draw_e(rng, w * g1[None, :])
            wf, csum, bf = fold_layernorm(w, b, g1, be1, scale_exp=e)
            wd, bd, cs = guard.inp("weight", wf), guard.inp("bias", bf), guard.inp("colsum", csum)
            lnst = guard.inp("ln_stats", chunked(lambda c: row_part_stats64(from_split(c).double()).float(), xs))
            ref = layernorm64(xq, g1.double(), be1.double()) @ w.double().t() + b.double()
            st = row_stats64(xq)
            fac = max(fac, float((1.0 + st[:, 0].abs() * st[:, 1]).max()))  # the documented loss of raw rows: log2(1 + |mean| / std) bits
            fac = max(fac, magnitude_factor(layernorm64(xq, g1.double(), be1.double())))
        else:
            wd, bd = guard.inp("weight", sp(w * 2.0 ** e)), guard.inp("bias", b)
            ref = xq @ w.double().t() + b.double()
        if act == 1:
            ref = gelu64(ref)
        res = None
        if res_kind != "none":
            r = rows_of_class(M, N, "normal", gd)
            if res_kind == "f32":
                res = guard.inp("residual", r)
                ref = ref + r[rows].cpu().double()
            else:
                rsp = sp(r)
                ref = ref + from_split(rsp[rows].cpu()).double()
                res = guard.out("residual/out", (M, N), init=rsp) if res_kind == "split_in_place" else guard.inp("residual", rsp)
        out = res if res_kind == "split_in_place" else guard.out("out", (M, N))
        so = guard.out("stats_out", (M, N // 96, 2)) if stats_out else None

        def go():
            launch("pp_linear_ln_folded_ws", xs.data_ptr(), wd.data_ptr(), bd.data_ptr(), L.ptr(res), SPLIT if res_kind.startswith("split") else 0,
                   out.data_ptr(), SPLIT if out_split else 0, M, N, K, act, L.ptr(lnst), L.ptr(cs), EPS, L.ptr(so), 2.0 ** -e)
        L.set_option("linear_loop", loop)
        product = (N, K) in ((768, 768), (2304, 768), (3072, 768), (768, 3072)) and L.lib.pp_linear_ln_folded_supported(M, N, K, int(with_ln)) == 2
        try:
            faults, snap = run_twice(guard, go)
        except Refused:
            if product:
                return [f"a product shape was refused"], 0.0, f"M {M} N {N} K {K}"
            raise
        outs = {id(o[5]): s for o, s in zip(guard.outs, snap)}
        o = outs[id(out)][rows]
        got = unsp(o) if out_split else o.cpu().double()
        base = TOL["linear_long"] if (with_ln or K > 768 or act) else TOL["linear"]
        ratio = error_ratio(got, ref, base * fac, base * fac)
        if stats_out:
            ratio = max(ratio, error_ratio(outs[id(so)][rows].cpu().double(), row_part_stats64(ref), TOL["part_stats"] * fac, TOL["part_stats"] * fac))
        return faults, ratio, f"M {M} N {N} K {K} ln {with_ln} act {act} res {res_kind} split_out {out_split} stats_out {stats_out} loop {loop} e {e} class {cls}"

    # ------------------------------------------------------------------------------------------------- residual Linear + LayerNorm
    def case_gemm_res_ln(rng, g):
        E = int(rng.choice([384, 768]))
        prec = int(rng.integers(0, 3))
        K = int(rng.choice([384, 768, 1536, 3072]))
        M = int(rng.choice([1, 95, 96, 97, 111, 112, 113, 250, 1000, 24576 + 40, int(rng.integers(1, 30000))]))
        M = max(1, min(M, int(MEM_CAP // (4 * (K + 3 * E) * 3))))
        res_mod = int(rng.choice([0, 0, 1, 48, 192, 432]))
        cls = str(rng.choice(["normal", "offset", "massive"]))
        gd = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
        w, b = cpu_rand(E, K, g=g, scale=1 / math.sqrt(K)), cpu_rand(E, g=g, scale=0.1)
        e = draw_e(rng, w) if prec == F16X3 else 0
        g_, be = 1 + 0.1 * cpu_rand(E, g=g), cpu_rand(E, g=g, scale=0.1)
        a = rows_of_class(M, K, "normal", gd)
        r = rows_of_class(res_mod if res_mod else M, E, cls, gd)
        rows = sample_rows(M, 112, rng)
        guard = Guard()
        if prec == F16X3:
            ad, wd, aq, wq = sp(a), sp(w * 2.0 ** e), a[rows].cpu().double(), w.double()
        else:
            dt = torch.bfloat16 if prec == BF16 else torch.float32
            ad, wd = a.to(dt).contiguous(), w.to(dt).cuda()
            aq, wq = a[rows].to(dt).cpu().double(), w.to(dt).double()
        hdt = torch.bfloat16 if prec == BF16 else torch.float32
        alias_h = K == E and rng.random() < 0.5  # act may alias h_out (same shape and format)
        wd, bd, gd_, bed = guard.inp("weight", wd), guard.inp("bias", b), guard.inp("gamma", g_), guard.inp("beta", be)
        in_place = res_mod == 0 and rng.random() < 0.5
        if in_place:
            xo = guard.out("residual/x_out", (M, E), init=r)
            res = xo
        else:
            res, xo = guard.inp("residual", r), guard.out("x_out", (M, E))
        if alias_h:
            ho = guard.out("act/h_out", (M, K), dtype=ad.dtype, init=ad)
            act_t = ho
        else:
            act_t, ho = guard.inp("act", ad), guard.out("h_out", (M, E), dtype=hdt)
        rr = r.cpu().double()[torch.arange(M)[rows] % res_mod] if res_mod else r[rows].cpu().double()
        x_ref = aq @ wq.t() + b.double() + rr
        h_ref = layernorm64(x_ref, g_.double(), be.double())
        hfmt = SPLIT if prec == F16X3 else int(prec == BF16)

        def go():
            launch("pp_gemm_residual_layernorm_ws", prec, act_t.data_ptr(), wd.data_ptr(), bd.data_ptr(), res.data_ptr(), res_mod, xo.data_ptr(),
                   gd_.data_ptr(), bed.data_ptr(), EPS, ho.data_ptr(), hfmt, M, E, K, K, K, 2.0 ** -e)
        faults, snap = run_twice(guard, go)
        outs = {id(o[5]): s for o, s in zip(guard.outs, snap)}
        fac = magnitude_factor(aq)
        tx, th = (TOL["gemm_ln_bf16_x"], TOL["gemm_ln_bf16_h"]) if prec == BF16 else (TOL["gemm_ln"], TOL["gemm_ln"])
        hg = outs[id(ho)][rows]
        hg = unsp(hg) if prec == F16X3 else hg.cpu().double()
        rx, rh = error_ratio(outs[id(xo)][rows].cpu(), x_ref, tx * fac, tx * fac), error_ratio(hg[:, :E], h_ref, th * fac * ln_factor(x_ref), th * fac * ln_factor(x_ref))
        return faults, max(rx, rh), f"prec {prec} M {M} E {E} K {K} res_mod {res_mod} in_place {in_place} alias_h {alias_h} e {e} class {cls} (x {rx:.3g}, h {rh:.3g})"

    # ------------------------------------------------------------------------------------------------- attention
    ATT_SHAPES = [(BF16, 192, 32), (BF16, 192, 64), (BF16, 432, 32), (BF16, 432, 64), (F32, 192, 32), (F32, 192, 64), (F32, 432, 32),
                  (F16X3, 192, 32), (F16X3, 192, 64), (F16X3, 432, 32), (F16X3, 432, 64)]

    def case_attention(rng, g):
        prec, S, hd = ATT_SHAPES[int(rng.integers(0, len(ATT_SHAPES)))]
        heads = int(rng.integers(1, 17))
        E = heads * hd
        n_seq = int(rng.choice([1, 2, 3, 7, 8, 64, 128, int(rng.integers(1, 300))]))
        n_seq = max(1, min(n_seq, int(MEM_CAP // (S * 4 * E * 4 * 2))))
        dma = int(rng.integers(0, 2))
        cls = str(rng.choice(["normal", "peaked_self", "peaked_sink"]))
        gd = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
        qkv = torch.randn(n_seq * S, 3, heads, hd, generator=gd, device="cuda") * 1.3
        if cls != "normal":
            target = float(rng.uniform(30, 60))
            if cls == "peaked_self":  # k = c q: each query's arg-max key is itself, in every key stage
                c = target / (1.69 * hd * 1.5 * hd ** -0.5)
                qkv[:, 1] = qkv[:, 0] * c
            else:  # one sink key per sequence, in the first or the last key stage, aligned with a direction every query shares
                u = torch.randn(heads, hd, generator=gd, device="cuda")
                u = u / u.norm(dim=1, keepdim=True)
                qkv[:, 0] += (2.0 - (qkv[:, 0] * u).sum(-1, keepdim=True)) * u  # q . u = 2 for every query: every logit of the sink key = target
                j = int(rng.integers(0, 16)) if rng.random() < 0.5 else S - 1 - int(rng.integers(0, 16))
                kk = qkv.view(n_seq, S, 3, heads, hd)
                kk[:, j, 1] = u * (target / (2.0 * hd ** -0.5))
        qkv = qkv.reshape(n_seq * S, 3 * E)
        idx_seq = torch.unique(torch.tensor([0, n_seq - 1] + rng.integers(0, n_seq, 4).tolist())) if n_seq > 6 else torch.arange(n_seq)
        rows = (idx_seq[:, None] * S + torch.arange(S)).reshape(-1)
        guard = Guard()
        if prec == F16X3:
            qd, qq = sp(qkv), qkv[rows].cpu().double()
            odt = torch.float32
        else:
            dt = torch.bfloat16 if prec == BF16 else torch.float32
            qd = qkv.to(dt).contiguous()
            qq, odt = qkv[rows].to(dt).cpu().double(), dt
        qd = guard.inp("qkv", qd)
        out = guard.out("out", (n_seq * S, E), dtype=odt)

        def go():
            launch("pp_attention", prec, qd.data_ptr(), out.data_ptr(), n_seq, S, heads, hd, hd ** -0.5)
        L.set_option("attn_dma", dma)
        faults, snap = run_twice(guard, go)
        ns = len(idx_seq)
        ref = attention64(qq, ns, S, heads, hd, hd ** -0.5)
        ml = max_logit64(qq, ns, S, heads, hd, hd ** -0.5)
        mv = float(qq.reshape(ns * S, 3, E)[:, 2].abs().max())
        got = unsp(snap[0][rows]) if prec == F16X3 else snap[0][rows].cpu().double()
        base = TOL["attention_bf16"] if prec == BF16 else TOL["attention"]
        ratio = error_ratio(got, ref, base, base + peaked_atol(ml, mv))
        return faults, ratio, f"prec {prec} S {S} hd {hd} heads {heads} n_seq {n_seq} attn_dma {dma} class {cls} max|logit| {ml:.1f}"

    entries = [
        ("pp_qkv_attention_split", lambda rng, g: case_qkv("plain", rng, g)),
        ("pp_qkv_attention_split_ws", lambda rng, g: case_qkv("ws", rng, g)),
        ("pp_qkv_attention_split_folded", lambda rng, g: case_qkv("folded", rng, g)),
        ("pp_proj_ffn_split_folded", case_proj_folded),
        ("pp_proj_ffn_split_residual_layernorm_ws", lambda rng, g: case_ffn("proj", rng, g)),
        ("pp_ffn_split_residual_layernorm_ws", lambda rng, g: case_ffn("ffn", rng, g)),
        ("pp_linear_ln_folded_ws", case_linear),
        ("pp_gemm_residual_layernorm_ws", case_gemm_res_ln),
        ("pp_attention", case_attention),
    ]
    return run_entries(entries, seconds, 70000, "LAYER", L)


def run_entries(entries, seconds, seed0, label, L, summary=None):
    """Round robin over the entry points until the time is up; prints the per-entry-point table (then `summary()`, when given: a non-empty list it
    returns names failures of its own) and the verdict. Returns the exit status."""
    stats = {name: dict(cases=0, refused=0, worst=0.0, bad=0) for name, _ in entries}
    t_end = time.time() + seconds
    seed = 0
    while time.time() < t_end or seed < len(entries):
        name, fn = entries[seed % len(entries)]
        rng = np.random.default_rng(seed0 + seed)
        g = torch.Generator().manual_seed(seed0 + seed)
        seed += 1
        st = stats[name]
        try:
            faults, ratio, info = fn(rng, g)
        except Refused:
            st["refused"] += 1
            continue
        finally:
            L.restore_options()
            torch.cuda.synchronize()
        st["cases"] += 1
        st["worst"] = max(st["worst"], ratio)
        if faults or not ratio <= 1.0:
            st["bad"] += 1
            print(f"MISMATCH {name} seed {seed0 + seed - 1}: {info}: error / tolerance {ratio:.3g} {'; '.join(faults)}", flush=True)
    bad = sum(s["bad"] for s in stats.values())
    idle = [n for n, s in stats.items() if s["cases"] == 0]
    print(f"{'entry point':44s} {'cases':>6s} {'refused':>8s} {'worst err/tol':>14s}")
    for n, s in stats.items():
        print(f"{n:44s} {s['cases']:6d} {s['refused']:8d} {s['worst']:14.3g}")
    extra = (summary() or []) if summary is not None else []
    print(f"{sum(s['cases'] for s in stats.values())} cases in {seconds:.0f} s, {bad} mismatches" + (f"; no accepted case: {', '.join(idle)}" if idle else "")
          + (f"; {len(extra)} summary failures" if extra else ""))
    print(f"{label} FUZZ", "FAILED" if (bad or idle or extra) else "OK")
    return 1 if (bad or idle or extra) else 0


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sys.exit(_main(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0))


if __name__ == "__main__":
    main()
