"""The fp64 references and tolerances of tests/fuzz_layer.py and tests/fuzz_head.py, on the CPU: (a) every reference agrees with an independent
torch form of the same operation in fp64; (b) the fuzzers' tolerances reject two simulated faulty kernels - one that drops the low halves of the
split operands (fp16 operands), one with bf16 operands - while the split format's own rounding passes. Emulated in fp64, no GPU needed: a kernel
that silently lost precision would fail the fuzzers."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fuzz_head as FH  # noqa: E402
import fuzz_layer as FL  # noqa: E402


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


# ------------------------------------------------------------------------------------------------- (a) references vs torch
def test_attention_reference_vs_sdpa():
    n_seq, S, heads, hd = 3, 40, 4, 32
    qkv = _rand(n_seq * S, 3 * heads * hd, seed=1, scale=1.3)
    q, k, v = qkv.reshape(n_seq, S, 3, heads, hd).permute(2, 0, 3, 1, 4)
    want = F.scaled_dot_product_attention(q, k, v, scale=hd ** -0.5).transpose(1, 2).reshape(n_seq * S, heads * hd)
    torch.testing.assert_close(FL.attention64(qkv, n_seq, S, heads, hd, hd ** -0.5), want, rtol=1e-12, atol=1e-12)
    assert FL.max_logit64(qkv, n_seq, S, heads, hd, hd ** -0.5) == pytest.approx(float((q @ k.transpose(-1, -2) * hd ** -0.5).abs().max()))


def test_layernorm_gelu_and_statistics_vs_torch():
    x = _rand(7, 384, seed=2) * 3 + _rand(7, 1, seed=3) * 10
    g, b = 1 + 0.1 * _rand(384, seed=4), _rand(384, seed=5, scale=0.1)
    ln = torch.nn.LayerNorm(384, eps=FL.EPS, dtype=torch.float64)
    with torch.no_grad():
        ln.weight.copy_(g), ln.bias.copy_(b)
        torch.testing.assert_close(FL.layernorm64(x, g, b), ln(x), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(FL.gelu64(x), F.gelu(x), rtol=1e-12, atol=1e-12)
    st = FL.row_stats64(x)
    torch.testing.assert_close(st[:, 0], x.mean(1))
    torch.testing.assert_close(st[:, 1], torch.rsqrt(x.var(1, unbiased=False) + FL.EPS))
    ps = FL.row_part_stats64(x)
    assert ps.shape == (7, 4, 2)
    torch.testing.assert_close(ps[:, 2, 1], x[:, 192:288].var(1, unbiased=False) * 96)


def test_ffn_and_projection_references_vs_nn_modules():
    E, Fd, M = 64, 128, 9
    att, r = _rand(M, E, seed=6), _rand(M, E, seed=7)
    proj, fc1, fc2 = (torch.nn.Linear(i, o, dtype=torch.float64) for i, o in ((E, E), (E, Fd), (Fd, E)))
    ln2 = torch.nn.LayerNorm(E, eps=FL.EPS, dtype=torch.float64)
    with torch.no_grad():
        ln2.weight.copy_(1 + 0.1 * _rand(E, seed=8))
        x_mid = r + proj(att)
        h_mid = ln2(x_mid)
        want = x_mid + fc2(F.gelu(fc1(h_mid)))
        got = FL.proj_ffn64(att, r, proj.weight, proj.bias, ln2.weight, ln2.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    for a, b in zip(got, (x_mid, h_mid, want)):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


def test_head_references_vs_torch_convolutions():
    B, Cin, Cout, H, W, K = 2, 16, 32, 5, 4, 7
    x = _rand(B, Cin, H, W, seed=10)
    w, b = _rand(Cin, Cout, 4, 4, seed=11, scale=0.2), _rand(Cout, seed=12)
    wf, bf = _rand(K, Cout, seed=13, scale=0.2), _rand(K, seed=14)
    mid = F.relu(F.conv_transpose2d(x, w, b, stride=2, padding=1))
    torch.testing.assert_close(FH.deconv_head64(x, w, b, wf, bf), F.conv2d(mid, wf[:, :, None, None], bf), rtol=1e-12, atol=1e-12)
    # the phase matrices the kernel is handed reproduce the same transposed convolution
    ph = FH.deconv_phases(w)
    xp = F.pad(x, (1, 1, 1, 1)).permute(0, 2, 3, 1)
    for py in range(2):
        for px in range(2):
            taps = torch.cat([xp[:, py + ty:py + ty + H, px + tx:px + tx + W] for ty in range(2) for tx in range(2)], dim=-1)
            torch.testing.assert_close((taps @ ph[py, px].t() + b).relu(), mid[:, :, py::2, px::2].permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    w3, b3 = _rand(Cout, Cin, 3, 3, seed=15, scale=0.1), _rand(Cout, seed=16)
    y = F.conv2d(F.pad(x, (0, 2, 3, 0)), w3, b3, padding=1)  # 8 x 6 maps
    torch.testing.assert_close(FH.conv3x3_64(F.pad(x, (0, 2, 3, 0)), w3, b3), y, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(FH.pool_relu64(y, 4, 3), F.relu(F.max_pool2d(y, (4, 3))), rtol=0, atol=0)


def test_tower_final_reference_elementwise():
    B, C, K = 3, 8, 5
    feat, w, bias = _rand(4, 2 * B, C, seed=20), _rand(4, K, C, seed=21), _rand(4, K, seed=22)
    fi = torch.tensor([0, 2, 1, 4, 3])
    got = FH.tower_final64(feat, w, bias, fi, B, 2, 7.0)
    for t in range(4):
        for i in range(B):
            for k in range(K):
                act = (lambda z: 1 / (1 + math.exp(-z))) if t < 3 else (lambda z: max(z, 0.0) / 7.0)
                a = act(float(feat[t, i] @ w[t, k] + bias[t, k]))
                f = act(float(feat[t, B + i] @ w[t, fi[k]] + bias[t, fi[k]]))
                assert got[t, i, k].item() == pytest.approx(0.5 * (a + f), rel=1e-12, abs=1e-15)


# ------------------------------------------------------------------------------------------------- (b) the tolerances catch lost precision
def _split_rounded(x):
    """x as the split format holds it (hi = fp16(x), lo = fp16(x - hi), hi + lo: weights.to_split / from_split element by element): what a
    correct kernel multiplies."""
    x = x.float()
    hi = x.half()
    return (hi.float() + (x - hi.float()).half().float()).double()


ROUNDINGS = {"split": _split_rounded, "fp16 (low halves dropped)": lambda x: x.half().double(), "bf16": lambda x: x.bfloat16().double()}


def _verdicts(compute, tol, atol=None):
    """compute(rounding) -> (got, ref) for every operand rounding; -> {name: error / tolerance}."""
    return {name: FL.error_ratio(*compute(rnd), tol, tol if atol is None else atol) for name, rnd in ROUNDINGS.items()}


def _check(v):
    assert v["split"] <= 1.0, v
    assert v["fp16 (low halves dropped)"] > 1.0 and v["bf16"] > 1.0, v


def test_tolerances_reject_lost_precision_linear_and_gemm_layernorm():
    M, N, K = 64, 192, 768
    x, w, b = _rand(M, K, seed=30), _rand(N, K, seed=31, scale=1 / math.sqrt(K)), _rand(N, seed=32, scale=0.1)
    ref = x @ w.t() + b
    _check(_verdicts(lambda rd: (rd(x) @ rd(w).t() + b, ref), FL.TOL["linear"]))
    g, be = 1 + 0.1 * _rand(N, seed=33), _rand(N, seed=34, scale=0.1)
    r = _rand(M, N, seed=35)
    h_ref = FL.layernorm64(ref + r, g, be)
    _check(_verdicts(lambda rd: (FL.layernorm64(rd(x) @ rd(w).t() + b + r, g, be), h_ref), FL.TOL["gemm_ln"]))


def test_tolerances_reject_lost_precision_ffn_chain():
    M, E, Fd = 32, 384, 1536
    att, r = _rand(M, E, seed=40), _rand(M, E, seed=41)
    wp, bp = _rand(E, E, seed=42, scale=1 / math.sqrt(E)), _rand(E, seed=43, scale=0.2)
    w1, b1 = _rand(Fd, E, seed=44, scale=1 / math.sqrt(E)), _rand(Fd, seed=45, scale=0.2)
    w2, b2 = _rand(E, Fd, seed=46, scale=1 / math.sqrt(Fd)), _rand(E, seed=47, scale=0.2)
    g2, be2 = 1 + 0.1 * _rand(E, seed=48), _rand(E, seed=49, scale=0.1)
    ref = FL.proj_ffn64(att, r, wp, bp, g2, be2, w1, b1, w2, b2)[2]

    def faulty(rd):  # every MFMA operand through the rounding: att, Wp, ln2 rows, W1, hidden activation, W2
        x_mid = r + rd(att) @ rd(wp).t() + bp
        h = rd(FL.layernorm64(x_mid, g2, be2))
        return x_mid + rd(FL.gelu64(h @ rd(w1).t() + b1)) @ rd(w2).t() + b2, ref
    _check(_verdicts(faulty, FL.TOL["proj_ffn"]))


def test_tolerances_reject_lost_precision_attention_and_peaked_bound():
    n_seq, S, heads, hd = 2, 192, 2, 32
    qkv = _rand(n_seq * S, 3 * heads * hd, seed=50, scale=1.3)
    ref = FL.attention64(qkv, n_seq, S, heads, hd, hd ** -0.5)
    _check(_verdicts(lambda rd: (FL.attention64(rd(qkv), n_seq, S, heads, hd, hd ** -0.5), ref), FL.TOL["attention"]))
    # peaked logits (k = c q: max |logit| ~ 50): the split rounding still passes the derived bound, fp16 / bf16 operands do not
    pk = qkv.reshape(n_seq * S, 3, heads, hd).clone()
    pk[:, 1] = pk[:, 0] * 4.0
    pk = pk.reshape(n_seq * S, -1)
    ml = FL.max_logit64(pk, n_seq, S, heads, hd, hd ** -0.5)
    assert 30 <= ml <= 120
    mv = float(pk.reshape(n_seq * S, 3, -1)[:, 2].abs().max())
    ref = FL.attention64(pk, n_seq, S, heads, hd, hd ** -0.5)
    tol = FL.TOL["attention"]
    _check(_verdicts(lambda rd: (FL.attention64(rd(pk), n_seq, S, heads, hd, hd ** -0.5), ref), tol, tol + FL.peaked_atol(ml, mv)))


def test_tolerances_reject_lost_precision_head_convolutions():
    B, C, H, W = 1, 128, 8, 6
    x, w, b = _rand(B, C, H, W, seed=60), _rand(C, C, 3, 3, seed=61, scale=1 / math.sqrt(9 * C)), _rand(C, seed=62)
    ref = FH.pool_relu64(FH.conv3x3_64(x, w, b), 4, 3)
    _check(_verdicts(lambda rd: (FH.pool_relu64(FH.conv3x3_64(rd(x), rd(w), b), 4, 3), ref), FH.TOL["conv_pool"]))
    _check(_verdicts(lambda rd: (FH.pool_relu64(FH.conv3x3_64(rd(x), rd(w), b), 4, 3), ref), FH.TOL["winograd"]))
    xd, wd, bd = _rand(1, 256, 4, 3, seed=63), _rand(256, 256, 4, 4, seed=64, scale=1 / math.sqrt(4 * 256)), _rand(256, seed=65, scale=0.2)
    wf, bf = _rand(17, 256, seed=66, scale=4 / math.sqrt(256)), _rand(17, seed=67)
    ref = FH.deconv_head64(xd, wd, bd, wf, bf)
    _check(_verdicts(lambda rd: (FH.deconv_head64(rd(xd), rd(wd), bd, rd(wf), bf), ref), FH.TOL["deconv_head"]))
