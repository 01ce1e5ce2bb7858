"""The fp64 references and tolerances of tests/fuzz_layer.py, tests/fuzz_head.py and tests/fuzz_conv.py, on the CPU: (a) every reference agrees
with an independent torch form of the same operation in fp64; (b) the fuzzers' tolerances reject two simulated faulty kernels - one that drops the
low halves of the split operands (fp16 operands), one with bf16 operands - while the split format's own rounding passes; (c) the convolution
fuzzer's checks reject a gather that reads the neighbouring image instead of the zero pad, swapped deconvolution phases, one wrong border tap
under the bf16-output bound, and a pooling max that drops NaN. Emulated in fp64, no GPU needed: a kernel that silently lost precision would fail
the fuzzers."""
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


# ------------------------------------------------------------------------------------------------- tests/fuzz_conv.py: references and rejections
import fuzz_conv as FC  # noqa: E402


def test_conv_references_vs_torch():
    B, Cin, Cout, H, W = 2, 16, 24, 5, 3
    x = _rand(B, Cin, H, W, seed=70)
    w, b = _rand(Cin, Cout, 4, 4, seed=71, scale=0.2), _rand(Cout, seed=72)
    torch.testing.assert_close(FC.deconv64(x, w, b), F.conv_transpose2d(x, w, b, stride=2, padding=1), rtol=1e-12, atol=1e-12)
    w3 = _rand(Cout, Cin, 3, 3, seed=73, scale=0.2)
    for act, fn in ((FC.ACT_NONE, lambda y: y), (FC.ACT_RELU, F.relu), (FC.ACT_GELU, F.gelu)):
        torch.testing.assert_close(FC.act64(FH.conv3x3_64(x, w3, b), act), fn(F.conv2d(x, w3, b, padding=1)), rtol=1e-12, atol=1e-12)
    y = _rand(3, 4, 7, 5, seed=74)
    for ph, pw in ((2, 2), (3, 2), (7, 5), (4, 3), (1, 1)):
        torch.testing.assert_close(FC.pool_relu_floor64(y, ph, pw), F.relu(F.max_pool2d(y, (ph, pw))), rtol=0, atol=0)
    y[1, 2, 3, 1] = math.nan  # a NaN in a window pools to NaN (torch's MaxPool2d), and ReLU keeps it
    assert math.isnan(FC.pool_relu_floor64(y, 2, 2)[1, 2, 1, 0].item())


def test_im2col_and_layernorm_references_vs_torch():
    from oracle import model_ref as M

    g = torch.Generator().manual_seed(75)
    img = torch.randint(0, 256, (2, 3, 37, 21), generator=g, dtype=torch.uint8)
    mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    for pad in range(4):
        for passes in (1, 2):
            for bgr in (True, False):
                x = M.preprocess(img, mean, std, bgr_to_rgb=bgr).double()
                x = torch.cat([x, x.flip(-1)]) if passes == 2 else x
                Hp, Wp = (37 + 2 * pad - 16) // 16 + 1, (21 + 2 * pad - 16) // 16 + 1
                want = F.unfold(F.pad(x, (pad,) * 4)[:, :, :Hp * 16, :Wp * 16], 16, stride=16).transpose(1, 2).reshape(-1, 768)
                torch.testing.assert_close(FC.im2col64(img, mean, std, pad, passes, bgr), want, rtol=1e-6, atol=1e-6)
    x = _rand(9, 1024, seed=76) * 4 + 3
    g_, b_ = 1 + 0.1 * _rand(1024, seed=77), _rand(1024, seed=78)
    torch.testing.assert_close(FL.layernorm64(x, g_, b_), F.layer_norm(x, (1024,), g_, b_, FL.EPS), rtol=1e-12, atol=1e-12)
    assert FC.ulp32(torch.tensor([1.0], dtype=torch.float64)).item() == 2.0 ** -23


def test_conv_fuzz_rejects_neighbour_image_reads():
    """A 3x3 gather that reads the neighbouring image instead of the zero pad (the batch stacked as one tall image): the border impulses make it
    fail every tolerance of the fuzzer by far, while the correct convolution passes."""
    B, C, H, W = 3, 64, 6, 4
    x = FC.border_impulses(B, H, W, C, torch.Generator().manual_seed(79)).double().permute(0, 3, 1, 2)
    w, b = _rand(C, C, 3, 3, seed=80, scale=1 / math.sqrt(9 * C)), _rand(C, seed=81, scale=0.3)
    ref = FH.conv3x3_64(x, w, b)
    tall = FH.conv3x3_64(x.permute(1, 0, 2, 3).reshape(1, C, B * H, W), w, b).reshape(C, B, H, W).permute(1, 0, 2, 3)
    assert FC.bf16_out_ratio(ref.float().bfloat16().double(), ref) <= 1.0
    assert FC.bf16_out_ratio(tall, ref) > 20 and FL.error_ratio(tall, ref, FC.F32_TOL, FC.F32_TOL) > 1e3
    assert FL.error_ratio(tall, ref, FH.TOL["conv_pool"] * 8, FH.TOL["conv_pool"] * 8) > 1e3  # the f16x3 tolerance at the class's magnitude


def test_conv_fuzz_rejects_swapped_deconv_phases_and_lost_precision():
    B, Cin, Cout, H, W = 1, 128, 64, 4, 3
    x, w = _rand(B, Cin, H, W, seed=82), _rand(Cin, Cout, 4, 4, seed=83, scale=1 / math.sqrt(4 * Cin))
    ref = FC.deconv64(x, w)
    bad = ref.clone()
    bad[:, :, 0::2, 1::2], bad[:, :, 1::2, 0::2] = ref[:, :, 1::2, 0::2], ref[:, :, 0::2, 1::2]
    assert FL.error_ratio(bad, ref, FC.BF16_F32OUT_TOL, FC.BF16_F32OUT_TOL) > 10
    # f16x3 with fp16 operands (low halves lost) and the fp32 path with bf16 operands: rejected; the split rounding passes
    v = _verdicts(lambda rd: (FC.deconv64(rd(x), rd(w)), ref), FH.TOL["deconv_head"])
    _check(v)
    xc, wc = _rand(B, Cin, H, W, seed=84), _rand(Cout, Cin, 3, 3, seed=85, scale=1 / math.sqrt(9 * Cin))
    refc = FH.conv3x3_64(xc, wc)
    assert FL.error_ratio(FH.conv3x3_64(xc.float().double(), wc.float().double()), refc, FC.F32_TOL, FC.F32_TOL) <= 1.0
    assert FL.error_ratio(FH.conv3x3_64(xc.bfloat16().double(), wc.bfloat16().double()), refc, FC.F32_TOL, FC.F32_TOL) > 1.0


def test_conv_fuzz_bf16_output_bound_rejects_one_wrong_tap():
    """One product of one border pixel read from the neighbouring image instead of the zero pad: about 1 / sqrt(9 * 384) = 0.017 at unit
    activations. The flat 2e-2 of the fixed-shape tests lets it through; 2^-8 |ref| + 2e-3 on the bf16-rounded reference does not."""
    C = 384
    x = _rand(1, C, 4, 4, seed=86).bfloat16().double()
    w = _rand(C, C, 3, 3, seed=87, scale=1 / math.sqrt(9 * C)).bfloat16().double()
    ref = FH.conv3x3_64(x, w)
    co = int(ref[0, :, 0, 0].abs().argmin())
    c = int((w[co, :, 0, 1].abs() - 1 / math.sqrt(9 * C)).abs().argmin())  # a typical weight of the tap that leaves the image at (0, 0)
    bad = ref.clone()
    bad[0, co, 0, 0] += 1.0 * w[co, c, 0, 1]  # the neighbour's pixel (value 1) where the pad's 0 belongs
    got = bad.float().bfloat16().double()
    assert FL.error_ratio(got, ref, 2e-2, 2e-2) <= 1.0  # what the fixed tests say
    assert FC.bf16_out_ratio(ref.float().bfloat16().double(), ref) <= 1.0
    assert FC.bf16_out_ratio(got, ref) > 1.0, FC.bf16_out_ratio(got, ref)


def test_poison_check_rejects_a_nan_dropping_max():
    """The poison contract: a max that skips NaN (v_max_f32 / torch.fmax: the other operand) turns a window of NaN into -inf and ReLU into 0 -
    rejected; the NaN-keeping max passes, and so does a NaN the split format adds inside the reach."""
    B, C, H, W = 2, 32, 8, 6
    x = _rand(B, H, W, C, seed=88)
    g = torch.Generator().manual_seed(89)
    FH.poison_(x[0], g, 3)
    w = _rand(C, C, 3, 3, seed=90, scale=1 / math.sqrt(9 * C))
    conv = FH.conv3x3_64(x.permute(0, 3, 1, 2), w)
    ref = FC.pool_relu_floor64(conv, 4, 3)
    reach = FH.conv_reach(FH.bad_pixels(x), 4, 3)
    assert not bool(torch.isfinite(ref).all())
    assert FH.poison_ratio(ref, ref, reach, 1e-5, 1e-5) <= 1.0
    inside = ref.clone()
    inside[reach.expand_as(ref)] = math.nan  # every reached output NaN: allowed
    assert FH.poison_ratio(inside, ref, reach, 1e-5, 1e-5) <= 1.0
    c = conv.reshape(B, C, 2, 4, 2, 3).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2, 2, 12)
    m = torch.full(c.shape[:-1], -math.inf, dtype=torch.float64)
    for i in range(12):
        m = torch.fmax(m, c[..., i])
    dropped = torch.fmax(m, torch.zeros_like(m))
    assert FH.poison_ratio(dropped, ref, reach, 1e-5, 1e-5) == math.inf
    outside = ref.clone()
    outside[~reach.expand_as(ref)] = math.nan
    assert FH.poison_ratio(outside, ref, reach, 1e-5, 1e-5) == math.inf
    wino = FH.conv_reach(FH.bad_pixels(x), 4, 3, winograd=True)
    assert bool((wino | ~reach).all()), "the Winograd reach holds the direct convolution's"
