"""The fp64 reference and the error model of tests/fuzz_mlp.py, on the CPU: (a) the unrounded reference chain agrees with torch modules
(nn.Linear, F.gelu, F.layer_norm, F.scaled_dot_product_attention) and the bf16 rounding with torch's; (b) the kernel's GELU polynomial - its
coefficients read out of pp_mlp.hip and evaluated as fp32 FMAs - stays within its documented 1.8e-4 of erf-GELU, and within the Lipschitz and
evaluation-error constants the model uses; (c) a faithful fp32 emulation of mlp_res_ln_kernel (bf16 roundings where the kernel rounds, fp32 sums in
a permuted order) passes the fuzzer's bound with margin on every value class; (d) emulations with one fault each fail it. No GPU needed: a kernel
with one of these faults would fail the fuzzer."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fuzz_mlp as FM  # noqa: E402

E, SEQ, HEADS, HD = FM.E, FM.SEQ, FM.HEADS, FM.HD


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _inputs(mode, M, F_, seed, cls="normal", wscale="unit", acls="normal"):
    """A launch's inputs as fp64 tensors holding bf16 / fp32 values, drawn as the fuzzer draws them."""
    proj, with_qkv, att = mode
    g = _gen(seed)

    def wt(n, k):
        return (torch.randn(n, k, generator=g) * (0.02 if wscale == "trained" else 1 / math.sqrt(k))).bfloat16().double()

    def vec(n, s):
        return (torch.randn(n, generator=g) * s).double()

    x = dict(w1=wt(F_, E), b1=vec(F_, 0.1), w2=wt(E, F_), b2=vec(E, 0.1), g=1 + 0.1 * vec(E, 1.0), be=vec(E, 0.1))
    if proj:
        x.update(wp=wt(E, E), bp=vec(E, 0.1), g2=1 + 0.1 * vec(E, 1.0), be2=vec(E, 0.1))
    if with_qkv:
        x.update(wq=wt(3 * E, E), bq=vec(3 * E, 0.3))
    x["res"] = FM.rows_of_class(M, E, cls, g, device="cpu").double()
    if att:
        scale = HD ** -0.5
        qkv = torch.randn(M, 3, HEADS, HD, generator=g) * 1.3
        if acls == "peaked":
            u = torch.randn(HEADS, HD, generator=g)
            u = u / u.norm(dim=1, keepdim=True)
            qkv[:, 0] += (2.0 - (qkv[:, 0] * u).sum(-1, keepdim=True)) * u
            for s in range(M // SEQ):
                qkv[s * SEQ + (3 if s % 2 == 0 else SEQ - 5), 1] = u * (45.0 / (2.0 * scale))
        x["qkv"], x["scale"] = qkv.reshape(M, 3 * E).bfloat16().double(), scale
    else:
        x["a"] = (FM.rows_of_class(M, E, "normal", g, device="cpu") * (0.7 if proj else 1.0)).bfloat16().double()
    return x


# ------------------------------------------------------------------------------------------------- the kernel, emulated in fp32
def _bf(x):
    return x.float().bfloat16().float()


def _trunc(x):
    return (x.float().view(torch.int32) & -65536).view(torch.float32)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def gelu32(x):
    """gelu_fast as the kernel evaluates it: clamp, fp32 FMAs."""
    t = x.clamp(-FM.GELU_CLAMP, FM.GELU_CLAMP)
    s = t * t
    c = [torch.tensor(v, dtype=torch.float32) for v in FM.GELU_COEF]
    q = _fma(s, c[0], c[1])
    for ci in c[2:]:
        q = _fma(s, q, ci)
    return x * _fma(t, q, torch.tensor(0.5))


def _mm32(a, w, perm):
    """fp32 products of fp32-exact operands, summed in fp32 in a permuted k order."""
    return a.float()[:, perm] @ w.float()[:, perm].t()


def _ln32(x, g, b):
    mean = x.sum(-1, keepdim=True) * torch.tensor(1.0 / E, dtype=torch.float32)
    c = x - mean
    var = (c * c).sum(-1, keepdim=True) * torch.tensor(1.0 / E, dtype=torch.float32)
    rs = 1.0 / torch.sqrt(var + FM.EPS)
    return c * rs * g.float() + b.float()


def emulate(mode, x, fault=None, seed=0):
    """mlp_res_ln_kernel in fp32 with the kernel's bf16 rounding points; fault names one deliberate error. -> {"x", "h", "qkv"} as fp64."""
    proj, with_qkv, att = mode
    gp = _gen(seed)
    M = x["res"].shape[0]
    F_ = x["w1"].shape[0]
    wg1 = slice(96, 192)  # the second workgroup's rows
    if att:
        q, k, v = x["qkv"].float().reshape(M // SEQ, SEQ, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
        s = q @ k.transpose(-1, -2)
        if fault == "neighbour_keys":  # queries 96..191 of sequence 0 attend to sequence 1's keys and values
            s[0, :, 96:] = q[0, :, 96:] @ k[1].transpose(-1, -2)
        if fault == "drop_key_tile":
            s[..., 16 * 5:16 * 6] = -math.inf
        mx = s.amax(-1, keepdim=True)
        sl2e = torch.tensor(x["scale"], dtype=torch.float32) * torch.tensor(FM.L2E32, dtype=torch.float32)
        mb = mx * sl2e
        p = torch.exp2(_fma(s, sl2e, -mb))
        P = _bf(p)
        num = P @ v
        if fault == "neighbour_keys":
            num[0, :, 96:] = P[0, :, 96:] @ v[1]
        O = num * (1.0 / P.sum(-1, keepdim=True))
        a = _bf(O).transpose(1, 2).reshape(M, E)
    else:
        a = x["a"].float()
    if proj:
        ap = a.clone()
        if fault == "proj_kstep":  # one 32-wide k-step of the projection missing in one workgroup
            ap[wg1, 32 * 7:32 * 8] = 0
        x1 = (x["res"].float() + x["bp"].float()) + _mm32(ap, x["wp"], torch.randperm(E, generator=gp))
        H = _bf(_ln32(x1, x["g2"], x["be2"]))
        xb = x1 + x["b2"].float()
    else:
        H = a
        xb = x["res"].float() + x["b2"].float()
    b1 = x["b1"].float().clone()
    if fault == "b1_chunk":
        b1[128:256] = 0
    G = _bf(gelu32(_mm32(H, x["w1"], torch.randperm(E, generator=gp)) + b1))
    if fault in ("drop_chunk_first", "drop_chunk_last"):  # workgroup 1 (xcd_rank 0: rotation 0) skips the first / last chunk it visits
        c = 0 if fault == "drop_chunk_first" else F_ // 128 - 1
        G[wg1, 128 * c:128 * (c + 1)] = 0
    xo = xb + _mm32(G, x["w2"], torch.randperm(F_, generator=gp))
    hf = _ln32(xo, x["g"], x["be"])
    out = {"x": xo.double(), "h": (_trunc(hf) if fault == "trunc_h" else _bf(hf)).double()}
    if with_qkv:
        bq = x["bq"].float().clone()
        if fault == "bq_block":
            bq[192 * 3:192 * 4] = 0
        qf = _mm32(_bf(hf), x["wq"], torch.randperm(E, generator=gp)) + bq
        out["qkv"] = (_trunc(qf) if fault == "trunc_qkv" else _bf(qf)).double()
    return out


# ------------------------------------------------------------------------------------------------- (a) references
def test_bf16_rounding_matches_torch():
    x = torch.cat([torch.randn(100000, generator=_gen(1)) * 10.0 ** torch.randint(-30, 30, (100000,), generator=_gen(2)).float(),
                   torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 2.0 ** -130, -3.0 * 2.0 ** -133, 1e38])])
    torch.testing.assert_close(FM.bf16(x.double()), x.bfloat16().double(), rtol=0, atol=0)
    half = FM.bf16_half_step(x.double())
    assert bool(((FM.bf16(x.double()) - x.double()).abs() <= half).all())
    r, e = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -10]).double(), torch.tensor([2.0 ** -20, 2.0 ** -20]).double()
    R, e2 = FM.flip(r, e)
    assert e2.tolist() == [2.0 ** -7, 0.0]  # on the boundary: one step; well inside an interval: none


@pytest.mark.parametrize("mode", [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)])
def test_layer_reference_vs_torch_modules(mode):
    proj, with_qkv, att = mode
    M, F_ = 2 * SEQ, 256
    x = _inputs(mode, M, F_, seed=3)
    got = FM.layer64(mode, x, exact_chain=True)
    lin = lambda i, o, w, b: torch.nn.Linear(i, o, dtype=torch.float64).requires_grad_(False)  # noqa: E731
    fc1, fc2 = lin(E, F_, None, None), lin(F_, E, None, None)
    fc1.weight.copy_(x["w1"]), fc1.bias.copy_(x["b1"]), fc2.weight.copy_(x["w2"]), fc2.bias.copy_(x["b2"])
    if att:
        q, k, v = x["qkv"].reshape(M // SEQ, SEQ, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
        a = F.scaled_dot_product_attention(q, k, v, scale=x["scale"]).transpose(1, 2).reshape(M, E)
        torch.testing.assert_close(FM.attention64(x["qkv"], M // SEQ, SEQ, HEADS, HD, x["scale"]), a, rtol=1e-12, atol=1e-12)
    else:
        a = x["a"]
    if proj:
        pr = lin(E, E, None, None)
        pr.weight.copy_(x["wp"]), pr.bias.copy_(x["bp"])
        x1 = x["res"] + pr(a)
        h2 = F.layer_norm(x1, (E,), x["g2"], x["be2"], FM.EPS)
    else:
        x1, h2 = x["res"], a
    xo = x1 + fc2(F.gelu(fc1(h2)))
    ho = F.layer_norm(xo, (E,), x["g"], x["be"], FM.EPS)
    torch.testing.assert_close(got["x"][0], xo, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(got["h"][0], ho, rtol=1e-10, atol=1e-10)
    if with_qkv:
        qk = lin(E, 3 * E, None, None)
        qk.weight.copy_(x["wq"]), qk.bias.copy_(x["bq"])
        torch.testing.assert_close(got["qkv"][0], qk(ho), rtol=1e-10, atol=1e-10)


# ------------------------------------------------------------------------------------------------- (b) the GELU polynomial
def test_gelu_polynomial_within_its_documented_error():
    x = torch.cat([torch.linspace(-12, 12, 2_000_001), torch.linspace(-0.05, 0.05, 100_001), torch.tensor([-4.2, 4.2, -4.25, 4.25, 0.0]),
                   torch.linspace(-1e4, 1e4, 200_001)])
    xd = x.double()
    poly = FM.gelu_poly64(xd)
    # the kernel's comment: |error| < 1.8e-4 + 1e-6 |x| against erf-GELU (t W(t^2) reaches 0.5 + 8e-7, not 0.5, at the clamp), for the
    # polynomial and for its fp32 evaluation
    for y in (poly, gelu32(x).double()):
        assert float(((y - F.gelu(xd)).abs() - 1e-6 * xd.abs()).max()) <= 1.8e-4
    inner = xd.abs() <= FM.GELU_CLAMP
    assert float((poly - F.gelu(xd))[inner].abs().max()) <= 1.8e-4
    ev = (gelu32(x).double() - poly).abs()
    assert bool((ev <= FM.gelu_eval_err(xd.abs())).all()), float((ev / FM.gelu_eval_err(xd.abs())).max())
    slope = (poly[1:2_000_001] - poly[:2_000_000]) / (xd[1:2_000_001] - xd[:2_000_000])
    assert float(slope.abs().max()) <= FM.GELU_LIP
    # saturation: x above the clamp passes (almost) unchanged, x below it goes (almost) to zero
    big = torch.tensor([5.0, 100.0, 3e4])
    assert bool(((gelu32(big) - big).abs() <= 1e-6 * big).all()) and bool((gelu32(-big).abs() <= 1e-6 * big).all())


# ------------------------------------------------------------------------------------------------- (c) / (d) the bound against emulations
MODES = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)]
CLASSES = [("normal", "unit", "normal"), ("offset", "trained", "normal"), ("massive", "unit", "peaked"), ("normal", "trained", "peaked"),
           ("offset", "unit", "peaked")]


def _worst(mode, x, fault=None, seed=0):
    """{output: error / bound} and {bf16 output: rounding bias} of the emulation"""
    ref = FM.layer64(mode, x)
    em = emulate(mode, x, fault, seed)
    return FM.ratios(ref, em), {k: FM.rounding_bias(em[k], ref[k][0]) for k in em if k != "x"}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cls", CLASSES)
def test_faithful_emulation_passes_with_margin(mode, cls):
    x = _inputs(mode, 2 * SEQ, 512, seed=11 + MODES.index(mode), cls=cls[0], wscale=cls[1], acls=cls[2])
    for seed in range(2):
        r, bias = _worst(mode, x, seed=seed)
        assert max(r.values()) < 0.5, r
        assert max(abs(b) for b in bias.values()) < FM.BIAS_LIMIT / 2, bias
    # the bound is finite everywhere and never looser than the fixed-shape tests' tolerance
    ref = FM.layer64(mode, x)
    for k, (rv, e) in ref.items():
        c = FM.capped(k, rv, e)
        assert bool(torch.isfinite(c).all()) and bool((c <= FM.BLANKET[k][1] + FM.BLANKET[k][0] * rv.abs()).all())


FAULTS = [("drop_chunk_first", MODES), ("drop_chunk_last", MODES), ("b1_chunk", MODES), ("proj_kstep", MODES[1:]), ("bq_block", [m for m in MODES if m[1]]),
          ("neighbour_keys", MODES[3:]), ("drop_key_tile", MODES[3:]), ("trunc_h", MODES), ("trunc_qkv", [m for m in MODES if m[1]])]


@pytest.mark.parametrize("fault,mode", [(f, m) for f, ms in FAULTS for m in ms])
def test_single_faults_fail_the_bound(fault, mode):
    """every fault fails the bound (error / bound > 1) or, for a truncating bf16 store, the rounding-bias check, on every class"""
    # (the key tile left out holds no sink key: with peaked attention its weights are ~e^-40 and the fault changes nothing, so no peaked rows)
    classes = [("normal", "unit", "normal"), ("offset", "trained", "normal")] + ([] if fault == "drop_key_tile" else [("massive", "trained", "peaked")])
    for cls in classes:
        x = _inputs(mode, 2 * SEQ, 512, seed=21, cls=cls[0], wscale=cls[1], acls=cls[2])
        r, bias = _worst(mode, x, fault)
        if fault.startswith("trunc_"):
            assert abs(bias[fault[6:]]) > FM.BIAS_LIMIT, (fault, cls, bias)
        else:
            assert max(r.values()) > 1.0, (fault, cls, r)
