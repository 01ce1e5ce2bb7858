"""GPU: pp_attention at 192 tokens x head dim 80 (ViT-H, csrc/pp_attention_hd80.hip) against attention64 in fp64.

Tolerances are tests/fuzz_layer.py's own, applied as its case_attention applies them: TOL["attention"] (f16x3, f32) or
TOL["attention_bf16"] relative and absolute, plus peaked_atol(max |logit|, max |v|) on the absolute part. Every case runs between
canaries, checks that its input is unchanged and that a second launch gives the same bits (tests/fuzz_attention_hd80.py
attention_case). Then the fuzzer over random head counts and sequence counts for a few seconds, and the refusals: another head dim
stays PP_ERR_UNSUPPORTED with "not instantiated" in the text, and a qkv tensor with NaN on either side of it gives a finite result -
the zeros that pad a head row to 96 are never read from behind the head's 80 values."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

PRECS = {"f16x3": 2, "bf16": 0, "f32": 1}
# (class, sink key): the sink in the first and in the last 16 keys
VALUE_CLASSES = [("normal", 0), ("peaked_self", 0), ("peaked_sink", 5), ("peaked_sink", 192 - 3)]


@pytest.mark.parametrize("cls,sink", VALUE_CLASSES)
@pytest.mark.parametrize("n_seq", [1, 7, 128])
@pytest.mark.parametrize("heads", [1, 3, 16])
@pytest.mark.parametrize("precision", list(PRECS))
def test_attention_192x80_against_fp64(precision, heads, n_seq, cls, sink):
    import fuzz_attention_hd80 as Fz

    seed = 1000 * heads + 10 * n_seq + sink
    faults, ratio, info = Fz.attention_case(PRECS[precision], n_seq, heads, cls, seed, target=30.0 + (seed % 31), sink_key=sink)
    print(f"{info}: error / tolerance {ratio:.3g}")
    assert not faults, (info, faults)
    assert ratio <= 1.0, f"{info}: error / tolerance {ratio:.3g}"


def test_fuzz_of_the_new_shape():
    r = subprocess.run([sys.executable, os.path.join(HERE, "fuzz_attention_hd80.py"), "8"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ATTENTION HD80 FUZZ OK" in r.stdout, (r.stdout[-1500:], r.stderr[-800:])


@pytest.mark.parametrize("precision", list(PRECS))
def test_other_head_dims_are_still_refused(precision):
    from probpose_code_amd import _lib as L

    heads, hd = 4, 48
    dt = torch.bfloat16 if precision == "bf16" else torch.float32
    qkv = torch.zeros(192, 3 * heads * hd, dtype=dt, device="cuda")
    out = torch.zeros(192, heads * hd, dtype=dt, device="cuda")
    with pytest.raises(L.ProbPoseLibraryError) as exc:
        L.call("pp_attention", PRECS[precision], qkv.data_ptr(), out.data_ptr(), 1, 192, heads, hd, hd ** -0.5, None)
    assert "UNSUPPORTED" in str(exc.value) and "not instantiated" in str(exc.value) and "80" in str(exc.value)
    # 432 tokens at head dim 80 is out of scope: refused as well
    qkv = torch.zeros(432, 3 * 80, dtype=dt, device="cuda")
    out = torch.zeros(432, 80, dtype=dt, device="cuda")
    with pytest.raises(L.ProbPoseLibraryError) as exc:
        L.call("pp_attention", PRECS[precision], qkv.data_ptr(), out.data_ptr(), 1, 432, 1, 80, 80 ** -0.5, None)
    assert "UNSUPPORTED" in str(exc.value)


@pytest.mark.parametrize("heads", [1, 16])
@pytest.mark.parametrize("precision", list(PRECS))
def test_nan_around_qkv_does_not_reach_the_result(precision, heads):
    """qkv sits between two stretches of NaN in one allocation: 0 * NaN = NaN, so a padding read from behind the last head's v part
    (or from in front of the first q) would show in the output."""
    import fuzz_attention_hd80 as Fz
    from probpose_code_amd import _lib as L
    from probpose_code_amd.weights import from_split, to_split

    n_seq, E = 2, heads * 80
    gd = torch.Generator(device="cuda").manual_seed(5)
    q = Fz.make_qkv(n_seq, heads, "normal", gd)
    if precision == "f16x3":
        q = to_split(q.float().reshape(-1)).reshape(q.shape)  # (blocked by the flat element index: heads = 1 has rows of 240 elements)
        nan_dt, nan_bits = torch.int16, 0x7E00  # fp16 NaN in every half
    elif precision == "bf16":
        q = q.to(torch.bfloat16)
        nan_dt, nan_bits = torch.int16, 0x7FC0
    else:
        nan_dt, nan_bits = torch.int32, 0x7FC00000
    raw = q.contiguous().view(torch.uint8).reshape(-1)
    pad = 1 << 16
    buf = torch.empty(raw.numel() + 2 * pad, dtype=torch.uint8, device="cuda")
    buf.view(nan_dt).fill_(nan_bits)
    buf[pad:pad + raw.numel()] = raw
    out = torch.empty(n_seq * 192, E, dtype=q.dtype, device="cuda")
    L.call("pp_attention", PRECS[precision], buf.data_ptr() + pad, out.data_ptr(), n_seq, 192, heads, 80, 80 ** -0.5, None)
    torch.cuda.synchronize()
    got = from_split(out.reshape(-1)).cpu() if precision == "f16x3" else out.float().cpu()
    assert bool(torch.isfinite(got).all()), "NaN from outside the qkv tensor reached the attention output"
