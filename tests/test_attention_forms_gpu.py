"""GPU: one table over every form pp_attention serves - the kernels of csrc/pp_attention.hip, pp_attention_hd80.hip and
pp_attention_dma.hip, which are put together from the shared pieces of csrc/pp_attention_core.h - each at two grids:
(n_seq, heads) = (1, 3), a block count that is no multiple of 8 (plain block ids), and (2, 4), 8 blocks or 32 with the four query
quarters (XCD-aware remap). The 27 query tiles of the 432-token split forms over four quarters include the six-tile last quarter.

Every case: the output against attention64 in fp64 (tests/fuzz_layer.py) under the tolerance the existing test of that precision
uses (test_kernels_gpu.ATTENTION_TOL, test_split_fp16.TOL; head dim 80: fuzz_layer's, as tests/fuzz_attention_hd80.py applies
them), one launch tallied for the source file that should serve the case and none for the other two, and the canary rows behind
the output untouched. The random inputs differ per head and per sequence, so a wrong head or sequence offset shows."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

BF16, F32, F16X3 = 0, 1, 2
FILES = ("pp_attention.hip", "pp_attention_dma.hip", "pp_attention_hd80.hip")
# (precision, tokens, head dim, attn_dma)
FORMS = ([(BF16, S, hd, 1) for S, hd in ((192, 32), (192, 64), (432, 32), (432, 64), (192, 80))] +
         [(F32, S, hd, 1) for S, hd in ((192, 32), (192, 64), (432, 32), (192, 80))] +
         [(F16X3, S, hd, 1) for S, hd in ((192, 32), (192, 64), (192, 80), (432, 32), (432, 64))] +
         [(F16X3, 432, hd, 0) for hd in (32, 64)])
CANARY_ROWS, CANARY_BITS = 8, 0x7FC0BEEF  # a NaN pattern in fp32 and, its upper half, in bf16


def served_by(prec, S, hd, dma):
    if hd == 80:
        return "pp_attention_hd80.hip"
    return "pp_attention_dma.hip" if prec == F16X3 and S == 432 and dma else "pp_attention.hip"


@pytest.mark.parametrize("n_seq,heads", [(1, 3), (2, 4)])
@pytest.mark.parametrize("prec,S,hd,dma", FORMS)
def test_attention_form(prec, S, hd, dma, n_seq, heads):
    import fuzz_layer as FL
    import test_kernels_gpu as TK
    import test_split_fp16 as TS
    from probpose_code_amd import _lib as L
    from probpose_code_amd.weights import from_split, to_split

    E = heads * hd
    qkv = TK._rand(n_seq * S, 3 * E, seed=1000 * S + 10 * hd + heads, scale=1.3)
    if prec == F16X3:  # (the format blocks a tensor by its flat element index: head dim 80 x 3 heads is no whole number of blocks per row)
        qd, seen = to_split(qkv.reshape(-1)).reshape(n_seq * S, 3 * E).cuda(), qkv.double()
    else:
        qd, seen = qkv.to(TK._dt(prec)).cuda(), TK._q(qkv, prec)
    buf = torch.empty((n_seq * S + CANARY_ROWS, E), dtype=qd.dtype, device="cuda")
    buf.view(torch.int16 if prec == BF16 else torch.int32).fill_(CANARY_BITS >> 16 if prec == BF16 else CANARY_BITS)
    canary = buf[n_seq * S:].clone()
    before = [L.launch_count(f) for f in FILES]
    L.set_option("attn_dma", dma)
    try:
        L.call("pp_attention", prec, qd.data_ptr(), buf.data_ptr(), n_seq, S, heads, hd, hd ** -0.5, None)
    finally:
        L.set_option("attn_dma", 1)
    torch.cuda.synchronize()
    rose = {f: L.launch_count(f) - b for f, b in zip(FILES, before)}
    assert rose == {f: int(f == served_by(prec, S, hd, dma)) for f in FILES}, rose

    bits = torch.int16 if prec == BF16 else torch.int32
    assert torch.equal(buf[n_seq * S:].view(bits), canary.view(bits)), "rows behind n_seq * S were written"

    out = buf[:n_seq * S]
    got = from_split(out.reshape(-1).cpu()).reshape(n_seq * S, E).double() if prec == F16X3 else out.cpu().double()
    ref = FL.attention64(seen, n_seq, S, heads, hd, hd ** -0.5)
    if hd == 80:
        base = FL.TOL["attention_bf16"] if prec == BF16 else FL.TOL["attention"]
        ml = FL.max_logit64(seen, n_seq, S, heads, hd, hd ** -0.5)
        mv = float(seen.reshape(n_seq * S, 3, E)[:, 2].abs().max())
        ratio = FL.error_ratio(got, ref, base, base + FL.peaked_atol(ml, mv))
        print(f"error / tolerance {ratio:.3g}")
        assert ratio <= 1.0, f"error / tolerance {ratio:.3g}"
    else:
        torch.testing.assert_close(got, ref, **(TS.TOL if prec == F16X3 else TK.ATTENTION_TOL[prec]))
