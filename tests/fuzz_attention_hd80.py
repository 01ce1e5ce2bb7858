#!/usr/bin/env python
"""Fuzz of pp_attention at 192 tokens x head dim 80 (ViT-H; csrc/pp_attention_hd80.hip) against torch fp64: the generator of
tests/fuzz_layer.py's case_attention restricted to the new shape, in the three precisions. Value classes: unit-normal rows, peaked
attention with each query's arg-max key its own ("peaked_self") or one sink key per sequence among the first or the last 16 keys
("peaked_sink"), max |logit| 30 - 60. Every case: the output between canaries (compared bit for bit), every element written, the
input bit-identical after the launch, a repeat launch bit-identical, fp64 accuracy under fuzz_layer's own tolerances
(TOL["attention"] for f16x3 and f32, TOL["attention_bf16"] for bf16, plus peaked_atol on the absolute part).
``attention_case`` is the single case, imported by tests/test_attention_hd80_gpu.py for its fixed grid.
python tests/fuzz_attention_hd80.py [seconds]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fuzz_layer import BF16, F16X3, F32, MEM_CAP, TOL, Guard, Refused, attention64, error_ratio, max_logit64, peaked_atol, run_entries, run_twice  # noqa: E402

S, HD = 192, 80
CLASSES = ("normal", "peaked_self", "peaked_sink")


def make_qkv(n_seq, heads, cls, gd, target=45.0, sink_key=0):
    """(n_seq * S, 3 * heads * HD) fp32 rows on the GPU, as case_attention of tests/fuzz_layer.py draws them."""
    qkv = torch.randn(n_seq * S, 3, heads, HD, generator=gd, device="cuda") * 1.3
    if cls == "peaked_self":  # k = c q: each query's arg-max key is itself
        qkv[:, 1] = qkv[:, 0] * (target / (1.69 * HD * 1.5 * HD ** -0.5))
    elif cls == "peaked_sink":  # one sink key per sequence, aligned with a direction every query shares
        u = torch.randn(heads, HD, generator=gd, device="cuda")
        u = u / u.norm(dim=1, keepdim=True)
        qkv[:, 0] += (2.0 - (qkv[:, 0] * u).sum(-1, keepdim=True)) * u  # q . u = 2 for every query: every logit of the sink key = target
        qkv.view(n_seq, S, 3, heads, HD)[:, sink_key, 1] = u * (target / (2.0 * HD ** -0.5))
    elif cls != "normal":
        raise ValueError(cls)
    return qkv.reshape(n_seq * S, 3 * heads * HD)


def attention_case(prec, n_seq, heads, cls, seed, target=45.0, sink_key=0, rng=None):
    """One guarded launch pair of pp_attention(prec, ..., 192, heads, 80) -> (faults, error / tolerance, description)."""
    from probpose_code_amd import _lib as L
    from probpose_code_amd.weights import from_split, to_split

    E = heads * HD
    rng = rng if rng is not None else np.random.default_rng(seed)
    gd = torch.Generator(device="cuda").manual_seed(int(seed))
    qkv = make_qkv(n_seq, heads, cls, gd, target, sink_key)
    idx_seq = torch.unique(torch.tensor([0, n_seq - 1] + rng.integers(0, n_seq, 4).tolist())) if n_seq > 6 else torch.arange(n_seq)
    rows = (idx_seq[:, None] * S + torch.arange(S)).reshape(-1)
    guard = Guard()
    if prec == F16X3:
        # (the format blocks a tensor by its flat element index: with an odd head count a row of 240 * heads elements is not a whole number of blocks)
        qd, qq, odt = to_split(qkv.float().reshape(-1)).reshape(n_seq * S, 3 * E), qkv[rows].cpu().double(), torch.float32
    else:
        odt = torch.bfloat16 if prec == BF16 else torch.float32
        qd = qkv.to(odt).contiguous()
        qq = qkv[rows].to(odt).cpu().double()
    qd = guard.inp("qkv", qd)
    out = guard.out("out", (n_seq * S, E), dtype=odt)

    def go():
        try:
            L.call("pp_attention", prec, qd.data_ptr(), out.data_ptr(), n_seq, S, heads, HD, HD ** -0.5, None)
        except L.ProbPoseLibraryError as exc:
            if "UNSUPPORTED" in str(exc) or "INVALID" in str(exc):
                raise Refused(str(exc)) from None
            raise
        torch.cuda.synchronize()

    faults, snap = run_twice(guard, go)
    ns = len(idx_seq)
    ref = attention64(qq, ns, S, heads, HD, HD ** -0.5)
    ml = max_logit64(qq, ns, S, heads, HD, HD ** -0.5)
    mv = float(qq.reshape(ns * S, 3, E)[:, 2].abs().max())
    got = from_split(snap[0].reshape(-1)).reshape(n_seq * S, E)[rows].cpu().double() if prec == F16X3 else snap[0][rows].cpu().double()
    base = TOL["attention_bf16"] if prec == BF16 else TOL["attention"]
    ratio = error_ratio(got, ref, base, base + peaked_atol(ml, mv))
    return faults, ratio, f"prec {prec} heads {heads} n_seq {n_seq} class {cls} sink key {sink_key} max|logit| {ml:.1f}"


def _main(seconds):
    from probpose_code_amd import _lib as L

    def case(prec):
        def run(rng, g):
            heads = int(rng.integers(1, 17))
            n_seq = int(rng.choice([1, 2, 3, 7, 8, 64, 128, int(rng.integers(1, 300))]))
            n_seq = max(1, min(n_seq, int(MEM_CAP // (S * 4 * heads * HD * 4 * 2))))
            cls = str(rng.choice(CLASSES))
            target = float(rng.uniform(30, 60))
            sink = int(rng.integers(0, 16)) if rng.random() < 0.5 else S - 1 - int(rng.integers(0, 16))
            return attention_case(prec, n_seq, heads, cls, int(rng.integers(1 << 30)), target, sink, rng)
        return run

    entries = [("pp_attention 192 x 80 f16x3", case(F16X3)), ("pp_attention 192 x 80 bf16", case(BF16)), ("pp_attention 192 x 80 f32", case(F32))]
    return run_entries(entries, seconds, 91000, "ATTENTION HD80", L)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sys.exit(_main(float(sys.argv[1]) if len(sys.argv) > 1 else 30.0))


if __name__ == "__main__":
    main()
