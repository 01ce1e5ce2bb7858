#!/usr/bin/env python
"""dev only: SHA-256 of the output buffer of every form pp_attention serves, at fixed seeds - the "same bits" check of a change to
the attention kernels that must not move their arithmetic. Per form (the table of tests/test_attention_forms_gpu.py) three grids:
(n_seq, heads) = (1, 3) and (2, 4), the test's, and the workload's (128, 12) ((128, 16) at head dim 80). Run it against a build of
each of the two commits and compare the listings:
    python scripts/attention_digest.py > digest.txt"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16, F32, F16X3 = 0, 1, 2
NAMES = {BF16: "bf16", F32: "f32", F16X3: "f16x3"}
FORMS = ([(BF16, S, hd, 1) for S, hd in ((192, 32), (192, 64), (432, 32), (432, 64), (192, 80))] +
         [(F32, S, hd, 1) for S, hd in ((192, 32), (192, 64), (432, 32), (192, 80))] +
         [(F16X3, S, hd, 1) for S, hd in ((192, 32), (192, 64), (192, 80), (432, 32), (432, 64))] +
         [(F16X3, 432, hd, 0) for hd in (32, 64)])


def main():
    from probpose_code_amd import _lib as L
    from probpose_code_amd.weights import to_split

    for prec, S, hd, dma in FORMS:
        for n_seq, heads in ((1, 3), (2, 4), (128, 16 if hd == 80 else 12)):
            E = heads * hd
            g = torch.Generator().manual_seed(1000 * S + 10 * hd + heads)
            qkv = torch.randn(n_seq * S, 3 * E, generator=g) * 1.3
            if prec == F16X3:
                qd = to_split(qkv.reshape(-1)).reshape(n_seq * S, 3 * E).cuda()
            else:
                qd = qkv.to(torch.bfloat16 if prec == BF16 else torch.float32).cuda()
            out = torch.zeros((n_seq * S, E), dtype=qd.dtype, device="cuda")
            L.set_option("attn_dma", dma)
            try:
                L.call("pp_attention", prec, qd.data_ptr(), out.data_ptr(), n_seq, S, heads, hd, hd ** -0.5, None)
            finally:
                L.set_option("attn_dma", 1)
            torch.cuda.synchronize()
            raw = out.view(torch.uint8).cpu().numpy().tobytes()
            print(f"{NAMES[prec]:5s} {S}x{hd:<2d} attn_dma {dma} n_seq {n_seq:3d} heads {heads:2d}  {hashlib.sha256(raw).hexdigest()}", flush=True)


if __name__ == "__main__":
    main()
