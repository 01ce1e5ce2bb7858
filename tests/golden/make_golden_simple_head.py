"""Pin tests/simple_head_ref.py to the REFERENCE's own classes for the ViTPose ``-simple`` neck and head.

Run in the build container only (needs the reference tree, see _ref_import.py):

    python tests/golden/make_golden_simple_head.py        ->  tests/golden/simple_head.npz

What runs here is the reference's own code, imported file by file behind the stubs of make_golden_head.py:

    mmpose/models/necks/fmap_proc_neck.py               FeatureMapProcessor(scale_factor=4.0, apply_relu=True).forward
    mmpose/models/utils/ops.py                          resize
    mmpose/models/heads/heatmap_heads/heatmap_head.py   HeatmapHead(deconv_out_channels=[], deconv_kernel_sizes=[],
                                                        final_layer=dict(kernel_size=3, padding=1)).forward

The fixture holds data only: the head's ``state_dict()`` key list and shapes, seeded weights (E 64, K 17), inputs of 4 x 3 and
16 x 12 maps at B 2 - values representable in fp16, stored as fp16 - and the fp32 outputs of ``head.forward(neck.forward((x,)))``.
tests/test_simple_head_host.py checks ``simple_head_ref.reference_order`` and the product's key names against it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_head as G  # noqa: E402  (the stubs: mmcv.cnn builders, mmengine BaseModule, registries)
from _ref_import import REF, _load, _shell  # noqa: E402


def main():
    G.load_reference_model()
    _load("mmpose.models.utils.ops", "mmpose/models/utils/ops.py")
    _shell("mmpose.models.necks", os.path.join(REF, "mmpose/models/necks"))
    neck_mod = _load("mmpose.models.necks.fmap_proc_neck", "mmpose/models/necks/fmap_proc_neck.py")
    _shell("mmpose.models.heads.heatmap_heads", os.path.join(REF, "mmpose/models/heads/heatmap_heads"))
    head_mod = _load("mmpose.models.heads.heatmap_heads.heatmap_head", "mmpose/models/heads/heatmap_heads/heatmap_head.py")
    E, K, B = 64, 17, 2
    neck = neck_mod.FeatureMapProcessor(scale_factor=4.0, apply_relu=True)
    head = head_mod.HeatmapHead(in_channels=E, out_channels=K, deconv_out_channels=[], deconv_kernel_sizes=[],
                                final_layer=dict(kernel_size=3, padding=1), loss=dict(type="KeypointMSELoss", use_target_weight=True),
                                decoder=None)
    head.eval()
    g = torch.Generator().manual_seed(0)
    weight = (torch.randn(K, E, 3, 3, generator=g) * 0.05).half().float()
    bias = torch.randn(K, generator=g).half().float()
    keys = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    head.load_state_dict({"final_layer.weight": weight, "final_layer.bias": bias}, strict=True)
    out = dict(state_keys=np.array(sorted(keys)), state_shapes=np.array([str(keys[k]) for k in sorted(keys)]),
               weight=weight.numpy().astype(np.float16), bias=bias.numpy().astype(np.float16))
    for name, (h, w) in (("small", (4, 3)), ("full", (16, 12))):
        x = (torch.randn(B, E, h, w, generator=g) * 3).half().float()
        with torch.no_grad():
            y = head.forward(neck.forward((x,)))
        assert tuple(y.shape) == (B, K, 4 * h, 4 * w) and y.dtype == torch.float32
        out[f"x_{name}"] = x.numpy().astype(np.float16)
        out[f"y_{name}"] = y.numpy()
    path = os.path.join(HERE, "simple_head.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
