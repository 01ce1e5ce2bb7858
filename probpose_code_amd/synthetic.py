"""Seeded synthetic weights and inputs for tests and ``bench.py`` (there is no network for
the published ``ProbPose-s.pth``, reference ``README.md:119-120``).

The state dict uses the reference's own key names (``backbone.*`` as
mmpretrain's ``VisionTransformer`` names them, ``head.*`` from ``probmap_head.py``), so the
same loader path that would ingest the real checkpoint is exercised.

Why not the reference's default init (``probmap_head.py:592-598``: Normal std 0.001)? It gives
logits ~ 0, Sparsemax ~ uniform 1/3072 and an argmax that is pure rounding noise,
which makes keypoint parity meaningless. The init below keeps activations O(1) through the
network and scales the last 1x1 conv so that logits have a spread of a few units: after
``/temperature`` + Sparsemax the maps are sparse and peaked like a trained model's. BatchNorm
running statistics and affine parameters are randomised so that BN folding is really tested.
"""
import math
from typing import Dict, Sequence

import torch

COCO_FLIP_INDICES = (0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15)
IMG_MEAN = (123.675, 116.28, 103.53)
IMG_STD = (58.395, 57.12, 57.375)

ARCHS = {
    # config :58 (explicit dict): embed 384, 12 layers, 12 heads (head_dim 32), FFN 1536
    "small": dict(embed_dims=384, num_layers=12, num_heads=12, feedforward_channels=1536),
    # mmpretrain preset "base" (BASELINE config 4): 768 / 12 / 12 heads (head_dim 64) / 3072
    "base": dict(embed_dims=768, num_layers=12, num_heads=12, feedforward_channels=3072),
    # mmpretrain presets "large" and "huge" (ViTPose-L / -H): 16 heads of 64 / of 80
    "large": dict(embed_dims=1024, num_layers=24, num_heads=16, feedforward_channels=4096),
    "huge": dict(embed_dims=1280, num_layers=32, num_heads=16, feedforward_channels=5120),
}


TRAINED_MASSIVE = (250.0, -120.0, 60.0)  # residual-stream values of the massive-activation channels (stats="trained")


def _trained_like(sd: Dict[str, torch.Tensor], E: int, L: int, heads: int, g: torch.Generator,
                  massive=TRAINED_MASSIVE, row_offset: float = 8.0, gamma_decades: float = 2.0,
                  small_rows: float = 1e-2) -> Dict[str, torch.Tensor]:
    """Re-parametrise the O(1) network above into the statistics a TRAINED ViT shows (the published ``ProbPose-s.pth``,
    ``README.md:119-120``, cannot be fetched; this is what its numerics must survive) - in place, same key names:

      * massive activations (Sun et al. 2024): ``len(massive)`` channels of the residual stream sit at 60 .. 250x the
        typical magnitude from the second layer on - injected through that layer's ``fc2`` bias, its ``fc2`` rows for
        those channels 20x wider so that the values also vary per token; every LayerNorm behind it carries a small
        gamma there and a gamma ~ row std on the ordinary channels (what training arrives at: the normalised ordinary
        channels would otherwise shrink to 1 / std);
      * LayerNorm gamma log-uniform over ``gamma_decades`` decades, the Linear layer behind it with the inverse column
        scale (function preserved, the stored weights are what changes);
      * a per-token offset of the whole row of up to ``row_offset`` (token mean / std up to ~ ``row_offset`` in the first
        layers) through ``pos_embed``;
      * weight rows down to ``small_rows`` of their width: q rows scaled by s with the k rows of the same head
        dimension by 1 / s, v rows by s with the ``proj`` columns by 1 / s, ``fc1`` rows by s with the ``fc2`` columns
        by 1 / sqrt(s) (fp16 subnormal low halves in the split format).
    """
    u = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    hd = E // heads
    n_mass = len(massive)
    chans = torch.randperm(E, generator=g)[:n_mass]
    inject = min(1, L - 1)
    mass_std = math.sqrt(sum(m * m for m in massive) / E)  # what the massive channels add to a row's std
    sd["backbone.pos_embed"] = sd["backbone.pos_embed"] + (u(1, sd["backbone.pos_embed"].shape[1], 1) * 2 - 1) * row_offset
    p = f"backbone.layers.{inject}."
    sd[p + "ffn.layers.1.bias"][chans] += torch.tensor(massive)
    sd[p + "ffn.layers.1.weight"][chans] *= 20.0

    def widen(depth):
        """What a LayerNorm behind the injection must multiply the ordinary channels with to hand on what the O(1) network's
        LayerNorm would: row std with the massive channels / row std without (the latter grows ~ 0.8 + 0.38 per layer)."""
        return math.sqrt(1.0 + (mass_std / (0.8 + 0.38 * depth)) ** 2)

    def regamma(ln_key, lin_keys, depth, after_massive):
        gam = 10.0 ** ((u(E) - 0.5) * gamma_decades)
        comp = 1.0 / gam  # the Linear behind sees gamma * norm(x): keep the product
        sd[ln_key + ".bias"] = sd[ln_key + ".bias"] * gam
        if after_massive:
            gam = gam * widen(depth)
            gam[chans] = 0.02 + 0.08 * u(n_mass)
            comp[chans] = 1.0
        sd[ln_key + ".weight"] = sd[ln_key + ".weight"] * gam
        for k in lin_keys:
            sd[k] = sd[k] * comp[None, :]

    for i in range(L):
        p = f"backbone.layers.{i}."
        regamma(p + "ln1", [p + "attn.qkv.weight"], i, i > inject)
        regamma(p + "ln2", [p + "ffn.layers.0.0.weight"], i + 0.5, i > inject)
        # small rows, function preserved
        s = small_rows ** u(heads, hd)  # log-uniform in [small_rows, 1]
        wq = sd[p + "attn.qkv.weight"].reshape(3, heads, hd, E)
        bq = sd[p + "attn.qkv.bias"].reshape(3, heads, hd)
        sv = small_rows ** u(heads, hd)
        for part, sc in ((0, s), (1, 1.0 / s), (2, sv)):
            wq[part] *= sc[..., None]
            bq[part] *= sc
        sd[p + "attn.proj.weight"] = sd[p + "attn.proj.weight"] / sv.reshape(1, E)
        sf = small_rows ** u(sd[p + "ffn.layers.0.0.weight"].shape[0])
        sd[p + "ffn.layers.0.0.weight"] = sd[p + "ffn.layers.0.0.weight"] * sf[:, None]
        sd[p + "ffn.layers.0.0.bias"] = sd[p + "ffn.layers.0.0.bias"] * sf
        sd[p + "ffn.layers.1.weight"] = sd[p + "ffn.layers.1.weight"] / sf.sqrt()[None, :]
    # the final LayerNorm feeds the head: small gamma on the massive channels, ordinary channels back at O(1)
    if L > inject + 1:
        gf = sd["backbone.ln1.weight"] * widen(L)
        gf[chans] = 0.02 + 0.08 * u(n_mass)
        sd["backbone.ln1.weight"] = gf
    return sd


def synthetic_state_dict(arch: str = "small", img_size=(256, 192), num_keypoints: int = 17,
                         deconv_out_channels: Sequence[int] = (256, 256), seed: int = 0,
                         logit_scale: float = 3.0, stats: str = "unit", head: str = "probmap", **trained_kw) -> Dict[str, torch.Tensor]:
    """``stats="unit"``: activations O(1) everywhere (the weights every round-1..5 parity figure was taken on);
    ``stats="trained"``: the same network re-parametrised to a trained ViT's statistics (``_trained_like``).
    ``head="heatmap"``: the state dict of a ``HeatmapHead`` model (the ViTPose baseline) - the same backbone and heatmap branch
    (the same tensors as ``head="probmap"`` at equal seed, the final layer's weights centred per keypoint), no scalar-tower keys.
    ``head="heatmap-simple"``: the head of the ViTPose ``-simple`` variants - the same backbone, no deconvolution keys,
    ``head.final_layer.weight`` (K, E, 3, 3) at std ``logit_scale / sqrt(9 E)``, centred per keypoint, drawn from a generator stream of its
    own (the other heads' tensors do not move); ``deconv_out_channels`` is ignored."""
    if head not in ("probmap", "heatmap", "heatmap-simple"):
        raise ValueError(f"head must be 'probmap', 'heatmap' or 'heatmap-simple', got {head!r}")
    if stats not in ("unit", "trained"):
        raise ValueError(f"stats must be 'unit' or 'trained', got {stats!r}")
    a = ARCHS[arch] if isinstance(arch, str) else arch
    E, L, Fd = a["embed_dims"], a["num_layers"], a["feedforward_channels"]
    g = torch.Generator().manual_seed(seed)
    n = lambda *s, std=1.0: torch.randn(*s, generator=g) * std  # noqa: E731
    u = lambda *s, lo=0.5, hi=1.5: torch.rand(*s, generator=g) * (hi - lo) + lo  # noqa: E731
    xav = lambda o, i: n(o, i, std=math.sqrt(2.0 / (o + i)))  # noqa: E731
    sd: Dict[str, torch.Tensor] = {}
    P = 16
    Hp, Wp = (img_size[0] + 4 - P) // P + 1, (img_size[1] + 4 - P) // P + 1
    sd["backbone.patch_embed.projection.weight"] = n(E, 3, P, P, std=math.sqrt(1.0 / (3 * P * P)))
    sd["backbone.patch_embed.projection.bias"] = n(E, std=0.1)
    sd["backbone.pos_embed"] = n(1, Hp * Wp, E, std=0.3)
    for i in range(L):
        p = f"backbone.layers.{i}."
        for ln in ("ln1", "ln2"):
            sd[p + ln + ".weight"] = 1.0 + n(E, std=0.1)
            sd[p + ln + ".bias"] = n(E, std=0.1)
        sd[p + "attn.qkv.weight"] = n(3 * E, E, std=1.5 / math.sqrt(E))
        sd[p + "attn.qkv.bias"] = n(3 * E, std=0.1)
        sd[p + "attn.proj.weight"] = xav(E, E)
        sd[p + "attn.proj.bias"] = n(E, std=0.05)
        sd[p + "ffn.layers.0.0.weight"] = xav(Fd, E)
        sd[p + "ffn.layers.0.0.bias"] = n(Fd, std=0.1)
        sd[p + "ffn.layers.1.weight"] = xav(E, Fd)
        sd[p + "ffn.layers.1.bias"] = n(E, std=0.05)
    sd["backbone.ln1.weight"] = 1.0 + n(E, std=0.1)
    sd["backbone.ln1.bias"] = n(E, std=0.1)

    def bn(prefix, c):
        sd[prefix + ".weight"] = u(c)
        sd[prefix + ".bias"] = n(c, std=0.2)
        sd[prefix + ".running_mean"] = n(c, std=0.2)
        sd[prefix + ".running_var"] = u(c)
        sd[prefix + ".num_batches_tracked"] = torch.tensor(1000)

    cin = E
    for j, cout in enumerate(deconv_out_channels):
        # ConvTranspose2d weight is (Cin, Cout, 4, 4); each output pixel sees 2x2 taps x Cin inputs
        sd[f"head.deconv_layers.{3 * j}.weight"] = n(cin, cout, 4, 4, std=math.sqrt(2.0 / (4 * cin)))
        bn(f"head.deconv_layers.{3 * j + 1}", cout)
        cin = cout
    sd["head.final_layer.weight"] = n(num_keypoints, cin, 1, 1, std=logit_scale / math.sqrt(cin))
    sd["head.final_layer.bias"] = n(num_keypoints, std=0.1)
    if head == "heatmap-simple":
        for k in [k for k in sd if k.startswith("head.deconv_layers.")]:
            del sd[k]
        gs = torch.Generator().manual_seed(seed + 7919)  # its own stream: nothing the other heads draw moves
        w = torch.randn(num_keypoints, E, 3, 3, generator=gs) * (logit_scale / math.sqrt(9 * E))
        # centred per keypoint, for the reason given below: the 3x3 conv reads ReLU'd (non-negative) features
        sd["head.final_layer.weight"] = w - w.mean(dim=(1, 2, 3), keepdim=True)
    if head == "heatmap":
        # HeatmapHead's maps are decoded as they are (no Sparsemax in front). A 1x1 conv of random sign on ReLU'd (non-negative) maps gives every
        # keypoint's map an offset of either sign, large against its peaks; with the flip-test average of two unrelated passes a map then often has
        # no positive value at all. Weights centred per keypoint take that offset out: the maps swing around zero, their maxima are positive.
        w = sd["head.final_layer.weight"]
        sd["head.final_layer.weight"] = w - w.mean(dim=1, keepdim=True)
    for t in ("probability", "visibility", "oks", "error") if head == "probmap" else ():
        for j in range(3):
            sd[f"head.{t}_layers.{4 * j}.weight"] = n(E, E, 3, 3, std=math.sqrt(2.0 / (9 * E)))
            sd[f"head.{t}_layers.{4 * j}.bias"] = n(E, std=0.1)
            bn(f"head.{t}_layers.{4 * j + 1}", E)
        sd[f"head.{t}_layers.12.weight"] = n(num_keypoints, E, 1, 1, std=1.0 / math.sqrt(E))
        sd[f"head.{t}_layers.12.bias"] = n(num_keypoints, std=0.3)
    if stats == "trained":
        _trained_like(sd, E, L, a["num_heads"], g, **trained_kw)
    return sd


def head_kind_of(cfg) -> str:
    """``head=`` of ``synthetic_state_dict`` for a config's ``model.head.type``: "heatmap" for ``HeatmapHead`` (the ViTPose baseline) -
    "heatmap-simple" when it has no deconvolutions (the ``-simple`` variants) -, "probmap" otherwise."""
    head_cfg = dict(dict(cfg["model"]).get("head") or {})
    head_type = str(head_cfg.get("type", "ProbMapHead"))
    if head_type.split(".")[-1] not in ("HeatmapHead", "HeatmapHeadMI355X"):
        return "probmap"
    return "heatmap" if head_cfg.get("deconv_out_channels", (256, 256, 256)) else "heatmap-simple"


def arch_of(cfg) -> Dict[str, int]:
    """``arch=`` of ``synthetic_state_dict`` for a config's ``model.backbone.arch``: the explicit dict, or the preset a name stands for in
    ``VisionTransformer`` ("base", "large", "huge": the ViTPose family)."""
    arch = dict(dict(cfg["model"]).get("backbone") or {}).get("arch", "base")
    if isinstance(arch, str):
        from .pose_estimators import _VIT_ARCHS

        if arch.lower() not in _VIT_ARCHS:
            raise ValueError(f"model.backbone.arch={arch!r} is not in the default archs {sorted(_VIT_ARCHS)}")
        arch = _VIT_ARCHS[arch.lower()]
    return {k: int(dict(arch)[k]) for k in ("embed_dims", "num_layers", "num_heads", "feedforward_channels")}


def synthetic_crops(batch: int, img_size=(256, 192), seed: int = 0) -> torch.Tensor:
    """uint8 BGR crops (B,3,H,W), uniform [0,255] as ``mmpose/testing/_utils.py:117`` does, but
    low-pass filtered a little so that neighbouring patches correlate like an image's."""
    g = torch.Generator().manual_seed(seed)
    H, W = img_size
    coarse = torch.rand((batch, 3, H // 8, W // 8), generator=g)
    fine = torch.rand((batch, 3, H, W), generator=g)
    img = 0.6 * torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False) + 0.4 * fine
    return (img * 255).round().clamp(0, 255).to(torch.uint8)


def whole_image_bbox_meta(batch: int, img_size=(256, 192), padding: float = 1.25):
    """input_center / input_scale of a whole-image bbox (apis/inference.py:168 + TopdownAffine
    padding, topdown_transforms.py:96-101): centre (W/2, H/2), scale (W, H) * 1.25."""
    import numpy as np

    H, W = img_size
    center = np.tile(np.array([W / 2, H / 2], np.float32), (batch, 1))
    scale = np.tile(np.array([W * padding, H * padding], np.float32), (batch, 1))
    return center, scale


def synthetic_coco_dataset(root: str, n_images: int, seed: int = 0, image_size=(640, 480), fmt: str = "png",
                           persons=(1, 8), invalid_image: bool = True, id_base: int = 0) -> int:
    """A seeded COCO-format keypoint set under ``root``: ``root/val2017/*.{png,jpg}`` (written by PIL) and
    ``root/annotations/person_keypoints_val2017.json``, ``persons`` boxes per image (some partly outside the image), 17
    keypoints each with random visibilities; the first image's instances are all crowd (invalid) when ``invalid_image``.
    Returns the number of valid instances. PNG decodes exactly on every decoder; JPEG is what a real set holds."""
    import json
    import os

    import numpy as np
    from PIL import Image

    rng = np.random.default_rng(seed)
    W, H = image_size
    os.makedirs(os.path.join(root, "val2017"), exist_ok=True)
    os.makedirs(os.path.join(root, "annotations"), exist_ok=True)
    yy, xx = np.mgrid[0:H, 0:W]
    images, anns, valid = [], [], 0
    for k in range(n_images):
        img_id = id_base + 1000 + 7 * k
        name = f"{img_id:012d}.{fmt}"
        base = (np.sin(xx / rng.uniform(8, 40) + rng.uniform(0, 6)) + np.cos(yy / rng.uniform(8, 40))) * 60 + 128
        img = np.clip(base[..., None] + rng.normal(0, 12, (H, W, 3)) + rng.uniform(-40, 40, 3), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, "val2017", name), **({"quality": 90} if fmt == "jpg" else {}))
        images.append(dict(id=img_id, file_name=name, width=W, height=H))
        for p in range(int(rng.integers(persons[0], persons[1] + 1))):
            w, h = rng.uniform(20, W * 0.6), rng.uniform(40, H * 0.9)
            x, y = rng.uniform(-0.2 * w, W - 0.8 * w), rng.uniform(-0.2 * h, H - 0.8 * h)
            v = rng.choice([0, 1, 2], 17, p=[0.2, 0.2, 0.6])
            kx, ky = rng.uniform(x, x + w, 17), rng.uniform(y, y + h, 17)
            kp = np.stack([np.where(v > 0, np.round(kx, 2), 0), np.where(v > 0, np.round(ky, 2), 0), v], 1)
            crowd = int(invalid_image and k == 0)
            nk = int((v > 0).sum())
            anns.append(dict(id=id_base * 100 + len(anns) + 1, image_id=img_id, category_id=1, iscrowd=crowd, num_keypoints=nk,
                             bbox=[round(float(x), 2), round(float(y), 2), round(float(w), 2), round(float(h), 2)],
                             area=round(float(w * h * 0.55), 2), keypoints=[float(t) if i % 3 < 2 else int(t) for i, t in enumerate(kp.flatten())]))
            valid += int(not crowd and nk > 0)
    doc = dict(images=images, annotations=anns, categories=[dict(id=1, name="person", supercategory="person")])
    with open(os.path.join(root, "annotations", "person_keypoints_val2017.json"), "w") as f:
        json.dump(doc, f)
    return valid
