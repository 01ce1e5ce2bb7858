"""References for the ViTPose ``-simple`` head (helper, no test): FeatureMapProcessor(scale_factor=4.0, apply_relu=True) in front of
HeatmapHead(deconv_out_channels=[], final_layer=dict(kernel_size=3, padding=1)).

* ``reference_order``: the reference's own order of operations in torch - ``conv2d(interpolate(relu(x), None, 4.0, "bilinear",
  align_corners=False), W, b, padding=1)`` (necks/fmap_proc_neck.py:66-70, models/utils/ops.py:60, heatmap_head.py:198-213) - in fp32
  or fp64. tests/golden/simple_head.npz pins it to the reference's classes (tests/test_simple_head_host.py).
* ``taps_of`` / ``composed``: the form the device runs (csrc/pp_simple_head.hip) - the nine taps at low resolution, then

      out[k, Y, X] = bias[k] + sum over the taps with 0 <= Y + dy < 4h and 0 <= X + dx < 4w of bil(T[3 (dy + 1) + dx + 1, k], Y + dy, X + dx)
      bil(P, Y', X'): sy = max((Y' + 0.5) / 4 - 0.5, 0), y0 = floor(sy), y1 = min(y0 + 1, h - 1), ly = sy - y0; x likewise
                      = (1 - ly) ((1 - lx) P[y0, x0] + lx P[y0, x1]) + ly ((1 - lx) P[y1, x0] + lx P[y1, x1])

  in numpy, in fp64 (the reference of the GPU test) or with every operation rounded to fp32 (an emulation of a kernel), together with
  ``S = |bias| + sum of weight x |tap|`` per output - the scale of the rounding bound ``41 * 2^-24 * S``: the weights and their products
  are exact, then one rounding per product or nested weight, at most 36 additions of terms and the bias - at most 40 roundings on any
  path whichever order a kernel sums in, plus one for the second-order term. ``fault=`` builds the single faults that bound must reject.
* ``relu_f32_bits`` / ``relu_bf16_bits`` / ``relu_split_bits``: pp_relu_operand bit for bit.
* ``calibrated_state_dict``: ``synthetic_state_dict(head="heatmap-simple")`` with ``bias[k] = -mean`` of the reference's bias-free,
  unflipped maps of keypoint k over ``synthetic_crops(16, seed=5)``: ReLU'd final-LayerNorm features have channel means that centred
  weights do not cancel, and the DARK decode takes a logarithm - with the generator's own bias 69 of the 1088 flip-averaged reference
  maps at B 64 have no positive value.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

BOUND = 41 * 2.0 ** -24  # x S
FAULTS = ("clamp_outside", "align_corners", "no_clamp0", "no_clamp_y1", "transposed", "bias_per_tap")


def reference_order(x: torch.Tensor, weight: torch.Tensor, bias, dtype=torch.float32, apply_relu: bool = True) -> torch.Tensor:
    """x (B, E, h, w), weight (K, E, 3, 3), bias (K) or None -> (B, K, 4h, 4w) in ``dtype``."""
    x, weight = x.to(dtype), weight.to(dtype)
    r = F.relu(x) if apply_relu else x
    up = F.interpolate(r, None, 4.0, "bilinear", align_corners=False)
    return F.conv2d(up, weight, None if bias is None else bias.to(dtype), padding=1)


def taps_of(x: torch.Tensor, weight: torch.Tensor, dtype=torch.float64, apply_relu: bool = True) -> np.ndarray:
    """The tap planes (B, 9 K, h * w), plane t K + k = relu(x) . W[k, :, dy + 1, dx + 1] with t = 3 (dy + 1) + (dx + 1)."""
    x, weight = x.to(dtype), weight.to(dtype)
    r = F.relu(x) if apply_relu else x
    B, E, h, w = r.shape
    K = weight.shape[0]
    t = torch.einsum("behw,keyx->byxkhw", r, weight)  # (B, 3, 3, K, h, w)
    return t.reshape(B, 9 * K, h * w).numpy()  # (in ``dtype``; the device's planes are fp32)


def _axis(n_low: int, d: int, dtype, fault):
    """Coordinates c = 0 .. 4 n_low - 1 of the output, sampled at c + d: (i0, i1, l, in_map) per coordinate."""
    c = np.arange(4 * n_low) + d
    in_map = (c >= 0) & (c < 4 * n_low)
    if fault == "clamp_outside":
        c = np.clip(c, 0, 4 * n_low - 1)
        in_map = np.ones_like(in_map)
    cf = c.astype(dtype)
    if fault == "align_corners":
        s = cf * dtype(n_low - 1) / dtype(max(4 * n_low - 1, 1))
    else:
        s = (cf + dtype(0.5)) / dtype(4) - dtype(0.5)
    if fault == "no_clamp0":
        i0 = np.trunc(s).astype(np.int64)  # (int)s of an unclamped coordinate: -0.375 -> 0 with the weight -0.375
    else:
        s = np.maximum(s, dtype(0))
        i0 = np.floor(s).astype(np.int64)
    l = (s - i0.astype(dtype)).astype(dtype)
    i1 = i0 + 1
    if fault != "no_clamp_y1":
        i1 = np.minimum(i1, n_low - 1)
    return i0, i1, l, in_map


def _rows(P, idx, axis):
    """P indexed along ``axis`` with idx; indices outside the plane read zero (what the faulty variants fall into)."""
    n = P.shape[axis]
    ok = (idx >= 0) & (idx < n)
    g = np.take(P, np.clip(idx, 0, n - 1), axis=axis)
    shape = [1] * P.ndim
    shape[axis] = -1
    return np.where(ok.reshape(shape), g, 0).astype(P.dtype)


def composed(taps: np.ndarray, bias: np.ndarray, K: int, h: int, w: int, dtype=np.float64, fault=None):
    """taps (n, 9 K, h * w) fp32 (fp64 taps are taken as they are: the algebra check), bias (K) -> (out (n, K, 4h, 4w) in ``dtype``,
    S (n, K, 4h, 4w) fp64). ``dtype=np.float32`` rounds every operation to fp32 (products, nested weights, additions: no fused multiply-add)."""
    assert fault is None or fault in FAULTS, fault
    taps = np.asarray(taps)
    n = taps.shape[0]
    assert taps.shape == (n, 9 * K, h * w)
    T = taps.reshape(n, 9, K, h, w)
    b = np.asarray(bias).astype(dtype).reshape(1, K, 1, 1)
    out = np.broadcast_to(b, (n, K, 4 * h, 4 * w)).astype(dtype).copy()
    S = np.broadcast_to(np.abs(b).astype(np.float64), out.shape).copy()
    if fault == "bias_per_tap":
        out[:] = 0
    for dy in (-1, 0, 1):
        y0, y1, ly, iny = _axis(h, dy, dtype, fault)
        for dx in (-1, 0, 1):
            x0, x1, lx, inx = _axis(w, dx, dtype, fault)
            t = 3 * (dx + 1) + (dy + 1) if fault == "transposed" else 3 * (dy + 1) + (dx + 1)
            mask = (iny[:, None] & inx[None, :])[None, None]
            for P, acc, D in ((T[:, t].astype(dtype), out, dtype), (np.abs(T[:, t]).astype(np.float64), S, np.float64)):
                wy1, wx1 = ly.astype(D), lx.astype(D)
                wy0, wx0 = D(1) - wy1, D(1) - wx1  # exact in either type
                if acc is S:  # (a faulty variant may have a negative weight)
                    wy0, wy1, wx0, wx1 = np.abs(wy0), np.abs(wy1), np.abs(wx0), np.abs(wx1)
                r0, r1 = _rows(P, y0, 2), _rows(P, y1, 2)
                top = wx0 * _rows(r0, x0, 3) + wx1 * _rows(r0, x1, 3)
                bot = wx0 * _rows(r1, x0, 3) + wx1 * _rows(r1, x1, 3)
                v = wy0[:, None] * top + wy1[:, None] * bot
                if fault == "bias_per_tap" and acc is out:
                    v = v + b
                assert v.dtype == D
                acc += np.where(mask, v, D(0))
    return out, S


# shapes (n_img, K, h, w) of the gather kernel's tests: one sample, one row, 2 x 2, odd sizes, the model's 16 x 12, and planes of more than one
# 16 x 16 tile with K = 133 (COCO-WholeBody)
GATHER_SHAPES = ((1, 1, 1, 1), (3, 17, 1, 3), (2, 21, 2, 2), (3, 17, 3, 5), (2, 17, 16, 12), (1, 133, 24, 18))


def gather_inputs(n_img: int, K: int, h: int, w: int, seed: int = 0):
    """The inputs of pp_taps_upsample4_conv3x3's tests for one shape, as (name, taps (n_img, 9 K, h * w) fp32, bias (K) fp32): random taps;
    one impulse per tap plane at each corner of the low-resolution plane (tap t weighs 1 + t / 16, so that a swapped or clamped tap shows; a
    wrong border rule moves or scales the corner's footprint); a constant plane per tap (the output counts the in-map taps: 4, 6 or 9)."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    out = [("random", (rng.standard_normal((n_img, 9 * K, h * w)) * 2).astype(np.float32), rng.standard_normal(K).astype(np.float32))]
    tap_w = (1 + np.arange(9) / 16).astype(np.float32)
    for name, (cy, cx) in (("impulse_tl", (0, 0)), ("impulse_tr", (0, w - 1)), ("impulse_bl", (h - 1, 0)), ("impulse_br", (h - 1, w - 1))):
        t = np.zeros((n_img, 9, K, h, w), np.float32)
        t[:, :, :, cy, cx] = tap_w[None, :, None]
        out.append((name, t.reshape(n_img, 9 * K, h * w), np.zeros(K, np.float32)))
    out.append(("constant", np.ones((n_img, 9 * K, h * w), np.float32), np.zeros(K, np.float32)))
    return out


# ------------------------------------------------------------------------------------------ pp_relu_operand, bit for bit
def relu_f32_bits(u32: np.ndarray) -> np.ndarray:
    x = u32.view(np.float32)
    return np.where((x > 0) | np.isnan(x), u32, np.uint32(0)).astype(np.uint32)


def relu_bf16_bits(u16: np.ndarray) -> np.ndarray:
    x = (u16.astype(np.uint32) << 16).view(np.float32)
    return np.where((x > 0) | np.isnan(x), u16, np.uint16(0)).astype(np.uint16)


def relu_split_bits(u16: np.ndarray) -> np.ndarray:
    """(..., 2 * row_len) halves of the split-fp16 container: blocks of 32 hi halves followed by 32 lo halves (csrc/pp_split.h). An element
    becomes (+0, +0) unless float(hi) + float(lo) > 0 or that sum is NaN."""
    blk = u16.reshape(-1, 2, 32)
    with np.errstate(invalid="ignore"):
        v = blk[:, 0].view(np.float16).astype(np.float32) + blk[:, 1].view(np.float16).astype(np.float32)
    keep = (v > 0) | np.isnan(v)
    return np.where(keep[:, None, :], blk, np.uint16(0)).astype(np.uint16).reshape(u16.shape)


# ------------------------------------------------------------------------------------------ the end-to-end reference
def features(sd, crops: torch.Tensor, num_heads: int = 12) -> torch.Tensor:
    """oracle.model_ref.vit_forward features (B, E, Hp, Wp) fp32 of uint8 crops."""
    from oracle import model_ref as M
    from probpose_code_amd import synthetic as S

    with torch.no_grad():
        return M.vit_forward(sd, M.preprocess(crops, S.IMG_MEAN, S.IMG_STD), num_heads)


def reference_heatmaps(sd, crops: torch.Tensor, flip: bool, num_heads: int = 12) -> np.ndarray:
    """HeatmapHead.predict's maps of the ``-simple`` model on the CPU in the reference's order, fp32: (a + flip_back(b)) * 0.5 under flip test
    (tests/test_vitpose_estimator_gpu.py::oracle_heatmaps for this head)."""
    from probpose_code_amd import synthetic as S

    W, b = sd["head.final_layer.weight"], sd["head.final_layer.bias"]
    with torch.no_grad():
        a = reference_order(features(sd, crops, num_heads), W, b)
        if flip:
            f = reference_order(features(sd, crops.flip(-1), num_heads), W, b)
            a = (a + f.flip(-1)[:, list(S.COCO_FLIP_INDICES)]) * 0.5
    return a.float().numpy()


@functools.lru_cache(maxsize=4)
def _calibrated(seed: int, arch: str):
    from probpose_code_amd import synthetic as S

    sd = S.synthetic_state_dict(arch, seed=seed, logit_scale=2.0, head="heatmap-simple")
    heads = S.ARCHS[arch]["num_heads"]
    with torch.no_grad():
        maps = reference_order(features(sd, S.synthetic_crops(16, seed=5), heads), sd["head.final_layer.weight"], None)
    sd["head.final_layer.bias"] = -maps.mean(dim=(0, 2, 3)).float()
    return sd


def calibrated_state_dict(seed: int = 0, arch: str = "small"):
    """A fresh dict of shared tensors per call (callers must not write into them)."""
    return dict(_calibrated(seed, arch))
