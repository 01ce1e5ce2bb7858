"""The loss mode restated in numpy fp64 for the tests: the OKS map loss (OKSHeatmapLoss, oks_type "minus", per_pixel, reduced to its
mean), the scalar targets (gt_oks, oks_weight, gt_errs, the visibility weights) and the four scalar losses of ProbMapHead.loss.

Keyword arguments of ``map_loss`` switch single FAULTS on - the emulations the bound has to reject.

Bounds (u = 2^-24). The reference sums fp32 values in torch's order, which is not ours to know, so a sum of n fp32 terms v_i, each
computed with c rounded operations, is taken to be within ``(n - 1 + c) u sum(|m_i|)`` of the fp64 value - n - 1 additions in the worst
(sequential) order, m_i the term's sum of magnitudes (every signed intermediate replaced by its absolute value) - as
tests/fuzz_decode_logits.py charges its summation tree. ``MAP_OPS`` / ``SCALAR_OPS`` count the per-term operations generously.
gt_oks = exp(-e), e = (dx^2 + dy^2) / var / area / 2: coordinates within d (tests/udp_ref.decode_f64's bound, scaled to input pixels,
target plus prediction) move e by at most (2 |dx| d_x + d_x^2 + 2 |dy| d_y + d_y^2) / var / area / 2 =: de, and |exp(-a) - exp(-b)| <=
|a - b| for a, b >= 0; the float32 store adds u.
"""
import numpy as np

U = 2.0 ** -24
MAP_OPS = 40      # two 3x3 correlations (9 products, 8 additions each), two squares, their sum, three weighted terms, the mask
SCALAR_OPS = 12   # a logarithm or two (2 ulp each), a handful of products and differences
COCO_VARS = (np.array([0.26, 0.25, 0.25, 0.35, 0.35, 0.79, 0.79, 0.72, 0.72, 0.62, 0.62, 1.07, 1.07, 0.87, 0.87, 0.89, 0.89]) / 10.0 * 2) ** 2
OKS_AREA = 64 * 48 * 0.53 + np.spacing(1)


def _correlate3(p, k, pad):
    P = np.pad(p, [(0, 0)] * (p.ndim - 2) + [(1, 1), (1, 1)], mode="constant" if pad == "zero" else "reflect")
    H, W = p.shape[-2:]
    return sum(k[i][j] * P[..., i:i + H, j:j + W] for i in range(3) for j in range(3))


def map_loss(p, t, w, smoothing_weight, gaussian_weight=0.0, loss_weight=1.0, pad="zero", sobel_rows_swapped=False, use_mask=True,
             mean_over_masked=False):
    """(B, K, H, W) maps, (B, K) weights -> dict(loss, map_sums (B, K), magnitude: sum of the terms' magnitudes, n: pixel count)."""
    p, t, w = np.asarray(p, np.float64), np.asarray(t, np.float64), np.asarray(w, np.float64)
    kx = [[1, 0, -1], [2, 0, -2], [1, 0, -1]]
    ky = [[1, 2, 1], [0, 0, 0], [-1, -2, -1]]
    if sobel_rows_swapped:  # FAULT: the middle row of the x kernel with the other sign
        kx = [[1, 0, -1], [-2, 0, 2], [1, 0, -1]]
    gx, gy = _correlate3(p, kx, pad), _correlate3(p, ky, pad)
    ax, ay = _correlate3(np.abs(p), np.abs(kx), pad), _correlate3(np.abs(p), np.abs(ky), pad)
    ow = 1 - smoothing_weight - gaussian_weight
    m = w[:, :, None, None] if use_mask else np.ones_like(w)[:, :, None, None]
    px = smoothing_weight * (gx ** 2 + gy ** 2) * m + ow * (p * (1 - t)) * m + gaussian_weight * (p - t) ** 2 * m
    mag = (abs(smoothing_weight) * (ax ** 2 + ay ** 2) + abs(ow) * np.abs(p) * (1 + np.abs(t)) + abs(gaussian_weight) * (np.abs(p) + np.abs(t)) ** 2) * np.abs(m)
    n = px.size
    if mean_over_masked:  # FAULT: the mean over the unmasked pixels only
        n = int((np.broadcast_to(m, px.shape) != 0).sum())
    return dict(loss=px.sum() / n * loss_weight, map_sums=px.sum((2, 3)), magnitude=float(mag.sum()), map_magnitudes=mag.sum((2, 3)), n=px.size)


def map_loss_bound(r, loss_weight=1.0):
    return (r["n"] - 1 + MAP_OPS) * U * r["magnitude"] / r["n"] * abs(loss_weight)


def map_sums_bound(r):
    """(B, K): the bound of a per-map sum whose fp32 pixel values were added in fp64 (the fixture's ``pixel_loss_map_sums``, the kernel's
    ``map_sums``): the per-pixel operations alone are charged, which is what makes a fault at the border pixels visible."""
    return MAP_OPS * U * r["map_magnitudes"]


def argmax_first(maps):
    flat = np.asarray(maps).reshape(maps.shape[0], maps.shape[1], -1)
    return flat.argmax(-1), flat.max(-1)


def scalar_targets(kp_gt, kp_dt, in_image, annotated, visibility, freeze_oks=False, freeze_error=True, d_gt=None, d_dt=None):
    """Decoded coordinates (B, K, 2) f64, flags (B, K) -> dict(gt_oks, oks_weight, gt_errs, vis_weights[, gt_oks_bound]) in fp64.
    ``d_gt`` / ``d_dt`` (B, K, 2): coordinate bounds in input pixels for ``gt_oks_bound``."""
    w = (np.asarray(in_image) != 0) & (np.asarray(annotated) != 0)
    g = np.where(np.isnan(kp_gt), 0.0, kp_gt) * w[..., None]
    d = np.asarray(kp_dt, np.float64) * w[..., None]
    diff = d - g
    e = (diff[..., 0] ** 2 + diff[..., 1] ** 2) / COCO_VARS / OKS_AREA / 2
    has = w.any(1)
    live = w & has[:, None] & (not freeze_oks)
    with np.errstate(invalid="ignore"):
        gt_oks = np.where(live, np.exp(-e), 0.0)
    out = dict(gt_oks=gt_oks, oks_weight=(has & (not freeze_oks)).astype(np.float64))
    if d_gt is not None:
        dd = np.asarray(d_gt) + np.asarray(d_dt)
        de = ((2 * np.abs(diff) * dd + dd ** 2).sum(-1)) / COCO_VARS / OKS_AREA / 2
        out["gt_oks_bound"] = np.where(live, np.minimum(de + U, 1.0), 0.0)  # (both values lie in [0, 1])
    g1 = np.where(np.isnan(kp_gt), -1.0, kp_gt)
    out["gt_errs"] = np.zeros(w.shape) if freeze_error else np.linalg.norm(g1 - kp_dt, axis=2)
    ann, vis = np.asarray(annotated) != 0, np.asarray(visibility) != 0
    n_inv, n_vis = int((ann & ~vis).sum()), int((ann & vis).sum())
    wv = np.zeros(w.shape)
    if n_inv:
        wv[ann & ~vis] = np.float64(np.float32(1) / np.float32(n_inv))  # torch: 1 / (int tensor + 1e-10) is float32
    if n_vis:
        wv[ann & vis] = np.float64(np.float32(1) / np.float32(n_vis))
    if (wv > 0).any():
        wv = wv / wv[wv > 0].min()
    out["vis_weights"] = wv.astype(np.float32).astype(np.float64)
    return out


def _bce(p, t):
    with np.errstate(divide="ignore"):
        return -(t * np.maximum(np.log(p), -100) + (1 - t) * np.maximum(np.log(1 - p), -100))


def _sum_bound(terms_mag, extra=0.0):
    terms_mag = np.asarray(terms_mag, np.float64)
    return (terms_mag.size - 1 + SCALAR_OPS) * U * float(terms_mag.sum()) / terms_mag.size + extra


def scalar_losses(scalars, tg, in_image, annotated, visibility, gt_oks_bound=None):
    """scalars (4, B, K), ``tg`` = scalar_targets(...) -> dict name -> (value, bound) in fp64 for loss_probability, loss_visibility, loss_oks,
    loss_error, mae_oks, mae_err (loss weights 1; BCE on probabilities)."""
    s = np.asarray(scalars, np.float64)
    ann, inn = (np.asarray(annotated) != 0).astype(np.float64), ((np.asarray(annotated) != 0) & (np.asarray(in_image) != 0))
    w = inn.astype(np.float64)
    gb = np.zeros(w.shape) if gt_oks_bound is None else gt_oks_bound
    out = {}
    t = _bce(s[0], (np.asarray(in_image) != 0).astype(np.float64)) * ann
    out["loss_probability"] = (t.mean(), _sum_bound(np.abs(t)))
    t = _bce(s[1], (np.asarray(visibility) != 0).astype(np.float64)) * tg["vis_weights"]
    out["loss_visibility"] = (t.mean(), _sum_bound(np.abs(t)))
    d = s[2] * w - tg["gt_oks"] * w
    out["loss_oks"] = ((d ** 2).mean(), _sum_bound((np.abs(s[2]) + np.abs(tg["gt_oks"])) ** 2 * w, float((2 * np.abs(d) * gb + gb ** 2).mean())))
    a, b = np.log(1 + s[3]) * w, np.log(1 + tg["gt_errs"]) * w
    d = np.abs(a - b)
    out["loss_error"] = (np.where(d < 1, 0.5 * d ** 2, d - 0.5).mean(), _sum_bound(np.maximum((np.abs(a) + np.abs(b)) ** 2, np.abs(a) + np.abs(b) + 0.5)))
    if inn.any():
        out["mae_oks"] = (np.abs(s[2] - tg["gt_oks"])[inn].mean(), _sum_bound((np.abs(s[2]) + np.abs(tg["gt_oks"]))[inn], float(gb[inn].mean())))
        out["mae_err"] = (np.abs(s[3] - tg["gt_errs"])[inn].mean(), _sum_bound((np.abs(s[3]) + np.abs(tg["gt_errs"]))[inn]))
    return out
