"""The loss modules of the ProbPose config (``mmpose/models/losses``) and the pieces of ``ProbMapHead.loss``
(``mmpose/models/heads/hybrid_heads/probmap_head.py:806-1012``), FORWARD values only: what ``model.eval(); model(..., mode="loss")``
computes in the reference. There are no gradients here and nothing to train with.

* ``OKSHeatmapLoss`` (heatmap_loss.py:513-681), ``oks_type="minus"``: the mean of the per-pixel loss over all B K H W pixels, with
  the argmax pixel of every predicted and target map as a by-product - two launches, ``pp_probmap_loss_maps``.
* ``BCELoss`` (classification_loss.py:12-66), ``MSELoss`` (regression_loss.py:524-553), ``L1LogLoss`` (regression_loss.py:135-179):
  configuration holders. Their values for a batch come out of ONE launch, ``pp_probmap_loss_scalars`` (``probmap_loss_scalars``
  below), together with the scalar targets ``gt_oks`` / ``gt_errs`` and the visibility weights - instead of a few dozen elementwise
  torch launches on 17 B numbers.
* ``pose_accuracy`` / ``binary_accuracy``: ``pose_pck_accuracy(method="argmax")`` from the argmax pixels, and
  ``get_binary_accuracy(force_balanced=True)``, on the host in numpy - the latter draws from ``np.random`` with the reference's calls in
  the reference's order, so the same seed gives the reference's numbers.

A loss type or an option outside the ProbPose config is refused by name.
"""
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib

PP_LOSS_FREEZE_OKS, PP_LOSS_FREEZE_ERROR, PP_LOSS_PROB_LOGITS, PP_LOSS_VIS_LOGITS = 1, 2, 4, 8


def _take(cfg: dict, role: str, want_type: str, defaults: dict) -> dict:
    cfg = dict(cfg)
    t = cfg.pop("type", None)
    t = t if isinstance(t, str) else getattr(t, "__name__", t)
    if t != want_type:
        raise NotImplementedError(f"{role}=dict(type={t!r}) has no MI355X loss kernel; the ProbPose config has type={want_type!r}")
    unknown = sorted(set(cfg) - set(defaults))
    if unknown:
        raise NotImplementedError(f"{role}: {want_type} option(s) {unknown} are not implemented on MI355X (known: {sorted(defaults)})")
    return {**defaults, **cfg}


class OKSHeatmapLoss:
    """heatmap_loss.py:513-681, the ``per_pixel=True`` branch reduced to its mean (probmap_head.py:878-879)."""

    def __init__(self, role: str = "keypoint_loss", **cfg):
        o = _take(dict(cfg, type=cfg.get("type", "OKSHeatmapLoss")), role, "OKSHeatmapLoss",
                  dict(use_target_weight=False, skip_empty_channel=False, smoothing_weight=0.2, gaussian_weight=0.0, loss_weight=1.0,
                       oks_type="minus"))
        if str(o["oks_type"]).lower() != "minus":
            raise NotImplementedError(f"{role}: OKSHeatmapLoss(oks_type={o['oks_type']!r}) is not implemented on MI355X (only 'minus', the "
                                      "ProbPose setting; 'plus' / 'both' are out of scope)")
        if o["skip_empty_channel"]:
            raise NotImplementedError(f"{role}: OKSHeatmapLoss(skip_empty_channel=True) is not implemented on MI355X")
        self.use_target_weight = bool(o["use_target_weight"])  # (the reference's _get_mask applies the weights whatever this says)
        self.smoothing_weight, self.gaussian_weight, self.loss_weight = float(o["smoothing_weight"]), float(o["gaussian_weight"]), float(o["loss_weight"])

    def __call__(self, output: torch.Tensor, target: torch.Tensor, target_weights: torch.Tensor, mask=None) -> Dict[str, torch.Tensor]:
        """``output``, ``target`` (B, K, H, W) and ``target_weights`` (B, K) on the device -> ``loss`` (0-d float32: the mean over all
        pixels times ``loss_weight``), ``map_sums`` (B, K) float64, ``argmax`` (B, K, 2) int32 and ``maxval`` (B, K, 2) float32 (index
        / value of the maximum of the predicted [..., 0] and of the target map [..., 1])."""
        if mask is not None:
            raise NotImplementedError("OKSHeatmapLoss with a spatial `mask` is not implemented on MI355X (ProbMapHead.loss passes none)")
        if not (output.is_cuda and target.is_cuda):
            raise RuntimeError("OKSHeatmapLoss needs tensors on the MI355X; there is no CPU fallback")
        assert output.dim() == 4 and output.shape == target.shape, "output and target should be (B, K, H, W) tensors of one shape"
        B, K, H, W = (int(v) for v in output.shape)
        assert tuple(target_weights.shape) == (B, K), f"target_weights and target have mismatched shapes {tuple(target_weights.shape)} v.s. {tuple(target.shape)}"
        dev = output.device
        p, t = output.detach().float().contiguous(), target.detach().to(dev).float().contiguous()
        w = target_weights.detach().to(device=dev, dtype=torch.float32).contiguous()
        out = dict(loss=torch.empty((1,), dtype=torch.float32, device=dev), map_sums=torch.empty((B, K), dtype=torch.float64, device=dev),
                   argmax=torch.empty((B, K, 2), dtype=torch.int32, device=dev), maxval=torch.empty((B, K, 2), dtype=torch.float32, device=dev))
        with torch.cuda.device(dev):
            _lib.call("pp_probmap_loss_maps", _lib.ptr(p), _lib.ptr(t), _lib.ptr(w), B, K, H, W, self.smoothing_weight, self.gaussian_weight,
                      self.loss_weight, _lib.ptr(out["map_sums"]), _lib.ptr(out["argmax"]), _lib.ptr(out["maxval"]), _lib.ptr(out["loss"]),
                      _lib.stream_ptr(dev))
        out["loss"] = out["loss"][0]
        return out


class _ScalarLoss:
    kind, defaults = "", {}

    def __init__(self, role: str, **cfg):
        o = _take(dict(cfg, type=cfg.get("type", self.kind)), role, self.kind, self.defaults)
        if not o["use_target_weight"]:
            raise NotImplementedError(f"{role}: {self.kind}(use_target_weight=False) is not implemented on MI355X (the ProbPose config weights every scalar loss)")
        if o.get("reduction", "mean") != "mean":
            raise NotImplementedError(f"{role}: {self.kind}(reduction={o['reduction']!r}) is not implemented on MI355X (only 'mean')")
        self.loss_weight = float(o["loss_weight"])
        self.use_sigmoid = bool(o.get("use_sigmoid", False))


class BCELoss(_ScalarLoss):
    """classification_loss.py:12-66. ``use_sigmoid=True`` is ``F.binary_cross_entropy`` on probabilities (the ProbPose setting: the towers
    end in a sigmoid), ``False`` ``binary_cross_entropy_with_logits``."""
    kind, defaults = "BCELoss", dict(use_target_weight=False, loss_weight=1.0, reduction="mean", use_sigmoid=False)


class MSELoss(_ScalarLoss):
    """regression_loss.py:524-553."""
    kind, defaults = "MSELoss", dict(use_target_weight=False, loss_weight=1.0)


class L1LogLoss(_ScalarLoss):
    """regression_loss.py:135-179: smooth L1 (beta 1) of log(1 + .)."""
    kind, defaults = "L1LogLoss", dict(use_target_weight=False, loss_weight=1.0)


def build_head_losses(keypoint_loss, probability_loss, visibility_loss, oks_loss, error_loss) -> Optional[dict]:
    """The five loss modules of ``ProbMapHead`` from its config dictionaries; ``None`` when the head was built without them (all five
    ``None``: an inference-only head, whose ``loss`` says so)."""
    cfgs = dict(keypoint_loss=keypoint_loss, probability_loss=probability_loss, visibility_loss=visibility_loss, oks_loss=oks_loss,
                error_loss=error_loss)
    if all(v is None for v in cfgs.values()):
        return None
    # the reference's defaults (probmap_head.py:104-108) for the ones left out; KeypointMSELoss, the default keypoint loss, has no kernel
    ref = dict(keypoint_loss=dict(type="KeypointMSELoss", use_target_weight=True), probability_loss=dict(type="BCELoss", use_target_weight=True),
               visibility_loss=dict(type="BCELoss", use_target_weight=True), oks_loss=dict(type="MSELoss", use_target_weight=True),
               error_loss=dict(type="L1LogLoss", use_target_weight=True))
    cfgs = {k: dict(v if v is not None else ref[k]) for k, v in cfgs.items()}
    cls = dict(keypoint_loss=OKSHeatmapLoss, probability_loss=BCELoss, visibility_loss=BCELoss, oks_loss=MSELoss, error_loss=L1LogLoss)
    return {k: cls[k](role=k, **cfgs[k]) for k in cfgs}


def probmap_loss_scalars(scalars: torch.Tensor, in_image: torch.Tensor, annotated: torch.Tensor, visibility: torch.Tensor,
                         kp_gt: torch.Tensor, kp_dt: torch.Tensor, losses: dict, freeze_oks: bool, freeze_error: bool) -> Dict[str, torch.Tensor]:
    """One ``pp_probmap_loss_scalars`` launch (include/probpose_mi355x.h): ``scalars`` (4, B, K) float32, the three (B, K) 0 / 1 flag
    tensors, the decoded target / predicted coordinates (B, K, 2) float64 -> ``gt_oks``, ``gt_errs``, ``vis_weights`` (B, K),
    ``oks_weight`` (B,), ``out`` (6,): loss_probability, loss_visibility, loss_oks, loss_error, mae_oks, mae_err."""
    import ctypes

    dev = scalars.device
    _, B, K = (int(v) for v in scalars.shape)
    u8 = lambda t: t.to(device=dev, dtype=torch.uint8).contiguous()  # noqa: E731
    out = dict(gt_oks=torch.empty((B, K), dtype=torch.float32, device=dev), oks_weight=torch.empty((B,), dtype=torch.float32, device=dev),
               gt_errs=torch.empty((B, K), dtype=torch.float32, device=dev), vis_weights=torch.empty((B, K), dtype=torch.float32, device=dev),
               out=torch.empty((6,), dtype=torch.float32, device=dev))
    lw = (ctypes.c_double * 4)(losses["probability_loss"].loss_weight, losses["visibility_loss"].loss_weight, losses["oks_loss"].loss_weight,
                               losses["error_loss"].loss_weight)
    flags = ((PP_LOSS_FREEZE_OKS if freeze_oks else 0) | (PP_LOSS_FREEZE_ERROR if freeze_error else 0)
             | (0 if losses["probability_loss"].use_sigmoid else PP_LOSS_PROB_LOGITS) | (0 if losses["visibility_loss"].use_sigmoid else PP_LOSS_VIS_LOGITS))
    ii, an, vi = u8(in_image), u8(annotated), u8(visibility)
    sc, g, d = scalars.float().contiguous(), kp_gt.double().contiguous(), kp_dt.double().contiguous()
    with torch.cuda.device(dev):
        _lib.call("pp_probmap_loss_scalars", _lib.ptr(sc), _lib.ptr(ii), _lib.ptr(an), _lib.ptr(vi), _lib.ptr(g), _lib.ptr(d), B, K, flags,
                  ctypes.cast(lw, ctypes.c_void_p), _lib.ptr(out["gt_oks"]), _lib.ptr(out["oks_weight"]), _lib.ptr(out["gt_errs"]),
                  _lib.ptr(out["vis_weights"]), _lib.ptr(out["out"]), _lib.stream_ptr(dev))
    return out


# ---- accuracies on the host (probmap_head.py:944-997, evaluation/functional/keypoint_eval.py:10-102, 185-240) -------------------------
def pose_accuracy(argmax: np.ndarray, maxval: np.ndarray, mask: np.ndarray, H: int, W: int, thr: float = 0.05):
    """``pose_pck_accuracy(output, target, mask, method="argmax")[1]`` from the argmax pixels: ``argmax`` (B, K, 2) int = row-major index
    of the maximum of the predicted / the target map, ``maxval`` (B, K, 2) those maxima, ``mask`` (B, K) bool. Locations are (x, y)
    float32, (-1, -1) where the maximum is <= 0 (get_heatmap_maximum); the differences are divided by [H, W] - in that order, as the
    reference's default ``normalize`` -, a keypoint's accuracy is the share of its masked instances closer than ``thr``, the result
    the mean over the keypoints that have one (0.0 when none has)."""
    locs = np.stack([argmax % W, argmax // W], axis=-1).astype(np.float32)  # (B, K, 2 [pred, target], 2 [x, y])
    locs[maxval <= 0.0] = -1
    pred, gt = locs[:, :, 0], locs[:, :, 1]
    N, K = mask.shape
    norm_factor = np.tile(np.array([[H, W]]), (N, 1))
    distances = np.full((N, K), -1, dtype=np.float32)
    m = mask.astype(bool)
    distances[m] = np.linalg.norm(((pred - gt) / norm_factor[:, None, :])[m], axis=-1)
    acc = []
    for d in distances.T:
        valid = d != -1
        acc.append((d[valid] < thr).sum() / valid.sum() if valid.sum() > 0 else -1)
    acc = np.array(acc)
    valid_acc = acc[acc >= 0]
    return valid_acc.mean() if len(valid_acc) > 0 else 0.0


def binary_accuracy(dt: np.ndarray, gt: np.ndarray, mask: np.ndarray, force_balanced: bool = True):
    """``ProbMapHead.get_binary_accuracy`` (probmap_head.py:955-997): the best accuracy over the thresholds 0.1, 0.15 .. 0.95 on a
    class-balanced subsample drawn with two ``np.random.shuffle`` calls (positives first). Returns a float32 (``None`` when one class
    is empty: the reference returns a one-element zero tensor there)."""
    dt, gt = dt[mask], gt[mask].astype(bool)
    if force_balanced:
        pos_num = np.sum(gt)
        num = min(pos_num, len(gt) - pos_num)
        if num == 0:
            return None
        pos_idx, neg_idx = np.where(gt)[0], np.where(~gt)[0]
        np.random.shuffle(pos_idx)
        np.random.shuffle(neg_idx)
        idx = np.concatenate([pos_idx[:num], neg_idx[:num]])
        dt, gt = dt[idx], gt[idx]
    thresholds = np.arange(0.1, 1.0, 0.05)
    counts = ((dt[:, None] > thresholds) == gt[:, None]).sum(axis=0)
    return np.float32(counts[np.argmax(counts)] / len(gt))
