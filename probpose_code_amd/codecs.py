"""``ProbMap`` keypoint codec on MI355X (reference: ``mmpose/codecs/probmap.py:19-220``,
``mmpose/codecs/base.py:9-77``).

Same constructor arguments, same ``decode`` contract (``(K, H, W)`` float32 numpy in,
``(1, K, 2)`` float64 keypoints in input-pixel space and ``(1, K)`` float32 scores out) --
but the arithmetic (OKS-kernel convolution, argmax, sub-pixel step, rescale) runs in the
fused HIP kernel ``pp_probmap_decode`` for a whole batch at once, optionally together with
the flip-test average. ``batch_decode`` is overridden, so ``support_batch_decoding`` is
True and ``BaseHead.decode`` (``mmpose/models/heads/base_head.py:57-62``) takes the batched
branch instead of the per-sample Python loop.
"""
from abc import ABCMeta, abstractmethod
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .registry import KEYPOINT_CODECS, register

# COCO keypoint sigmas (x100) that the reference hard-wires into its OKS kernels
# (mmpose/codecs/utils/post_processing.py:16); the decode is therefore limited to K <= 17.
_KPT_SIGMAS = np.array([2.6, 2.5, 2.5, 3.5, 3.5, 7.9, 7.9, 7.2, 7.2, 6.2, 6.2, 10.7, 10.7, 8.7, 8.7, 8.9, 8.9]) / 100


def oks_kernel_taps(K: int, H: int, W: int) -> Tuple[np.ndarray, np.ndarray]:
    """Separable factors of the reference's OKS kernels (post_processing.py:13-39).

    The reference builds, per keypoint, ``exp(-d^2 / 2s) / sum`` on a (2r+1)^2 grid with
    ``s = clip((2 sigma_k)^2 * sqrt(H/1.25 * W/1.25) * 2, 0.55, 3.0)`` and ``r = ceil(3 s)``.
    That kernel is the outer product of ``g / sum(g)``, ``g[t] = exp(-t^2 / 2s)``, with
    itself; the HIP kernel convolves rows then columns with this vector in float64, which
    rounds to the same float32 map (tests/test_decode_parity.py checks the maps bit for bit).

    Returns ``taps`` (K, PP_MAX_TAPS) float64 (row k: 2 r_k + 1 factors, zero padded) and
    ``radius`` (K,) int32.
    """
    if K > len(_KPT_SIGMAS):
        raise IndexError(f"ProbMap decode is defined for at most {len(_KPT_SIGMAS)} (COCO) keypoints, got {K}")
    area = np.sqrt(H / 1.25 * W / 1.25)
    taps = np.zeros((K, _lib.PP_MAX_TAPS), np.float64)
    radius = np.zeros((K,), np.int32)
    for k in range(K):
        s = float(np.clip((_KPT_SIGMAS[k] * 2) ** 2 * area * 2, 0.55, 3.0))
        r = int(np.ceil(s * 3))
        t = np.arange(-r, r + 1, dtype=np.float64)
        g = np.exp(-(t**2) / (2 * s))
        taps[k, : 2 * r + 1] = g / g.sum()
        radius[k] = r
    return taps, radius


class BaseKeypointCodec(metaclass=ABCMeta):
    """base.py:9-77."""

    auxiliary_encode_keys = set()
    field_mapping_table: Dict[str, str] = dict()
    instance_mapping_table: Dict[str, str] = dict()
    label_mapping_table: Dict[str, str] = dict()

    @abstractmethod
    def encode(self, keypoints: np.ndarray, keypoints_visible: Optional[np.ndarray] = None) -> dict:
        """Encode keypoints."""

    @abstractmethod
    def decode(self, encoded: Any) -> Tuple[np.ndarray, np.ndarray]:
        """Decode keypoints."""

    def batch_decode(self, batch_encoded: Any) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        raise NotImplementedError()

    @property
    def support_batch_decoding(self) -> bool:
        return getattr(type(self), "batch_decode") is not BaseKeypointCodec.batch_decode


@register(KEYPOINT_CODECS, reference_name="ProbMap", mi355x_name="ProbMapMI355X")
class ProbMap(BaseKeypointCodec):
    """Expected-OKS probability-map codec; decode on the GPU.

    Args are those of the reference (probmap.py:71-96): ``input_size`` [w, h],
    ``heatmap_size`` [W, H], ``heatmap_type`` in {"gaussian", "combined"} (only
    "gaussian" -- the one ProbPose uses -- is decodable here), ``sigma``,
    ``radius_factor``, ``blur_kernel_size``, ``increase_sigma_with_padding``.
    """

    label_mapping_table = dict(keypoint_weights="keypoint_weights")
    field_mapping_table = dict(heatmaps="heatmaps")
    decode_kind = "expmax"  # which decode the engine runs behind the head: expected-OKS maximisation ("expmax") or UDP argmax + DARK ("dark")

    def __init__(
        self,
        input_size: Tuple[int, int],
        heatmap_size: Tuple[int, int],
        heatmap_type: str = "gaussian",
        sigma: float = 2.0,
        radius_factor: float = 0.0546875,
        blur_kernel_size: int = 11,
        increase_sigma_with_padding=False,
    ) -> None:
        super().__init__()
        self.input_size = input_size
        self.heatmap_size = heatmap_size
        self.radius_factor = radius_factor
        self.heatmap_type = heatmap_type
        self.blur_kernel_size = blur_kernel_size
        self.scale_factor = ((np.array(input_size) - 1) / (np.array(heatmap_size) - 1)).astype(np.float32)
        self.increase_sigma_with_padding = increase_sigma_with_padding
        self.sigma = sigma
        if self.heatmap_type not in {"gaussian", "combined"}:
            raise ValueError(
                f"{self.__class__.__name__} got invalid `heatmap_type` value"
                f"{self.heatmap_type}. Should be one of "
                '{"gaussian", "combined"}'
            )
        self._tables: Dict[Tuple[int, int, int, str], Tuple[torch.Tensor, torch.Tensor]] = {}

    # -- encode: the label generator of GenerateTarget; what the loss mode (ProbMapHead.loss) scores the head's outputs against
    def _check_encodable(self, K: int) -> None:
        if self.heatmap_type != "gaussian":
            raise NotImplementedError("only heatmap_type='gaussian' (the ProbPose setting) is encodable on MI355X")
        if not (self.sigma is not None and self.sigma > 0) and K != len(_KPT_SIGMAS):
            raise ValueError(f"{type(self).__name__}.encode with sigma <= 0 uses the {len(_KPT_SIGMAS)} COCO keypoint sigmas "
                             f"(oks_map.py:39): got {K} keypoints")

    def encode(self, keypoints: np.ndarray, keypoints_visible: Optional[np.ndarray] = None, id_similarity: Optional[float] = 0.0,
               keypoints_visibility: Optional[np.ndarray] = None) -> dict:
        """probmap.py:98-168 for ONE instance, on the host in numpy: ``keypoints`` (1, K, 2) in input-pixel space, ``keypoints_visible``
        (1, K) -> the reference's dictionary: ``heatmaps`` (K, H, W) float32 - per labelled keypoint ``exp(-d^2 / 2s)`` in float64 around
        ``keypoints / scale_factor``, ``s = clip((2 sigma_k)^2 sqrt(H / 1.25 * W / 1.25) 2, 0.55, 3.0)`` or a positive ``sigma`` -,
        ``keypoint_weights`` (1, K) (``keypoints_visible`` with the labelled entries replaced by "the float64 map has a value above
        zero": 0 for a keypoint far outside), ``annotated``, ``in_image`` (1, K) bool, ``keypoints_scaled``, ``heatmap_keypoints``,
        ``identification_similarity``. The batched form on the device is ``encode_device``; this one is its restatement."""
        assert keypoints.shape[0] == 1, f"{self.__class__.__name__} only support single-instance keypoint encoding"
        N, K, _ = keypoints.shape
        self._check_encodable(K)
        if keypoints_visibility is None:
            keypoints_visibility = np.zeros(keypoints.shape[:2], dtype=np.float32)
        if keypoints_visible is None:
            keypoints_visible = np.ones(keypoints.shape[:2], dtype=np.float32)
        W, H = self.heatmap_size
        scaled = keypoints / self.scale_factor
        heatmaps = np.zeros((K, H, W), dtype=np.float32)
        keypoint_weights = keypoints_visible.copy()
        bbox_area = np.sqrt(H / 1.25 * W / 1.25)
        y_idx, x_idx = np.indices((H, W))
        for k in range(K):
            if keypoints_visible[0, k] < 0.5:  # unlabelled: the zero map, the weight as it came
                continue
            dx = x_idx - scaled[0, k, 0]
            dy = y_idx - scaled[0, k, 1]
            dist = np.sqrt(dx**2 + dy**2)
            s = np.clip((_KPT_SIGMAS[k] * 2) ** 2 * bbox_area * 2, 0.55, 3.0) if not (self.sigma is not None and self.sigma > 0) else self.sigma
            oks_map = np.exp(-(dist**2 / (2 * s)))
            keypoint_weights[0, k] = int(oks_map.max() > 0)
            heatmaps[k] = oks_map
        in_image = (keypoints[:, :, 0] >= 0) & (keypoints[:, :, 0] < self.input_size[0]) & (keypoints[:, :, 1] >= 0) & (
            keypoints[:, :, 1] < self.input_size[1])
        return dict(heatmaps=heatmaps, keypoint_weights=keypoint_weights, annotated=keypoints_visible > 0, in_image=in_image,
                    keypoints_scaled=keypoints, heatmap_keypoints=keypoints / self.scale_factor,
                    identification_similarity=id_similarity)

    def encode_device(self, keypoints: torch.Tensor, keypoints_visible: torch.Tensor) -> Dict[str, torch.Tensor]:
        """``encode`` for a batch in ONE launch (``pp_probmap_encode``): ``keypoints`` (B, K, 2) in input-pixel space and
        ``keypoints_visible`` (B, K) on the device (converted to float32: the division by ``scale_factor`` is float32, as for the float32
        keypoints of the data pipeline) -> device tensors ``heatmaps`` (B, K, H, W) float32, ``keypoint_weights`` (B, K) float32,
        ``annotated`` and ``in_image`` (B, K) bool. The maps are never built on the host."""
        if not (isinstance(keypoints, torch.Tensor) and keypoints.is_cuda):
            raise RuntimeError(f"{type(self).__name__}.encode_device needs tensors on the MI355X; there is no CPU fallback "
                               "(the host form is `encode`)")
        assert keypoints.dim() == 3 and keypoints.shape[-1] == 2, "keypoints should be a (B, K, 2) tensor"
        B, K = int(keypoints.shape[0]), int(keypoints.shape[1])
        assert tuple(keypoints_visible.shape) == (B, K), "keypoints_visible should be a (B, K) tensor"
        self._check_encodable(K)
        dev = keypoints.device
        W, H = self.heatmap_size
        kp = keypoints.to(torch.float32).contiguous()
        vis = keypoints_visible.to(device=dev, dtype=torch.float32).contiguous()
        out = dict(heatmaps=torch.empty((B, K, H, W), dtype=torch.float32, device=dev),
                   keypoint_weights=torch.empty((B, K), dtype=torch.float32, device=dev),
                   annotated=torch.empty((B, K), dtype=torch.uint8, device=dev),
                   in_image=torch.empty((B, K), dtype=torch.uint8, device=dev))
        with torch.cuda.device(dev):
            _lib.call("pp_probmap_encode", _lib.ptr(kp), _lib.ptr(vis), B, K, H, W, float(self.input_size[0]), float(self.input_size[1]),
                      float(self.sigma if self.sigma is not None else -1.0), _lib.ptr(out["heatmaps"]), _lib.ptr(out["keypoint_weights"]),
                      _lib.ptr(out["annotated"]), _lib.ptr(out["in_image"]), _lib.stream_ptr(dev))
        out["annotated"], out["in_image"] = out["annotated"].bool(), out["in_image"].bool()
        return out

    # -- device-side tables, built once per (K, H, W, device) instead of on every call (post_processing.py:344)
    def _device_tables(self, K: int, H: int, W: int, device: torch.device):
        key = (K, H, W, str(device))
        if key not in self._tables:
            taps, radius = oks_kernel_taps(K, H, W)
            self._tables[key] = (torch.from_numpy(taps).to(device), torch.from_numpy(radius).to(device))
        return self._tables[key]

    def decode_device(
        self,
        heatmaps: torch.Tensor,
        heatmaps_flip: Optional[torch.Tensor] = None,
        flip_indices: Optional[Sequence[int]] = None,
        return_avg: bool = False,
        return_conv: bool = False,
        shift_heatmap: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """Batched decode on device tensors; nothing is copied to the host.

        heatmaps (B, K, H, W) float32 on a CUDA/HIP device; ``heatmaps_flip`` (same shape)
        is the output of the horizontally flipped pass -- it is flipped back, channel-permuted
        by ``flip_indices`` and averaged inside the kernel (probmap_head.py:757-763); ``shift_heatmap``: the flipped-back
        map is moved one pixel to the right first (``flip_heatmaps(..., shift_heatmap=True)``, models/utils/tta.py:64-66).
        Returns device tensors: ``keypoints`` (B, K, 2) f64 input-pixel space, ``scores``
        (B, K) f32, ``locs`` (B, K, 2) f32 heatmap space and optionally ``heatmaps`` (the
        averaged maps) / ``conv`` (the OKS-convolved maps).
        """
        assert isinstance(heatmaps, torch.Tensor) and heatmaps.dim() == 4, "heatmaps should be a (B, K, H, W) tensor"
        if self.heatmap_type != "gaussian":
            raise NotImplementedError("only heatmap_type='gaussian' (the ProbPose setting) is decodable on MI355X")
        if not heatmaps.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.decode_device needs tensors on the MI355X; there is no CPU fallback")
        B, K, H, W = heatmaps.shape
        Wc, Hc = self.heatmap_size
        assert (H, W) == (Hc, Wc), f"heatmap shape {(H, W)} does not match codec heatmap_size {(Hc, Wc)}"
        dev = heatmaps.device
        hm = heatmaps.contiguous().float()
        hmf = fi = None
        if heatmaps_flip is not None:
            assert heatmaps_flip.shape == heatmaps.shape
            assert flip_indices is not None and len(flip_indices) == K
            hmf = heatmaps_flip.contiguous().float()
            fi = self._flip_tensor(tuple(int(i) for i in flip_indices), dev)
        taps, radius = self._device_tables(K, H, W, dev)
        out = dict(
            locs=torch.empty((B, K, 2), dtype=torch.float32, device=dev),
            keypoints=torch.empty((B, K, 2), dtype=torch.float64, device=dev),
            scores=torch.empty((B, K), dtype=torch.float32, device=dev),
        )
        avg = torch.empty_like(hm) if return_avg else None
        conv = torch.empty_like(hm) if return_conv else None
        with torch.cuda.device(dev):
            self._launch(hm, hmf, fi, taps, radius, avg, conv, out, shift_heatmap, dev)
        if return_avg:
            out["heatmaps"] = avg
        if return_conv:
            out["conv"] = conv
        return out

    def _launch(self, hm, hmf, fi, taps, radius, avg, conv, out, shift_heatmap, dev) -> None:
        B, K, H, W = hm.shape
        _lib.call(
            "pp_probmap_decode_flags", _lib.ptr(hm), _lib.ptr(hmf), _lib.ptr(fi), _lib.ptr(taps), _lib.ptr(radius),
            B, K, H, W, float(self.input_size[0]), float(self.input_size[1]), 1.0, 1.0,
            _lib.ptr(avg), _lib.ptr(conv), _lib.ptr(out["locs"]), _lib.ptr(out["keypoints"]),
            _lib.ptr(out["scores"]), 4 if shift_heatmap else 0, _lib.stream_ptr(dev),
        )  # fmt: skip  (flags: PP_DECODE_SHIFT_HEATMAP = 4)

    def _flip_tensor(self, flip_indices: Tuple[int, ...], device) -> torch.Tensor:
        key = ("flip", flip_indices, str(device))
        if key not in self._tables:
            self._tables[key] = torch.tensor(flip_indices, dtype=torch.int32, device=device)
        return self._tables[key]

    def batch_decode(self, batch_heatmaps: torch.Tensor) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """(B, K, H, W) device tensor -> per-sample lists, each element shaped as ``decode`` returns."""
        out = self.decode_device(batch_heatmaps)
        kpts = out["keypoints"].cpu().numpy()
        scores = out["scores"].cpu().numpy()
        return [kpts[i][None] for i in range(kpts.shape[0])], [scores[i][None] for i in range(scores.shape[0])]

    def decode(self, encoded: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """probmap.py:170-220 for one sample: (K, H, W) numpy -> ((1, K, 2) f64, (1, K) f32)."""
        if self.heatmap_type != "gaussian":
            raise NotImplementedError("only heatmap_type='gaussian' (the ProbPose setting) is decodable on MI355X")
        assert isinstance(encoded, np.ndarray), "heatmaps should be numpy.ndarray"
        assert encoded.ndim == 3, f"Invalid shape {encoded.shape}"
        hm = torch.from_numpy(np.ascontiguousarray(encoded, dtype=np.float32)).cuda()[None]
        kpts, scores = self.batch_decode(hm)
        return kpts[0], scores[0]


@register(KEYPOINT_CODECS, reference_name="UDPHeatmap", mi355x_name="UDPHeatmapMI355X")
class UDPHeatmap(BaseKeypointCodec):
    """Unbiased-data-processing heatmap codec with DARK refinement (reference: ``mmpose/codecs/udp_heatmap.py:14-196``), the codec
    of the ViTPose baseline; decode on the GPU (``pp_udp_heatmap_decode``: maximum of the map, Gaussian modulation, one Newton
    step on the log map, rescale - for a whole batch in one launch, optionally together with the flip-test average).

    Args are the reference's (udp_heatmap.py:68-88): ``input_size`` [w, h], ``heatmap_size`` [W, H], ``heatmap_type``
    ("gaussian" only: "combined" belongs to heads with offset maps), ``sigma``, ``radius_factor``, ``blur_kernel_size``
    (odd, at most 19; 11 for sigma 2, 17 for sigma 3)."""

    label_mapping_table = dict(keypoint_weights="keypoint_weights")
    field_mapping_table = dict(heatmaps="heatmaps")
    decode_kind = "dark"

    def __init__(self, input_size: Tuple[int, int], heatmap_size: Tuple[int, int], heatmap_type: str = "gaussian",
                 sigma: float = 2.0, radius_factor: float = 0.0546875, blur_kernel_size: int = 11) -> None:
        super().__init__()
        self.input_size = input_size
        self.heatmap_size = heatmap_size
        self.sigma = sigma
        self.radius_factor = radius_factor
        self.heatmap_type = heatmap_type
        self.blur_kernel_size = blur_kernel_size
        self.scale_factor = ((np.array(input_size) - 1) / (np.array(heatmap_size) - 1)).astype(np.float32)
        if self.heatmap_type not in {"gaussian", "combined"}:
            raise ValueError(
                f"{self.__class__.__name__} got invalid `heatmap_type` value"
                f"{self.heatmap_type}. Should be one of "
                '{"gaussian", "combined"}'
            )
        if self.heatmap_type == "combined":
            raise NotImplementedError("UDPHeatmap(heatmap_type='combined') (udp_heatmap.py:170-190: classification + offset maps) has no "
                                      "MI355X kernel; the ViTPose configs use 'gaussian'")
        if int(blur_kernel_size) % 2 != 1 or not 1 <= int(blur_kernel_size) <= _lib.PP_MAX_TAPS:
            raise ValueError(f"blur_kernel_size must be odd and at most {_lib.PP_MAX_TAPS} (pp_udp_heatmap_decode), got {blur_kernel_size}")
        self._tables: Dict[tuple, torch.Tensor] = {}

    def encode(self, keypoints, keypoints_visible=None) -> dict:
        raise NotImplementedError(
            "UDPHeatmap.encode (udp_heatmap.py:90-144) generates training targets and is outside the "
            "MI355X inference hot path (SURVEY.md 2: 'decode only; encode is training')."
        )

    def decode_device(self, heatmaps: torch.Tensor, heatmaps_flip: Optional[torch.Tensor] = None,
                      flip_indices: Optional[Sequence[int]] = None, return_avg: bool = False,
                      shift_heatmap: bool = False) -> Dict[str, torch.Tensor]:
        """Batched decode on device tensors; nothing is copied to the host. Arguments and results as ``ProbMap.decode_device``:
        ``keypoints`` (B, K, 2) f64 input-pixel space, ``scores`` (B, K) f32 (the maximum of the - averaged - map), ``locs``
        (B, K, 2) f32 (that maximum's pixel; (-1, -1) where it is <= 0), optionally ``heatmaps`` (the averaged maps). A map with a
        non-finite value gives NaN results."""
        assert isinstance(heatmaps, torch.Tensor) and heatmaps.dim() == 4, "heatmaps should be a (B, K, H, W) tensor"
        if not heatmaps.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.decode_device needs tensors on the MI355X; there is no CPU fallback")
        B, K, H, W = heatmaps.shape
        Wc, Hc = self.heatmap_size
        assert (H, W) == (Hc, Wc), f"heatmap shape {(H, W)} does not match codec heatmap_size {(Hc, Wc)}"
        dev = heatmaps.device
        hm = heatmaps.contiguous().float()
        hmf = fi = None
        if heatmaps_flip is not None:
            assert heatmaps_flip.shape == heatmaps.shape
            assert flip_indices is not None and len(flip_indices) == K
            hmf = heatmaps_flip.contiguous().float()
            key = (tuple(int(i) for i in flip_indices), str(dev))
            if key not in self._tables:
                self._tables[key] = torch.tensor(key[0], dtype=torch.int32, device=dev)
            fi = self._tables[key]
        out = dict(
            locs=torch.empty((B, K, 2), dtype=torch.float32, device=dev),
            keypoints=torch.empty((B, K, 2), dtype=torch.float64, device=dev),
            scores=torch.empty((B, K), dtype=torch.float32, device=dev),
        )
        avg = torch.empty_like(hm) if return_avg else None
        with torch.cuda.device(dev):
            _lib.call(
                "pp_udp_heatmap_decode", _lib.ptr(hm), _lib.ptr(hmf), _lib.ptr(fi), B, K, H, W, float(self.input_size[0]),
                float(self.input_size[1]), int(self.blur_kernel_size), _lib.ptr(avg), _lib.ptr(out["locs"]),
                _lib.ptr(out["keypoints"]), _lib.ptr(out["scores"]), 4 if (shift_heatmap and hmf is not None) else 0,
                _lib.stream_ptr(dev),
            )  # fmt: skip  (flags: PP_DECODE_SHIFT_HEATMAP = 4)
        if return_avg:
            out["heatmaps"] = avg
        return out

    def batch_decode(self, batch_heatmaps: torch.Tensor) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """(B, K, H, W) device tensor -> per-sample lists, each element shaped as ``decode`` returns."""
        out = self.decode_device(batch_heatmaps)
        kpts = out["keypoints"].cpu().numpy()
        scores = out["scores"].cpu().numpy()
        if not (np.isfinite(kpts).all() and np.isfinite(scores).all()):
            raise FloatingPointError(f"{type(self).__name__}.decode: non-finite keypoints / scores (a heatmap holds a non-finite value)")
        return [kpts[i][None] for i in range(kpts.shape[0])], [scores[i][None] for i in range(scores.shape[0])]

    def decode(self, encoded: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """udp_heatmap.py:146-196 for one sample: (K, H, W) numpy -> ((1, K, 2) f64, (1, K) f32)."""
        assert isinstance(encoded, np.ndarray), "heatmaps should be numpy.ndarray"
        assert encoded.ndim == 3, f"Invalid shape {encoded.shape}"
        hm = torch.from_numpy(np.ascontiguousarray(encoded, dtype=np.float32)).cuda()[None]
        kpts, scores = self.batch_decode(hm)
        return kpts[0], scores[0]


@register(KEYPOINT_CODECS, reference_name="UDPExpMaxHeatmap", mi355x_name="UDPExpMaxHeatmapMI355X")
class UDPExpMaxHeatmap(ProbMap):
    """Gaussian heatmaps decoded by expected-OKS maximisation (reference: ``mmpose/codecs/udp_expmax_heatmap.py:16-254``): the
    ViTPose heads with the ProbPose decoder. Decode on the GPU, ``pp_expmax_heatmap_decode``: ``ProbMap``'s arithmetic on the RAW maps
    (values below 0 and above 1 pass through), for a whole batch in one launch, optionally together with the flip-test average.

    Args are the reference's (udp_expmax_heatmap.py:79-101): ``input_size`` [w, h], ``heatmap_size`` [W, H], ``heatmap_type``
    ("gaussian" only), ``sigma``, ``radius_factor``, ``blur_kernel_size``, ``increase_sigma_with_padding``, ``normalize`` and
    ``parzen_size`` - the last two are stored; the reference's decode does not use them either (``normalize`` acts in ``encode``,
    ``parzen_size`` is an argument ``get_heatmap_expected_value`` ignores)."""

    decode_kind = "expmax"

    def __init__(self, input_size: Tuple[int, int], heatmap_size: Tuple[int, int], heatmap_type: str = "gaussian",
                 sigma: float = 2.0, radius_factor: float = 0.0546875, blur_kernel_size: int = 11,
                 increase_sigma_with_padding=False, normalize=False, parzen_size=0.1) -> None:
        super().__init__(input_size, heatmap_size, heatmap_type=heatmap_type, sigma=sigma, radius_factor=radius_factor,
                         blur_kernel_size=blur_kernel_size, increase_sigma_with_padding=increase_sigma_with_padding)
        self.normalize = normalize
        self.parzen_size = parzen_size
        if self.heatmap_type == "combined":
            raise NotImplementedError("UDPExpMaxHeatmap(heatmap_type='combined') (udp_expmax_heatmap.py:228-249: classification + offset "
                                      "maps, argmax decode) has no MI355X kernel; the expected-OKS decode is the 'gaussian' branch")

    def encode(self, keypoints, keypoints_visible=None, id_similarity=0.0, keypoints_visibility=None) -> dict:
        raise NotImplementedError(
            "UDPExpMaxHeatmap.encode (udp_expmax_heatmap.py:110-200) generates the Gaussian training targets of the ViTPose heads and is "
            "not implemented on MI355X; the target generator that is, is ProbMap.encode / ProbMap.encode_device (the loss mode)."
        )

    def encode_device(self, keypoints, keypoints_visible):
        raise NotImplementedError("UDPExpMaxHeatmap.encode_device: this codec's training targets are Gaussians, not OKS maps; "
                                  "ProbMap.encode_device is the target generator that runs")

    def _launch(self, hm, hmf, fi, taps, radius, avg, conv, out, shift_heatmap, dev) -> None:
        B, K, H, W = hm.shape
        _lib.call(
            "pp_expmax_heatmap_decode", _lib.ptr(hm), _lib.ptr(hmf), _lib.ptr(fi), _lib.ptr(taps), _lib.ptr(radius), B, K, H, W,
            float(self.input_size[0]), float(self.input_size[1]), _lib.ptr(avg), _lib.ptr(conv), _lib.ptr(out["locs"]),
            _lib.ptr(out["keypoints"]), _lib.ptr(out["scores"]), 4 if (shift_heatmap and hmf is not None) else 0, _lib.stream_ptr(dev),
        )  # fmt: skip  (flags: PP_DECODE_SHIFT_HEATMAP = 4)

    def batch_decode(self, batch_heatmaps: torch.Tensor) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """(B, K, H, W) device tensor -> per-sample lists, each element shaped as ``decode`` returns."""
        out = self.decode_device(batch_heatmaps)
        kpts = out["keypoints"].cpu().numpy()
        scores = out["scores"].cpu().numpy()
        if not (np.isfinite(kpts).all() and np.isfinite(scores).all()):
            raise FloatingPointError("UDPExpMaxHeatmap.decode: non-finite keypoints / scores (a heatmap holds a non-finite value)")
        return [kpts[i][None] for i in range(kpts.shape[0])], [scores[i][None] for i in range(scores.shape[0])]


@register(KEYPOINT_CODECS, reference_name="ArgMaxProbMap", mi355x_name="ArgMaxProbMapMI355X")
class ArgMaxProbMap(UDPHeatmap):
    """Probability maps decoded by UDP argmax + DARK (reference: ``mmpose/codecs/argmax_probmap.py:18-260``): the ProbPose head with
    the ViTPose decoder, the argmax column of the paper's decoding ablation. ``decode`` / ``decode_device`` take MAPS, as the
    reference's decode does, and run ``pp_udp_heatmap_decode`` on them - the same steps as ``UDPHeatmap.decode``. Behind a
    ``ProbMapHead`` the engine starts from the logits instead and runs Sparsemax, the flip-test average and this decode in one launch
    (``pp_argmax_probmap_decode``).

    Args are the reference's (argmax_probmap.py:74-92): ``input_size`` [w, h], ``heatmap_size`` [W, H], ``heatmap_type`` ("gaussian"
    only), ``sigma`` (-1), ``radius_factor``, ``blur_kernel_size`` (odd, at most 19), ``increase_sigma_with_padding``."""

    decode_kind = "dark"

    def __init__(self, input_size: Tuple[int, int], heatmap_size: Tuple[int, int], heatmap_type: str = "gaussian",
                 sigma: float = -1, radius_factor: float = 0.0546875, blur_kernel_size: int = 11,
                 increase_sigma_with_padding=False) -> None:
        if heatmap_type == "combined":
            raise NotImplementedError("ArgMaxProbMap(heatmap_type='combined') (argmax_probmap.py: classification + offset maps) has no "
                                      "MI355X kernel; ProbPose's maps are 'gaussian'")
        super().__init__(input_size, heatmap_size, heatmap_type=heatmap_type, sigma=sigma, radius_factor=radius_factor,
                         blur_kernel_size=blur_kernel_size)
        self.increase_sigma_with_padding = increase_sigma_with_padding

    def encode(self, keypoints, keypoints_visible=None, id_similarity=0.0, keypoints_visibility=None) -> dict:
        raise NotImplementedError(
            "ArgMaxProbMap.encode (argmax_probmap.py:101-170) generates training targets and is not implemented on MI355X: "
            "it is a decoder here; the target generator that runs is ProbMap.encode / ProbMap.encode_device (the loss mode)."
        )
