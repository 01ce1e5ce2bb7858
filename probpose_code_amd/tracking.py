"""Follow persons through a video: the boxes of frame t + 1 from the poses of frame t, on the device.

Every other entry point takes person boxes from outside (the reference's video demo gets them from an mmdet detector per frame). ProbPose
predicts a presence probability per keypoint and localises keypoints outside the crop it was given, so a box built from frame t's confident
keypoints is a sound crop for frame t + 1 - and it can grow as a person walks into view. Only the first frame needs boxes.

The rule (``next_boxes_host`` states it in numpy and is the test oracle; ``csrc/pp_track_core.h`` is the form the device runs):

* keypoints go to image space with the expression of ``TopdownPoseEstimator.add_pred_to_datasample``;
* the gate of a keypoint is its presence probability (``prob``) for a head with towers, its confidence (``conf``) for a ``HeatmapHead``;
  a keypoint is selected when the gate is finite and ``>= kpt_thr`` and its coordinates are finite;
* with at least ``min_keypoints`` selected the new box is their min/max box grown about its centre by ``expand``, each side at least
  ``min_side`` pixels, blended with the old box by ``smooth`` (``smooth * old + (1 - smooth) * new``; 0: exactly the new box), rounded to
  float32, and ``lost`` returns to 0; otherwise the box is kept and ``lost`` grows by one - beyond ``max_lost`` the track dies and stays dead;
* two tracks updated in one frame whose image-space poses have an OKS (``mmpose/evaluation/functional/nms.py::oks_iou``: the dataset sigmas, the
  mean area of the two new boxes) above ``dup_oks_thr`` are duplicates: the one with the lower mean gate over its selected keypoints dies, the
  higher index on a tie; the pairs are visited in the order (0, 1), (0, 2), ..., (1, 2), ... and a dead track takes no further part;
* a dead or free slot keeps its last box: the batch shape never changes, every frame replays one captured graph.

The defaults below are parameters, NOT VALIDATED ON REAL FOOTAGE: no published checkpoint and no real video were at hand when they were
chosen; they come from the reference's drawing threshold (0.3), its box padding (1.25) and its OKS-NMS threshold (0.9).

Not here: a detector, re-identification, smoothing of keypoints in time, rotation, pipelines without ``use_udp=True``, more than 64 tracks,
several GPUs.
"""
from collections import deque
from typing import Dict, List, Optional, Tuple

import numpy as np

TRACK_DEFAULTS = dict(kpt_thr=0.3, min_keypoints=4, expand=1.25, min_side=8.0, smooth=0.0, max_lost=10, dup_oks_thr=0.9)
MAX_TRACKS = 64        # PP_TRACK_MAX_TRACKS
MAX_KEYPOINTS = 256    # PP_TRACK_MAX_KEYPOINTS
GATE_PROB, GATE_CONF = 0, 1  # PP_TRACK_GATE_*
_COL = {"prob": 3, "conf": 2}  # columns of the record (dist.RECORD_FIELDS)


def track_params(**params) -> dict:
    """``TRACK_DEFAULTS`` with ``params`` over them, checked (the conditions of ``pp_track_update``)."""
    unknown = sorted(set(params) - set(TRACK_DEFAULTS))
    if unknown:
        raise TypeError(f"unknown tracking parameter(s) {unknown}; known: {sorted(TRACK_DEFAULTS)}")
    p = dict(TRACK_DEFAULTS, **params)
    p["min_keypoints"], p["max_lost"] = int(p["min_keypoints"]), int(p["max_lost"])
    for k in ("kpt_thr", "expand", "min_side", "smooth", "dup_oks_thr"):
        p[k] = float(p[k])
    if np.isnan(p["kpt_thr"]) or np.isnan(p["dup_oks_thr"]):
        raise ValueError("kpt_thr and dup_oks_thr must not be NaN")
    if p["min_keypoints"] < 1 or p["max_lost"] < 0:
        raise ValueError("min_keypoints is at least 1, max_lost at least 0")
    if not (0 < p["expand"] < np.inf and 0 < p["min_side"] < np.inf and 0 <= p["smooth"] < 1):
        raise ValueError("expand and min_side are positive and finite, smooth is in [0, 1)")
    return p


def _tree_sum(v: np.ndarray) -> np.ndarray:
    """Sum over the last axis through the tree of adjacent pairs, the axis padded with zeros to a power of two (the order the kernel adds in)."""
    v = np.asarray(v, np.float64)
    p = 1
    while p < v.shape[-1]:
        p *= 2
    v = np.concatenate([v, np.zeros(v.shape[:-1] + (p - v.shape[-1],))], axis=-1)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def image_space_keypoints(records: np.ndarray, centers: np.ndarray, scales: np.ndarray, input_size: Tuple[int, int]) -> np.ndarray:
    """(n, K, 2) float64: topdown.py:165-167 for a batch - the keypoints of the records, cut with ``centers`` / ``scales`` (n, 2) float32."""
    rec = np.asarray(records, np.float64)
    cen, sca = np.asarray(centers, np.float32)[:, None, :], np.asarray(scales, np.float32)[:, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        return rec[..., :2] / np.asarray(input_size) * sca + cen - 0.5 * sca


def pose_oks(kp_i: np.ndarray, kp_j: np.ndarray, area_i: float, area_j: float, sigmas: np.ndarray) -> float:
    """``oks_iou`` (nms.py:58-116) of two (K, 2) poses in float64, the sum over K through ``_tree_sum``."""
    var = (np.asarray(sigmas, np.float64) * 2) ** 2
    with np.errstate(invalid="ignore", over="ignore"):  # (a non-finite coordinate makes the OKS NaN, which is above no threshold)
        d = kp_j - kp_i
        e = (d[:, 0] ** 2 + d[:, 1] ** 2) / var / ((area_i + area_j) / 2 + np.spacing(1)) / 2
        return float(_tree_sum(np.exp(-e)) / len(e))


def next_boxes_host(records, centers, scales, input_size, boxes, alive, lost, sigmas, gate: str = "prob", return_oks: bool = False,
                    image_keypoints=None, **params):
    """The rule of the module's docstring for one frame. ``records`` (n, K, 7) float64 in crop space as ``pp_pack_records`` leaves them,
    ``centers`` / ``scales`` (n, 2) float32 the crops were cut with, ``input_size`` (w, h), the track state ``boxes`` (n, 4) float32 xyxy,
    ``alive`` and ``lost`` (n) int32, ``sigmas`` (K). Returns ``(boxes, alive, lost)`` of the next frame (new arrays); with ``return_oks`` also
    the list of ``(i, j, oks)`` of every pair of updated tracks (how far a duplicate decision is from its threshold). ``image_keypoints``
    (n, K, 2): keypoints already in image space - those of ``inference_topdown``'s samples - instead of the records' mapped ones (a host loop
    over ``inference_topdown`` holds these; ``centers`` / ``scales`` are then not read and the records need their gate column only)."""
    p = track_params(**params)
    rec = np.asarray(records, np.float64)
    n, K = rec.shape[:2]
    boxes = np.array(boxes, np.float32).reshape(n, 4)
    alive, lost = np.array(alive, np.int32).reshape(n), np.array(lost, np.int32).reshape(n)
    kp = image_space_keypoints(rec, centers, scales, input_size) if image_keypoints is None else np.asarray(image_keypoints, np.float64).reshape(n, K, 2)
    g = rec[..., _COL[gate]]
    with np.errstate(invalid="ignore"):
        sel = np.isfinite(g) & (g >= p["kpt_thr"]) & np.isfinite(kp).all(-1)
    updated, mean_gate, area = np.zeros(n, bool), np.zeros(n), np.zeros(n)
    for i in range(n):
        if not alive[i]:
            continue
        count = int(sel[i].sum())
        if count < p["min_keypoints"]:
            lost[i] += 1
            if lost[i] > p["max_lost"]:
                alive[i] = 0
            continue
        pts = kp[i][sel[i]]
        lo, hi = pts.min(0), pts.max(0)
        c = (lo + hi) * 0.5
        side = np.maximum((hi - lo) * p["expand"], p["min_side"])
        new = np.concatenate([c - 0.5 * side, c + 0.5 * side])
        if p["smooth"] != 0.0:
            new = p["smooth"] * boxes[i].astype(np.float64) + (1.0 - p["smooth"]) * new
        boxes[i] = new.astype(np.float32)
        lost[i] = 0
        updated[i] = True
        mean_gate[i] = _tree_sum(np.where(sel[i], g[i], 0.0)) / count
        b = boxes[i].astype(np.float64)
        area[i] = (b[2] - b[0]) * (b[3] - b[1])
    pairs = []
    for i in range(n):
        for j in range(i + 1, n):
            if updated[i] and updated[j]:
                pairs.append((i, j, pose_oks(kp[i], kp[j], area[i], area[j], sigmas)))
    dead = set()
    for i, j, oks in pairs:  # (already in the order (0, 1), (0, 2), ..., (1, 2), ...)
        if oks > p["dup_oks_thr"] and i not in dead and j not in dead:
            loser = i if mean_gate[i] < mean_gate[j] else j
            dead.add(loser)
            alive[loser] = 0
    return (boxes, alive, lost, pairs) if return_oks else (boxes, alive, lost)


def affine_params_host(boxes, input_size: Tuple[int, int], input_padding: float = 1.25):
    """Centres and scales (n, 2) float32 and the dst -> src maps (n, 2, 3) float64 of ``pp_warp_affine_u8`` for (n, 4) float32 xyxy boxes: what
    GetBBoxCenterScale + TopdownAffine(use_udp=True) compute per box before the warp, with ``rot = 0``, and ``cv2.warpAffine``'s inverse.
    Stated once more, box by box in numpy scalars; equal to ``transforms.topdown_affine_params`` + ``transforms.invert_affine`` bit for bit."""
    w, h = int(input_size[0]), int(input_size[1])
    f = np.float32
    pad, aspect = f(input_padding), f(w / h)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    n = len(boxes)
    centers, scales, maps = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros((n, 2, 3), np.float64)
    with np.errstate(all="ignore"):
        for i, (x0, y0, x1, y1) in enumerate(boxes):
            bw, bh = (x1 - x0) * pad, (y1 - y0) * pad
            cx, cy = (x1 + x0) * f(0.5), (y1 + y0) * f(0.5)
            sw, sh = (bw, bw / aspect) if bw > bh * aspect else (bh * aspect, bh)
            centers[i], scales[i] = (cx, cy), (sw, sh)
            sx, sy = f(w - 1) / sw, f(h - 1) / sh
            m = np.zeros((2, 3), np.float32)  # get_udp_warp_matrix at rot = 0: cos = 1.0, sin = 0.0
            m[0, 0], m[0, 1] = f(1.0) * sx, f(-0.0) * sx
            m[0, 2] = sx * (f(-0.5) * (cx * f(2)) * f(1.0) + f(0.5) * (cy * f(2)) * f(0.0) + f(0.5) * sw)
            m[1, 0], m[1, 1] = f(0.0) * sy, f(1.0) * sy
            m[1, 2] = sy * (f(-0.5) * (cx * f(2)) * f(0.0) - f(0.5) * (cy * f(2)) * f(1.0) + f(0.5) * sh)
            M = m.astype(np.float64)
            det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
            det = 1.0 / det if det != 0 else 0.0
            a00, a01, a10, a11 = M[1, 1] * det, M[0, 1] * -det, M[1, 0] * -det, M[0, 0] * det
            maps[i] = [[a00, a01, -a00 * M[0, 2] - a01 * M[1, 2]], [a10, a11, -a10 * M[0, 2] - a11 * M[1, 2]]]
    return centers, scales, maps


# ------------------------------------------------------------------------------------------------------------------ the device loop
def _udp_affine_of(model):
    """The ``TopdownAffine`` of the model's val pipeline; anything the device-side crop parameters do not restate is refused by name."""
    from . import transforms as T
    from .apis import _val_pipeline

    pipe = _val_pipeline(model)
    affine = [t for t in pipe.transforms if isinstance(t, T.TopdownAffine)]
    if len(affine) != 1:
        raise NotImplementedError(f"tracking needs a val pipeline with one TopdownAffine, found {len(affine)}")
    if not affine[0].use_udp:
        raise NotImplementedError("tracking: TopdownAffine(use_udp=False) is not supported - the device computes the crop parameters of "
                                  "get_udp_warp_matrix only (every config in configs/ sets use_udp=True)")
    if affine[0].with_bbox_mask:
        raise NotImplementedError("tracking: TopdownAffine(with_bbox_mask=True) is not supported")
    for t in pipe.transforms:
        if isinstance(t, T.LoadImage) and (t.pad_to_aspect_ratio or t.to_float32):
            raise NotImplementedError("tracking: LoadImage(pad_to_aspect_ratio=True) / LoadImage(to_float32=True) are not supported")
        if isinstance(t, T.GenerateTarget):
            raise NotImplementedError("tracking: a val pipeline with GenerateTarget is not supported")
    return pipe, affine[0]


class PoseTracker:
    """The closed loop on the device. Per ``submit(img)``, on the tracker's own stream and without waiting for anything: the crop warp from
    the device-side maps (``pp_warp_affine_u8``), the model step at batch ``max_tracks`` (``engine.forward_graph``; ``engine.forward`` when graph
    replay is off), ``dist.pack_records``, ``pp_track_update`` - the next frame's boxes together with their crop parameters - and ONE copy of
    the records and the track rows into pinned memory. Up to ``depth`` frames are in flight (the model steps are serial by their data
    dependency; the host decodes ahead and collects late). ``result()`` delivers, in order, what ``apis.inference_topdown(model, img, boxes)``
    returns for the boxes the tracker used for that frame - one ``PoseDataSample`` per track alive at the frame, with ``track_id`` (and
    ``track_slot``, ``track_lost``) in its metainfo; ``frame_state`` holds the downloaded rows of the frame delivered last."""

    def __init__(self, model, max_tracks: int, depth: int = 2, graph_replay: Optional[bool] = None, **params):
        import torch

        from .evaluation import COCO_SIGMAS
        from .pose_estimators import HeatmapHead

        if not 1 <= int(max_tracks) <= MAX_TRACKS:
            raise ValueError(f"max_tracks must be in 1..{MAX_TRACKS} (one workgroup follows them), got {max_tracks}")
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self.model, self.n, self.depth = model, int(max_tracks), int(depth)
        self.params = track_params(**params)
        self._pipeline, affine = _udp_affine_of(model)
        self.input_padding = float(affine.input_padding)
        eng = model.engine  # (refuses a model that is not on the GPU)
        self.engine, self.device = eng, torch.device(eng.device)
        self.K = int(eng.K)
        if self.K > MAX_KEYPOINTS:
            raise NotImplementedError(f"tracking follows poses of at most {MAX_KEYPOINTS} keypoints, the model has {self.K}")
        self.input_size = tuple(int(v) for v in model.head.decoder.input_size)  # (w, h)
        if tuple(affine.input_size) != self.input_size:
            raise ValueError(f"TopdownAffine.input_size {tuple(affine.input_size)} differs from the decoder's {self.input_size}")
        self.gate = "conf" if isinstance(model.head, HeatmapHead) else "prob"
        sig = (model.dataset_meta or {}).get("sigmas")
        if sig is None:
            if self.K != len(COCO_SIGMAS):
                raise ValueError(f"tracking needs dataset_meta['sigmas'] for a model of {self.K} keypoints (COCO's are built in)")
            sig = COCO_SIGMAS
        self.sigmas = np.asarray(sig, np.float64).reshape(-1)
        if len(self.sigmas) != self.K:
            raise ValueError(f"{len(self.sigmas)} sigmas for {self.K} keypoints")
        self.graph_replay = bool(model.graph_replay if graph_replay is None else graph_replay)
        self._flip = model._check_flip_cfg()
        self._flip_indices = list(model.dataset_meta["flip_indices"]) if self._flip else None
        self._shift = model._shift_heatmap
        self._want_hm = bool(model.test_cfg.get("output_heatmaps", False))
        # a workspace (and graph) of the tracker's own: inference_topdown on the same model may run while frames are in flight
        # (the lowest slot no living tracker of this engine holds: trackers made one after the other share a workspace and a graph)
        in_use = eng.__dict__.setdefault("_tracker_slots", set())
        self._slot = next(s for s in range(1000, 1000 + len(in_use) + 1) if s not in in_use)
        in_use.add(self._slot)
        self.stream = torch.cuda.Stream(device=self.device)
        n, K = self.n, self.K
        # one block per parity: the frame's records and the track rows its crops were cut with; the update writes the other block's rows
        self._layout, off = {}, 0
        for name, dtype, shape in (("records", torch.float64, (n, K, 7)), ("maps", torch.float64, (n, 2, 3)), ("boxes", torch.float32, (n, 4)),
                                   ("centers", torch.float32, (n, 2)), ("scales", torch.float32, (n, 2)), ("alive", torch.int32, (n,)),
                                   ("lost", torch.int32, (n,))):
            size = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            self._layout[name] = (off, size, dtype, shape)
            off += size
        self._block_bytes = off
        self._dev = [torch.zeros(off, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self._host = [torch.zeros(off, dtype=torch.uint8, pin_memory=True) for _ in range(self.depth)]
        self._events = [torch.cuda.Event() for _ in range(self.depth)]
        self._sigmas_dev = torch.as_tensor(self.sigmas).to(self.device)
        self._crops = None if self.graph_replay else torch.zeros((n, 3, self.input_size[1], self.input_size[0]), dtype=torch.uint8, device=self.device)
        self._next = 0                       # index of the next frame submitted
        self._pending = deque()              # frames submitted and not delivered, oldest first
        self._uploads = []                   # pinned rows of add() still on their way
        self._ids = [-1] * n                 # track id per slot (-1: free)
        self._since = [0] * n                # the frame a slot's occupant started at
        self._free = set(range(n))           # slots the host knows to be dead or never used
        self._next_id = 0
        self._started = False
        self.frame_state: Optional[Dict[str, np.ndarray]] = None

    def __del__(self):
        try:
            self.engine.__dict__.get("_tracker_slots", set()).discard(self._slot)
        except AttributeError:  # (the constructor refused)
            pass

    # -- views
    def _view(self, buf, name):
        off, size, dtype, shape = self._layout[name]
        return buf[off:off + size].view(dtype).view(shape)

    def _affine(self, buf) -> None:
        """Centres, scales and maps of every slot of a block from its boxes (one launch on the current stream)."""
        import torch

        from . import _lib

        _lib.call("pp_track_affine_params", self._view(buf, "boxes").data_ptr(), self.n, self.input_size[0], self.input_size[1],
                  self.input_padding, self._view(buf, "centers").data_ptr(), self._view(buf, "scales").data_ptr(),
                  self._view(buf, "maps").data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)

    def _update(self, cur, nxt) -> None:
        """The rule on block ``cur`` (records and the rows its crops were cut with) into the rows of block ``nxt``, with their crop parameters
        (one launch on the current stream)."""
        import torch

        from . import _lib

        v, p = self._view, self.params
        _lib.call("pp_track_update", v(cur, "records").data_ptr(), v(cur, "centers").data_ptr(), v(cur, "scales").data_ptr(), self.n, self.K,
                  self.input_size[0], self.input_size[1], GATE_PROB if self.gate == "prob" else GATE_CONF, self._sigmas_dev.data_ptr(),
                  v(cur, "boxes").data_ptr(), v(cur, "alive").data_ptr(), v(cur, "lost").data_ptr(), p["kpt_thr"], p["min_keypoints"], p["expand"],
                  p["min_side"], p["smooth"], p["max_lost"], p["dup_oks_thr"], v(nxt, "boxes").data_ptr(), v(nxt, "alive").data_ptr(),
                  v(nxt, "lost").data_ptr(), self.input_padding, v(nxt, "centers").data_ptr(), v(nxt, "scales").data_ptr(), v(nxt, "maps").data_ptr(),
                  torch.cuda.current_stream(self.device).cuda_stream)

    # -- tracks
    def start(self, bboxes) -> List[int]:
        """The first frame's boxes (m <= max_tracks, xyxy): slots 0 .. m-1; the others are free and hold the box of the input itself until
        ``add`` fills them. Forgets every earlier track. Returns the track ids."""
        import torch

        if self._pending:
            raise RuntimeError("start() with frames in flight: collect their results first")
        bboxes = np.asarray(bboxes, np.float32).reshape(-1, 4)
        if not 1 <= len(bboxes) <= self.n:
            raise ValueError(f"start() takes 1..{self.n} boxes, got {len(bboxes)}")
        if not np.isfinite(bboxes).all():
            raise ValueError("boxes must be finite")
        torch.cuda.synchronize(self.device)
        if self.graph_replay:  # the capture (a device-wide synchronisation) happens here, not between two frames
            self.engine.capture(self.n, self._flip, self._flip_indices, self._want_hm, self._slot, self._shift)
        n, m = self.n, len(bboxes)
        rows = np.zeros(self._block_bytes, np.uint8)
        boxes = np.tile(np.array([0, 0, self.input_size[0], self.input_size[1]], np.float32), (n, 1))
        boxes[:m] = bboxes
        alive = np.zeros(n, np.int32)
        alive[:m] = 1
        for name, a in (("boxes", boxes), ("alive", alive)):
            off, size = self._layout[name][:2]
            rows[off:off + size] = a.view(np.uint8).reshape(-1)
        self._next_id = getattr(self, "_next_id", 0)
        self._ids = [-1] * n
        ids = []
        for s in range(m):
            self._ids[s] = self._next_id
            ids.append(self._next_id)
            self._next_id += 1
        self._since = [self._next] * n
        self._free = set(range(m, n))
        self._parity = 0
        with torch.cuda.stream(self.stream):
            self._dev[0].copy_(torch.from_numpy(rows))
            self._dev[1].copy_(self._dev[0])
            self._affine(self._dev[0])
        self.stream.synchronize()
        self._started = True
        return ids

    def free_slots(self) -> List[int]:
        """Slots the host knows to be free: never used, or seen dead in a delivered frame (a dead track stays dead)."""
        return sorted(self._free)

    def add(self, bboxes) -> List[int]:
        """New boxes into free slots, from the next submitted frame on; returns their (fresh) track ids. A small upload enqueued on the
        tracker's stream - no synchronisation. The host learns of a death when the frame's result is delivered, so a slot is free up to
        ``depth`` frames after its track died; more boxes than free slots is an error."""
        import torch

        if not self._started:
            raise RuntimeError("add() before start()")
        bboxes = np.asarray(bboxes, np.float32).reshape(-1, 4)
        if not np.isfinite(bboxes).all():
            raise ValueError("boxes must be finite")
        slots = self.free_slots()[:len(bboxes)]
        if len(slots) < len(bboxes):
            raise RuntimeError(f"add(): {len(bboxes)} boxes for {len(slots)} free slot(s) of {self.n}")
        if not slots:
            return []
        up = torch.zeros((len(slots), 4), dtype=torch.float32).pin_memory()
        up.copy_(torch.from_numpy(bboxes))
        idx = torch.tensor(slots, dtype=torch.int64).pin_memory()
        buf = self._dev[self._parity]
        with torch.cuda.stream(self.stream):
            didx = idx.to(self.device, non_blocking=True)
            self._view(buf, "boxes").index_copy_(0, didx, up.to(self.device, non_blocking=True))
            self._view(buf, "alive").index_fill_(0, didx, 1)
            self._view(buf, "lost").index_fill_(0, didx, 0)
            self._affine(buf)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._uploads = [u for u in self._uploads if not u[0].query()] + [(ev, up, idx)]  # the pinned rows live until their copy has run
        ids = []
        for s in slots:
            self._free.discard(s)
            self._ids[s], self._since[s] = self._next_id, self._next
            ids.append(self._next_id)
            self._next_id += 1
        return ids

    # -- frames
    def submit(self, img) -> int:
        """Enqueue one frame ((H, W, 3) uint8 BGR, device tensor or host array); returns its index. Waits for nothing; at most ``depth``
        frames may be undelivered."""
        import torch

        from . import _lib
        from .dist import pack_records

        if not self._started:
            raise RuntimeError("submit() before start()")
        if len(self._pending) >= self.depth:
            raise RuntimeError(f"{self.depth} frames are in flight: collect result() before submitting another")
        if isinstance(img, np.ndarray):
            img = torch.from_numpy(np.ascontiguousarray(img)).to(self.device)
        if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3):
            raise TypeError("a frame is an (H, W, 3) uint8 BGR image")
        img = img.contiguous()
        t, j = self._next, self._next % self.depth
        cur, nxt = self._dev[self._parity], self._dev[1 - self._parity]
        eng, n = self.engine, self.n
        w, h = self.input_size
        v = self._view
        self.stream.wait_stream(torch.cuda.current_stream(self.device))  # the frame's producer
        with torch.cuda.stream(self.stream):
            s = self.stream.cuda_stream
            crops = eng.capture(n, self._flip, self._flip_indices, self._want_hm, self._slot, self._shift) if self.graph_replay else self._crops
            _lib.call("pp_warp_affine_u8", img.data_ptr(), int(img.shape[0]), int(img.shape[1]), 3, v(cur, "maps").data_ptr(), crops.data_ptr(),
                      n, h, w, s)
            run = eng.forward_graph if self.graph_replay else eng.forward
            out = run(crops, self._flip, self._flip_indices, return_heatmaps=self._want_hm, slot=self._slot, shift_heatmap=self._shift)
            pack_records(out, into=v(cur, "records"))
            self._update(cur, nxt)
            heatmaps = out["heatmaps"][:n].clone() if self._want_hm else None  # the workspace is overwritten by the next frame
            self._host[j].copy_(cur, non_blocking=True)
            self._events[j].record(self.stream)
        self._pending.append(dict(index=t, slot=j, img=img, shape=tuple(int(x) for x in img.shape), ids=list(self._ids), heatmaps=heatmaps))
        self._parity = 1 - self._parity
        self._next = t + 1
        return t

    def _samples(self, shape, boxes: np.ndarray) -> list:
        """The ``data_samples`` of ``inference_topdown`` for these boxes: the model's val pipeline without the image and without the warp."""
        import torch

        from . import transforms as T

        frame = torch.empty(shape, dtype=torch.uint8, device="meta")  # LoadImage reads its shape only
        nothing = torch.empty(0, dtype=torch.uint8)
        out = []
        for bbox in boxes:
            r = dict(img=frame, bbox=bbox[None, :4], bbox_score=np.ones(1, dtype=np.float32))
            r.update(self.model.dataset_meta)
            for t in self._pipeline.transforms:
                if isinstance(t, T.TopdownAffine):
                    t.prepare(r)
                    r["img"] = nothing
                else:
                    r = t(r)
            out.append(r["data_samples"])
        return out

    def result(self) -> list:
        """The oldest undelivered frame: ``list[PoseDataSample]`` of the tracks alive at it (blocks until its copy has landed)."""
        if not self._pending:
            raise RuntimeError("result() without a frame in flight")
        e = self._pending.popleft()
        self._events[e["slot"]].synchronize()
        host = self._host[e["slot"]].numpy()
        st = {}
        for name, (off, size, dtype, shape) in self._layout.items():
            st[name] = host[off:off + size].view(dict(float64=np.float64, float32=np.float32, int32=np.int32)[str(dtype).split(".")[1]]).reshape(shape).copy()
        st["track_ids"] = np.array(e["ids"], np.int64)
        st["index"] = e["index"]
        self.frame_state = st
        for s in range(self.n):  # deaths the host learns of now (a slot refilled since keeps its new occupant)
            if not st["alive"][s] and e["ids"][s] >= 0 and self._ids[s] == e["ids"][s]:
                self._ids[s] = -1
                self._free.add(s)
        live = [s for s in range(self.n) if st["alive"][s] and e["ids"][s] >= 0]
        if not live:
            return []
        samples = self._samples(e["shape"], st["boxes"][live])
        for ds, s in zip(samples, live):
            # the very centre and scale the device cut the crop with (equal to the pipeline's: tests/test_track_gpu.py)
            ds.set_metainfo(dict(input_center=st["centers"][s].copy(), input_scale=st["scales"][s].copy(), track_id=int(e["ids"][s]),
                                 track_slot=int(s), track_lost=int(st["lost"][s])))
            if self.model.metainfo is not None:
                ds.set_metainfo(self.model.metainfo)
        rec = np.ascontiguousarray(st["records"][live])
        test_cfg = self.model.test_cfg
        if self._want_hm:
            preds, fields = self.model.head.pack_records(rec, test_cfg, e["heatmaps"][live])
        else:
            preds, fields = self.model.head.pack_records(rec, test_cfg), None
        return self.model.add_pred_to_datasample(preds, fields, samples)

    def drain(self) -> List[list]:
        """Every undelivered frame, in order."""
        out = []
        while self._pending:
            out.append(self.result())
        return out

    @property
    def in_flight(self) -> int:
        return len(self._pending)


def inference_topdown_track(model, frames, init_bboxes, depth: int = 2, max_tracks: Optional[int] = None, **params):
    """``inference_topdown`` over the frames of a video with the boxes following the persons: ``init_bboxes`` (m, 4) xyxy are the first
    frame's, every later frame is cropped with the boxes ``PoseTracker`` derived from the frame before it - on the device, ``depth`` frames in
    flight. ``frames`` yields (H, W, 3) uint8 BGR images (device tensors or host arrays); the generator yields one ``list[PoseDataSample]`` per
    frame, in order. ``max_tracks`` (default: the number of first boxes) is the fixed batch of the loop; ``params``: ``TRACK_DEFAULTS``."""
    import torch

    init_bboxes = np.asarray(init_bboxes, np.float32).reshape(-1, 4)
    tracker = PoseTracker(model, max_tracks or len(init_bboxes), depth=depth, **params)
    tracker.start(init_bboxes)
    with torch.no_grad():
        for img in frames:
            while tracker.in_flight >= depth:
                yield tracker.result()
            tracker.submit(img)
        while tracker.in_flight:
            yield tracker.result()
