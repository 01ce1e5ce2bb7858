"""The ``--draw-heatmap`` picture of the reference demo on the device (mmpose/visualization/local_visualizer.py:215-343,
520-585, 796-865): the pose panel - boxes, skeleton links and keypoints on the image - and under it the presence-probability
area of every keypoint on the padded canvas that shows keypoints outside the image.

All drawing runs in ``csrc/pp_render.hip`` (the rules are stated there); the host uploads the instances and copies the
finished image back once. The drawing rules differ from the reference where the reference is not reproducible:
  * the reference draws links and points through matplotlib (anti-aliased); here a pixel takes a link's colour when its
    distance to the segment between the two int positions is at most max(thickness, 1) / 2, and a keypoint's colour
    (blended by ``alpha``) when its distance to the keypoint is at most ``radius`` - fp32 formulas in pp_render.hip;
  * the outline of a probability area is every mask pixel with a 4-neighbour outside the mask or the canvas. cv2 draws the
    RETR_EXTERNAL contours with LINE_4 instead: it leaves the rims of holes un-outlined and its diagonal steps can put an
    outline pixel one pixel outside the mask;
  * the panel resize is bilinear with half-pixel centres in fp32 (cv2.resize uses fixed-point weights).
cv2 and matplotlib are not available to pin the difference.

``draw_datasamples`` draws the pictures of a whole batch of samples in one set of launches (``csrc/pp_render_batch.hip``, the
same per-pixel bodies): what ``tools/test.py --show-dir`` dumps. Byte for byte the pictures of ``draw_datasample``.
"""
import numpy as np
import torch

from . import _lib

PAREA_MAX_KEYPOINTS = 22  # colours of the reference's probability-area table (local_visualizer.py:523-547)

# configs/_base_/datasets/coco.py: skeleton_info (as keypoint indices), its link colours, keypoint_info colours (RGB)
COCO_SKELETON = ((15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9), (8, 10),
                 (1, 2), (0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6))
_GREEN, _ORANGE, _BLUE = (0, 255, 0), (255, 128, 0), (51, 153, 255)
COCO_LINK_COLORS = (_GREEN, _GREEN, _ORANGE, _ORANGE, _BLUE, _BLUE, _BLUE, _BLUE, _GREEN, _ORANGE, _GREEN, _ORANGE, _BLUE, _BLUE,
                    _BLUE, _BLUE, _BLUE, _BLUE, _BLUE)
COCO_KEYPOINT_COLORS = (_BLUE,) * 5 + (_GREEN, _ORANGE) * 6

_INT_LIMIT = 2 ** 30  # box corners are clipped to this before the int conversion (the kernels compare ints only)


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _as_device_image(image_rgb, device):
    t = torch.as_tensor(np.ascontiguousarray(image_rgb)) if isinstance(image_rgb, np.ndarray) else image_rgb
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"expected an (H, W, 3) uint8 RGB image, got {tuple(t.shape)} {t.dtype}")
    return t.to(device).contiguous()


def _output(out, shape, device):
    """``out`` as given - checked to be a dense uint8 tensor of ``shape`` on ``device``, the kernels write all of it - or a new one."""
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.uint8 or out.device != device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {tuple(shape)} on {device}, got {tuple(out.shape)} "
                         f"{out.dtype} on {out.device}")
    return out


def _check_device(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the visualizer draws on the GPU only (no CPU fallback)")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def int_boxes(boxes) -> np.ndarray:
    """(n, 4) x1, y1, x2, y2 -> int32 corners as ``int()`` gives them (truncation toward zero) after clipping to +-2^30; a box
    with a non-finite corner is dropped."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    b = b[np.isfinite(b).all(axis=1)]
    return np.clip(b, -_INT_LIMIT, _INT_LIMIT).astype(np.int64).astype(np.int32)


def aspect_boxes(boxes, image_pad) -> np.ndarray:
    """The rectangles of the heatmap panel (local_visualizer.py:844-858): every box shifted by the (left, top) pad, grown to
    3:4 and padded 1.25 (fix_bbox_aspect_ratio), corners truncated to int. Returns int32 (n, 4)."""
    from .transforms import fix_bbox_aspect_ratio_xyxy

    b = np.array(boxes, np.float32).reshape(-1, 4)
    pad = np.asarray(image_pad).reshape(4)
    b[:, :2] += pad[:2]
    b[:, 2:] += pad[:2]
    return int_boxes(fix_bbox_aspect_ratio_xyxy(b, aspect_ratio=3 / 4, padding=1.25))


def probability_area_thresholds(maps):
    """Per keypoint the threshold of its probability area and whether it is drawn (pp_parea_thresholds): for a (K, H, W)
    float32 device tensor, thr[k] = the largest value v of maps[k] whose superlevel set {x >= v} holds at least 0.75 of the
    map's fp64 mass, and draw[k] = 0 when the map has a negative or non-finite value or a mass below 0.75 (:560-568). The
    area is ``maps[k] > thr[k]``. Returns (thr float32 (K,), draw int32 (K,)) device tensors."""
    device = _check_device(maps.device)
    maps = maps.to(torch.float32).contiguous()
    K, H, W = maps.shape
    n = int(_lib.lib.pp_parea_scratch_bytes(K, H, W))
    if n < 0:
        raise _lib.ProbPoseLibraryError("pp_parea_scratch_bytes", _lib.lib.pp_status_string(n).decode(), _lib.last_error())
    scratch = torch.empty(n, dtype=torch.uint8, device=device)
    thr = torch.empty(K, dtype=torch.float32, device=device)
    draw = torch.empty(K, dtype=torch.int32, device=device)
    _lib.call("pp_parea_thresholds", maps.data_ptr(), K, H, W, scratch.data_ptr(), thr.data_ptr(), draw.data_ptr(), _stream(device))
    return thr, draw


def render_probability_areas(posterior, image_rgb, image_pad, boxes=None, out=None):
    """The heatmap panel (local_visualizer.py:520-585, 844-858) as an (Hp, Wp, 3) uint8 device tensor: ``image_rgb`` (H, W, 3)
    inside an (80, 80, 80) border of ``image_pad`` = [left, top, right, bottom], the probability area of every keypoint of
    ``posterior`` (K <= 22, Hp, Wp) blended over it in the reference's colours and outlined, then the aspect-fixed
    rectangles of ``boxes`` (n, 4) xyxy in image coordinates, or none."""
    device = _check_device(posterior.device)
    posterior = posterior.to(torch.float32).contiguous()
    K, Hp, Wp = posterior.shape
    img = _as_device_image(image_rgb, device)
    H, W = img.shape[:2]
    pad = [int(v) for v in np.asarray(image_pad).reshape(4)]
    if (Hp, Wp) != (H + pad[1] + pad[3], W + pad[0] + pad[2]):
        raise ValueError(f"maps {(Hp, Wp)} are not the image {(H, W)} padded by {pad}")
    thr, draw = probability_area_thresholds(posterior)
    rects = aspect_boxes(boxes, pad) if boxes is not None else np.zeros((0, 4), np.int32)
    rects_d = torch.from_numpy(np.ascontiguousarray(rects)).to(device)
    out = _output(out, (Hp, Wp, 3), device)
    _lib.call("pp_parea_compose", img.data_ptr(), H, W, pad[0], pad[1], posterior.data_ptr(), K, thr.data_ptr(), draw.data_ptr(),
              rects_d.data_ptr() if len(rects) else None, len(rects), _lib.ptr(out), Hp, Wp, _stream(device))
    return out


def draw_poses(image_rgb, keypoints, keypoints_visible, bboxes=None, skeleton=COCO_SKELETON, link_colors=COCO_LINK_COLORS,
               keypoint_colors=COCO_KEYPOINT_COLORS, kpt_thr=0.3, radius=3.0, thickness=1.0, alpha=0.8, out=None,
               device="cuda:0"):
    """The pose panel (_draw_instances_kpts + _draw_instances_bbox, local_visualizer.py:215-343) as an (H, W, 3) uint8 device
    tensor: per instance its box (int corners, 1-px green), its links (skipped as in :285-297), its points (drawn when
    ``keypoints_visible >= kpt_thr``). ``keypoints`` (n, K, 2), ``keypoints_visible`` (n, K), ``bboxes`` (n, 4) xyxy or None."""
    device = _check_device(image_rgb.device if isinstance(image_rgb, torch.Tensor) else device)
    img = _as_device_image(image_rgb, device)
    H, W = img.shape[:2]
    K = len(keypoint_colors)
    kp = np.ascontiguousarray(np.asarray(keypoints, np.float32).reshape(-1, K, 2))
    n = len(kp)
    vis = np.ascontiguousarray(np.asarray(keypoints_visible, np.float32).reshape(n, K))
    sk = np.ascontiguousarray(np.asarray(skeleton, np.int32).reshape(-1, 2))
    L = len(sk)
    if L and (sk.min() < 0 or sk.max() >= K):
        raise ValueError(f"skeleton links name keypoints outside 0..{K - 1}")
    lc = np.ascontiguousarray(np.asarray(link_colors, np.uint8).reshape(L, 3))
    kc = np.ascontiguousarray(np.asarray(keypoint_colors, np.uint8).reshape(K, 3))
    boxes = None
    if bboxes is not None:
        b = np.asarray(bboxes, np.float64).reshape(n, 4)
        ib = int_boxes(b)
        if len(ib) != n:  # keep the rows aligned with the instances: a non-finite box is drawn nowhere
            ib = np.full((n, 4), -_INT_LIMIT, np.int32)
            ok = np.isfinite(b).all(axis=1)
            ib[ok] = int_boxes(b[ok])
        boxes = torch.from_numpy(ib).to(device)
    dev = {name: torch.from_numpy(a).to(device) for name, a in (("kp", kp), ("vis", vis), ("sk", sk), ("lc", lc), ("kc", kc))}
    out = _output(out, (H, W, 3), device)
    _lib.call("pp_draw_poses", img.data_ptr(), H, W, dev["kp"].data_ptr(), dev["vis"].data_ptr(), _lib.ptr(boxes), n, K,
              dev["sk"].data_ptr() if L else None, dev["lc"].data_ptr() if L else None, dev["kc"].data_ptr(), L, float(kpt_thr),
              float(radius), float(thickness), float(alpha), _lib.ptr(out), _stream(device))
    return out


def resize_rgb(src, size_hw, out=None):
    """cv2.resize(src, (W, H), INTER_LINEAR) of an (h, w, 3) uint8 device tensor (fp32 bilinear, half-pixel centres)."""
    device = _check_device(src.device)
    H, W = int(size_hw[0]), int(size_hw[1])
    if src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3 or not src.is_contiguous():
        raise ValueError(f"expected a contiguous (h, w, 3) uint8 tensor, got {tuple(src.shape)} {src.dtype}")
    out = _output(out, (H, W, 3), device)
    _lib.call("pp_resize_bilinear_u8", _lib.ptr(src), src.shape[0], src.shape[1], _lib.ptr(out), H, W, _stream(device))
    return out


# pp_render_picture / pp_render_instance of include/probpose_mi355x.h
_PICTURE = np.dtype([("image", "<u8"), ("out", "<u8"), ("scratch_offset", "<i8"), ("height", "<i4"), ("width", "<i4"), ("bgr", "<i4"),
                     ("heatmap", "<i4"), ("pad", "<i4", (4,)), ("canvas_h", "<i4"), ("canvas_w", "<i4"), ("first", "<i4"), ("count", "<i4")])
RENDER_MAX_KEYPOINTS = 32
RENDER_MAX_INSTANCES = 255  # per picture (PP_RENDER_MAX_INSTANCES)
_INSTANCE = np.dtype([("maps", "<u8"), ("inverse", "<f8", (6,)), ("keypoints", "<f4", (2 * RENDER_MAX_KEYPOINTS,)),
                      ("visible", "<f4", (RENDER_MAX_KEYPOINTS,)), ("presence", "<f4", (RENDER_MAX_KEYPOINTS,)), ("box", "<i4", (4,)),
                      ("rect", "<i4", (4,)), ("box_valid", "<i4"), ("rect_valid", "<i4")])
assert _PICTURE.itemsize == 72 and _INSTANCE.itemsize == 608
RENDER_SCRATCH_DEFAULT = 1 << 30  # a memory bound (64 full-HD pictures would need about 10 GB at once), not a tuned number
# the stages of one pp_render_samples_batch call with a heatmap panel among its pictures, in launch order (without: the pose panel alone)
RENDER_BATCH_LAUNCHES = ("revert", "sum", "scale") + ("hist", "select") * 3 + ("compose", "poses", "resize")
batch_calls = 0  # pp_render_samples_batch calls since import
batch_uploads = 0  # host-to-device copies of draw_datasamples since import (one per call)


def render_share_bytes(K: int, canvas_h: int, canvas_w: int) -> int:
    """Scratch of one heatmap picture in a batched call, as ``pp_render_batch_scratch_bytes`` gives it: the (K, Hp, Wp) float32
    posterior maps, the (Hp, Wp, 3) canvas, 64 sum partials, and per keypoint the radix select's state (5), part flags and
    2048-bin part histograms (float64), thresholds and draw flags; the regions on multiples of 256 bytes where it matters."""
    from .staging import _align

    hw = int(canvas_h) * int(canvas_w)
    parts = min(max((hw + 16383) // 16384, 1), 32)
    at = _align(K * hw * 4)
    at = _align(at + hw * 3)
    at += K * 64 * 8 + K * 5 * 8 + K * parts * 8 + K * parts * 2048 * 8 + K * 4 + K * 4
    return _align(at)


def plan_render_chunks(shapes, pads, K: int, budget: int = RENDER_SCRATCH_DEFAULT) -> list:
    """The host plan of ``draw_datasamples`` (numpy only): ``shapes[i]`` = (H, W) of picture i, ``pads[i]`` = its [left, top,
    right, bottom] canvas border, or None for a picture without heatmap panel. The pictures are cut, in order, into chunks
    whose scratch fits ``budget`` bytes (a picture that alone exceeds it goes alone); one ``pp_render_samples_batch`` call draws
    a chunk. Per chunk a dict: ``pictures`` (their indices), ``canvas`` (n, 2) int (Hp, Wp; the image's for a picture without
    panel), ``scratch_offset`` (n,) int64 (each share on a multiple of 256, disjoint, in order; 0 without panel),
    ``scratch_bytes`` (their sum) and ``tiles``, int32 2 (n + 1): the exclusive prefix (total last) of the canvas row tiles
    Hp * ceil(Wp / 256) of the panel pictures, then that of the image row tiles H * ceil(W / 256) of all pictures - the flat
    grids of the launches."""
    if len(shapes) != len(pads):
        raise ValueError("one pad entry (or None) per picture")
    if budget < 0:
        raise ValueError("budget must not be negative")
    shares, canvas = [], []
    for (H, W), pad in zip(shapes, pads):
        H, W = int(H), int(W)
        if H <= 0 or W <= 0:
            raise ValueError(f"empty picture {(H, W)}")
        if pad is None:
            canvas.append((H, W))
            shares.append(0)
        else:
            p = [int(v) for v in np.asarray(pad).reshape(4)]
            if min(p) < 0:
                raise ValueError(f"negative padding {p}")
            canvas.append((H + p[1] + p[3], W + p[0] + p[2]))
            shares.append(render_share_bytes(K, *canvas[-1]))
    chunks, cur, used = [], [], 0
    for i, share in enumerate(shares):
        if cur and share and used + share > budget:  # (a picture without panel needs no scratch: it never opens a chunk)
            chunks.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += share
    if cur:
        chunks.append(cur)
    out = []
    for idx in chunks:
        n = len(idx)
        offsets, tiles, at = np.zeros(n, np.int64), np.zeros(2 * (n + 1), np.int64), 0
        for j, i in enumerate(idx):
            H, W = int(shapes[i][0]), int(shapes[i][1])
            if shares[i]:
                offsets[j] = at
                at += shares[i]
            tiles[j + 1] = tiles[j] + (canvas[i][0] * ((canvas[i][1] + 255) // 256) if shares[i] else 0)
            tiles[n + 2 + j] = tiles[n + 1 + j] + H * ((W + 255) // 256)
        if tiles.max() >= 2 ** 31 - 1:
            raise ValueError("a chunk of 2^31 row tiles or more: lower the scratch budget")
        out.append(dict(pictures=idx, canvas=np.array([canvas[i] for i in idx], np.int64).reshape(n, 2), scratch_offset=offsets,
                        scratch_bytes=int(at), tiles=tiles.astype(np.int32)))
    return out


class _Picture:
    """What ``draw_datasamples`` reads of one merged sample (everything on the host but the image and the maps)."""

    __slots__ = ("key", "image", "host_image", "H", "W", "n", "kpts", "vis", "boxes", "box_ok", "maps", "inv", "pad", "rects", "rect_ok", "presence")


def _gather_picture(image, ds, K, draw_bbox, draw_heatmap, device) -> _Picture:
    """The host half of ``PoseLocalVisualizer.draw_datasample`` for one sample: the same fields, the same conversions, the same
    padding, inverse maps, int boxes and aspect boxes."""
    from .structures import _image_padding
    from .transforms import fix_bbox_aspect_ratio_xyxy, get_warp_matrix, invert_affine

    p = _Picture()
    p.key = id(image)
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError(f"expected an (H, W, 3) uint8 image, got {image.shape} {image.dtype}")
        p.host_image, p.image = np.ascontiguousarray(image), None
        p.H, p.W = image.shape[:2]
    else:
        p.host_image, p.image = None, _as_device_image(image, device)
        p.H, p.W = p.image.shape[:2]
    pi = ds.pred_instances if "pred_instances" in ds else None
    with_heatmap = bool(draw_heatmap) and pi is not None and "pred_fields" in ds and "heatmaps" in ds.pred_fields
    p.n, p.maps, p.pad, p.boxes, p.rects = 0, None, None, None, None
    if pi is not None and "keypoints" in pi:
        kpts = pi.get("transformed_keypoints", pi.keypoints)
        p.kpts = np.ascontiguousarray(np.asarray(kpts, np.float32).reshape(-1, K, 2))
        p.n = len(p.kpts)
        vis = pi.keypoints_visible if "keypoints_visible" in pi else np.ones(np.asarray(kpts).shape[:-1], np.float32)
        p.vis = np.ascontiguousarray(np.asarray(vis, np.float32).reshape(p.n, K))
        if draw_bbox and "bboxes" in pi:
            b = np.asarray(pi.bboxes, np.float64).reshape(p.n, 4)
            p.box_ok = np.isfinite(b).all(axis=1)
            p.boxes = np.zeros((p.n, 4), np.int32)
            p.boxes[p.box_ok] = int_boxes(b[p.box_ok])
    elif with_heatmap:
        raise ValueError("draw_heatmap needs pred_instances.keypoints")
    if p.n > RENDER_MAX_INSTANCES:
        raise ValueError(f"{p.n} instances in one picture: the batched drawing takes at most {RENDER_MAX_INSTANCES} (draw_datasample has no limit)")
    if not with_heatmap:
        return p
    if "keypoints_probs" not in pi:
        raise ValueError("draw_heatmap needs pred_instances.keypoints_probs (the presence probabilities of ProbPose)")
    meta = ds.metainfo
    centers = np.asarray(meta["input_center"], np.float64).reshape(-1, 2)
    scales = np.asarray(meta["input_scale"], np.float64).reshape(-1, 2)
    maps = ds.pred_fields.heatmaps
    maps = maps if isinstance(maps, torch.Tensor) else torch.as_tensor(np.asarray(maps))
    if maps.dim() != 4 or maps.shape[1] != K or maps.shape[0] != p.n or len(centers) != p.n:
        raise ValueError(f"draw_datasamples takes the un-reverted (n, K, h, w) maps of a sample's n instances; got {tuple(maps.shape)} for "
                         f"{p.n} instances of {K} keypoints and {len(centers)} input centers")
    p.maps = maps.to(device=device, dtype=torch.float32).contiguous()
    ori_shape = meta["ori_shape"]
    if (int(ori_shape[0]), int(ori_shape[1])) != (p.H, p.W):
        raise ValueError(f"ori_shape {tuple(ori_shape)} is not the image {(p.H, p.W)}")
    p.pad = np.asarray(_image_padding(centers, scales, ori_shape)).reshape(4)
    h, w = int(maps.shape[2]), int(maps.shape[3])
    # merge_data_samples: the maps go back on the padded image, each centre shifted by the (left, top) pad
    p.inv = np.stack([invert_affine(get_warp_matrix(centers[i] + p.pad[:2], scales[i], 0, (w, h), inv=True)) for i in range(p.n)])
    p.presence = np.ascontiguousarray(np.asarray(pi.keypoints_probs, np.float32).reshape(-1, K))
    if len(p.presence) != p.n:
        raise ValueError(f"keypoints_probs of {len(p.presence)} instances for {p.n} instances")
    if draw_bbox:
        src = ds.gt_instances if "gt_instances" in ds and "bboxes" in ds.gt_instances else pi
        if "bboxes" in src:
            b = np.array(src.bboxes, np.float32).reshape(-1, 4)  # aspect_boxes, row by row
            if len(b) != p.n:
                raise ValueError(f"{len(b)} boxes for {p.n} instances")
            b[:, :2] += p.pad[:2]
            b[:, 2:] += p.pad[:2]
            fixed = np.asarray(fix_bbox_aspect_ratio_xyxy(b, aspect_ratio=3 / 4, padding=1.25), np.float64).reshape(-1, 4)
            p.rect_ok = np.isfinite(fixed).all(axis=1)
            p.rects = np.zeros((p.n, 4), np.int32)
            p.rects[p.rect_ok] = int_boxes(fixed[p.rect_ok])
    return p


def draw_datasamples(images, data_samples, draw_bbox=True, draw_heatmap=False, kpt_thr=0.3, channel_order="rgb",
                     scratch_bytes=RENDER_SCRATCH_DEFAULT, skeleton=COCO_SKELETON, link_colors=COCO_LINK_COLORS,
                     keypoint_colors=COCO_KEYPOINT_COLORS, radius=3.0, thickness=1.0, alpha=0.8, device="cuda:0", staging=None, out=None,
                     scratch=None):
    """The pictures of many merged samples in one set of launches per chunk (pp_render_samples_batch): a list of uint8 RGB
    device tensors, element i byte for byte ``PoseLocalVisualizer.draw_datasample(images[i], data_samples[i], ...)`` applied
    to the RGB image - (H, W, 3), or with ``draw_heatmap`` and heatmaps in ``pred_fields`` (2H, W, 3). ``images[i]``: (H, W, 3)
    uint8, host array (uploaded with the tables) or device tensor, in ``channel_order`` "rgb" or "bgr" (swapped where the
    kernels read it). ``data_samples[i]``: a merged sample (``merge_data_samples``-shaped: the instances concatenated,
    ``input_center`` / ``input_scale`` stacked) whose ``pred_fields.heatmaps``, when present, are the UN-REVERTED (n_i, K, h, w)
    maps of its instances as a device tensor: reverting, merging and the posterior run inside the call. ``draw_bbox`` and
    ``kpt_thr``: one value, or one per picture.

    A chunk of pictures costs ONE host-to-device copy (picture table, instance table, tile prefixes, skeleton, colours and the
    host images) and one pp_render_samples_batch call: twelve launches whatever the number of pictures (one - the pose panel -
    when none of them has a heatmap panel). The batch is cut into chunks whose scratch (the posterior maps of every picture of
    the chunk at once) fits ``scratch_bytes``; the default, 1 GiB, is a memory bound and was not tuned. ``kpt_thr`` is an
    argument of the call, so a list of differing values cuts the batch at every change as well. ``out``: a list of dense uint8
    device tensors to draw into; ``scratch``: a uint8 device tensor to use when it is large enough for a chunk."""
    global batch_calls, batch_uploads
    from .staging import BatchStaging, StagedBlock, _align

    if channel_order not in ("rgb", "bgr"):
        raise ValueError(f"channel_order must be 'rgb' or 'bgr', got {channel_order!r}")
    device = _check_device(device)
    images, data_samples = list(images), list(data_samples)
    n_all = len(images)
    if len(data_samples) != n_all:
        raise ValueError(f"{n_all} images for {len(data_samples)} samples")
    if n_all == 0:
        return []
    K = len(keypoint_colors)
    if K > RENDER_MAX_KEYPOINTS:
        raise ValueError(f"{K} keypoints: the batched drawing takes at most {RENDER_MAX_KEYPOINTS}")
    sk = np.ascontiguousarray(np.asarray(skeleton, np.int32).reshape(-1, 2))
    L = len(sk)
    if L and (sk.min() < 0 or sk.max() >= K):
        raise ValueError(f"skeleton links name keypoints outside 0..{K - 1}")
    lc = np.ascontiguousarray(np.asarray(link_colors, np.uint8).reshape(L, 3))
    kc = np.ascontiguousarray(np.asarray(keypoint_colors, np.uint8).reshape(K, 3))
    per = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * n_all  # noqa: E731
    bbox_of, thr_of = [bool(v) for v in per(draw_bbox)], [float(v) for v in per(kpt_thr)]
    if len(bbox_of) != n_all or len(thr_of) != n_all:
        raise ValueError("draw_bbox / kpt_thr: one value, or one per picture")
    pics = [_gather_picture(im, ds, K, bb, draw_heatmap, device) for im, ds, bb in zip(images, data_samples, bbox_of)]
    if any(p.maps is not None for p in pics) and K > PAREA_MAX_KEYPOINTS:
        raise ValueError(f"{K} keypoints: the probability areas have {PAREA_MAX_KEYPOINTS} colours")
    hm_hw = {tuple(p.maps.shape[2:]) for p in pics if p.maps is not None}
    if len(hm_hw) > 1:
        raise ValueError(f"the maps of one call share their shape, got {sorted(hm_hw)}")
    hm_h, hm_w = hm_hw.pop() if hm_hw else (0, 0)
    shapes = [(p.H, p.W) for p in pics]
    if out is not None:
        out = list(out)
        if len(out) != n_all:
            raise ValueError(f"{len(out)} outputs for {n_all} pictures")
        out = [_output(o, ((2 * p.H if p.maps is not None else p.H), p.W, 3), device) for o, p in zip(out, pics)]
    results = [None] * n_all
    staging = staging if staging is not None else BatchStaging()
    stream = _stream(device)
    # kpt_thr is one value per call: pictures are planned in runs of one value (a run is a whole batch unless the caller varies it)
    lo = 0
    while lo < n_all:
        hi = lo + 1
        while hi < n_all and thr_of[hi] == thr_of[lo]:
            hi += 1
        for chunk in plan_render_chunks(shapes[lo:hi], [p.pad if p.maps is not None else None for p in pics[lo:hi]], K, int(scratch_bytes)):
            mine = [pics[lo + j] for j in chunk["pictures"]]
            n, m = len(mine), sum(p.n for p in mine)
            first_of = {}  # a host array given for several pictures (the instances of one image) is uploaded once
            owner = [first_of.setdefault(p.key, j) for j, p in enumerate(mine)]
            blk = StagedBlock([("pictures", 72 * n), ("instances", 608 * max(m, 1)), ("tiles", 4 * len(chunk["tiles"])), ("skeleton", 8 * max(L, 1)),
                               ("link_rgb", 3 * max(L, 1)), ("kpt_rgb", 3 * K)],
                              [("image", [p.H * p.W * 3 if (p.host_image is not None and owner[j] == j) else 0 for j, p in enumerate(mine)])])
            sizes = [(2 * p.H if p.maps is not None else p.H) * p.W * 3 for p in mine]
            if out is None:
                o_at = np.concatenate([[0], np.cumsum([_align(s) for s in sizes])])
                obuf = torch.empty(int(o_at[-1]), dtype=torch.uint8, device=device)
                outs = [obuf[int(o_at[j]):int(o_at[j]) + sizes[j]].view(-1, mine[j].W, 3) for j in range(n)]
            else:
                outs = [out[lo + j] for j in chunk["pictures"]]
            need = chunk["scratch_bytes"]
            scr = scratch if (scratch is not None and scratch.numel() >= need) else (torch.empty(need, dtype=torch.uint8, device=device) if need else None)
            blk.acquire(staging, device)
            rows, inst = blk.host("pictures", _PICTURE), blk.host("instances", _INSTANCE)
            inst[:] = 0
            blk.host("tiles", np.int32)[:] = chunk["tiles"]
            if L:
                blk.host("skeleton", np.int32)[:] = sk.reshape(-1)
                blk.host("link_rgb")[:] = lc.reshape(-1)
            blk.host("kpt_rgb")[:] = kc.reshape(-1)
            first, img_ptrs, img_hosts = 0, blk.ptrs("image"), blk.hosts("image")
            for j, p in enumerate(mine):
                if p.host_image is not None and owner[j] == j:
                    img_hosts[j][:] = p.host_image.reshape(-1)
                heat = p.maps is not None
                rows[j] = (img_ptrs[owner[j]] if p.host_image is not None else p.image.data_ptr(), outs[j].data_ptr(), int(chunk["scratch_offset"][j]),
                           p.H, p.W, int(channel_order == "bgr"), int(heat), tuple(int(v) for v in p.pad) if heat else (0, 0, 0, 0),
                           int(chunk["canvas"][j][0]), int(chunk["canvas"][j][1]), first, p.n)
                r = inst[first:first + p.n]
                if p.n:
                    r["keypoints"][:, :2 * K] = p.kpts.reshape(p.n, 2 * K)
                    r["visible"][:, :K] = p.vis
                    if p.boxes is not None:
                        r["box"], r["box_valid"] = p.boxes, p.box_ok
                    if heat:
                        r["maps"] = [p.maps.data_ptr() + 4 * i * K * hm_h * hm_w for i in range(p.n)]
                        r["inverse"] = p.inv.reshape(p.n, 6)
                        r["presence"][:, :K] = p.presence
                        if p.rects is not None:
                            r["rect"], r["rect_valid"] = p.rects, p.rect_ok
                first += p.n
            blk.upload()
            batch_uploads += 1
            host = blk.pinned.ctypes.data
            _lib.call("pp_render_samples_batch", host + blk.offset["pictures"], host + blk.offset["instances"] if m else None,
                      host + blk.offset["tiles"], blk.ptr("pictures"), blk.ptr("instances") if m else None, blk.ptr("tiles"), n, m, K, hm_h, hm_w,
                      blk.ptr("skeleton") if L else None, blk.ptr("link_rgb") if L else None, blk.ptr("kpt_rgb"), L, thr_of[lo], float(radius),
                      float(thickness), float(alpha), _lib.ptr(scr), int(scr.numel()) if scr is not None else 0, stream)
            batch_calls += 1
            for j, o in zip(chunk["pictures"], outs):
                results[lo + j] = o
        lo = hi
    return results


class PoseLocalVisualizer:
    """mmpose/visualization/local_visualizer.py:PoseLocalVisualizer for what ProbPose's demo draws: predictions in the
    "mmpose" skeleton style, their boxes, and (``draw_heatmap``) the probability areas of the posterior maps on the padded
    canvas, stacked under the pose panel. Everything is drawn on the GPU; ``add_datasample`` copies the image back once."""

    def __init__(self, name="visualizer", radius=3, line_width=1, alpha=0.8, device="cuda:0", image_encoder="host", png_encoder="host", png_match="runs",
                 jpeg_optimize=False, png_code="host", jpeg_restart_rows=0):
        if image_encoder not in ("host", "device"):
            raise ValueError(f"image_encoder must be 'host' or 'device', got {image_encoder!r}")
        if png_encoder not in ("host", "device"):
            raise ValueError(f"png_encoder must be 'host' or 'device', got {png_encoder!r}")
        if png_match not in ("runs", "lz"):
            raise ValueError(f"png_match must be 'runs' or 'lz', got {png_match!r}")
        if png_code not in ("host", "device"):
            raise ValueError(f"png_code must be 'host' or 'device', got {png_code!r}")
        self.image_encoder = image_encoder  # "device": a .jpg / .jpeg out_file is written by jpeg.imwrite_device
        self.png_encoder = png_encoder  # "device": a .png out_file is written by png.imwrite_device
        self.jpeg_optimize = bool(jpeg_optimize)  # that writer's optimize=: the picture's own Huffman tables (the same pixels, a smaller file)
        if isinstance(jpeg_restart_rows, bool) or not isinstance(jpeg_restart_rows, (int, np.integer)) or not 0 <= int(jpeg_restart_rows) <= 65535:
            raise ValueError(f"jpeg_restart_rows must be an int in 0..65535, got {jpeg_restart_rows!r}")
        self.jpeg_restart_rows = int(jpeg_restart_rows)  # that writer's restart_rows=: a restart marker every so many MCU rows (0: none; the same pixels)
        self.png_match = png_match  # the match mode of that writer: "runs", or "lz" (pixel and row distances: smaller files of drawn frames)
        self.png_code = png_code  # where that writer builds its Huffman codes: "host" (a round trip between its halves), or "device" (one launch more)
        self.name = name
        self.radius = radius
        self.line_width = line_width
        self.alpha = alpha
        self.device = _check_device(device)
        self.skeleton, self.link_color, self.kpt_color = COCO_SKELETON, COCO_LINK_COLORS, COCO_KEYPOINT_COLORS
        self._image = None

    def set_dataset_meta(self, dataset_meta, skeleton_style="mmpose"):
        """Skeleton, link colours and keypoint colours from ``dataset_meta`` (keys ``skeleton_links``,
        ``skeleton_link_colors``, ``keypoint_colors``); the COCO ones where a key is absent."""
        if skeleton_style != "mmpose":
            raise NotImplementedError(f"skeleton_style={skeleton_style!r}: only the 'mmpose' style is drawn (ProbPose's demo uses it)")
        meta = dataset_meta or {}
        self.dataset_meta = meta
        self.skeleton = meta.get("skeleton_links", COCO_SKELETON)
        self.link_color = meta.get("skeleton_link_colors", COCO_LINK_COLORS)
        self.kpt_color = meta.get("keypoint_colors", COCO_KEYPOINT_COLORS)

    def get_image(self):
        return self._image

    def draw_instance_heatmap(self, posterior, image_rgb, image_pad, boxes=None, draw_type="p_area"):
        """_draw_instance_heatmap (:480-585) for the reference's probability-area drawing; returns the (Hp, Wp, 3) device
        panel."""
        if draw_type in ("featmap", "contours"):
            raise NotImplementedError(f"draw_type={draw_type!r}: only ProbPose's 'p_area' drawing is implemented")
        if draw_type != "p_area":
            raise ValueError(f"unknown draw_type {draw_type!r}")
        return render_probability_areas(posterior, image_rgb, image_pad, boxes)

    def draw_datasample(self, image, data_sample, draw_bbox=True, draw_heatmap=False, kpt_thr=0.3):
        """The drawing half of ``add_datasample``: the predictions of one merged sample drawn on ``image`` ((H, W, 3) uint8
        RGB, host array or device tensor), returned as the (H, W, 3) - with ``draw_heatmap`` and heatmaps in ``pred_fields``
        (2H, W, 3) - uint8 RGB DEVICE tensor. No host copy, no file: a video loop hands it to ``jpeg.encode_batch``."""
        from .structures import _image_padding, posterior_heatmaps

        img = _as_device_image(image, self.device)
        H, W = img.shape[:2]
        pi = data_sample.pred_instances if "pred_instances" in data_sample else None
        with_heatmap = bool(draw_heatmap) and pi is not None and "pred_fields" in data_sample and "heatmaps" in data_sample.pred_fields
        out = torch.empty((2 * H if with_heatmap else H, W, 3), dtype=torch.uint8, device=self.device)
        top = out[:H]
        if pi is not None and "keypoints" in pi:
            kpts = pi.get("transformed_keypoints", pi.keypoints)
            vis = pi.keypoints_visible if "keypoints_visible" in pi else np.ones(np.asarray(kpts).shape[:-1], np.float32)
            boxes = pi.bboxes if draw_bbox and "bboxes" in pi else None
            draw_poses(img, kpts, vis, boxes, self.skeleton, self.link_color, self.kpt_color, kpt_thr, self.radius, self.line_width,
                       self.alpha, out=top)
        else:
            top.copy_(img)
        if with_heatmap:
            if "keypoints_probs" not in pi:
                raise ValueError("draw_heatmap needs pred_instances.keypoints_probs (the presence probabilities of ProbPose)")
            meta = data_sample.metainfo
            pad = meta.get("image_pad")
            if pad is None:
                pad = _image_padding(np.asarray(meta["input_center"]).reshape(-1, 2), np.asarray(meta["input_scale"]).reshape(-1, 2),
                                     meta["ori_shape"])
            posterior = posterior_heatmaps(data_sample.pred_fields.heatmaps, pi.keypoints_probs, device=self.device)
            boxes = None
            if draw_bbox:
                src = data_sample.gt_instances if "gt_instances" in data_sample and "bboxes" in data_sample.gt_instances else pi
                boxes = src.bboxes if "bboxes" in src else None
            panel = render_probability_areas(posterior, img, pad, boxes)
            resize_rgb(panel, (H, W), out=out[H:])
        return out

    def draw_datasamples(self, images, data_samples, draw_bbox=True, draw_heatmap=False, kpt_thr=0.3, channel_order="rgb",
                         scratch_bytes=RENDER_SCRATCH_DEFAULT, **kw):
        """``draw_datasample`` for a batch in one set of launches per chunk (``visualization.draw_datasamples`` with this
        visualizer's skeleton, colours, radius, line width and alpha): a list of device tensors, each byte for byte what
        ``draw_datasample`` gives for its sample. The samples carry the un-reverted (n, K, h, w) maps of their instances."""
        return draw_datasamples(images, data_samples, draw_bbox=draw_bbox, draw_heatmap=draw_heatmap, kpt_thr=kpt_thr,
                                channel_order=channel_order, scratch_bytes=scratch_bytes, skeleton=self.skeleton,
                                link_colors=self.link_color, keypoint_colors=self.kpt_color, radius=self.radius, thickness=self.line_width,
                                alpha=self.alpha, device=self.device, **kw)

    def add_datasample(self, name, image, data_sample, draw_gt=False, draw_bbox=True, draw_heatmap=False, kpt_thr=0.3,
                       out_file=None, show_kpt_idx=False, skeleton_style="mmpose", show=False, wait_time=0, step=0):
        """Draw the predictions of one merged sample on ``image`` ((H, W, 3) uint8 RGB, host array or device tensor). Returns
        the (H, W, 3) pose panel, or with ``draw_heatmap`` (and heatmaps in ``pred_fields``) the (2H, W, 3) stack of the pose
        panel over the probability areas resized to (H, W) (:796-865); ``out_file`` is written with Pillow - or, for a visualizer
        built with ``image_encoder="device"`` and a ``.jpg`` / ``.jpeg`` name, by the split JPEG encoder from the frame on the
        device (Pillow's default quality 75 and 4:2:0: a file that decodes to the same pixels; ``jpeg_optimize=True``: with the
        Huffman tables of Pillow's ``optimize=True``, the same pixels again in fewer bytes); with ``png_encoder="device"`` a
        ``.png`` name is written by the device PNG writer (``png.imwrite_device`` in the visualizer's ``png_match`` mode, its codes
        built where ``png_code`` says: the same pixels, other bytes than Pillow's).
        ``draw_datasample`` plus the copy to the host and the file."""
        if draw_gt:
            raise NotImplementedError("draw_gt: ground-truth drawing is outside ProbPose's demo")
        if show_kpt_idx:
            raise NotImplementedError("show_kpt_idx: keypoint index text is not drawn")
        if skeleton_style != "mmpose":
            raise NotImplementedError(f"skeleton_style={skeleton_style!r}: only the 'mmpose' style is drawn")
        if show:
            raise NotImplementedError("show: no window system; use out_file or get_image()")
        out = self.draw_datasample(image, data_sample, draw_bbox=draw_bbox, draw_heatmap=draw_heatmap, kpt_thr=kpt_thr)
        self._image = out.cpu().numpy()
        if out_file is not None:
            if self.image_encoder == "device" and str(out_file).lower().endswith((".jpg", ".jpeg")):
                from . import jpeg

                jpeg.imwrite_device(out_file, out, quality=75, subsampling="4:2:0", channel_order="rgb", optimize=self.jpeg_optimize,
                                    restart_rows=self.jpeg_restart_rows)
            elif self.png_encoder == "device" and str(out_file).lower().endswith(".png"):
                from . import png

                png.imwrite_device(out_file, out, channel_order="rgb", match=self.png_match, code=self.png_code)
            else:
                from PIL import Image

                Image.fromarray(self._image).save(out_file)
        return self._image


__all__ = ["PoseLocalVisualizer", "probability_area_thresholds", "render_probability_areas", "draw_poses", "resize_rgb", "aspect_boxes",
           "int_boxes", "draw_datasamples", "plan_render_chunks", "render_share_bytes", "COCO_SKELETON", "COCO_LINK_COLORS", "COCO_KEYPOINT_COLORS", "PAREA_MAX_KEYPOINTS"]
