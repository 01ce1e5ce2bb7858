"""numpy restatement of the --draw-heatmap drawing (probpose_code_amd/csrc/pp_render.hip), written from the definitions in
that file's header: the yardstick of tests/test_visualization*.py. Every fp32 formula is copied operation for operation
(float32 arrays, float32 scalars); the kernels are built without fused multiply-adds so the two round alike."""
import numpy as np

f32 = np.float32

# mmpose/visualization/local_visualizer.py:523-547
PAREA_RGB = np.array([
    [230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200], [245, 130, 48], [145, 30, 180], [70, 240, 240], [240, 50, 230],
    [210, 245, 60], [250, 190, 212], [0, 128, 128], [220, 190, 255], [255, 250, 200], [128, 0, 0], [170, 255, 195], [128, 128, 0],
    [255, 215, 180], [255, 255, 255], [170, 110, 40], [0, 0, 128], [128, 128, 128], [0, 0, 0]], np.uint8)


def threshold_fp64(m):
    """(thr, draw) of one map by the contract: fp64 cumsum of the values sorted in descending order, the first index where it
    reaches 0.75 of the total; draw = 0 for a negative / non-finite value or a total below 0.75."""
    x = np.asarray(m, np.float32).ravel()
    if not np.isfinite(x).all() or (x < 0).any():
        return f32(0), 0
    s = np.sort(x)[::-1]
    cs = np.cumsum(s.astype(np.float64))
    total = cs[-1]
    if not total >= 0.75:
        return f32(0), 0
    return f32(s[np.searchsorted(cs, 0.75 * total)]), 1


def threshold_reference_f32(m):
    """The reference's literal form (local_visualizer.py:557-568): float32 sum, sort, cumsum and searchsorted. None when
    the map is skipped."""
    heatmap = np.asarray(m, np.float32)
    prob_thr = 0.75
    if heatmap.sum() < prob_thr:
        return None
    htm_sort = np.sort(heatmap.flatten())[::-1]
    htm_cusum = np.cumsum(htm_sort)
    return htm_sort[np.searchsorted(htm_cusum, prob_thr * htm_cusum[-1])]


def thresholds(maps):
    out = [threshold_fp64(m) for m in maps]
    return np.array([t for t, _ in out], np.float32), np.array([d for _, d in out], np.int32)


def rect_mask(H, W, box):
    """1-px outline of an int box (corners in any order), clipped to the picture."""
    x1, y1, x2, y2 = (int(v) for v in box)
    x1, x2, y1, y2 = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
    Y, X = np.mgrid[0:H, 0:W]
    return (((Y == y1) | (Y == y2)) & (X >= x1) & (X <= x2)) | (((X == x1) | (X == x2)) & (Y >= y1) & (Y <= y2))


def int_boxes(boxes):
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    b = b[np.isfinite(b).all(axis=1)]
    return np.clip(b, -2 ** 30, 2 ** 30).astype(np.int64)


def aspect_boxes(boxes, pad):
    """local_visualizer.py:844-858 (the box arithmetic of fix_bbox_aspect_ratio restated, xyxy)."""
    b = np.array(boxes, np.float32).reshape(-1, 4)
    b[:, :2] += np.asarray(pad)[:2]
    b[:, 2:] += np.asarray(pad)[:2]
    centers = b[:, :2] + (b[:, 2:] - b[:, :2]) / 2
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    nw, nh = w.astype(np.float32), h.astype(np.float32)
    for i in range(len(b)):
        wi = w[i] if w[i] != 0 else 1
        hi = h[i] if h[i] != 0 else 1
        if wi / hi > 3 / 4:
            nh[i] = wi / (3 / 4)
        else:
            nw[i] = hi * (3 / 4)
    nw, nh = nw * 1.25, nh * 1.25
    out = np.array([centers[:, 0] - nw / 2, centers[:, 1] - nh / 2, centers[:, 0] + nw / 2, centers[:, 1] + nh / 2]).T
    return int_boxes(out)


def compose(image, pad, maps, thr, draw, rect_boxes):
    """(b): the padded canvas, the areas and outlines, then the rectangles (already int, canvas coordinates)."""
    K, Hp, Wp = maps.shape
    H, W = image.shape[:2]
    c = np.full((Hp, Wp, 3), 80, np.float32)
    c[pad[1]:pad[1] + H, pad[0]:pad[0] + W] = image
    for k in range(K):
        if not draw[k]:
            continue
        m = maps[k] > thr[k]
        mp = np.pad(m, 1, constant_values=False)
        interior = mp[:-2, 1:-1] & mp[2:, 1:-1] & mp[1:-1, :-2] & mp[1:-1, 2:]
        edge = m & ~interior
        col = PAREA_RGB[k].astype(np.float32)
        blend = np.clip(np.rint(f32(0.7) * col + f32(0.3) * c), 0, 255)
        c = np.where(m[..., None], blend, c)
        c = np.where(edge[..., None], col, c)
    for box in np.asarray(rect_boxes).reshape(-1, 4):
        c[rect_mask(Hp, Wp, box)] = (0, 255, 0)
    return c.astype(np.uint8)


def _seg_dist2(X, Y, ax, ay, bx, by):
    ex, ey = f32(bx - ax), f32(by - ay)
    wx, wy = X - f32(ax), Y - f32(ay)
    L2 = f32(ex * ex + ey * ey)
    t = (wx * ex + wy * ey) / L2 if L2 > 0 else np.zeros_like(X)
    t = np.minimum(np.maximum(t, f32(0)), f32(1))
    dx, dy = wx - t * ex, wy - t * ey
    return dx * dx + dy * dy


def draw_poses(image, keypoints, visible, boxes, skeleton, link_rgb, kpt_rgb, kpt_thr, radius, thickness, alpha):
    """(c): per instance its box (int32 corners or None), links, points."""
    H, W = image.shape[:2]
    c = image.astype(np.float32)
    Y, X = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    h = f32(max(f32(thickness), f32(1)) * f32(0.5))
    h2, r2 = f32(h * h), f32(f32(radius) * f32(radius))
    a, oma = f32(alpha), f32(f32(1) - f32(alpha))
    kp = np.asarray(keypoints, np.float32)
    vi = np.asarray(visible, np.float32)
    for i in range(len(kp)):
        if boxes is not None:
            c[rect_mask(H, W, boxes[i])] = (0, 255, 0)
        for l, (p, q) in enumerate(skeleton):
            pos = [kp[i, p, 0], kp[i, p, 1], kp[i, q, 0], kp[i, q, 1]]
            lims = [W, H, W, H]
            if not all(v >= 1 and v < lim for v, lim in zip(pos, lims)):
                continue
            if not (float(vi[i, p]) >= kpt_thr and float(vi[i, q]) >= kpt_thr):
                continue
            ip = [f32(int(v)) for v in pos]
            on = _seg_dist2(X, Y, *ip) <= h2
            c[on] = np.asarray(link_rgb[l], np.float32)
        for j in range(kp.shape[1]):
            if not float(vi[i, j]) >= kpt_thr:
                continue
            dx, dy = X - kp[i, j, 0], Y - kp[i, j, 1]
            on = dx * dx + dy * dy <= r2
            col = np.asarray(kpt_rgb[j], np.float32)
            c[on] = np.clip(np.rint(a * col + oma * c[on]), 0, 255)
    return c.astype(np.uint8)


def resize(src, H, W):
    """(d): fp32 bilinear, half-pixel centres, edge clamp."""
    Hs, Ws = src.shape[:2]

    def axis(n_out, n_in):
        scale = f32(n_in) / f32(n_out)
        s = np.maximum((np.arange(n_out, dtype=np.float32) + f32(0.5)) * scale - f32(0.5), f32(0))
        i0 = np.floor(s).astype(np.int64)
        fr = s - i0.astype(np.float32)
        clamp = i0 >= n_in - 1
        i0[clamp], fr[clamp] = n_in - 1, 0
        return i0, np.minimum(i0 + 1, n_in - 1), fr

    x0, x1, fx = axis(W, Ws)
    y0, y1, fy = axis(H, Hs)
    p = src.astype(np.float32)
    fx, fy = fx[None, :, None], fy[:, None, None]
    one = f32(1)
    top = (one - fx) * p[y0][:, x0] + fx * p[y0][:, x1]
    bot = (one - fx) * p[y1][:, x0] + fx * p[y1][:, x1]
    return np.clip(np.rint((one - fy) * top + fy * bot), 0, 255).astype(np.uint8)


def render(image, keypoints, visible, pose_boxes, maps, pad, gt_boxes, skeleton, link_rgb, kpt_rgb, kpt_thr=0.3, radius=3,
           thickness=1, alpha=0.8, draw_bbox=True):
    """The whole (2H, W, 3) picture from posterior ``maps`` (already computed)."""
    H, W = image.shape[:2]
    top = draw_poses(image, keypoints, visible, int_boxes(pose_boxes) if draw_bbox else None, skeleton, link_rgb, kpt_rgb,
                     kpt_thr, radius, thickness, alpha)
    thr, draw = thresholds(maps)
    rects = aspect_boxes(gt_boxes, pad) if draw_bbox else np.zeros((0, 4), np.int64)
    return np.concatenate([top, resize(compose(image, pad, maps, thr, draw, rects), H, W)], axis=0)


def posterior_like_maps(K, H, W, seed):
    """Seeded maps shaped like posterior heatmaps: a few anisotropic Gaussian blobs over a faint floor, normalised to sum to a
    presence probability in [0.8, 1)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64)
    out = np.empty((K, H, W), np.float32)
    for k in range(K):
        m = np.full((H, W), 1e-9)
        for _ in range(int(rng.integers(1, 4))):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            sy, sx = rng.uniform(0.01, 0.08) * H, rng.uniform(0.01, 0.08) * W
            m += rng.uniform(0.3, 1.0) * np.exp(-0.5 * ((ys - cy) / sy) ** 2)[:, None] * np.exp(-0.5 * ((xs - cx) / sx) ** 2)[None, :]
        out[k] = m / m.sum() * rng.uniform(0.8, 1.0)
    return out
