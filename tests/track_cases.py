"""Cases of the pose tracker's box rule, shared by tests/test_track_host.py (which asserts what ``tracking.next_boxes_host`` makes of the
crafted ones) and tests/test_track_gpu.py (``pp_track_update`` against ``next_boxes_host`` on all of them, bit for bit). A case is a dict
``records, centers, scales, boxes, alive, lost`` (the arguments of ``next_boxes_host``), ``gate`` and ``params``."""
import numpy as np

INPUT = (192, 256)
OKS_GUARD = 1e-9  # an OKS this close to dup_oks_thr could be decided by the last bits of exp(): no case may come that close


def sigmas(K):
    from probpose_code_amd.evaluation import COCO_SIGMAS

    return np.resize(COCO_SIGMAS, K).astype(np.float64)


def crop_params(boxes):
    from probpose_code_amd import transforms as T

    c, s, _ = T.topdown_affine_params(np.asarray(boxes, np.float32).reshape(-1, 4), INPUT)
    return c, s


def grid_pose(K, ox, oy):
    """(K, 2): keypoint k at (ox + 7 (k mod 5), oy + 11 (k div 5)) - 28 x 33 pixels at K = 17."""
    k = np.arange(K)
    return np.stack([ox + 7.0 * (k % 5), oy + 11.0 * (k // 5)], -1)


def records_of(points, gates, centers, scales):
    """Records (n, K, 7) whose image-space keypoints are ``points`` (n, K, 2) up to rounding, both gate columns ``gates`` (n, K)."""
    points, gates = np.asarray(points, np.float64), np.asarray(gates, np.float64)
    rec = np.zeros(points.shape[:2] + (7,))
    c, s = centers.astype(np.float64)[:, None], scales.astype(np.float64)[:, None]
    rec[..., :2] = (points - c + 0.5 * s) / s * np.asarray(INPUT)
    rec[..., 2] = rec[..., 3] = gates
    return rec


def case(boxes, points, gates, alive=None, lost=None, gate="prob", **params):
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    n = len(boxes)
    centers, scales = crop_params(boxes)
    return dict(records=records_of(points, gates, centers, scales), centers=centers, scales=scales, boxes=boxes,
                alive=np.ones(n, np.int32) if alive is None else np.asarray(alive, np.int32),
                lost=np.zeros(n, np.int32) if lost is None else np.asarray(lost, np.int32), gate=gate, params=params)


def run_host(c, **kw):
    from probpose_code_amd import tracking

    K = c["records"].shape[1]
    return tracking.next_boxes_host(c["records"], c["centers"], c["scales"], INPUT, c["boxes"], c["alive"], c["lost"], sigmas(K), gate=c["gate"],
                                    **dict(c["params"], **kw))


def crafted(K=17):
    """name -> case. K = 1 keeps the structure (min_keypoints is capped at K by the caller's params)."""
    mk = min(4, K)
    full = np.full((1, K), 0.9)
    out = {}
    out["follow"] = case([[40, 30, 90, 100]], grid_pose(K, 53, 40)[None], full, min_keypoints=mk)
    few = np.where(np.arange(K) < mk, 0.9, 0.0)[None]
    out["exactly_min"] = case([[10, 10, 60, 80]], grid_pose(K, 20, 20)[None], few, min_keypoints=mk)
    out["one_short"] = case([[10, 10, 60, 80]], grid_pose(K, 20, 20)[None], np.where(np.arange(K) < mk - 1, 0.9, 0.0)[None], min_keypoints=mk)
    out["last_miss"] = case([[10, 10, 60, 80]], grid_pose(K, 20, 20)[None], np.zeros((1, K)), lost=[2], max_lost=2, min_keypoints=mk)
    out["dead"] = case([[10, 10, 60, 80]], grid_pose(K, 20, 20)[None], full, alive=[0], lost=[3], min_keypoints=mk)
    line = np.stack([np.full(K, 50.0), 10.0 + 2 * np.arange(K)], -1)[None]
    out["collinear"] = case([[0, 0, 100, 100]], line, full, min_keypoints=mk)
    c = case([[0, 0, 100, 100]], line, full, min_keypoints=1)
    r = c["records"]
    if K >= 6:
        r[0, 0, 0], r[0, 1, 1], r[0, 2, 3], r[0, 3, 3], r[0, 4, 0], r[0, 2, 2], r[0, 3, 2] = np.nan, np.inf, np.nan, np.inf, -np.inf, np.nan, np.inf
    else:
        r[0, 0, 0] = np.nan
    out["non_finite"] = c
    out["smooth"] = case([[40, 30, 90, 100]], grid_pose(K, 50, 40)[None], full, smooth=0.5, min_keypoints=mk)
    # the prob column selects, the conf column does not - and the other way round
    c = case([[40, 30, 90, 100]], grid_pose(K, 50, 40)[None], full, min_keypoints=mk)
    c["records"][..., 2] = 0.1
    out["gate_prob"] = c
    c = case([[40, 30, 90, 100]], grid_pose(K, 50, 40)[None], full, gate="conf", min_keypoints=mk)
    c["records"][..., 3] = 0.1
    out["gate_conf"] = c
    c = case([[40, 30, 90, 100]], grid_pose(K, 50, 40)[None], full, gate="conf", min_keypoints=mk)
    c["records"][..., 2] = 0.1
    out["gate_conf_low"] = c
    three = [[40, 30, 90, 100], [38, 28, 92, 102], [200, 30, 260, 100]]
    pts = np.stack([grid_pose(K, 50, 40), grid_pose(K, 50, 40), grid_pose(K, 210, 40)])
    for name, g0, g1 in (("dup_tie", 0.9, 0.9), ("dup_first_lower", 0.6, 0.9), ("dup_second_lower", 0.9, 0.6)):
        out[name] = case(three, pts, np.stack([np.full(K, g0), np.full(K, g1), np.full(K, 0.5)]), min_keypoints=mk)
    return out


def random_case(n, K, seed):
    rng = np.random.default_rng(seed)
    x0, y0 = rng.uniform(-100, 500, n), rng.uniform(-100, 300, n)
    boxes = np.stack([x0, y0, x0 + rng.uniform(1, 300, n), y0 + rng.uniform(1, 300, n)], -1).astype(np.float32)
    if n > 1 and seed % 2 == 0:
        boxes[1] = boxes[0]
    centers, scales = crop_params(boxes)
    rec = rng.uniform(-30, 300, (n, K, 7))
    rec[..., 2:4] = rng.uniform(0, 1, (n, K, 2))
    u = rng.uniform(0, 1, rec.shape)
    rec[u < 0.01], rec[(u >= 0.01) & (u < 0.02)], rec[(u >= 0.02) & (u < 0.03)] = np.nan, np.inf, -np.inf
    alive = (rng.uniform(0, 1, n) < 0.85).astype(np.int32)
    if n > 1 and seed % 2 == 0:  # slot 1 repeats slot 0: a duplicate whenever both are updated
        rec[1], alive[1] = rec[0], alive[0]
    if n > 2:                   # and slot 2 is slot 0 moved by a few pixels: an OKS between 0 and 1
        rec[2, :, :2] = rec[0, :, :2] + rng.uniform(-2, 2, (K, 2))
        boxes[2], centers[2], scales[2] = boxes[0], centers[0], scales[0]
    params = dict(kpt_thr=float(rng.uniform(0.1, 0.6)), min_keypoints=int(rng.integers(1, min(K, 6) + 1)), expand=float(rng.uniform(1.0, 1.5)),
                  min_side=float(rng.uniform(1, 16)), smooth=0.0 if seed % 3 else float(rng.uniform(0, 0.9)), max_lost=int(rng.integers(0, 3)),
                  dup_oks_thr=float(rng.uniform(0.3, 0.95)))
    return dict(records=rec, centers=centers, scales=scales, boxes=boxes, alive=alive, lost=rng.integers(0, 3, n).astype(np.int32),
                gate="prob" if seed % 2 else "conf", params=params)
