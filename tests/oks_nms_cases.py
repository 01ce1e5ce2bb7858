"""Inputs of the OKS-NMS tests (not collected): a seeded batch of images shaped like a detector's output - clusters of
near-duplicate poses, exact duplicates, tied scores, a NaN keypoint - and every pair's fp64 OKS in numpy, from which the tests
predict which images the device must report undecided."""
import numpy as np

SEED = 20261020
THRESHOLDS = (0.5, 0.7, 0.9)
FIXED_SIZES = (0, 1, 2, 63, 64, 65, 128, 129)  # around the 64-column words of the bit matrix and the 16-row blocks
N_IMAGES = 300
K = 17


def make_image(rng, n, area_dtype=np.float64):
    """(keypoints (n, 17, 3) float64, scores (n,) float64 with ties, areas (n,))."""
    base = rng.uniform(50, 400, (max(n // 4, 1), K, 2))
    kp = np.zeros((n, K, 3))
    for i in range(n):
        kp[i, :, :2] = base[rng.integers(0, len(base))] + rng.normal(0, rng.choice([0.0, 1.0, 3.0, 6.0, 30.0]), (K, 2))
        kp[i, :, 2] = rng.uniform(0, 1, K)
    score = np.round(rng.uniform(0.1, 1.0, n), 2)  # two decimals: ties from a few dozen instances on
    area = rng.uniform(3000, 30000, n).astype(area_dtype)
    return kp, score, area


def make_batch(seed=SEED, area_dtype=np.float64, n_images=N_IMAGES):
    rng = np.random.default_rng(seed)
    sizes = list(FIXED_SIZES) + [int(rng.integers(0, 101)) for _ in range(n_images - len(FIXED_SIZES))]
    images = [make_image(rng, n, area_dtype) for n in sizes]
    images[5][0][3, 4, 0] = np.nan  # one NaN keypoint (65-instance image): its OKS to everything is NaN, which suppresses
    return images


def sorted_arrays(image):
    """The image's arrays in suppression order, and the order (the call oks_nms itself makes)."""
    kp, score, area = image
    order = np.array(score).argsort()[::-1]
    return kp[order], area[order], order


def pair_oks(kp, area, sigmas):
    """fp64 OKS of every pair i < j of one image (arrays in suppression order), as oks_iou forms it: (n, n), NaN elsewhere."""
    n = len(kp)
    var = (np.asarray(sigmas) * 2) ** 2
    d = kp[None, :, :, :2] - kp[:, None, :, :2]
    half = ((area[:, None] + area[None, :]) / 2).astype(np.float64) + np.spacing(1)  # float32 areas: mean in float32
    e = (d[..., 0] ** 2 + d[..., 1] ** 2) / var / half[..., None] / 2
    with np.errstate(invalid="ignore"):
        oks = np.exp(-e).sum(-1) / K
    oks[np.tril_indices(n)] = np.nan
    return oks


def nearest_pair(images, sigmas, midpoint):
    """Per image: the smallest |oks - midpoint| over its pairs (inf without a finite pair)."""
    out = np.full(len(images), np.inf)
    for n, img in enumerate(images):
        kp, area, _ = sorted_arrays(img)
        if len(kp) > 1:
            d = np.abs(pair_oks(kp, area, sigmas) - midpoint)
            if np.isfinite(d).any():
                out[n] = np.nanmin(d)
    return out
