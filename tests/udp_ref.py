"""The UDP heatmap decode with DARK refinement (the ViTPose baseline's codec), restated twice in numpy for the tests:

* ``decode_f32``: step by step in the dtypes the reference computes in (fp32 maps, blur, rescale, clip, log and seven-point
  differences; fp64 from ``H + eps * I`` on; the refined location rounded to fp32). With its default arguments it equals the
  reference's own functions bit for bit on tests/golden/udp_decode_cases.npz (tests/test_udp_references.py). Its keyword
  arguments switch single FAULTS on - the emulations the error bound has to reject.
* ``decode_f64``: the same arithmetic in fp64 from the (fp32) averaged map on, with, per keypoint, what the error bound
  needs: the Hessian's condition number, ``||H^+||``, the step, and the bound itself.

The blur is a plain zero-padded separable Gaussian: the reference pads the map by (ks - 1) / 2 zeros before it calls
cv2.GaussianBlur and cuts the centre out afterwards, so cv2's own border mode never reaches the kept region. cv2 is NOT
installed where the fixture was made: the order of the fp32 sums below (taps ascending, rows first, one rounding per
operator) is this project's choice, not pinned against cv2 (tests/golden/make_golden_udp.py says what to re-run).

Error bound (``decode_f64(...)["bound"]``, heatmap pixels per coordinate, u = 2^-24):
  blur      two passes of ks products and sums in fp32: |d blur_i| <= g * blur(|map|)_i, g = 2 (ks + 2) u
            (the fp32 taps are the definition in both forms, so they add nothing);
  rescale   ratio = origin_max / (max(blur) + 1e-12): relative error e_b = g * max(blur(|map|)) / |max(blur) + 1e-12| + 2 u,
            v_i = blur_i * ratio: |d v_i| <= |ratio| |d blur_i| + |v_i| (e_b + 2 u);
  log       L_i = log(clip(v_i, 1e-3, 50)) is 1 / v-Lipschitz inside the clip and constant outside:
            e_i = |d v_i| / max(v_i - |d v_i|, 1e-3) + 3 u |L_i| + u  (log's own rounding, two ulp allowed to the device's logf);
  stencil   with E = max e_i and Lm = max |L_i| over the seven points: |d dx|, |d dy| <= E + 2 u Lm;
            |d dxx|, |d dyy|, |d dxy| <= 4 E + 8 u Lm (their fp32 partial sums), so ||dg|| <= sqrt(2) (E + 2 u Lm) and
            ||dH|| <= ||dH||_F <= 2 (4 E + 8 u Lm);
  solve     s = H^+ g: ||ds|| <= ||H^+|| (||dg|| + ||dH|| ||s||) / (1 - ||H^+|| ||dH||)   (first order in dH; where
            ||H^+|| ||dH|| > 1/2 - a Hessian that is eps * I because every point is clipped - the factor stays 2: both
            forms then have g = 0 and s = 0 exactly);
  result    the fp32 rounding of loc - s: u * max(|x|, |y|) * 2; the fp64 closed form against LAPACK: 1e-12 * cond.
A keypoint is comparable when the fp64 Hessian's condition number is < 100 (``decode_f64(...)["cond"]``).
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
EPS32 = float(np.finfo(np.float32).eps)


def gaussian_taps(ks: int, sigma_ks: int = None) -> np.ndarray:
    """cv2.getGaussianKernel(ks, sigma <= 0) as cv2.GaussianBlur uses it: sigma from the kernel size, factors normalised in double,
    rounded to fp32. ``sigma_ks``: FAULT - the sigma of another kernel size."""
    s_ks = ks if sigma_ks is None else sigma_ks
    sigma = 0.3 * ((s_ks - 1) * 0.5 - 1.0) + 0.8
    r = (ks - 1) // 2
    e = [float(np.exp(-0.5 * float(j - r) * float(j - r) / (sigma * sigma))) for j in range(ks)]
    total = 0.0
    for v in e:
        total += v
    return np.array([v / total for v in e], np.float64).astype(F32)


def blur(maps: np.ndarray, ks: int, dtype=F32, border: str = "zero", sigma_ks: int = None) -> np.ndarray:
    """(..., H, W) maps -> separable Gaussian blur, rows first, taps ascending, one rounding per operator in ``dtype``."""
    taps = gaussian_taps(ks, sigma_ks).astype(dtype)
    r = (ks - 1) // 2
    m = np.asarray(maps, dtype)
    H, W = m.shape[-2:]
    lead = [(0, 0)] * (m.ndim - 2)
    mode = dict(mode="constant") if border == "zero" else dict(mode="reflect")  # "reflect" = cv2.BORDER_REFLECT_101 (the FAULT)
    p = np.pad(m, lead + [(0, 0), (r, r)], **mode) if r else m
    h = np.zeros(m.shape, dtype)
    for j in range(ks):
        h = h + taps[j] * p[..., :, j:j + W]
    p = np.pad(h, lead + [(r, r), (0, 0)], **mode) if r else h
    v = np.zeros(m.shape, dtype)
    for j in range(ks):
        v = v + taps[j] * p[..., j:j + H, :]
    return v


def flip_average(a: np.ndarray, b: np.ndarray, flip_indices, shift: bool = False) -> np.ndarray:
    """(a + flip_back(b)) * 0.5 in fp32 on (B, K, H, W) maps: channels permuted, columns reversed, with ``shift`` moved one pixel
    to the right (column 0 keeps its value)."""
    f = np.asarray(b, F32)[:, list(flip_indices)][..., ::-1]
    if shift:
        f = np.concatenate([f[..., :1], f[..., :-1]], axis=-1)
    return ((np.asarray(a, F32) + f) * F32(0.5)).astype(F32)


def _maximum(hm, last_tie=False):
    K, H, W = hm.shape
    flat = hm.reshape(K, -1)
    idx = flat.argmax(1)
    if last_tie:  # FAULT: the last index of equal maxima
        idx = flat.shape[1] - 1 - flat[:, ::-1].argmax(1)
    vals = flat[np.arange(K), idx]
    locs = np.stack([idx % W, idx // W], -1).astype(F32)
    return locs, vals


def _log_maps(hm, vals, ks, dtype, border="zero", rescale=True, sigma_ks=None, clip_lo=1e-3):
    """Blur, rescale to the original maximum, clip, log, edge-pad by one: (K, H + 2, W + 2) in ``dtype``."""
    b = blur(hm, ks, dtype, border, sigma_ks)
    if rescale:
        with np.errstate(all="ignore"):
            ratio = vals.astype(dtype) / (b.reshape(b.shape[0], -1).max(1) + dtype(1e-12))
        b = b * ratio[:, None, None]
    b = np.log(np.clip(b, dtype(clip_lo), dtype(50.0)))
    return np.pad(b, ((0, 0), (1, 1), (1, 1)), mode="edge")


def _seven_points(logs, locs):
    """The reference's flat index into the padded log maps of one sample: for loc = (-1, -1) three of the points lie in the map
    before (Python's negative index: the last map for k = 0)."""
    K, Hp, Wp = logs.shape
    flat = logs.reshape(-1)
    base = (locs[:, 0].astype(np.int64) + 1) + (locs[:, 1].astype(np.int64) + 1) * Wp + Hp * Wp * np.arange(K)
    offs = dict(c=0, xp=1, yp=Wp, xpyp=Wp + 1, xmym=-Wp - 1, xm=-1, ym=-Wp)
    return {n: flat[base + o] for n, o in offs.items()}, {n: (base + o) % flat.size for n, o in offs.items()}


def newton_step_f32(p, dxy_half=True, eps_identity=True):
    """The seven fp32 points {c, xp, yp, xpyp, xmym, xm, ym} (arrays of K) -> the step H^+ g (K, 2) f64: derivative and Hessian in
    fp32, ``H + eps32 * I`` and everything behind it in fp64."""
    K = p["c"].shape[0]
    half = F32(0.5)
    dx = half * (p["xp"] - p["xm"])
    dy = half * (p["yp"] - p["ym"])
    dxx = p["xp"] - F32(2) * p["c"] + p["xm"]
    dyy = p["yp"] - F32(2) * p["c"] + p["ym"]
    dxy = (half if dxy_half else F32(1)) * (p["xpyp"] - p["xp"] - p["yp"] + p["c"] + p["c"] - p["xm"] - p["ym"] + p["xmym"])
    deriv = np.stack([dx, dy], 1).reshape(K, 2, 1)
    hess = np.stack([dxx, dxy, dxy, dyy], 1).reshape(K, 2, 2)
    hinv = np.linalg.pinv(hess + (np.finfo(np.float32).eps if eps_identity else 0.0) * np.eye(2))
    return np.einsum("imn,ink->imk", hinv, deriv).squeeze(-1)


def decode_f32(hm: np.ndarray, ks: int, input_size, border="zero", rescale=True, sigma_ks=None, clip_lo=1e-3, dxy_half=True,
               eps_identity=True, argmax_on_blur=False, last_tie=False):
    """One sample's (K, H, W) fp32 maps -> keypoints (1, K, 2) f64 in input pixels, scores (1, K) f32, locs (K, 2) f32 (integer
    maximum, (-1, -1) where the maximum is <= 0), refined (K, 2) f32 (heatmap pixels). Defaults = the reference; every keyword
    is one FAULT."""
    hm = np.ascontiguousarray(hm, F32)
    K, H, W = hm.shape
    locs, vals = _maximum(hm, last_tie)
    if argmax_on_blur:  # FAULT: the location of the blurred map's maximum
        locs, _ = _maximum(blur(hm, ks, F32), last_tie)
    locs[vals <= 0] = -1
    logs = _log_maps(hm, vals, ks, F32, border, rescale, sigma_ks, clip_lo)
    p, _ = _seven_points(logs, locs)
    step = newton_step_f32(p, dxy_half, eps_identity)
    refined = locs.copy()[None]
    refined[0] -= step
    keypoints = refined / [W - 1, H - 1] * np.asarray(input_size)
    return keypoints, vals[None].copy(), locs, refined[0]


def decode_f64(hm: np.ndarray, ks: int, input_size):
    """The same decode in fp64 from the fp32 maps on (maximum and score are the fp32 map's own). Returns a dict of per-keypoint
    arrays: keypoints (K, 2) input pixels, refined (K, 2) heatmap pixels, locs, scores, cond, pinv_norm, step (K, 2), bound (K,)
    heatmap pixels (module docstring)."""
    hm = np.ascontiguousarray(hm, F32)
    K, H, W = hm.shape
    D = np.float64
    locs, vals = _maximum(hm)
    locs[vals <= 0] = -1
    hm64 = hm.astype(D)
    logs = _log_maps(hm64, vals.astype(D), ks, D)
    p, where = _seven_points(logs, locs)
    dx = 0.5 * (p["xp"] - p["xm"])
    dy = 0.5 * (p["yp"] - p["ym"])
    dxx = p["xp"] - 2 * p["c"] + p["xm"]
    dyy = p["yp"] - 2 * p["c"] + p["ym"]
    dxy = 0.5 * (p["xpyp"] - p["xp"] - p["yp"] + p["c"] + p["c"] - p["xm"] - p["ym"] + p["xmym"])
    g = np.stack([dx, dy], 1)
    hess = np.stack([dxx, dxy, dxy, dyy], 1).reshape(K, 2, 2) + EPS32 * np.eye(2)
    sv = np.linalg.svd(hess, compute_uv=False)
    with np.errstate(all="ignore"):
        cond = sv[:, 0] / sv[:, 1]
    hinv = np.linalg.pinv(hess)
    pinv_norm = np.linalg.norm(hinv, 2, axis=(1, 2))
    step = np.einsum("imn,in->im", hinv, g)
    refined = locs.astype(D) - step
    # ---- the bound
    gam = 2 * (ks + 2) * U
    b = blur(hm64, ks, D)
    babs = blur(np.abs(hm64), ks, D)
    bmax = b.reshape(K, -1).max(1)
    with np.errstate(all="ignore"):
        ratio = vals.astype(D) / (bmax + 1e-12)
        e_b = gam * babs.reshape(K, -1).max(1) / np.abs(bmax + 1e-12) + 2 * U
    bp = np.pad(b * ratio[:, None, None], ((0, 0), (1, 1), (1, 1)), mode="edge").reshape(-1)
    dbp = np.pad(np.abs(ratio)[:, None, None] * gam * babs, ((0, 0), (1, 1), (1, 1)), mode="edge").reshape(-1)
    ebp = np.repeat(e_b, (H + 2) * (W + 2))
    lflat = logs.reshape(-1)
    E = np.zeros(K)
    Lm = np.zeros(K)
    for n, idx in where.items():
        v = bp[idx]
        dv = dbp[idx] + np.abs(v) * (ebp[idx] + 2 * U)
        with np.errstate(all="ignore"):
            e = dv / np.maximum(v - dv, 1e-3) + 3 * U * np.abs(lflat[idx]) + U
        e = np.where((v + dv < 1e-3) | (v - dv > 50.0), 0.0, e)  # clipped in both forms: the same constant
        E = np.maximum(E, np.where(np.isfinite(e), e, np.inf))
        Lm = np.maximum(Lm, np.abs(lflat[idx]))
    dg = np.sqrt(2.0) * (E + 2 * U * Lm)
    dH = 2 * (4 * E + 8 * U * Lm)
    with np.errstate(all="ignore"):
        amp = pinv_norm * dH
        factor = np.where(amp <= 0.5, 1.0 / (1.0 - np.minimum(amp, 0.5)), 2.0)
        bound = pinv_norm * (dg + dH * np.linalg.norm(step, axis=1)) * factor
        bound = bound + 2 * U * np.abs(refined).max(1) + 1e-12 * np.where(np.isfinite(cond), cond, 0.0)
    keypoints = refined.astype(F32).astype(D) / [W - 1, H - 1] * np.asarray(input_size)
    return dict(keypoints=keypoints, refined=refined, locs=locs, scores=vals, cond=cond, pinv_norm=pinv_norm, step=step, bound=bound)


# ---- value classes shared by the CPU reference tests and the GPU fuzzer ---------------------------------------------------
BLOB_CLASSES = ("blob", "blob_noisy", "blob_border")  # the classes the 1 % cap on left-out keypoints applies to
OTHER_CLASSES = ("noise", "flat", "nonpositive", "ties", "two_peaks")  # compared like the blobs (condition number < 100), without a cap on the share left out
ALL_CLASSES = BLOB_CLASSES + OTHER_CLASSES


def make_maps(cls: str, n: int, H: int, W: int, rng) -> np.ndarray:
    """``n`` fp32 maps (n, H, W) of one value class. Blob classes: a Gaussian of sigma 2, amplitude 0.5 - 1, noise sigma <= 0.02,
    centre inside the map ("blob", "blob_noisy") or anywhere from two pixels outside it ("blob_border")."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)

    def blobs(cx, cy, amp, sig=2.0):
        return amp[:, None, None] * np.exp(-((xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2) / (2 * sig * sig))

    amp = rng.uniform(0.5, 1.0, n)
    if cls in ("blob", "blob_noisy"):
        m = blobs(rng.uniform(1, W - 2, n), rng.uniform(1, H - 2, n), amp)
        m = m + rng.normal(0, 0.002 if cls == "blob" else 0.02, m.shape)
    elif cls == "blob_border":
        side = rng.integers(0, 4, n)
        cx, cy = rng.uniform(-2, W + 1, n), rng.uniform(-2, H + 1, n)
        cx = np.where(side == 0, rng.uniform(-2, 1, n), np.where(side == 1, rng.uniform(W - 2, W + 1, n), cx))
        cy = np.where(side == 2, rng.uniform(-2, 1, n), np.where(side == 3, rng.uniform(H - 2, H + 1, n), cy))
        m = blobs(cx, cy, amp) + rng.normal(0, 0.01, (n, H, W))
    elif cls == "noise":
        m = rng.normal(0, 0.05, (n, H, W)) + blobs(rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n), rng.uniform(0, 0.05, n))
    elif cls == "flat":
        m = np.broadcast_to(rng.uniform(0.01, 1.0, n)[:, None, None], (n, H, W)).copy()
    elif cls == "nonpositive":
        m = -np.abs(rng.normal(0, 0.1, (n, H, W)))
        m[rng.random(n) < 0.3] = 0.0
        m[rng.random(n) < 0.3] = -0.1
    elif cls == "ties":
        m = np.round(rng.random((n, H, W)) * 4) / 4
    elif cls == "two_peaks":
        cx, cy = rng.uniform(2, W - 3, n), rng.uniform(2, H - 3, n)
        m = blobs(cx, cy, amp) + blobs(W - 1 - cx, H - 1 - cy, amp * (1 + rng.choice([-1e-6, 0.0, 1e-6], n)))
    else:
        raise ValueError(cls)
    return m.astype(F32)
