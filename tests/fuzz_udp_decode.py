#!/usr/bin/env python
"""Differential fuzz of pp_udp_heatmap_decode against tests/udp_ref.py.

Every case: random B (1 - 512), K (1 - 28), map size (8 x 6 up to 12 288 pixels, odd sizes included), blur kernel size, row-major or
phase-separated input, with or without the flipped pass and the one-pixel shift. Checked per case:
  * ``locs`` and ``scores`` equal numpy's argmax / max of the fp32 averaged map bit for bit; the averaged map itself bit for bit;
  * keypoints within the error bound of udp_ref.decode_f64 (heatmap pixels, scaled to input pixels) of the fp64 decode, for EVERY value
    class: blobs, two near-equal peaks, exact ties, flat maps (the pseudo-inverse's rad == 0 path), non-positive maps (the read of the
    neighbouring map) and noise. A keypoint is left out of the coordinate comparison only where the fp64 Hessian's condition number is
    >= 100 (its maximum and score are still compared); on the blob classes at most 1 % may be left out (``run`` returns the counts per
    class, the test asserts the cap). No class is excluded as a whole: the noise class (amplitude <= noise) has steps of many pixels
    and ill-conditioned Hessians more often, but where the condition number is < 100 the bound - which grows with ``||H^+||`` and the
    step length - holds there too;
  * canaries in front of and behind every output buffer intact, inputs unchanged, a second launch bit-identical.
python tests/fuzz_udp_decode.py [seconds]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import udp_ref as R  # noqa: E402
from probpose_code_amd import _lib  # noqa: E402

GUARD = 64  # canary elements either side of an output


def to_phased(x: np.ndarray) -> np.ndarray:
    """(..., H, W) row-major -> the phase-separated layout of pp_deconv_head: blocks (y & 1, x & 1), each (H/2, W/2) row-major."""
    return np.ascontiguousarray(np.stack([x[..., py::2, px::2] for py in range(2) for px in range(2)], axis=-3)).reshape(x.shape)


class Guarded:
    """An output buffer between two canary runs."""

    def __init__(self, shape, dtype, dev):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.raw = torch.full((self.n + 2 * GUARD,), -777.0, dtype=dtype, device=dev)

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD * self.raw.element_size()

    def get(self):
        r = self.raw.cpu().numpy()
        assert (r[:GUARD] == -777.0).all() and (r[GUARD + self.n:] == -777.0).all(), "canary overwritten"
        return r[GUARD:GUARD + self.n].reshape(self.shape).copy()


def launch(a, b, flip_indices, ks, input_size, phased=False, shift=False, want_avg=True, dev="cuda"):
    """a, b: (B, K, H, W) fp32 numpy in the layout given (b None: no flipped pass) -> dict of numpy results; canaries and inputs
    checked."""
    B, K, H, W = a.shape
    ta = torch.from_numpy(a).to(dev)
    tb = torch.from_numpy(b).to(dev) if b is not None else None
    fi = torch.tensor(list(flip_indices), dtype=torch.int32, device=dev) if b is not None else None
    outs = dict(avg=Guarded((B, K, H, W), torch.float32, dev) if want_avg else None, locs=Guarded((B, K, 2), torch.float32, dev),
                keypoints=Guarded((B, K, 2), torch.float64, dev), scores=Guarded((B, K), torch.float32, dev))
    flags = (2 if phased else 0) | (4 if shift else 0)
    _lib.call("pp_udp_heatmap_decode", ta.data_ptr(), _lib.ptr(tb), _lib.ptr(fi), B, K, H, W, float(input_size[0]), float(input_size[1]),
              int(ks), outs["avg"].ptr if want_avg else None, outs["locs"].ptr, outs["keypoints"].ptr, outs["scores"].ptr, flags,
              _lib.stream_ptr(torch.device(dev)))
    torch.cuda.synchronize()
    res = {k: v.get() for k, v in outs.items() if v is not None}
    assert np.array_equal(ta.cpu().numpy(), a, equal_nan=True) and (b is None or np.array_equal(tb.cpu().numpy(), b, equal_nan=True)), "input changed"
    return res


def check_case(maps, maps_flip, flip_indices, ks, input_size, classes, phased=False, shift=False, stats=None):
    """maps / maps_flip: (B, K, H, W) row-major fp32; classes: (B, K) value-class names. Raises AssertionError on a mismatch;
    ``stats`` collects per class [compared, left out, worst error / bound]."""
    B, K, H, W = maps.shape
    a = to_phased(maps) if phased else maps
    b = None if maps_flip is None else (to_phased(maps_flip) if phased else maps_flip)
    res = launch(a, b, flip_indices, ks, input_size, phased, shift)
    again = launch(a, b, flip_indices, ks, input_size, phased, shift)
    for k_ in res:
        assert np.array_equal(res[k_], again[k_], equal_nan=True), f"{k_}: a second launch differs"
    avg = maps if maps_flip is None else R.flip_average(maps, maps_flip, flip_indices, shift)
    assert np.array_equal(res["avg"], avg), "averaged maps differ from numpy"
    scale = np.asarray(input_size, np.float64) / [W - 1, H - 1]
    for i in range(B):
        ref = R.decode_f64(avg[i], ks, input_size)
        assert np.array_equal(res["locs"][i], ref["locs"]), f"sample {i}: locs {res['locs'][i].tolist()} != {ref['locs'].tolist()}"
        assert np.array_equal(res["scores"][i], ref["scores"]), f"sample {i}: scores differ"
        assert np.isfinite(res["keypoints"][i]).all(), f"sample {i}: non-finite keypoints from finite maps"
        err = np.abs(res["keypoints"][i] - ref["keypoints"]) / scale  # heatmap pixels
        # the reference rounds loc - step to fp32 before it rescales: the fp64 form's result is rounded the same way (decode_f64), the
        # rounding itself is part of the bound
        for k in range(K):
            cls = str(classes[i][k])
            st = stats.setdefault(cls, [0, 0, 0.0]) if stats is not None else [0, 0, 0.0]
            if not ref["cond"][k] < 100:
                st[1] += 1
                continue
            st[0] += 1
            e, bd = float(err[k].max()), float(ref["bound"][k])
            st[2] = max(st[2], e / bd if bd > 0 else (0.0 if e == 0 else np.inf))
            assert e <= bd, (f"sample {i} keypoint {k} ({cls}, {H}x{W}, ks {ks}, phased {phased}, flip {maps_flip is not None}, shift {shift}): "
                             f"|gpu - fp64| = {e:.3e} heatmap px > bound {bd:.3e} (cond {ref['cond'][k]:.1f}, step {ref['step'][k].tolist()})")


def random_case(rng, max_maps=4096):
    """One random case; sizes drawn so that small and large maps, batches and keypoint counts all occur."""
    while True:
        H, W = int(rng.integers(6, 129)), int(rng.integers(6, 129))
        if rng.random() < 0.4:
            H, W = [(64, 48), (96, 72), (8, 6), (128, 96), (33, 27)][int(rng.integers(0, 5))]
        if H * W <= 12288:
            break
    ks = int(rng.choice([11, 17, 11, 3, 19, 1, 7]))
    if ((W + ks) * H + (H + ks - 1) * W + 64) * 4 > 160 * 1024 - 256:  # (the kernel holds 256 bytes statically: UDP_STATIC_LDS)
        ks = 11
    K = int(rng.integers(1, 29))
    budget = max(1, min(max_maps, (1 << 21) // (H * W)))
    B = max(1, min(512, int(rng.choice([1, 2, 8, 64, 512, rng.integers(1, 513)])), budget // K))
    phased = bool(H % 2 == 0 and W % 2 == 0 and rng.random() < 0.5)
    flip = bool(rng.random() < 0.6)
    shift = bool(flip and rng.random() < 0.4)
    classes = rng.choice(R.ALL_CLASSES, (B, K), p=[0.3, 0.15, 0.2, 0.07, 0.05, 0.1, 0.06, 0.07])
    maps = np.empty((B, K, H, W), np.float32)
    for cls in R.ALL_CLASSES:
        sel = classes == cls
        if sel.any():
            maps[sel] = R.make_maps(cls, int(sel.sum()), H, W, rng)
    perm = rng.permutation(K)  # (any permutation: the kernel only looks the flipped pass's channel up)
    flip_indices = perm.tolist()
    maps_flip = None
    if flip:
        # the flipped pass of the same scene: the mirrored, channel-permuted maps plus a little noise, so that the average keeps the
        # value class (a map of a noise class stays one); the average itself is checked bit for bit
        inv = np.argsort(flip_indices)
        back = maps[:, inv]
        if shift:  # (the decode moves the flipped-back map one pixel to the right)
            back = np.concatenate([back[..., 1:], back[..., -1:]], axis=-1)
        back = back[..., ::-1]
        maps_flip = (back + (rng.normal(0, 1e-3, back.shape) * (back != 0)).astype(np.float32)).astype(np.float32)
        for cls in ("flat", "ties", "nonpositive"):  # keep exact ties / signs: the same values again
            sel = (classes == cls)[:, inv]
            maps_flip[sel] = back[sel]
    return dict(maps=maps, maps_flip=maps_flip, flip_indices=flip_indices, ks=ks, input_size=(4 * W, 4 * H), classes=classes, phased=phased,
                shift=shift)


def run(seconds: float = 4.0, seed: int = 0, min_cases: int = 12):
    stats, n, t_end = {}, 0, time.time() + seconds
    while time.time() < t_end or n < min_cases:
        rng = np.random.default_rng(77000 + 1000 * seed + n)
        check_case(stats=stats, **random_case(rng))
        n += 1
    return n, stats


if __name__ == "__main__":
    n, stats = run(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0)
    for cls, (cmp_, out, worst) in sorted(stats.items()):
        print(f"{cls:12s} compared {cmp_:7d}  left out (cond >= 100) {out:6d} = {100.0 * out / max(1, cmp_ + out):.2f} %  worst error / bound {worst:.3f}")
    print(f"{n} cases; UDP DECODE FUZZ OK")
