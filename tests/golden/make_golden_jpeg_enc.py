"""Writes tests/golden/jpeg_enc_cases.npz: a few images of the encoder's test grid (tests/jpeg_enc_ref.py) with what Pillow
(bundled libjpeg-turbo) wrote for them - the quantised coefficients and quantisation tables of its file, parsed by
tests/jpeg_ref.parse. Data from Pillow, nothing from the reference project. tests/test_jpeg_enc_references.py holds the
numpy restatement of the compressor to these, so the pin does not depend on the Pillow build of the machine it runs on.

    python tests/golden/make_golden_jpeg_enc.py

The cases: partial MCUs on both axes with dummy luma blocks (17x33 and 7x5 at 4:2:0, 31x15 at 4:2:2), an odd 4:4:4 size,
one pixel, whole MCUs at quality 100 (all-ones tables: the largest coefficients), every content kind, the extreme qualities.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_enc_ref as E  # noqa: E402
import jpeg_ref as J  # noqa: E402

# (content, width, height, subsampling, quality)
CASES = (("noise", 17, 33, "4:2:0", 75), ("checker", 31, 15, "4:2:2", 24), ("gradient", 9, 17, "4:4:4", 95), ("noise", 7, 5, "4:2:0", 1),
         ("noise", 48, 64, "4:2:0", 100), ("flat255", 1, 1, "4:2:0", 50), ("noise", 31, 15, "4:2:2", 75), ("checker", 16, 16, "4:4:4", 100))


def main():
    out = {"cases": np.array(["|".join(str(v) for v in c) for c in CASES])}
    for i, (content, W, H, ss, q) in enumerate(CASES):
        rgb = E.image(content, W, H)
        p = J.parse(E.pillow_bytes(rgb, q, ss))
        assert (p["hs"], p["vs"]) == E.SUBSAMPLING[ss]
        out[f"rgb_{i}"] = rgb
        out[f"coef_{i}"] = J.flat_coefficients(p)
        out[f"qt_{i}"] = p["qtables"]
    path = os.path.join(HERE, "jpeg_enc_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
