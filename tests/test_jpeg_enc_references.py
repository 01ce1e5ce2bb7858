"""CPU: the numpy restatement of the JPEG compressor (tests/jpeg_enc_ref.py) - the arbiter of csrc/pp_jpeg_enc.hip - equals
libjpeg-turbo: for every image of the grid the quantised coefficients, quantisation tables and sampling factors of Pillow's
file (parsed by tests/jpeg_ref.parse) are the restatement's, value for value. Where Pillow is built on another libjpeg
the committed fixtures (tests/golden/jpeg_enc_cases.npz) hold the same pin. Single mistakes a first version makes - no edge
replication, a constant downsampling bias, truncating quantisation, dummy blocks with a zero DC - are shown to fail it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_enc_ref as E  # noqa: E402
import jpeg_ref as J  # noqa: E402

QUALITIES = (1, 24, 50, 75, 95, 100)
FAULTS = ("no_edge_replication", "constant_bias", "truncating_quantisation", "dummy_dc_zero")


def _turbo():
    try:
        from PIL import features

        return bool(features.check_feature("libjpeg_turbo"))
    except Exception:  # noqa: BLE001
        return False


@pytest.mark.skipif(not _turbo(), reason="Pillow is not built on libjpeg-turbo: the committed fixtures hold the pin")
@pytest.mark.parametrize("subsampling", sorted(E.SUBSAMPLING))
@pytest.mark.parametrize("size", E.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_pillow(size, subsampling):
    W, H = size
    for quality in QUALITIES:
        for content in E.CONTENTS:
            rgb = E.image(content, W, H)
            p = J.parse(E.pillow_bytes(rgb, quality, subsampling))
            f = E.forward(rgb, quality, subsampling)
            what = (size, subsampling, quality, content)
            assert (p["width"], p["height"], p["ncomp"], p["hs"], p["vs"]) == (W, H, 3, f["hs"], f["vs"]), what
            assert (p["mcus_x"], p["mcus_y"], p["comp_bw"], p["comp_bh"]) == (f["mcus_x"], f["mcus_y"], f["comp_bw"], f["comp_bh"]), what
            assert np.array_equal(p["qtables"], f["qtables"]), what
            for c in range(3):
                assert p["coef"][c].dtype == f["coef"][c].dtype == np.int16
                assert np.array_equal(p["coef"][c], f["coef"][c]), (what, c, int((p["coef"][c] != f["coef"][c]).sum()))


def _golden():
    z = np.load(os.path.join(HERE, "golden", "jpeg_enc_cases.npz"))
    for i, case in enumerate(str(c) for c in z["cases"]):
        content, W, H, ss, q = case.split("|")
        yield case, z[f"rgb_{i}"], ss, int(q), z[f"coef_{i}"], z[f"qt_{i}"], (content, int(W), int(H))


def test_restatement_equals_the_committed_fixtures():
    n = 0
    for case, rgb, ss, q, coef, qt, (content, W, H) in _golden():
        assert np.array_equal(rgb, E.image(content, W, H)), case  # the grid's content generator has not drifted
        f = E.forward(rgb, q, ss)
        assert np.array_equal(qt, f["qtables"]), case
        assert coef.dtype == np.int16 and np.array_equal(coef, E.flat_coefficients(f)), case
        assert coef.size == f["coef_count"], case
        n += 1
    assert n >= 6


def test_quality_tables():
    assert (E.quality_tables(100) == 1).all()
    assert np.array_equal(E.quality_tables(50)[0], E.STD_LUMA_Q) and np.array_equal(E.quality_tables(50)[2], E.STD_CHROMA_Q)
    t1 = E.quality_tables(1)
    assert t1.max() == 255 and t1.min() == 255  # 50 x the base tables, clamped for baseline files
    for bad in (0, 101, -3):
        with pytest.raises(ValueError):
            E.quality_tables(bad)


@pytest.mark.parametrize("fault", FAULTS)
def test_single_faults_are_rejected(fault):
    """Each mistake changes the coefficients of at least one committed fixture (and the restatement without it matches all)."""
    differs = [case for case, rgb, ss, q, coef, qt, _ in _golden() if not np.array_equal(coef, E.flat_coefficients(E.forward(rgb, q, ss, faults=(fault,))))]
    assert differs, f"no fixture notices {fault}"
