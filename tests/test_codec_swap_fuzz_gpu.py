"""GPU: the fixed case table of tests/fuzz_codec_swap.py on pp_argmax_probmap_decode and pp_expmax_heatmap_decode - every shape class the
argument checks admit, against the fp64 Sparsemax / fp64 DARK decode under their derived bounds (argmax) and the oracle bit for bit (expmax);
what is checked per case, and why no tolerance is new, is in that module's docstring. tests/test_codec_swap_references.py shows on the CPU
that the table reaches what it claims and that the checkers reject single faults."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_codec_swap as F  # noqa: E402

pytestmark = pytest.mark.gpu

# (kind, the table's groups, part, of parts): a few seconds each
ARGMAX_GROUPS = [("argmax", ("small",), 0, 2), ("argmax", ("small",), 1, 2), ("argmax", ("production",), 0, 3), ("argmax", ("production",), 1, 3),
                 ("argmax", ("production",), 2, 3), ("argmax", ("long",), 0, 1), ("argmax", ("poison", "refused"), 0, 1)]
EXPMAX_GROUPS = [("expmax", ("dense",), 0, 2), ("expmax", ("dense",), 1, 2), ("expmax", ("sparse",), 0, 1), ("expmax", ("poison", "refused"), 0, 1)]


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("needs the MI355X")


@functools.lru_cache(maxsize=None)
def _run(kind, groups, part, parts):
    cases = [c for c in (F.argmax_table() if kind == "argmax" else F.expmax_table()) if c["group"] in groups][part::parts]
    stats = F.new_stats()
    for case in cases:
        F.run_case(case, stats)
    return len(cases), stats


@pytest.mark.parametrize("kind,groups,part,parts", ARGMAX_GROUPS + EXPMAX_GROUPS, ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_table_group(kind, groups, part, parts):
    n, stats = _run(kind, groups, part, parts)
    print(F.report(stats, f"{kind} {'+'.join(groups)} {part + 1}/{parts}: {n} cases"))
    assert n > 0


def test_blob_keypoints_left_out_stay_under_the_cap():
    """cond >= 100 leaves at most 2 % of the blob class out, over the whole table, with at least 2 000 blob keypoints compared."""
    stats = F.new_stats()
    for g in ARGMAX_GROUPS:
        F.merge_stats(stats, _run(*g)[1])
    print(F.report(stats, "argmax, the whole table"))
    compared, left_out, share = F.blob_cap(stats)
    assert compared >= F.BLOB_MIN and share <= F.BLOB_CAP, (compared, left_out, share)
    # every case the restated checks say both launches of the chain admit was compared with it (no silent skip)
    expected = sum(F.chain_expected(c) for c in F.argmax_table())
    assert stats["#cases compared with the chain"] == expected >= 80, (stats["#cases compared with the chain"], expected)  # (91 in this table: H, W >= 9, no poison)
    # normalize None: avg_out is the reference's bits, so the keypoints left out are the reference's, to the count (the blob_clamped
    # class has no cap - tests/test_codec_swap_references.py shows the reference alone exceeds it - but it has this)
    ref = F.new_stats()
    for c in F.argmax_table():
        if c["refused"] is None and c["normalize"] is None:
            F.check_argmax(c, F.reference_outputs(c), ref)
    key = "#left out under normalize None"
    assert stats[key] == ref[key] > 0, (stats[key], ref[key])


def test_udp_decode_at_the_lds_edge_the_argmax_table_found():
    """The chain's second launch has the LDS check the fused launch had (tests/fuzz_codec_swap.py, the LDS rule): the largest H at W = 4 and kernel
    size 19 decodes within udp_ref's bound, the next one is refused with nothing written."""
    H, W, ks = F.UDP_TOP_H, 4, 19
    rng = np.random.default_rng(940000)
    maps = F.R.make_maps("blob", 2, H, W, rng).reshape(1, 2, H, W)
    out = F.launch_udp(maps, ks)
    assert out["status"] == F.OK, out
    ref = F.R.decode_f64(maps[0], ks, (4 * W, 4 * H))
    assert np.array_equal(out["locs"][0], ref["locs"]) and np.array_equal(out["scores"][0], ref["scores"])
    err = (np.abs(out["keypoints"][0] - ref["keypoints"]) / (np.asarray([4.0 * W, 4.0 * H]) / [W - 1, H - 1])).max(-1)
    ok = ref["cond"] < 100
    print(f"error / bound {np.max(err[ok] / ref['bound'][ok]) if ok.any() else 0:.3f}, compared {int(ok.sum())} of 2")
    assert (err[ok] <= ref["bound"][ok]).all(), (err, ref["bound"])
    refused = F.launch_udp(np.zeros((1, 1, H + 1, W), np.float32), ks)
    assert refused["status"] == F.UNSUPPORTED and "LDS" in refused["error"] and refused["untouched"], refused
