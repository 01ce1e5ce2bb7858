"""CPU: the host side of the batched drawing (visualization.plan_render_chunks: scratch offsets, chunk cut, tile prefixes),
the picture names of --show-dir (runner.show_file_names), the argument checks of pp_render_samples_batch - which run
before any HIP call - and the flag in tools/test.py --help."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 1), (5, 255), (7, 256), (33, 257), (64, 48), (120, 90)]
PADS = [[0, 0, 0, 0], None, [3, 0, 0, 9], [0, 12, 300, 0], None, [10, 10, 10, 10]]


def test_share_bytes_restate_the_library(lib_built):
    from probpose_code_amd import _lib
    from probpose_code_amd import visualization as V

    for K, h, w in ((1, 1, 1), (3, 2, 2), (17, 64, 48), (17, 128, 128), (17, 129, 127), (22, 1216, 2047), (17, 480 + 75, 640 + 90)):
        assert V.render_share_bytes(K, h, w) == _lib.lib.pp_render_batch_scratch_bytes(K, h, w), (K, h, w)
        assert V.render_share_bytes(K, h, w) % 256 == 0 and V.render_share_bytes(K, h, w) > K * h * w * 4 + h * w * 3
    assert _lib.lib.pp_render_batch_scratch_bytes(23, 4, 4) == _lib.PP_ERR_INVALID_ARG
    assert _lib.lib.pp_render_batch_scratch_bytes(17, 0, 4) == _lib.PP_ERR_INVALID_ARG
    assert _lib.lib.pp_render_batch_scratch_bytes(17, 65536, 4) == _lib.PP_ERR_UNSUPPORTED
    assert _lib.lib.pp_render_batch_scratch_bytes(1, 32768, 16384) == _lib.PP_ERR_UNSUPPORTED  # 2^29 values


def _check_chunk(chunk, shapes, pads, K):
    from probpose_code_amd import visualization as V

    idx, n = chunk["pictures"], len(chunk["pictures"])
    spans = []
    for j, i in enumerate(idx):
        H, W = shapes[i]
        if pads[i] is None:
            assert tuple(chunk["canvas"][j]) == (H, W) and chunk["scratch_offset"][j] == 0
            continue
        p = pads[i]
        hp, wp = H + p[1] + p[3], W + p[0] + p[2]
        assert tuple(chunk["canvas"][j]) == (hp, wp)
        o = int(chunk["scratch_offset"][j])
        assert o % 256 == 0
        spans.append((o, o + V.render_share_bytes(K, hp, wp)))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "shares overlap"
    assert chunk["scratch_bytes"] == (spans[-1][1] if spans else 0) and (not spans or spans[0][0] == 0)
    t = chunk["tiles"]
    assert t.dtype == np.int32 and len(t) == 2 * (n + 1) and t[0] == 0 and t[n + 1] == 0
    canvas_tiles = [chunk["canvas"][j][0] * -(-chunk["canvas"][j][1] // 256) if pads[i] is not None else 0 for j, i in enumerate(idx)]
    image_tiles = [shapes[i][0] * -(-shapes[i][1] // 256) for i in idx]
    assert list(np.diff(t[:n + 1])) == canvas_tiles and list(np.diff(t[n + 1:])) == image_tiles
    assert t[n] == sum(canvas_tiles) and t[-1] == sum(image_tiles)  # the prefixes end in the grid sizes


def test_plan_render_chunks_offsets_tiles_and_cuts():
    from probpose_code_amd import visualization as V

    K = 17
    share = [V.render_share_bytes(K, h + p[1] + p[3], w + p[0] + p[2]) if p is not None else 0 for (h, w), p in zip(SHAPES, PADS)]
    everything = V.plan_render_chunks(SHAPES, PADS, K)  # the default budget: one chunk
    assert [c["pictures"] for c in everything] == [[0, 1, 2, 3, 4, 5]]
    _check_chunk(everything[0], SHAPES, PADS, K)
    assert everything[0]["scratch_bytes"] == sum(share)
    # (7, 256) + pad -> 259 columns: two row tiles per row; (33, 257) + 300 columns of pad: three
    assert everything[0]["tiles"][3] - everything[0]["tiles"][2] == 16 * 2 and everything[0]["tiles"][4] - everything[0]["tiles"][3] == 45 * 3
    alone = V.plan_render_chunks(SHAPES, PADS, K, budget=1)  # every picture above the budget: each panel picture closes a chunk
    assert [c["pictures"] for c in alone] == [[0, 1], [2], [3, 4], [5]]
    for c in alone:
        _check_chunk(c, SHAPES, PADS, K)
        assert sum(p is not None for p in (PADS[i] for i in c["pictures"])) == 1
    some = V.plan_render_chunks(SHAPES, PADS, K, budget=share[0] + share[2])  # exactly the first two panel pictures fit
    assert [c["pictures"] for c in some][0] == [0, 1, 2] and len(some) >= 2
    assert sorted(i for c in some for i in c["pictures"]) == list(range(6))
    for c in some:
        _check_chunk(c, SHAPES, PADS, K)
        assert c["scratch_bytes"] <= share[0] + share[2] or len([i for i in c["pictures"] if PADS[i] is not None]) == 1
    big_first = V.plan_render_chunks([(120, 90), (1, 1)], [[10, 10, 10, 10], [0, 0, 0, 0]], K, budget=share[0])  # a picture above the budget stands alone
    assert [c["pictures"] for c in big_first] == [[0], [1]]
    none = V.plan_render_chunks(SHAPES, [None] * 6, K, budget=0)  # no panel: no scratch, one chunk whatever the budget
    assert len(none) == 1 and none[0]["scratch_bytes"] == 0 and none[0]["tiles"][6] == 0
    with pytest.raises(ValueError):
        V.plan_render_chunks(SHAPES, PADS[:5], K)
    with pytest.raises(ValueError):
        V.plan_render_chunks([(4, 4)], [[0, -1, 0, 0]], K)


def test_show_file_names_follow_the_reference_rule():
    from probpose_code_amd.runner import show_file_names

    assert show_file_names(["d/a.jpg", "d/a.jpg", "d/b.png", "d/a.jpg"], []) == ["a_0.jpg", "a_1.jpg", "b_0.png", "a_2.jpg"]
    assert show_file_names(["d/a.jpg", "e/b.jpg"], ["a_0.jpg", "a_1.jpg", "notes.txt"]) == ["a_2.jpg", "b_0.jpg"]  # files on disk shift the index
    # the reference counts every name that STARTS WITH the stem (visualization_hook.py:155): a1 also counts a12's pictures
    assert show_file_names(["a12.jpg", "a1.jpg", "a12.jpg", "a1.jpg"], []) == ["a12_0.jpg", "a1_1.jpg", "a12_1.jpg", "a1_3.jpg"]
    assert show_file_names(["x/000000001000.tar.png"], ["000000001000.tar_0.png"]) == ["000000001000.tar_1.png"]  # cut at the last dot
    first = show_file_names(["p/a.jpg"] * 2, [])
    assert show_file_names(["p/a.jpg"], first) == ["a_2.jpg"]  # a later batch of the run: the names given out count
    with pytest.raises(ValueError):
        show_file_names(["no_suffix"], [])


def _tables(n_pictures=1, heatmap=0, count=0, K=17):
    from probpose_code_amd import visualization as V

    img = np.zeros((4, 4, 3), np.uint8)
    out = np.zeros((8, 4, 3), np.uint8)
    pics = np.zeros(max(n_pictures, 1), V._PICTURE)
    inst = np.zeros(max(count, 1), V._INSTANCE)
    for p in pics:
        p["image"], p["out"], p["height"], p["width"], p["heatmap"], p["canvas_h"], p["canvas_w"], p["count"] = \
            img.ctypes.data, out.ctypes.data, 4, 4, heatmap, 4, 4, count
    tiles = np.array([0, 4 * heatmap, 0, 4], np.int32)
    return pics, inst, tiles, (img, out)


def _call(pics, inst, tiles, n, m, K, scratch=None, scratch_bytes=0, null_tables=False):
    from probpose_code_amd import _lib

    colours = np.zeros(3 * 32, np.uint8)
    a = None if null_tables else pics.ctypes.data
    return _lib.lib.pp_render_samples_batch(a, inst.ctypes.data, tiles.ctypes.data, a, inst.ctypes.data, tiles.ctypes.data, n, m, K, 64, 48,
                                            None, None, colours.ctypes.data, 0, 0.3, 3.0, 1.0, 0.8, scratch, scratch_bytes, None)


def test_batch_entry_refuses_before_any_launch(lib_built):
    """NULL tables, K = 23, zero pictures, a heatmap picture without instances: refused with nothing launched. (The tables
    are host memory here: a call that passed the checks would launch, so only refusals are made.)"""
    from probpose_code_amd import _lib

    _lib.reset_launch_counts()
    pics, inst, tiles, keep = _tables()
    assert _call(pics, inst, tiles, 1, 0, 17, null_tables=True) == _lib.PP_ERR_INVALID_ARG
    assert b"NULL" in _lib.lib.pp_last_error()
    assert _call(pics, inst, tiles, 0, 0, 17) == _lib.PP_ERR_INVALID_ARG  # zero pictures
    assert _call(pics, inst, tiles, -1, 0, 17) == _lib.PP_ERR_INVALID_ARG
    assert _call(pics, inst, tiles, 1, 0, 0) == _lib.PP_ERR_INVALID_ARG
    assert _call(pics, inst, tiles, 1, 0, 33) == _lib.PP_ERR_INVALID_ARG  # above the revert's 32 channels, even without a panel
    scratch = np.zeros(1 << 20, np.uint8)
    pics, inst, tiles, keep = _tables(heatmap=1, count=1, K=23)
    inst["maps"] = scratch.ctypes.data
    assert _call(pics, inst, tiles, 1, 1, 23, scratch.ctypes.data, scratch.size) in (_lib.PP_ERR_INVALID_ARG, _lib.PP_ERR_UNSUPPORTED)
    assert b"22" in _lib.lib.pp_last_error()
    pics, inst, tiles, keep = _tables(heatmap=1, count=0)
    assert _call(pics, inst, tiles, 1, 0, 17, scratch.ctypes.data, scratch.size) == _lib.PP_ERR_INVALID_ARG
    assert b"without instances" in _lib.lib.pp_last_error()
    pics, inst, tiles, keep = _tables(heatmap=1, count=1)
    inst["maps"] = scratch.ctypes.data
    assert _call(pics, inst, tiles, 1, 1, 17, scratch.ctypes.data, 1024) == _lib.PP_ERR_WORKSPACE  # the share does not fit
    pics["canvas_h"] = 5  # not the image plus its padding
    assert _call(pics, inst, tiles, 1, 1, 17, scratch.ctypes.data, scratch.size) == _lib.PP_ERR_INVALID_ARG
    pics, inst, tiles, keep = _tables()
    pics["count"] = 256
    assert _call(pics, np.zeros(256, inst.dtype), tiles, 1, 256, 17) == _lib.PP_ERR_UNSUPPORTED
    pics, inst, tiles, keep = _tables()
    pics["height"] = 65536
    assert _call(pics, inst, tiles, 1, 0, 17) == _lib.PP_ERR_UNSUPPORTED
    pics, inst, tiles, keep = _tables()
    tiles[3] = 5  # a prefix that is not the table's
    assert _call(pics, inst, tiles, 1, 0, 17) == _lib.PP_ERR_INVALID_ARG
    assert _lib.launch_count("pp_render_batch.hip") == 0


def test_cli_help_names_show_dir():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--show-dir" in r.stdout
