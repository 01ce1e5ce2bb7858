"""The cases the JPEG layout and size tests share: Pillow-encoded sources (made on the spot from make_golden_jpeg.content, each
encoded and parsed once), the layouts tests/jpeg_write.py transcodes them into, the streams the split decoder must refuse, and
the image sizes that reach the index ranges of csrc/pp_jpeg.hip the committed 48 x 64 grid cannot. Pillow is the encoder here
and nothing else; who judges the pixels is up to the test."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import jpeg_ref as J  # noqa: E402
import jpeg_write as JW  # noqa: E402
from make_golden_jpeg import content, encode  # noqa: E402

# name -> (H, W, sampling, quality, content class, restart interval Pillow writes)
SOURCES = {
    "33x17_420": (33, 17, "420", 75, "noise", 0),
    "37x29_444": (37, 29, "444", 95, "smooth", 0),
    "31x50_422": (31, 50, "422", 30, "noise", 3),
    "48x64_grey": (48, 64, "grey", 75, "bilevel", 0),
    "120x300_420": (120, 300, "420", 90, "smooth", 1),
    "8x1037_422": (8, 1037, "422", 75, "noise", 0),
    "9x1037_420": (9, 1037, "420", 75, "noise", 0),  # 65 MCUs in a row, two block rows of luma
    "480x640_420": (480, 640, "420", 75, "smooth", 0),  # the two workload-sized images
    "333x500_422": (333, 500, "422", 90, "smooth", 0),
}
LAYOUT_SOURCES = ["33x17_420", "37x29_444", "31x50_422", "48x64_grey", "120x300_420", "8x1037_422"]
SMALL_SOURCES = ["33x17_420", "37x29_444", "31x50_422", "48x64_grey", "9x1037_420"]  # at most 48 x 64, plus 9 x 1037

# the must-decode layouts: name -> knobs of jpeg_write.write
LAYOUTS = {
    "plain": dict(),
    "ri7_dht_split": dict(restart=7, dht_split=True),  # 7 divides no MCU row of the sources
    "ri65535": dict(restart=65535),  # above every MCU count: a DRI segment and no restart marker
    "fibonacci": dict(huffman="fibonacci"),
    "fibonacci_shared_ri5_fill2": dict(huffman="fibonacci", dc_slots=(1, 1, 1), ac_slots=(1, 1, 1), restart=5, fill=2),
    "shared_pair_slots_2_3": dict(dc_slots=(2, 2, 2), ac_slots=(3, 3, 3), q_slots=(2, 0, 0)),
    "slots_3_2_split": dict(dc_slots=(3, 2, 2), ac_slots=(2, 3, 3), q_slots=(3, 2, 2), dqt_split=True, dht_split=True),
    "pq1_sof1": dict(pq=1, sof=0xC1, q_slots=(1, 3, 3)),
    "pq1_sof0_split": dict(pq=1, sof=0xC0, dqt_split=True, restart=2),
    "ids_rgb_with_jfif": dict(comp_ids=(ord("R"), ord("G"), ord("B")), jfif=True),  # JFIF says YCbCr whatever the ids
    "ids_odd_no_jfif_fill3_ri1": dict(comp_ids=(0, 200, 7), jfif=False, fill=3, restart=1),
    "segments_adobe1": dict(extra=("com", "app1", "app2"), jfif=False, adobe=1, restart=3, dht_split=True),
}
assert len(LAYOUTS) == 12

# streams outside the subset: name -> (knobs, luma sampling to re-lay the blocks under or None, the word its reason must hold)
REFUSED = {
    "three_scans": (dict(scans="separate"), None, "scans"),
    "sampling_1x2": (dict(), (1, 2), "sampling"),
    "sampling_4x1": (dict(), (4, 1), "sampling"),
    "adobe_transform_0": (dict(jfif=False, adobe=0), None, "Adobe"),
    "ids_rgb_no_jfif": (dict(comp_ids=(ord("R"), ord("G"), ord("B")), jfif=False), None, "RGB"),
}
REFUSED_SOURCE = "37x29_444"  # 4 x 5 blocks a component: enough for one 4x1 and two 1x2 MCUs

# H x W beyond the grid: the second and third workgroup column of jpeg_color_kernel (256 pixels each) with a tail of one pixel
# (257), a full last thread (260) and three pixels (515); 65 MCUs in a row / column and tens of jpeg_idct_kernel workgroups
SIZES = [(5, 257), (6, 260), (3, 515), (9, 1037), (1037, 9)]
SAMPLINGS = ["420", "422", "444", "grey"]

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def encoded(H, W, sampling, quality, kind, restart) -> bytes:
    """Pillow's file of a deterministic image (cached; do not modify)."""
    def make():
        rng = np.random.default_rng([H, W, quality, restart, SAMPLINGS.index(sampling)])
        return encode(content(kind, H, W, 1 if sampling == "grey" else 3, rng), sampling, quality, restart)

    return _once(("jpg", H, W, sampling, quality, kind, restart), make)


def source(name: str) -> bytes:
    return encoded(*SOURCES[name])


def source_parsed(name: str) -> dict:
    """jpeg_ref.parse of a source, computed once and shared (do not modify)."""
    return _once(("parsed", name), lambda: J.parse(source(name)))


def transcoded(name: str, layout: str) -> bytes:
    return _once(("layout", name, layout), lambda: JW.write(source_parsed(name), **LAYOUTS[layout]))


def transcoded_parsed(name: str, layout: str) -> dict:
    """jpeg_ref.parse of a transcoded file, computed once and shared (do not modify)."""
    return _once(("layout parsed", name, layout), lambda: J.parse(transcoded(name, layout)))


def layout_cases():
    """(source, layout) of the fixed list: every layout over the six sources, the two workload-sized sources once each."""
    return [(s, l) for s in LAYOUT_SOURCES for l in LAYOUTS] + [("480x640_420", "ri7_dht_split"), ("333x500_422", "slots_3_2_split")]


def refused(name: str):
    """(file bytes, the word the reason must hold) of a stream outside the subset."""
    knobs, samp, word = REFUSED[name]
    parsed = source_parsed(REFUSED_SOURCE)
    if samp:
        parsed = JW.relayout(parsed, *samp)
    return _once(("refused", name), lambda: JW.write(parsed, **knobs)), word


def size_case(H: int, W: int, sampling: str) -> bytes:
    """The file of one size case: quality, content and restart interval rotate over the cases."""
    i = SIZES.index((H, W)) * 4 + SAMPLINGS.index(sampling)
    return encoded(H, W, sampling, [75, 95, 30, 100, 1][i % 5], ["noise", "smooth", "bilevel"][i % 3], [0, 1, 3, 0][(i // 3) % 4])
