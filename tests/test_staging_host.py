"""CPU: the arithmetic of ``staging.StagedBlock`` (no pinned buffer, no device): offsets are the running 256-aligned sums
of the reservations in their order, regions do not overlap, the total is the aligned end, a head upload ends where the
named region begins. This half loads staging.py alone, so it needs no built library. Then the four upload blocks of
``probpose_code_amd.jpeg`` for a batch of two images (8x8 at 4:4:4 and 17x33 at 4:2:0), staged in host memory through a
stand-in for the pinned buffer: every offset the builder gives equals the offset of the formulas these blocks were laid
out by before there was a builder, restated here literally. The geometry comes from ``jpeg.encode_plan`` (the library, no
GPU)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_staging_alone", os.path.join(ROOT, "probpose_code_amd", "staging.py"))
staging = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(staging)
StagedBlock = staging.StagedBlock


def _align(v, a=256):  # (restated: the tests do not take the rounding from the code under test)
    return (v + a - 1) // a * a


# (name, bytes): a zero-length and a 1-byte region among them
RESERVATIONS = [("desc", 128), ("empty", 0), ("one", 1), ("tables", 384), ("exact", 256), ("coef", 1000), ("tail", 257)]
OFFSETS = {"desc": 0, "empty": 256, "one": 256, "tables": 512, "exact": 1024, "coef": 1280, "tail": 2304}
TOTAL = 2816


def test_offsets_are_running_aligned_sums():
    blk = StagedBlock(RESERVATIONS)
    assert blk.offset == OFFSETS and blk.total == TOTAL
    at = 0
    for name, nbytes in RESERVATIONS:
        assert blk.offset[name] == at and at % 256 == 0 and blk.nbytes[name] == nbytes
        at = _align(at + nbytes)
    assert blk.total == at == _align(blk.offset["tail"] + 257)
    assert StagedBlock([]).total == 0


def test_per_image_regions_follow_the_head_image_by_image():
    blk = StagedBlock([("desc", 100)], [("a", [0, 300]), ("b", [1, 256])])
    assert blk.offset == {"desc": 0} and blk.offsets == {"a": [256, 512], "b": [256, 1024]} and blk.total == 1280
    assert blk.sizes["a"] == [0, 300] and blk.head_bytes("a") == 256 and blk.head_bytes("b") == 256


def test_regions_do_not_overlap_and_stay_inside_the_block():
    blk = StagedBlock(RESERVATIONS)
    spans = sorted((blk.offset[name], blk.offset[name] + nbytes) for name, nbytes in RESERVATIONS if nbytes)
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert end <= start
    assert spans[-1][1] <= blk.total


def test_head_upload_ends_where_the_named_region_begins():
    blk = StagedBlock(RESERVATIONS)
    assert blk.head_bytes() == TOTAL
    assert blk.head_bytes("coef") == OFFSETS["coef"] == 1280
    assert blk.head_bytes("desc") == 0 and blk.head_bytes("one") == 256


def test_a_region_is_reserved_once():
    with pytest.raises(ValueError):
        StagedBlock([("a", 1), ("a", 2)])
    with pytest.raises(ValueError):
        StagedBlock([("a", 1)], [("b", [1]), ("b", [2])])


class HostStaging:
    """A stand-in for ``BatchStaging`` in host memory: ``uploaded`` keeps the length of every upload."""

    def __init__(self):
        self.uploaded = []

    def acquire(self, nbytes):
        self.buf = np.zeros(nbytes, np.uint8)
        return self.buf

    def upload(self, dev, nbytes):
        self.uploaded.append(nbytes)


@pytest.fixture(scope="module")
def jpeg(lib_built):
    from probpose_code_amd import jpeg

    return jpeg


@pytest.fixture(scope="module")
def infos(jpeg):
    """The plans of the two images of the batch."""
    got = [jpeg.encode_plan(8, 8, "4:4:4"), jpeg.encode_plan(17, 33, "4:2:0")]
    assert [int(i.coef_count) for i in got] == [3 * 64, (4 * 6 + 2 * 2 * 3) * 64]  # one MCU of three blocks; 2 x 3 MCUs of six blocks
    return got


def _coefficients(jpeg, infos):
    return [jpeg.JpegCoefficients(i, np.zeros(int(i.coef_count), np.int16), jpeg.quality_tables(75)) for i in infos]


def test_reconstruct_layout(jpeg, infos):
    counts, n = [int(i.coef_count) for i in infos], len(infos)
    off, o_qt, o_coef = _align(64 * n), [], []
    for c in counts:
        o_qt.append(off)
        off = _align(off + 384)
        o_coef.append(off)
        off = _align(off + 2 * c)
    stage = HostStaging()
    blk = jpeg._stage(_coefficients(jpeg, infos), "cpu", stage, None, None).block
    assert blk.offset == {"desc": 0} and blk.offsets == {"qtables": o_qt, "coef": o_coef} and blk.total == off and stage.uploaded == [off]
    assert blk.sizes["coef"] == [2 * c for c in counts]


def test_huffman_layout(jpeg, infos):
    import io

    from PIL import Image

    files = []
    for (W, H), ss in (((8, 8), 0), ((17, 33), 2)):
        buf = io.BytesIO()
        Image.fromarray(np.full((H, W, 3), 90, np.uint8)).save(buf, "JPEG", quality=75, subsampling=ss)
        files.append(buf.getvalue())
    scans = [jpeg.scan_prepare(f) for f in files]
    assert [int(s.info.coef_count) for s in scans] == [int(i.coef_count) for i in infos]
    n = len(scans)
    o_res = _align(72 * n)
    o_rec = _align(o_res + 16 * n)
    off, o_tab, o_qt, o_str = _align(o_rec + 64 * n), [], [], []
    for s in scans:
        o_tab.append(off)
        off = _align(off + s.tables.size)
        o_qt.append(off)
        off = _align(off + 384)
        o_str.append(off)
        off = _align(off + max(int(s.stream.size), 1))
    for reconstruct in (False, True):
        stage = HostStaging()
        blk = jpeg._stage_huffman(scans, "cpu", stage, 3, reconstruct).block
        assert blk.offset == {"desc": 0, "results": o_res, "recon": o_rec} and blk.offsets == {"tables": o_tab, "qtables": o_qt, "stream": o_str}
        assert blk.total == off and stage.uploaded == [off]


@pytest.mark.parametrize("entropy", [False, True])
def test_forward_layout(jpeg, entropy):
    """(One call of the encoder has one sampling: both images are planned at 4:2:0 here.)"""
    import torch

    images = [torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((33, 17, 3), dtype=torch.uint8)]
    counts, n = [int(jpeg.encode_plan(8, 8, "4:2:0").coef_count), int(jpeg.encode_plan(17, 33, "4:2:0").coef_count)], 2
    o_qt = _align(64 * n)
    o_ent = _align(o_qt + 384)
    o_res = _align(o_ent + 64 * n) if entropy else o_ent
    off, o_coef = (_align(o_res + 16 * n) if entropy else o_ent), []
    for c in counts:
        o_coef.append(off)
        off = _align(off + 2 * c)
    total, head = off, o_coef[0]
    stage = HostStaging()
    job = jpeg._stage_encode(images, jpeg.quality_tables(75), "4:2:0", "bgr", "cpu", stage, entropy)
    want = {"desc": 0, "qtables": o_qt}
    if entropy:
        want.update(entropy=o_ent, results=o_res)
    assert job.block.offset == want and job.block.offsets == {"coef": o_coef} and job.block.total == total
    assert stage.uploaded == [head] and job.block.head_bytes("coef") == head  # the upload stops in front of the coefficients
    assert (job.entropy is not None) == entropy


def test_entropy_layout(jpeg, infos):
    counts, n = [int(i.coef_count) for i in infos], len(infos)
    o_res = _align(64 * n)
    off, o_coef = _align(o_res + 16 * n), []
    for c in counts:
        o_coef.append(off)
        off = _align(off + 2 * c)
    stage = HostStaging()
    blk = jpeg._stage_entropy(_coefficients(jpeg, infos), "cpu", stage).block
    assert blk.offset == {"desc": 0, "results": o_res} and blk.offsets == {"coef": o_coef} and blk.total == off and stage.uploaded == [off]
