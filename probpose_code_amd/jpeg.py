"""Baseline JPEG files decoded in two halves: markers and Huffman codes on host threads (``pp_jpeg_entropy_decode``, plain
C++ behind ctypes - the call releases the GIL), then dequantisation, inverse DCT, chroma upsampling, YCbCr -> BGR and HWC
packing on the device (``pp_jpeg_reconstruct_bgr_batch``: all images of a batch in two launches). The pixels are bit for
bit those of ``apis.load_image_bgr`` (libjpeg-turbo's default decoder); the (H, W, 3) uint8 BGR device tensors are what
``pp_warp_affine_u8_batch`` reads in place.

Accepted: SOF0 / SOF1, 8 bits, Huffman coding, one interleaved scan, grey or YCbCr with 4:4:4 / 4:2:2 / 4:2:0 sampling,
any tables, restart intervals. Every other file - progressive, arithmetic-coded, 12-bit, CMYK, other sampling, several
scans, a damaged stream - is refused (``JpegUnsupported``); ``imread_device`` then decodes it with ``load_image_bgr``, so
such a file gives the pixels or the exception it gave before. The path is opt-in: ``LoadImage(imdecode_backend="mi355x")``,
``runner.test_dataset(decode="device")``, ``--decode device`` of tools/test.py and demo/image_demo.py.

The encoder is the same split the other way round: ``encode_batch`` converts, downsamples, transforms and quantises all
images of a batch on the device (``pp_jpeg_forward_batch``: two launches), copies the coefficients to the host once and
Huffman-codes them on host threads (``pp_jpeg_entropy_encode``, GIL-free). The file holds the coefficients, tables and
sampling Pillow's ``Image.save(path, "JPEG", quality=q, subsampling=s)`` writes for the same pixels, so it decodes to the
same pixels; its marker layout may differ. Opt-in as well: ``PoseLocalVisualizer(image_encoder="device")``, ``--encode device``
of demo/image_demo.py.

``encode_batch(..., entropy="device")`` codes on the device as well (``pp_jpeg_entropy_encode_batch``, csrc/pp_jpeg_entropy.hip:
seven launches behind the forward call's two, on the same stream): the coefficients never leave the device, the host
receives the finished streams and puts ``pp_jpeg_write_headers``' bytes in front and ``FF D9`` behind. The files are byte
for byte those of the host coder. With restart intervals: ``restart_rows``, at the end of this text; the default stays ``entropy="host"``.

``optimize=True`` (``entropy_encode``, ``entropy_encode_device``, ``encode_batch``, ``imwrite_device``) codes every file with the
Huffman tables libjpeg builds from the image's own symbol statistics - the tables and the scan of Pillow's
``save(..., optimize=True)`` for the same coefficients: identical pixels in fewer bytes. On the host that is
``pp_jpeg_entropy_encode_opt``; with ``entropy="device"`` it is ``pp_jpeg_entropy_encode_opt_batch``
(csrc/pp_jpeg_entropy_opt.hip: histogram, code build and the coder's seven phases in ten launches, no host round trip between
them), whose per-image records bring the tables back with the result slots. The default, ``optimize=False``, writes the
annex K tables: every byte as before.

``decode_batch(..., entropy="device")`` decodes the Huffman codes on the device as well (``pp_jpeg_huffman_decode_batch``,
csrc/pp_jpeg_huffdec.hip: ``sync_passes`` + 4 launches in front of the reconstruct call's two, on the same stream): the host
only reads the headers (``scan_prepare``), a file goes up as its own bytes and the coefficients never cross the bus. The
stream is decoded in subsequences of 128 bytes by self-synchronising passes; an image the passes did not synchronise, or
whose stream is damaged, is refused by its result slot - never decoded wrongly - and goes through ``entropy_decode``.
Files with a restart interval decode there as well (``scan_prepare(data, restart=True)``): an RSTn marker is a point where
the decoder's state is known, so inside such a file the synchronisation distance is bounded by the interval's length; the
order and number of the markers are checked on the device. (A file with more than 7 fill bytes in front of a marker is
turned away by the preparation and decodes on the host, uncounted.) The pixels are those of ``entropy="host"``, which stays
the default. Not done on the device: progressive, arithmetic-coded and 12-bit files (no decoder here takes them).

Restart intervals are coded on the device too: ``entropy_encode_device(..., restart_interval=R)`` (an int, or one per image)
and ``encode_batch(..., entropy="device", restart_rows=N)`` (a marker every N MCU rows of each image's own width, libjpeg's
``restart_in_rows``) run ``pp_jpeg_entropy_encode_restart_batch`` resp. ``pp_jpeg_entropy_encode_opt_restart_batch`` - the
same seven resp. ten launches with a segmented level: the DC prediction cut at every interval start, every interval padded
to a byte, unstuffed RSTn markers between them - and give the files of ``entropy="host"`` at the same interval byte for
byte. Without either keyword every path makes the calls it made before. (``encode_batch(entropy="device",
restart_interval=R)`` with R != 0 is still refused: one MCU count means another thing for every width of a mixed batch.)
"""
import ctypes
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .staging import BatchStaging, StagedBlock, _align

fallbacks = 0  # files imread_device / the test loop handed to the host decoder since import (diagnostics)
reconstruct_calls = 0  # pp_jpeg_reconstruct_bgr_batch calls since import
forward_calls = 0  # pp_jpeg_forward_batch calls since import
entropy_device_calls = 0  # pp_jpeg_entropy_encode_batch / pp_jpeg_entropy_encode_opt_batch calls since import
entropy_opt_device_calls = 0  # pp_jpeg_entropy_encode_opt_batch calls among them
entropy_restart_device_calls = 0  # the *_restart_batch forms among both
huffman_device_calls = 0  # pp_jpeg_huffman_decode_batch calls since import
unsynchronised = 0  # images the device Huffman decoder refused by their result slot since import (each also counts in fallbacks)


class JpegInfo(ctypes.Structure):
    """pp_jpeg_info of include/probpose_mi355x.h."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ncomp", ctypes.c_int32), ("precision", ctypes.c_int32),
                ("hs", ctypes.c_int32), ("vs", ctypes.c_int32), ("mcus_x", ctypes.c_int32), ("mcus_y", ctypes.c_int32),
                ("comp_bw", ctypes.c_int32 * 3), ("comp_bh", ctypes.c_int32 * 3), ("restart_interval", ctypes.c_int32),
                ("supported", ctypes.c_int32), ("coef_count", ctypes.c_int64), ("reason", ctypes.c_char * 96)]


# pp_jpeg_desc: four pointers, eight int32
_DESC = np.dtype([("coef", "<u8"), ("qtables", "<u8"), ("planes", "<u8"), ("out", "<u8"), ("width", "<i4"), ("height", "<i4"),
                  ("ncomp", "<i4"), ("hs", "<i4"), ("vs", "<i4"), ("mcus_x", "<i4"), ("mcus_y", "<i4"), ("reserved", "<i4")])
assert _DESC.itemsize == 64
# pp_jpeg_enc_desc: four pointers, eight int32
_ENC_DESC = np.dtype([("src", "<u8"), ("qtables", "<u8"), ("planes", "<u8"), ("coef", "<u8"), ("width", "<i4"), ("height", "<i4"),
                      ("row_stride", "<i4"), ("rgb", "<i4"), ("hs", "<i4"), ("vs", "<i4"), ("mcus_x", "<i4"), ("mcus_y", "<i4")])
assert _ENC_DESC.itemsize == 64
# pp_jpeg_ent_desc: four pointers, the capacity, four int32, the restart interval, four reserved bytes; pp_jpeg_ent_result.
# _ENT_DESC keeps the shape its users fill row by row, ten values: its last field is the interval and the reserved word as
# one little-endian int64 (an interval 0..65535 written there lands in restart_interval, 0 in reserved); _ENT_RESTART_DESC
# names the two fields of the header.
_ENT_DESC = np.dtype([("coef", "<u8"), ("scratch", "<u8"), ("out", "<u8"), ("result", "<u8"), ("capacity", "<i8"), ("hs", "<i4"),
                      ("vs", "<i4"), ("mcus_x", "<i4"), ("mcus_y", "<i4"), ("reserved", "<i8")])
assert _ENT_DESC.itemsize == 64
_ENT_RESTART_DESC = np.dtype(_ENT_DESC.descr[:-1] + [("restart_interval", "<i4"), ("reserved", "<i4")])
assert _ENT_RESTART_DESC.itemsize == 64 and _ENT_RESTART_DESC.fields["restart_interval"][1] == 56
_ENT_RESULT = np.dtype([("bytes", "<i8"), ("status", "<i4"), ("reserved", "<i4")])
assert _ENT_RESULT.itemsize == 16
# pp_jpeg_ent_opt_desc: pp_jpeg_ent_desc and the record's address; pp_jpeg_opt_record
_ENT_OPT_DESC = np.dtype(_ENT_DESC.descr + [("record", "<u8")])
assert _ENT_OPT_DESC.itemsize == 72
_ENT_OPT_RESTART_DESC = np.dtype(_ENT_RESTART_DESC.descr + [("record", "<u8")])
assert _ENT_OPT_RESTART_DESC.itemsize == 72
_OPT_RECORD = np.dtype([("hist", "<u4", (4, 257)), ("bits", "u1", (4, 16)), ("vals", "u1", (4, 256)), ("lookup", "<u4", (4, 256)),
                        ("status", "<i4"), ("nvals", "<i4", (4,)), ("reserved", "<i4", (7,))])
assert _OPT_RECORD.itemsize == 9344 and _OPT_RECORD.fields["lookup"][1] == 5200
ENTROPY = ("host", "device")


class HuffTable(ctypes.Structure):
    """pp_jpeg_huff_table of include/probpose_mi355x.h."""
    _fields_ = [("look", ctypes.c_uint16 * 512), ("maxcode", ctypes.c_int32 * 18), ("valoffset", ctypes.c_int32 * 18),
                ("vals", ctypes.c_uint8 * 256)]


class _Scan(ctypes.Structure):
    """pp_jpeg_scan of include/probpose_mi355x.h."""
    _fields_ = [("info", JpegInfo), ("qtables", ctypes.c_uint16 * 192), ("tables", HuffTable * 6), ("stream_offset", ctypes.c_int64),
                ("stream_bytes", ctypes.c_int64)]


TABLE_BYTES = ctypes.sizeof(HuffTable)
assert TABLE_BYTES == 1424
# pp_jpeg_hd_desc: five pointers, the stream's length, six int32; pp_jpeg_hd_result
_HD_DESC = np.dtype([("stream", "<u8"), ("tables", "<u8"), ("coef", "<u8"), ("scratch", "<u8"), ("result", "<u8"), ("stream_bytes", "<i8"),
                     ("hs", "<i4"), ("vs", "<i4"), ("mcus_x", "<i4"), ("mcus_y", "<i4"), ("ncomp", "<i4"), ("restart_interval", "<i4")])
assert _HD_DESC.itemsize == 72
_HD_RESULT = np.dtype([("status", "<i4"), ("passes", "<i4"), ("blocks", "<i4"), ("reason", "<i4")])
assert _HD_RESULT.itemsize == 16
SUBSEQUENCE_BYTES = 128  # HD_S of csrc/pp_jpeg_huffdec_core.h
INNER_ITERATIONS = 32  # HD_INNER
MAX_SYNC_PASSES = 64
# p launches carry a decoder state over 32 (p - 1) + 2 subsequences: 3 launches cover 8448 bytes, above the 8 KiB the default is to cover
DEFAULT_SYNC_PASSES = 3
assert SUBSEQUENCE_BYTES * (INNER_ITERATIONS * (DEFAULT_SYNC_PASSES - 1) + 2) >= 8192
HD_REASONS = {0: "", 1: "not synchronised", 2: "data ends before the last MCU", 3: "bad Huffman code, category or coefficient index",
              4: "DC coefficient out of range", 5: "data after the last MCU", 6: "descriptor outside the subset",
              7: "restart markers out of place, order or number"}
SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}  # pp_jpeg_encode_plan's numbering (Pillow's as well)


class JpegUnsupported(ValueError):
    """The file is outside the subset the split decoder accepts (``reason`` says why): decode it on the host."""

    def __init__(self, reason: str):
        super().__init__(f"JPEG outside the GPU decoder's subset: {reason}")
        self.reason = reason


class JpegCoefficients(NamedTuple):
    """What the host half leaves of one file: ``info`` (geometry), ``coef`` (info.coef_count int16: per component
    [block_row][block_col][64], natural order, whole MCUs), ``qtables`` (ncomp, 64) uint16 in natural order."""

    info: JpegInfo
    coef: np.ndarray
    qtables: np.ndarray

    @property
    def shape(self):
        return (int(self.info.height), int(self.info.width), 3)


def _cuda_device(device, function: str) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"probpose_code_amd.jpeg.{function} runs on the GPU only (no CPU fallback)")
    return device


def _check_entropy(entropy) -> None:
    if entropy not in ENTROPY:
        raise ValueError(f"entropy must be one of {ENTROPY}, got {entropy!r}")


def _size(query: str, value) -> int:
    """What a size query of the library returned; a negative value is its status."""
    if value < 0:
        raise _lib.ProbPoseLibraryError(query, _lib.lib.pp_status_string(value).decode(), _lib.last_error())
    return int(value)


def _bytes_of(data) -> bytes:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return bytes(data)
    if isinstance(data, np.ndarray):
        return data.astype(np.uint8, copy=False).tobytes()
    with open(data, "rb") as f:
        return f.read()


def probe(data) -> JpegInfo:
    """Geometry, sampling, block grid, coefficient count and restart interval of a file (bytes or a path), read from its
    headers. ``info.supported`` is 0 and ``info.reason`` says why when the file is outside the accepted subset."""
    raw = _bytes_of(data)
    info = JpegInfo()
    st = _lib.lib.pp_jpeg_probe(raw, len(raw), ctypes.byref(info))
    if st not in (_lib.PP_OK, _lib.PP_ERR_UNSUPPORTED):
        _lib.check("pp_jpeg_probe", st)
    return info


def entropy_decode(data) -> JpegCoefficients:
    """The host half: the quantised coefficients and quantisation tables of a file (bytes or a path). Thread-safe and
    GIL-free while it decodes. Raises ``JpegUnsupported`` for a file outside the subset or with an irregular stream."""
    raw = _bytes_of(data)
    info = probe(raw)
    if not info.supported:
        raise JpegUnsupported(info.reason.decode("utf-8", "replace"))
    coef = np.empty(int(info.coef_count), np.int16)
    qt = np.zeros((3, 64), np.uint16)
    st = _lib.lib.pp_jpeg_entropy_decode(raw, len(raw), coef.ctypes.data, coef.size, qt.ctypes.data, ctypes.byref(info))
    if st == _lib.PP_ERR_UNSUPPORTED:
        raise JpegUnsupported(info.reason.decode("utf-8", "replace"))
    _lib.check("pp_jpeg_entropy_decode", st)
    return JpegCoefficients(info, coef, qt[:int(info.ncomp)])


class JpegScan(NamedTuple):
    """What ``scan_prepare`` reads from a file's headers: ``info`` (geometry), ``qtables`` (ncomp, 64) uint16 in natural order,
    ``tables`` (the 2 x ncomp ``pp_jpeg_huff_table`` of the components as uint8: DC, AC of each), ``stream`` (the entropy-coded
    segment, byte stuffing included, a uint8 view of ``data``) and ``data`` (the file's bytes)."""

    info: JpegInfo
    qtables: np.ndarray
    tables: np.ndarray
    stream: np.ndarray
    data: bytes

    @property
    def shape(self):
        return (int(self.info.height), int(self.info.width), 3)


def scan_prepare(data, restart: bool = False) -> JpegScan:
    """The host's share of ``entropy="device"``: the headers of a file (bytes or a path) and the bounds of its entropy-coded
    segment; no bit of it is decoded. Thread-safe and GIL-free. Raises ``JpegUnsupported`` for what ``entropy_decode`` refuses
    by the headers, for a file with a restart interval and for a segment no EOI marker ends. ``restart=True``
    (``pp_jpeg_scan_prepare_restart``): a file with a restart interval is accepted too - ``info.restart_interval`` says so and
    the segment holds its RSTn markers; every other file gives what it gives without the flag."""
    raw = _bytes_of(data)
    scan = _Scan()
    name = "pp_jpeg_scan_prepare_restart" if restart else "pp_jpeg_scan_prepare"
    st = getattr(_lib.lib, name)(raw, len(raw), ctypes.byref(scan))
    if st == _lib.PP_ERR_UNSUPPORTED:
        raise JpegUnsupported(scan.info.reason.decode("utf-8", "replace"))
    _lib.check(name, st)
    ncomp = int(scan.info.ncomp)
    info = JpegInfo.from_buffer_copy(scan.info)
    qt = np.frombuffer(scan, np.uint16, 64 * ncomp, _Scan.qtables.offset).reshape(ncomp, 64).copy()
    tables = np.frombuffer(scan, np.uint8, 2 * ncomp * TABLE_BYTES, _Scan.tables.offset).copy()
    stream = np.frombuffer(raw, np.uint8, int(scan.stream_bytes), int(scan.stream_offset))
    return JpegScan(info, qt, tables, stream, raw)


class _ReconJob(NamedTuple):
    """One ``pp_jpeg_reconstruct_bgr_batch`` call: ``args`` (its arguments), ``out`` (the (H, W, 3) output tensors), ``block``
    (the uploaded ``StagedBlock``) and ``keep`` (the other tensors the launches use)."""

    args: tuple
    out: list
    block: StagedBlock
    keep: tuple


class _HuffmanJob(NamedTuple):
    """One ``pp_jpeg_huffman_decode_batch`` call: ``coef`` (image i's int16 coefficients, views of one tensor), ``results``
    (n x 16 bytes, a view of the uploaded block), ``args`` (the call's arguments), ``recon_args`` / ``out`` (the arguments of
    ``pp_jpeg_reconstruct_bgr_batch`` on the same coefficients and its output tensors, or None), ``block`` (the uploaded
    ``StagedBlock``) and ``keep`` (the other tensors the launches use)."""

    coef: list
    results: torch.Tensor
    args: tuple
    recon_args: Optional[tuple]
    out: Optional[list]
    block: StagedBlock
    keep: tuple


def _sync_passes(sync_passes) -> int:
    p = DEFAULT_SYNC_PASSES if sync_passes is None else sync_passes
    if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 1 <= int(p) <= MAX_SYNC_PASSES:
        raise ValueError(f"sync_passes must be an int in 1..{MAX_SYNC_PASSES}, got {sync_passes!r}")
    return int(p)


def _stage_huffman(scans: Sequence[JpegScan], device, staging, sync_passes: int, reconstruct: bool) -> _HuffmanJob:
    """Pack the descriptor tables, the Huffman and quantisation tables and the streams of a batch into the pinned buffer and
    upload them with one copy. ``reconstruct``: the descriptors of ``pp_jpeg_reconstruct_bgr_batch`` travel in the same copy
    and point at the coefficients where the decoder leaves them."""
    n = len(scans)
    infos = (JpegInfo * n)(*[s.info for s in scans])
    lens = (ctypes.c_longlong * n)(*[int(s.stream.size) for s in scans])
    shares = [_size("pp_jpeg_huffman_scratch_bytes", _lib.lib.pp_jpeg_huffman_scratch_bytes(ctypes.byref(infos[i]), ctypes.byref(lens, 8 * i), 1))
              for i in range(n)]
    # the block: decoder descriptors (n x 72 bytes) | result slots (n x 16) | reconstruct descriptors (n x 64) | per image:
    # Huffman tables, quantisation tables (3 x 64 u16), stream bytes
    blk = StagedBlock([("desc", 72 * n), ("results", 16 * n), ("recon", 64 * n)],
                      [("tables", [s.tables.size for s in scans]), ("qtables", [384] * n), ("stream", [max(int(s.stream.size), 1) for s in scans])])
    counts = [int(s.info.coef_count) for s in scans]
    o_coef, at = [], 0
    for c in counts:
        o_coef.append(at)
        at += _align(2 * c) // 2
    coef_all = torch.empty(max(at, 1), dtype=torch.int16, device=device)
    scratch = torch.empty(sum(shares), dtype=torch.uint8, device=device)
    blk.acquire(staging, device)
    planes = torch.empty(sum(_align(c) for c in counts), dtype=torch.uint8, device=device) if reconstruct else None
    out = [torch.empty(s.shape, dtype=torch.uint8, device=device) for s in scans] if reconstruct else None
    desc, rec = blk.host("desc", _HD_DESC), blk.host("recon", _DESC)
    blk.host("results")[:] = 0
    tables, qtables, streams = blk.hosts("tables"), blk.hosts("qtables", np.uint16), blk.hosts("stream")
    p_tables, p_qtables, p_streams, p_results = blk.ptrs("tables"), blk.ptrs("qtables"), blk.ptrs("stream"), blk.ptr("results")
    s_at, p_at = scratch.data_ptr(), (planes.data_ptr() if reconstruct else 0)
    for i, s in enumerate(scans):
        info = s.info
        if s.tables.size != 2 * int(info.ncomp) * TABLE_BYTES or s.tables.dtype != np.uint8 or s.stream.dtype != np.uint8:
            raise ValueError("a JpegScan holds 2 x ncomp tables and its stream as uint8")
        tables[i][:] = s.tables
        qtables[i][:64 * len(s.qtables)] = s.qtables.reshape(-1)
        streams[i][:s.stream.size] = s.stream
        coef_ptr = coef_all.data_ptr() + 2 * o_coef[i]
        desc[i] = (p_streams[i], p_tables[i], coef_ptr, s_at, p_results + 16 * i, s.stream.size, info.hs, info.vs, info.mcus_x, info.mcus_y,
                   info.ncomp, info.restart_interval)
        s_at += shares[i]
        if reconstruct:
            rec[i] = (coef_ptr, p_qtables[i], p_at, out[i].data_ptr(), info.width, info.height, info.ncomp, info.hs, info.vs, info.mcus_x,
                      info.mcus_y, 0)
            p_at += _align(counts[i])
    blk.upload()
    max_blocks = max(c // 64 for c in counts)
    args = (blk.base, n, max(int(s.stream.size) for s in scans), max_blocks, sync_passes)
    recon_args = (blk.ptr("recon"), n, max_blocks, max(int(s.info.height) for s in scans), max(int(s.info.width) for s in scans)) if reconstruct else None
    return _HuffmanJob([coef_all[o:o + c] for o, c in zip(o_coef, counts)], blk.device("results"), args, recon_args, out, blk, (scratch, coef_all, planes))


def _huffman_launch(job: _HuffmanJob, stream) -> None:
    global huffman_device_calls
    _lib.call("pp_jpeg_huffman_decode_batch", *job.args, stream.cuda_stream)
    huffman_device_calls += 1


def huffman_decode_device(scans: Sequence[JpegScan], device="cuda", staging=None, sync_passes: Optional[int] = None):
    """The Huffman half on the device for a batch of ``JpegScan`` of any mix of sizes and sampling: one upload of the
    descriptors, tables and stream bytes through the pinned buffer of ``staging``, then ONE ``pp_jpeg_huffman_decode_batch``
    call (``sync_passes`` + 4 launches, default ``DEFAULT_SYNC_PASSES``) on the current stream, then one read-back of the
    result slots. Returns (the int16 device tensors of ``info.coef_count`` coefficients in ``entropy_decode``'s layout, the
    slots as a structured array: status, passes, blocks, reason). Where ``status`` is not ``PP_OK`` (``HD_REASONS[reason]``
    says why: above all "not synchronised") the coefficients are undefined."""
    scans = list(scans)
    passes = _sync_passes(sync_passes)
    if len(scans) == 0:
        return [], np.zeros(0, _HD_RESULT)
    device = _cuda_device(device, "huffman_decode_device")
    job = _stage_huffman(scans, device, staging if staging is not None else BatchStaging(), passes, False)
    _huffman_launch(job, torch.cuda.current_stream(device))
    return job.coef, job.results.cpu().numpy().view(_HD_RESULT).copy()


def decode_scans(scans: Sequence[JpegScan], device="cuda", staging=None, sync_passes: Optional[int] = None) -> List[torch.Tensor]:
    """The (H, W, 3) uint8 BGR device tensors of a batch of ``JpegScan``: one upload, ``pp_jpeg_huffman_decode_batch`` and
    ``pp_jpeg_reconstruct_bgr_batch`` on the coefficients where they lie, one read-back of the result slots. An image whose
    slot is not ``PP_OK`` is decoded again through ``entropy_decode`` (outside its subset: by the host decoder) and counted
    in ``fallbacks`` and ``unsynchronised``."""
    global reconstruct_calls
    scans = list(scans)
    passes = _sync_passes(sync_passes)
    if len(scans) == 0:
        return []
    device = _cuda_device(device, "decode_scans")
    staging = staging if staging is not None else BatchStaging()
    job = _stage_huffman(scans, device, staging, passes, True)
    stream = torch.cuda.current_stream(device)
    _huffman_launch(job, stream)
    _lib.call("pp_jpeg_reconstruct_bgr_batch", *job.recon_args, stream.cuda_stream)
    reconstruct_calls += 1
    out = list(job.out)
    res = job.results.cpu().numpy().view(_HD_RESULT)  # (waits for the stream: the launches have run)
    again = [i for i, r in enumerate(res) if int(r["status"]) != _lib.PP_OK]
    for i, decoded in zip(again, _step_down([scans[i].data for i in again], "huffman", device)):
        out[i] = decoded
    return _reconstruct_pending(out, device, staging)


def _stage(coefficients: Sequence[JpegCoefficients], device, staging, out, scratch) -> _ReconJob:
    """Pack the descriptor table, the tables and the coefficients of a batch into the pinned buffer and upload them with one
    copy."""
    n = len(coefficients)
    infos = (JpegInfo * n)(*[c.info for c in coefficients])
    need = _size("pp_jpeg_scratch_bytes", _lib.lib.pp_jpeg_scratch_bytes(infos, n))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=device)
    elif scratch.numel() < need or scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.data_ptr() % 8:
        raise ValueError(f"scratch must be a contiguous 8-byte aligned uint8 tensor of at least {need} bytes")
    if out is None:
        out = [torch.empty(c.shape, dtype=torch.uint8, device=device) for c in coefficients]
    else:
        if len(out) != n:
            raise ValueError("one out tensor per image")
        for t, c in zip(out, coefficients):
            if tuple(t.shape) != c.shape or t.dtype != torch.uint8 or not t.is_contiguous() or t.device != scratch.device:
                raise ValueError(f"out tensors must be contiguous uint8 {c.shape} on {scratch.device}")
    # the block: descriptors (n x 64 bytes) | per image: quantisation tables (3 x 64 u16), coefficients (int16)
    blk = StagedBlock([("desc", 64 * n)], [("qtables", [384] * n), ("coef", [2 * c.coef.size for c in coefficients])]).acquire(staging, device)
    desc, planes = blk.host("desc", _DESC), scratch.data_ptr()
    qtables, coef, p_qtables, p_coef = blk.hosts("qtables", np.uint16), blk.hosts("coef", np.int16), blk.ptrs("qtables"), blk.ptrs("coef")
    for i, c in enumerate(coefficients):
        info = c.info
        if c.coef.size != info.coef_count or c.coef.dtype != np.int16:
            raise ValueError("coefficient array does not match its info")
        qtables[i][:64 * len(c.qtables)] = c.qtables.reshape(-1)
        coef[i][:] = c.coef
        desc[i] = (p_coef[i], p_qtables[i], planes, out[i].data_ptr(), info.width, info.height, info.ncomp, info.hs, info.vs, info.mcus_x,
                   info.mcus_y, 0)
        planes += _align(int(info.coef_count))
    blk.upload()
    args = (blk.base, n, max(int(c.info.coef_count) // 64 for c in coefficients), max(int(c.info.height) for c in coefficients),
            max(int(c.info.width) for c in coefficients))
    return _ReconJob(args, list(out), blk, (scratch,))


def reconstruct_batch(coefficients: Sequence[JpegCoefficients], device="cuda", staging=None, out: Optional[Sequence[torch.Tensor]] = None,
                      scratch: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """The device half for a batch of images of any mix of sizes and sampling: one upload of the descriptor table, the
    coefficients and the tables through the pinned buffer of ``staging`` (a ``transforms.BatchStaging``), then ONE
    ``pp_jpeg_reconstruct_bgr_batch`` call (two launches) on the current stream. Returns the (H, W, 3) uint8 BGR device
    tensors. ``out`` / ``scratch``: caller-provided output tensors (contiguous, of those shapes) and plane scratch."""
    global reconstruct_calls
    if len(coefficients) == 0:
        return []
    device = _cuda_device(device, "reconstruct_batch")
    job = _stage(coefficients, device, staging if staging is not None else BatchStaging(), out, scratch)
    _lib.call("pp_jpeg_reconstruct_bgr_batch", *job.args, torch.cuda.current_stream(device).cuda_stream)
    reconstruct_calls += 1
    return job.out


def _step_down(sources: list, failed: str, device) -> list:
    """One step down the ladder device Huffman decoder -> ``entropy_decode`` -> host decoder for files (paths or bytes), counted
    first. ``failed="huffman"``: refused by the result slot (``fallbacks``, ``unsynchronised``), on to ``entropy_decode`` and, outside
    its subset, to the host decoder. ``failed="entropy"``: refused by ``entropy_decode`` or unreadable (``fallbacks``), on to the host
    decoder, which raises what it always raised. Per file its ``JpegCoefficients``, still to be reconstructed, or its pixels."""
    global fallbacks, unsynchronised
    fallbacks += len(sources)
    if failed == "huffman":
        unsynchronised += len(sources)
    out = []
    for source in sources:
        decoded = None
        if failed == "huffman":
            try:
                decoded = entropy_decode(source)
            except JpegUnsupported:
                pass
        out.append(decoded if decoded is not None else torch.from_numpy(_host_decode(source)).to(device))
    return out


def _reconstruct_pending(out: list, device, staging) -> list:
    """``out`` with every ``JpegCoefficients`` in it replaced by its pixels: one ``reconstruct_batch`` for all of them."""
    todo = [i for i, c in enumerate(out) if isinstance(c, JpegCoefficients)]
    if todo:
        for i, t in zip(todo, reconstruct_batch([out[i] for i in todo], device, staging)):
            out[i] = t
    return out


def imread_device(path_or_bytes: Union[str, bytes], device="cuda", staging=None, entropy: str = "host") -> torch.Tensor:
    """A file (path or bytes) as the (H, W, 3) uint8 BGR device tensor ``torch.from_numpy(load_image_bgr(path)).to(device)``
    gives, decoded on the device where the file is inside the subset. Any other file goes through ``load_image_bgr`` and an
    upload: the same pixels, the same exceptions. ``entropy``: "host" (Huffman decoding on the host) or "device"
    (``decode_batch``'s device path for this one file)."""
    _check_entropy(entropy)
    if entropy == "device":
        return decode_batch([path_or_bytes], device, entropy="device", staging=staging)[0]
    try:
        c = entropy_decode(path_or_bytes)
    except (JpegUnsupported, OSError):  # (an unreadable path: the host decoder raises what it always raised)
        return _step_down([path_or_bytes], "entropy", device)[0]
    return reconstruct_batch([c], device, staging)[0]


def _host_decode(path_or_bytes) -> np.ndarray:
    from .apis import load_image_bgr

    if isinstance(path_or_bytes, str):
        return load_image_bgr(path_or_bytes)
    raw = _bytes_of(path_or_bytes)  # load_image_bgr for bytes in memory: cv2 where it exists, Pillow otherwise
    try:
        import cv2  # type: ignore

        img = cv2.imdecode(np.frombuffer(raw, np.uint8), cv2.IMREAD_COLOR)
        if img is None:
            raise OSError("cv2 could not decode the image bytes")
        return img
    except ImportError:
        pass
    import io

    from PIL import Image

    with Image.open(io.BytesIO(raw)) as im:
        rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def decode_batch(files: Sequence, device="cuda", entropy: str = "host", staging=None, sync_passes: Optional[int] = None) -> List[torch.Tensor]:
    """The (H, W, 3) uint8 BGR device tensors ``imread_device`` gives for a batch of files (paths or bytes) of any mix of sizes
    and sampling. ``entropy="host"``: ``entropy_decode`` per file, one ``reconstruct_batch``. ``entropy="device"``: the host only
    prepares the files (``scan_prepare(f, restart=True)``), their bytes go up in one copy, ``pp_jpeg_huffman_decode_batch`` and
    ``pp_jpeg_reconstruct_bgr_batch`` run on the current stream, and the result slots come back in one copy. A file the
    preparation refuses goes the ``entropy="host"`` way; an image whose slot is not ``PP_OK`` (not synchronised within
    ``sync_passes``, a damaged stream) goes through ``entropy_decode`` - or, outside its subset, through the host decoder - and
    is counted in ``fallbacks`` and in ``unsynchronised``. Pixels and exceptions are those of ``imread_device``."""
    _check_entropy(entropy)
    if isinstance(files, (str, bytes, bytearray, memoryview, np.ndarray)):
        raise ValueError("decode_batch takes a sequence of files; imread_device takes one")
    files = list(files)
    device = torch.device(device)
    staging = staging if staging is not None else BatchStaging()
    out = [None] * len(files)  # per file: its pixels, or its JpegCoefficients until _reconstruct_pending
    scans = []
    for i, f in enumerate(files):
        try:
            if entropy == "device":
                f = _bytes_of(f)
                try:
                    scans.append((i, scan_prepare(f, restart=True)))
                    continue
                except JpegUnsupported:
                    pass
            out[i] = entropy_decode(f)
        except (JpegUnsupported, OSError):  # (an unreadable path: the host decoder raises what it always raised)
            out[i] = _step_down([files[i]], "entropy", device)[0]
    if scans:
        for (i, _), t in zip(scans, decode_scans([s for _, s in scans], device, staging, sync_passes)):
            out[i] = t
    return _reconstruct_pending(out, device, staging)


def decode_or_host(path: str):
    """A worker's share of the test loop: the file's coefficients, or - outside the subset - its pixels from the host decoder."""
    try:
        return entropy_decode(path)
    except JpegUnsupported:
        return _host_decode(path)


def prepare_or_host(path: str):
    """A worker's share of the test loop with ``decode_entropy="device"``: the file's prepared scan (no bit decoded); for a file
    the preparation refuses its coefficients, or - outside the subset - its pixels from the host decoder."""
    raw = _bytes_of(path)
    try:
        return scan_prepare(raw, restart=True)
    except JpegUnsupported:
        pass
    try:
        return entropy_decode(raw)
    except JpegUnsupported:
        return _host_decode(path)


# ------------------------------------------------------------------------------------------------------------ encoder
def quality_tables(quality: int) -> np.ndarray:
    """(3, 64) uint16 quantisation tables in natural order (luma, chroma, chroma) of libjpeg's quality 1..100."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be an int in 1..100, got {quality!r}")
    qt = np.zeros((3, 64), np.uint16)
    _lib.call("pp_jpeg_quality_tables", int(quality), qt.ctypes.data)
    return qt


def encode_plan(width: int, height: int, subsampling: str = "4:2:0") -> JpegInfo:
    """The block geometry (``JpegInfo``) of a width x height file with ``subsampling`` "4:4:4", "4:2:2" or "4:2:0"."""
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLING)}, got {subsampling!r}")
    if not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
        raise ValueError(f"a JPEG file holds 1..65535 pixels a side, got {width} x {height}")
    info = JpegInfo()
    _lib.call("pp_jpeg_encode_plan", int(width), int(height), SUBSAMPLING[subsampling], ctypes.byref(info))
    return info


def _checked_coefficients(coefficients: JpegCoefficients, restart_interval):
    info, coef = coefficients.info, np.ascontiguousarray(coefficients.coef, np.int16)
    if coef.size != info.coef_count:
        raise ValueError("the encoder takes info.coef_count coefficients")
    if not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"restart_interval must be in 0..65535, got {restart_interval!r}")
    return info, coef


def symbol_histogram(coefficients: JpegCoefficients, restart_interval: int = 0) -> np.ndarray:
    """(4, 257) uint32: how often the scan of ``coefficients`` codes each symbol with the DC luma, AC luma, DC chroma and AC
    chroma table (``pp_jpeg_symbol_histogram``); bin 256, libjpeg's pseudo-symbol, is 0."""
    info, coef = _checked_coefficients(coefficients, restart_interval)
    hist = np.zeros((4, 257), np.uint32)
    _lib.call("pp_jpeg_symbol_histogram", coef.ctypes.data, ctypes.byref(info), int(restart_interval), hist.ctypes.data)
    return hist


def optimal_table(freq) -> tuple:
    """libjpeg's optimal Huffman table for 257 symbol frequencies (``pp_jpeg_optimal_table``; bin 256 is taken as 1):
    (``bits`` (16,) uint8: codes per length 1..16, ``vals`` uint8: the symbols in code order)."""
    freq = np.ascontiguousarray(freq, np.uint32)
    if freq.shape != (257,):
        raise ValueError("a table is built from 257 frequencies")
    bits, vals, n = np.zeros(16, np.uint8), np.zeros(256, np.uint8), ctypes.c_int(0)
    _lib.call("pp_jpeg_optimal_table", freq.ctypes.data, bits.ctypes.data, vals.ctypes.data, ctypes.byref(n))
    return bits, vals[:n.value].copy()


def entropy_encode(coefficients: JpegCoefficients, restart_interval: int = 0, optimize: bool = False) -> bytes:
    """The host half of the encoder: the baseline JFIF file of ``coefficients`` (three components, tables (3, 64) with values
    1..255). Thread-safe and GIL-free while it codes. ``optimize``: with the image's own optimal Huffman tables
    (``pp_jpeg_entropy_encode_opt``) instead of annex K's."""
    info, coef = coefficients.info, np.ascontiguousarray(coefficients.coef, np.int16)
    qt = np.ascontiguousarray(coefficients.qtables, np.uint16)
    if qt.shape != (3, 64) or coef.size != info.coef_count:
        raise ValueError("the encoder takes three (64,) tables and info.coef_count coefficients")
    if not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"restart_interval must be in 0..65535, got {restart_interval!r}")
    out = np.empty(_size("pp_jpeg_encoded_bound", _lib.lib.pp_jpeg_encoded_bound(ctypes.byref(info))), np.uint8)
    size = ctypes.c_size_t(0)
    _lib.call("pp_jpeg_entropy_encode_opt" if optimize else "pp_jpeg_entropy_encode", coef.ctypes.data, qt.ctypes.data, ctypes.byref(info),
              int(restart_interval), out.ctypes.data, out.size, ctypes.byref(size))
    return out[:size.value].tobytes()


def _encoder_images(images, device):
    """``images`` as (H, W, 3) uint8 device tensors with dense pixel rows; ValueError for anything else."""
    dev, checked = None, []
    for im in images:
        if isinstance(im, np.ndarray):
            if im.dtype != np.uint8:
                raise ValueError(f"the encoder takes (H, W, 3) uint8 images, got dtype {im.dtype}")
            im = torch.from_numpy(np.ascontiguousarray(im))
        if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            what = f"{tuple(im.shape)} {im.dtype}" if isinstance(im, torch.Tensor) else type(im).__name__
            raise ValueError(f"the encoder takes (H, W, 3) uint8 images, got {what}")
        if im.shape[0] == 0 or im.shape[1] == 0:
            raise ValueError("empty image")
        if im.shape[0] > 65535 or im.shape[1] > 65535:
            raise ValueError(f"a JPEG file holds at most 65535 pixels a side, got {im.shape[1]} x {im.shape[0]}")
        if im.is_cuda:
            if dev is not None and im.device != dev:
                raise ValueError(f"images of one batch must share a device: {im.device} and {dev}")
            dev = im.device
        checked.append(im)
    dev = _cuda_device(dev if dev is not None else (device or "cuda"), "encode_batch")
    out = []
    for im in checked:
        im = im.to(dev)  # a host array is uploaded first
        if im.stride(2) != 1 or im.stride(1) != 3 or im.stride(0) < 3 * im.shape[1] or im.stride(0) >= 2 ** 31:
            im = im.contiguous()  # (a view of whole rows, such as a vertical crop, is read in place)
        out.append(im)
    return out, dev


class _EntropyJob(NamedTuple):
    """One ``pp_jpeg_entropy_encode_batch`` call and its device buffers: ``desc_ptr`` (the uploaded descriptor table),
    ``results`` (n x 16 bytes, a view of the uploaded block), the streams (``out``: image i's at ``o_out[i]``, ``capacity[i]``
    bytes), the scratch, the infos, ``block`` (the uploaded ``StagedBlock``) and ``records_at`` (with ``optimize``: where, in
    ``results``, the n ``pp_jpeg_opt_record`` of ``pp_jpeg_entropy_encode_opt_batch`` begin; None without) and ``restart``
    (every image's restart interval: the ``*_restart_batch`` form of the call; None: the call without intervals)."""

    desc_ptr: int
    results: torch.Tensor
    out: torch.Tensor
    o_out: list
    capacity: list
    scratch: torch.Tensor
    infos: list
    block: StagedBlock
    records_at: Optional[int] = None
    restart: Optional[list] = None


def _entropy_call(job: "_EntropyJob") -> str:
    return "pp_jpeg_entropy_encode" + ("" if job.records_at is None else "_opt") + ("" if job.restart is None else "_restart") + "_batch"


def _entropy_regions(name: str, n: int, optimize: bool) -> list:
    """The head regions of a coded batch: the descriptor table ``name`` and "results" - the result slots and, with ``optimize``,
    the per-image records behind them (64-byte aligned), so that one copy brings both back."""
    if not optimize:
        return [(name, 64 * n), ("results", 16 * n)]
    return [(name, 72 * n), ("results", _records_at(n) + _OPT_RECORD.itemsize * n)]


def _records_at(n: int) -> int:
    return (16 * n + 63) // 64 * 64


class _ForwardJob(NamedTuple):
    """One ``pp_jpeg_forward_batch`` call: ``args`` (its arguments), ``block`` (the uploaded ``StagedBlock``; the coefficients
    are its per-image region "coef", behind everything the upload sent), ``infos``, ``qt`` (the tables), ``keep`` (the other
    tensors the launches use) and ``entropy`` (the ``pp_jpeg_entropy_encode_batch`` call on the same coefficients, or None)."""

    args: tuple
    block: StagedBlock
    infos: list
    qt: np.ndarray
    keep: tuple
    entropy: Optional[_EntropyJob]


def _stage_encode(images, qt, subsampling, channel_order, dev, staging, entropy=False, optimize=False, restart=None) -> _ForwardJob:
    """Pack the descriptor table and the tables of a batch into the pinned buffer and upload them with one copy. ``entropy``:
    the table and result slots of ``pp_jpeg_entropy_encode_batch`` travel in the same copy."""
    n = len(images)
    infos = [encode_plan(im.shape[1], im.shape[0], subsampling) for im in images]
    # the block: descriptors (n x 64 bytes) | quantisation tables (3 x 64 u16) | with entropy: its descriptors (n x 64 bytes),
    # result slots (n x 16 bytes) | per image: coefficients (int16)
    blk = StagedBlock([("desc", 64 * n), ("qtables", 384)] + (_entropy_regions("entropy", n, optimize) if entropy else []),
                      [("coef", [2 * int(i.coef_count) for i in infos])])
    scratch = torch.empty(sum(_align(int(i.coef_count)) for i in infos), dtype=torch.uint8, device=dev)
    blk.acquire(staging, dev)
    desc, planes, p_qtables, p_coef = blk.host("desc", _ENC_DESC), scratch.data_ptr(), blk.ptr("qtables"), blk.ptrs("coef")
    blk.host("qtables", np.uint16)[:] = qt.reshape(-1)
    for i, (im, info) in enumerate(zip(images, infos)):
        desc[i] = (im.data_ptr(), p_qtables, planes, p_coef[i], info.width, info.height, im.stride(0), int(channel_order == "rgb"),
                   info.hs, info.vs, info.mcus_x, info.mcus_y)
        planes += _align(int(info.coef_count))
    job = _entropy_job(blk, "entropy", infos, p_coef, dev, optimize, restart) if entropy else None
    blk.upload(before="coef")  # (the coefficient regions are only written on the device)
    args = (blk.base, n, max(int(i.coef_count) // 64 for i in infos), max(int(i.height) for i in infos), max(int(i.width) for i in infos))
    return _ForwardJob(args, blk, infos, qt, (images, scratch), job)


def write_headers(qtables: np.ndarray, info: JpegInfo, restart_interval: int = 0, tables=None) -> bytes:
    """The bytes SOI .. SOS of the file ``entropy_encode`` writes for these tables and this geometry (one code path).
    ``tables``: the file's Huffman tables as (``bits`` (4, 16) uint8, ``vals`` (4, 256) uint8) in the order DC luma, AC luma,
    DC chroma, AC chroma (``pp_jpeg_write_headers_tables``); None: annex K's."""
    qt = np.ascontiguousarray(qtables, np.uint16)
    if qt.shape != (3, 64):
        raise ValueError("the encoder takes three (64,) tables")
    out = np.empty(2048, np.uint8)
    size = ctypes.c_size_t(0)
    if tables is None:
        _lib.call("pp_jpeg_write_headers", qt.ctypes.data, ctypes.byref(info), int(restart_interval), out.ctypes.data, out.size, ctypes.byref(size))
    else:
        bits, vals = (np.ascontiguousarray(t, np.uint8) for t in tables)
        if bits.shape != (4, 16) or vals.shape != (4, 256):
            raise ValueError("tables are (bits (4, 16), vals (4, 256))")
        _lib.call("pp_jpeg_write_headers_tables", qt.ctypes.data, ctypes.byref(info), int(restart_interval), bits.ctypes.data, vals.ctypes.data,
                  out.ctypes.data, out.size, ctypes.byref(size))
    return out[:size.value].tobytes()


def _entropy_job(blk: StagedBlock, desc: str, infos, p_coef, dev, optimize=False, restart=None) -> _EntropyJob:
    """Allocate the scratch and the stream buffers of a batch, fill the n ``_ENT_DESC`` rows (with ``optimize``: ``_ENT_OPT_DESC``,
    the records behind the result slots) of region ``desc`` of ``blk`` and clear its "results" region; ``p_coef``: the device
    addresses of the coefficients. The caller uploads the block. A stream gets ``pp_jpeg_encoded_bound`` bytes: no stream of
    its geometry is longer, with annex K's tables or the image's own, at any restart interval. ``restart``: every image's
    interval for the ``*_restart_batch`` form (its scratch query, the interval in the rows); None: the form without."""
    shares, capacity = [], []
    query = "pp_jpeg_entropy_opt_scratch_bytes" if optimize else "pp_jpeg_entropy_scratch_bytes"
    if restart is not None:
        query = "pp_jpeg_entropy_restart_scratch_bytes"
    for info in infos:
        one = int(getattr(_lib.lib, query)(ctypes.byref(info), 1))
        bound = int(_lib.lib.pp_jpeg_encoded_bound(ctypes.byref(info)))
        _size(query, min(one, bound))
        shares.append(one)
        capacity.append(_align(bound))
    scratch = torch.empty(sum(shares), dtype=torch.uint8, device=dev)
    out = torch.empty(sum(capacity), dtype=torch.uint8, device=dev)
    if restart is None:
        rows = blk.host(desc, _ENT_OPT_DESC if optimize else _ENT_DESC)
    else:
        rows = blk.host(desc, _ENT_OPT_RESTART_DESC if optimize else _ENT_RESTART_DESC)
    p_results = blk.ptr("results")
    blk.host("results")[:] = 0
    records_at = _records_at(len(infos)) if optimize else None
    o_out, s_at, o_at = [], scratch.data_ptr(), 0
    for i, info in enumerate(infos):
        row = (p_coef[i], s_at, out.data_ptr() + o_at, p_results + 16 * i, capacity[i], info.hs, info.vs, info.mcus_x, info.mcus_y, 0)
        if restart is not None:
            row = row[:-1] + (int(restart[i]), 0)
        rows[i] = row + (p_results + records_at + _OPT_RECORD.itemsize * i,) if optimize else row
        o_out.append(o_at)
        s_at += shares[i]
        o_at += capacity[i]
    return _EntropyJob(blk.ptr(desc), blk.device("results"), out, o_out, capacity, scratch, list(infos), blk, records_at,
                       None if restart is None else [int(r) for r in restart])


def _entropy_launch(job: _EntropyJob, stream) -> None:
    global entropy_device_calls, entropy_opt_device_calls, entropy_restart_device_calls
    _lib.call(_entropy_call(job), job.desc_ptr, len(job.infos), max(int(i.coef_count) // 64 for i in job.infos), stream.cuda_stream)
    entropy_device_calls += 1
    entropy_opt_device_calls += job.records_at is not None
    entropy_restart_device_calls += job.restart is not None


def _entropy_collect(job: "_EntropyJob", qtables, stream, staging) -> List[bytes]:
    """The files of a coded batch: the result slots first (one copy, one synchronisation; with ``optimize`` the records, and
    in them every image's tables, come in the same copy), then the used bytes of every stream into the pinned buffer (one
    copy per image, one synchronisation), each between its headers and ``FF D9``."""
    n, name = len(job.infos), _entropy_call(job)
    back = job.results.cpu().numpy()  # (waits for the stream: the launches have run)
    res = back[:16 * n].view(_ENT_RESULT)
    records = None if job.records_at is None else back[job.records_at:job.records_at + _OPT_RECORD.itemsize * n].view(_OPT_RECORD)
    for i, r in enumerate(res):
        if int(r["status"]) != _lib.PP_OK:
            why = ("a coefficient no baseline code expresses (DC difference outside -2047..2047 or AC outside -1023..1023)"
                   if int(r["status"]) == _lib.PP_ERR_INVALID_ARG else f"the stream needs {int(r['bytes'])} bytes, {job.capacity[i]} were given")
            if records is not None and int(records[i]["status"]) != _lib.PP_OK:
                why = "the image's record was refused (too many blocks, or a code tree deeper than 32)"
            raise _lib.ProbPoseLibraryError(name, _lib.lib.pp_status_string(int(r["status"])).decode(), f"image {i}: {why}")
    sizes = [int(r["bytes"]) for r in res]
    at, offs = 0, []
    for sz in sizes:
        offs.append(at)
        at += _align(sz)
    blk = staging.acquire(max(at, 1))
    for o, sz, oo in zip(offs, sizes, job.o_out):
        staging.buf[o:o + sz].copy_(job.out[oo:oo + sz], non_blocking=True)
    stream.synchronize()
    tables = [None] * n if records is None else [(r["bits"], r["vals"]) for r in records]
    restart = [0] * n if job.restart is None else job.restart
    return [write_headers(qt, info, r, t) + blk[o:o + sz].tobytes() + b"\xff\xd9"
            for qt, info, r, t, o, sz in zip(qtables, job.infos, restart, tables, offs, sizes)]


def _stage_entropy(coefficients, dev, staging, optimize=False, restart=None) -> _EntropyJob:
    """Pack the descriptor table, the result slots and the coefficients of a batch into the pinned buffer and upload them
    with one copy."""
    n = len(coefficients)
    # the block: descriptors (n x 64 bytes) | result slots (n x 16 bytes) | per image: coefficients (int16)
    blk = StagedBlock(_entropy_regions("desc", n, optimize), [("coef", [2 * int(c.info.coef_count) for c in coefficients])]).acquire(staging, dev)
    for view, c in zip(blk.hosts("coef", np.int16), coefficients):
        view[:] = np.asarray(c.coef).reshape(-1)
    job = _entropy_job(blk, "desc", [c.info for c in coefficients], blk.ptrs("coef"), dev, optimize, restart)
    blk.upload()
    return job


def _restart_value(name: str, value) -> int:
    """``value`` as an int in 0..65535; booleans, floats and anything else are refused."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) <= 65535:
        raise ValueError(f"{name} must be an int in 0..65535, got {value!r}")
    return int(value)


def entropy_encode_device(coefficients: Sequence[JpegCoefficients], device=None, staging=None, optimize: bool = False,
                          restart_interval=0) -> List[bytes]:
    """The files ``entropy_encode`` gives for a list of ``JpegCoefficients`` (three components, geometry of ``encode_plan``),
    coded on the device: the coefficient arrays are uploaded with the table in one copy, then ONE
    ``pp_jpeg_entropy_encode_batch`` call (seven launches) on the current stream. Invalid coefficients raise what
    ``entropy_encode`` raises for them (``ProbPoseLibraryError``, PP_ERR_INVALID_ARG). ``optimize``: the files of
    ``entropy_encode(c, optimize=True)`` from ONE ``pp_jpeg_entropy_encode_opt_batch`` call (ten launches).
    ``restart_interval``: MCUs between restart markers, an int for all images or one int per image (0: none for that image):
    the files of ``entropy_encode(c, R, optimize)`` from ONE ``pp_jpeg_entropy_encode_restart_batch`` resp.
    ``pp_jpeg_entropy_encode_opt_restart_batch`` call (seven resp. ten launches again). With every interval 0 the call is the
    one made without the keyword."""
    coefficients = list(coefficients)
    if isinstance(restart_interval, (list, tuple, np.ndarray)):
        if len(restart_interval) != len(coefficients):
            raise ValueError(f"restart_interval holds {len(restart_interval)} values for {len(coefficients)} images")
        restart = [_restart_value("restart_interval", r) for r in restart_interval]
    else:
        restart = [_restart_value("restart_interval", restart_interval)] * len(coefficients)
    if len(coefficients) == 0:
        return []
    dev = _cuda_device(device or "cuda", "entropy_encode_device")
    staging = staging if staging is not None else BatchStaging()
    qts = []
    for c in coefficients:
        coef, qt = np.asarray(c.coef), np.ascontiguousarray(c.qtables, np.uint16)
        if qt.shape != (3, 64) or coef.size != c.info.coef_count or coef.dtype != np.int16:
            raise ValueError("the encoder takes three (64,) tables and info.coef_count int16 coefficients")
        write_headers(qt, c.info)  # (refuses an info that is no encode_plan result, and tables outside 1..255, before any GPU work)
        qts.append(qt)
    job = _stage_entropy(coefficients, dev, staging, bool(optimize), restart if any(restart) else None)
    stream = torch.cuda.current_stream(dev)
    _entropy_launch(job, stream)
    return _entropy_collect(job, qts, stream, staging)


def _forward(images, quality, subsampling, channel_order, device, staging, entropy: bool, optimize: bool = False,
             restart=None) -> Optional[_ForwardJob]:
    """What ``forward_batch`` and ``_encode_batch_device`` begin with: the options and images checked, the batch staged and
    ``pp_jpeg_forward_batch`` enqueued on the current stream. None for no images."""
    global forward_calls
    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"channel_order must be 'bgr' or 'rgb', got {channel_order!r}")
    qt = quality_tables(quality)
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLING)}, got {subsampling!r}")
    images, dev = _encoder_images(list(images), device)
    if len(images) == 0:
        return None
    job = _stage_encode(images, qt, subsampling, channel_order, dev, staging if staging is not None else BatchStaging(), entropy, optimize, restart)
    _lib.call("pp_jpeg_forward_batch", *job.args, torch.cuda.current_stream(dev).cuda_stream)
    forward_calls += 1
    return job


def forward_batch(images: Sequence, quality: int = 75, subsampling: str = "4:2:0", channel_order: str = "bgr", device=None,
                  staging=None, copy: bool = True) -> List[JpegCoefficients]:
    """The device half of the encoder for a batch of (H, W, 3) uint8 images of any mix of sizes: ONE
    ``pp_jpeg_forward_batch`` call (two launches) on the current stream, then one copy of all coefficients into the pinned
    buffer of ``staging`` (a ``transforms.BatchStaging``). Returns what ``entropy_decode`` gives for the finished files; with
    ``copy=False`` the coefficient arrays are views of the pinned buffer, valid until ``staging`` is used again."""
    job = _forward(images, quality, subsampling, channel_order, device, staging, False)
    if job is None:
        return []
    blk = job.block
    head = blk.head_bytes("coef")
    blk.staging.buf[head:blk.total].copy_(blk.dev[head:blk.total], non_blocking=True)
    torch.cuda.current_stream(blk.dev.device).synchronize()  # the coefficients are in the pinned buffer; ``job`` is no longer read
    return [JpegCoefficients(info, v.copy() if copy else v, job.qt) for v, info in zip(blk.hosts("coef", np.int16), job.infos)]


def encode_batch(images: Sequence, quality: int = 75, subsampling: str = "4:2:0", channel_order: str = "bgr", restart_interval: int = 0,
                 workers: int = 8, device=None, staging=None, entropy: str = "host", optimize: bool = False, restart_rows: int = 0) -> List[bytes]:
    """Baseline JPEG files of a batch of (H, W, 3) uint8 images (device tensors; a host array is uploaded first) of any mix
    of sizes: ``forward_batch`` on the device, then Huffman coding on a pool of ``workers`` host threads (at most
    ``runner.MAX_WORKERS``). ``quality`` 1..100, ``subsampling`` "4:4:4" / "4:2:2" / "4:2:0" and ``restart_interval`` (MCUs
    between restart markers, 0: none) mean what they mean to Pillow's ``Image.save``; ``channel_order``: "bgr" or "rgb"
    pixels. Each file decodes to the pixels Pillow's own file of that image decodes to.

    ``restart_rows`` (0: none) asks for a restart marker every ``restart_rows`` MCU rows of each image's OWN width - libjpeg's
    ``restart_in_rows``, ``cjpeg -restart N`` - which is what a mixed-size batch needs: image i is coded at the interval
    ``restart_rows * mcus_x[i]``. It excludes a non-zero ``restart_interval``; an interval above 65535 (the DRI segment holds
    16 bits) raises ``ValueError`` naming the image.

    ``entropy="device"`` codes on the device instead (``restart_interval`` must be 0 there; ``restart_rows`` is taken and runs
    the ``*_restart_batch`` forms of the calls, launch for launch the same number): the forward launches, then
    ``pp_jpeg_entropy_encode_batch`` on the same stream; the coefficients stay on the device and ``workers`` is not used. A
    batch of n images then costs one upload (tables and descriptors), 1 + n downloads (the result slots, then the used
    bytes of each stream) and two synchronisations, one after each kind of download. The files are byte for byte those
    of ``entropy="host"``; invalid coefficients raise the same ``ProbPoseLibraryError``.

    ``optimize=True`` gives every file the Huffman tables libjpeg builds from its own symbol statistics (Pillow's
    ``optimize=True``): the same coefficients, so the same pixels, in fewer bytes. With ``entropy="device"`` the statistics,
    the code build and the coding are ``pp_jpeg_entropy_encode_opt_batch``'s ten launches in place of the seven, the copies
    and synchronisations stay as they are (the tables come back with the result slots), and the files are byte for byte
    those of ``entropy="host"``. The default writes annex K's tables, every byte as before."""
    from concurrent.futures import ThreadPoolExecutor

    from .runner import MAX_WORKERS

    if isinstance(restart_interval, bool) or not isinstance(restart_interval, (int, np.integer)) or not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"restart_interval must be an int in 0..65535, got {restart_interval!r}")
    rows = _restart_value("restart_rows", restart_rows)
    if rows and int(restart_interval):
        raise ValueError("restart_rows and restart_interval exclude each other: one of them must be 0")
    if isinstance(images, (torch.Tensor, np.ndarray)):
        raise ValueError("encode_batch takes a sequence of (H, W, 3) images; imwrite_device takes one")
    _check_entropy(entropy)
    if entropy == "device" and int(restart_interval) != 0:
        raise ValueError("entropy='device' takes no restart_interval (one MCU count is no row of every width in a batch): ask for restart "
                         "markers with restart_rows, or code coefficients with entropy_encode_device(..., restart_interval=...)")
    restart = None
    if rows:
        images = list(images)
        restart = _row_intervals(images, subsampling, rows)
    if entropy == "device":
        return _encode_batch_device(images, quality, subsampling, channel_order, device, staging, bool(optimize), restart)
    coefs = forward_batch(images, quality, subsampling, channel_order, device, staging, copy=False)  # (coded before staging is used again)
    each = [int(restart_interval)] * len(coefs) if restart is None else restart
    if len(coefs) <= 1 or int(workers) <= 1:
        return [entropy_encode(c, r, optimize) for c, r in zip(coefs, each)]
    with ThreadPoolExecutor(max_workers=max(1, min(MAX_WORKERS, int(workers), len(coefs)))) as pool:
        return list(pool.map(lambda cr: entropy_encode(cr[0], cr[1], optimize), zip(coefs, each)))


def _row_intervals(images, subsampling, rows: int) -> list:
    """Every image's restart interval for a marker each ``rows`` MCU rows: ``rows`` x the MCUs of a row of its own width.
    ``ValueError`` for one that a DRI segment cannot hold. (What is no image is left to the encoder's own checks.)"""
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLING)}, got {subsampling!r}")
    out = []
    for i, im in enumerate(images):
        shape = tuple(getattr(im, "shape", ()))
        if len(shape) != 3 or not 1 <= shape[0] <= 65535 or not 1 <= shape[1] <= 65535:
            out.append(0)
            continue
        mcus_x = int(encode_plan(int(shape[1]), int(shape[0]), subsampling).mcus_x)
        if rows * mcus_x > 65535:
            raise ValueError(f"image {i} ({shape[1]} x {shape[0]}): restart_rows={rows} x {mcus_x} MCUs a row is an interval of {rows * mcus_x}, "
                             "above the 65535 a DRI segment holds")
        out.append(rows * mcus_x)
    return out


def _encode_batch_device(images, quality, subsampling, channel_order, device, staging, optimize=False, restart=None) -> List[bytes]:
    """``encode_batch`` with both halves on the device: nine launches on the current stream (twelve with ``optimize``), no
    coefficient copy. ``restart``: every image's interval (the ``*_restart_batch`` form of the entropy call), or None."""
    job = _forward(images, quality, subsampling, channel_order, device, staging, True, optimize, restart)
    if job is None:
        return []
    stream = torch.cuda.current_stream(job.block.dev.device)
    _entropy_launch(job.entropy, stream)
    return _entropy_collect(job.entropy, [job.qt] * len(job.infos), stream, job.block.staging)  # (``job`` lives until the streams are down)


def imwrite_device(path: str, image, **kw) -> None:
    """One picture written as a baseline JPEG file by ``encode_batch`` (its keyword arguments, ``entropy``, ``optimize`` and
    ``restart_rows`` among them)."""
    data = encode_batch([image], **kw)[0]
    with open(path, "wb") as f:
        f.write(data)
