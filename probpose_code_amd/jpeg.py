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
for byte those of the host coder. Restart interval 0 only; the default stays ``entropy="host"``.

``decode_batch(..., entropy="device")`` decodes the Huffman codes on the device as well (``pp_jpeg_huffman_decode_batch``,
csrc/pp_jpeg_huffdec.hip: ``sync_passes`` + 4 launches in front of the reconstruct call's two, on the same stream): the host
only reads the headers (``scan_prepare``), a file goes up as its own bytes and the coefficients never cross the bus. The
stream is decoded in subsequences of 128 bytes by self-synchronising passes; an image the passes did not synchronise, or
whose stream is damaged, is refused by its result slot - never decoded wrongly - and goes through ``entropy_decode``.
Files with a restart interval keep the host Huffman decoder. The pixels are those of ``entropy="host"``, which stays
the default.
"""
import ctypes
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib

fallbacks = 0  # files imread_device / the test loop handed to the host decoder since import (diagnostics)
reconstruct_calls = 0  # pp_jpeg_reconstruct_bgr_batch calls since import
forward_calls = 0  # pp_jpeg_forward_batch calls since import
entropy_device_calls = 0  # pp_jpeg_entropy_encode_batch calls since import
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
# pp_jpeg_ent_desc: four pointers, the capacity, four int32, eight reserved bytes; pp_jpeg_ent_result
_ENT_DESC = np.dtype([("coef", "<u8"), ("scratch", "<u8"), ("out", "<u8"), ("result", "<u8"), ("capacity", "<i8"), ("hs", "<i4"),
                      ("vs", "<i4"), ("mcus_x", "<i4"), ("mcus_y", "<i4"), ("reserved", "<i8")])
assert _ENT_DESC.itemsize == 64
_ENT_RESULT = np.dtype([("bytes", "<i8"), ("status", "<i4"), ("reserved", "<i4")])
assert _ENT_RESULT.itemsize == 16
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
                     ("hs", "<i4"), ("vs", "<i4"), ("mcus_x", "<i4"), ("mcus_y", "<i4"), ("ncomp", "<i4"), ("reserved", "<i4")])
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
              4: "DC coefficient out of range", 5: "data after the last MCU", 6: "descriptor outside the subset"}
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


def scan_prepare(data) -> JpegScan:
    """The host's share of ``entropy="device"``: the headers of a file (bytes or a path) and the bounds of its entropy-coded
    segment; no bit of it is decoded. Thread-safe and GIL-free. Raises ``JpegUnsupported`` for what ``entropy_decode`` refuses
    by the headers, for a file with a restart interval and for a segment no EOI marker ends."""
    raw = _bytes_of(data)
    scan = _Scan()
    st = _lib.lib.pp_jpeg_scan_prepare(raw, len(raw), ctypes.byref(scan))
    if st == _lib.PP_ERR_UNSUPPORTED:
        raise JpegUnsupported(scan.info.reason.decode("utf-8", "replace"))
    _lib.check("pp_jpeg_scan_prepare", st)
    ncomp = int(scan.info.ncomp)
    info = JpegInfo.from_buffer_copy(scan.info)
    qt = np.frombuffer(scan, np.uint16, 64 * ncomp, _Scan.qtables.offset).reshape(ncomp, 64).copy()
    tables = np.frombuffer(scan, np.uint8, 2 * ncomp * TABLE_BYTES, _Scan.tables.offset).copy()
    stream = np.frombuffer(raw, np.uint8, int(scan.stream_bytes), int(scan.stream_offset))
    return JpegScan(info, qt, tables, stream, raw)


def _align(v: int, a: int = 256) -> int:
    return (v + a - 1) // a * a


class _HuffmanJob(NamedTuple):
    """The device buffers of one ``pp_jpeg_huffman_decode_batch`` call: ``coef`` (image i's int16 coefficients, views of one
    tensor), ``results`` (n x 16 bytes, a view of the uploaded block), ``desc_ptr`` / ``args`` (the call's arguments),
    ``recon`` (the arguments of ``pp_jpeg_reconstruct_bgr_batch`` on the same coefficients and its output tensors, or None)
    and ``keep`` (every tensor the launches use)."""

    coef: list
    results: torch.Tensor
    args: tuple
    recon: Optional[tuple]
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
    shares = []
    for i in range(n):
        one = int(_lib.lib.pp_jpeg_huffman_scratch_bytes(ctypes.byref(infos[i]), ctypes.byref(lens, 8 * i), 1))
        if one < 0:
            raise _lib.ProbPoseLibraryError("pp_jpeg_huffman_scratch_bytes", _lib.lib.pp_status_string(one).decode(), _lib.last_error())
        shares.append(one)
    # the block: decoder descriptors (n x 72 bytes) | result slots (n x 16) | reconstruct descriptors (n x 64) | per image:
    # Huffman tables, quantisation tables (3 x 64 u16), stream bytes
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
    total = off
    counts = [int(s.info.coef_count) for s in scans]
    o_coef, at = [], 0
    for c in counts:
        o_coef.append(at)
        at += _align(2 * c) // 2
    coef_all = torch.empty(max(at, 1), dtype=torch.int16, device=device)
    scratch = torch.empty(sum(shares), dtype=torch.uint8, device=device)
    block = torch.empty(total, dtype=torch.uint8, device=device)
    planes = torch.empty(sum(_align(c) for c in counts), dtype=torch.uint8, device=device) if reconstruct else None
    out = [torch.empty(s.shape, dtype=torch.uint8, device=device) for s in scans] if reconstruct else None
    blk = staging.acquire(total)
    desc = blk[:72 * n].view(_HD_DESC)
    rec = blk[o_rec:o_rec + 64 * n].view(_DESC)
    blk[o_res:o_res + 16 * n] = 0
    base, s_at, p_at = block.data_ptr(), scratch.data_ptr(), (planes.data_ptr() if reconstruct else 0)
    for i, s in enumerate(scans):
        info = s.info
        if s.tables.size != 2 * int(info.ncomp) * TABLE_BYTES or s.tables.dtype != np.uint8 or s.stream.dtype != np.uint8:
            raise ValueError("a JpegScan holds 2 x ncomp tables and its stream as uint8")
        blk[o_tab[i]:o_tab[i] + s.tables.size] = s.tables
        blk[o_qt[i]:o_qt[i] + 128 * len(s.qtables)].view(np.uint16)[:] = s.qtables.reshape(-1)
        blk[o_str[i]:o_str[i] + s.stream.size] = s.stream
        coef_ptr = coef_all.data_ptr() + 2 * o_coef[i]
        desc[i] = (base + o_str[i], base + o_tab[i], coef_ptr, s_at, base + o_res + 16 * i, s.stream.size, info.hs, info.vs, info.mcus_x,
                   info.mcus_y, info.ncomp, 0)
        s_at += shares[i]
        if reconstruct:
            rec[i] = (coef_ptr, base + o_qt[i], p_at, out[i].data_ptr(), info.width, info.height, info.ncomp, info.hs, info.vs, info.mcus_x,
                      info.mcus_y, 0)
            p_at += _align(counts[i])
    staging.upload(block, total)
    max_blocks = max(c // 64 for c in counts)
    args = (base, n, max(int(s.stream.size) for s in scans), max_blocks, sync_passes)
    recon = ((base + o_rec, n, max_blocks, max(int(s.info.height) for s in scans), max(int(s.info.width) for s in scans)), out) if reconstruct else None
    return _HuffmanJob([coef_all[o:o + c] for o, c in zip(o_coef, counts)], block[o_res:o_res + 16 * n], args, recon, (block, scratch, coef_all, planes))


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
    from .transforms import BatchStaging

    scans = list(scans)
    passes = _sync_passes(sync_passes)
    if len(scans) == 0:
        return [], np.zeros(0, _HD_RESULT)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("probpose_code_amd.jpeg.huffman_decode_device runs on the GPU only (no CPU fallback)")
    job = _stage_huffman(scans, device, staging if staging is not None else BatchStaging(), passes, False)
    _huffman_launch(job, torch.cuda.current_stream(device))
    return job.coef, job.results.cpu().numpy().view(_HD_RESULT).copy()


def decode_scans(scans: Sequence[JpegScan], device="cuda", staging=None, sync_passes: Optional[int] = None) -> List[torch.Tensor]:
    """The (H, W, 3) uint8 BGR device tensors of a batch of ``JpegScan``: one upload, ``pp_jpeg_huffman_decode_batch`` and
    ``pp_jpeg_reconstruct_bgr_batch`` on the coefficients where they lie, one read-back of the result slots. An image whose
    slot is not ``PP_OK`` is decoded again through ``entropy_decode`` (outside its subset: by the host decoder) and counted
    in ``fallbacks`` and ``unsynchronised``."""
    global fallbacks, unsynchronised, reconstruct_calls
    from .transforms import BatchStaging

    scans = list(scans)
    passes = _sync_passes(sync_passes)
    if len(scans) == 0:
        return []
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("probpose_code_amd.jpeg.decode_scans runs on the GPU only (no CPU fallback)")
    staging = staging if staging is not None else BatchStaging()
    job = _stage_huffman(scans, device, staging, passes, True)
    stream = torch.cuda.current_stream(device)
    _huffman_launch(job, stream)
    _lib.call("pp_jpeg_reconstruct_bgr_batch", *job.recon[0], stream.cuda_stream)
    reconstruct_calls += 1
    out = list(job.recon[1])
    res = job.results.cpu().numpy().view(_HD_RESULT)  # (waits for the stream: the launches have run)
    again = [i for i, r in enumerate(res) if int(r["status"]) != _lib.PP_OK]
    fallbacks += len(again)
    unsynchronised += len(again)
    coefs = []
    for i in again:
        try:
            coefs.append((i, entropy_decode(scans[i].data)))
        except JpegUnsupported:
            out[i] = torch.from_numpy(_host_decode(scans[i].data)).to(device)
    if coefs:
        for (i, _), t in zip(coefs, reconstruct_batch([c for _, c in coefs], device, staging)):
            out[i] = t
    return out


def _stage(coefficients: Sequence[JpegCoefficients], device, staging, out, scratch):
    """Pack the descriptor table, the tables and the coefficients of a batch into the pinned buffer, upload them with one copy
    and return (the arguments of ``pp_jpeg_reconstruct_bgr_batch``, the output tensors, the tensors the launches read)."""
    n = len(coefficients)
    infos = (JpegInfo * n)(*[c.info for c in coefficients])
    need = int(_lib.lib.pp_jpeg_scratch_bytes(infos, n))
    if need < 0:
        raise _lib.ProbPoseLibraryError("pp_jpeg_scratch_bytes", _lib.lib.pp_status_string(need).decode(), _lib.last_error())
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
    off, o_qt, o_coef = _align(64 * n), [], []
    for c in coefficients:
        o_qt.append(off)
        off = _align(off + 384)
        o_coef.append(off)
        off = _align(off + 2 * c.coef.size)
    total = off
    dev = torch.empty(total, dtype=torch.uint8, device=device)
    blk = staging.acquire(total)
    desc = blk[:64 * n].view(_DESC)
    base, planes = dev.data_ptr(), scratch.data_ptr()
    for i, c in enumerate(coefficients):
        info = c.info
        if c.coef.size != info.coef_count or c.coef.dtype != np.int16:
            raise ValueError("coefficient array does not match its info")
        blk[o_qt[i]:o_qt[i] + 128 * len(c.qtables)].view(np.uint16)[:] = c.qtables.reshape(-1)
        blk[o_coef[i]:o_coef[i] + 2 * c.coef.size].view(np.int16)[:] = c.coef
        desc[i] = (base + o_coef[i], base + o_qt[i], planes, out[i].data_ptr(), info.width, info.height, info.ncomp, info.hs, info.vs,
                   info.mcus_x, info.mcus_y, 0)
        planes += _align(int(info.coef_count))
    staging.upload(dev, total)
    args = (base, n, max(int(c.info.coef_count) // 64 for c in coefficients), max(int(c.info.height) for c in coefficients),
            max(int(c.info.width) for c in coefficients))
    return args, list(out), (dev, scratch)


def reconstruct_batch(coefficients: Sequence[JpegCoefficients], device="cuda", staging=None, out: Optional[Sequence[torch.Tensor]] = None,
                      scratch: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """The device half for a batch of images of any mix of sizes and sampling: one upload of the descriptor table, the
    coefficients and the tables through the pinned buffer of ``staging`` (a ``transforms.BatchStaging``), then ONE
    ``pp_jpeg_reconstruct_bgr_batch`` call (two launches) on the current stream. Returns the (H, W, 3) uint8 BGR device
    tensors. ``out`` / ``scratch``: caller-provided output tensors (contiguous, of those shapes) and plane scratch."""
    global reconstruct_calls
    from .transforms import BatchStaging

    if len(coefficients) == 0:
        return []
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("probpose_code_amd.jpeg.reconstruct_batch runs on the GPU only (no CPU fallback)")
    args, out, _ = _stage(coefficients, device, staging if staging is not None else BatchStaging(), out, scratch)
    _lib.call("pp_jpeg_reconstruct_bgr_batch", *args, torch.cuda.current_stream(device).cuda_stream)
    reconstruct_calls += 1
    return out


def imread_device(path_or_bytes: Union[str, bytes], device="cuda", staging=None, entropy: str = "host") -> torch.Tensor:
    """A file (path or bytes) as the (H, W, 3) uint8 BGR device tensor ``torch.from_numpy(load_image_bgr(path)).to(device)``
    gives, decoded on the device where the file is inside the subset. Any other file goes through ``load_image_bgr`` and an
    upload: the same pixels, the same exceptions. ``entropy``: "host" (Huffman decoding on the host) or "device"
    (``decode_batch``'s device path for this one file)."""
    global fallbacks
    if entropy not in ENTROPY:
        raise ValueError(f"entropy must be one of {ENTROPY}, got {entropy!r}")
    if entropy == "device":
        return decode_batch([path_or_bytes], device, entropy="device", staging=staging)[0]
    try:
        c = entropy_decode(path_or_bytes)
    except (JpegUnsupported, OSError):  # (an unreadable path: the host decoder raises what it always raised)
        fallbacks += 1
        return torch.from_numpy(_host_decode(path_or_bytes)).to(device)
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
    prepares the files (``scan_prepare``), their bytes go up in one copy, ``pp_jpeg_huffman_decode_batch`` and
    ``pp_jpeg_reconstruct_bgr_batch`` run on the current stream, and the result slots come back in one copy. A file the
    preparation refuses goes the ``entropy="host"`` way; an image whose slot is not ``PP_OK`` (not synchronised within
    ``sync_passes``, a damaged stream) goes through ``entropy_decode`` - or, outside its subset, through the host decoder - and
    is counted in ``fallbacks`` and in ``unsynchronised``. Pixels and exceptions are those of ``imread_device``."""
    global fallbacks
    from .transforms import BatchStaging

    if entropy not in ENTROPY:
        raise ValueError(f"entropy must be one of {ENTROPY}, got {entropy!r}")
    if isinstance(files, (str, bytes, bytearray, memoryview, np.ndarray)):
        raise ValueError("decode_batch takes a sequence of files; imread_device takes one")
    files = list(files)
    device = torch.device(device)
    staging = staging if staging is not None else BatchStaging()
    out = [None] * len(files)
    scans, coefs = [], []
    for i, f in enumerate(files):
        try:
            if entropy == "device":
                raw = _bytes_of(f)
                try:
                    scans.append((i, scan_prepare(raw)))
                    continue
                except JpegUnsupported:
                    pass
                coefs.append((i, entropy_decode(raw)))
            else:
                coefs.append((i, entropy_decode(f)))
        except (JpegUnsupported, OSError):  # (an unreadable path: the host decoder raises what it always raised)
            fallbacks += 1
            out[i] = torch.from_numpy(_host_decode(f)).to(device)
    if scans:
        for (i, _), t in zip(scans, decode_scans([s for _, s in scans], device, staging, sync_passes)):
            out[i] = t
    if coefs:
        for (i, _), t in zip(coefs, reconstruct_batch([c for _, c in coefs], device, staging)):
            out[i] = t
    return out


def decode_or_host(path: str):
    """A worker's share of the test loop: the file's coefficients, or - outside the subset - its pixels from the host decoder."""
    try:
        return entropy_decode(path)
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


def entropy_encode(coefficients: JpegCoefficients, restart_interval: int = 0) -> bytes:
    """The host half of the encoder: the baseline JFIF file of ``coefficients`` (three components, tables (3, 64) with values
    1..255). Thread-safe and GIL-free while it codes."""
    info, coef = coefficients.info, np.ascontiguousarray(coefficients.coef, np.int16)
    qt = np.ascontiguousarray(coefficients.qtables, np.uint16)
    if qt.shape != (3, 64) or coef.size != info.coef_count:
        raise ValueError("the encoder takes three (64,) tables and info.coef_count coefficients")
    if not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"restart_interval must be in 0..65535, got {restart_interval!r}")
    bound = int(_lib.lib.pp_jpeg_encoded_bound(ctypes.byref(info)))
    if bound < 0:
        raise _lib.ProbPoseLibraryError("pp_jpeg_encoded_bound", _lib.lib.pp_status_string(bound).decode(), _lib.last_error())
    out = np.empty(bound, np.uint8)
    size = ctypes.c_size_t(0)
    _lib.call("pp_jpeg_entropy_encode", coef.ctypes.data, qt.ctypes.data, ctypes.byref(info), int(restart_interval), out.ctypes.data,
              out.size, ctypes.byref(size))
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
    dev = dev if dev is not None else torch.device(device or "cuda")
    if dev.type != "cuda":
        raise RuntimeError("probpose_code_amd.jpeg.encode_batch runs on the GPU only (no CPU fallback)")
    out = []
    for im in checked:
        im = im.to(dev)  # a host array is uploaded first
        if im.stride(2) != 1 or im.stride(1) != 3 or im.stride(0) < 3 * im.shape[1] or im.stride(0) >= 2 ** 31:
            im = im.contiguous()  # (a view of whole rows, such as a vertical crop, is read in place)
        out.append(im)
    return out, dev


def _stage_encode(images, qt, subsampling, channel_order, dev, staging, entropy=False):
    """Pack the descriptor table and the tables of a batch into the pinned buffer and upload them with one copy. Returns (the
    arguments of ``pp_jpeg_forward_batch``, (device block, pinned buffer, first and last byte of the coefficients in both, each
    image's offset, the infos), the tensors the launches use). ``entropy``: the table and result slots of
    ``pp_jpeg_entropy_encode_batch`` travel in the same copy; the returned tuple then ends with an ``_EntropyJob``."""
    n = len(images)
    infos = [encode_plan(im.shape[1], im.shape[0], subsampling) for im in images]
    # the block: descriptors (n x 64 bytes) | quantisation tables (3 x 64 u16) | with entropy: its descriptors (n x 64 bytes),
    # result slots (n x 16 bytes) | per image: coefficients (int16)
    o_qt = _align(64 * n)
    o_ent = _align(o_qt + 384)
    o_res = _align(o_ent + 64 * n) if entropy else o_ent
    off, o_coef = (_align(o_res + 16 * n) if entropy else o_ent), []
    for info in infos:
        o_coef.append(off)
        off = _align(off + 2 * int(info.coef_count))
    total, head = off, o_coef[0]
    scratch = torch.empty(sum(_align(int(i.coef_count)) for i in infos), dtype=torch.uint8, device=dev)
    block = torch.empty(total, dtype=torch.uint8, device=dev)
    blk = staging.acquire(total)
    desc = blk[:64 * n].view(_ENC_DESC)
    blk[o_qt:o_qt + 384].view(np.uint16)[:] = qt.reshape(-1)
    base, planes = block.data_ptr(), scratch.data_ptr()
    for i, (im, info) in enumerate(zip(images, infos)):
        desc[i] = (im.data_ptr(), base + o_qt, planes, base + o_coef[i], info.width, info.height, im.stride(0), int(channel_order == "rgb"),
                   info.hs, info.vs, info.mcus_x, info.mcus_y)
        planes += _align(int(info.coef_count))
    job = None
    if entropy:
        blk[o_res:o_res + 16 * n] = 0
        job = _entropy_job(blk[o_ent:o_ent + 64 * n].view(_ENT_DESC), infos, [base + o for o in o_coef], block[o_res:o_res + 16 * n], dev)
    staging.upload(block, head)
    args = (base, n, max(int(i.coef_count) // 64 for i in infos), max(int(i.height) for i in infos), max(int(i.width) for i in infos))
    if entropy:
        return args, (block, blk, head, total, o_coef, infos), (images, block, scratch), (base + o_ent, job)
    return args, (block, blk, head, total, o_coef, infos), (images, block, scratch)


def write_headers(qtables: np.ndarray, info: JpegInfo, restart_interval: int = 0) -> bytes:
    """The bytes SOI .. SOS of the file ``entropy_encode`` writes for these tables and this geometry (one code path)."""
    qt = np.ascontiguousarray(qtables, np.uint16)
    if qt.shape != (3, 64):
        raise ValueError("the encoder takes three (64,) tables")
    out = np.empty(1024, np.uint8)
    size = ctypes.c_size_t(0)
    _lib.call("pp_jpeg_write_headers", qt.ctypes.data, ctypes.byref(info), int(restart_interval), out.ctypes.data, out.size, ctypes.byref(size))
    return out[:size.value].tobytes()


class _EntropyJob(NamedTuple):
    """The device buffers of one ``pp_jpeg_entropy_encode_batch`` call: ``results`` (n x 16 bytes, a view of the uploaded
    block), the streams (``out``: image i's at ``o_out[i]``, ``capacity[i]`` bytes), the scratch, and the infos."""

    results: torch.Tensor
    out: torch.Tensor
    o_out: list
    capacity: list
    scratch: torch.Tensor
    infos: list


def _entropy_job(desc: np.ndarray, infos, coef_ptrs, results: torch.Tensor, dev) -> "_EntropyJob":
    """Allocate the scratch and the stream buffers of a batch and fill ``desc`` (a host view of n ``_ENT_DESC`` rows that
    the caller uploads). A stream gets ``pp_jpeg_encoded_bound`` bytes: no stream of its geometry is longer."""
    shares, capacity = [], []
    for info in infos:
        one = int(_lib.lib.pp_jpeg_entropy_scratch_bytes(ctypes.byref(info), 1))
        bound = int(_lib.lib.pp_jpeg_encoded_bound(ctypes.byref(info)))
        if one < 0 or bound < 0:
            raise _lib.ProbPoseLibraryError("pp_jpeg_entropy_scratch_bytes", _lib.lib.pp_status_string(min(one, bound)).decode(), _lib.last_error())
        shares.append(one)
        capacity.append(_align(bound))
    scratch = torch.empty(sum(shares), dtype=torch.uint8, device=dev)
    out = torch.empty(sum(capacity), dtype=torch.uint8, device=dev)
    o_out, s_at, o_at = [], scratch.data_ptr(), 0
    for i, info in enumerate(infos):
        desc[i] = (coef_ptrs[i], s_at, out.data_ptr() + o_at, results.data_ptr() + 16 * i, capacity[i], info.hs, info.vs, info.mcus_x,
                   info.mcus_y, 0)
        o_out.append(o_at)
        s_at += shares[i]
        o_at += capacity[i]
    return _EntropyJob(results, out, o_out, capacity, scratch, list(infos))


def _entropy_launch(desc_ptr: int, job: "_EntropyJob", stream) -> None:
    global entropy_device_calls
    _lib.call("pp_jpeg_entropy_encode_batch", desc_ptr, len(job.infos), max(int(i.coef_count) // 64 for i in job.infos), stream.cuda_stream)
    entropy_device_calls += 1


def _entropy_collect(job: "_EntropyJob", qtables, stream, staging) -> List[bytes]:
    """The files of a coded batch: the result slots first (one copy, one synchronisation), then the used bytes of every
    stream into the pinned buffer (one copy per image, one synchronisation), each between its headers and ``FF D9``."""
    res = job.results.cpu().numpy().view(_ENT_RESULT)  # (waits for the stream: the launches have run)
    for i, r in enumerate(res):
        if int(r["status"]) != _lib.PP_OK:
            why = ("a coefficient no baseline code expresses (DC difference outside -2047..2047 or AC outside -1023..1023)"
                   if int(r["status"]) == _lib.PP_ERR_INVALID_ARG else f"the stream needs {int(r['bytes'])} bytes, {job.capacity[i]} were given")
            raise _lib.ProbPoseLibraryError("pp_jpeg_entropy_encode_batch", _lib.lib.pp_status_string(int(r["status"])).decode(), f"image {i}: {why}")
    sizes = [int(r["bytes"]) for r in res]
    at, offs = 0, []
    for sz in sizes:
        offs.append(at)
        at += _align(sz)
    blk = staging.acquire(max(at, 1))
    for o, sz, oo in zip(offs, sizes, job.o_out):
        staging.buf[o:o + sz].copy_(job.out[oo:oo + sz], non_blocking=True)
    stream.synchronize()
    return [write_headers(qt, info) + blk[o:o + sz].tobytes() + b"\xff\xd9" for qt, info, o, sz in zip(qtables, job.infos, offs, sizes)]


def entropy_encode_device(coefficients: Sequence[JpegCoefficients], device=None, staging=None) -> List[bytes]:
    """The files ``entropy_encode`` gives for a list of ``JpegCoefficients`` (three components, geometry of ``encode_plan``),
    coded on the device: the coefficient arrays are uploaded with the table in one copy, then ONE
    ``pp_jpeg_entropy_encode_batch`` call (seven launches) on the current stream. Invalid coefficients raise what
    ``entropy_encode`` raises for them (``ProbPoseLibraryError``, PP_ERR_INVALID_ARG)."""
    from .transforms import BatchStaging

    coefficients = list(coefficients)
    n = len(coefficients)
    if n == 0:
        return []
    dev = torch.device(device or "cuda")
    if dev.type != "cuda":
        raise RuntimeError("probpose_code_amd.jpeg.entropy_encode_device runs on the GPU only (no CPU fallback)")
    staging = staging if staging is not None else BatchStaging()
    infos, qts = [], []
    for c in coefficients:
        coef, qt = np.asarray(c.coef), np.ascontiguousarray(c.qtables, np.uint16)
        if qt.shape != (3, 64) or coef.size != c.info.coef_count or coef.dtype != np.int16:
            raise ValueError("the encoder takes three (64,) tables and info.coef_count int16 coefficients")
        write_headers(qt, c.info)  # (refuses an info that is no encode_plan result, and tables outside 1..255, before any GPU work)
        infos.append(c.info)
        qts.append(qt)
    # the block: descriptors (n x 64 bytes) | result slots (n x 16 bytes) | per image: coefficients (int16)
    o_res = _align(64 * n)
    off, o_coef = _align(o_res + 16 * n), []
    for info in infos:
        o_coef.append(off)
        off = _align(off + 2 * int(info.coef_count))
    block = torch.empty(off, dtype=torch.uint8, device=dev)
    blk = staging.acquire(off)
    blk[o_res:o_res + 16 * n] = 0
    for o, c in zip(o_coef, coefficients):
        blk[o:o + 2 * c.coef.size].view(np.int16)[:] = np.asarray(c.coef).reshape(-1)
    base = block.data_ptr()
    job = _entropy_job(blk[:64 * n].view(_ENT_DESC), infos, [base + o for o in o_coef], block[o_res:o_res + 16 * n], dev)
    staging.upload(block, off)
    stream = torch.cuda.current_stream(dev)
    _entropy_launch(base, job, stream)
    return _entropy_collect(job, qts, stream, staging)


def forward_batch(images: Sequence, quality: int = 75, subsampling: str = "4:2:0", channel_order: str = "bgr", device=None,
                  staging=None, copy: bool = True) -> List[JpegCoefficients]:
    """The device half of the encoder for a batch of (H, W, 3) uint8 images of any mix of sizes: ONE
    ``pp_jpeg_forward_batch`` call (two launches) on the current stream, then one copy of all coefficients into the pinned
    buffer of ``staging`` (a ``transforms.BatchStaging``). Returns what ``entropy_decode`` gives for the finished files; with
    ``copy=False`` the coefficient arrays are views of the pinned buffer, valid until ``staging`` is used again."""
    global forward_calls
    from .transforms import BatchStaging

    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"channel_order must be 'bgr' or 'rgb', got {channel_order!r}")
    qt = quality_tables(quality)
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLING)}, got {subsampling!r}")
    images, dev = _encoder_images(list(images), device)
    n = len(images)
    if n == 0:
        return []
    staging = staging if staging is not None else BatchStaging()
    args, (block, blk, head, total, o_coef, infos), keep = _stage_encode(images, qt, subsampling, channel_order, dev, staging)
    stream = torch.cuda.current_stream(dev)
    _lib.call("pp_jpeg_forward_batch", *args, stream.cuda_stream)
    forward_calls += 1
    staging.buf[head:total].copy_(block[head:total], non_blocking=True)
    stream.synchronize()  # the coefficients are in the pinned buffer; images, block and scratch (``keep``) are no longer read
    del keep
    views = [blk[o:o + 2 * int(info.coef_count)].view(np.int16) for o, info in zip(o_coef, infos)]
    return [JpegCoefficients(info, v.copy() if copy else v, qt) for v, info in zip(views, infos)]


def encode_batch(images: Sequence, quality: int = 75, subsampling: str = "4:2:0", channel_order: str = "bgr", restart_interval: int = 0,
                 workers: int = 8, device=None, staging=None, entropy: str = "host") -> List[bytes]:
    """Baseline JPEG files of a batch of (H, W, 3) uint8 images (device tensors; a host array is uploaded first) of any mix
    of sizes: ``forward_batch`` on the device, then Huffman coding on a pool of ``workers`` host threads (at most
    ``runner.MAX_WORKERS``). ``quality`` 1..100, ``subsampling`` "4:4:4" / "4:2:2" / "4:2:0" and ``restart_interval`` (MCUs
    between restart markers, 0: none) mean what they mean to Pillow's ``Image.save``; ``channel_order``: "bgr" or "rgb"
    pixels. Each file decodes to the pixels Pillow's own file of that image decodes to.

    ``entropy="device"`` codes on the device instead (restart interval 0 only): the forward launches, then
    ``pp_jpeg_entropy_encode_batch`` on the same stream; the coefficients stay on the device and ``workers`` is not used. A
    batch of n images then costs one upload (tables and descriptors), 1 + n downloads (the result slots, then the used
    bytes of each stream) and two synchronisations, one after each kind of download. The files are byte for byte those
    of ``entropy="host"``; invalid coefficients raise the same ``ProbPoseLibraryError``."""
    from concurrent.futures import ThreadPoolExecutor

    from .runner import MAX_WORKERS

    if isinstance(restart_interval, bool) or not isinstance(restart_interval, (int, np.integer)) or not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"restart_interval must be an int in 0..65535, got {restart_interval!r}")
    if isinstance(images, (torch.Tensor, np.ndarray)):
        raise ValueError("encode_batch takes a sequence of (H, W, 3) images; imwrite_device takes one")
    if entropy not in ENTROPY:
        raise ValueError(f"entropy must be one of {ENTROPY}, got {entropy!r}")
    if entropy == "device":
        if int(restart_interval) != 0:
            raise ValueError("entropy='device' codes without restart intervals: restart_interval must be 0")
        return _encode_batch_device(images, quality, subsampling, channel_order, device, staging)
    coefs = forward_batch(images, quality, subsampling, channel_order, device, staging, copy=False)  # (coded before staging is used again)
    if len(coefs) <= 1 or int(workers) <= 1:
        return [entropy_encode(c, restart_interval) for c in coefs]
    with ThreadPoolExecutor(max_workers=max(1, min(MAX_WORKERS, int(workers), len(coefs)))) as pool:
        return list(pool.map(lambda c: entropy_encode(c, restart_interval), coefs))


def _encode_batch_device(images, quality, subsampling, channel_order, device, staging) -> List[bytes]:
    """``encode_batch`` with both halves on the device: nine launches on the current stream, no coefficient copy."""
    global forward_calls
    from .transforms import BatchStaging

    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"channel_order must be 'bgr' or 'rgb', got {channel_order!r}")
    qt = quality_tables(quality)
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLING)}, got {subsampling!r}")
    images, dev = _encoder_images(list(images), device)
    if len(images) == 0:
        return []
    staging = staging if staging is not None else BatchStaging()
    args, _, keep, (ent_ptr, job) = _stage_encode(images, qt, subsampling, channel_order, dev, staging, entropy=True)
    stream = torch.cuda.current_stream(dev)
    _lib.call("pp_jpeg_forward_batch", *args, stream.cuda_stream)
    forward_calls += 1
    _entropy_launch(ent_ptr, job, stream)
    files = _entropy_collect(job, [qt] * len(images), stream, staging)
    del keep
    return files


def imwrite_device(path: str, image, **kw) -> None:
    """One picture written as a baseline JPEG file by ``encode_batch`` (its keyword arguments, ``entropy`` among them)."""
    data = encode_batch([image], **kw)[0]
    with open(path, "wb") as f:
        f.write(data)
