"""PNG files written from the device: 8-bit truecolour (colour type 2), non-interlaced, one ``IDAT`` chunk, no ancillary
chunk - the lossless counterpart of ``jpeg.encode_batch`` for the pictures the visualizer draws on the GPU.

The format (csrc/pp_png_core.h states it in full). Every row takes, of the five PNG filters, the one with the smallest sum
of ``min(b, 256 - b)`` over its filtered bytes, the lowest number on a tie. The filtered stream is cut into tiles of 4096
bytes; a run of equal bytes inside a tile becomes a literal and matches of length 3..258 at distance 1 - the only LZ77
matches this coder finds. The tokens of a picture are one dynamic deflate block under a Huffman code built from the
picture's own histogram. Any decoder opens the files; they are not the bytes another encoder would write.

``encode_batch`` runs the filters, the token histogram, the bit packing and both checksums on the device (csrc/pp_png.hip:
three launches, then five). Between the two halves the host reads the histograms of the whole batch in one copy, builds
each picture's code and header (``pp_deflate_build_code``) and uploads them in one copy: one synchronisation more than the
JPEG coder needs. ``encode_host`` is the sequential form of the same core (``pp_png_encode``) and gives the same bytes.
``zlib_compress_device`` is the deflate stage alone on raw byte strings. Opt-in: ``PoseLocalVisualizer(png_encoder="device")``,
``--encode-png device`` of demo/image_demo.py.

``match="lz"`` (every entry point takes it; ``"runs"``, the default, is the coder above and gives the bytes it always gave)
adds matches one pixel back (distance 3) and one row back (distance ``P = 1 + 3 * width`` and ``P - 3``, ``P + 3``; for a raw
stream ``period=`` gives ``P``), chosen by a greedy rule with a one-byte lookahead that csrc/pp_png_core.h states in full,
and a second Huffman code for the distances. Which positions start a token then depends on the whole chain before them in
the tile; the kernel resolves the chain by pointer doubling in LDS and stores the parse once. Still eight launches
(``LAUNCHES_TOKENS_LZ``, ``LAUNCHES_DEFLATE_LZ``), still the host form's bytes. Opt-in: ``png_match="lz"`` of the
visualizer, ``--png-match lz`` of the demo.

``code="device"`` (``encode_batch``, ``zlib_compress_device``, ``imwrite_device``; ``"host"``, the default, is the round trip
above) builds the codes on the device instead: one launch more (``LAUNCHES_CODE`` / ``LAUNCHES_CODE_LZ``: a workgroup per
stream runs the steps of csrc/pp_png_code_core.h in LDS) between the halves, nine launches in all, no histogram download,
no host build, no code upload, two synchronisations instead of three - and the same bytes, since the kernel gives the
``pp_deflate_code`` of the host builder byte for byte. Opt-in: ``png_code="device"`` of the visualizer, ``--png-code device``
of the demo.

Not done: alpha, grey, palette, 16-bit and Adam7 pictures; a hash-table or general-window matcher (``lz`` mode finds a
repeat only at the pixel and row distances above, so a picture whose repeats lie elsewhere stays larger than from zlib);
lazy matching beyond one byte; reading PNG files (inflate); choosing ``code=`` by the batch's shape.
"""
import ctypes
import struct
import zlib
from typing import List, NamedTuple, Sequence

import numpy as np
import torch

from . import _lib
from .staging import BatchStaging, StagedBlock, _align

host_calls = 0  # pp_png_encode / pp_zlib_compress calls since import
tokens_calls = 0  # pp_png_tokens_batch calls since import
deflate_calls = 0  # pp_png_deflate_batch calls since import
code_calls = 0  # pp_png_code_batch calls since import

# pp_deflate_desc: seven pointers, len, capacity, width, height, row_stride, rgb, crc_init, period (lz mode, raw streams); pp_deflate_result
_DESC = np.dtype([("pixels", "<u8"), ("data", "<u8"), ("hist", "<u8"), ("code", "<u8"), ("scratch", "<u8"), ("out", "<u8"), ("result", "<u8"),
                  ("len", "<i8"), ("capacity", "<i8"), ("width", "<i4"), ("height", "<i4"), ("row_stride", "<i8"), ("rgb", "<i4"),
                  ("crc_init", "<u4"), ("period", "<i8")])
assert _DESC.itemsize == 104
_RESULT = np.dtype([("bytes", "<i8"), ("status", "<i4"), ("crc", "<u4")])
assert _RESULT.itemsize == 16
HIST_BYTES = 4 * 288
CODE_BYTES = 1472  # sizeof(pp_deflate_code)
LAUNCHES_TOKENS = ("png_filter", "png_clear", "png_hist")  # pp_launch_count tags of pp_png_tokens_batch (png_filter: pictures only)
LAUNCHES_DEFLATE = ("png_bits", "png_scan", "png_zero", "png_pack", "png_crc")  # ... of pp_png_deflate_batch
HIST_BYTES_LZ = 4 * 320  # lz mode: the 288 words, then the counts of the 30 distance symbols
CODE_BYTES_LZ = 1600  # sizeof(pp_deflate_code_lz)
LAUNCHES_TOKENS_LZ = ("png_filter", "png_clear_lz", "png_parse_lz")  # ... of pp_png_tokens_batch_lz
LAUNCHES_DEFLATE_LZ = ("png_bits_lz", "png_scan_lz", "png_zero_lz", "png_pack_lz", "png_crc_lz")  # ... of pp_png_deflate_batch_lz
LAUNCHES_CODE = ("png_code",)  # ... of pp_png_code_batch (code="device": between the two halves)
LAUNCHES_CODE_LZ = ("png_code_lz",)  # ... of pp_png_code_batch_lz
_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_IDAT_REGISTER = ~zlib.crc32(b"IDAT") & 0xFFFFFFFF  # the CRC-32 register in front of the stream's first byte


def _check_order(channel_order) -> int:
    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"channel_order must be 'bgr' or 'rgb', got {channel_order!r}")
    return int(channel_order == "rgb")


def _check_match(match) -> bool:
    if match not in ("runs", "lz"):
        raise ValueError(f"match must be 'runs' or 'lz', got {match!r}")
    return match == "lz"


def _check_code(code) -> bool:
    if code not in ("host", "device"):
        raise ValueError(f"code must be 'host' or 'device', got {code!r}")
    return code == "device"


def _check_period(period, lz: bool) -> int:
    """The row period of a raw stream; runs mode ignores it."""
    if not lz:
        return 0
    if not isinstance(period, (int, np.integer)) or isinstance(period, bool) or period < 0:
        raise ValueError(f"period must be an integer >= 0, got {period!r}")
    return int(period)


def _check_picture(im) -> None:
    """ValueError for anything but an (H, W, 3) uint8 array or tensor that one file holds."""
    if not isinstance(im, (np.ndarray, torch.Tensor)):
        raise ValueError(f"the encoder takes (H, W, 3) uint8 images, got {type(im).__name__}")
    if im.dtype != (np.uint8 if isinstance(im, np.ndarray) else torch.uint8) or len(im.shape) != 3 or im.shape[2] != 3:
        raise ValueError(f"the encoder takes (H, W, 3) uint8 images, got {tuple(im.shape)} {im.dtype}")
    if im.shape[0] == 0 or im.shape[1] == 0:
        raise ValueError("empty image")
    if im.shape[0] > 65535 or im.shape[1] > 65535:
        raise ValueError(f"this writer holds at most 65535 pixels a side, got {im.shape[1]} x {im.shape[0]}")
    if _lib.lib.pp_png_encoded_bound(int(im.shape[1]), int(im.shape[0])) < 0:
        raise ValueError(f"a {im.shape[1]} x {im.shape[0]} picture needs a stream of 2^31 bytes or more")


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _frame(width: int, height: int, stream: bytes, register: int) -> bytes:
    """The file around a zlib stream; ``register``: the CRC-32 register behind "IDAT" and the stream (pp_deflate_result.crc)."""
    return (_SIGNATURE + _chunk(b"IHDR", struct.pack(">II5B", width, height, 8, 2, 0, 0, 0)) + struct.pack(">I", len(stream)) + b"IDAT" + stream
            + struct.pack(">I", ~register & 0xFFFFFFFF) + _chunk(b"IEND", b""))


def encode_host(image, channel_order: str = "bgr", match: str = "runs") -> bytes:
    """The PNG file of one (H, W, 3) uint8 picture, written on the host by the sequential form of the core the kernels run
    (``pp_png_encode``, ``pp_png_encode_lz``): the bytes ``encode_batch`` gives in the same ``match`` mode. No GPU is used."""
    global host_calls
    rgb = _check_order(channel_order)
    lz = _check_match(match)
    _check_picture(image)
    px = np.ascontiguousarray(image.cpu().numpy() if isinstance(image, torch.Tensor) else image)
    h, w = px.shape[:2]
    bound = _size("pp_deflate_bound_lz", _lib.lib.pp_deflate_bound_lz(h * (1 + 3 * w))) + 57 if lz else _lib.lib.pp_png_encoded_bound(w, h)
    out = np.empty(int(bound), np.uint8)
    size = ctypes.c_size_t(0)
    _lib.call("pp_png_encode_lz" if lz else "pp_png_encode", px.ctypes.data, w, h, 3 * w, rgb, out.ctypes.data, out.size, ctypes.byref(size))
    host_calls += 1
    return out[:size.value].tobytes()


def _raw(buffer) -> np.ndarray:
    raw = np.frombuffer(bytes(buffer), np.uint8) if isinstance(buffer, (bytes, bytearray, memoryview)) else buffer
    if not isinstance(raw, np.ndarray) or raw.dtype != np.uint8 or raw.ndim != 1:
        raise ValueError("the deflate stage takes bytes or one-dimensional uint8 arrays")
    if raw.size == 0 or _lib.lib.pp_deflate_bound(raw.size) < 0:
        raise ValueError(f"the deflate stage takes streams of 1 .. 2^31 - 1 bytes whose bound stays below 2^31, got {raw.size}")
    return np.ascontiguousarray(raw)


def zlib_compress_host(buffer, return_tokens: bool = False, match: str = "runs", period: int = 0):
    """The zlib stream of a byte string by the host form of the deflate stage (``pp_zlib_compress``, ``pp_zlib_compress_lz``);
    with ``return_tokens`` also the number of literals and matches in it. ``period``: the row period of ``match="lz"`` (0: near
    candidates only); runs mode ignores it."""
    global host_calls
    raw = _raw(buffer)
    lz = _check_match(match)
    period = _check_period(period, lz)
    size, tokens = ctypes.c_size_t(0), ctypes.c_longlong(0)
    if lz:
        out = np.empty(_size("pp_deflate_bound_lz", _lib.lib.pp_deflate_bound_lz(raw.size)), np.uint8)
        _lib.call("pp_zlib_compress_lz", raw.ctypes.data, raw.size, period, out.ctypes.data, out.size, ctypes.byref(size), ctypes.byref(tokens))
    else:
        out = np.empty(int(_lib.lib.pp_deflate_bound(raw.size)), np.uint8)
        _lib.call("pp_zlib_compress", raw.ctypes.data, raw.size, out.ctypes.data, out.size, ctypes.byref(size), ctypes.byref(tokens))
    host_calls += 1
    data = out[:size.value].tobytes()
    return (data, int(tokens.value)) if return_tokens else data


def _size(query: str, value) -> int:
    if value < 0:
        raise _lib.ProbPoseLibraryError(query, _lib.lib.pp_status_string(int(value)).decode(), _lib.last_error())
    return int(value)


class _Job(NamedTuple):
    """One batch on the device: ``block`` (the uploaded ``StagedBlock``: descriptors, result slots, histograms, codes, raw
    streams), ``lens`` (the stream lengths), ``max_height`` (0 for raw streams), the zlib streams (``out``: stream i's at
    ``o_out[i]``, ``capacity[i]`` bytes), ``keep`` (the other tensors the launches use) and ``lz`` (the match mode)."""

    block: StagedBlock
    lens: list
    max_height: int
    out: torch.Tensor
    o_out: list
    capacity: list
    keep: tuple
    lz: bool = False


def _stage(pictures, raws, rgb: int, dev, staging, lz: bool = False, period: int = 0) -> _Job:
    """Allocate the buffers of a batch of pictures (device tensors with dense pixel rows) or of raw streams (uint8 arrays),
    fill the descriptor table and upload it - with the raw streams - in one copy. lz: the match mode of the whole batch;
    period: the row period of its raw streams."""
    n = len(pictures) if pictures is not None else len(raws)
    lens = [im.shape[0] * (1 + 3 * im.shape[1]) for im in pictures] if pictures is not None else [int(r.size) for r in raws]
    q_scratch, q_bound = ("pp_deflate_scratch_bytes_lz", "pp_deflate_bound_lz") if lz else ("pp_deflate_scratch_bytes", "pp_deflate_bound")
    hist_bytes, code_bytes = (HIST_BYTES_LZ, CODE_BYTES_LZ) if lz else (HIST_BYTES, CODE_BYTES)
    shares = [_size(q_scratch, getattr(_lib.lib, q_scratch)(ln)) for ln in lens]
    capacity = [_align(_size(q_bound, getattr(_lib.lib, q_bound)(ln))) for ln in lens]
    # the block: descriptors (n x 104 bytes) | result slots (n x 16) | histograms (n x 288 u32, lz: 320, written on the device,
    # read back in one copy) | codes (n x pp_deflate_code, lz: pp_deflate_code_lz, uploaded in one copy once they are built) |
    # per raw stream: its bytes
    blk = StagedBlock([("desc", 104 * n), ("results", 16 * n), ("hist", hist_bytes * n), ("code", code_bytes * n)],
                      [("data", [0] * n if pictures is not None else lens)])
    scratch = torch.empty(sum(shares), dtype=torch.uint8, device=dev)
    out = torch.empty(sum(capacity), dtype=torch.uint8, device=dev)
    filtered = torch.empty(sum(_align(ln) for ln in lens), dtype=torch.uint8, device=dev) if pictures is not None else None
    blk.acquire(staging, dev)
    rows, p_results, p_hist, p_code, p_data = blk.host("desc", _DESC), blk.ptr("results"), blk.ptr("hist"), blk.ptr("code"), blk.ptrs("data")
    blk.host("results")[:] = 0
    s_at, o_at, f_at, o_out = scratch.data_ptr(), 0, (filtered.data_ptr() if pictures is not None else 0), []
    for i in range(n):
        if pictures is not None:
            im = pictures[i]
            pixels, data, w, h, stride = im.data_ptr(), f_at, im.shape[1], im.shape[0], im.stride(0)
            f_at += _align(lens[i])
        else:
            blk.hosts("data")[i][:] = raws[i]
            pixels, data, w, h, stride = 0, p_data[i], 0, 0, 0
        rows[i] = (pixels, data, p_hist + hist_bytes * i, p_code + code_bytes * i, s_at, out.data_ptr() + o_at, p_results + 16 * i, lens[i],
                   capacity[i], w, h, stride, rgb, _IDAT_REGISTER, period if pictures is None else 0)
        o_out.append(o_at)
        s_at += shares[i]
        o_at += capacity[i]
    blk.upload()
    return _Job(blk, lens, max(im.shape[0] for im in pictures) if pictures is not None else 0, out, o_out, capacity, (pictures, scratch, filtered), lz)


def _launch_tokens(job: _Job, stream) -> None:
    global tokens_calls
    _lib.call("pp_png_tokens_batch_lz" if job.lz else "pp_png_tokens_batch", job.block.base, len(job.lens), job.max_height, max(job.lens), stream.cuda_stream)
    tokens_calls += 1


def _launch_deflate(job: _Job, stream) -> None:
    global deflate_calls
    _lib.call("pp_png_deflate_batch_lz" if job.lz else "pp_png_deflate_batch", job.block.base, len(job.lens), max(job.lens), stream.cuda_stream)
    deflate_calls += 1


def _launch_code(job: _Job, stream) -> None:
    global code_calls
    _lib.call("pp_png_code_batch_lz" if job.lz else "pp_png_code_batch", job.block.base, len(job.lens), stream.cuda_stream)
    code_calls += 1


def _build_codes_host(job: _Job, stream) -> None:
    """The histograms down (one copy, one synchronisation), the codes built in the pinned buffer, the codes up (one copy)."""
    blk, n = job.block, len(job.lens)
    hist_bytes, code_bytes, build = (HIST_BYTES_LZ, CODE_BYTES_LZ, "pp_deflate_build_code_lz") if job.lz else (HIST_BYTES, CODE_BYTES, "pp_deflate_build_code")
    staging = blk.staging
    o_h, o_c = blk.offset["hist"], blk.offset["code"]
    staging.buf[o_h:o_h + hist_bytes * n].copy_(blk.dev[o_h:o_h + hist_bytes * n], non_blocking=True)
    stream.synchronize()
    hist, code = blk.host("hist").ctypes.data, blk.host("code").ctypes.data
    for i in range(n):
        _lib.call(build, hist + hist_bytes * i, code + code_bytes * i)
    blk.dev[o_c:o_c + code_bytes * n].copy_(staging.buf[o_c:o_c + code_bytes * n], non_blocking=True)
    staging.ev.record(stream)  # (the next user of the pinned buffer waits for this copy)


def _run(job: _Job, device_code: bool = False) -> list:
    """Both halves of a staged batch on the current stream and the code build between them - on the host, or with
    ``device_code`` by one launch more and nothing else: (zlib stream, CRC-32 register) per entry."""
    blk = job.block
    staging, stream = blk.staging, torch.cuda.current_stream(blk.dev.device)
    _launch_tokens(job, stream)
    if device_code:
        _launch_code(job, stream)
    else:
        _build_codes_host(job, stream)
    _launch_deflate(job, stream)
    res = blk.device("results").cpu().numpy().view(_RESULT)  # (waits for the stream: the launches have run)
    for i, r in enumerate(res):
        if int(r["status"]) != _lib.PP_OK:
            raise _lib.ProbPoseLibraryError("pp_png_deflate_batch_lz" if job.lz else "pp_png_deflate_batch", _lib.lib.pp_status_string(int(r["status"])).decode(),
                                            f"stream {i}: it needs {int(r['bytes'])} bytes, {job.capacity[i]} were given")
    sizes = [int(r["bytes"]) for r in res]
    at, offs = 0, []
    for sz in sizes:
        offs.append(at)
        at += _align(sz)
    pinned = staging.acquire(max(at, 1))
    for o, sz, oo in zip(offs, sizes, job.o_out):
        staging.buf[o:o + sz].copy_(job.out[oo:oo + sz], non_blocking=True)
    stream.synchronize()
    return [(pinned[o:o + sz].tobytes(), int(r["crc"])) for o, sz, r in zip(offs, sizes, res)]


def encode_batch(images: Sequence, channel_order: str = "bgr", device=None, staging=None, match: str = "runs", code: str = "host") -> List[bytes]:
    """PNG files of a batch of (H, W, 3) uint8 pictures (device tensors; a host array is uploaded first) of any mix of sizes,
    ``channel_order`` "bgr" or "rgb" in memory. Filters, tokens, bit packing and checksums run on the device: a batch of n
    pictures costs one upload (descriptors), the histogram round trip (one download, the codes built on the host, one
    upload), then 1 + n downloads (the result slots, then the used bytes of each stream) - three synchronisations - and
    eight launches whatever n is, in either ``match`` mode. With ``code="device"`` the codes are built by a ninth launch
    between the halves: no histogram download, no host build, no code upload, two synchronisations. The files are byte for
    byte those of ``encode_host`` in that ``match`` mode, whatever ``code`` is."""
    from .jpeg import _encoder_images

    rgb = _check_order(channel_order)
    lz = _check_match(match)
    device_code = _check_code(code)
    if isinstance(images, (torch.Tensor, np.ndarray)):
        raise ValueError("encode_batch takes a sequence of (H, W, 3) images; imwrite_device takes one")
    images = list(images)
    for im in images:
        _check_picture(im)
    if len(images) == 0:
        return []
    images, dev = _encoder_images(images, device)
    streams = _run(_stage(images, None, rgb, dev, staging if staging is not None else BatchStaging(), lz), device_code)
    return [_frame(im.shape[1], im.shape[0], z, register) for im, (z, register) in zip(images, streams)]


def zlib_compress_device(buffers: Sequence, device=None, staging=None, match: str = "runs", period: int = 0, code: str = "host") -> List[bytes]:
    """The deflate stage alone: the zlib streams of a batch of byte strings (bytes or one-dimensional uint8 arrays of at
    least one byte), coded on the device in seven launches (eight with ``code="device"``: the code build on the device, as in
    ``encode_batch``) - the streams ``zlib_compress_host`` gives with the same ``match`` and ``period`` (one period for the
    whole batch), which ``zlib.decompress`` turns back into the input."""
    from .jpeg import _cuda_device

    lz = _check_match(match)
    device_code = _check_code(code)
    period = _check_period(period, lz)
    if isinstance(buffers, (bytes, bytearray, memoryview, np.ndarray)):
        raise ValueError("zlib_compress_device takes a sequence of byte strings")
    raws = [_raw(b) for b in buffers]
    if len(raws) == 0:
        return []
    dev = _cuda_device(device or "cuda", "zlib_compress_device")
    return [z for z, _ in _run(_stage(None, raws, 0, dev, staging if staging is not None else BatchStaging(), lz, period), device_code)]


def imwrite_device(path: str, image, **kw) -> None:
    """One picture written as a PNG file by ``encode_batch`` (its keyword arguments, ``match`` and ``code`` among them)."""
    data = encode_batch([image], **kw)[0]
    with open(path, "wb") as f:
        f.write(data)
