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
"""
import ctypes
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib

fallbacks = 0  # files imread_device / the test loop handed to the host decoder since import (diagnostics)
reconstruct_calls = 0  # pp_jpeg_reconstruct_bgr_batch calls since import


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


def _align(v: int, a: int = 256) -> int:
    return (v + a - 1) // a * a


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


def imread_device(path_or_bytes: Union[str, bytes], device="cuda", staging=None) -> torch.Tensor:
    """A file (path or bytes) as the (H, W, 3) uint8 BGR device tensor ``torch.from_numpy(load_image_bgr(path)).to(device)``
    gives, decoded on the device where the file is inside the subset. Any other file goes through ``load_image_bgr`` and an
    upload: the same pixels, the same exceptions."""
    global fallbacks
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


def decode_or_host(path: str):
    """A worker's share of the test loop: the file's coefficients, or - outside the subset - its pixels from the host decoder."""
    try:
        return entropy_decode(path)
    except JpegUnsupported:
        return _host_decode(path)
