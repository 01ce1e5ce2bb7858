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
"""
import ctypes
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib

fallbacks = 0  # files imread_device / the test loop handed to the host decoder since import (diagnostics)
reconstruct_calls = 0  # pp_jpeg_reconstruct_bgr_batch calls since import
forward_calls = 0  # pp_jpeg_forward_batch calls since import


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


def _stage_encode(images, qt, subsampling, channel_order, dev, staging):
    """Pack the descriptor table and the tables of a batch into the pinned buffer and upload them with one copy. Returns (the
    arguments of ``pp_jpeg_forward_batch``, (device block, pinned buffer, first and last byte of the coefficients in both, each
    image's offset, the infos), the tensors the launches use)."""
    n = len(images)
    infos = [encode_plan(im.shape[1], im.shape[0], subsampling) for im in images]
    # the block: descriptors (n x 64 bytes) | quantisation tables (3 x 64 u16) | per image: coefficients (int16)
    o_qt = _align(64 * n)
    off, o_coef = _align(o_qt + 384), []
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
    staging.upload(block, head)
    args = (base, n, max(int(i.coef_count) // 64 for i in infos), max(int(i.height) for i in infos), max(int(i.width) for i in infos))
    return args, (block, blk, head, total, o_coef, infos), (images, block, scratch)


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
                 workers: int = 8, device=None, staging=None) -> List[bytes]:
    """Baseline JPEG files of a batch of (H, W, 3) uint8 images (device tensors; a host array is uploaded first) of any mix
    of sizes: ``forward_batch`` on the device, then Huffman coding on a pool of ``workers`` host threads (at most
    ``runner.MAX_WORKERS``). ``quality`` 1..100, ``subsampling`` "4:4:4" / "4:2:2" / "4:2:0" and ``restart_interval`` (MCUs
    between restart markers, 0: none) mean what they mean to Pillow's ``Image.save``; ``channel_order``: "bgr" or "rgb"
    pixels. Each file decodes to the pixels Pillow's own file of that image decodes to."""
    from concurrent.futures import ThreadPoolExecutor

    from .runner import MAX_WORKERS

    if isinstance(restart_interval, bool) or not isinstance(restart_interval, (int, np.integer)) or not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"restart_interval must be an int in 0..65535, got {restart_interval!r}")
    if isinstance(images, (torch.Tensor, np.ndarray)):
        raise ValueError("encode_batch takes a sequence of (H, W, 3) images; imwrite_device takes one")
    coefs = forward_batch(images, quality, subsampling, channel_order, device, staging, copy=False)  # (coded before staging is used again)
    if len(coefs) <= 1 or int(workers) <= 1:
        return [entropy_encode(c, restart_interval) for c in coefs]
    with ThreadPoolExecutor(max_workers=max(1, min(MAX_WORKERS, int(workers), len(coefs)))) as pool:
        return list(pool.map(lambda c: entropy_encode(c, restart_interval), coefs))


def imwrite_device(path: str, image, **kw) -> None:
    """One picture written as a baseline JPEG file by ``encode_batch`` (its keyword arguments)."""
    data = encode_batch([image], **kw)[0]
    with open(path, "wb") as f:
        f.write(data)
