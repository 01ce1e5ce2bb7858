"""Motion-JPEG in an AVI container, written and read in pure Python: the file a video loop reads its frames from and writes
its drawn frames to without cv2. Every frame is a whole JPEG file (``jpeg.encode_batch`` writes them, ``jpeg.imread_device``
reads them), so the container only frames bytes:

    RIFF 'AVI '
      LIST 'hdrl'   avih (frame period, frame count, size)
        LIST 'strl' strh ('vids' / 'MJPG', rate / scale = fps, length)   strf (BITMAPINFOHEADER, biCompression 'MJPG', 24 bits)
      LIST 'movi'   '00dc' chunks, one per frame, padded to even length
      idx1          one entry per frame: '00dc', AVIIF_KEYFRAME, offset from the 'movi' fourcc, length

One video stream, no audio, AVI 1.0: the file ends below 2 GiB (``max_bytes``; OpenDML is not written or read)."""
import struct
from fractions import Fraction
from typing import Iterator, Tuple

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
_HEADER_BYTES = 224  # RIFF .. the 'movi' fourcc: the first frame chunk starts here
_MOVI_FOURCC_AT = 220


def jpeg_size(data: bytes) -> Tuple[int, int]:
    """(width, height) from the frame header (SOFn) of a JPEG file; ValueError for bytes that hold none."""
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise ValueError("not a JPEG file: no SOI marker")
    o = 2
    while o + 4 <= len(data):
        if data[o] != 0xFF:
            raise ValueError("not a JPEG file: marker expected")
        m = data[o + 1]
        if m == 0xFF:  # fill byte
            o += 1
            continue
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            o += 2
            continue
        size = (data[o + 2] << 8) | data[o + 3]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if size < 8 or o + 9 > len(data):
                break
            return (data[o + 7] << 8) | data[o + 8], (data[o + 5] << 8) | data[o + 6]
        if m == 0xDA or m == 0xD9:
            break
        o += 2 + size
    raise ValueError("not a JPEG file: no frame header before the scan")


class MjpegAviWriter:
    """``with MjpegAviWriter(path, fps) as w: w.write(jpeg_bytes)``. The first frame's SOF fixes width and height; a later
    frame of another size raises ``ValueError``. ``close()`` writes the index and patches the sizes and frame counts. A frame
    that would take the finished file past ``max_bytes`` raises ``ValueError`` before anything of it is written: the file
    stays closable and valid with the frames written so far."""

    def __init__(self, path: str, fps: float, max_bytes: int = 2 ** 31 - 1):
        rate = Fraction(fps).limit_denominator(100000)
        if not rate > 0 or rate.numerator >= 2 ** 32:
            raise ValueError(f"fps must be positive, got {fps!r}")
        if not _HEADER_BYTES + 8 <= int(max_bytes) <= 2 ** 31 - 1:
            raise ValueError(f"max_bytes must be in {_HEADER_BYTES + 8} .. 2^31 - 1 (AVI 1.0), got {max_bytes!r}")
        self.path, self.rate, self.max_bytes = path, rate, int(max_bytes)
        self.width = self.height = 0
        self.index = []  # (offset from the 'movi' fourcc, length) per frame
        self.largest = 0
        self._at = _HEADER_BYTES  # where the next chunk goes
        self._f = open(path, "wb")
        self._f.write(self._header())

    @property
    def frame_count(self) -> int:
        return len(self.index)

    def _header(self) -> bytes:
        n, w, h = len(self.index), self.width, self.height
        usec = int(round(1e6 * self.rate.denominator / self.rate.numerator))
        movi_bytes = self._at - _HEADER_BYTES + 4
        riff_bytes = self._at + 16 * n  # (the closed file is _at + 8 + 16 n bytes long)
        avih = struct.pack("<14I", usec, int(self.largest * float(self.rate)) & 0xFFFFFFFF, 0, AVIF_HASINDEX, n, 0, 1, self.largest, w, h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.rate.denominator, self.rate.numerator, 0, n, self.largest,
                           0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = (b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" +
                struct.pack("<I", movi_bytes) + b"movi")
        assert len(head) == _HEADER_BYTES and head[_MOVI_FOURCC_AT:] == b"movi"
        return head

    def write(self, jpeg_bytes: bytes) -> None:
        if self._f is None:
            raise ValueError("the writer is closed")
        data = bytes(jpeg_bytes)
        w, h = jpeg_size(data)
        if self.index and (w, h) != (self.width, self.height):
            raise ValueError(f"frame {len(self.index)} is {w} x {h}, the video is {self.width} x {self.height}")
        pad = len(data) & 1
        after = self._at + 8 + len(data) + pad + 8 + 16 * (len(self.index) + 1)  # the file's size were it closed behind this frame
        if after > self.max_bytes:
            raise ValueError(f"frame {len(self.index)} would take the file to {after} bytes, past max_bytes = {self.max_bytes}")
        if not self.index:
            self.width, self.height = w, h
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * pad)
        self.index.append((self._at - _MOVI_FOURCC_AT, len(data)))
        self.largest = max(self.largest, len(data))
        self._at += 8 + len(data) + pad

    def close(self) -> None:
        if self._f is None:
            return
        f, self._f = self._f, None
        try:
            f.write(b"idx1" + struct.pack("<I", 16 * len(self.index)))
            f.write(b"".join(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, off, size) for off, size in self.index))
            f.seek(0)
            f.write(self._header())
        finally:
            f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class MjpegAvi:
    """What ``read_mjpeg_avi`` returns: ``fps``, ``width``, ``height``, ``frame_count`` from the headers; iterating yields each
    frame's JPEG bytes in file order by walking the 'movi' list (the index is not needed and not read)."""

    def __init__(self, path: str):
        self.path = path
        with open(path, "rb") as f:
            head = f.read(12)
            if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
                raise ValueError(f"{path}: not a RIFF AVI file")
            f.seek(0, 2)
            self._end = min(f.tell(), 8 + struct.unpack("<I", head[4:8])[0])
            self._movi = None
            avih = strh = strf = None
            at = 12
            while at + 8 <= self._end:
                f.seek(at)
                cid, size = struct.unpack("<4sI", f.read(8))
                if cid == b"LIST":
                    kind = f.read(4)
                    if kind == b"hdrl":
                        avih, strh, strf = self._headers(f.read(size - 4))
                    elif kind == b"movi" and self._movi is None:
                        self._movi = (at + 12, min(at + 8 + size, self._end))
                at += 8 + size + (size & 1)
        if avih is None or strh is None or strf is None:
            raise ValueError(f"{path}: no video stream header (avih / strh / strf)")
        if self._movi is None:
            raise ValueError(f"{path}: no 'movi' list")
        handler, compression = strh[4:8], strf[16:20]
        if compression.upper() != b"MJPG" or handler.upper() not in (b"MJPG", b"\0\0\0\0"):
            raise ValueError(f"{path}: the video stream is {handler!r} / {compression!r}, only Motion-JPEG ('MJPG') is read")
        usec, _, _, _, total = struct.unpack("<5I", avih[:20])
        scale, rate = struct.unpack("<II", strh[20:28])
        self.fps = rate / scale if scale and rate else (1e6 / usec if usec else 0.0)
        self.frame_count = int(total) if total else int(struct.unpack("<I", strh[32:36])[0])
        self.width, self.height = (abs(v) for v in struct.unpack("<ii", strf[4:12]))

    @staticmethod
    def _headers(hdrl: bytes):
        """avih and the strh / strf of the first 'vids' stream out of the body of LIST 'hdrl'."""
        avih = strh = strf = None
        at = 0
        while at + 8 <= len(hdrl):
            cid, size = struct.unpack("<4sI", hdrl[at:at + 8])
            body = hdrl[at + 8:at + 8 + size]
            if cid == b"avih" and size >= 40:
                avih = body
            elif cid == b"LIST" and body[:4] == b"strl" and strh is None:
                sub, h, fm = 4, None, None
                while sub + 8 <= len(body):
                    scid, ssize = struct.unpack("<4sI", body[sub:sub + 8])
                    if scid == b"strh" and ssize >= 36:
                        h = body[sub + 8:sub + 8 + ssize]
                    elif scid == b"strf" and ssize >= 20:
                        fm = body[sub + 8:sub + 8 + ssize]
                    sub += 8 + ssize + (ssize & 1)
                if h is not None and h[:4] == b"vids":
                    strh, strf = h, fm
            at += 8 + size + (size & 1)
        return avih, strh, strf

    def __len__(self) -> int:
        return self.frame_count

    def __iter__(self) -> Iterator[bytes]:
        with open(self.path, "rb") as f:
            stack = [self._movi]
            while stack:
                at, end = stack.pop()
                while at + 8 <= end:
                    f.seek(at)
                    cid, size = struct.unpack("<4sI", f.read(8))
                    nxt = at + 8 + size + (size & 1)
                    if cid == b"LIST":  # 'rec ' groups: their chunks first, then the rest of this list
                        stack.append((nxt, end))
                        stack.append((at + 12, min(at + 8 + size, end)))
                        break
                    if cid[2:] in (b"dc", b"db") and cid[:2] == b"00" and size > 0:
                        data = f.read(size)
                        if len(data) == size:
                            yield data
                    at = nxt


def read_mjpeg_avi(path: str) -> MjpegAvi:
    """Open a Motion-JPEG AVI file. Another codec, or a file that is no RIFF AVI, raises ``ValueError`` with the reason.
    Frames are returned as stored. Some cameras store frames without Huffman tables (the 'AVI1' convention: the annex K
    tables are implied); those are out of scope - such a frame is handed on unchanged, and the frame decoder falls back to
    the host decoder or fails as it does for any such file today."""
    return MjpegAvi(path)


__all__ = ["MjpegAviWriter", "MjpegAvi", "read_mjpeg_avi", "jpeg_size"]
