"""Uploads through one pinned buffer: ``BatchStaging`` (the reused pinned host buffer and the event that guards it) and
``StagedBlock`` (the layout of one upload: named regions, each on a multiple of 256 bytes, filled on the host and sent to
the device with one copy). Behind ``transforms.warp_affine_crops_batch`` and every batched call of ``jpeg``."""
from typing import Optional, Sequence, Tuple

import numpy as np
import torch


def _align(v: int, a: int = 256) -> int:
    return (v + a - 1) // a * a


class BatchStaging:
    """The reused pinned host buffer behind ``warp_affine_crops_batch``: the tables and the host images of one batch are
    packed into it and go to the device in ONE host-to-device copy. An event recorded after the copy guards it: the next
    batch waits for that copy before it writes into the buffer (a copy in flight still reads it)."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.ev: Optional[torch.cuda.Event] = None

    def acquire(self, nbytes: int) -> np.ndarray:
        if self.ev is not None:
            self.ev.synchronize()
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(1 << max(20, (nbytes - 1).bit_length()), dtype=torch.uint8, pin_memory=True)
        return self.buf.numpy()

    def upload(self, dev: torch.Tensor, nbytes: int) -> None:
        stream = torch.cuda.current_stream(dev.device)
        dev[:nbytes].copy_(self.buf[:nbytes], non_blocking=True)
        if self.ev is None:
            self.ev = torch.cuda.Event()
        self.ev.record(stream)


class StagedBlock:
    """One upload block. Regions are reserved in order as (name, nbytes): first those of ``head``, then image by image
    those of ``per_image``, whose nbytes is a list with one size per image. Each region starts at a multiple of 256 (the
    kernels load sixteen bytes at a time from some, eight from others); ``total`` is the aligned end of the last.
    ``offset`` / ``nbytes`` hold the head regions, ``offsets`` / ``sizes`` the per-image ones as lists over the images.
    ``acquire`` allocates the device block and takes the pinned buffer; from then on a head region is a numpy view of the
    pinned buffer (``host``), a device address (``ptr``) and a view of the device tensor (``device``), a per-image region the
    list of its views (``hosts``) and addresses (``ptrs``), made in one go. ``upload`` sends the whole block, or the head of
    it in front of a region, with one copy on the current stream."""

    __slots__ = ("offset", "nbytes", "offsets", "sizes", "total", "staging", "dev", "pinned", "base")

    def __init__(self, head: Sequence[Tuple[str, int]], per_image: Sequence[Tuple[str, Sequence[int]]] = ()):
        self.offset, self.nbytes, at = {}, dict(head), 0
        for name, nbytes in head:
            self.offset[name] = at
            at = _align(at + nbytes)
        self.offsets, self.sizes = {name: [] for name, _ in per_image}, dict(per_image)
        columns = [(self.offsets[name], sizes) for name, sizes in per_image]
        for i in range(len(per_image[0][1]) if per_image else 0):
            for offsets, sizes in columns:
                offsets.append(at)
                at = _align(at + sizes[i])
        self.total = at
        if len(self.offset) + len(self.offsets) != len(head) + len(per_image):
            raise ValueError("a region is reserved once")

    def head_bytes(self, before: Optional[str] = None) -> int:
        """The bytes ``upload(before)`` copies: everything in front of region ``before`` (of the first image's, for a
        per-image region), the whole block for None."""
        if before is None:
            return self.total
        return self.offsets[before][0] if before in self.offsets else self.offset[before]

    def acquire(self, staging: BatchStaging, device) -> "StagedBlock":
        self.staging = staging
        self.dev = torch.empty(self.total, dtype=torch.uint8, device=device)
        self.pinned = staging.acquire(self.total)
        self.base = self.dev.data_ptr()
        return self

    def host(self, name: str, dtype=None) -> np.ndarray:
        """A head region's bytes in the pinned buffer, as uint8 or as ``dtype`` (a structured one, int16, uint16)."""
        o = self.offset[name]
        view = self.pinned[o:o + self.nbytes[name]]
        return view if dtype is None else view.view(dtype)

    def hosts(self, name: str, dtype=None) -> list:
        """A per-image region's bytes in the pinned buffer, image by image."""
        buf, spans = self.pinned, zip(self.offsets[name], self.sizes[name])
        return [buf[o:o + n] for o, n in spans] if dtype is None else [buf[o:o + n].view(dtype) for o, n in spans]

    def device(self, name: str) -> torch.Tensor:
        o = self.offset[name]
        return self.dev[o:o + self.nbytes[name]]

    def ptr(self, name: str) -> int:
        return self.base + self.offset[name]

    def ptrs(self, name: str) -> list:
        base = self.base
        return [base + o for o in self.offsets[name]]

    def upload(self, before: Optional[str] = None) -> None:
        self.staging.upload(self.dev, self.head_bytes(before))
