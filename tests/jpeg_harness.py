"""The guarded call of the device half of the split JPEG decoder that tests/test_jpeg_gpu.py and tests/fuzz_jpeg.py share."""
import numpy as np
import torch

DEV = "cuda:0"
CANARY = 0xA5
GUARD = 4096
GAP = 67  # canary bytes between two output images: odd, so the images start at every alignment


def _align(v, a=256):
    return (v + a - 1) // a * a


def raw_reconstruct(jpeg, coefs):
    """pp_jpeg_reconstruct_bgr_batch on buffers of this test's own: the input block (descriptors, tables, coefficients), the
    plane scratch and all output images inside canary bytes. Runs the call twice. Returns the images (numpy, BGR)."""
    _lib = jpeg._lib
    n = len(coefs)
    off, o_qt, o_coef = _align(64 * n), [], []
    for c in coefs:
        o_qt.append(off)
        off = _align(off + 384)
        o_coef.append(off)
        off = _align(off + 2 * c.coef.size)
    host = np.zeros(off, np.uint8)
    sizes = [int(np.prod(c.shape)) for c in coefs]
    o_out, p = [], GUARD
    for s in sizes:
        o_out.append(p)
        p += s + GAP
    out = torch.full((p - GAP + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    infos = (jpeg.JpegInfo * n)(*[c.info for c in coefs])
    need = int(_lib.lib.pp_jpeg_scratch_bytes(infos, n))
    assert need == sum(_align(int(c.info.coef_count)) for c in coefs)
    scratch = torch.full((need + 2 * GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    dev = torch.empty(off, dtype=torch.uint8, device=DEV)
    desc = host[:64 * n].view(jpeg._DESC)
    planes = scratch.data_ptr() + GUARD
    for i, c in enumerate(coefs):
        host[o_qt[i]:o_qt[i] + 128 * len(c.qtables)].view(np.uint16)[:] = c.qtables.reshape(-1)
        host[o_coef[i]:o_coef[i] + 2 * c.coef.size].view(np.int16)[:] = c.coef
        desc[i] = (dev.data_ptr() + o_coef[i], dev.data_ptr() + o_qt[i], planes, out.data_ptr() + o_out[i], c.info.width, c.info.height,
                   c.info.ncomp, c.info.hs, c.info.vs, c.info.mcus_x, c.info.mcus_y, 0)
        planes += _align(int(c.info.coef_count))
    dev.copy_(torch.from_numpy(host))
    args = (dev.data_ptr(), n, max(int(c.info.coef_count) // 64 for c in coefs), max(c.info.height for c in coefs),
            max(c.info.width for c in coefs), torch.cuda.current_stream().cuda_stream)
    _lib.reset_launch_counts()
    _lib.call("pp_jpeg_reconstruct_bgr_batch", *args)
    torch.cuda.synchronize()
    counts = (_lib.launch_count("jpeg_idct"), _lib.launch_count("jpeg_color"), _lib.launch_count("pp_jpeg.hip"))
    assert counts == (1, 1, 2), f"launches per call {counts} for n = {n}"
    first = out.cpu().numpy()
    out[GUARD:len(out) - GUARD] = CANARY  # (the images and the gaps between them)
    _lib.call("pp_jpeg_reconstruct_bgr_batch", *args)
    torch.cuda.synchronize()
    second = out.cpu().numpy()
    assert np.array_equal(first, second), "a second launch gives other bytes"
    assert np.array_equal(dev.cpu().numpy(), host), "the kernels changed their input"
    sc = scratch.cpu().numpy()
    assert (sc[:GUARD] == CANARY).all() and (sc[GUARD + need:] == CANARY).all(), "bytes outside the plane scratch written"
    at = GUARD
    for c in coefs:  # an image's planes take coef_count bytes: the padding up to the next image's stays untouched
        assert (sc[at + int(c.info.coef_count):at + _align(int(c.info.coef_count))] == CANARY).all(), "bytes behind an image's planes written"
        at += _align(int(c.info.coef_count))
    mask = np.ones(len(first), bool)
    for o, s in zip(o_out, sizes):
        mask[o:o + s] = False
    assert (first[mask] == CANARY).all(), "bytes outside an output image written"
    return [first[o:o + s].reshape(c.shape) for o, s, c in zip(o_out, sizes, coefs)]
