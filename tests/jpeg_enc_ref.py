"""numpy restatement of the baseline JPEG compressor the split GPU encoder reproduces (csrc/pp_jpeg_enc.hip +
csrc/pp_jpeg_enc_host.h): pixels -> quantisation tables and quantised coefficients, by libjpeg's integer rules in int64:

  * quality tables: annex K.1 scaled by jpeg_quality_scaling, clamped to 1..255 (force_baseline);
  * colour: 16-bit fixed point, Y rounds with ONE_HALF, Cb / Cr carry the (128 << 16) + ONE_HALF - 1 offset;
  * edge expansion: the right edge repeats the last column of the full-resolution input, the bottom edge repeats the last
    input row up to a whole row group (v rows) and, after downsampling, the last row of every component;
  * downsampling without smoothing: h2v1 (a + b + bias) >> 1, bias 0, 1, 0, 1 ...; h2v2 (a + b + c + d + bias) >> 2, bias
    1, 2, 1, 2 ...;
  * FDCT: jfdctint "islow" (CONST_BITS 13, PASS1_BITS 2), rows then columns, 8 x the true DCT;
  * quantisation by (q << 3), rounding half away from zero;
  * dummy blocks - inside the last MCU column / row but outside the component's own block grid - have zero AC and the DC
    of the block before them in the MCU (jccoefct.c).

It is the arbiter of the kernels' arithmetic: tests/test_jpeg_enc_references.py pins it to Pillow's bundled libjpeg-turbo,
coefficient for coefficient. ``faults`` switches single mistakes on, for the tests that show the pin rejects them."""
import numpy as np

SUBSAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}

STD_LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                       87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                       101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
STD_CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99] +
                        [99] * 36, np.int64)


def quality_tables(quality: int) -> np.ndarray:
    """(3, 64) uint16 in natural order: luma, chroma, chroma."""
    if not 1 <= quality <= 100:
        raise ValueError("quality outside 1..100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    t = [np.clip((base * scale + 50) // 100, 1, 255) for base in (STD_LUMA_Q, STD_CHROMA_Q, STD_CHROMA_Q)]
    return np.stack(t).astype(np.uint16)


def geometry(W: int, H: int, subsampling: str) -> dict:
    hs, vs = SUBSAMPLING[subsampling]
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    return dict(width=W, height=H, ncomp=3, hs=hs, vs=vs, mcus_x=mx, mcus_y=my, comp_bw=[mx * hs, mx, mx], comp_bh=[my * vs, my, my],
                coef_count=64 * (mx * hs * my * vs + 2 * mx * my))


def color_planes(rgb: np.ndarray):
    """(H, W, 3) uint8 RGB -> Y, Cb, Cr int64 (H, W)."""
    r, g, b = (rgb[:, :, k].astype(np.int64) for k in range(3))
    off = (128 << 16) + 32767
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16, (-11059 * r - 21709 * g + 32768 * b + off) >> 16,
            (32768 * r - 27439 * g - 5329 * b + off) >> 16)


def _expand(p, rows, cols, replicate=True):
    """Grow a plane to (rows, cols) by repeating its last column and row (or - the fault - with zeros)."""
    mode = dict(mode="edge") if replicate else dict(mode="constant", constant_values=0)
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), **mode)


def component_planes(rgb: np.ndarray, subsampling: str, faults=()) -> list:
    """The three sample planes over whole MCUs, as the forward DCT reads them."""
    H, W = rgb.shape[:2]
    g = geometry(W, H, subsampling)
    hs, vs = g["hs"], g["vs"]
    rep = "no_edge_replication" not in faults
    Y, Cb, Cr = color_planes(rgb)
    out = [_expand(Y, g["comp_bh"][0] * 8, g["comp_bw"][0] * 8, rep)]
    ch = -(-H // vs)  # real chroma rows
    for p in (Cb, Cr):
        p = _expand(p, ch * vs, g["mcus_x"] * 8 * hs, rep)  # the input: right edge to whole blocks, bottom to a whole row group
        if hs == 2:
            cols = np.arange(p.shape[1] // 2)
            if vs == 2:
                bias = np.where(cols % 2 == 0, 1, 2) if "constant_bias" not in faults else 2
                p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
            else:
                bias = cols % 2 if "constant_bias" not in faults else 1
                p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        out.append(_expand(p, g["mcus_y"] * 8, g["mcus_x"] * 8, rep))  # after downsampling: the last row repeated
    return out


def _fdct_pass(d, first):
    sh = 11 if first else 15
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2

    def ds(v, n):
        return (v + (1 << (n - 1))) >> n

    out = [None] * 8
    out[0] = (tmp10 + tmp11) << 2 if first else ds(tmp10 + tmp11, 2)
    out[4] = (tmp10 - tmp11) << 2 if first else ds(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * 4433
    out[2] = ds(z1 + tmp13 * 6270, sh)
    out[6] = ds(z1 - tmp12 * 15137, sh)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7] = ds(tmp4 + z1 + z3, sh)
    out[5] = ds(tmp5 + z2 + z4, sh)
    out[3] = ds(tmp6 + z2 + z3, sh)
    out[1] = ds(tmp7 + z1 + z4, sh)
    return out


def fdct_quantise(plane: np.ndarray, qtable: np.ndarray, faults=()) -> np.ndarray:
    """(8 bh, 8 bw) samples + (64,) table -> (bh, bw, 64) int16 in natural order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.astype(np.int64).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128  # [brow][bcol][r][c]
    rows = np.stack(_fdct_pass([d[:, :, :, k] for k in range(8)], True), axis=3)  # along c
    full = np.stack(_fdct_pass([rows[:, :, k, :] for k in range(8)], False), axis=2)  # along r
    q = qtable.astype(np.int64).reshape(8, 8) << 3
    mag = np.abs(full)
    mag = mag // q if "truncating_quantisation" in faults else (mag + (q >> 1)) // q
    return (np.sign(full) * mag).reshape(bh, bw, 64).astype(np.int16)


def forward(rgb: np.ndarray, quality=75, subsampling="4:2:0", qtables=None, faults=()) -> dict:
    """(H, W, 3) uint8 RGB -> the dict tests/jpeg_ref.parse gives for libjpeg's file of these pixels: geometry, ``coef`` (per
    component (block_rows, block_cols, 64) int16, natural order, whole MCUs) and ``qtables`` (3, 64) uint16."""
    rgb = np.asarray(rgb)
    H, W = rgb.shape[:2]
    g = geometry(W, H, subsampling)
    qt = quality_tables(quality) if qtables is None else np.asarray(qtables, np.uint16).reshape(3, 64)
    coef = [fdct_quantise(p, qt[c], faults) for c, p in enumerate(component_planes(rgb, subsampling, faults))]
    # dummy blocks: only the luma grid can be smaller than its share of the MCU grid
    y = coef[0]
    bwr, bhr, hs = -(-W // 8), -(-H // 8), g["hs"]
    if "dummy_dc_zero" in faults:
        y[:, bwr:] = 0
        y[bhr:] = 0
    else:
        if bwr < y.shape[1]:  # a dummy column: DC of the block on its left
            y[:, bwr, 1:] = 0
            y[:, bwr, 0] = y[:, bwr - 1, 0]
        if bhr < y.shape[0]:  # a dummy row: DC of the last block of the MCU's row above
            y[bhr, :, 1:] = 0
            last = y[bhr - 1, hs - 1::hs, 0]
            y[bhr, :, 0] = np.repeat(last, hs)
    out = dict(g)
    out.update(restart_interval=0, coef=coef, qtables=qt)
    return out


def flat_coefficients(fwd: dict) -> np.ndarray:
    return np.concatenate([c.reshape(-1) for c in fwd["coef"]])


def pillow_bytes(rgb: np.ndarray, quality=75, subsampling="4:2:0") -> bytes:
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, "JPEG", quality=quality, subsampling=PIL_SUBSAMPLING[subsampling])
    return buf.getvalue()


# ------------------------------------------------------------------------------------------------------ the test grid
SIZES = ((1, 1), (7, 5), (8, 8), (9, 17), (16, 16), (17, 33), (24, 8), (31, 15), (48, 64))  # width x height
CONTENTS = ("noise", "flat0", "flat255", "checker", "gradient")
_IMAGES = {}


def image(content: str, W: int, H: int) -> np.ndarray:
    """(H, W, 3) uint8 RGB test content, computed once per (content, size) and shared (do not modify)."""
    key = (content, W, H)
    if key not in _IMAGES:
        if content == "noise":
            a = np.random.default_rng(1000 * W + H).integers(0, 256, (H, W, 3), dtype=np.uint8)
        elif content == "flat0":
            a = np.zeros((H, W, 3), np.uint8)
        elif content == "flat255":
            a = np.full((H, W, 3), 255, np.uint8)
        elif content == "checker":  # 0 / 255 per pixel: the largest AC magnitudes
            yy, xx = np.mgrid[0:H, 0:W]
            a = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
        elif content == "gradient":
            yy, xx = np.mgrid[0:H, 0:W]
            a = np.stack([(255 * xx) // max(W - 1, 1), (255 * yy) // max(H - 1, 1), (255 * (xx + yy)) // max(W + H - 2, 1)], axis=2).astype(np.uint8)
        else:
            raise ValueError(content)
        a.setflags(write=False)
        _IMAGES[key] = a
    return _IMAGES[key]
