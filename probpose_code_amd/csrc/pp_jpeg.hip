// The data-parallel half of the split JPEG decoder: from the quantised coefficients the host's Huffman decoder leaves
// (csrc/pp_jpeg_host.h) to the (H, W, 3) uint8 BGR image pp_warp_affine_u8_batch reads in place. Two launches per batch of
// images of any mix of sizes and sampling, driven by a device table of pp_jpeg_desc:
//   jpeg_idct    dequantise + 8x8 inverse DCT into the component planes (uint8, whole MCUs);
//   jpeg_color   chroma upsampling + YCbCr -> BGR + HWC packing.
// Integer arithmetic only; the rules are libjpeg's (restated in numpy, tests/jpeg_ref.py, which equals Pillow's bundled
// libjpeg-turbo bit for bit on the test grid):
//   * IDCT: jidctint "islow", CONST_BITS 13, PASS1_BITS 2: columns first (descale by 11 bits, round half up), then rows
//     (descale by 18), + 128, clamp to [0, 255];
//   * a chroma plane is ceil(W h_c / h_max) x ceil(H v_c / v_max) samples: the neighbour of an edge sample is the edge
//     sample itself (the last REAL row / column, never the MCU padding);
//   * a chroma plane of one or two samples per row is replicated, not interpolated (jdsample interpolates only for
//     downsampled_width > 2); wider ones take the
//   * fancy upsampling h2v1: out[2i] = (3 p[i] + p[i-1] + 1) >> 2, out[2i+1] = (3 p[i] + p[i+1] + 2) >> 2;
//     h2v2: t = 3 near_row + far_row (upper output row pairs with the row above, lower with the row below),
//     out[2i] = (3 t[i] + t[i-1] + 8) >> 4, out[2i+1] = (3 t[i] + t[i+1] + 7) >> 4;
//   * colour, cb and cr reduced by 128: R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
//     G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), clamped to [0, 255].
// int32 throughout (the reference restatement is int64). It cannot overflow for coefficients that come from an encoder:
// a dequantised coefficient of 8-bit samples is at most 8 x 128 + q / 2 < 2^11 in magnitude for 8-bit tables, so a column
// pass sums at most four products with constants < 2^15 plus a term << 13: < 2^29; its outputs are 4 x a one-dimensional
// transform of samples in [-128, 127] plus the quantisation error, < 2^13, and the row pass is bounded the same way: < 2^31.
// The upsampling and colour terms are products of bytes with constants < 2^17. A hostile coefficient stream can exceed
// these bounds; the file is built with -fwrapv (Makefile), so its arithmetic then wraps - wrong pixels inside the image,
// and nothing else: no address depends on a sample value.
// Memory-bound and, at the batch sizes of a test loop, launch-latency-sized: ~2.8 MB moved per 640 x 480 4:2:0 image
// (coefficients in, planes out and in, pixels out).
#include "pp_common.h"
#include "pp_jpeg_host.h"

#include <cstdint>

namespace pp {

// what probpose_code_amd/jpeg.py mirrors (_DESC)
static_assert(sizeof(pp_jpeg_desc) == 64 && offsetof(pp_jpeg_desc, width) == 32, "four pointers, eight int32");

__device__ __forceinline__ int descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

// One 8-point pass of jidctint's islow IDCT; `shift`: 11 after the column pass, 18 after the row pass.
__device__ __forceinline__ void idct8(const int (&in)[8], int (&out)[8], int shift) {
    int z1 = (in[2] + in[6]) * 4433;
    int tmp2 = z1 + in[6] * -15137, tmp3 = z1 + in[2] * 6270;
    int tmp0 = (in[0] + in[4]) * 8192, tmp1 = (in[0] - in[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7];
    tmp1 = in[5];
    tmp2 = in[3];
    tmp3 = in[1];
    z1 = tmp0 + tmp3;
    int z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    out[0] = descale(tmp10 + tmp3, shift);
    out[7] = descale(tmp10 - tmp3, shift);
    out[1] = descale(tmp11 + tmp2, shift);
    out[6] = descale(tmp11 - tmp2, shift);
    out[2] = descale(tmp12 + tmp1, shift);
    out[5] = descale(tmp12 - tmp1, shift);
    out[3] = descale(tmp13 + tmp0, shift);
    out[4] = descale(tmp13 - tmp0, shift);
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

constexpr int IDCT_BLOCKS = 32;  // 8x8 blocks per workgroup: eight lanes per block

// blockIdx.y: image; blockIdx.x: 32 of its blocks (all components, in coefficient order). Lane l of a block's eight takes
// column l, the eight exchange the intermediate through LDS, then lane l takes row l and stores its eight bytes at once.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const pp_jpeg_desc* __restrict__ descs) {
    __shared__ int ws[IDCT_BLOCKS][8][9];
    const pp_jpeg_desc d = descs[blockIdx.y];
    const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
    const long long b = (long long)blockIdx.x * IDCT_BLOCKS + g;
    const int bw0 = d.mcus_x * d.hs, bwc = d.mcus_x;
    const long long nb0 = (long long)bw0 * d.mcus_y * d.vs, nbc = d.ncomp == 3 ? (long long)bwc * d.mcus_y : 0;
    const bool live = b < nb0 + 2 * nbc;
    int c = 0, bw = bw0;
    long long local = b;
    if (live) {
        if (b >= nb0) {
            c = b >= nb0 + nbc ? 2 : 1;
            local = b - nb0 - (c == 2 ? nbc : 0);
            bw = bwc;
        }
        const int16_t* __restrict__ coef = d.coef + b * 64;
        const uint16_t* __restrict__ q = d.qtables + 64 * c;
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = (int)coef[k * 8 + l] * (int)q[k * 8 + l];
        idct8(in, out, 11);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[g][k][l] = out[k];
    }
    __syncthreads();
    if (live) {
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = ws[g][l][k];
        idct8(in, out, 18);
        uint2 px;
        px.x = clamp255(out[0] + 128) | (clamp255(out[1] + 128) << 8) | (clamp255(out[2] + 128) << 16) | (clamp255(out[3] + 128) << 24);
        px.y = clamp255(out[4] + 128) | (clamp255(out[5] + 128) << 8) | (clamp255(out[6] + 128) << 16) | (clamp255(out[7] + 128) << 24);
        const long long brow = local / bw, bcol = local % bw;
        uint8_t* plane = d.planes + (b - local) * 64;  // this component's plane: (block rows x 8, bw x 8) bytes
        *reinterpret_cast<uint2*>(plane + ((brow * 8 + l) * bw + bcol) * 8) = px;
    }
}

// One chroma sample at output pixel (x, y). p: the component's plane (row stride `stride`), cw x ch real samples.
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int stride, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(size_t)y * stride + x];
    if (cw <= 2) return p[(size_t)(vs == 2 ? y >> 1 : y) * stride + (x >> 1)];
    const int i = x >> 1, side = (x & 1) ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
    if (vs == 1) {
        const uint8_t* r = p + (size_t)y * stride;
        return (3 * r[i] + r[side] + 1 + (x & 1)) >> 2;
    }
    const int j = y >> 1, far = (y & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
    const uint8_t* rn = p + (size_t)j * stride;
    const uint8_t* rf = p + (size_t)far * stride;
    const int t = 3 * rn[i] + rf[i], ts = 3 * rn[side] + rf[side];
    return (3 * t + ts + 8 - (x & 1)) >> 4;
}

// blockIdx.z: image; a thread takes four pixels of a row: 12 bytes, three dword stores where the address allows.
__global__ __launch_bounds__(256) void jpeg_color_kernel(const pp_jpeg_desc* __restrict__ descs) {
    const pp_jpeg_desc d = descs[blockIdx.z];
    const int x0 = 4 * (blockIdx.x * blockDim.x + threadIdx.x), y = blockIdx.y * blockDim.y + threadIdx.y;
    if (y >= d.height || x0 >= d.width) return;
    const int W = d.width, npx = W - x0 < 4 ? W - x0 : 4;
    const int stride0 = d.mcus_x * d.hs * 8, cstride = d.mcus_x * 8;
    const size_t nb0 = (size_t)d.mcus_x * d.hs * d.mcus_y * d.vs, nbc = (size_t)d.mcus_x * d.mcus_y;
    const uint8_t* __restrict__ yp = d.planes + (size_t)y * stride0;
    const uint8_t* __restrict__ cbp = d.planes + nb0 * 64;
    const uint8_t* __restrict__ crp = cbp + nbc * 64;
    const int cw = (W + d.hs - 1) / d.hs, ch = (d.height + d.vs - 1) / d.vs;
    unsigned char px[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + (k < npx ? k : 0);
        const int Y = yp[x];
        int R = Y, G = Y, B = Y;
        if (d.ncomp == 3) {
            const int cb = chroma_at(cbp, cstride, cw, ch, d.hs, d.vs, x, y) - 128;
            const int cr = chroma_at(crp, cstride, cw, ch, d.hs, d.vs, x, y) - 128;
            R = Y + ((91881 * cr + 32768) >> 16);
            B = Y + ((116130 * cb + 32768) >> 16);
            G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        }
        px[3 * k] = (unsigned char)clamp255(B);
        px[3 * k + 1] = (unsigned char)clamp255(G);
        px[3 * k + 2] = (unsigned char)clamp255(R);
    }
    uint8_t* o = d.out + ((size_t)y * W + x0) * 3;
    if (npx == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * npx; ++k) o[k] = px[k];
    }
}

}  // namespace pp

extern "C" int pp_jpeg_probe(const void* data_host, size_t size, pp_jpeg_info* info) {
    const int st = pp::jpeg::probe(reinterpret_cast<const uint8_t*>(data_host), size, info);
    if (st != PP_OK) pp::set_error("pp_jpeg_probe: %s", pp::jpeg::g_reason);
    return st;
}

extern "C" int pp_jpeg_entropy_decode(const void* data_host, size_t size, int16_t* coef_host, long long coef_capacity,
                                      uint16_t* qtables_host, pp_jpeg_info* info) {
    const int st = pp::jpeg::entropy_decode(reinterpret_cast<const uint8_t*>(data_host), size, coef_host, coef_capacity, qtables_host, info);
    if (st != PP_OK) pp::set_error("pp_jpeg_entropy_decode: %s", pp::jpeg::g_reason);
    return st;
}

extern "C" long long pp_jpeg_scratch_bytes(const pp_jpeg_info* infos_host, int n) {
    if (!infos_host || n < 0) {
        pp::set_error("pp_jpeg_scratch_bytes: bad argument");
        return PP_ERR_INVALID_ARG;
    }
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        if (infos_host[i].coef_count <= 0 || !infos_host[i].supported) {
            pp::set_error("pp_jpeg_scratch_bytes: entry %d describes no supported file", i);
            return PP_ERR_INVALID_ARG;
        }
        total += (infos_host[i].coef_count + 255) / 256 * 256;
    }
    return total;
}

extern "C" int pp_jpeg_reconstruct_bgr_batch(const pp_jpeg_desc* descriptors, int n, long long max_blocks, int max_height,
                                             int max_width, void* stream) {
    using namespace pp;
    if (n == 0) return PP_OK;
    PP_REQUIRE(descriptors, PP_ERR_INVALID_ARG, "pp_jpeg_reconstruct_bgr_batch: NULL argument");
    PP_REQUIRE(n > 0 && max_blocks > 0 && max_height > 0 && max_width > 0, PP_ERR_INVALID_ARG, "pp_jpeg_reconstruct_bgr_batch: bad shape");
    PP_REQUIRE(n <= 65535 && max_height <= 65535 && max_width <= 65535 && max_blocks <= 3ll * 8192 * 8192, PP_ERR_UNSUPPORTED,
               "pp_jpeg_reconstruct_bgr_batch: at most 65535 images of sides up to 65535");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), n), dim3(256), 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_idct");
    hipLaunchKernelGGL(jpeg_color_kernel, dim3(((max_width + 3) / 4 + 63) / 64, (max_height + 3) / 4, n), dim3(64, 4), 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_color");
    return PP_OK;
}
