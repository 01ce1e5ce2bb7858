// The data-parallel half of the split JPEG encoder: from (H, W, 3) uint8 pixels on the device to the quantised coefficients
// the Huffman coder writes into a file - the host's (csrc/pp_jpeg_enc_host.h), or the device's (csrc/pp_jpeg_entropy.hip), which
// reads them where this file leaves them and writes the same bytes. Two launches per batch of images of any mix of
// sizes and sampling, driven by a device table of pp_jpeg_enc_desc:
//   jpeg_enc_color  BGR / RGB -> YCbCr, edge expansion, chroma downsampling into the component planes (uint8, whole MCUs);
//   jpeg_enc_fdct   level shift, 8x8 forward DCT, quantisation into int16 coefficients in natural order - the layout of
//                   pp_jpeg_desc.coef: per component [block_row][block_col][64] over whole MCUs.
// Integer arithmetic only; the rules are libjpeg's default compressor's (restated in numpy, tests/jpeg_enc_ref.py, which
// equals Pillow's bundled libjpeg-turbo coefficient for coefficient on the test grid):
//   * colour, 16-bit fixed point: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,
//     Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16;
//   * edges: a pixel right of the image is the row's last pixel, a pixel row below the image is the last row - but a chroma
//     row below the last REAL chroma row (ceil(H / v) of them) repeats that row, it is not downsampled again;
//   * downsampling without smoothing: h2v1 (a + b + bias) >> 1 with bias 0, 1, 0, 1 ... along the row, h2v2
//     (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2 ...;
//   * FDCT: jfdctint "islow", CONST_BITS 13, PASS1_BITS 2: rows first (outputs scaled up by 4), then columns (descale by
//     2 resp. 15 bits, round half up): 8 x the true DCT;
//   * quantisation by (table value << 3), rounding half away from zero;
//   * a luma block right of or below the component's own block grid (ceil(W / 8) x ceil(H / 8); chroma has none at these
//     samplings) is a dummy block: AC zero, DC that of the block before it in the MCU - its left neighbour, or for a dummy
//     row the last block of the MCU's row above (jccoefct.c).
// int32 throughout: samples are bytes, so a row pass stays below 2^11 x 2^15 and a column pass below 2^14 x 2^15 x 2.
// Memory-bound: a 1920 x 1080 frame is 6.2 MB of pixels in, 3.1 MB (4:2:0) of planes out and in again, 6.2 MB of
// coefficients out. The source image is read as dwords where a thread's pixels lie inside the image on a 4-byte boundary,
// bytewise (with the edge clamp) elsewhere; plane and coefficient stores are 4 to 16 bytes wide.
// Alignment: desc.planes 8 bytes, desc.coef 16 bytes (the Python wrapper places both on 256).
#include "pp_common.h"
#include "pp_jpeg_enc_host.h"

#include <cstdint>

namespace pp {

// what probpose_code_amd/jpeg.py mirrors (_ENC_DESC)
static_assert(sizeof(pp_jpeg_enc_desc) == 64 && offsetof(pp_jpeg_enc_desc, width) == 32, "four pointers, eight int32");

// Converts one row segment of NP = 4 * HS pixels starting at column x0 of source row `row`; columns past W - 1 repeat it.
template <int HS>
__device__ __forceinline__ void load_row(const uint8_t* __restrict__ row, int x0, int W, int rgb, int (&R)[4 * HS], int (&G)[4 * HS],
                                         int (&B)[4 * HS]) {
    constexpr int NP = 4 * HS;
    const uint8_t* p = row + 3 * (size_t)x0;
    unsigned c[3 * NP];
    if (x0 + NP <= W && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int k = 0; k < 3 * HS; ++k) {
            const uint32_t w = p4[k];
            c[4 * k] = w & 255u;
            c[4 * k + 1] = (w >> 8) & 255u;
            c[4 * k + 2] = (w >> 16) & 255u;
            c[4 * k + 3] = w >> 24;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int x = x0 + k < W ? x0 + k : W - 1;
            const uint8_t* q = row + 3 * (size_t)x;
            c[3 * k] = q[0];
            c[3 * k + 1] = q[1];
            c[3 * k + 2] = q[2];
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        R[k] = (int)(rgb ? c[3 * k] : c[3 * k + 2]);
        G[k] = (int)c[3 * k + 1];
        B[k] = (int)(rgb ? c[3 * k + 2] : c[3 * k]);
    }
}

constexpr int CBCR_OFFSET = (128 << 16) + 32767;

// One thread: chroma columns i0 .. i0 + 3 of chroma row j, and the 4 HS x vs luma samples above them.
template <int HS>
__device__ __forceinline__ void color_body(const pp_jpeg_enc_desc& d, int i0, int j) {
    constexpr int NP = 4 * HS;
    const int W = d.width, H = d.height, vs = d.vs;
    const int cstride = d.mcus_x * 8, ystride = cstride * HS;
    const size_t nb0 = (size_t)d.mcus_x * HS * d.mcus_y * vs, nbc = (size_t)d.mcus_x * d.mcus_y;
    uint8_t* __restrict__ yp = d.planes;
    uint8_t* __restrict__ cbp = d.planes + nb0 * 64;
    uint8_t* __restrict__ crp = cbp + nbc * 64;
    const int ch = (H + vs - 1) / vs, jj = j < ch ? j : ch - 1;  // jj: the real chroma row this one repeats
    int cb[4] = {0, 0, 0, 0}, cr[4] = {0, 0, 0, 0};
    int R[NP], G[NP], B[NP];
    for (int dy = 0; dy < vs; ++dy) {
        const int yo = j * vs + dy, y = yo < H ? yo : H - 1;
        load_row<HS>(d.src + (size_t)y * d.row_stride, i0 * HS, W, d.rgb, R, G, B);
        unsigned lum[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) lum[k] = (unsigned)((19595 * R[k] + 38470 * G[k] + 7471 * B[k] + 32768) >> 16);
        uint32_t* o = reinterpret_cast<uint32_t*>(yp + (size_t)yo * ystride + (size_t)i0 * HS);
#pragma unroll
        for (int k = 0; k < HS; ++k) o[k] = lum[4 * k] | (lum[4 * k + 1] << 8) | (lum[4 * k + 2] << 16) | (lum[4 * k + 3] << 24);
        if (jj == j) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                cb[k / HS] += (-11059 * R[k] - 21709 * G[k] + 32768 * B[k] + CBCR_OFFSET) >> 16;
                cr[k / HS] += (32768 * R[k] - 27439 * G[k] - 5329 * B[k] + CBCR_OFFSET) >> 16;
            }
        }
    }
    if (jj != j) {  // padding rows under the image: the chroma of the last real chroma row
        for (int dy = 0; dy < vs; ++dy) {
            const int yo = jj * vs + dy, y = yo < H ? yo : H - 1;
            load_row<HS>(d.src + (size_t)y * d.row_stride, i0 * HS, W, d.rgb, R, G, B);
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                cb[k / HS] += (-11059 * R[k] - 21709 * G[k] + 32768 * B[k] + CBCR_OFFSET) >> 16;
                cr[k / HS] += (32768 * R[k] - 27439 * G[k] - 5329 * B[k] + CBCR_OFFSET) >> 16;
            }
        }
    }
    if (HS == 2) {
        const int shift = vs == 2 ? 2 : 1, base = vs == 2 ? 1 : 0;  // bias 1, 2, 1, 2 (h2v2) or 0, 1, 0, 1 (h2v1); i0 is even
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cb[k] = (cb[k] + base + (k & 1)) >> shift;
            cr[k] = (cr[k] + base + (k & 1)) >> shift;
        }
    }
    const size_t co = (size_t)j * cstride + i0;
    *reinterpret_cast<uint32_t*>(cbp + co) = (unsigned)cb[0] | ((unsigned)cb[1] << 8) | ((unsigned)cb[2] << 16) | ((unsigned)cb[3] << 24);
    *reinterpret_cast<uint32_t*>(crp + co) = (unsigned)cr[0] | ((unsigned)cr[1] << 8) | ((unsigned)cr[2] << 16) | ((unsigned)cr[3] << 24);
}

// blockIdx.z: image; a thread takes four chroma samples of a chroma row (plane rows are whole MCUs: multiples of 8 wide).
__global__ __launch_bounds__(256) void jpeg_enc_color_kernel(const pp_jpeg_enc_desc* __restrict__ descs) {
    const pp_jpeg_enc_desc d = descs[blockIdx.z];
    const int i0 = 4 * (blockIdx.x * blockDim.x + threadIdx.x), j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i0 >= d.mcus_x * 8 || j >= d.mcus_y * 8) return;
    if (d.hs == 2) color_body<2>(d, i0, j);
    else color_body<1>(d, i0, j);
}

__device__ __forceinline__ int descale_up(int v, int n) { return (v + (1 << (n - 1))) >> n; }

// One 8-point pass of jfdctint's islow FDCT. Row pass: FIRST = true (even outputs << 2, odd ones descaled by 11);
// column pass: FIRST = false (descaled by 2 resp. 15).
template <bool FIRST>
__device__ __forceinline__ void fdct8(const int (&d)[8], int (&out)[8]) {
    constexpr int SH = FIRST ? 11 : 15;
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (FIRST) {
        out[0] = (tmp10 + tmp11) * 4;
        out[4] = (tmp10 - tmp11) * 4;
    } else {
        out[0] = descale_up(tmp10 + tmp11, 2);
        out[4] = descale_up(tmp10 - tmp11, 2);
    }
    int z1 = (tmp12 + tmp13) * 4433;
    out[2] = descale_up(z1 + tmp13 * 6270, SH);
    out[6] = descale_up(z1 + tmp12 * -15137, SH);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    out[7] = descale_up(t4 + z1 + z3, SH);
    out[5] = descale_up(t5 + z2 + z4, SH);
    out[3] = descale_up(t6 + z2 + z3, SH);
    out[1] = descale_up(t7 + z1 + z4, SH);
}

constexpr int FDCT_BLOCKS = 32;  // 8x8 blocks per workgroup: eight lanes per block

// blockIdx.y: image; blockIdx.x: 32 of its blocks (all components, in coefficient order). Lane l of a block's eight loads
// sample row l (8 bytes), the eight exchange the intermediate through LDS, lane l takes column l and quantises it, and a
// second exchange gives every lane one row of eight coefficients to store as 16 bytes.
__global__ __launch_bounds__(256) void jpeg_enc_fdct_kernel(const pp_jpeg_enc_desc* __restrict__ descs) {
    __shared__ int ws[FDCT_BLOCKS][8][9];
    __shared__ int wq[FDCT_BLOCKS][8][9];
    const pp_jpeg_enc_desc d = descs[blockIdx.y];
    const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
    const long long b = (long long)blockIdx.x * FDCT_BLOCKS + g;
    const int bw0 = d.mcus_x * d.hs, bwc = d.mcus_x;
    const long long nb0 = (long long)bw0 * d.mcus_y * d.vs, nbc = (long long)bwc * d.mcus_y;
    const bool live = b < nb0 + 2 * nbc;
    int c = 0;
    bool dummy = false;
    if (live) {
        int bw = bw0;
        long long local = b;
        if (b >= nb0) {
            c = b >= nb0 + nbc ? 2 : 1;
            local = b - nb0 - (c == 2 ? nbc : 0);
            bw = bwc;
        }
        int brow = (int)(local / bw), bcol = (int)(local % bw);
        if (c == 0) {  // a dummy block transforms the block whose DC it repeats
            const int bwr = (d.width + 7) >> 3, bhr = (d.height + 7) >> 3;
            if (brow >= bhr) {
                dummy = true;
                brow -= 1;
                bcol = bcol / d.hs * d.hs + d.hs - 1;
            }
            if (bcol >= bwr) {
                dummy = true;
                bcol -= 1;
            }
        }
        const uint8_t* plane = d.planes + (b - local) * 64;  // this component's plane: (block rows x 8, bw x 8) bytes
        const uint2 px = *reinterpret_cast<const uint2*>(plane + ((size_t)(brow * 8 + l) * bw + bcol) * 8);
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            in[k] = (int)((px.x >> (8 * k)) & 255u) - 128;
            in[4 + k] = (int)((px.y >> (8 * k)) & 255u) - 128;
        }
        fdct8<true>(in, out);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[g][l][k] = out[k];
    }
    __syncthreads();
    if (live) {
        const uint16_t* __restrict__ q = d.qtables + 64 * c;
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = ws[g][k][l];
        fdct8<false>(in, out);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int qv = (int)q[k * 8 + l] << 3, v = out[k];
            const int a = ((v < 0 ? -v : v) + (qv >> 1)) / qv;
            wq[g][k][l] = (dummy && (k | l)) ? 0 : (v < 0 ? -a : a);
        }
    }
    __syncthreads();
    if (live) {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = ((uint32_t)wq[g][l][2 * k] & 0xFFFFu) | ((uint32_t)wq[g][l][2 * k + 1] << 16);
        *reinterpret_cast<uint4*>(d.coef + b * 64 + l * 8) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace pp

extern "C" int pp_jpeg_quality_tables(int quality, uint16_t* qtables_host) {
    const int st = pp::jpeg::quality_tables(quality, qtables_host);
    if (st != PP_OK) pp::set_error("pp_jpeg_quality_tables: %s", pp::jpeg::g_reason);
    return st;
}

extern "C" int pp_jpeg_encode_plan(int width, int height, int subsampling, pp_jpeg_info* info) {
    const int st = pp::jpeg::encode_plan(width, height, subsampling, info);
    if (st != PP_OK) pp::set_error("pp_jpeg_encode_plan: %s", pp::jpeg::g_reason);
    return st;
}

extern "C" long long pp_jpeg_encoded_bound(const pp_jpeg_info* info) {
    const long long r = pp::jpeg::encoded_bound(info);
    if (r < 0) pp::set_error("pp_jpeg_encoded_bound: %s", pp::jpeg::g_reason);
    return r;
}

extern "C" int pp_jpeg_entropy_encode(const int16_t* coef_host, const uint16_t* qtables_host, const pp_jpeg_info* info,
                                      int restart_interval, void* out_host, size_t capacity, size_t* size_out) {
    const int st = pp::jpeg::entropy_encode(coef_host, qtables_host, info, restart_interval, reinterpret_cast<uint8_t*>(out_host), capacity, size_out);
    if (st != PP_OK) pp::set_error("pp_jpeg_entropy_encode: %s", pp::jpeg::g_reason);
    return st;
}

extern "C" int pp_jpeg_write_headers(const uint16_t* qtables_host, const pp_jpeg_info* info, int restart_interval, void* out_host,
                                     size_t capacity, size_t* size_out) {
    const int st = pp::jpeg::write_headers(qtables_host, info, restart_interval, reinterpret_cast<uint8_t*>(out_host), capacity, size_out);
    if (st != PP_OK) pp::set_error("pp_jpeg_write_headers: %s", pp::jpeg::g_reason);
    return st;
}

extern "C" int pp_jpeg_forward_batch(const pp_jpeg_enc_desc* descriptors, int n, long long max_blocks, int max_height, int max_width,
                                     void* stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0, PP_ERR_INVALID_ARG, "pp_jpeg_forward_batch: n < 0");
    if (n == 0) return PP_OK;
    PP_REQUIRE(descriptors, PP_ERR_INVALID_ARG, "pp_jpeg_forward_batch: NULL argument");
    PP_REQUIRE(max_blocks > 0 && max_height > 0 && max_width > 0, PP_ERR_INVALID_ARG, "pp_jpeg_forward_batch: bad shape");
    PP_REQUIRE(n <= 65535 && max_height <= 65535 && max_width <= 65535 && max_blocks <= 3ll * 8192 * 8192, PP_ERR_INVALID_ARG,
               "pp_jpeg_forward_batch: at most 65535 images of sides up to 65535");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // chroma planes are at most ceil(W / 8) * 8 samples wide and ceil(H / 8) * 8 high (4:4:4); a thread takes four of a row
    const unsigned cw = (unsigned)((max_width + 7) / 8 * 8), chh = (unsigned)((max_height + 7) / 8 * 8);
    hipLaunchKernelGGL(jpeg_enc_color_kernel, dim3((cw / 4 + 63) / 64, (chh + 3) / 4, n), dim3(64, 4), 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_enc_color");
    hipLaunchKernelGGL(jpeg_enc_fdct_kernel, dim3((unsigned)((max_blocks + FDCT_BLOCKS - 1) / FDCT_BLOCKS), n), dim3(256), 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_enc_fdct");
    return PP_OK;
}
