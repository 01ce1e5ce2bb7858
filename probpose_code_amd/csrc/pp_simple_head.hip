// The head of the ViTPose "-simple" variants (mmpose/models/necks/fmap_proc_neck.py:52-92 + heatmap_head.py:198-213 with
// deconv_out_channels = [] and final_layer = 3x3): ReLU -> bilinear x4 upsampling -> zero-padded 3x3 convolution E -> K. Everything
// behind the ReLU is linear, so the convolution runs BEFORE the upsampling, at the backbone's resolution:
//
//   r       = relu(feat)                                   pp_relu_operand            (operand format in, operand format out)
//   T[t, k] = r . W[k, :, dy + 1, dx + 1]                  pp_gemm_ws, planar output  (nine tap planes of h x w per keypoint, fp32)
//   out[k, Y, X] = bias[k] + sum over the taps (dy, dx) with 0 <= Y + dy < 4h and 0 <= X + dx < 4w of bil(T[3 (dy + 1) + dx + 1, k], Y + dy, X + dx)
//                                                          pp_taps_upsample4_conv3x3
//
// bil is torch's bilinear sample with align_corners = False at scale 4: sy = max((Y' + 0.5) / 4 - 0.5, 0), y0 = floor(sy), y1 = min(y0 + 1,
// h - 1), ly = sy - y0 (0, 0.125, 0.375, 0.625 or 0.875: exact, as are the products of two of them). A tap outside the UPSAMPLED map is the
// convolution's zero padding - it contributes nothing, it is not a clamped sample - and is left out by a select, never multiplied by zero
// (a NaN of a neighbouring sample must not leak through a term the reference does not have). The (n_img, 4h, 4w, E) upsampled map is
// never built: 604 MB at batch size 64 with flip test in the split-fp16 format, against 15 MB of tap planes.
//
// The gather kernel is bound by the logits it writes (n_img K 16 h w floats; the tap planes are 9 / 16 of that and are read once). One workgroup
// computes a tile of up to 64 x 64 outputs of one (image, keypoint): the up to 18 x 18 samples of each of the nine planes it needs go through
// LDS (11.7 KiB, five workgroups' worth fit a CU many times over), every thread then produces runs of four neighbouring outputs of a row -
// one 16-byte store - whose 3 x 6 sample positions share their row and column weights.
#include "pp_common.h"
#include "pp_split.h"

namespace pp {
namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_TILE = 16;              // low-resolution rows / columns per workgroup tile (64 x 64 outputs)
constexpr int SH_STAGE = SH_TILE + 2;    // + one sample of halo on either side
constexpr int SH_PITCH = SH_STAGE + 1;   // LDS row pitch in floats (odd: the column walks of neighbouring rows spread over the banks)

// ---------------------------------------------------------------------------------------------------------------- ReLU of an operand tensor
// One thread per 16 bytes. fp32: four values; bf16: eight; split fp16: the eight hi halves of a chunk and, 64 bytes further, their lo halves
// (pp_split.h: blocks of 32 hi + 32 lo halves). An element that is neither > 0 nor NaN becomes +0 (both halves); every other one is copied
// bit for bit - the NaN of an out-of-range operand included (relu_keep_nan's rule: the decode behind it must see it).
template <int FMT>
__global__ __launch_bounds__(SH_THREADS) void relu_operand_kernel(const u32x4* __restrict__ in, u32x4* __restrict__ out, long long n_vec) {
    const long long i = (long long)blockIdx.x * SH_THREADS + threadIdx.x;
    if (i >= n_vec) return;
    if constexpr (FMT == PP_OUT_F32) {
        u32x4 v = in[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned u = v[j];  // (a scalar copy: __builtin_bit_cast of a vector ELEMENT reads element 0)
            const float x = __builtin_bit_cast(float, u);
            v[j] = (x > 0.f || x != x) ? u : 0u;
        }
        out[i] = v;
    } else if constexpr (FMT == PP_OUT_BF16) {
        u32x4 v = in[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned u = v[j], ul = u << 16, uh = u & 0xffff0000u;
            const float a = __builtin_bit_cast(float, ul), b = __builtin_bit_cast(float, uh);
            const unsigned ka = (a > 0.f || a != a) ? 0x0000ffffu : 0u, kb = (b > 0.f || b != b) ? 0xffff0000u : 0u;
            v[j] &= ka | kb;
        }
        out[i] = v;
    } else {
        // vector i -> block i / 4 (128 bytes = eight vectors), hi chunk i % 4, lo chunk 4 + i % 4
        const long long at = (i >> 2) * 8 + (i & 3);
        u32x4 hi = in[at], lo = in[at + 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned hu = hi[j], lu = lo[j];
            const f16x2 h = __builtin_bit_cast(f16x2, hu), l = __builtin_bit_cast(f16x2, lu);
            const float a = (float)h[0] + (float)l[0], b = (float)h[1] + (float)l[1];
            const unsigned keep = ((a > 0.f || a != a) ? 0x0000ffffu : 0u) | ((b > 0.f || b != b) ? 0xffff0000u : 0u);
            hi[j] &= keep;
            lo[j] &= keep;
        }
        out[at] = hi;
        out[at + 4] = lo;
    }
}

// ---------------------------------------------------------------------------------------------------------------- taps -> logits
// One coordinate of the upsampled map -> the two low-resolution samples and the weight of the second (torch's area_pixel_compute_source_index
// with align_corners = False, scale 1 / 4), relative to the staged window that starts at `first`.
struct Axis {
    int i0, i1;
    float l;
    bool in_map;
};
__device__ __forceinline__ Axis axis_of(int c, int n_low, int first) {
    Axis a;
    a.in_map = c >= 0 && c < 4 * n_low;
    const float s = fmaxf(((float)c + 0.5f) * 0.25f - 0.5f, 0.f);
    int i0 = (int)s;  // s >= 0: truncation = floor
    i0 = min(i0, n_low - 1);  // (an out-of-map coordinate past the end: its samples are never used, its addresses stay inside the window)
    a.l = s - (float)i0;
    a.i1 = min(i0 + 1, n_low - 1) - first;
    a.i0 = i0 - first;
    return a;
}

__global__ __launch_bounds__(SH_THREADS) void taps_upsample4_conv3x3_kernel(const float* __restrict__ taps, const float* __restrict__ bias,
                                                                             float* __restrict__ out, int K, int h, int w, int tiles_y,
                                                                             int tiles_x, int vec_store) {
    __shared__ float s[9][SH_STAGE * SH_PITCH];
    const int ntiles = tiles_y * tiles_x;
    const int tile = blockIdx.x % ntiles, ik = blockIdx.x / ntiles;  // ik = image * K + keypoint
    const int img = ik / K, k = ik - img * K;
    const int r0 = (tile / tiles_x) * SH_TILE, c0 = (tile % tiles_x) * SH_TILE;
    const int LR = min(SH_TILE, h - r0), LC = min(SH_TILE, w - c0);
    // staged window of every tap plane: the tile's samples and one more on either side, inside the plane
    const int sr0 = max(r0 - 1, 0), sc0 = max(c0 - 1, 0);
    const int nsr = min(r0 + LR, h - 1) - sr0 + 1, nsc = min(c0 + LC, w - 1) - sc0 + 1;  // <= SH_STAGE each
    const size_t hw = (size_t)h * w;
    const float* plane0 = taps + ((size_t)img * 9 * K + k) * hw;  // tap t of this keypoint: K planes further each
    const int per = nsr * nsc;
    for (int i = threadIdx.x; i < 9 * per; i += SH_THREADS) {
        const int t = i / per, q = i - t * per;
        const int rr = q / nsc, cc = q - rr * nsc;
        s[t][rr * SH_PITCH + cc] = plane0[(size_t)t * K * hw + (size_t)(sr0 + rr) * w + (sc0 + cc)];
    }
    __syncthreads();
    const float b = bias[k];
    float* oplane = out + (size_t)ik * 16 * hw;
    const size_t W4 = (size_t)4 * w;
    for (int i = threadIdx.x; i < 4 * LR * LC; i += SH_THREADS) {
        const int yy = i / LC, cc = i - yy * LC;
        const int Y = 4 * r0 + yy, X0 = 4 * (c0 + cc);
        Axis ay[3], ax[6];
#pragma unroll
        for (int d = 0; d < 3; ++d) ay[d] = axis_of(Y + d - 1, h, sr0);
#pragma unroll
        for (int d = 0; d < 6; ++d) ax[d] = axis_of(X0 + d - 1, w, sc0);
        float acc[4] = {b, b, b, b};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int o0 = ay[dy].i0 * SH_PITCH, o1 = ay[dy].i1 * SH_PITCH;
            const float ly = ay[dy].l;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float* pl = s[3 * dy + dx];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const Axis& a = ax[p + dx];
                    const float top = (1.f - a.l) * pl[o0 + a.i0] + a.l * pl[o0 + a.i1];
                    const float bot = (1.f - a.l) * pl[o1 + a.i0] + a.l * pl[o1 + a.i1];
                    const float v = (1.f - ly) * top + ly * bot;
                    acc[p] = (ay[dy].in_map && a.in_map) ? acc[p] + v : acc[p];  // zero padding of the conv: the tap is left out
                }
            }
        }
        float* o = oplane + (size_t)Y * W4 + X0;
        if (vec_store) {
            *reinterpret_cast<f32x4*>(o) = f32x4{acc[0], acc[1], acc[2], acc[3]};
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) o[p] = acc[p];
        }
    }
}

}  // namespace
}  // namespace pp

extern "C" int pp_relu_operand(int format, const void* in, void* out, int n_rows, int row_len, void* stream) {
    using namespace pp;
    PP_REQUIRE(format == PP_OUT_F32 || format == PP_OUT_BF16 || format == PP_OUT_SPLIT, PP_ERR_INVALID_ARG, "pp_relu_operand: unknown format");
    PP_REQUIRE(n_rows >= 0 && row_len > 0, PP_ERR_INVALID_ARG, "pp_relu_operand: bad n_rows / row_len");
    PP_REQUIRE(row_len % 32 == 0, PP_ERR_UNSUPPORTED, "pp_relu_operand: rows are multiples of 32 elements (the operand formats' block)");
    if (n_rows == 0) return PP_OK;
    PP_REQUIRE(in && out, PP_ERR_INVALID_ARG, "pp_relu_operand: in and out must be non-NULL");
    PP_REQUIRE(reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0, PP_ERR_INVALID_ARG,
               "pp_relu_operand: in and out must be 16-byte aligned");
    const long long n = (long long)n_rows * row_len;
    // threads: fp32 four elements each, bf16 eight, split fp16 eight (a hi chunk and its lo chunk)
    const long long n_vec = format == PP_OUT_F32 ? n / 4 : n / 8;
    const long long blocks = (n_vec + SH_THREADS - 1) / SH_THREADS;
    PP_REQUIRE(blocks < (1ll << 31), PP_ERR_UNSUPPORTED, "pp_relu_operand: tensor too large for one launch");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const u32x4* src = reinterpret_cast<const u32x4*>(in);
    u32x4* dst = reinterpret_cast<u32x4*>(out);
    if (format == PP_OUT_F32)
        hipLaunchKernelGGL(relu_operand_kernel<PP_OUT_F32>, dim3((unsigned)blocks), dim3(SH_THREADS), 0, s, src, dst, n_vec);
    else if (format == PP_OUT_BF16)
        hipLaunchKernelGGL(relu_operand_kernel<PP_OUT_BF16>, dim3((unsigned)blocks), dim3(SH_THREADS), 0, s, src, dst, n_vec);
    else
        hipLaunchKernelGGL(relu_operand_kernel<PP_OUT_SPLIT>, dim3((unsigned)blocks), dim3(SH_THREADS), 0, s, src, dst, n_vec);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

extern "C" int pp_taps_upsample4_conv3x3(const float* taps, const float* bias, float* out, int n_img, int K, int h, int w, void* stream) {
    using namespace pp;
    PP_REQUIRE(n_img >= 0 && K > 0 && h > 0 && w > 0, PP_ERR_INVALID_ARG, "pp_taps_upsample4_conv3x3: bad n_img / K / h / w");
    if (n_img == 0) return PP_OK;  // empty batch: nothing to read or write (buffers may be NULL)
    PP_REQUIRE(taps && bias && out, PP_ERR_INVALID_ARG, "pp_taps_upsample4_conv3x3: taps, bias and out must be non-NULL");
    PP_REQUIRE(h <= (1 << 20) && w <= (1 << 20), PP_ERR_UNSUPPORTED, "pp_taps_upsample4_conv3x3: planes of at most 2^20 rows / columns");
    const long long tiles_y = (h + SH_TILE - 1) / SH_TILE, tiles_x = (w + SH_TILE - 1) / SH_TILE;
    const long long blocks = (long long)n_img * K * tiles_y * tiles_x;
    PP_REQUIRE(tiles_y * tiles_x < (1ll << 31) && blocks < (1ll << 31), PP_ERR_UNSUPPORTED, "pp_taps_upsample4_conv3x3: too many output tiles for one launch");
    const int vec_store = reinterpret_cast<uintptr_t>(out) % 16 == 0;  // (rows are 4 w floats: a 16-byte aligned base keeps every run of four aligned)
    hipLaunchKernelGGL(taps_upsample4_conv3x3_kernel, dim3((unsigned)blocks), dim3(SH_THREADS), 0, reinterpret_cast<hipStream_t>(stream), taps,
                       bias, out, K, h, w, (int)tiles_y, (int)tiles_x, vec_store);
    PP_LAUNCH_CHECK();
    return PP_OK;
}
