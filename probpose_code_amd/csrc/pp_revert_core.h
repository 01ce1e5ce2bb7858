// The per-pixel and per-part bodies of the heatmap revert and of the posterior normalisation, shared by the kernels of one
// picture (pp_warp.hip) and those of a batch of pictures (pp_render_batch.hip): the arithmetic is stated once, here. Both
// files are built with -ffp-contract=off (csrc/Makefile; the reasons are in pp_warp.hip's header).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

namespace pp {

__device__ __forceinline__ int round_to_int(double v) {  // saturate_cast<int>(double) = cvRound: nearest, ties to even
    v = rint(v);
    return v >= 2147483647.0 ? 2147483647 : (v <= -2147483648.0 ? (int)0x80000000 : (int)v);
}

constexpr int RV_MAXK = 32;

// IEEE 754-2019 maximum (NaN if either operand is): one v_maximum3_f32 on gfx950, where fmaxf is one v_max_f32
__device__ __forceinline__ float max_keep_nan(float acc, float v) { return __builtin_elementwise_maximum(acc, v); }

// One pixel (x, y) of the (K, H, W) merged maps: cv2's float warp of every person's (K, hh, hw) maps (the same
// 5-fractional-bit source coordinates as the uint8 warp, the four weights in float32, v = s00 w00 + s01 w01 + s10 w10 +
// s11 w11, zero border), merged by np.max (NaN stays, the maxima start at -inf). person(b, M, hm) names person b's inverse
// map (six doubles) and its maps.
template <class Person>
__device__ __forceinline__ void revert_max_pixel(Person person, int n, int K, int hh, int hw, float* __restrict__ out, int H, int W,
                                                 int x, int y) {
    float acc[RV_MAXK];
#pragma unroll
    for (int k = 0; k < RV_MAXK; ++k) acc[k] = -__builtin_huge_valf();
    for (int b = 0; b < n; ++b) {
        const double* M;
        const float* hm;
        person(b, M, hm);
        const int X0 = round_to_int((M[1] * y + M[2]) * 1024.0) + 16, Y0 = round_to_int((M[4] * y + M[5]) * 1024.0) + 16;
        const int X = (X0 + round_to_int(M[0] * x * 1024.0)) >> 5, Y = (Y0 + round_to_int(M[3] * x * 1024.0)) >> 5;
        int sx = X >> 5, sy = Y >> 5;
        sx = sx > 32767 ? 32767 : (sx < -32768 ? -32768 : sx);
        sy = sy > 32767 ? 32767 : (sy < -32768 ? -32768 : sy);
        const bool x0in = sx >= 0 && sx < hw, x1in = sx + 1 >= 0 && sx + 1 < hw;
        const bool y0in = sy >= 0 && sy < hh, y1in = sy + 1 >= 0 && sy + 1 < hh;
        if (!((x0in || x1in) && (y0in || y1in))) {  // this person's map is 0 here (border value)
#pragma unroll
            for (int k = 0; k < RV_MAXK; ++k) acc[k] = max_keep_nan(acc[k], 0.f);
            continue;
        }
        const float ax = (float)(X & 31) * (1.f / 32.f), ay = (float)(Y & 31) * (1.f / 32.f);
        const float w00 = (1.f - ay) * (1.f - ax), w01 = (1.f - ay) * ax, w10 = ay * (1.f - ax), w11 = ay * ax;
        const float* s = hm + (ptrdiff_t)sy * hw + sx;
#pragma unroll
        for (int k = 0; k < RV_MAXK; ++k) {
            if (k < K) {
                const float* sk = s + (size_t)k * hh * hw;
                const float v00 = (x0in && y0in) ? sk[0] : 0.f, v01 = (x1in && y0in) ? sk[1] : 0.f;
                const float v10 = (x0in && y1in) ? sk[hw] : 0.f, v11 = (x1in && y1in) ? sk[hw + 1] : 0.f;
                const float v = v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11;
                acc[k] = max_keep_nan(acc[k], v);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < RV_MAXK; ++k)
        if (k < K) out[((size_t)k * H + y) * W + x] = acc[k];
}

// heatmaps / heatmaps.sum(axis=(1, 2)) * presence[k]   (local_visualizer.py:827-837): per-channel partial sums in float64
// (fixed order), then the scaling
constexpr int PS_PARTS = 64;

// One workgroup of 256 threads: part `part` of the PS_PARTS partial sums of one channel (HW values at ch) -> *out.
// red: 256 doubles of LDS. Every thread of the workgroup calls it.
__device__ __forceinline__ void channel_partial_sum(const float* __restrict__ ch, int HW, int part, double* red, double* __restrict__ out) {
    const size_t per = ((size_t)HW + PS_PARTS - 1) / PS_PARTS, lo = part * per, hi = lo + per < (size_t)HW ? lo + per : (size_t)HW;
    double s = 0.0;
    for (size_t i = lo + threadIdx.x; i < hi; i += 256) s += (double)ch[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

// The channel's sum from its PS_PARTS partials (in part order), as the float32 the values are divided by
__device__ __forceinline__ float channel_total(const double* __restrict__ parts) {
    double s = 0.0;
    for (int i = 0; i < PS_PARTS; ++i) s += parts[i];
    return (float)s;
}

__device__ __forceinline__ float channel_scaled(float v, float total, float presence) { return v / total * presence; }

}  // namespace pp
