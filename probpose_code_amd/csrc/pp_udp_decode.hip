// UDP heatmap decode with DARK refinement for gfx950 (the ViTPose baseline's codec), fused with the flip-test average:
//   (a + flip_back(b)) * 0.5 in fp32                                                   (heatmap_head.py:246-258, tta.py:35-39, 64-66)
//   -> first-occurrence argmax of the UNBLURRED average, score = that maximum          (post_processing.py:178-217)
//   -> zero-padded separable Gaussian blur, fp32 taps and sums, rescale to the original maximum, clip(1e-3, 50), log
//                                                                                       (post_processing.py:220-249, refinement.py:125-128)
//   -> seven-point derivative / Hessian in fp32 on the edge-replicated log map, (H + eps I)^+ and the step in fp64,
//      loc - step rounded to fp32, rescale to input pixels in fp64                      (refinement.py:130-157, udp_heatmap.py:193-194)
// One 256-thread workgroup per (crop, keypoint). The averaged map and the row pass each have an LDS image; consecutive lanes
// own consecutive pixels of a row in every pass, so within a row a ds_read_b32 / ds_write_b32 lane group walks consecutive banks
// whatever the pitch. A lane group that wraps into the next row jumps by the pitch: the averaged map's odd pitch keeps that jump off
// a multiple of the bank count (at most a 2-way overlap of a few lanes), the row-pass image (pitch W) takes what W gives.
// Only the nine log-map values around the maximum are ever clipped and logged.
//
// The stages from the averaged map on (and the reference's quirk for a map whose maximum is <= 0) are in pp_decode_stages.h;
// pp_argmax_decode.hip runs the same stages behind a Sparsemax.
#include <cmath>

// numpy evaluates the fp32 expressions one rounding per operator; keep it so.
#pragma clang fp contract(off)

#include "pp_decode_stages.h"

namespace pp {
namespace {

// Offset of pixel (y, x) in the phase-separated layout of pp_deconv_head: the four 2x2 output phases one after the other, each a
// (H/2, W/2) row-major block, ordered (y & 1, x & 1).
__device__ __forceinline__ int udp_phased_offset(const UdpGeom& g, int y, int x) {
    return (y & 1) * (g.HW >> 1) + (x & 1) * (g.HW >> 2) + (y >> 1) * (g.W >> 1) + (x >> 1);
}

// Averages one map into A (pitch PA, data from column R): this thread's pixels, the best of them and whether one was not finite.
template <bool HAS_FLIP>
__device__ __forceinline__ UdpFill udp_load_average(const float* __restrict__ src, const float* __restrict__ srcf,
                                                    float* __restrict__ avg_dst, const UdpGeom& g, float* __restrict__ A, int R) {
    const int tid = threadIdx.x;
    const int W = g.W, HW = g.HW, PA = g.PA;
    UdpBest best{-__builtin_inff(), 0x7fffffff};
    float chk = 0.f;
    int y = tid / W, x = tid - y * W;
    for (int i = tid; i < HW; i += UDP_THREADS) {
        float a = g.phased ? src[udp_phased_offset(g, y, x)] : src[i];
        chk = __builtin_fmaf(a, 0.f, chk);  // x * 0 is NaN for x = +-inf / NaN
        if (HAS_FLIP) {
            // flip back; shift_heatmap moves the flipped-back map one pixel to the right, column 0 keeps its value
            const int xf = g.shift ? (x >= 1 ? W - x : W - 1) : W - 1 - x;
            const float f = g.phased ? srcf[udp_phased_offset(g, y, xf)] : srcf[y * W + xf];
            chk = __builtin_fmaf(f, 0.f, chk);
            a = (a + f) * 0.5f;
        }
        A[y * PA + R + x] = a;
        if (avg_dst) avg_dst[i] = a;
        if (a > best.v) best = UdpBest{a, i};  // (i ascends: the first of equal values stays)
        x += g.rx;
        y += g.qy;
        if (x >= W) {
            x -= W;
            ++y;
        }
    }
    return UdpFill{best, chk != chk};
}

template <bool HAS_FLIP, int RT>
__global__ __launch_bounds__(UDP_THREADS) void udp_heatmap_decode_kernel(
    const float* __restrict__ maps, const float* __restrict__ maps_flip, const int32_t* __restrict__ flip_indices, int K, int H,
    int W, double in_w, double in_h, UdpTaps taps, float* __restrict__ avg_out, float* __restrict__ locs,
    double* __restrict__ keypoints, float* __restrict__ scores, int phased, int shift, int radius) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int R = RT >= 0 ? RT : radius;
    const int bk = blockIdx.x;
    const int b = bk / K, k = bk - b * K;
    const UdpGeom g = udp_geom(H, W, R, phased, shift);
    float* scr = reinterpret_cast<float*>(smem);
    float* A = scr + UDP_RED_FLOATS;  // [H][PA]
    float* Bf = A + H * g.PA;         // [H + 2 R][W]
    udp_prepare<RT>(g, A, Bf, scr, taps, R, true);

    const size_t HW = (size_t)g.HW;
    auto fill = [&](int kk, float* avg_dst) {
        const float* src = maps + ((size_t)b * K + kk) * HW;
        const float* srcf = HAS_FLIP ? maps_flip + ((size_t)b * K + flip_indices[kk]) * HW : nullptr;
        return udp_load_average<HAS_FLIP>(src, srcf, avg_dst, g, A, R);
    };
    udp_dark_decode<RT>(fill, bk, k, K, g, A, Bf, scr, taps, R, in_w, in_h, avg_out ? avg_out + (size_t)bk * HW : nullptr, locs,
                        keypoints, scores);
}

typedef void (*UdpKernel)(const float*, const float*, const int32_t*, int, int, int, double, double, UdpTaps, float*, float*, double*,
                          float*, int, int, int);

template <int RT>
UdpKernel udp_pick(bool flip) {
    return flip ? udp_heatmap_decode_kernel<true, RT> : udp_heatmap_decode_kernel<false, RT>;
}

UdpKernel udp_kernel(int r, bool flip) {
    if (r == 5) return udp_pick<5>(flip);  // blur_kernel_size 11 (sigma 2)
    if (r == 8) return udp_pick<8>(flip);  // 17 (sigma 3)
    return udp_pick<-1>(flip);             // every other size: radius at run time
}

}  // namespace
}  // namespace pp

extern "C" int pp_udp_heatmap_decode(const float* maps, const float* maps_flip, const int32_t* flip_indices, int B, int K, int H,
                                     int W, double in_w, double in_h, int blur_kernel_size, float* avg_out, float* locs,
                                     double* keypoints, float* scores, int flags, void* stream) {
    using namespace pp;
    PP_REQUIRE((flags & ~(PP_DECODE_PHASED | PP_DECODE_SHIFT_HEATMAP)) == 0, PP_ERR_INVALID_ARG, "pp_udp_heatmap_decode: unknown flag");
    PP_REQUIRE(B >= 0 && K > 0 && H > 1 && W > 1, PP_ERR_INVALID_ARG, "pp_udp_heatmap_decode: bad B/K/H/W (maps of at least 2 x 2)");
    PP_REQUIRE(blur_kernel_size >= 1 && blur_kernel_size % 2 == 1, PP_ERR_INVALID_ARG, "pp_udp_heatmap_decode: blur_kernel_size must be odd");
    PP_REQUIRE(blur_kernel_size <= 2 * UDP_MAX_R + 1, PP_ERR_UNSUPPORTED, "pp_udp_heatmap_decode: blur_kernel_size above 19");
    const bool phased = (flags & PP_DECODE_PHASED) != 0;
    PP_REQUIRE(!phased || (H % 2 == 0 && W % 2 == 0), PP_ERR_UNSUPPORTED, "pp_udp_heatmap_decode: PP_DECODE_PHASED needs an even height and width");
    if (B == 0) return PP_OK;  // empty batch: nothing to read or write (buffers may be NULL)
    PP_REQUIRE(maps && locs && keypoints && scores, PP_ERR_INVALID_ARG, "pp_udp_heatmap_decode: maps, locs, keypoints and scores must be non-NULL");
    PP_REQUIRE(!maps_flip || flip_indices, PP_ERR_INVALID_ARG, "pp_udp_heatmap_decode: flip_indices is required when maps_flip is given");
    PP_REQUIRE((long)H * W <= 12288, PP_ERR_UNSUPPORTED, "pp_udp_heatmap_decode: H*W exceeds 12288 pixels");
    const int r = (blur_kernel_size - 1) / 2;
    const size_t lds = ((size_t)UDP_RED_FLOATS + (size_t)H * ((W + 2 * r) | 1) + (size_t)(H + 2 * r) * W) * 4;
    PP_REQUIRE(lds <= UDP_MAX_DYNAMIC_LDS, PP_ERR_UNSUPPORTED, "pp_udp_heatmap_decode: the map and its blur halo exceed one CU's LDS");
    const UdpTaps taps = udp_gaussian_taps(blur_kernel_size);
    UdpKernel kern = udp_kernel(r, maps_flip != nullptr);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(B * K), dim3(UDP_THREADS), lds, s, maps, maps_flip, flip_indices, K, H, W, in_w, in_h, taps, avg_out,
                       locs, keypoints, scores, phased ? 1 : 0, (maps_flip && (flags & PP_DECODE_SHIFT_HEATMAP)) ? 1 : 0, r);
    PP_LAUNCH_CHECK();
    return PP_OK;
}
