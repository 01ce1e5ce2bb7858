// ArgMaxProbMap decode for gfx950: ProbMapHead's map construction and the UDP argmax + DARK decode in ONE launch
//   logits -> x / T -> Sparsemax over the H*W pixels -> * normalize -> clamp(0,1) per pass -> flip-back + average   (probmap_head.py:637-646, 757-763)
//   -> first-occurrence argmax, Gaussian modulation, one Newton step on the log map, rescale                        (argmax_probmap.py decode:
//      get_heatmap_maximum + refine_keypoints_dark_udp, the steps of UDPHeatmap.decode)
// One 256-thread workgroup per (crop, keypoint). Both halves are the stages of pp_decode_stages.h, the very code pp_probmap_decode_flags
// (PP_DECODE_LOGITS) and pp_udp_heatmap_decode run in the same thread mapping, so this launch returns the bits of those two chained -
// without the averaged map's round trip through HBM (17 x 64 x 48 maps: 209 KB written and read again per crop).
//
// LDS: 512 bytes of reduction scratch (the Sparsemax stage's at the head, the DARK stage's from byte 256), then the x-padded map the
// Sparsemax stage writes ([H][W + 24]; its head doubles as that stage's candidate lists), then the DARK stage's map image A
// ([H][(W + 2 R) | 1]). The blur's row image Bf ([H + 2 R][W]) takes the padded map's place: that map is dead once it is copied into A.
// 64 x 48, kernel size 11: 0.5 + 18.1 + 15.9 = 34.5 KiB, four workgroups per CU; 96 x 72, size 17: 0.5 + 36.1 + 33.4 = 70 KiB, two.
#include "pp_common.h"

// numpy evaluates the fp32 expressions one rounding per operator; keep it so.
#pragma clang fp contract(off)

#include "pp_decode_stages.h"

namespace pp {
namespace {

static_assert(DEC_THREADS == UDP_THREADS, "the two stages share a workgroup");

// floats of the region the padded map, the candidate lists and the blur's row image share
size_t argmax_region_floats(int H, int W, int r) {
    size_t n = (size_t)H * (W + 2 * PAD) + 32;
    n = std::max(n, (size_t)2 * SMX_CAP);
    n = std::max(n, (size_t)(H + 2 * r) * W);
    return (n + 3) & ~(size_t)3;
}

template <bool HAS_FLIP, int NV, int RT>
__global__ __launch_bounds__(DEC_THREADS) void argmax_probmap_decode_kernel(
    const float* __restrict__ logits, const float* __restrict__ logits_flip, const int32_t* __restrict__ flip_indices, int K, int H,
    int W, double in_w, double in_h, float temperature, float normalize, UdpTaps taps, float* __restrict__ avg_out,
    float* __restrict__ locs, double* __restrict__ keypoints, float* __restrict__ scores, int phased, int shift, int radius,
    int region_floats) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int R = RT >= 0 ? RT : radius;
    const int bk = blockIdx.x;
    const int b = bk / K, k = bk - b * K;
    const int Wp = W + 2 * PAD;
    const UdpGeom g = udp_geom(H, W, R, 0, 0);  // (layout and shift are the Sparsemax stage's business)
    float* scr = reinterpret_cast<float*>(smem + 256);
    float* mapf = reinterpret_cast<float*>(smem + RED_BYTES);  // [H][Wp] averaged map of the Sparsemax stage
    float* Bf = mapf;                                          // [H + 2 R][W] row pass of the blur, once the map is in A
    float* A = mapf + region_floats;                           // [H][PA]
    udp_prepare<RT>(g, A, Bf, scr, taps, R, false);

    const size_t HW = (size_t)g.HW;
    auto fill = [&](int kk, float* avg_dst) -> UdpFill {
        const f32x4* src = reinterpret_cast<const f32x4*>(logits + ((size_t)b * K + kk) * HW);
        const f32x4* srcf = HAS_FLIP ? reinterpret_cast<const f32x4*>(logits_flip + ((size_t)b * K + flip_indices[kk]) * HW) : nullptr;
        UdpBest best{-__builtin_inff(), 0x7fffffff};
        auto nan_map = [&]() {
            if (avg_dst)
                for (int i = tid; i < g.HW; i += UDP_THREADS) avg_dst[i] = __builtin_nanf("");
        };
        if (!sparsemax_average<HAS_FLIP, NV>(src, srcf, smem, mapf, H, W, temperature, normalize, phased, shift, nan_map))  // (workgroup-uniform)
            return UdpFill{best, true};
        __syncthreads();  // the averaged map is complete
        {
            int y = tid / W, x = tid - y * W;
            for (int i = tid; i < g.HW; i += UDP_THREADS) {
                const float a = mapf[y * Wp + PAD + x];
                A[y * g.PA + R + x] = a;
                if (avg_dst) avg_dst[i] = a;
                if (a > best.v) best = UdpBest{a, i};  // (i ascends: the first of equal values stays)
                x += g.rx;
                y += g.qy;
                if (x >= W) {
                    x -= W;
                    ++y;
                }
            }
        }
        __syncthreads();  // every read of the padded map is through: the blur's row image takes its place, R zero rows either end
        for (int i = tid; i < R * W; i += UDP_THREADS) {
            Bf[i] = 0.f;
            Bf[(H + R) * W + i] = 0.f;
        }
        return UdpFill{best, false};
    };
    udp_dark_decode<RT>(fill, bk, k, K, g, A, Bf, scr, taps, R, in_w, in_h, avg_out ? avg_out + (size_t)bk * HW : nullptr, locs,
                        keypoints, scores);
}

typedef void (*ArgmaxKernel)(const float*, const float*, const int32_t*, int, int, int, double, double, float, float, UdpTaps, float*,
                             float*, double*, float*, int, int, int, int);

template <int NV, int RT>
ArgmaxKernel argmax_pick(bool flip) {
    return flip ? argmax_probmap_decode_kernel<true, NV, RT> : argmax_probmap_decode_kernel<false, NV, RT>;
}

template <int NV>
ArgmaxKernel argmax_pick_r(int r, bool flip) {
    if (r == 5) return argmax_pick<NV, 5>(flip);  // blur_kernel_size 11 (sigma 2)
    if (r == 8) return argmax_pick<NV, 8>(flip);  // 17 (sigma 3)
    return argmax_pick<NV, -1>(flip);             // every other size: radius at run time
}

}  // namespace
}  // namespace pp

extern "C" int pp_argmax_probmap_decode(const float* logits, const float* logits_flip, const int32_t* flip_indices, int B, int K, int H,
                                        int W, double in_w, double in_h, float temperature, float normalize, int blur_kernel_size,
                                        float* avg_out, float* locs, double* keypoints, float* scores, int flags, void* stream) {
    using namespace pp;
    PP_REQUIRE((flags & ~(PP_DECODE_PHASED | PP_DECODE_SHIFT_HEATMAP)) == 0, PP_ERR_INVALID_ARG, "pp_argmax_probmap_decode: unknown flag");
    PP_REQUIRE(B >= 0 && K > 0 && H > 1 && W > 1, PP_ERR_INVALID_ARG, "pp_argmax_probmap_decode: bad B/K/H/W (maps of at least 2 x 2)");
    PP_REQUIRE(blur_kernel_size >= 1 && blur_kernel_size % 2 == 1, PP_ERR_INVALID_ARG, "pp_argmax_probmap_decode: blur_kernel_size must be odd");
    PP_REQUIRE(blur_kernel_size <= 2 * UDP_MAX_R + 1, PP_ERR_UNSUPPORTED, "pp_argmax_probmap_decode: blur_kernel_size above 19");
    PP_REQUIRE(temperature > 0.f, PP_ERR_INVALID_ARG, "pp_argmax_probmap_decode: temperature must be positive");
    PP_REQUIRE(W % 4 == 0, PP_ERR_UNSUPPORTED, "pp_argmax_probmap_decode: heatmap width must be a multiple of 4");
    const bool phased = (flags & PP_DECODE_PHASED) != 0;
    PP_REQUIRE(!phased || (H % 2 == 0 && W % 8 == 0), PP_ERR_UNSUPPORTED,
               "pp_argmax_probmap_decode: PP_DECODE_PHASED needs an even height and a width that is a multiple of 8");
    PP_REQUIRE((long)H * W <= 12288, PP_ERR_UNSUPPORTED, "pp_argmax_probmap_decode: H*W exceeds 12288 pixels");
    const int r = (blur_kernel_size - 1) / 2;
    const size_t region = argmax_region_floats(H, W, r);
    const size_t lds = RED_BYTES + (region + (size_t)H * ((W + 2 * r) | 1)) * 4;
    PP_REQUIRE(lds <= UDP_MAX_DYNAMIC_LDS, PP_ERR_UNSUPPORTED,
               "pp_argmax_probmap_decode: the Sparsemax map and the blur's map image exceed one CU's LDS");
    if (B == 0) return PP_OK;  // empty batch: nothing to read or write (buffers may be NULL)
    PP_REQUIRE(logits && locs && keypoints && scores, PP_ERR_INVALID_ARG,
               "pp_argmax_probmap_decode: logits, locs, keypoints and scores must be non-NULL");
    PP_REQUIRE(!logits_flip || flip_indices, PP_ERR_INVALID_ARG, "pp_argmax_probmap_decode: flip_indices is required when logits_flip is given");
    const UdpTaps taps = udp_gaussian_taps(blur_kernel_size);
    const bool flip = logits_flip != nullptr;
    const int nv = (H * W / 4 + DEC_THREADS - 1) / DEC_THREADS;
    ArgmaxKernel kern = nv <= 3 ? argmax_pick_r<3>(r, flip) : nv <= 7 ? argmax_pick_r<7>(r, flip) : argmax_pick_r<12>(r, flip);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(B * K), dim3(DEC_THREADS), lds, s, logits, logits_flip, flip_indices, K, H, W, in_w, in_h, temperature,
                       normalize, taps, avg_out, locs, keypoints, scores, phased ? 1 : 0, (flip && (flags & PP_DECODE_SHIFT_HEATMAP)) ? 1 : 0, r,
                       (int)region);
    PP_LAUNCH_CHECK_AS("pp_argmax_probmap_decode");
    return PP_OK;
}
