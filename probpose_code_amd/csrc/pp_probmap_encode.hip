// ProbMap target generation for gfx950: ProbMap.encode (mmpose/codecs/probmap.py:98-168, codecs/utils/oks_map.py) for a whole batch
// in one launch. One 256-thread workgroup per (instance, keypoint) map; consecutive lanes write consecutive pixels. The arithmetic
// is fp64 (3072 exp per 64 x 48 map): the reference decides keypoint_weights on the float64 map - a keypoint far outside has a
// map that underflows to zero in fp64 long after it has in fp32 - so the decision is taken before the values are rounded for the
// store. The phase bodies are in pp_probmap_loss_core.h, shared with the sequential host form.
#include "pp_common.h"

// numpy evaluates dx**2 + dy**2, sqrt, **2, / one rounding per operator; keep it so.
#pragma clang fp contract(off)

#include "pp_probmap_loss_core.h"

namespace pp {
namespace {

struct EncodeS {
    double two_s[PML_COCO_K];  // 2 s per keypoint; with sigma > 0 (any K) only entry 0 is used
};

__global__ __launch_bounds__(PML_THREADS) void probmap_encode_kernel(
    const float* __restrict__ keypoints, const float* __restrict__ visible, int K, int H, int W, float in_w, float in_h, float scale_x,
    float scale_y, EncodeS tab, int per_keypoint, float* __restrict__ heatmaps, float* __restrict__ weights,
    unsigned char* __restrict__ annotated, unsigned char* __restrict__ in_image) {
    __shared__ int any_positive;
    const int bk = blockIdx.x, tid = threadIdx.x;
    const int k = bk % K;
    const float x = keypoints[2 * (size_t)bk], y = keypoints[2 * (size_t)bk + 1], vis = visible[bk];
    float* map = heatmaps + (size_t)bk * H * W;
    if (tid == 0) {
        any_positive = 0;
        annotated[bk] = vis > 0.f;
        in_image[bk] = pml_in_image(x, y, in_w, in_h);
    }
    if (vis < 0.5f) {  // unlabelled (oks_map.py:49-50): the zero map, the weight stays what it was
        pml_zero_map(map, H * W, tid, PML_THREADS);
        if (tid == 0) weights[bk] = vis;
        return;
    }
    __syncthreads();
    const double kx = (double)(x / scale_x), ky = (double)(y / scale_y);  // the float32 division of probmap.py:138
    const bool any = pml_encode_map(map, H, W, kx, ky, tab.two_s[per_keypoint ? k : 0], tid, PML_THREADS);
    if (any) any_positive = 1;  // (every writer stores the same value)
    __syncthreads();
    if (tid == 0) weights[bk] = any_positive ? 1.f : 0.f;
}

int encode_table(const char* who, int K, int H, int W, double sigma, EncodeS* tab) {
    if (!(K > 0 && H > 0 && W > 0)) return fail(PP_ERR_INVALID_ARG, "pp_probmap_encode: K, H and W must be positive");
    if (!(sigma > 0) && K != PML_COCO_K)
        return fail(PP_ERR_INVALID_ARG, "pp_probmap_encode: with sigma <= 0 the per-keypoint sigmas are COCO's: K must be 17");
    (void)who;
    for (int k = 0; k < PML_COCO_K; ++k) tab->two_s[k] = 2 * pml_keypoint_s(k, H, W, sigma);
    return PP_OK;
}

}  // namespace
}  // namespace pp

extern "C" int pp_probmap_encode_s(int K, int H, int W, double sigma, double* s_host) {
    using namespace pp;
    PP_REQUIRE(s_host, PP_ERR_INVALID_ARG, "pp_probmap_encode_s: s_host must be non-NULL");
    EncodeS tab;
    const int st = encode_table("pp_probmap_encode_s", K, H, W, sigma, &tab);
    if (st != PP_OK) return st;
    for (int k = 0; k < K; ++k) s_host[k] = pml_keypoint_s(sigma > 0 ? 0 : k, H, W, sigma);
    return PP_OK;
}

extern "C" int pp_probmap_encode(const float* keypoints, const float* visible, int B, int K, int H, int W, double in_w, double in_h,
                                 double sigma, float* heatmaps, float* keypoint_weights, unsigned char* annotated,
                                 unsigned char* in_image, void* stream) {
    using namespace pp;
    PP_REQUIRE(B >= 0, PP_ERR_INVALID_ARG, "pp_probmap_encode: B must not be negative");
    EncodeS tab;
    const int st = encode_table("pp_probmap_encode", K, H, W, sigma, &tab);
    if (st != PP_OK) return st;
    PP_REQUIRE(in_w > 0 && in_h > 0, PP_ERR_INVALID_ARG, "pp_probmap_encode: the input size must be positive");
    PP_REQUIRE((long long)B * K <= 0x7fffffffLL && (long long)H * W <= 0x7fffffffLL, PP_ERR_UNSUPPORTED,
               "pp_probmap_encode: B * K and H * W must fit 31 bits");
    if (B == 0) return PP_OK;  // empty batch: nothing to read or write (buffers may be NULL)
    PP_REQUIRE(keypoints && visible && heatmaps && keypoint_weights && annotated && in_image, PP_ERR_INVALID_ARG,
               "pp_probmap_encode: keypoints, visible, heatmaps, keypoint_weights, annotated and in_image must be non-NULL");
    // scale_factor = ((input_size - 1) / (heatmap_size - 1)).astype(float32) (probmap.py:87); a 1-pixel axis divides by zero: inf, as numpy
    const float sx = (float)((in_w - 1) / (double)(W - 1)), sy = (float)((in_h - 1) / (double)(H - 1));
    hipLaunchKernelGGL(probmap_encode_kernel, dim3(B * K), dim3(PML_THREADS), 0, reinterpret_cast<hipStream_t>(stream), keypoints, visible,
                       K, H, W, (float)in_w, (float)in_h, sx, sy, tab, sigma > 0 ? 0 : 1, heatmaps, keypoint_weights, annotated, in_image);
    PP_LAUNCH_CHECK_AS("probmap_encode");
    return PP_OK;
}
