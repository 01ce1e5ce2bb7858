// The OKS map loss for gfx950: OKSHeatmapLoss.forward(per_pixel=True), oks_type "minus" (mmpose/models/losses/heatmap_loss.py:552-638)
// reduced to its mean, and the argmax pixels of prediction and target that pose_pck_accuracy(method="argmax") reads - what
// ProbMapHead.loss needs of the maps (probmap_head.py:878-879, 905), in two launches.
//
// Launch one, one 256-thread workgroup per (instance, keypoint) map: the predicted map is staged once in LDS with a one-pixel zero
// halo (pitch W + 2: 13.2 KB for 64 x 48; with the 6 KB of reduction scratch eight workgroups fit a CU's 160 KB, which is the 32-wave
// cap as well), so the eight Sobel taps and the centre of every pixel are LDS reads instead of nine global ones and the border needs no
// branches. Consecutive lanes own consecutive pixels: global loads of the target coalesce, and a wave's LDS reads walk
// consecutive banks within a row. Sums are fp64 and leave the workgroup through a fixed tree; launch two (one workgroup) adds the
// per-map sums in a fixed order as well. No atomics anywhere: the result is the same bits launch after launch.
// The phase bodies are in pp_probmap_loss_core.h, shared with the sequential host form (scripts/probmap_loss_host_check.cpp).
#include "pp_common.h"
#include "pp_probmap_loss_core.h"

namespace pp {
namespace {

static_assert(PML_MAX_TILE_FLOATS == PP_PROBMAP_LOSS_MAX_TILE, "header and core disagree on the LDS stage");

// Fixed tree over the workgroup's partials; the result is in red[0] after the last barrier.
__device__ __forceinline__ void pml_block_reduce(PmlPartial* red, const PmlPartial& mine) {
    const int tid = threadIdx.x;
    red[tid] = mine;
    __syncthreads();
    for (int stride = PML_THREADS / 2; stride >= 1; stride >>= 1) {
        if (tid < stride) pml_reduce_step(red, tid, stride);
        __syncthreads();
    }
}

__global__ __launch_bounds__(PML_THREADS) void probmap_loss_maps_kernel(
    const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ weights, int H, int W, double sw, double ow,
    double gw, double* __restrict__ map_sums, int32_t* __restrict__ argmax, float* __restrict__ maxval) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    PmlPartial* red = reinterpret_cast<PmlPartial*>(smem);                   // [PML_THREADS]
    float* tile = reinterpret_cast<float*>(smem + sizeof(PmlPartial) * PML_THREADS);  // [(H + 2) (W + 2)]
    const size_t bk = blockIdx.x;
    const int tid = threadIdx.x;
    const size_t HW = (size_t)H * W;
    pml_stage(tile, pred + bk * HW, H, W, tid, PML_THREADS);
    __syncthreads();
    const PmlPartial mine = pml_accumulate(tile, target + bk * HW, H, W, sw, ow, gw, tid, PML_THREADS);
    pml_block_reduce(red, mine);
    if (tid == 0) {
        const PmlPartial r = red[0];
        map_sums[bk] = (double)weights[bk] * r.sum;  // _get_mask: the keypoint's weight over its whole map (heatmap_loss.py:655-668)
        argmax[2 * bk] = r.p.i;
        argmax[2 * bk + 1] = r.t.i;
        maxval[2 * bk] = r.p.v;
        maxval[2 * bk + 1] = r.t.v;
    }
}

__global__ __launch_bounds__(PML_THREADS) void probmap_loss_mean_kernel(const double* __restrict__ map_sums, long count, double scale,
                                                                        float* __restrict__ loss) {
    __shared__ PmlPartial red[PML_THREADS];
    const PmlBest none{0.f, 0};
    pml_block_reduce(red, PmlPartial{pml_sum_strided(map_sums, count, threadIdx.x, PML_THREADS), none, none});
    if (threadIdx.x == 0) loss[0] = (float)(red[0].sum * scale);
}

struct PmsTables {
    double vars[PML_COCO_K];
    double loss_weights[4];
};

// One workgroup: the scalar targets and the four scalar losses of a batch (pp_probmap_loss_core.h, "scalar targets and losses").
__global__ __launch_bounds__(PML_THREADS) void probmap_loss_scalars_kernel(PmsArgs a, PmsTables tab, float* __restrict__ out) {
    __shared__ PmsPartial red[PML_THREADS];
    __shared__ PmsPartial counts;
    const int tid = threadIdx.x;
    a.vars = tab.vars;
    auto reduce = [&](const PmsPartial& mine) {
        red[tid] = mine;
        __syncthreads();
        for (int stride = PML_THREADS / 2; stride >= 1; stride >>= 1) {
            if (tid < stride) pms_reduce_step(red, tid, stride);
            __syncthreads();
        }
    };
    reduce(pms_phase_a(a, tid, PML_THREADS));  // (its barriers also publish gt_oks / gt_errs to the workgroup)
    if (tid == 0) counts = red[0];
    __syncthreads();
    const PmsPartial c = counts;
    reduce(pms_phase_b(a, c, tid, PML_THREADS));
    if (tid == 0) pms_finish(red[0], tab.loss_weights, (double)a.B * a.K, out);
}

}  // namespace
}  // namespace pp

extern "C" int pp_probmap_loss_scalars(const float* scalars, const unsigned char* in_image, const unsigned char* annotated,
                                       const unsigned char* visibility, const double* kp_gt, const double* kp_dt, int B, int K, int flags,
                                       const double* loss_weights_host, float* gt_oks, float* oks_weight, float* gt_errs,
                                       float* vis_weights, float* out, void* stream) {
    using namespace pp;
    PP_REQUIRE((flags & ~15) == 0, PP_ERR_INVALID_ARG, "pp_probmap_loss_scalars: unknown flag");
    PP_REQUIRE(B >= 0 && K > 0, PP_ERR_INVALID_ARG, "pp_probmap_loss_scalars: bad B/K");
    PP_REQUIRE(K == PML_COCO_K, PP_ERR_INVALID_ARG, "pp_probmap_loss_scalars: compute_oks's sigmas are COCO's: K must be 17");
    PP_REQUIRE(loss_weights_host, PP_ERR_INVALID_ARG, "pp_probmap_loss_scalars: loss_weights_host must be non-NULL");
    PP_REQUIRE((long long)B * K <= 0x7fffffffLL, PP_ERR_UNSUPPORTED, "pp_probmap_loss_scalars: B * K must fit 31 bits");
    if (B == 0) return PP_OK;  // empty batch: nothing to read or write (buffers may be NULL)
    PP_REQUIRE(scalars && in_image && annotated && visibility && kp_gt && kp_dt && gt_oks && oks_weight && gt_errs && vis_weights && out,
               PP_ERR_INVALID_ARG, "pp_probmap_loss_scalars: every buffer must be non-NULL");
    static const double tenths[PML_COCO_K] = {0.26, 0.25, 0.25, 0.35, 0.35, 0.79, 0.79, 0.72, 0.72, 0.62, 0.62, 1.07, 1.07, 0.87, 0.87, 0.89, 0.89};
    PmsTables tab;
    for (int k = 0; k < PML_COCO_K; ++k) {
        const double two_sigma = tenths[k] / 10.0 * 2;  // compute_oks: vars = (sigmas * 2) ** 2, sigmas = [...] / 10.0
        tab.vars[k] = two_sigma * two_sigma;
    }
    for (int i = 0; i < 4; ++i) tab.loss_weights[i] = loss_weights_host[i];
    PmsArgs a{};
    a.scalars = scalars, a.in_image = in_image, a.annotated = annotated, a.visibility = visibility, a.kp_gt = kp_gt, a.kp_dt = kp_dt;
    a.vars = nullptr;                                // (the kernel points it at its own copy of the table)
    a.area = (double)(48 * 64) * 0.53 + 2.220446049250313e-16;  // bbox [0, 0, 64, 48] whatever the map's size (:561-568); + np.spacing(1)
    a.B = B, a.K = K;
    a.freeze_oks = flags & PP_LOSS_FREEZE_OKS ? 1 : 0, a.freeze_error = flags & PP_LOSS_FREEZE_ERROR ? 1 : 0;
    a.prob_logits = flags & PP_LOSS_PROB_LOGITS ? 1 : 0, a.vis_logits = flags & PP_LOSS_VIS_LOGITS ? 1 : 0;
    a.gt_oks = gt_oks, a.oks_weight = oks_weight, a.gt_errs = gt_errs, a.vis_weights = vis_weights;
    hipLaunchKernelGGL(probmap_loss_scalars_kernel, dim3(1), dim3(PML_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a, tab, out);
    PP_LAUNCH_CHECK_AS("probmap_loss_scalars");
    return PP_OK;
}

extern "C" int pp_probmap_loss_maps(const float* pred, const float* target, const float* weights, int B, int K, int H, int W,
                                    double smoothing_weight, double gaussian_weight, double loss_weight, double* map_sums,
                                    int32_t* argmax, float* maxval, float* loss, void* stream) {
    using namespace pp;
    PP_REQUIRE(B >= 0 && K > 0 && H > 0 && W > 0, PP_ERR_INVALID_ARG, "pp_probmap_loss_maps: bad B/K/H/W");
    PP_REQUIRE((long long)(H + 2) * (W + 2) <= PML_MAX_TILE_FLOATS, PP_ERR_UNSUPPORTED,
               "pp_probmap_loss_maps: the map and its halo exceed the LDS stage ((H + 2) (W + 2) <= 15360 floats)");
    PP_REQUIRE((long long)B * K <= 0x7fffffffLL, PP_ERR_UNSUPPORTED, "pp_probmap_loss_maps: B * K must fit 31 bits");
    if (B == 0) return PP_OK;  // empty batch: nothing to read or write (buffers may be NULL)
    PP_REQUIRE(pred && target && weights && map_sums && argmax && maxval && loss, PP_ERR_INVALID_ARG,
               "pp_probmap_loss_maps: pred, target, weights, map_sums, argmax, maxval and loss must be non-NULL");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = sizeof(PmlPartial) * PML_THREADS + (size_t)(H + 2) * (W + 2) * sizeof(float);
    PP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(probmap_loss_maps_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    hipLaunchKernelGGL(probmap_loss_maps_kernel, dim3(B * K), dim3(PML_THREADS), lds, s, pred, target, weights, H, W, smoothing_weight,
                       1.0 - smoothing_weight - gaussian_weight, gaussian_weight, map_sums, argmax, maxval);
    PP_LAUNCH_CHECK_AS("probmap_loss_maps");
    const double scale = loss_weight / ((double)B * K * H * W);
    hipLaunchKernelGGL(probmap_loss_mean_kernel, dim3(1), dim3(PML_THREADS), 0, s, map_sums, (long)B * K, scale, loss);
    PP_LAUNCH_CHECK_AS("probmap_loss_mean");
    return PP_OK;
}
