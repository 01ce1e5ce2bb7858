// The --draw-heatmap picture on the device (mmpose/visualization/local_visualizer.py:215-343, 520-585, 796-865):
//   (a) pp_parea_thresholds   the probability-area threshold of every keypoint's posterior map, without a sort;
//   (b) pp_parea_compose      the padded canvas, the translucent areas with their outlines, the aspect-fixed boxes;
//   (c) pp_draw_poses         boxes, links and points of every instance on the un-padded image;
//   (d) pp_resize_bilinear_u8 the heatmap panel resized to the image (written under the pose panel by the caller's pointer).
//
// (a) Definition, per keypoint k: total = fp64 sum of P[k]; draw = 0 when a value is negative or non-finite or total < 0.75;
// otherwise thr = the largest value v present in P[k] with mass{x >= v} >= 0.75 total (fp64 masses) - what
// sorted_desc[searchsorted(cumsum(sorted_desc), 0.75 total)] gives (:560-568). Radix select on the float bit pattern
// (non-negative float32 bits are monotone in the value): three passes over bits 30..21, 20..10, 9..0 (the sign bit is 0
// for every value admitted), each an fp64 mass histogram of the values under the prefix chosen so far, then a scan from
// the top bin down for the first bin that brings the mass at or above the target.
// Every value of one bin has the same float exponent, so a bin's mass is a sum of multiples of one power of two below
// 2^(e+1): exact in fp64 while a map has fewer than 2^29 values (checked). The LDS atomics and the run-length combining
// therefore add exactly, in any order, and the per-workgroup partials are reduced in a fixed order: the threshold is
// the same bits run to run. Only the scans across bins round, in a fixed order (top bin down, 8-bin chunks); against
// an fp64 cumsum of the sorted values they can differ only when a mass lies within fp64 rounding of the target.
//
// (b) Per canvas pixel: the image inside a constant (80, 80, 80) border (cv2.copyMakeBorder); then for k = 0..K-1 with
// draw[k]: inside mask_k = P[k] > thr[k] (strict, :570) the pixel becomes sat_u8(rint(0.7f c_k + 0.3f p)) per channel
// (cv2.addWeighted(probmap_i, 0.7, painted, 0.3, 0) restricted to the mask, :574-579); then an outline pixel of mask_k -
// a mask pixel with a 4-neighbour outside the mask or outside the canvas - becomes c_k. That stands in for
// drawContours(thickness=1, LINE_4) of the RETR_EXTERNAL contours (:581-583). KNOWN DIFFERENCE: this rule also outlines
// the rims of holes in a mask, which cv2 does not, and cv2's LINE_4 diagonal steps can put an outline pixel one pixel
// outside the mask, which this rule never does. Last, the 1-px green rectangles of the boxes (:844-858).
//
// (c) Per image pixel, instance by instance: its box (1-px green outline), its links, its points (the reference's order is
// _draw_instances_kpts then the boxes; these rules are ours: the reference draws through matplotlib, anti-aliased and not
// reproducible). A link is skipped as in :285-297 (int positions strictly inside (0, W) x (0, H), both visibilities >=
// kpt_thr); a pixel (x, y) takes the link colour when its squared distance to the segment between the two int positions
// is <= h * h, h = max(thickness, 1) / 2. A point is drawn when its visibility >= kpt_thr: a pixel within squared distance
// radius * radius of the float keypoint is blended sat_u8(rint(alpha c + (1 - alpha) p)). fp32, no contraction:
//   segment  ex = bx - ax, ey = by - ay, wx = x - ax, wy = y - ay, L2 = ex ex + ey ey,
//            t = L2 > 0 ? (wx ex + wy ey) / L2 : 0, t = min(max(t, 0), 1), dx = wx - t ex, dy = wy - t ey, d2 = dx dx + dy dy
//   point    dx = x - kx, dy = y - ky, d2 = dx dx + dy dy
//
// (d) cv2.resize(INTER_LINEAR) restated in fp32: sx = (x + 0.5) (Ws / Wd) - 0.5 clamped at 0, x0 = floor(sx), fx = sx - x0,
// x1 = min(x0 + 1, Ws - 1) (x0 >= Ws - 1: x0 = Ws - 1, fx = 0); the same in y;
// v = (1 - fy) ((1 - fx) p00 + fx p01) + fy ((1 - fx) p10 + fx p11), sat_u8(rint(v)). cv2 itself uses fixed-point weights;
// cv2 is absent here, parity unpinned.
//
// All four are bandwidth-bound element-wise passes: one thread per pixel / map value.
// The per-pixel and per-part bodies are in pp_render_core.h: pp_render_batch.hip runs the same ones over many pictures at once.
#include "pp_common.h"
#include "pp_render_core.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace pp {

// parts (K, n_parts, PA_BINS), bad_parts (K, n_parts), state (K, PA_STATE)
__global__ __launch_bounds__(PA_THREADS) void parea_hist_kernel(const float* __restrict__ P, const double* __restrict__ state,
                                                                double* __restrict__ parts, double* __restrict__ bad_parts,
                                                                long long HW, int n_parts, int pass) {
    __shared__ double h[PA_BINS];
    const int k = blockIdx.y, part = blockIdx.x;
    parea_hist_part(P + (size_t)k * HW, state + k * PA_STATE, parts + ((size_t)k * n_parts + part) * PA_BINS,
                    bad_parts + k * n_parts + part, HW, n_parts, part, pass, h);
}

__global__ __launch_bounds__(256) void parea_select_kernel(const double* __restrict__ parts, const double* __restrict__ bad_parts,
                                                           double* __restrict__ state, float* __restrict__ thr, int* __restrict__ draw,
                                                           int n_parts, int pass) {
    __shared__ double m[PA_BINS];
    __shared__ double chunk[256];
    const int k = blockIdx.x;
    parea_select_one(parts + (size_t)k * n_parts * PA_BINS, bad_parts + k * n_parts, state + k * PA_STATE, thr + k, draw + k, n_parts,
                     pass, m, chunk);
}

__global__ __launch_bounds__(256) void parea_compose_kernel(const uint8_t* __restrict__ img, int H, int W, int pad_l, int pad_t,
                                                            const float* __restrict__ P, int K, const float* __restrict__ thr,
                                                            const int* __restrict__ draw, const int* __restrict__ boxes, int n_boxes,
                                                            uint8_t* __restrict__ canvas, int Hp, int Wp) {
    __shared__ float s_thr[RD_MAXK];
    __shared__ int s_draw[RD_MAXK];
    if ((int)threadIdx.x < K) {
        s_thr[threadIdx.x] = thr[threadIdx.x];
        s_draw[threadIdx.x] = draw[threadIdx.x];
    }
    __syncthreads();
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= Wp) return;
    parea_compose_pixel(img, H, W, false, pad_l, pad_t, P, K, s_thr, s_draw, [=](int b) { return boxes + 4 * b; }, n_boxes, canvas, Hp, Wp,
                        x, y);
}

__global__ __launch_bounds__(256) void draw_poses_kernel(const uint8_t* __restrict__ img, int H, int W, const float* __restrict__ kpts,
                                                         const float* __restrict__ vis, const int* __restrict__ boxes, int n, int K,
                                                         const int* __restrict__ skeleton, const uint8_t* __restrict__ link_rgb,
                                                         const uint8_t* __restrict__ kpt_rgb, int L, double kpt_thr, float r2, float h2,
                                                         float alpha, uint8_t* __restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    draw_poses_pixel(
        img, H, W, false,
        [=](int i, const float*& kp, const float*& vi, const int*& box) {
            kp = kpts + (size_t)i * K * 2, vi = vis + (size_t)i * K, box = boxes ? boxes + 4 * i : nullptr;
        },
        n, K, skeleton, link_rgb, kpt_rgb, L, kpt_thr, r2, h2, alpha, out, x, y);
}

__global__ __launch_bounds__(256) void resize_bilinear_u8_kernel(const uint8_t* __restrict__ src, int Hs, int Ws,
                                                                 uint8_t* __restrict__ dst, int Hd, int Wd, float scale_x, float scale_y) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= Wd) return;
    resize_bilinear_pixel(src, Hs, Ws, dst, Wd, scale_x, scale_y, x, y);
}

}  // namespace pp

extern "C" long long pp_parea_scratch_bytes(int K, int H, int W) {
    using namespace pp;
    PP_REQUIRE(K > 0 && K <= RD_MAXK && H > 0 && W > 0, PP_ERR_INVALID_ARG, "pp_parea_scratch_bytes: bad shape (K <= 22)");
    const long long np = parea_parts((long long)H * W);
    return ((long long)K * PA_STATE + (long long)K * np + (long long)K * np * PA_BINS) * (long long)sizeof(double);
}

extern "C" int pp_parea_thresholds(const float* maps, int K, int H, int W, void* scratch, float* thr, int* draw, void* stream) {
    using namespace pp;
    PP_REQUIRE(maps && scratch && thr && draw, PP_ERR_INVALID_ARG, "pp_parea_thresholds: NULL argument");
    PP_REQUIRE(K > 0 && K <= RD_MAXK && H > 0 && W > 0, PP_ERR_INVALID_ARG, "pp_parea_thresholds: bad shape (K <= 22)");
    const long long HW = (long long)H * W;
    PP_REQUIRE(HW < (1LL << 29), PP_ERR_UNSUPPORTED, "pp_parea_thresholds: maps of 2^29 values or more (fp64 bin masses no longer exact)");
    const int np = parea_parts(HW);
    double* state = reinterpret_cast<double*>(scratch);
    double* bad_parts = state + K * PA_STATE;
    double* parts = bad_parts + K * np;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (int pass = 0; pass < 3; ++pass) {
        hipLaunchKernelGGL(parea_hist_kernel, dim3(np, K), dim3(PA_THREADS), 0, s, maps, state, parts, bad_parts, HW, np, pass);
        PP_LAUNCH_CHECK();
        hipLaunchKernelGGL(parea_select_kernel, dim3(K), dim3(256), 0, s, parts, bad_parts, state, thr, draw, np, pass);
        PP_LAUNCH_CHECK();
    }
    return PP_OK;
}

extern "C" int pp_parea_compose(const void* image_rgb, int img_h, int img_w, int pad_left, int pad_top, const float* maps, int K,
                                const float* thr, const int* draw, const int* boxes, int n_boxes, void* canvas_rgb, int canvas_h,
                                int canvas_w, void* stream) {
    using namespace pp;
    PP_REQUIRE(image_rgb && maps && thr && draw && canvas_rgb && (boxes || n_boxes == 0), PP_ERR_INVALID_ARG,
               "pp_parea_compose: NULL argument");
    PP_REQUIRE(K > 0 && K <= RD_MAXK && img_h > 0 && img_w > 0 && canvas_h > 0 && canvas_w > 0 && n_boxes >= 0, PP_ERR_INVALID_ARG,
               "pp_parea_compose: bad shape (K <= 22)");
    PP_REQUIRE(pad_left >= 0 && pad_top >= 0 && pad_left + img_w <= canvas_w && pad_top + img_h <= canvas_h, PP_ERR_INVALID_ARG,
               "pp_parea_compose: the padded image does not fit the canvas");
    PP_REQUIRE(canvas_h <= 65535, PP_ERR_UNSUPPORTED, "pp_parea_compose: canvas taller than 65535");
    hipLaunchKernelGGL(parea_compose_kernel, dim3((canvas_w + 255) / 256, canvas_h), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint8_t*>(image_rgb), img_h, img_w, pad_left, pad_top, maps, K, thr, draw, boxes, n_boxes,
                       reinterpret_cast<uint8_t*>(canvas_rgb), canvas_h, canvas_w);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

extern "C" int pp_draw_poses(const void* image_rgb, int img_h, int img_w, const float* keypoints, const float* visible,
                             const int* boxes, int n, int K, const int* skeleton, const void* link_rgb, const void* kpt_rgb, int n_links,
                             double kpt_thr, float radius, float thickness, float alpha, void* out_rgb, void* stream) {
    using namespace pp;
    PP_REQUIRE(image_rgb && out_rgb && (n == 0 || (keypoints && visible && kpt_rgb)) && (n_links == 0 || (skeleton && link_rgb)),
               PP_ERR_INVALID_ARG, "pp_draw_poses: NULL argument");
    PP_REQUIRE(img_h > 0 && img_w > 0 && n >= 0 && K > 0 && n_links >= 0 && radius >= 0.f && thickness >= 0.f, PP_ERR_INVALID_ARG,
               "pp_draw_poses: bad shape or size");
    PP_REQUIRE(img_h <= 65535, PP_ERR_UNSUPPORTED, "pp_draw_poses: image taller than 65535");
    const float h = fmaxf(thickness, 1.f) * 0.5f;
    hipLaunchKernelGGL(draw_poses_kernel, dim3((img_w + 255) / 256, img_h), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint8_t*>(image_rgb), img_h, img_w, keypoints, visible, boxes, n, K, skeleton,
                       reinterpret_cast<const uint8_t*>(link_rgb), reinterpret_cast<const uint8_t*>(kpt_rgb), n_links, kpt_thr,
                       radius * radius, h * h, alpha, reinterpret_cast<uint8_t*>(out_rgb));
    PP_LAUNCH_CHECK();
    return PP_OK;
}

extern "C" int pp_resize_bilinear_u8(const void* src_rgb, int src_h, int src_w, void* dst_rgb, int dst_h, int dst_w, void* stream) {
    using namespace pp;
    PP_REQUIRE(src_rgb && dst_rgb, PP_ERR_INVALID_ARG, "pp_resize_bilinear_u8: NULL argument");
    PP_REQUIRE(src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0, PP_ERR_INVALID_ARG, "pp_resize_bilinear_u8: bad shape");
    PP_REQUIRE(dst_h <= 65535, PP_ERR_UNSUPPORTED, "pp_resize_bilinear_u8: output taller than 65535");
    hipLaunchKernelGGL(resize_bilinear_u8_kernel, dim3((dst_w + 255) / 256, dst_h), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint8_t*>(src_rgb), src_h, src_w, reinterpret_cast<uint8_t*>(dst_rgb), dst_h, dst_w,
                       (float)src_w / (float)dst_w, (float)src_h / (float)dst_h);
    PP_LAUNCH_CHECK();
    return PP_OK;
}
