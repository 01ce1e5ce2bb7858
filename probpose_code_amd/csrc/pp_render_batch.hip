// The --show-dir pictures of a whole batch of samples in one set of launches: what pp_revert_heatmaps_max,
// pp_heatmap_posterior, pp_parea_thresholds, pp_parea_compose, pp_draw_poses and pp_resize_bilinear_u8 (pp_warp.hip,
// pp_render.hip) give picture by picture - about twelve launches and nine small uploads each - for every picture of a
// device table at once. The pictures differ in size, so every stage that runs over pixels is one launch over a flat list of
// row tiles (256 pixels of one row): the caller builds the exclusive prefix of the pictures' tile counts and a workgroup
// finds its picture by a binary search in it, as the JPEG and PNG batch calls do. Stages whose partition per picture is
// fixed (the 64 sum parts, the at most 32 histogram parts, one select workgroup per keypoint) take the picture from
// blockIdx.z / blockIdx.y instead.
//
// Nothing is computed here that is not computed there: every stage calls the per-pixel / per-part body of
// pp_revert_core.h / pp_render_core.h that the single-picture kernel calls, with arguments read from the tables, and keeps
// that kernel's partition per picture (PS_PARTS sum parts with the same strided order and tree; parea_parts(Hp Wp)
// histogram parts reduced in part order; one PA_STATE record per picture and keypoint). The bytes are those of the
// single-picture path (tests/test_render_batch_gpu.py). Two things are stated here alone:
//   * a B G R source is swapped where the image is read (pose panel, compose); the outputs are R G B;
//   * the presence probability of a keypoint is the mean over the picture's instances, which the single-picture path takes
//     with torch (`probs.mean(dim=0)` on the device, float32). Its reduction order for fewer than 256 rows is restated in
//     presence_mean below: four running sums over the rows i = j mod 4, combined ((s0 + s1) + s2) + s3, times the float32
//     quotient K / (n K). Pictures with 256 instances or more are refused.
//
// Scratch: one share per heatmap picture (render_share below): its (K, Hp, Wp) float32 posterior maps, its (Hp, Wp, 3)
// canvas, the sum partials, the states, flags and histogram partials of the radix select, the thresholds.
// Built with -ffp-contract=off (csrc/Makefile), like the two files whose bodies it runs.
#include "pp_common.h"
#include "pp_render_core.h"
#include "pp_revert_core.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace pp {

static_assert(sizeof(pp_render_picture) == 72 && sizeof(pp_render_instance) == 608, "the table layouts are part of the ABI");
static_assert(PP_RENDER_MAX_KEYPOINTS == RV_MAXK, "the instance table holds what the revert admits");

struct RenderShare {  // byte offsets inside a picture's share
    long long maps, canvas, sums, state, bad, hist, thr, draw, total;
};

__host__ __device__ inline long long align256(long long v) { return (v + 255) / 256 * 256; }

__host__ __device__ inline RenderShare render_share(int K, long long HW) {
    const long long np = parea_parts(HW);
    RenderShare s;
    s.maps = 0;
    s.canvas = align256(s.maps + (long long)K * HW * 4);
    s.sums = align256(s.canvas + HW * 3);
    s.state = s.sums + (long long)K * PS_PARTS * 8;
    s.bad = s.state + (long long)K * PA_STATE * 8;
    s.hist = s.bad + (long long)K * np * 8;
    s.thr = s.hist + (long long)K * np * PA_BINS * 8;
    s.draw = s.thr + (long long)K * 4;
    s.total = align256(s.draw + (long long)K * 4);
    return s;
}

// prefix: n + 1 ascending values, prefix[0] = 0; b < prefix[n]. The picture p with prefix[p] <= b < prefix[p + 1] (a picture
// with no tile is never found); t <- b's index among that picture's tiles.
__device__ __forceinline__ int tile_picture(const int* __restrict__ prefix, int n, int b, int& t) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= b) lo = mid;
        else hi = mid;
    }
    t = b - prefix[lo];
    return lo;
}

// torch's float32 mean over the rows of an (n, K) tensor, n < 256 (see the header)
__device__ __forceinline__ float presence_mean(const pp_render_instance* __restrict__ inst, int n, int k, int K) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int i = 0;
    for (; i + 3 < n; i += 4)
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] + inst[i + j].presence[k];
    for (int j = 0; i + j < n; ++j) acc[j] = acc[j] + inst[i + j].presence[k];
    const float s = ((acc[0] + acc[1]) + acc[2]) + acc[3];
    return s * ((float)K / (float)(n * K));
}

__global__ __launch_bounds__(256) void batch_revert_kernel(const pp_render_picture* __restrict__ pics,
                                                           const pp_render_instance* __restrict__ inst, const int* __restrict__ tiles, int n,
                                                           uint8_t* __restrict__ scratch, int K, int hh, int hw) {
    int t;
    const pp_render_picture& pc = pics[tile_picture(tiles, n, blockIdx.x, t)];
    const int Hp = pc.canvas_h, Wp = pc.canvas_w, tx = (Wp + 255) / 256;
    const int y = t / tx, x = (t % tx) * 256 + (int)threadIdx.x;
    if (x >= Wp) return;
    const pp_render_instance* mine = inst + pc.first;
    revert_max_pixel([=](int b, const double*& M, const float*& maps) { M = mine[b].inverse, maps = mine[b].maps; }, pc.count, K, hh, hw,
                     reinterpret_cast<float*>(scratch + pc.scratch_offset), Hp, Wp, x, y);
}

// grid (PS_PARTS, K, n)
__global__ __launch_bounds__(256) void batch_partial_sum_kernel(const pp_render_picture* __restrict__ pics, uint8_t* __restrict__ scratch,
                                                                int K) {
    __shared__ double red[256];
    const pp_render_picture& pc = pics[blockIdx.z];
    if (!pc.heatmap) return;
    const int k = blockIdx.y, part = blockIdx.x, HW = pc.canvas_h * pc.canvas_w;
    uint8_t* share = scratch + pc.scratch_offset;
    const RenderShare sh = render_share(K, HW);
    channel_partial_sum(reinterpret_cast<const float*>(share + sh.maps) + (size_t)k * HW, HW, part, red,
                        reinterpret_cast<double*>(share + sh.sums) + k * PS_PARTS + part);
}

__global__ __launch_bounds__(256) void batch_scale_kernel(const pp_render_picture* __restrict__ pics,
                                                          const pp_render_instance* __restrict__ inst, const int* __restrict__ tiles, int n,
                                                          uint8_t* __restrict__ scratch, int K) {
    __shared__ float s_total[RV_MAXK], s_pr[RV_MAXK];
    int t;
    const pp_render_picture& pc = pics[tile_picture(tiles, n, blockIdx.x, t)];
    const int Hp = pc.canvas_h, Wp = pc.canvas_w, tx = (Wp + 255) / 256;
    const size_t HW = (size_t)Hp * Wp;
    uint8_t* share = scratch + pc.scratch_offset;
    const RenderShare sh = render_share(K, (long long)HW);
    if ((int)threadIdx.x < K) {
        s_total[threadIdx.x] = channel_total(reinterpret_cast<const double*>(share + sh.sums) + threadIdx.x * PS_PARTS);
        s_pr[threadIdx.x] = presence_mean(inst + pc.first, pc.count, threadIdx.x, K);
    }
    __syncthreads();
    const int y = t / tx, x = (t % tx) * 256 + (int)threadIdx.x;
    if (x >= Wp) return;
    float* v = reinterpret_cast<float*>(share + sh.maps) + (size_t)y * Wp + x;
    for (int k = 0; k < K; ++k) v[k * HW] = channel_scaled(v[k * HW], s_total[k], s_pr[k]);
}

// grid (PA_MAX_PARTS, K, n)
__global__ __launch_bounds__(PA_THREADS) void batch_hist_kernel(const pp_render_picture* __restrict__ pics, uint8_t* __restrict__ scratch,
                                                                int K, int pass) {
    __shared__ double h[PA_BINS];
    const pp_render_picture& pc = pics[blockIdx.z];
    if (!pc.heatmap) return;
    const long long HW = (long long)pc.canvas_h * pc.canvas_w;
    const int k = blockIdx.y, part = blockIdx.x, np = parea_parts(HW);
    if (part >= np) return;
    uint8_t* share = scratch + pc.scratch_offset;
    const RenderShare sh = render_share(K, HW);
    parea_hist_part(reinterpret_cast<const float*>(share + sh.maps) + (size_t)k * HW, reinterpret_cast<const double*>(share + sh.state) + k * PA_STATE,
                    reinterpret_cast<double*>(share + sh.hist) + ((size_t)k * np + part) * PA_BINS,
                    reinterpret_cast<double*>(share + sh.bad) + k * np + part, HW, np, part, pass, h);
}

// grid (K, n)
__global__ __launch_bounds__(256) void batch_select_kernel(const pp_render_picture* __restrict__ pics, uint8_t* __restrict__ scratch, int K,
                                                           int pass) {
    __shared__ double m[PA_BINS];
    __shared__ double chunk[256];
    const pp_render_picture& pc = pics[blockIdx.y];
    if (!pc.heatmap) return;
    const long long HW = (long long)pc.canvas_h * pc.canvas_w;
    const int k = blockIdx.x, np = parea_parts(HW);
    uint8_t* share = scratch + pc.scratch_offset;
    const RenderShare sh = render_share(K, HW);
    parea_select_one(reinterpret_cast<const double*>(share + sh.hist) + (size_t)k * np * PA_BINS,
                     reinterpret_cast<const double*>(share + sh.bad) + k * np, reinterpret_cast<double*>(share + sh.state) + k * PA_STATE,
                     reinterpret_cast<float*>(share + sh.thr) + k, reinterpret_cast<int*>(share + sh.draw) + k, np, pass, m, chunk);
}

__global__ __launch_bounds__(256) void batch_compose_kernel(const pp_render_picture* __restrict__ pics,
                                                            const pp_render_instance* __restrict__ inst, const int* __restrict__ tiles, int n,
                                                            uint8_t* __restrict__ scratch, int K) {
    __shared__ float s_thr[RD_MAXK];
    __shared__ int s_draw[RD_MAXK];
    int t;
    const pp_render_picture& pc = pics[tile_picture(tiles, n, blockIdx.x, t)];
    const int Hp = pc.canvas_h, Wp = pc.canvas_w, tx = (Wp + 255) / 256;
    uint8_t* share = scratch + pc.scratch_offset;
    const RenderShare sh = render_share(K, (long long)Hp * Wp);
    if ((int)threadIdx.x < K) {
        s_thr[threadIdx.x] = reinterpret_cast<const float*>(share + sh.thr)[threadIdx.x];
        s_draw[threadIdx.x] = reinterpret_cast<const int*>(share + sh.draw)[threadIdx.x];
    }
    __syncthreads();
    const int y = t / tx, x = (t % tx) * 256 + (int)threadIdx.x;
    if (x >= Wp) return;
    const pp_render_instance* mine = inst + pc.first;
    parea_compose_pixel(pc.image, pc.height, pc.width, pc.bgr != 0, pc.pad[0], pc.pad[1], reinterpret_cast<const float*>(share + sh.maps), K,
                        s_thr, s_draw, [=](int b) { return mine[b].rect_valid ? mine[b].rect : nullptr; }, pc.count, share + sh.canvas, Hp, Wp,
                        x, y);
}

__global__ __launch_bounds__(256) void batch_poses_kernel(const pp_render_picture* __restrict__ pics,
                                                          const pp_render_instance* __restrict__ inst, const int* __restrict__ tiles, int n,
                                                          int K, const int* __restrict__ skeleton, const uint8_t* __restrict__ link_rgb,
                                                          const uint8_t* __restrict__ kpt_rgb, int L, double kpt_thr, float r2, float h2,
                                                          float alpha) {
    int t;
    const pp_render_picture& pc = pics[tile_picture(tiles, n, blockIdx.x, t)];
    const int H = pc.height, W = pc.width, tx = (W + 255) / 256;
    const int y = t / tx, x = (t % tx) * 256 + (int)threadIdx.x;
    if (x >= W) return;
    const pp_render_instance* mine = inst + pc.first;
    draw_poses_pixel(
        pc.image, H, W, pc.bgr != 0,
        [=](int i, const float*& kp, const float*& vi, const int*& box) {
            kp = mine[i].keypoints, vi = mine[i].visible, box = mine[i].box_valid ? mine[i].box : nullptr;
        },
        pc.count, K, skeleton, link_rgb, kpt_rgb, L, kpt_thr, r2, h2, alpha, pc.out, x, y);
}

// the canvas of every heatmap picture resized to its image, into the lower half of its output
__global__ __launch_bounds__(256) void batch_resize_kernel(const pp_render_picture* __restrict__ pics, const int* __restrict__ tiles, int n,
                                                           const uint8_t* __restrict__ scratch, int K) {
    int t;
    const pp_render_picture& pc = pics[tile_picture(tiles, n, blockIdx.x, t)];
    if (!pc.heatmap) return;
    const int H = pc.height, W = pc.width, Hp = pc.canvas_h, Wp = pc.canvas_w, tx = (W + 255) / 256;
    const int y = t / tx, x = (t % tx) * 256 + (int)threadIdx.x;
    if (x >= W) return;
    const RenderShare sh = render_share(K, (long long)Hp * Wp);
    resize_bilinear_pixel(scratch + pc.scratch_offset + sh.canvas, Hp, Wp, pc.out + (size_t)H * W * 3, W, (float)Wp / (float)W,
                          (float)Hp / (float)H, x, y);
}

}  // namespace pp

extern "C" long long pp_render_batch_scratch_bytes(int K, int canvas_h, int canvas_w) {
    using namespace pp;
    PP_REQUIRE(K > 0 && K <= RD_MAXK && canvas_h > 0 && canvas_w > 0, PP_ERR_INVALID_ARG, "pp_render_batch_scratch_bytes: bad shape (K <= 22)");
    const long long HW = (long long)canvas_h * canvas_w;
    PP_REQUIRE(canvas_h <= 65535 && HW < (1LL << 29), PP_ERR_UNSUPPORTED,
               "pp_render_batch_scratch_bytes: canvas taller than 65535 or of 2^29 pixels or more");
    return render_share(K, HW).total;
}

extern "C" int pp_render_samples_batch(const pp_render_picture* pictures_host, const pp_render_instance* instances_host,
                                       const int* tiles_host, const pp_render_picture* pictures, const pp_render_instance* instances,
                                       const int* tiles, int n_pictures, int n_instances, int K, int hm_h, int hm_w, const int* skeleton,
                                       const void* link_rgb, const void* kpt_rgb, int n_links, double kpt_thr, float radius,
                                       float thickness, float alpha, void* scratch, long long scratch_bytes, void* stream) {
    using namespace pp;
    PP_REQUIRE(pictures_host && tiles_host && pictures && tiles, PP_ERR_INVALID_ARG, "pp_render_samples_batch: NULL table");
    PP_REQUIRE(n_pictures > 0 && n_instances >= 0 && K > 0 && n_links >= 0, PP_ERR_INVALID_ARG,
               "pp_render_samples_batch: counts must be positive (n_instances, n_links: not negative)");
    PP_REQUIRE(n_instances == 0 || (instances_host && instances && kpt_rgb), PP_ERR_INVALID_ARG,
               "pp_render_samples_batch: NULL instance table or keypoint colours");
    PP_REQUIRE(n_links == 0 || (skeleton && link_rgb), PP_ERR_INVALID_ARG, "pp_render_samples_batch: NULL skeleton or link colours");
    PP_REQUIRE(radius >= 0.f && thickness >= 0.f, PP_ERR_INVALID_ARG, "pp_render_samples_batch: negative radius or thickness");
    PP_REQUIRE(K <= RV_MAXK, PP_ERR_INVALID_ARG, "pp_render_samples_batch: more than 32 keypoints");
    PP_REQUIRE(n_pictures <= 65535, PP_ERR_UNSUPPORTED, "pp_render_samples_batch: more than 65535 pictures in a call");
    long long canvas_tiles = 0, image_tiles = 0;
    bool any_heatmap = false;
    for (int p = 0; p < n_pictures; ++p) {
        const pp_render_picture& pc = pictures_host[p];
        PP_REQUIRE(pc.image && pc.out, PP_ERR_INVALID_ARG, "pp_render_samples_batch: a picture without image or output");
        PP_REQUIRE(pc.height > 0 && pc.width > 0 && pc.count >= 0 && pc.first >= 0 && (long long)pc.first + pc.count <= n_instances,
                   PP_ERR_INVALID_ARG, "pp_render_samples_batch: a picture's shape or its rows of the instance table");
        PP_REQUIRE(pc.height <= 65535, PP_ERR_UNSUPPORTED, "pp_render_samples_batch: image taller than 65535");
        PP_REQUIRE(pc.count <= PP_RENDER_MAX_INSTANCES, PP_ERR_UNSUPPORTED, "pp_render_samples_batch: more than 255 instances in a picture");
        PP_REQUIRE(tiles_host[p] == canvas_tiles && tiles_host[n_pictures + 1 + p] == image_tiles, PP_ERR_INVALID_ARG,
                   "pp_render_samples_batch: the tile prefixes do not belong to the picture table");
        image_tiles += (long long)pc.height * ((pc.width + 255) / 256);
        if (pc.heatmap) {
            any_heatmap = true;
            PP_REQUIRE(pc.count > 0, PP_ERR_INVALID_ARG, "pp_render_samples_batch: a heatmap picture without instances");
            PP_REQUIRE(K <= RD_MAXK, PP_ERR_INVALID_ARG, "pp_render_samples_batch: more than 22 keypoints (the colour table)");
            PP_REQUIRE(hm_h > 0 && hm_w > 0, PP_ERR_INVALID_ARG, "pp_render_samples_batch: bad map shape");
            PP_REQUIRE(hm_h < 32768 && hm_w < 32768, PP_ERR_UNSUPPORTED, "pp_render_samples_batch: map sides too large");
            PP_REQUIRE(pc.pad[0] >= 0 && pc.pad[1] >= 0 && pc.pad[2] >= 0 && pc.pad[3] >= 0 &&
                           (long long)pc.canvas_h == (long long)pc.height + pc.pad[1] + pc.pad[3] &&
                           (long long)pc.canvas_w == (long long)pc.width + pc.pad[0] + pc.pad[2],
                       PP_ERR_INVALID_ARG, "pp_render_samples_batch: the canvas is not the image plus its padding");
            const long long HW = (long long)pc.canvas_h * pc.canvas_w;
            PP_REQUIRE(pc.canvas_h <= 65535 && HW < (1LL << 29), PP_ERR_UNSUPPORTED,
                       "pp_render_samples_batch: canvas taller than 65535 or of 2^29 pixels or more");
            PP_REQUIRE(scratch && pc.scratch_offset >= 0 && pc.scratch_offset % 256 == 0 &&
                           pc.scratch_offset + render_share(K, HW).total <= scratch_bytes,
                       PP_ERR_WORKSPACE, "pp_render_samples_batch: a picture's share lies outside the scratch");
            for (int i = 0; i < pc.count; ++i)
                PP_REQUIRE(instances_host[pc.first + i].maps, PP_ERR_INVALID_ARG, "pp_render_samples_batch: a heatmap instance without maps");
            canvas_tiles += (long long)pc.canvas_h * ((pc.canvas_w + 255) / 256);
        }
        PP_REQUIRE(canvas_tiles < (1LL << 31) - 1 && image_tiles < (1LL << 31) - 1, PP_ERR_UNSUPPORTED,
                   "pp_render_samples_batch: 2^31 row tiles or more in a call");
    }
    PP_REQUIRE(tiles_host[n_pictures] == canvas_tiles && tiles_host[2 * n_pictures + 1] == image_tiles, PP_ERR_INVALID_ARG,
               "pp_render_samples_batch: the tile prefixes do not belong to the picture table");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t* scr = reinterpret_cast<uint8_t*>(scratch);
    const int n = n_pictures;
    const int* image_prefix = tiles + n + 1;
    if (any_heatmap) {
        hipLaunchKernelGGL(batch_revert_kernel, dim3((unsigned)canvas_tiles), dim3(256), 0, s, pictures, instances, tiles, n, scr, K, hm_h, hm_w);
        PP_LAUNCH_CHECK();
        hipLaunchKernelGGL(batch_partial_sum_kernel, dim3(PS_PARTS, K, n), dim3(256), 0, s, pictures, scr, K);
        PP_LAUNCH_CHECK();
        hipLaunchKernelGGL(batch_scale_kernel, dim3((unsigned)canvas_tiles), dim3(256), 0, s, pictures, instances, tiles, n, scr, K);
        PP_LAUNCH_CHECK();
        for (int pass = 0; pass < 3; ++pass) {
            hipLaunchKernelGGL(batch_hist_kernel, dim3(PA_MAX_PARTS, K, n), dim3(PA_THREADS), 0, s, pictures, scr, K, pass);
            PP_LAUNCH_CHECK();
            hipLaunchKernelGGL(batch_select_kernel, dim3(K, n), dim3(256), 0, s, pictures, scr, K, pass);
            PP_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(batch_compose_kernel, dim3((unsigned)canvas_tiles), dim3(256), 0, s, pictures, instances, tiles, n, scr, K);
        PP_LAUNCH_CHECK();
    }
    const float h = fmaxf(thickness, 1.f) * 0.5f;
    hipLaunchKernelGGL(batch_poses_kernel, dim3((unsigned)image_tiles), dim3(256), 0, s, pictures, instances, image_prefix, n, K, skeleton,
                       reinterpret_cast<const uint8_t*>(link_rgb), reinterpret_cast<const uint8_t*>(kpt_rgb), n_links, kpt_thr,
                       radius * radius, h * h, alpha);
    PP_LAUNCH_CHECK();
    if (any_heatmap) {
        hipLaunchKernelGGL(batch_resize_kernel, dim3((unsigned)image_tiles), dim3(256), 0, s, pictures, image_prefix, n, scr, K);
        PP_LAUNCH_CHECK();
    }
    return PP_OK;
}
