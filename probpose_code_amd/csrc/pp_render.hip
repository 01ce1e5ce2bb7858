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
#include "pp_common.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace pp {

constexpr int PA_THREADS = 512;       // histogram workgroup
constexpr int PA_BINS = 2048;         // widest pass (11 bits)
constexpr int PA_MAX_PARTS = 32;      // workgroups per keypoint
constexpr int PA_PER_PART = 16384;    // values per workgroup below which fewer workgroups are used
constexpr int PA_STATE = 5;           // per keypoint: target, base, prefix bits, draw, exact mass above the prefix within the pass-0 bin
constexpr int RD_MAXK = 22;           // colours of the reference's table
__device__ __forceinline__ int pa_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__device__ __forceinline__ int pa_nbits(int pass) { return pass == 1 ? 11 : 10; }

// local_visualizer.py:523-547
__constant__ uint8_t PAREA_RGB[RD_MAXK][3] = {
    {230, 25, 75},  {60, 180, 75},  {255, 225, 25}, {0, 130, 200},   {245, 130, 48},  {145, 30, 180},
    {70, 240, 240}, {240, 50, 230}, {210, 245, 60}, {250, 190, 212}, {0, 128, 128},   {220, 190, 255},
    {255, 250, 200}, {128, 0, 0},   {170, 255, 195}, {128, 128, 0},  {255, 215, 180}, {255, 255, 255},
    {170, 110, 40}, {0, 0, 128},    {128, 128, 128}, {0, 0, 0}};

static int parea_parts(long long HW) {
    long long p = (HW + PA_PER_PART - 1) / PA_PER_PART;
    return (int)(p < 1 ? 1 : (p > PA_MAX_PARTS ? PA_MAX_PARTS : p));
}

__device__ __forceinline__ uint8_t sat_u8(float v) {  // v already rounded
    return (uint8_t)(v <= 0.f ? 0.f : (v >= 255.f ? 255.f : v));
}

// One pass of the radix select: per-workgroup fp64 mass histogram of the values of P[k] whose bits above `shift + nbits`
// equal the prefix chosen so far. parts (K, n_parts, PA_BINS); pass 0 also writes the workgroup's bad-value flag.
__global__ __launch_bounds__(PA_THREADS) void parea_hist_kernel(const float* __restrict__ P, const double* __restrict__ state,
                                                                double* __restrict__ parts, double* __restrict__ bad_parts,
                                                                long long HW, int n_parts, int pass) {
    __shared__ double h[PA_BINS];
    const int k = blockIdx.y, part = blockIdx.x;
    const int shift = pa_shift(pass), nbins = 1 << pa_nbits(pass);
    unsigned prefix = 0;
    if (pass > 0) {
        if (state[k * PA_STATE + 3] == 0.0) return;  // not drawn: the partials are not read
        prefix = (unsigned)state[k * PA_STATE + 2];
    }
    for (int b = threadIdx.x; b < nbins; b += PA_THREADS) h[b] = 0.0;
    __syncthreads();
    const long long per = (HW + n_parts - 1) / n_parts, lo = part * per, hi = lo + per < HW ? lo + per : HW;
    const float* p = P + (size_t)k * HW;
    int bad = 0, cur_bin = -1;
    double cur = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += PA_THREADS) {
        const float x = p[i];
        if (pass == 0 && !(x >= 0.f && x < __builtin_huge_valf())) {
            bad = 1;
            continue;
        }
        if (x == 0.f) continue;  // no mass (also -0.0, whose bits would land in the top bin)
        const unsigned u = __float_as_uint(x);
        if (pass > 0 && (u >> (shift + pa_nbits(pass))) != prefix) continue;
        const int bin = (int)((u >> shift) & (unsigned)(nbins - 1));
        if (bin != cur_bin) {  // neighbouring values mostly share a bin: one LDS atomic per run
            if (cur_bin >= 0) atomicAdd(&h[cur_bin], cur);
            cur_bin = bin;
            cur = 0.0;
        }
        cur += (double)x;
    }
    if (cur_bin >= 0) atomicAdd(&h[cur_bin], cur);
    bad = __syncthreads_or(bad);
    double* out = parts + ((size_t)k * n_parts + part) * PA_BINS;
    for (int b = threadIdx.x; b < nbins; b += PA_THREADS) out[b] = h[b];
    if (pass == 0 && threadIdx.x == 0) bad_parts[k * n_parts + part] = bad ? 1.0 : 0.0;
}

// One workgroup per keypoint: the partials reduced in part order, then the scan from the top bin down. 256 threads own 8
// consecutive bins each (in descending order); thread 0 scans the 256 chunk sums, then the 8 bins of the crossing chunk.
__global__ __launch_bounds__(256) void parea_select_kernel(const double* __restrict__ parts, const double* __restrict__ bad_parts,
                                                           double* __restrict__ state, float* __restrict__ thr, int* __restrict__ draw,
                                                           int n_parts, int pass) {
    __shared__ double m[PA_BINS];
    __shared__ double chunk[256];
    const int k = blockIdx.x, t = threadIdx.x;
    double* st = state + k * PA_STATE;
    if (pass > 0 && st[3] == 0.0) return;
    const int nbins = 1 << pa_nbits(pass), per = nbins / 256;
    double c = 0.0;
    for (int j = 0; j < per; ++j) {
        const int b = nbins - 1 - (t * per + j);
        double s = 0.0;
        for (int q = 0; q < n_parts; ++q) s += parts[((size_t)k * n_parts + q) * PA_BINS + b];
        m[b] = s;
        c += s;
    }
    chunk[t] = c;
    __syncthreads();
    if (t != 0) return;
    // mass{x >= v} = base + E: base = the (rounded) mass of the pass-0 bins above the chosen one, E = the exact mass of the
    // values above v inside the chosen pass-0 bin (one exponent: exact). Every comparison of passes 1 and 2 rounds once, so
    // the bin that crossed the target in one pass holds a sub-bin that crosses it in the next.
    double base = 0.0, E = 0.0, target;
    unsigned prefix = 0;
    if (pass == 0) {
        bool bad = false;
        for (int q = 0; q < n_parts; ++q) bad |= bad_parts[k * n_parts + q] != 0.0;
        double total = 0.0;
        for (int i = 0; i < 256; ++i) total += chunk[i];
        if (bad || !(total >= 0.75)) {
            st[3] = 0.0;
            thr[k] = 0.f;
            draw[k] = 0;
            return;
        }
        target = 0.75 * total;
    } else {
        target = st[0];
        base = st[1];
        prefix = (unsigned)st[2];
        E = st[4];
    }
    int ci = 255;
    for (int i = 0; i < 256; ++i) {
        if (base + (E + chunk[i]) >= target) {
            ci = i;
            break;
        }
        E += chunk[i];
    }
    int chosen = -1, last_nonzero = -1;
    for (int j = 0; j < per; ++j) {
        const int b = nbins - 1 - (ci * per + j);
        if (m[b] == 0.0) continue;
        last_nonzero = b;
        if (base + (E + m[b]) >= target) {
            chosen = b;
            break;
        }
        E += m[b];
    }
    // A bin is always found (see above); should it not be, the lowest non-empty bin keeps the result a value of the map.
    if (chosen < 0) chosen = last_nonzero >= 0 ? last_nonzero : 0;
    prefix = (prefix << pa_nbits(pass)) | (unsigned)chosen;
    st[0] = target;
    st[1] = pass == 0 ? E : base;
    st[2] = (double)prefix;
    st[3] = 1.0;
    st[4] = pass == 0 ? 0.0 : E;
    if (pass == 2) {
        thr[k] = __uint_as_float(prefix);
        draw[k] = 1;
    }
}

__device__ __forceinline__ bool on_rect(int x, int y, const int* r) {
    const int x1 = min(r[0], r[2]), x2 = max(r[0], r[2]), y1 = min(r[1], r[3]), y2 = max(r[1], r[3]);
    return ((y == y1 || y == y2) && x >= x1 && x <= x2) || ((x == x1 || x == x2) && y >= y1 && y <= y2);
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
    const int ix = x - pad_l, iy = y - pad_t;
    float c[3];
    if (ix >= 0 && ix < W && iy >= 0 && iy < H) {
        const uint8_t* s = img + ((size_t)iy * W + ix) * 3;
        c[0] = s[0], c[1] = s[1], c[2] = s[2];
    } else {
        c[0] = c[1] = c[2] = 80.f;
    }
    const size_t HW = (size_t)Hp * Wp, o = (size_t)y * Wp + x;
    for (int k = 0; k < K; ++k) {
        if (!s_draw[k]) continue;
        const float t = s_thr[k];
        const float* pk = P + k * HW;
        if (!(pk[o] > t)) continue;
        const bool edge = x == 0 || !(pk[o - 1] > t) || x == Wp - 1 || !(pk[o + 1] > t) || y == 0 || !(pk[o - Wp] > t) ||
                          y == Hp - 1 || !(pk[o + Wp] > t);
        for (int ch = 0; ch < 3; ++ch) {
            const float ck = (float)PAREA_RGB[k][ch];
            c[ch] = edge ? ck : (float)sat_u8(rintf(0.7f * ck + 0.3f * c[ch]));
        }
    }
    for (int b = 0; b < n_boxes; ++b)
        if (on_rect(x, y, boxes + 4 * b)) c[0] = 0.f, c[1] = 255.f, c[2] = 0.f;
    uint8_t* d = canvas + o * 3;
    d[0] = (uint8_t)c[0], d[1] = (uint8_t)c[1], d[2] = (uint8_t)c[2];
}

__device__ __forceinline__ float seg_dist2(float px, float py, float ax, float ay, float bx, float by) {
    const float ex = bx - ax, ey = by - ay, wx = px - ax, wy = py - ay;
    const float L2 = ex * ex + ey * ey;
    float t = L2 > 0.f ? (wx * ex + wy * ey) / L2 : 0.f;
    t = fminf(fmaxf(t, 0.f), 1.f);
    const float dx = wx - t * ex, dy = wy - t * ey;
    return dx * dx + dy * dy;
}

// int(v) strictly inside (0, lim): v >= 1 and v < lim (NaN fails both)
__device__ __forceinline__ bool int_inside(float v, int lim) { return v >= 1.f && v < (float)lim; }

__global__ __launch_bounds__(256) void draw_poses_kernel(const uint8_t* __restrict__ img, int H, int W, const float* __restrict__ kpts,
                                                         const float* __restrict__ vis, const int* __restrict__ boxes, int n, int K,
                                                         const int* __restrict__ skeleton, const uint8_t* __restrict__ link_rgb,
                                                         const uint8_t* __restrict__ kpt_rgb, int L, double kpt_thr, float r2, float h2,
                                                         float alpha, uint8_t* __restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t o = ((size_t)y * W + x) * 3;
    float c[3] = {(float)img[o], (float)img[o + 1], (float)img[o + 2]};
    const float px = (float)x, py = (float)y, oma = 1.f - alpha;
    for (int i = 0; i < n; ++i) {
        if (boxes && on_rect(x, y, boxes + 4 * i)) c[0] = 0.f, c[1] = 255.f, c[2] = 0.f;
        const float* kp = kpts + (size_t)i * K * 2;
        const float* vi = vis + (size_t)i * K;
        for (int l = 0; l < L; ++l) {
            const int a = skeleton[2 * l], b = skeleton[2 * l + 1];
            const float ax = kp[2 * a], ay = kp[2 * a + 1], bx = kp[2 * b], by = kp[2 * b + 1];
            if (!(int_inside(ax, W) && int_inside(ay, H) && int_inside(bx, W) && int_inside(by, H))) continue;
            if (!((double)vi[a] >= kpt_thr && (double)vi[b] >= kpt_thr)) continue;
            if (seg_dist2(px, py, (float)(int)ax, (float)(int)ay, (float)(int)bx, (float)(int)by) <= h2)
                for (int ch = 0; ch < 3; ++ch) c[ch] = (float)link_rgb[3 * l + ch];
        }
        for (int j = 0; j < K; ++j) {
            if (!((double)vi[j] >= kpt_thr)) continue;
            const float dx = px - kp[2 * j], dy = py - kp[2 * j + 1];
            if (dx * dx + dy * dy <= r2)
                for (int ch = 0; ch < 3; ++ch) c[ch] = (float)sat_u8(rintf(alpha * (float)kpt_rgb[3 * j + ch] + oma * c[ch]));
        }
    }
    out[o] = (uint8_t)c[0], out[o + 1] = (uint8_t)c[1], out[o + 2] = (uint8_t)c[2];
}

__global__ __launch_bounds__(256) void resize_bilinear_u8_kernel(const uint8_t* __restrict__ src, int Hs, int Ws,
                                                                 uint8_t* __restrict__ dst, int Hd, int Wd, float scale_x, float scale_y) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= Wd) return;
    float sx = fmaxf(((float)x + 0.5f) * scale_x - 0.5f, 0.f), sy = fmaxf(((float)y + 0.5f) * scale_y - 0.5f, 0.f);
    int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
    float fx = sx - (float)x0, fy = sy - (float)y0;
    if (x0 >= Ws - 1) x0 = Ws - 1, fx = 0.f;
    if (y0 >= Hs - 1) y0 = Hs - 1, fy = 0.f;
    const int x1 = min(x0 + 1, Ws - 1), y1 = min(y0 + 1, Hs - 1);
    const uint8_t *r0 = src + (size_t)y0 * Ws * 3, *r1 = src + (size_t)y1 * Ws * 3;
    uint8_t* d = dst + ((size_t)y * Wd + x) * 3;
    for (int ch = 0; ch < 3; ++ch) {
        const float top = (1.f - fx) * (float)r0[3 * x0 + ch] + fx * (float)r0[3 * x1 + ch];
        const float bot = (1.f - fx) * (float)r1[3 * x0 + ch] + fx * (float)r1[3 * x1 + ch];
        d[ch] = sat_u8(rintf((1.f - fy) * top + fy * bot));
    }
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
