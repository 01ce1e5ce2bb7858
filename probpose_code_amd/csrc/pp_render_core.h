// The per-pixel and per-part bodies of the --draw-heatmap picture, shared by the kernels of one picture (pp_render.hip, where
// the rules (a) - (d) are stated) and those of a batch of pictures (pp_render_batch.hip): the arithmetic is stated once,
// here. Both files are built with -ffp-contract=off (csrc/Makefile): the fp32 rules are restated in numpy op for op
// (tests/render_ref.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
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
static __constant__ uint8_t PAREA_RGB[RD_MAXK][3] = {
    {230, 25, 75},  {60, 180, 75},  {255, 225, 25}, {0, 130, 200},   {245, 130, 48},  {145, 30, 180},
    {70, 240, 240}, {240, 50, 230}, {210, 245, 60}, {250, 190, 212}, {0, 128, 128},   {220, 190, 255},
    {255, 250, 200}, {128, 0, 0},   {170, 255, 195}, {128, 128, 0},  {255, 215, 180}, {255, 255, 255},
    {170, 110, 40}, {0, 0, 128},    {128, 128, 128}, {0, 0, 0}};

__host__ __device__ inline int parea_parts(long long HW) {
    long long p = (HW + PA_PER_PART - 1) / PA_PER_PART;
    return (int)(p < 1 ? 1 : (p > PA_MAX_PARTS ? PA_MAX_PARTS : p));
}

__device__ __forceinline__ uint8_t sat_u8(float v) {  // v already rounded
    return (uint8_t)(v <= 0.f ? 0.f : (v >= 255.f ? 255.f : v));
}

// One pass of the radix select, one workgroup of PA_THREADS threads: the fp64 mass histogram of part `part` of the HW
// values at p (one keypoint's map) whose bits above `shift + nbits` equal the prefix chosen so far -> out (PA_BINS); pass 0
// also writes the part's bad-value flag. st: the keypoint's PA_STATE record; h: PA_BINS doubles of LDS. Every thread of the
// workgroup calls it.
__device__ __forceinline__ void parea_hist_part(const float* __restrict__ p, const double* __restrict__ st, double* __restrict__ out,
                                                double* __restrict__ bad_out, long long HW, int n_parts, int part, int pass, double* h) {
    const int shift = pa_shift(pass), nbins = 1 << pa_nbits(pass);
    unsigned prefix = 0;
    if (pass > 0) {
        if (st[3] == 0.0) return;  // not drawn: the partials are not read
        prefix = (unsigned)st[2];
    }
    for (int b = threadIdx.x; b < nbins; b += PA_THREADS) h[b] = 0.0;
    __syncthreads();
    const long long per = (HW + n_parts - 1) / n_parts, lo = part * per, hi = lo + per < HW ? lo + per : HW;
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
    for (int b = threadIdx.x; b < nbins; b += PA_THREADS) out[b] = h[b];
    if (pass == 0 && threadIdx.x == 0) *bad_out = bad ? 1.0 : 0.0;
}

// One workgroup of 256 threads per keypoint: the partials (n_parts, PA_BINS) reduced in part order, then the scan from the
// top bin down. The threads own 8 consecutive bins each (in descending order); thread 0 scans the 256 chunk sums, then the
// 8 bins of the crossing chunk. bad: the keypoint's n_parts flags; st: its PA_STATE record; m: PA_BINS, chunk: 256 doubles
// of LDS.
__device__ __forceinline__ void parea_select_one(const double* __restrict__ parts, const double* __restrict__ bad, double* __restrict__ st,
                                                 float* __restrict__ thr, int* __restrict__ draw, int n_parts, int pass, double* m,
                                                 double* chunk) {
    const int t = threadIdx.x;
    if (pass > 0 && st[3] == 0.0) return;
    const int nbins = 1 << pa_nbits(pass), per = nbins / 256;
    double c = 0.0;
    for (int j = 0; j < per; ++j) {
        const int b = nbins - 1 - (t * per + j);
        double s = 0.0;
        for (int q = 0; q < n_parts; ++q) s += parts[(size_t)q * PA_BINS + b];
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
        bool any_bad = false;
        for (int q = 0; q < n_parts; ++q) any_bad |= bad[q] != 0.0;
        double total = 0.0;
        for (int i = 0; i < 256; ++i) total += chunk[i];
        if (any_bad || !(total >= 0.75)) {
            st[3] = 0.0;
            *thr = 0.f;
            *draw = 0;
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
        *thr = __uint_as_float(prefix);
        *draw = 1;
    }
}

__device__ __forceinline__ bool on_rect(int x, int y, const int* r) {
    const int x1 = min(r[0], r[2]), x2 = max(r[0], r[2]), y1 = min(r[1], r[3]), y2 = max(r[1], r[3]);
    return ((y == y1 || y == y2) && x >= x1 && x <= x2) || ((x == x1 || x == x2) && y >= y1 && y <= y2);
}

// One canvas pixel (x, y) of the heatmap panel. img: (H, W, 3) uint8, R G B or (bgr) B G R - swapped where it is read, the
// canvas is RGB; thr / draw: the K thresholds and flags; rect(b): rectangle b of n_rects (x1, y1, x2, y2 in canvas pixels), or
// NULL for one that is not drawn.
template <class Rect>
__device__ __forceinline__ void parea_compose_pixel(const uint8_t* __restrict__ img, int H, int W, bool bgr, int pad_l, int pad_t,
                                                    const float* __restrict__ P, int K, const float* thr, const int* draw, Rect rect,
                                                    int n_rects, uint8_t* __restrict__ canvas, int Hp, int Wp, int x, int y) {
    const int ix = x - pad_l, iy = y - pad_t;
    float c[3];
    if (ix >= 0 && ix < W && iy >= 0 && iy < H) {
        const uint8_t* s = img + ((size_t)iy * W + ix) * 3;
        c[0] = s[bgr ? 2 : 0], c[1] = s[1], c[2] = s[bgr ? 0 : 2];
    } else {
        c[0] = c[1] = c[2] = 80.f;
    }
    const size_t HW = (size_t)Hp * Wp, o = (size_t)y * Wp + x;
    for (int k = 0; k < K; ++k) {
        if (!draw[k]) continue;
        const float t = thr[k];
        const float* pk = P + k * HW;
        if (!(pk[o] > t)) continue;
        const bool edge = x == 0 || !(pk[o - 1] > t) || x == Wp - 1 || !(pk[o + 1] > t) || y == 0 || !(pk[o - Wp] > t) ||
                          y == Hp - 1 || !(pk[o + Wp] > t);
        for (int ch = 0; ch < 3; ++ch) {
            const float ck = (float)PAREA_RGB[k][ch];
            c[ch] = edge ? ck : (float)sat_u8(rintf(0.7f * ck + 0.3f * c[ch]));
        }
    }
    for (int b = 0; b < n_rects; ++b) {
        const int* r = rect(b);
        if (r && on_rect(x, y, r)) c[0] = 0.f, c[1] = 255.f, c[2] = 0.f;
    }
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

// One pixel (x, y) of the pose panel. img as in parea_compose_pixel, out is RGB; instance(i, kp, vi, box) names instance i's
// (K, 2) keypoints, its K visibilities and its box (x1, y1, x2, y2), or NULL for no box.
template <class Instance>
__device__ __forceinline__ void draw_poses_pixel(const uint8_t* __restrict__ img, int H, int W, bool bgr, Instance instance, int n, int K,
                                                 const int* __restrict__ skeleton, const uint8_t* __restrict__ link_rgb,
                                                 const uint8_t* __restrict__ kpt_rgb, int L, double kpt_thr, float r2, float h2,
                                                 float alpha, uint8_t* __restrict__ out, int x, int y) {
    const size_t o = ((size_t)y * W + x) * 3;
    float c[3] = {(float)img[o + (bgr ? 2 : 0)], (float)img[o + 1], (float)img[o + (bgr ? 0 : 2)]};
    const float px = (float)x, py = (float)y, oma = 1.f - alpha;
    for (int i = 0; i < n; ++i) {
        const float *kp, *vi;
        const int* box;
        instance(i, kp, vi, box);
        if (box && on_rect(x, y, box)) c[0] = 0.f, c[1] = 255.f, c[2] = 0.f;
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

// One pixel (x, y) of the (Hd, Wd, 3) bilinear resize of src (Hs, Ws, 3); scale_x = Ws / Wd, scale_y = Hs / Hd in float32
__device__ __forceinline__ void resize_bilinear_pixel(const uint8_t* __restrict__ src, int Hs, int Ws, uint8_t* __restrict__ dst, int Wd,
                                                      float scale_x, float scale_y, int x, int y) {
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
