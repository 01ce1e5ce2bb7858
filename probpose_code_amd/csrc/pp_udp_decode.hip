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
// The reference's quirk is kept: a map whose maximum is <= 0 has loc = (-1, -1), and the flat index of refinement.py:137-145
// then reads three of its seven points from the tail of the PREVIOUS keypoint's padded log map (keypoint K - 1 for k = 0:
// a negative index). Such a workgroup blurs that neighbour map as well, in the same LDS, and takes the two pixels it needs.
#include <cmath>

#include "pp_common.h"

// numpy evaluates the fp32 expressions one rounding per operator; keep it so.
#pragma clang fp contract(off)

namespace pp {
namespace {

constexpr int UDP_THREADS = 256;
constexpr int UDP_MAX_R = PP_MAX_RADIUS;  // blur_kernel_size <= 19
constexpr int UDP_RED_FLOATS = 64;        // head of the dynamic LDS region: cross-wave reduction scratch, from UDP_TAPS_AT the taps of the runtime-radius kernel
constexpr int UDP_TAPS_AT = 32;

struct UdpTaps {
    float t[2 * UDP_MAX_R + 1];
};

struct UdpBest {
    float v;
    int idx;
};

// np.argmax semantics: NaN counts as the maximum, first occurrence wins ties.
__device__ __forceinline__ bool udp_better(float v, int idx, float bv, int bidx) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || idx < bidx);
    return v > bv || (v == bv && idx < bidx);
}

__device__ __forceinline__ UdpBest udp_block_argmax(UdpBest b, float* scr) {
#pragma unroll
    for (int o = WAVE / 2; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(b.v, o);
        const int oi = __shfl_xor(b.idx, o);
        if (udp_better(ov, oi, b.v, b.idx)) b = UdpBest{ov, oi};
    }
    __syncthreads();  // the scratch may still be read from the reduction before
    if (lane_id() == 0) {
        scr[2 * wave_id()] = b.v;
        scr[2 * wave_id() + 1] = __builtin_bit_cast(float, b.idx);
    }
    __syncthreads();
    UdpBest r{scr[0], __builtin_bit_cast(int, scr[1])};
#pragma unroll
    for (int w = 1; w < UDP_THREADS / WAVE; ++w) {
        const float ov = scr[2 * w];
        const int oi = __builtin_bit_cast(int, scr[2 * w + 1]);
        if (udp_better(ov, oi, r.v, r.idx)) r = UdpBest{ov, oi};
    }
    return r;
}

// np.max semantics: a NaN wins
__device__ __forceinline__ float udp_nanmax(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }

__device__ __forceinline__ float udp_block_max(float v, float* scr) {
#pragma unroll
    for (int o = WAVE / 2; o >= 1; o >>= 1) v = udp_nanmax(v, __shfl_xor(v, o));
    __syncthreads();
    if (lane_id() == 0) scr[wave_id()] = v;
    __syncthreads();
    float r = scr[0];
#pragma unroll
    for (int w = 1; w < UDP_THREADS / WAVE; ++w) r = udp_nanmax(r, scr[w]);
    return r;
}

struct UdpGeom {
    int H, W, HW;
    int PA;      // pitch of the averaged / blurred map: W + 2 R zero columns, odd
    int qy, rx;  // UDP_THREADS = qy * W + rx: a thread's next pixel
    int phased, shift;
};

struct UdpStat {
    float omax;  // maximum of the averaged map (the score)
    int oidx;    // its first flat index
    float bmax;  // maximum of the blurred map
    bool bad;    // a non-finite input value
};

// Offset of pixel (y, x) in the phase-separated layout of pp_deconv_head: the four 2x2 output phases one after the other, each a
// (H/2, W/2) row-major block, ordered (y & 1, x & 1).
__device__ __forceinline__ int udp_phased_offset(const UdpGeom& g, int y, int x) {
    return (y & 1) * (g.HW >> 1) + (x & 1) * (g.HW >> 2) + (y >> 1) * (g.W >> 1) + (x >> 1);
}

// Averages one map into A (pitch PA, data from column R), blurs it into A again through Bf ((H + 2 R) rows of W, R zero rows either
// end) and returns the two maxima. The zero halos of A and Bf are the caller's; they are never written here.
// RT >= 0: the radius at compile time, taps from the kernel arguments (SGPRs), loops unrolled - the two kernel sizes the codec is used
// with (11 for sigma 2, 17 for sigma 3). RT < 0: any radius 0 .. 9 at run time, taps from LDS (`tl`, one broadcast read per tap). Both
// forms sum in the same order.
template <bool HAS_FLIP, int RT>
__device__ __forceinline__ UdpStat udp_process(const float* __restrict__ src, const float* __restrict__ srcf,
                                               float* __restrict__ avg_dst, const UdpGeom& g, float* __restrict__ A,
                                               float* __restrict__ Bf, float* __restrict__ scr, const UdpTaps& taps, int R) {
    const int tid = threadIdx.x;
    const float* tl = scr + UDP_TAPS_AT;
    const int W = g.W, HW = g.HW, PA = g.PA;
    UdpBest best{-__builtin_inff(), 0x7fffffff};
    float chk = 0.f;
    {
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
    }
    UdpStat st;
    st.bad = __syncthreads_or(chk != chk) != 0;
    best = udp_block_argmax(best, scr);  // (its barriers also publish A)
    st.omax = best.v;
    st.oidx = best.idx;
    // ---- row pass: Bf[y + R][x] = sum_j tap[j] * A[y][x - R + j], taps ascending, one rounding per operator
    {
        int y = tid / W, x = tid - y * W;
        for (int i = tid; i < HW; i += UDP_THREADS) {
            const float* p = A + y * PA + x;
            float acc = 0.f;
            if constexpr (RT >= 0) {
#pragma unroll
                for (int j = 0; j <= 2 * RT; ++j) acc = acc + taps.t[j] * p[j];
            } else {
                for (int j = 0; j <= 2 * R; ++j) acc = acc + tl[j] * p[j];
            }
            Bf[(y + R) * W + x] = acc;
            x += g.rx;
            y += g.qy;
            if (x >= W) {
                x -= W;
                ++y;
            }
        }
    }
    __syncthreads();
    // ---- column pass into A (the averaged map is dead: its maximum is known) + maximum of the blurred map
    float bm = -__builtin_inff();
    {
        int y = tid / W, x = tid - y * W;
        for (int i = tid; i < HW; i += UDP_THREADS) {
            const float* p = Bf + y * W + x;
            float acc = 0.f;
            if constexpr (RT >= 0) {
#pragma unroll
                for (int j = 0; j <= 2 * RT; ++j) acc = acc + taps.t[j] * p[j * W];
            } else {
                for (int j = 0; j <= 2 * R; ++j) acc = acc + tl[j] * p[j * W];
            }
            A[y * PA + R + x] = acc;
            bm = udp_nanmax(bm, acc);
            x += g.rx;
            y += g.qy;
            if (x >= W) {
                x -= W;
                ++y;
            }
        }
    }
    st.bmax = udp_block_max(bm, scr);  // (its barriers also publish the blurred map)
    return st;
}

// heatmaps[k] *= origin_max / (max(blur) + 1e-12); clip(1e-3, 50); log - for one pixel, fp32 throughout
__device__ __forceinline__ float udp_log_value(const float* A, const UdpGeom& g, int R, const UdpStat& st, int y, int x) {
    const float ratio = st.omax / (st.bmax + 1e-12f);
    float v = A[y * g.PA + R + x] * ratio;
    v = fminf(fmaxf(v, 1e-3f), 50.0f);
    return logf(v);
}

template <bool HAS_FLIP, int RT>
__global__ __launch_bounds__(UDP_THREADS) void udp_heatmap_decode_kernel(
    const float* __restrict__ maps, const float* __restrict__ maps_flip, const int32_t* __restrict__ flip_indices, int K, int H,
    int W, double in_w, double in_h, UdpTaps taps, float* __restrict__ avg_out, float* __restrict__ locs,
    double* __restrict__ keypoints, float* __restrict__ scores, int phased, int shift, int radius) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int R = RT >= 0 ? RT : radius;
    const int bk = blockIdx.x;
    const int b = bk / K, k = bk - b * K;
    UdpGeom g;
    g.H = H;
    g.W = W;
    g.HW = H * W;
    g.PA = (W + 2 * R) | 1;
    g.qy = UDP_THREADS / W;
    g.rx = UDP_THREADS - g.qy * W;
    g.phased = phased;
    g.shift = shift;
    float* scr = reinterpret_cast<float*>(smem);
    float* A = scr + UDP_RED_FLOATS;  // [H][PA]
    float* Bf = A + H * g.PA;         // [H + 2 R][W]

    if constexpr (RT < 0) {  // the taps into LDS (constant indices: the argument block is not indexed at run time)
#pragma unroll
        for (int j = 0; j <= 2 * UDP_MAX_R; ++j)
            if (tid == j) scr[UDP_TAPS_AT + j] = taps.t[j];
    }
    // zero halos: the columns of A either side of the map, the R rows of Bf above and below it
    {
        const int nh = g.PA - W;
        for (int i = tid; i < H * nh; i += UDP_THREADS) {
            const int y = i / nh, c = i - y * nh;
            A[y * g.PA + (c < R ? c : W + c)] = 0.f;
        }
        for (int i = tid; i < R * W; i += UDP_THREADS) {
            Bf[i] = 0.f;
            Bf[(H + R) * W + i] = 0.f;
        }
    }

    const size_t HW = (size_t)g.HW;
    const float* src = maps + (size_t)bk * HW;
    const float* srcf = HAS_FLIP ? maps_flip + ((size_t)b * K + flip_indices[k]) * HW : nullptr;
    UdpStat st = udp_process<HAS_FLIP, RT>(src, srcf, avg_out ? avg_out + (size_t)bk * HW : nullptr, g, A, Bf, scr, taps, R);

    // the seven points of refinement.py:139-145 (and the centre)
    float i_ = 0.f, ix1 = 0.f, iy1 = 0.f, ix1y1 = 0.f, ix1_y1_ = 0.f, ix1_ = 0.f, iy1_ = 0.f;
    float lx = -1.f, ly = -1.f;
    bool bad = st.bad;
    if (!bad && st.omax > 0.f) {
        const int yi = st.oidx / W, xi = st.oidx - yi * W;
        lx = (float)xi;
        ly = (float)yi;
        if (tid == 0) {
            const int xm = max(xi - 1, 0), xp = min(xi + 1, W - 1), ym = max(yi - 1, 0), yp = min(yi + 1, H - 1);  // np.pad(mode="edge")
            i_ = udp_log_value(A, g, R, st, yi, xi);
            ix1 = udp_log_value(A, g, R, st, yi, xp);
            iy1 = udp_log_value(A, g, R, st, yp, xi);
            ix1y1 = udp_log_value(A, g, R, st, yp, xp);
            ix1_y1_ = udp_log_value(A, g, R, st, ym, xm);
            ix1_ = udp_log_value(A, g, R, st, yi, xm);
            iy1_ = udp_log_value(A, g, R, st, ym, xi);
        }
    } else if (!bad) {
        // loc = (-1, -1): index = this map's padded corner. index, index + 1, index + W + 2, index + W + 3 are all pixel (0, 0) of
        // this map; index - 1 and index - W - 3 are pixel (H - 1, W - 1), index - 2 - W pixel (H - 1, 0) of the map before it.
        i_ = ix1 = iy1 = ix1y1 = udp_log_value(A, g, R, st, 0, 0);
        const int kn = k > 0 ? k - 1 : K - 1;
        const float* nsrc = maps + ((size_t)b * K + kn) * HW;
        const float* nsrcf = HAS_FLIP ? maps_flip + ((size_t)b * K + flip_indices[kn]) * HW : nullptr;
        __syncthreads();  // every thread has read pixel (0, 0)
        const UdpStat sn = udp_process<HAS_FLIP, RT>(nsrc, nsrcf, nullptr, g, A, Bf, scr, taps, R);
        bad = sn.bad;
        if (!bad) {
            ix1_y1_ = ix1_ = udp_log_value(A, g, R, sn, H - 1, W - 1);
            iy1_ = udp_log_value(A, g, R, sn, H - 1, 0);
        }
    }
    if (tid != 0) return;
    if (bad) {
        // project policy: a non-finite value must not decode to a pixel with a plausible score
        const float qnan = __builtin_nanf("");
        locs[2 * bk + 0] = locs[2 * bk + 1] = qnan;
        keypoints[2 * bk + 0] = keypoints[2 * bk + 1] = (double)qnan;
        scores[bk] = qnan;
        return;
    }
    const float dx = 0.5f * (ix1 - ix1_);
    const float dy = 0.5f * (iy1 - iy1_);
    const float dxx = ix1 - 2.f * i_ + ix1_;
    const float dyy = iy1 - 2.f * i_ + iy1_;
    const float dxy = 0.5f * (ix1y1 - ix1 - iy1 + i_ + i_ - ix1_ - iy1_ + ix1_y1_);
    // np.linalg.pinv(hessian + eps32 * eye(2)), fp64, default rcond 1e-15: for a symmetric 2x2 the singular values are the absolute
    // eigenvalues, M^+ = sum over |l_i| > rcond * max|l| of v_i v_i^T / l_i
    const double eps = 1.1920928955078125e-07;
    const double ha = (double)dxx + eps, hb = (double)dxy, hc = (double)dyy + eps;
    const double m = 0.5 * (ha + hc), d = 0.5 * (ha - hc), rad = hypot(d, hb);
    const double l1 = m + rad, l2 = m - rad;
    double vx = 1.0, vy = 0.0;  // eigenvector of l1; (-vy, vx) is l2's
    if (rad > 0.0) {
        if (d >= 0.0) {
            vx = d + rad;
            vy = hb;
        } else {
            vx = hb;
            vy = rad - d;
        }
        const double n = hypot(vx, vy);
        vx /= n;
        vy /= n;
    }
    const double cut = 1e-15 * fmax(fabs(l1), fabs(l2));
    const double gx = (double)dx, gy = (double)dy;
    double sx = 0.0, sy = 0.0;
    if (fabs(l1) > cut) {
        const double c1 = (vx * gx + vy * gy) / l1;
        sx += c1 * vx;
        sy += c1 * vy;
    }
    if (fabs(l2) > cut) {
        const double c2 = (-vy * gx + vx * gy) / l2;
        sx += c2 * -vy;
        sy += c2 * vx;
    }
    // keypoints[n] -= step on a float32 array: the difference is taken in fp64 and rounded once
    const float rx32 = (float)((double)lx - sx), ry32 = (float)((double)ly - sy);
    locs[2 * bk + 0] = lx;
    locs[2 * bk + 1] = ly;
    keypoints[2 * bk + 0] = (double)rx32 / (double)(W - 1) * in_w;
    keypoints[2 * bk + 1] = (double)ry32 / (double)(H - 1) * in_h;
    scores[bk] = st.omax;
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
    PP_REQUIRE(lds <= (size_t)160 * 1024, PP_ERR_UNSUPPORTED, "pp_udp_heatmap_decode: the map and its blur halo exceed one CU's LDS");
    // cv2.getGaussianKernel for sigma <= 0: sigma from the kernel size, factors normalised in double, rounded to fp32
    UdpTaps taps;
    {
        const double sigma = 0.3 * ((blur_kernel_size - 1) * 0.5 - 1.0) + 0.8;
        double e[2 * UDP_MAX_R + 1], sum = 0.0;
        for (int j = 0; j <= 2 * r; ++j) {
            const double t = (double)(j - r);
            e[j] = std::exp(-0.5 * t * t / (sigma * sigma));
            sum += e[j];
        }
        for (int j = 0; j <= 2 * UDP_MAX_R; ++j) taps.t[j] = j <= 2 * r ? (float)(e[j] / sum) : 0.f;
    }
    UdpKernel kern = udp_kernel(r, maps_flip != nullptr);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(B * K), dim3(UDP_THREADS), lds, s, maps, maps_flip, flip_indices, K, H, W, in_w, in_h, taps, avg_out,
                       locs, keypoints, scores, phased ? 1 : 0, (maps_flip && (flags & PP_DECODE_SHIFT_HEATMAP)) ? 1 : 0, r);
    PP_LAUNCH_CHECK();
    return PP_OK;
}
