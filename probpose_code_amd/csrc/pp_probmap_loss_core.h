// Phase bodies of the ProbMap target generator (pp_probmap_encode.hip) and of the OKS map loss (pp_probmap_loss.hip), shared with
// a sequential host form (scripts/probmap_loss_host_check.cpp runs every phase for thread 0 .. n-1 in turn, under the host
// sanitizers). Every phase is written for "thread tid of n": the kernels call it with their thread index, the host form in a loop.
//
//   encode   ProbMap.encode (codecs/probmap.py:98-168, codecs/utils/oks_map.py): exp(-d^2 / 2s) in fp64 around the keypoint divided
//            by the codec's float32 scale factor; the weight is decided on the fp64 values, the map is stored as float32.
//   loss     OKSHeatmapLoss.forward, oks_type "minus", per_pixel (models/losses/heatmap_loss.py:552-638): per pixel
//            sw (Gx^2 + Gy^2) + ow p (1 - t) + gw (p - t)^2, each term times the keypoint's weight; Gx, Gy the 3x3 Sobel responses of p
//            with zero padding. The map is staged once with a one-pixel zero halo (pitch W + 2) and every tap reads the stage.
//            Products and sums are fp64: the per-map sum is then the fp64 value up to the order of 256 partial sums, which is fixed.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PP_HD __host__ __device__ __forceinline__
#else
#define PP_HD inline
#endif

namespace pp {

constexpr int PML_THREADS = 256;
constexpr int PML_COCO_K = 17;
// the staged map with its halo, (H + 2) (W + 2) floats, shares the workgroup's 64 KB with the reduction scratch
constexpr long PML_MAX_TILE_FLOATS = 15360;

struct PmlBest {  // a maximum and its row-major index
    float v;
    int i;
};

struct PmlPartial {
    double sum;
    PmlBest p, t;
};

// numpy's argmax order: the first NaN wins, else the larger value, else the lower index
PP_HD bool pml_better(const PmlBest& a, const PmlBest& b) {
    const bool an = a.v != a.v, bn = b.v != b.v;
    if (an != bn) return an;
    if (!an && a.v != b.v) return a.v > b.v;
    return a.i < b.i;
}

// s = clip((2 sigma_k)^2 sqrt(H / 1.25 * W / 1.25) 2, 0.55, 3.0); a positive sigma replaces it (oks_map.py:39-61)
inline double pml_keypoint_s(int k, int H, int W, double sigma) {
    static const double hundredths[PML_COCO_K] = {2.6, 2.5, 2.5, 3.5, 3.5, 7.9, 7.9, 7.2, 7.2, 6.2, 6.2, 10.7, 10.7, 8.7, 8.7, 8.9, 8.9};
    if (sigma > 0) return sigma;
    const double area = std::sqrt(H / 1.25 * W / 1.25);
    const double two_sigma = hundredths[k] / 100 * 2;
    double s = two_sigma * two_sigma * area * 2;
    return s < 0.55 ? 0.55 : (s > 3.0 ? 3.0 : s);
}

// ---- encode ---------------------------------------------------------------------------------------------------------------------
// One rounding per operator, as numpy evaluates it: dist = sqrt(dx^2 + dy^2); e = dist^2 / (2 s); exp(-e).
PP_HD double pml_oks_value(int y, int x, double kx, double ky, double two_s) {
#pragma clang fp contract(off)
    const double dx = (double)x - kx, dy = (double)y - ky;
    const double dx2 = dx * dx, dy2 = dy * dy;
    const double dist = sqrt(dx2 + dy2);
    const double e = dist * dist / two_s;
    return exp(-e);
}

// Thread tid of n fills its pixels of one map; returns whether one of their fp64 values is above zero.
PP_HD bool pml_encode_map(float* map, int H, int W, double kx, double ky, double two_s, int tid, int n) {
    bool any = false;
    const int HW = H * W;
    for (int i = tid; i < HW; i += n) {
        const int y = i / W, x = i - y * W;
        const double v = pml_oks_value(y, x, kx, ky, two_s);
        any = any || v > 0.0;
        map[i] = (float)v;
    }
    return any;
}

PP_HD void pml_zero_map(float* map, int HW, int tid, int n) {
    for (int i = tid; i < HW; i += n) map[i] = 0.f;
}

// the four comparisons of probmap.py:145-156 on the unscaled coordinates (a NaN coordinate is outside)
PP_HD bool pml_in_image(float x, float y, float in_w, float in_h) { return x >= 0.f && x < in_w && y >= 0.f && y < in_h; }

// ---- loss -----------------------------------------------------------------------------------------------------------------------
// Stage p with its zero halo: tile is (H + 2) x (W + 2), pixel (y, x) at [(y + 1) (W + 2) + x + 1].
PP_HD void pml_stage(float* tile, const float* p, int H, int W, int tid, int n) {
    const int P = W + 2, T = (H + 2) * P;
    for (int i = tid; i < T; i += n) {
        const int yy = i / P, xx = i - yy * P;
        const bool inside = yy >= 1 && yy <= H && xx >= 1 && xx <= W;
        tile[i] = inside ? p[(yy - 1) * W + (xx - 1)] : 0.f;
    }
}

PP_HD double pml_pixel_loss(const float* tile, int P, int y, int x, float t, double sw, double ow, double gw) {
    const float* c = tile + (y + 1) * P + (x + 1);
    const double a = c[-P - 1], b = c[-P], d = c[-P + 1], e = c[-1], f = c[1], g = c[P - 1], h = c[P], j = c[P + 1];
    const double gx = (a - d) + 2.0 * (e - f) + (g - j);   // [[1, 0, -1], [2, 0, -2], [1, 0, -1]]
    const double gy = (a - g) + 2.0 * (b - h) + (d - j);   // [[1, 2, 1], [0, 0, 0], [-1, -2, -1]]
    const double pv = c[0], tv = t;
    const double diff = pv - tv;
    return sw * (gx * gx + gy * gy) + ow * (pv * (1.0 - tv)) + gw * (diff * diff);
}

// Thread tid of n: the sum of its pixels' loss and the best of its pixels of p (from the stage) and of t.
PP_HD PmlPartial pml_accumulate(const float* tile, const float* t, int H, int W, double sw, double ow, double gw, int tid, int n) {
    const int P = W + 2, HW = H * W;
    PmlPartial r{0.0, PmlBest{-INFINITY, 0x7fffffff}, PmlBest{-INFINITY, 0x7fffffff}};
    for (int i = tid; i < HW; i += n) {
        const int y = i / W, x = i - y * W;
        const float tv = t[i];
        r.sum += pml_pixel_loss(tile, P, y, x, tv, sw, ow, gw);
        const PmlBest bp{tile[(y + 1) * P + x + 1], i}, bt{tv, i};
        if (pml_better(bp, r.p)) r.p = bp;
        if (pml_better(bt, r.t)) r.t = bt;
    }
    return r;
}

// One step of the fixed tree over red[0 .. 2 stride): entry tid takes entry tid + stride in. Run for tid < stride, stride = n/2 .. 1,
// with a barrier between steps: the order of the additions does not depend on timing, so a repeat launch gives the same bits.
PP_HD void pml_reduce_step(PmlPartial* red, int tid, int stride) {
    PmlPartial a = red[tid];
    const PmlPartial b = red[tid + stride];
    a.sum += b.sum;
    if (pml_better(b.p, a.p)) a.p = b.p;
    if (pml_better(b.t, a.t)) a.t = b.t;
    red[tid] = a;
}

// The final reduction of the per-map sums (second launch, one workgroup): thread tid of n adds its maps in index order.
PP_HD double pml_sum_strided(const double* sums, long count, int tid, int n) {
    double s = 0.0;
    for (long i = tid; i < count; i += n) s += sums[i];
    return s;
}

// ---- scalar targets and losses (ProbMapHead.loss, probmap_head.py:830-941, on (B, K) values) --------------------------------------
// One workgroup. Phase A, thread tid of n over INSTANCES: gt_oks / oks_weight (_oks_from_heatmaps + compute_oks(use_area=False,
// per_kpt=True)), gt_errs (_error_from_heatmaps) from the decoded coordinates, and the counts of annotated invisible / visible
// keypoints. Phase B, over KEYPOINTS, after the counts are reduced: the visibility weights (:883-889) and the six sums. Elementwise
// values are fp64 from the float32 inputs; sums are fp64 through the fixed tree.
constexpr int PMS_SLOTS = 8;
enum { PMS_PROB = 0, PMS_VIS, PMS_OKS, PMS_ERR, PMS_MAE_OKS, PMS_MAE_ERR, PMS_N_IN, PMS_UNUSED };
enum { PMS_N_INVISIBLE = 0, PMS_N_VISIBLE = 1 };

struct PmsPartial {
    double v[PMS_SLOTS];
};

struct PmsArgs {
    const float* scalars;              // (4, B, K): predicted probability, visibility, oks, error
    const unsigned char* in_image;     // (B, K) 0 / 1
    const unsigned char* annotated;    // (B, K) 0 / 1: keypoints_visible.astype(int)
    const unsigned char* visibility;   // (B, K) 0 / 1: keypoints_visibility.astype(int)
    const double* kp_gt;               // (B, K, 2) decoded from the target maps
    const double* kp_dt;               // (B, K, 2) decoded from the predicted maps
    const double* vars;                // (K): (2 sigma_k)^2, compute_oks's sigmas (/ 10)
    double area;                       // compute_oks's tmparea + spacing(1)
    int B, K;
    int freeze_oks, freeze_error;
    int prob_logits, vis_logits;       // BCELoss(use_sigmoid=False): binary_cross_entropy_with_logits
    float* gt_oks;                     // (B, K) out
    float* oks_weight;                 // (B) out
    float* gt_errs;                    // (B, K) out
    float* vis_weights;                // (B, K) out
};

PP_HD void pms_reduce_step(PmsPartial* red, int tid, int stride) {
    for (int s = 0; s < PMS_SLOTS; ++s) red[tid].v[s] += red[tid + stride].v[s];
}

PP_HD PmsPartial pms_phase_a(const PmsArgs& a, int tid, int n) {
    PmsPartial r{};
    for (int b = tid; b < a.B; b += n) {
        const size_t row = (size_t)b * a.K;
        int valid = 0;
        for (int k = 0; k < a.K; ++k) {
            const size_t i = row + k;
            const bool w = a.in_image[i] && a.annotated[i];
            valid += w;
            if (a.annotated[i]) r.v[a.visibility[i] ? PMS_N_VISIBLE : PMS_N_INVISIBLE] += 1.0;
        }
        a.oks_weight[b] = (!a.freeze_oks && valid > 0) ? 1.f : 0.f;
        for (int k = 0; k < a.K; ++k) {
            const size_t i = row + k;
            const double w = (a.in_image[i] && a.annotated[i]) ? 1.0 : 0.0;
            double xg = a.kp_gt[2 * i], yg = a.kp_gt[2 * i + 1];
            const double xd = a.kp_dt[2 * i], yd = a.kp_dt[2 * i + 1];
            float oks = 0.f;
            if (!a.freeze_oks && valid > 0 && w > 0.0) {  // (a keypoint with weight 0 is set to 0 whatever its coordinates, :1121)
                const double xg0 = xg != xg ? 0.0 : xg, yg0 = yg != yg ? 0.0 : yg;  // NaN target coordinates -> 0 (:540)
                const double dx = xd * w - xg0 * w, dy = yd * w - yg0 * w;
                const double e = (dx * dx + dy * dy) / a.vars[k] / a.area / 2;
                oks = (float)exp(-e);
            }
            a.gt_oks[i] = oks;
            float err = 0.f;
            if (!a.freeze_error) {  // NaN target coordinates -> -1 (:502)
                const double ex = (xg != xg ? -1.0 : xg) - xd, ey = (yg != yg ? -1.0 : yg) - yd;
                err = (float)sqrt(ex * ex + ey * ey);
            }
            a.gt_errs[i] = err;
        }
    }
    return r;
}

// torch's binary_cross_entropy (log clamped at -100) / binary_cross_entropy_with_logits for one element
PP_HD double pms_bce(double p, double t, int logits) {
    if (logits) return (p > 0 ? p : 0.0) - p * t + log1p(exp(-fabs(p)));
    const double lp = log(p), lq = log(1.0 - p);
    return -(t * (lp < -100.0 ? -100.0 : lp) + (1.0 - t) * (lq < -100.0 ? -100.0 : lq));
}

// counts: the reduced result of phase A. The weights of :883-889: 1 / count of its class (formed in float32, as torch forms
// 1 / (int tensor + 1e-10)), divided in fp64 by the smallest positive weight.
PP_HD PmsPartial pms_phase_b(const PmsArgs& a, const PmsPartial& counts, int tid, int n) {
    PmsPartial r{};
    const double n_inv = counts.v[PMS_N_INVISIBLE], n_vis = counts.v[PMS_N_VISIBLE];
    const double w_inv = n_inv > 0 ? (double)(1.0f / (float)n_inv) : 0.0, w_vis = n_vis > 0 ? (double)(1.0f / (float)n_vis) : 0.0;
    const double w_min = w_inv > 0 && (w_vis <= 0 || w_inv < w_vis) ? w_inv : w_vis;  // 0: nothing annotated (the reference raises there)
    const size_t BK = (size_t)a.B * a.K;
    for (size_t i = tid; i < BK; i += n) {
        const double ann = a.annotated[i] ? 1.0 : 0.0, gt_prob = a.in_image[i] ? 1.0 : 0.0, gt_vis = a.visibility[i] ? 1.0 : 0.0;
        const double in = (a.annotated[i] && a.in_image[i]) ? 1.0 : 0.0;
        const float wv = a.annotated[i] ? (float)((gt_vis > 0 ? w_vis : w_inv) / w_min) : 0.f;
        a.vis_weights[i] = wv;
        const double dt_prob = a.scalars[i], dt_vis = a.scalars[BK + i], dt_oks = a.scalars[2 * BK + i], dt_err = a.scalars[3 * BK + i];
        const double gt_oks = a.gt_oks[i], gt_err = a.gt_errs[i];
        r.v[PMS_PROB] += pms_bce(dt_prob, gt_prob, a.prob_logits) * ann;
        r.v[PMS_VIS] += pms_bce(dt_vis, gt_vis, a.vis_logits) * (double)wv;
        const double d_oks = dt_oks * in - gt_oks * in;
        r.v[PMS_OKS] += d_oks * d_oks;
        const double d_err = fabs(log(1.0 + dt_err) * in - log(1.0 + gt_err) * in);
        r.v[PMS_ERR] += d_err < 1.0 ? 0.5 * d_err * d_err : d_err - 0.5;  // smooth_l1_loss, beta 1
        if (in > 0) {
            r.v[PMS_MAE_OKS] += fabs(dt_oks - gt_oks);
            r.v[PMS_MAE_ERR] += fabs(dt_err - gt_err);
            r.v[PMS_N_IN] += 1.0;
        }
    }
    return r;
}

// out[0 .. 6): loss_probability, loss_visibility, loss_oks, loss_error (means over B K, times their loss weights), mae_oks, mae_err
// (means over the annotated keypoints inside the image; NaN when there is none, as numpy's mean of nothing)
PP_HD void pms_finish(const PmsPartial& sums, const double* loss_weights, double BK, float* out) {
    for (int s = 0; s < 4; ++s) out[s] = (float)(sums.v[s] / BK * loss_weights[s]);
    const double n = sums.v[PMS_N_IN];
    out[4] = n > 0 ? (float)(sums.v[PMS_MAE_OKS] / n) : NAN;
    out[5] = n > 0 ? (float)(sums.v[PMS_MAE_ERR] / n) : NAN;
}

}  // namespace pp
