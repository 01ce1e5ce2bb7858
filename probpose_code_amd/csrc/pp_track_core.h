// Per-track bodies of the pose tracker (pp_track.hip), shared with a sequential host form (scripts/track_host_check.cpp runs every
// phase for track 0 .. n-1 in turn, under the host sanitizers). The rule - the next frame's person boxes from this frame's poses:
//
//   update   keypoints to image space with the expression of TopdownPoseEstimator.add_pred_to_datasample (topdown.py:165-167),
//            x / size * scale + centre - 0.5 * scale, float64 from the float32 centres and scales (0.5 * scale is a float32 product, as
//            numpy forms it). A keypoint is selected when its gate (the presence probability of a head with towers, the confidence of a
//            HeatmapHead) is finite and >= kpt_thr and both coordinates are finite. With at least min_keypoints selected the new box
//            is their min/max box grown about its centre by `expand`, each side at least `min_side`, blended with the old box by
//            `smooth` and rounded to float32; lost <- 0. Otherwise the box stays, lost <- lost + 1, and beyond max_lost the track dies.
//   pairs    OKS (mmpose/evaluation/functional/nms.py:58-116: exp(-d^2 / (2 sigma)^2 / ((a_i + a_j) / 2 + eps) / 2), mean over K) of the
//            image-space poses of every two tracks updated in this frame, the areas those of their new float32 boxes.
//   resolve  the pairs above dup_oks_thr in the order (0,1) (0,2) .. (1,2) ..: of two tracks still alive the one with the lower mean
//            gate over its selected keypoints dies, the higher index on a tie.
//   affine   transforms.topdown_affine_params (bbox_xyxy2cs with input_padding, fix_aspect_ratio, get_udp_warp_matrix at rot = 0 in
//            float32 as numpy promotes it) and transforms.invert_affine (float64) of every slot's box: one rounding per operator.
//
// Sums over K go through one fixed tree (adjacent pairs of the keypoints padded with zeros to a power of two), contraction is off:
// the same bits on the host and on the device, launch after launch - up to exp(), which the two libraries may round differently in
// the last place (an OKS within a few ulp of dup_oks_thr could be decided either way; boxes and lost counts never depend on it).
#pragma once
#include <cmath>
#include <cstdint>

#ifndef PP_HD
#if defined(__HIPCC__)
#define PP_HD __host__ __device__ __forceinline__
#else
#define PP_HD inline
#endif
#endif

namespace pp {

constexpr int TRK_MAX_TRACKS = 64;  // one wave, one dup mask word per track
constexpr int TRK_MAX_K = 256;
constexpr int TRK_TREE_LEVELS = 9;  // log2(TRK_MAX_K) + 1
constexpr int TRK_RECORD = 7;       // x, y, conf, prob, vis, oks, err (pp_pack_records)

struct TrkArgs {
    // this frame: records (n, K, 7) float64 in crop space, the centres and scales (n, 2) float32 its crops were cut with
    const double* records;
    const float* centers;
    const float* scales;
    const double* sigmas;  // (K)
    int n, K;
    double in_w, in_h;
    int gate_col;  // 3: prob, 2: conf
    double kpt_thr, expand, min_side, smooth, dup_oks_thr;
    int min_keypoints, max_lost;
    // track state: boxes (n, 4) float32 xyxy, alive and lost (n) int32; the outputs may be the inputs
    const float* boxes_in;
    const int32_t* alive_in;
    const int32_t* lost_in;
    float* boxes_out;
    int32_t* alive_out;
    int32_t* lost_out;
    // affine phase (all three NULL: skipped): centres and scales (n, 2) float32, dst -> src maps (n, 2, 3) float64 of boxes_out
    float pad, aspect, out_w1, out_h1;  // input_padding, w / h, w - 1, h - 1 as float32
    float* next_centers;
    float* next_scales;
    double* next_maps;
};

struct TrkTrack {   // what the update of a track leaves for the duplicate phases
    int updated;    // selected >= min_keypoints in this frame (and alive)
    double mean_gate, area;
};

// Sum of leaf(0 .. K-1) through the tree of adjacent pairs over the leaves padded with 0.0 to a power of two.
template <class Leaf>
PP_HD double trk_tree_sum(int K, Leaf leaf) {
#pragma clang fp contract(off)
    int P = 1, levels = 0;
    while (P < K) P <<= 1, ++levels;
    double st[TRK_TREE_LEVELS];
    for (int l = 0; l < TRK_TREE_LEVELS; ++l) st[l] = 0.0;
    for (int i = 0; i < P; ++i) {
        double acc = i < K ? leaf(i) : 0.0;
        int level = 0;
        for (int j = i; j & 1; j >>= 1, ++level) acc = st[level] + acc;
        st[level] = acc;
    }
    return st[levels];
}

PP_HD bool trk_finite(double v) { return v - v == 0.0; }

// topdown.py:165-167 for keypoint k of track i
PP_HD void trk_image_point(const TrkArgs& a, int i, int k, double& x, double& y) {
#pragma clang fp contract(off)
    const double* r = a.records + ((size_t)i * a.K + k) * TRK_RECORD;
    const float sx = a.scales[2 * i], sy = a.scales[2 * i + 1];
    x = r[0] / a.in_w * (double)sx + (double)a.centers[2 * i] - (double)(0.5f * sx);
    y = r[1] / a.in_h * (double)sy + (double)a.centers[2 * i + 1] - (double)(0.5f * sy);
}

PP_HD bool trk_selected(const TrkArgs& a, int i, int k, double x, double y) {
    const double g = a.records[((size_t)i * a.K + k) * TRK_RECORD + a.gate_col];
    return trk_finite(g) && g >= a.kpt_thr && trk_finite(x) && trk_finite(y);
}

// phase "update" of track i
PP_HD void trk_update(const TrkArgs& a, int i, TrkTrack& t) {
#pragma clang fp contract(off)
    float box[4] = {a.boxes_in[4 * i], a.boxes_in[4 * i + 1], a.boxes_in[4 * i + 2], a.boxes_in[4 * i + 3]};
    int alive = a.alive_in[i] != 0, lost = a.lost_in[i];
    t.updated = 0, t.mean_gate = 0.0, t.area = 0.0;
    if (alive) {
        int count = 0;
        double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
        for (int k = 0; k < a.K; ++k) {
            double x, y;
            trk_image_point(a, i, k, x, y);
            if (!trk_selected(a, i, k, x, y)) continue;
            ++count;
            x0 = x < x0 ? x : x0, x1 = x > x1 ? x : x1;
            y0 = y < y0 ? y : y0, y1 = y > y1 ? y : y1;
        }
        if (count >= a.min_keypoints) {
            const double cx = (x0 + x1) * 0.5, cy = (y0 + y1) * 0.5;
            double w = (x1 - x0) * a.expand, h = (y1 - y0) * a.expand;
            w = w > a.min_side ? w : a.min_side;
            h = h > a.min_side ? h : a.min_side;
            double nb[4] = {cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h};
            if (a.smooth != 0.0)
                for (int c = 0; c < 4; ++c) nb[c] = a.smooth * (double)box[c] + (1.0 - a.smooth) * nb[c];
            for (int c = 0; c < 4; ++c) box[c] = (float)nb[c];
            lost = 0;
            const double gates = trk_tree_sum(a.K, [&](int k) {
                double x, y;
                trk_image_point(a, i, k, x, y);
                return trk_selected(a, i, k, x, y) ? a.records[((size_t)i * a.K + k) * TRK_RECORD + a.gate_col] : 0.0;
            });
            t.updated = 1;
            t.mean_gate = gates / (double)count;
            t.area = ((double)box[2] - (double)box[0]) * ((double)box[3] - (double)box[1]);
        } else {
            lost = lost < INT32_MAX ? lost + 1 : lost;
            if (lost > a.max_lost) alive = 0;
        }
    }
    for (int c = 0; c < 4; ++c) a.boxes_out[4 * i + c] = box[c];
    a.alive_out[i] = alive;
    a.lost_out[i] = lost;
}

// nms.py:58-116 for the poses of tracks i and j
PP_HD double trk_pair_oks(const TrkArgs& a, int i, int j, double area_i, double area_j) {
#pragma clang fp contract(off)
    const double scale = (area_i + area_j) / 2 + 2.220446049250313e-16;  // + np.spacing(1)
    const double sum = trk_tree_sum(a.K, [&](int k) {
        double xi, yi, xj, yj;
        trk_image_point(a, i, k, xi, yi);
        trk_image_point(a, j, k, xj, yj);
        const double two_sigma = a.sigmas[k] * 2;
        const double dx = xj - xi, dy = yj - yi;
        const double e = (dx * dx + dy * dy) / (two_sigma * two_sigma) / scale / 2;
        return exp(-e);
    });
    return sum / (double)a.K;
}

// phase "pairs" of track i: bit j (j > i) of the result = the two tracks were updated and their OKS is above the threshold
PP_HD uint64_t trk_pairs(const TrkArgs& a, int i, const TrkTrack* tr) {
    uint64_t mask = 0;
    if (!tr[i].updated) return 0;
    for (int j = i + 1; j < a.n; ++j)
        if (tr[j].updated && trk_pair_oks(a, i, j, tr[i].area, tr[j].area) > a.dup_oks_thr) mask |= (uint64_t)1 << j;
    return mask;
}

// phase "resolve": sequential, one caller
PP_HD void trk_resolve(const TrkArgs& a, const TrkTrack* tr, const uint64_t* dup, uint64_t& dead) {
    dead = 0;
    for (int i = 0; i < a.n; ++i)
        for (int j = i + 1; j < a.n; ++j) {
            if (!((dup[i] >> j) & 1) || ((dead >> i) & 1) || ((dead >> j) & 1)) continue;
            const int loser = tr[i].mean_gate < tr[j].mean_gate ? i : j;
            dead |= (uint64_t)1 << loser;
            a.alive_out[loser] = 0;
        }
}

// phase "affine" of slot i: topdown_affine_params + invert_affine of box (4 floats)
PP_HD void trk_affine(const float* box, float pad, float aspect, float out_w1, float out_h1, float* center, float* scale, double* map) {
#pragma clang fp contract(off)
    const float bw = (box[2] - box[0]) * pad, bh = (box[3] - box[1]) * pad;  // bbox_xyxy2cs
    const float cx = (box[2] + box[0]) * 0.5f, cy = (box[3] + box[1]) * 0.5f;
    const float ha = bh * aspect;                                            // fix_aspect_ratio
    float w, h;
    if (bw > ha)
        w = bw, h = bw / aspect;
    else
        w = ha, h = bh;
    center[0] = cx, center[1] = cy, scale[0] = w, scale[1] = h;
    // get_udp_warp_matrix, rot = 0: c = 1.0, s = 0.0 (the products with them are kept: signed zeros, inf * 0)
    const float c = 1.0f, s = 0.0f;
    const float isx = cx * 2, isy = cy * 2;
    const float sx = out_w1 / w, sy = out_h1 / h;
    const float m00 = c * sx;
    const float m01 = -s * sx;
    const float m02 = sx * (-0.5f * isx * c + 0.5f * isy * s + 0.5f * w);
    const float m10 = s * sy;
    const float m11 = c * sy;
    const float m12 = sy * (-0.5f * isx * s - 0.5f * isy * c + 0.5f * h);
    // invert_affine
    double M00 = m00, M01 = m01, M02 = m02, M10 = m10, M11 = m11, M12 = m12;
    double D = M00 * M11 - M01 * M10;
    D = D != 0 ? 1.0 / D : 0.0;
    const double A11 = M11 * D, A22 = M00 * D;
    M00 = A11;
    M01 = M01 * -D;
    M10 = M10 * -D;
    M11 = A22;
    const double b1 = -M00 * M02 - M01 * M12;
    const double b2 = -M10 * M02 - M11 * M12;
    map[0] = M00, map[1] = M01, map[2] = b1, map[3] = M10, map[4] = M11, map[5] = b2;
}

// Why a parameter set is refused, or nullptr (shared by the entry points and the host form).
inline const char* trk_check_params(double kpt_thr, int min_keypoints, double expand, double min_side, double smooth, int max_lost,
                                    double dup_oks_thr) {
    if (kpt_thr != kpt_thr) return "kpt_thr must not be NaN";
    if (min_keypoints < 1) return "min_keypoints must be at least 1";
    if (!(expand > 0.0) || !trk_finite(expand)) return "expand must be positive and finite";
    if (!(min_side > 0.0) || !trk_finite(min_side)) return "min_side must be positive and finite";
    if (!(smooth >= 0.0 && smooth < 1.0)) return "smooth must be in [0, 1)";
    if (max_lost < 0) return "max_lost must not be negative";
    if (dup_oks_thr != dup_oks_thr) return "dup_oks_thr must not be NaN";
    return nullptr;
}

}  // namespace pp
