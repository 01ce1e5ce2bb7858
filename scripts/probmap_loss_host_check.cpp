// Sequential host form of the ProbMap target generator and of the OKS map loss: the phase bodies of pp_probmap_loss_core.h, run for
// thread 0 .. 255 in turn on heap buffers of exactly the size the kernels are given, so that the host sanitizers see every index the
// device code forms. Host only - no HIP, nothing here is loaded into Python:
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I probpose_code_amd/csrc \
//       scripts/probmap_loss_host_check.cpp -o /tmp/probmap_loss_host_check && /tmp/probmap_loss_host_check
// Besides running clean it checks the phases against a plain restatement that tests every tap's bounds instead of staging a halo.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pp_probmap_loss_core.h"

using namespace pp;

static unsigned g_rng = 12345u;
static float uniform01() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (float)(g_rng >> 8) / 16777216.0f;
}

static int g_failures = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            std::printf("FAIL %s: ", #cond);     \
            std::printf(__VA_ARGS__);            \
            std::printf("\n");                   \
            ++g_failures;                        \
        }                                        \
    } while (0)

// p[y][x] or 0 outside: zero "same" padding
static double at(const std::vector<float>& p, int H, int W, int y, int x) {
    return (y < 0 || y >= H || x < 0 || x >= W) ? 0.0 : (double)p[(size_t)y * W + x];
}

static double plain_map_sum(const std::vector<float>& p, const std::vector<float>& t, int H, int W, double sw, double ow, double gw) {
    double s = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const double gx = at(p, H, W, y - 1, x - 1) - at(p, H, W, y - 1, x + 1) + 2 * at(p, H, W, y, x - 1) - 2 * at(p, H, W, y, x + 1) +
                              at(p, H, W, y + 1, x - 1) - at(p, H, W, y + 1, x + 1);
            const double gy = at(p, H, W, y - 1, x - 1) + 2 * at(p, H, W, y - 1, x) + at(p, H, W, y - 1, x + 1) - at(p, H, W, y + 1, x - 1) -
                              2 * at(p, H, W, y + 1, x) - at(p, H, W, y + 1, x + 1);
            const double pv = at(p, H, W, y, x), tv = t[(size_t)y * W + x];
            s += sw * (gx * gx + gy * gy) + ow * pv * (1 - tv) + gw * (pv - tv) * (pv - tv);
        }
    return s;
}

static int plain_argmax(const std::vector<float>& v) {
    int best = 0;
    for (size_t i = 1; i < v.size(); ++i)
        if (v[i] > v[best]) best = (int)i;
    return best;
}

static PmlPartial run_loss_map(const std::vector<float>& p, const std::vector<float>& t, int H, int W, double sw, double ow, double gw) {
    std::vector<float> tile((size_t)(H + 2) * (W + 2), -7.f);  // exactly the LDS stage; every entry must be overwritten
    for (int tid = 0; tid < PML_THREADS; ++tid) pml_stage(tile.data(), p.data(), H, W, tid, PML_THREADS);
    for (float v : tile) CHECK(v != -7.f, "stage entry not written (%dx%d)", H, W);
    std::vector<PmlPartial> red(PML_THREADS);
    for (int tid = 0; tid < PML_THREADS; ++tid) red[tid] = pml_accumulate(tile.data(), t.data(), H, W, sw, ow, gw, tid, PML_THREADS);
    for (int stride = PML_THREADS / 2; stride >= 1; stride >>= 1)
        for (int tid = 0; tid < stride; ++tid) pml_reduce_step(red.data(), tid, stride);
    return red[0];
}

static void check_loss(int H, int W, int variant) {
    const size_t HW = (size_t)H * W;
    std::vector<float> p(HW), t(HW);
    for (size_t i = 0; i < HW; ++i) {
        p[i] = variant == 1 ? 0.f : uniform01();
        t[i] = uniform01();
    }
    if (variant == 2) {  // ties: the maximum twice, the first must win
        p[HW - 1] = 2.f;
        p[HW / 2] = 2.f;
        t[0] = 3.f;
        t[HW - 1] = 3.f;
    }
    const double sw = 0.05, gw = 0.1, ow = 1 - sw - gw;
    const PmlPartial r = run_loss_map(p, t, H, W, sw, ow, gw);
    const double want = plain_map_sum(p, t, H, W, sw, ow, gw);
    CHECK(std::fabs(r.sum - want) <= 1e-12 * (1 + std::fabs(want)), "%dx%d variant %d: sum %.17g, plain %.17g", H, W, variant, r.sum, want);
    CHECK(r.p.i == plain_argmax(p), "%dx%d variant %d: argmax p %d, plain %d", H, W, variant, r.p.i, plain_argmax(p));
    CHECK(r.t.i == plain_argmax(t), "%dx%d variant %d: argmax t %d, plain %d", H, W, variant, r.t.i, plain_argmax(t));
    CHECK(r.p.v == p[r.p.i] && r.t.v == t[r.t.i], "%dx%d variant %d: maximum is not the value at its index", H, W, variant);
}

static void check_encode(int H, int W) {
    const size_t HW = (size_t)H * W;
    const double kxs[] = {0.0, W - 1.0, W * 0.37, -3.5, W + 40.0, 1e4};
    for (int k = 0; k < PML_COCO_K; k += 8)
        for (double kx : kxs) {
            const double ky = H * 0.61, two_s = 2 * pml_keypoint_s(k, H, W, -1);
            std::vector<float> map(HW, -7.f);
            bool any = false;
            for (int tid = 0; tid < PML_THREADS; ++tid) any = pml_encode_map(map.data(), H, W, kx, ky, two_s, tid, PML_THREADS) || any;
            bool want_any = false;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const double d = std::sqrt((x - kx) * (x - kx) + (y - ky) * (y - ky));
                    const double v = std::exp(-(d * d) / two_s);
                    want_any = want_any || v > 0;
                    CHECK(map[(size_t)y * W + x] == (float)v, "encode %dx%d k %d kx %g: pixel (%d, %d)", H, W, k, kx, y, x);
                }
            CHECK(any == want_any, "encode %dx%d k %d kx %g: weight", H, W, k, kx);
            if (kx == 1e4) CHECK(!any, "a keypoint 1e4 pixels away must underflow in fp64");
            for (int tid = 0; tid < PML_THREADS; ++tid) pml_zero_map(map.data(), (int)HW, tid, PML_THREADS);
            for (float v : map) CHECK(v == 0.f, "zero map");
        }
}

// The scalar phases on exactly-sized buffers, against a plain restatement of the two quantities that need counts of the whole batch.
static void check_scalars(int B, int variant) {
    const int K = PML_COCO_K;
    const size_t BK = (size_t)B * K;
    std::vector<float> scalars(4 * BK), gt_oks(BK, -7.f), oks_weight((size_t)B, -7.f), gt_errs(BK, -7.f), vis_weights(BK, -7.f);
    std::vector<unsigned char> in_image(BK), annotated(BK), visibility(BK);
    std::vector<double> kp_gt(2 * BK), kp_dt(2 * BK), vars((size_t)K);
    for (int k = 0; k < K; ++k) vars[(size_t)k] = 0.01 * (k + 1);
    for (size_t i = 0; i < 4 * BK; ++i) scalars[i] = 0.01f + 0.98f * uniform01();
    for (size_t i = 0; i < BK; ++i) {
        in_image[i] = variant == 1 ? 0 : uniform01() < 0.7f;
        annotated[i] = variant == 2 ? 0 : uniform01() < 0.8f;
        visibility[i] = uniform01() < 0.5f;
    }
    for (size_t i = 0; i < 2 * BK; ++i) {
        kp_gt[i] = 200.0 * uniform01();
        kp_dt[i] = kp_gt[i] + uniform01() - 0.5;
    }
    kp_gt[0] = NAN;
    PmsArgs a{};
    a.scalars = scalars.data(), a.in_image = in_image.data(), a.annotated = annotated.data(), a.visibility = visibility.data();
    a.kp_gt = kp_gt.data(), a.kp_dt = kp_dt.data(), a.vars = vars.data(), a.area = 1628.16, a.B = B, a.K = K;
    a.freeze_error = variant == 0, a.prob_logits = variant == 1;
    a.gt_oks = gt_oks.data(), a.oks_weight = oks_weight.data(), a.gt_errs = gt_errs.data(), a.vis_weights = vis_weights.data();
    std::vector<PmsPartial> red(PML_THREADS);
    auto reduce = [&] {
        for (int stride = PML_THREADS / 2; stride >= 1; stride >>= 1)
            for (int tid = 0; tid < stride; ++tid) pms_reduce_step(red.data(), tid, stride);
    };
    for (int tid = 0; tid < PML_THREADS; ++tid) red[tid] = pms_phase_a(a, tid, PML_THREADS);
    reduce();
    const PmsPartial counts = red[0];
    for (int tid = 0; tid < PML_THREADS; ++tid) red[tid] = pms_phase_b(a, counts, tid, PML_THREADS);
    reduce();
    const double lw[4] = {1, 1, 1, 1};
    float out[6];
    pms_finish(red[0], lw, (double)BK, out);
    for (size_t i = 0; i < BK; ++i) CHECK(gt_oks[i] != -7.f && gt_errs[i] != -7.f && vis_weights[i] != -7.f, "scalars B %d: output %zu not written", B, i);
    long n_inv = 0, n_vis = 0, n_in = 0;
    for (size_t i = 0; i < BK; ++i) {
        n_inv += annotated[i] && !visibility[i];
        n_vis += annotated[i] && visibility[i];
        n_in += annotated[i] && in_image[i];
    }
    CHECK(counts.v[PMS_N_INVISIBLE] == n_inv && counts.v[PMS_N_VISIBLE] == n_vis, "scalars B %d variant %d: class counts", B, variant);
    CHECK(red[0].v[PMS_N_IN] == n_in, "scalars B %d variant %d: count of annotated keypoints inside", B, variant);
    for (int b = 0; b < B; ++b) {
        bool any = false;
        for (int k = 0; k < K; ++k) any = any || (annotated[(size_t)b * K + k] && in_image[(size_t)b * K + k]);
        CHECK(oks_weight[(size_t)b] == (any ? 1.f : 0.f), "scalars B %d variant %d: oks_weight of instance %d", B, variant, b);
    }
    double least = 1e300;
    for (size_t i = 0; i < BK; ++i)
        if (vis_weights[i] > 0) least = vis_weights[i] < least ? vis_weights[i] : least;
    CHECK(n_inv + n_vis == 0 || least == 1.0, "scalars B %d variant %d: the smallest positive visibility weight is 1", B, variant);
    CHECK((n_in == 0) == (out[4] != out[4]), "scalars B %d variant %d: mae is NaN exactly without keypoints", B, variant);
    for (int s = 0; s < 4; ++s) CHECK(out[s] == out[s] && out[s] >= 0, "scalars B %d variant %d: loss %d is %g (a NaN target coordinate must not reach it)", B, variant, s, out[s]);
}

int main() {
    for (int B : {1, 3, 15, 16, 17, 300})
        for (int variant = 0; variant < 3; ++variant) check_scalars(B, variant);
    const int sizes[][2] = {{1, 1}, {2, 2}, {3, 5}, {64, 48}, {5, 3}, {17, 1}, {1, 300}};
    for (const auto& hw : sizes) {
        for (int variant = 0; variant < 3; ++variant) check_loss(hw[0], hw[1], variant);
        check_encode(hw[0], hw[1]);
    }
    // the final reduction of the per-map sums: every count around the workgroup size
    for (long count : {1L, 17L, 51L, 255L, 256L, 257L, 1088L}) {
        std::vector<double> sums((size_t)count);
        double want = 0;
        for (long i = 0; i < count; ++i) want += (sums[(size_t)i] = uniform01());
        std::vector<PmlPartial> red(PML_THREADS);
        for (int tid = 0; tid < PML_THREADS; ++tid)
            red[tid] = PmlPartial{pml_sum_strided(sums.data(), count, tid, PML_THREADS), PmlBest{0.f, 0}, PmlBest{0.f, 0}};
        for (int stride = PML_THREADS / 2; stride >= 1; stride >>= 1)
            for (int tid = 0; tid < stride; ++tid) pml_reduce_step(red.data(), tid, stride);
        CHECK(std::fabs(red[0].sum - want) <= 1e-12 * want, "mean over %ld maps", count);
    }
    CHECK(pml_in_image(0.f, 0.f, 192.f, 256.f) && !pml_in_image(192.f, 0.f, 192.f, 256.f) && !pml_in_image(-0.5f, 3.f, 192.f, 256.f) &&
              !pml_in_image(NAN, 3.f, 192.f, 256.f) && !pml_in_image(3.f, 256.f, 192.f, 256.f), "in_image comparisons");
    if (g_failures) {
        std::printf("%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("probmap loss host check: OK\n");
    return 0;
}
