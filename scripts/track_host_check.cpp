// Sequential host form of the pose tracker's box rule: the phase bodies of pp_track_core.h, run for track 0 .. n-1 in turn on heap
// buffers of exactly the size the kernel is given, so that the host sanitizers see every index the device code forms. Host only - no
// HIP, nothing here is loaded into Python:
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I probpose_code_amd/csrc \
//       scripts/track_host_check.cpp -o /tmp/track_host_check && /tmp/track_host_check
// Besides running clean it checks properties of the rule on crafted and random cases: a translating pose is followed, the lost count
// and death, a dead track stays dead, min_side on collinear keypoints, non-finite inputs never reach a box, the duplicate decision and
// its tie, in-place update equals out-of-place, the crop maps send the crop's corners onto the padded box.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "pp_track_core.h"

using namespace pp;

static unsigned g_rng = 2463534242u;
static double uniform01() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (double)(g_rng >> 8) / 16777216.0;
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

static const double COCO[17] = {.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089};

struct Case {
    int n, K;
    std::vector<double> records, sigmas, maps;
    std::vector<float> centers, scales, boxes, next_centers, next_scales;
    std::vector<int32_t> alive, lost;
    TrkArgs a{};

    Case(int n_, int K_) : n(n_), K(K_), records((size_t)n_ * K_ * TRK_RECORD, 0.0), sigmas(K_), maps((size_t)n_ * 6), centers(2 * n_),
                           scales(2 * n_), boxes(4 * n_), next_centers(2 * n_), next_scales(2 * n_), alive(n_, 1), lost(n_, 0) {
        for (int k = 0; k < K; ++k) sigmas[k] = COCO[k % 17];
        a.n = n, a.K = K, a.in_w = 192, a.in_h = 256, a.gate_col = 3;
        a.kpt_thr = 0.3, a.expand = 1.25, a.min_side = 8, a.smooth = 0, a.dup_oks_thr = 0.9, a.min_keypoints = 4, a.max_lost = 10;
        a.pad = 1.25f, a.aspect = 0.75f, a.out_w1 = 191.f, a.out_h1 = 255.f;
        bind();
    }
    void bind() {  // (vectors never reallocate after construction; out = in: the in-place form the loop uses)
        a.records = records.data(), a.centers = centers.data(), a.scales = scales.data(), a.sigmas = sigmas.data();
        a.boxes_in = boxes.data(), a.alive_in = alive.data(), a.lost_in = lost.data();
        a.boxes_out = boxes.data(), a.alive_out = alive.data(), a.lost_out = lost.data();
        a.next_centers = next_centers.data(), a.next_scales = next_scales.data(), a.next_maps = maps.data();
    }
    void set_box(int i, float x0, float y0, float x1, float y1) {
        float b[4] = {x0, y0, x1, y1};
        std::memcpy(&boxes[4 * i], b, sizeof b);
        trk_affine(&boxes[4 * i], a.pad, a.aspect, a.out_w1, a.out_h1, &centers[2 * i], &scales[2 * i], &maps[6 * i]);
    }
    // keypoint k of track i at image point (x, y): the inverse of the image-space map, so the rule sees (x, y) up to rounding
    void put(int i, int k, double x, double y, double gate) {
        double* r = &records[((size_t)i * K + k) * TRK_RECORD];
        r[0] = (x - centers[2 * i] + 0.5 * scales[2 * i]) / scales[2 * i] * a.in_w;
        r[1] = (y - centers[2 * i + 1] + 0.5 * scales[2 * i + 1]) / scales[2 * i + 1] * a.in_h;
        r[2] = r[3] = gate;
    }
    // the sequential form of the kernel; crops of the next frame are cut with the new parameters
    void step() {
        std::vector<TrkTrack> tr(n);
        std::vector<uint64_t> dup(n);
        for (int i = 0; i < n; ++i) trk_update(a, i, tr[i]);
        for (int i = 0; i < n; ++i) dup[i] = trk_pairs(a, i, tr.data());
        uint64_t dead;
        trk_resolve(a, tr.data(), dup.data(), dead);
        for (int i = 0; i < n; ++i)
            trk_affine(a.boxes_out + 4 * i, a.pad, a.aspect, a.out_w1, a.out_h1, a.next_centers + 2 * i, a.next_scales + 2 * i, a.next_maps + 6 * i);
        centers = next_centers, scales = next_scales;
        bind();
    }
};

static void pose(Case& c, int i, double ox, double oy, double gate, int count = -1) {
    for (int k = 0; k < c.K; ++k)
        c.put(i, k, ox + 7.0 * (k % 5), oy + 11.0 * (k / 5), (count < 0 || k < count) ? gate : 0.0);
}

static void crafted() {
    {  // a pose translating 3 px per frame: the box follows, lost stays 0
        Case c(1, 17);
        c.set_box(0, 40, 30, 90, 100);
        for (int f = 0; f < 6; ++f) {
            pose(c, 0, 50 + 3 * f, 40, 0.9);
            c.step();
            const double cx = 0.5 * (c.boxes[0] + c.boxes[2]);
            CHECK(std::fabs(cx - (50 + 3 * f + 14)) < 1e-3 && c.alive[0] == 1 && c.lost[0] == 0, "frame %d: centre %f", f, cx);
            CHECK(std::fabs((c.boxes[2] - c.boxes[0]) - 28 * 1.25) < 1e-3 && std::fabs((c.boxes[3] - c.boxes[1]) - 33 * 1.25) < 1e-3, "size");
        }
    }
    {  // exactly min_keypoints / one fewer; lost counting, death at max_lost + 1, dead stays dead
        Case c(2, 17);
        c.a.max_lost = 2;
        c.set_box(0, 10, 10, 60, 80), c.set_box(1, 100, 10, 160, 90);
        pose(c, 0, 20, 20, 0.9, 4), pose(c, 1, 110, 20, 0.9, 3);
        const std::vector<float> before = c.boxes;
        c.step();
        CHECK(c.lost[0] == 0 && c.lost[1] == 1 && c.alive[1] == 1, "lost %d %d", c.lost[0], c.lost[1]);
        CHECK(std::memcmp(&before[4], &c.boxes[4], 16) == 0 && std::memcmp(&before[0], &c.boxes[0], 16) != 0, "kept / moved");
        for (int f = 2; f <= 3; ++f) {
            pose(c, 1, 110, 20, 0.9, 3);
            c.step();
            CHECK(c.lost[1] == f && c.alive[1] == (f <= 2), "frame %d: lost %d alive %d", f, c.lost[1], c.alive[1]);
        }
        pose(c, 1, 110, 20, 0.9);  // a perfect pose does not revive it
        c.step();
        CHECK(c.alive[1] == 0 && c.lost[1] == 3 && std::memcmp(&before[4], &c.boxes[4], 16) == 0, "dead stays dead");
    }
    {  // collinear keypoints: min_side; NaN / inf coordinates and gates are never selected
        Case c(1, 17);
        c.set_box(0, 0, 0, 100, 100);
        for (int k = 0; k < 17; ++k) c.put(0, k, 50, 10 + 2 * k, 0.8);
        const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
        c.records[0 * TRK_RECORD + 0] = nan, c.records[1 * TRK_RECORD + 1] = inf, c.records[2 * TRK_RECORD + 3] = nan;
        c.records[3 * TRK_RECORD + 3] = inf, c.records[4 * TRK_RECORD + 0] = -inf;
        c.step();
        CHECK(std::fabs((c.boxes[2] - c.boxes[0]) - 8) < 1e-4, "width %f", c.boxes[2] - c.boxes[0]);
        CHECK(std::fabs(c.boxes[1] - (10 + 2 * 5 + 22 * 0.5 - 22 * 1.25 * 0.5)) < 1e-3, "top %f (keypoints 5 .. 16 selected)", c.boxes[1]);
        for (int q = 0; q < 4; ++q) CHECK(std::isfinite(c.boxes[q]), "box[%d]", q);
        for (int q = 0; q < 6; ++q) CHECK(std::isfinite(c.maps[q]), "map[%d]", q);
    }
    {  // smooth
        Case c(1, 17);
        c.a.smooth = 0.5;
        c.set_box(0, 40, 30, 90, 100);
        pose(c, 0, 50, 40, 0.9);
        c.step();
        CHECK(std::fabs(c.boxes[0] - 0.5 * (40 + (64 - 17.5))) < 1e-3, "x0 %f", c.boxes[0]);
    }
    {  // two tracks on one pose: the lower mean gate dies, the higher index on a tie; a third elsewhere is untouched
        for (int variant = 0; variant < 3; ++variant) {
            Case c(3, 17);
            c.set_box(0, 40, 30, 90, 100), c.set_box(1, 38, 28, 92, 102), c.set_box(2, 200, 30, 260, 100);
            pose(c, 0, 50, 40, variant == 1 ? 0.6 : 0.9), pose(c, 1, 50, 40, variant == 2 ? 0.6 : 0.9), pose(c, 2, 210, 40, 0.5);
            c.step();
            const int want0 = variant != 1, want1 = variant == 1;
            CHECK(c.alive[0] == want0 && c.alive[1] == want1 && c.alive[2] == 1, "variant %d: alive %d %d %d", variant, c.alive[0], c.alive[1], c.alive[2]);
        }
    }
}

static void random_cases() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const int shapes[][2] = {{1, 17}, {2, 17}, {5, 17}, {64, 17}, {64, 1}, {3, 1}, {7, 256}, {9, 33}};
    for (const auto& sh : shapes)
        for (int rep = 0; rep < 40; ++rep) {
            Case c(sh[0], sh[1]);
            c.a.min_keypoints = 1 + (int)(uniform01() * (sh[1] < 6 ? sh[1] : 6));
            c.a.max_lost = (int)(uniform01() * 3);
            c.a.smooth = rep % 3 ? 0.0 : uniform01() * 0.9;
            c.a.gate_col = rep % 2 ? 3 : 2;
            c.a.dup_oks_thr = 0.5;
            for (int i = 0; i < c.n; ++i) {
                const float x0 = (float)(uniform01() * 600 - 100), y0 = (float)(uniform01() * 400 - 100);
                c.set_box(i, x0, y0, x0 + 1 + (float)(uniform01() * 300), y0 + 1 + (float)(uniform01() * 300));
                c.alive[i] = uniform01() < 0.85, c.lost[i] = (int)(uniform01() * 3);
            }
            for (int f = 0; f < 3; ++f) {
                for (size_t q = 0; q < c.records.size(); ++q) {
                    const double u = uniform01();
                    c.records[q] = u < 0.01 ? nan : u < 0.02 ? inf : u < 0.03 ? -inf : uniform01() * 300 - 30;
                    if (q % TRK_RECORD == 2 || q % TRK_RECORD == 3) c.records[q] = u < 0.03 ? c.records[q] : uniform01();
                }
                if (c.n > 1 && rep % 4 == 0)  // a copy of track 0's records and crop in slot 1: a duplicate when both are updated
                    for (int k = 0; k < c.K * TRK_RECORD; ++k) c.records[c.K * TRK_RECORD + k] = c.records[k];
                if (c.n > 1 && rep % 4 == 0)
                    c.set_box(1, c.boxes[0], c.boxes[1], c.boxes[2], c.boxes[3]), c.alive[1] = c.alive[0];
                const std::vector<int32_t> alive0 = c.alive, lost0 = c.lost;
                const std::vector<float> boxes0 = c.boxes;
                // out of place first, then in place: the same bits
                std::vector<float> ob(c.boxes.size());
                std::vector<int32_t> oa(c.n), ol(c.n);
                {
                    TrkArgs b = c.a;
                    b.boxes_out = ob.data(), b.alive_out = oa.data(), b.lost_out = ol.data();
                    std::vector<TrkTrack> tr(c.n);
                    std::vector<uint64_t> dup(c.n);
                    for (int i = 0; i < c.n; ++i) trk_update(b, i, tr[i]);
                    for (int i = 0; i < c.n; ++i) dup[i] = trk_pairs(b, i, tr.data());
                    uint64_t dead;
                    trk_resolve(b, tr.data(), dup.data(), dead);
                }
                c.step();
                CHECK(std::memcmp(ob.data(), c.boxes.data(), ob.size() * 4) == 0 && oa == c.alive && ol == c.lost, "in place differs (n %d K %d)", c.n, c.K);
                for (int i = 0; i < c.n; ++i) {
                    for (int q = 0; q < 4; ++q) CHECK(std::isfinite(c.boxes[4 * i + q]), "box %d[%d] = %f", i, q, c.boxes[4 * i + q]);
                    CHECK(c.boxes[4 * i + 2] > c.boxes[4 * i] && c.boxes[4 * i + 3] > c.boxes[4 * i + 1], "box %d is empty", i);
                    CHECK(!(alive0[i] == 0 && c.alive[i] != 0), "track %d revived", i);
                    if (!alive0[i]) CHECK(c.lost[i] == lost0[i] && std::memcmp(&boxes0[4 * i], &c.boxes[4 * i], 16) == 0, "dead slot %d changed", i);
                    if (alive0[i] && c.lost[i] != 0) CHECK(c.lost[i] == lost0[i] + 1 && std::memcmp(&boxes0[4 * i], &c.boxes[4 * i], 16) == 0, "miss %d", i);
                    if (c.a.smooth == 0.0 && alive0[i] && c.lost[i] == 0)
                        CHECK(c.boxes[4 * i + 2] - c.boxes[4 * i] >= 7.99f && c.boxes[4 * i + 3] - c.boxes[4 * i + 1] >= 7.99f, "min_side %d", i);
                    // the crop's corners (0, 0) and (w - 1, h - 1) land on the corners of the padded, aspect-fixed box
                    const double* m = &c.maps[6 * i];
                    const double cx = c.centers[2 * i], cy = c.centers[2 * i + 1], sw = c.scales[2 * i], shh = c.scales[2 * i + 1];
                    const double tol = 1e-4 * (std::fabs(cx) + std::fabs(cy) + sw + shh);
                    CHECK(std::fabs(m[2] - (cx - 0.5 * sw)) <= tol && std::fabs(m[5] - (cy - 0.5 * shh)) <= tol, "slot %d: origin", i);
                    CHECK(std::fabs(m[0] * 191 + m[2] - (cx + 0.5 * sw)) <= tol && std::fabs(m[4] * 255 + m[5] - (cy + 0.5 * shh)) <= tol, "slot %d: far corner", i);
                    CHECK(m[1] == 0.0 && m[3] == 0.0, "slot %d: rotation terms", i);
                }
                bool finite0 = true;  // (a non-finite coordinate makes the OKS NaN, which is above no threshold)
                for (int k = 0; k < c.K; ++k) finite0 = finite0 && std::isfinite(c.records[k * TRK_RECORD]) && std::isfinite(c.records[k * TRK_RECORD + 1]);
                if (c.n > 1 && rep % 4 == 0 && alive0[0] && finite0) CHECK(!(c.alive[0] && c.alive[1] && c.lost[0] == 0 && c.lost[1] == 0), "duplicate survived");
            }
        }
}

int main() {
    CHECK(trk_check_params(0.3, 4, 1.25, 8, 0, 10, 0.9) == nullptr, "defaults refused");
    CHECK(trk_check_params(std::nan(""), 4, 1.25, 8, 0, 10, 0.9) && trk_check_params(0.3, 0, 1.25, 8, 0, 10, 0.9) &&
              trk_check_params(0.3, 4, 0, 8, 0, 10, 0.9) && trk_check_params(0.3, 4, 1.25, 0, 0, 10, 0.9) &&
              trk_check_params(0.3, 4, 1.25, 8, 1.0, 10, 0.9) && trk_check_params(0.3, 4, 1.25, 8, 0, -1, 0.9),
          "a bad parameter set passed");
    const double ones[5] = {1, 2, 3, 4, 5};
    CHECK(trk_tree_sum(5, [&](int k) { return ones[k]; }) == 15.0 && trk_tree_sum(1, [&](int k) { return ones[k]; }) == 1.0, "tree sum");
    CHECK(trk_tree_sum(256, [&](int) { return 1.0; }) == 256.0, "tree sum at TRK_MAX_K");
    crafted();
    random_cases();
    if (g_failures) {
        std::printf("%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("track_host_check: all checks passed\n");
    return 0;
}
