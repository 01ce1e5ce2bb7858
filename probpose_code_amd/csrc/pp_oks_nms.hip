// Greedy OKS suppression (oks_nms, mmpose/evaluation/functional/nms.py:119-170, with oks_iou :58-116) of every image of a
// dataset in two launches. The instances arrive in each image's suppression order (the host's scores.argsort()[::-1]:
// numpy's tie order is the host's to decide), so the greedy rule is "walk the rows in order; a row that nobody removed is
// kept and removes every later row it overlaps by more than thr".
//   oks_nms_pairs   one wave per row i of an image: a lane per column j > i computes the pair's OKS in fp64, in numpy's operation
//                   order (this file is built with -ffp-contract=off); the suppression bits of 64 columns are gathered by a wave
//                   ballot and written as one 64-bit word by one vector store. No atomics, no word is written twice.
//   oks_nms_sweep   one wave per image: the removed set lives in registers, one 64-bit word per lane (64 x 64 = 4096 instances);
//                   row i is kept if its bit is clear, then its word row is ORed in.
// Exactness: the reference compares float32(oks) with float32(thr), i.e. fp64 oks against the rounding midpoint above
// float32(thr). exp() and the summation order may differ from numpy's in the last bits, which can only matter for an OKS
// next to that midpoint: a pair within `guard` of it marks its image PP_OKS_NMS_UNDECIDED and the caller decides it on the host.
#include <cmath>
#include <vector>

#include "pp_common.h"

namespace pp {

constexpr int kNmsRowsPerBlock = 16;  // rows of one image per workgroup of four waves

struct OksNmsParams {
    const double* kpts;    // (N, K, 3) x, y, (third value not read)
    const double* areas;   // (N)
    const double* sigmas;  // (K)
    const long long* inst_off;  // (I + 1) first instance of an image
    const long long* word_off;  // (I + 1) first matrix word of an image (an image above the capacity has none)
    const int* items;           // (n_items, 2) image, first row of the block
    unsigned long long* matrix;  // image i: n rows of ceil(n / 64) words; bit j of row r = "r removes j"; words below r / 64 unwritten
    unsigned char* row_near;     // (N) a pair of this row lies within guard of the midpoint
    unsigned char* keep;         // (N)
    int* status;                 // (I)
    int K, area_f32;
    double midpoint, guard;
};

// the reference's e / oks of rows a and b (global indices), fp64
__device__ __forceinline__ double oks_pair(const OksNmsParams& p, long long a, long long b) {
    const double* g = p.kpts + a * p.K * 3;
    const double* d = p.kpts + b * p.K * 3;
    double half;  // (a_g + a_d) / 2: in the areas' own dtype (float32 areas add and halve in float32), then + np.spacing(1) in fp64
    if (p.area_f32) half = (double)(((float)p.areas[a] + (float)p.areas[b]) / 2.0f);
    else half = (p.areas[a] + p.areas[b]) / 2;
    const double scale = half + 2.220446049250313e-16;
    double sum = 0.0;
    for (int k = 0; k < p.K; ++k) {
        const double dx = d[3 * k] - g[3 * k], dy = d[3 * k + 1] - g[3 * k + 1];
        const double s2 = p.sigmas[k] * 2;
        const double e = (dx * dx + dy * dy) / (s2 * s2) / scale / 2;
        sum += exp(-e);
    }
    return sum / (double)p.K;
}

__global__ __launch_bounds__(256) void oks_nms_pairs(const OksNmsParams p) {
    const int img = p.items[2 * blockIdx.x];
    const long long base = p.inst_off[img];
    const int n = (int)(p.inst_off[img + 1] - base);
    const int W = (n + WAVE - 1) / WAVE;
    unsigned long long* mat = p.matrix + p.word_off[img];
    const int row_end = min(p.items[2 * blockIdx.x + 1] + kNmsRowsPerBlock, n);
    for (int i = p.items[2 * blockIdx.x + 1] + wave_id(); i < row_end; i += 4) {
        bool near = false;
        for (int w = i / WAVE; w < W; ++w) {
            const int j = w * WAVE + lane_id();
            bool remove = false;
            if (j > i && j < n) {
                const double oks = oks_pair(p, base + i, base + j);
                remove = !(oks <= p.midpoint);  // NaN removes: `ovr <= thr` is false
                near |= fabs(oks - p.midpoint) <= p.guard;
            }
            const unsigned long long bits = __ballot(remove);
            if (lane_id() == 0) mat[(long long)i * W + w] = bits;
        }
        const unsigned long long any_near = __ballot(near);
        if (lane_id() == 0) p.row_near[base + i] = any_near != 0ull;
    }
}

__global__ __launch_bounds__(64) void oks_nms_sweep(const OksNmsParams p, int capacity) {
    const int img = blockIdx.x;
    const long long base = p.inst_off[img];
    const long long n64 = p.inst_off[img + 1] - base;
    const int lane = lane_id();
    if (n64 > capacity) {  // the caller's job; its keep bytes are defined all the same
        for (long long r = lane; r < n64; r += WAVE) p.keep[base + r] = 0;
        if (lane == 0) p.status[img] = PP_OKS_NMS_HOST;
        return;
    }
    const int n = (int)n64;
    const int W = (n + WAVE - 1) / WAVE;
    const unsigned long long* mat = p.matrix + p.word_off[img];
    unsigned long long removed = 0, kept = 0;  // lane l: instances 64 l .. 64 l + 63
    bool near = false;
    unsigned long long next = (n > 0 && lane < W) ? mat[lane] : 0ull;  // row 0 (every word of it is written)
    for (int i = 0; i < n; ++i) {
        const unsigned long long row = next;
        const int w1 = (i + 1) / WAVE;
        next = (i + 1 < n && lane >= w1 && lane < W) ? mat[(long long)(i + 1) * W + lane] : 0ull;  // fetched ahead of the decision on row i
        const unsigned long long word = __shfl(removed, i / WAVE);
        if (!((word >> (i % WAVE)) & 1ull)) {
            removed |= row;
            if (lane == i / WAVE) kept |= 1ull << (i % WAVE);
        }
    }
    for (int c = 0; c < W; ++c) {
        const unsigned long long word = __shfl(kept, c);  // (read with every lane active)
        const int r = c * WAVE + lane;
        if (r < n) {
            p.keep[base + r] = (unsigned char)((word >> lane) & 1ull);
            near |= p.row_near[base + r] != 0;
        }
    }
    const unsigned long long any_near = __ballot(near);
    if (lane == 0) p.status[img] = any_near ? PP_OKS_NMS_UNDECIDED : PP_OKS_NMS_DECIDED;
}

// the layout both entry points agree on: [inst_off (I + 1) i64][word_off (I + 1) i64][items (n_items, 2) i32, padded to 8][row_near (N), padded to 8][matrix]
struct OksNmsLayout {
    long long n_items, n_words, items_at, near_at, matrix_at, total;
};

static int oks_nms_layout(const long long* img_off, long long N, int I, OksNmsLayout& l, const char* who) {
    char msg[160];
    if (N < 0 || I < 0) {
        snprintf(msg, sizeof msg, "%s: negative count", who);
        return fail(PP_ERR_INVALID_ARG, msg);
    }
    if (!img_off) {
        snprintf(msg, sizeof msg, "%s: NULL image offsets", who);
        return fail(PP_ERR_INVALID_ARG, msg);
    }
    l.n_items = l.n_words = 0;
    bool ok = img_off[0] == 0 && img_off[I] == N;
    for (int i = 0; i < I && ok; ++i) {
        const long long n = img_off[i + 1] - img_off[i];
        ok = n >= 0;
        if (n > 0 && n <= PP_OKS_NMS_MAX_PER_IMAGE) {
            l.n_items += (n + kNmsRowsPerBlock - 1) / kNmsRowsPerBlock;
            l.n_words += n * ((n + WAVE - 1) / WAVE);
        }
    }
    if (!ok) {
        snprintf(msg, sizeof msg, "%s: image offsets must start at 0, never decrease and end at n_instances", who);
        return fail(PP_ERR_INVALID_ARG, msg);
    }
    if (l.n_items > 0x7fffffffLL) {
        snprintf(msg, sizeof msg, "%s: too many row blocks for one launch", who);
        return fail(PP_ERR_UNSUPPORTED, msg);
    }
    l.items_at = 2 * (long long)(I + 1) * 8;
    l.near_at = l.items_at + (l.n_items * 8 + 7) / 8 * 8;
    l.matrix_at = l.near_at + (N + 7) / 8 * 8;
    l.total = l.matrix_at + l.n_words * 8;
    return PP_OK;
}

}  // namespace pp

extern "C" long long pp_oks_nms_workspace_bytes(const long long* img_off_host, long long n_instances, int n_images) {
    using namespace pp;
    OksNmsLayout l;
    const int st = oks_nms_layout(img_off_host, n_instances, n_images, l, "pp_oks_nms_workspace_bytes");
    return st == PP_OK ? l.total : st;
}

extern "C" int pp_oks_nms_batch(const double* kpts, const double* areas, const long long* img_off_host, const double* sigmas,
                                long long n_instances, int n_images, int K, double thr, double guard, int area_f32,
                                void* workspace, long long workspace_bytes, unsigned char* keep, int* status, void* stream) {
    using namespace pp;
    PP_REQUIRE(n_instances >= 0 && n_images >= 0, PP_ERR_INVALID_ARG, "pp_oks_nms_batch: negative count");
    PP_REQUIRE(K > 0, PP_ERR_INVALID_ARG, "pp_oks_nms_batch: K must be positive");
    PP_REQUIRE(img_off_host && sigmas, PP_ERR_INVALID_ARG, "pp_oks_nms_batch: NULL argument");
    PP_REQUIRE(n_images == 0 || (status && workspace), PP_ERR_INVALID_ARG, "pp_oks_nms_batch: NULL argument");
    PP_REQUIRE(n_instances == 0 || (kpts && areas && keep), PP_ERR_INVALID_ARG, "pp_oks_nms_batch: NULL argument");
    PP_REQUIRE(thr == thr && guard >= 0.0 && std::isfinite(thr) && std::isfinite(guard), PP_ERR_INVALID_ARG,
               "pp_oks_nms_batch: thr and guard must be finite, guard >= 0");
    PP_REQUIRE(n_instances * (long long)K * 3 < (1LL << 40), PP_ERR_UNSUPPORTED, "pp_oks_nms_batch: too many keypoints");
    OksNmsLayout l;
    const int st = oks_nms_layout(img_off_host, n_instances, n_images, l, "pp_oks_nms_batch");
    if (st != PP_OK) return st;
    PP_REQUIRE(workspace_bytes >= l.total, PP_ERR_WORKSPACE, "pp_oks_nms_batch: workspace smaller than pp_oks_nms_workspace_bytes");
    if (n_images == 0) return PP_OK;
    PP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, PP_ERR_INVALID_ARG, "pp_oks_nms_batch: workspace must be 8-byte aligned");

    // the tables of this batch: offsets and the (image, first row) list of the pairs launch, built here and uploaded in one copy
    std::vector<long long> table((size_t)(l.near_at / 8), 0);
    long long words = 0;
    int* items = reinterpret_cast<int*>(table.data() + 2 * (n_images + 1));
    long long it = 0;
    for (int i = 0; i <= n_images; ++i) {
        table[i] = img_off_host[i];
        table[n_images + 1 + i] = words;
        if (i == n_images) break;
        const long long n = img_off_host[i + 1] - img_off_host[i];
        if (n > 0 && n <= PP_OKS_NMS_MAX_PER_IMAGE) {
            for (long long r = 0; r < n; r += kNmsRowsPerBlock, ++it) {
                items[2 * it] = i;
                items[2 * it + 1] = (int)r;
            }
            words += n * ((n + WAVE - 1) / WAVE);
        }
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    PP_HIP_CHECK(hipMemcpyWithStream(ws, table.data(), (size_t)l.near_at, hipMemcpyHostToDevice, s));  // (done when it returns: `table` is local)

    const float t32 = (float)thr;  // float32(oks) > float32(thr)  <=>  oks above the rounding midpoint of t32 and its successor
    const double midpoint = ((double)t32 + (double)std::nextafterf(t32, INFINITY)) / 2;
    OksNmsParams p{kpts, areas, sigmas, reinterpret_cast<const long long*>(ws), reinterpret_cast<const long long*>(ws) + n_images + 1,
                   reinterpret_cast<const int*>(ws + l.items_at), reinterpret_cast<unsigned long long*>(ws + l.matrix_at),
                   reinterpret_cast<unsigned char*>(ws + l.near_at), keep, status, K, area_f32 ? 1 : 0, midpoint, guard};
    if (l.n_items > 0) {
        hipLaunchKernelGGL(oks_nms_pairs, dim3((unsigned)l.n_items), dim3(256), 0, s, p);
        PP_LAUNCH_CHECK_AS("oks_nms_pairs");
    }
    hipLaunchKernelGGL(oks_nms_sweep, dim3(n_images), dim3(64), 0, s, p, (int)PP_OKS_NMS_MAX_PER_IMAGE);
    PP_LAUNCH_CHECK_AS("oks_nms_sweep");
    return PP_OK;
}
