// The pose tracker's box rule for gfx950: the person boxes of frame t + 1 from the poses of frame t, and the crop parameters that
// go with them, in ONE launch of one 64-lane workgroup - lane i owns track i (at most 64 tracks). Between two frames of a video the
// loop is then warp, model step, record pack and this launch, with no host round trip (probpose_code_amd/tracking.py).
//
// Phases, separated by workgroup barriers (bodies in pp_track_core.h, shared with scripts/track_host_check.cpp):
//   update   lane i: its track's keypoints to image space, the gate, the new box or the lost count
//   pairs    lane i: the OKS of its updated track to every updated track j > i, as a 64-bit mask in LDS
//   resolve  lane 0: the masks in a fixed pair order - the result never depends on scheduling
//   affine   lane i: centre, scale and the dst -> src map of pp_warp_affine_u8 for its slot's box
// A lane reads and writes global rows of its own track only (lane 0 also clears `alive` of a duplicate, which nobody reads again), so the
// state may be updated in place. Plain vector stores, no atomics, sums over K through one fixed tree: the same bits launch after launch.
// The work is a few hundred flops per track and latency-bound by design: it exists to keep the host out of the loop, not to fill the chip.
#include "pp_common.h"
#include "pp_track_core.h"

namespace pp {
namespace {

static_assert(TRK_MAX_TRACKS == PP_TRACK_MAX_TRACKS && TRK_MAX_K == PP_TRACK_MAX_KEYPOINTS, "header and core disagree");
static_assert(TRK_MAX_TRACKS == WAVE, "one lane per track, one mask bit per lane");

__global__ __launch_bounds__(TRK_MAX_TRACKS) void track_update_kernel(TrkArgs a) {
    __shared__ TrkTrack tr[TRK_MAX_TRACKS];
    __shared__ uint64_t dup[TRK_MAX_TRACKS];
    const int i = threadIdx.x;
    if (a.records) {
        if (i < a.n) trk_update(a, i, tr[i]);
        __syncthreads();
        if (i < a.n) dup[i] = trk_pairs(a, i, tr);
        __syncthreads();
        if (i == 0) {
            uint64_t dead;
            trk_resolve(a, tr, dup, dead);
        }
    }
    // (a lane reads back only the box it wrote itself)
    if (a.next_maps && i < a.n)
        trk_affine(a.boxes_out + 4 * i, a.pad, a.aspect, a.out_w1, a.out_h1, a.next_centers + 2 * i, a.next_scales + 2 * i, a.next_maps + 6 * i);
}

int check_affine(const char* fn, int n, int input_w, int input_h, double input_padding) {
    if (n < 1 || n > TRK_MAX_TRACKS) {
        set_error("%s: n must be in 1..%d (one workgroup, one lane per track), got %d", fn, TRK_MAX_TRACKS, n);
        return PP_ERR_INVALID_ARG;
    }
    if (input_w < 2 || input_h < 2 || input_w > 32767 || input_h > 32767) {
        set_error("%s: the input size must be in 2..32767 per side, got %d x %d", fn, input_w, input_h);
        return PP_ERR_INVALID_ARG;
    }
    if (!(input_padding > 0.0) || !trk_finite(input_padding)) {
        set_error("%s: input_padding must be positive and finite", fn);
        return PP_ERR_INVALID_ARG;
    }
    return PP_OK;
}

void set_affine(TrkArgs& a, int input_w, int input_h, double input_padding, float* centers, float* scales, double* maps) {
    a.pad = (float)input_padding;                  // numpy: a Python float beside a float32 array is float32
    a.aspect = (float)((double)input_w / input_h);  // aspect_ratio = w / h
    a.out_w1 = (float)(input_w - 1), a.out_h1 = (float)(input_h - 1);
    a.next_centers = centers, a.next_scales = scales, a.next_maps = maps;
}

}  // namespace
}  // namespace pp

extern "C" int pp_track_update(const double* records, const float* centers, const float* scales, int n, int K, int input_w, int input_h,
                               int gate, const double* sigmas, const float* boxes_in, const int32_t* alive_in, const int32_t* lost_in,
                               double kpt_thr, int min_keypoints, double expand, double min_side, double smooth, int max_lost,
                               double dup_oks_thr, float* boxes_out, int32_t* alive_out, int32_t* lost_out, double input_padding,
                               float* next_centers, float* next_scales, double* next_maps, void* stream) {
    using namespace pp;
    (void)hipGetLastError();  // (a stale error of the caller's, as PP_REQUIRE drops it)
    if (const int st = check_affine("pp_track_update", n, input_w, input_h, input_padding)) return st;
    PP_REQUIRE(K >= 1 && K <= TRK_MAX_K, PP_ERR_INVALID_ARG, "pp_track_update: K must be in 1..256");
    PP_REQUIRE(gate == PP_TRACK_GATE_PROB || gate == PP_TRACK_GATE_CONF, PP_ERR_INVALID_ARG,
               "pp_track_update: gate must be PP_TRACK_GATE_PROB or PP_TRACK_GATE_CONF");
    if (const char* why = trk_check_params(kpt_thr, min_keypoints, expand, min_side, smooth, max_lost, dup_oks_thr)) {
        set_error("pp_track_update: %s", why);
        return PP_ERR_INVALID_ARG;
    }
    PP_REQUIRE(records && centers && scales && sigmas && boxes_in && alive_in && lost_in && boxes_out && alive_out && lost_out,
               PP_ERR_INVALID_ARG, "pp_track_update: records, centers, scales, sigmas and the track state in and out must be non-NULL");
    const bool any = next_centers || next_scales || next_maps, all = next_centers && next_scales && next_maps;
    PP_REQUIRE(any == all, PP_ERR_INVALID_ARG, "pp_track_update: next_centers, next_scales and next_maps are given together or not at all");
    TrkArgs a{};
    a.records = records, a.centers = centers, a.scales = scales, a.sigmas = sigmas, a.n = n, a.K = K;
    a.in_w = (double)input_w, a.in_h = (double)input_h;
    a.gate_col = gate == PP_TRACK_GATE_PROB ? 3 : 2;
    a.kpt_thr = kpt_thr, a.expand = expand, a.min_side = min_side, a.smooth = smooth, a.dup_oks_thr = dup_oks_thr;
    a.min_keypoints = min_keypoints, a.max_lost = max_lost;
    a.boxes_in = boxes_in, a.alive_in = alive_in, a.lost_in = lost_in;
    a.boxes_out = boxes_out, a.alive_out = alive_out, a.lost_out = lost_out;
    set_affine(a, input_w, input_h, input_padding, next_centers, next_scales, next_maps);
    hipLaunchKernelGGL(track_update_kernel, dim3(1), dim3(TRK_MAX_TRACKS), 0, reinterpret_cast<hipStream_t>(stream), a);
    PP_LAUNCH_CHECK_AS("track_update");
    return PP_OK;
}

extern "C" int pp_track_affine_params(const float* boxes, int n, int input_w, int input_h, double input_padding, float* centers,
                                      float* scales, double* maps, void* stream) {
    using namespace pp;
    (void)hipGetLastError();
    if (const int st = check_affine("pp_track_affine_params", n, input_w, input_h, input_padding)) return st;
    PP_REQUIRE(boxes && centers && scales && maps, PP_ERR_INVALID_ARG, "pp_track_affine_params: boxes, centers, scales and maps must be non-NULL");
    TrkArgs a{};
    a.n = n;
    a.boxes_out = const_cast<float*>(boxes);  // (read only: without records the kernel runs the affine phase alone)
    set_affine(a, input_w, input_h, input_padding, centers, scales, maps);
    hipLaunchKernelGGL(track_update_kernel, dim3(1), dim3(TRK_MAX_TRACKS), 0, reinterpret_cast<hipStream_t>(stream), a);
    PP_LAUNCH_CHECK_AS("track_affine_params");
    return PP_OK;
}
