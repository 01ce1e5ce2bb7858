// Shared host-side helpers of libprobpose_mi355x.so: status codes, thread-local error
// string, launch checking, and the workgroup scans. gfx950 only -- no dual paths, no CUDA shims.
// (the device-side primitives of the kernels are in pp_device.h)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/probpose_mi355x.h"
#include "pp_device.h"  // WAVE, lane_id, wave_id (block_scan below) and the matrix kernels' device primitives

namespace pp {

void set_error(const char* fmt, ...);
int option(const char* name);  // explicit dev switches (pp_set_option); the library never reads the environment
// Diagnostics (pp_launch_count): every kernel launch is tallied under its source file's name ("pp_winograd.hip") and, where a file holds
// several kernel families, under an explicit tag as well ("linear_dma_tile"). Host side, a few string compares per launch.
void count_launch(const char* file_or_tag);

inline int fail(int code, const char* what) {
    set_error("%s", what);
    return code;
}

// Argument check at the head of every entry point. It also drops whatever error an EARLIER runtime call of this
// thread (the caller's, e.g. a device probe of the framework around us) left in HIP's sticky per-thread slot, so that
// PP_LAUNCH_CHECK reports this entry point's own launches only.
#define PP_REQUIRE(cond, code, msg)          \
    do {                                     \
        (void)hipGetLastError();             \
        if (!(cond)) {                       \
            ::pp::set_error("%s", (msg));    \
            return (code);                   \
        }                                    \
    } while (0)

#define PP_HIP_CHECK(expr)                                                              \
    do {                                                                                \
        hipError_t e__ = (expr);                                                        \
        if (e__ != hipSuccess) {                                                        \
            ::pp::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),     \
                            __FILE__, __LINE__);                                        \
            return PP_ERR_HIP;                                                          \
        }                                                                               \
    } while (0)

// Called after every kernel launch: surfaces launch-configuration errors without syncing.
#define PP_LAUNCH_CHECK()                  \
    do {                                   \
        ::pp::count_launch(__FILE__);      \
        PP_HIP_CHECK(hipGetLastError());   \
    } while (0)
#define PP_LAUNCH_CHECK_AS(tag)            \
    do {                                   \
        ::pp::count_launch(tag);           \
        PP_LAUNCH_CHECK();                 \
    } while (0)

// Exclusive prefix of v over the 256 threads of a workgroup; total <- the sum. lds: four words.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* lds, uint32_t& total) {
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane_id() >= o) incl += up;
    }
    if (lane_id() == WAVE - 1) lds[wave_id()] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t s = lds[w];
        if (w < wave_id()) before += s;
        total += s;
    }
    __syncthreads();  // (lds is free for the next call)
    return before + incl - v;
}

// One workgroup: out[i] <- the sum of in[0 .. i) over n entries, in[] read with a stride of `stride` words; returns the total.
__device__ __forceinline__ unsigned long long scan_u32_to_u64(const uint32_t* in, int stride, long long n, unsigned long long* out, uint32_t* red) {
    unsigned long long carry = 0;
    for (long long base = 0; base < n; base += 256) {
        const long long i = base + threadIdx.x;
        const uint32_t v = i < n ? in[i * stride] : 0u;
        uint32_t total;
        const uint32_t before = block_scan(v, red, total);
        if (i < n) out[i] = carry + before;
        carry += total;
    }
    return carry;
}

}  // namespace pp
