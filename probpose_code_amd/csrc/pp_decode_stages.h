// Stages the decode kernels share (pp_decode.hip, pp_udp_decode.hip, pp_argmax_decode.hip), each written once:
//   * the head's map construction: x / T -> Sparsemax over the H*W pixels -> * normalize -> clamp(0, 1) per pass, flip-back and
//     average, into an x-padded LDS map                                                        (probmap_head.py:637-646, tta.py:35-39, 64-66)
//   * UDP argmax + DARK refinement from an averaged map in LDS on                               (post_processing.py:178-249, refinement.py:125-157)
// A kernel that chains the two gives the bits of the two kernels launched one after the other only because it runs THIS code in
// the same thread mapping (the fp32 sums of the Sparsemax threshold search depend on who adds what).
#pragma once
#include <cmath>

#include "pp_common.h"
#include "pp_device.h"

// numpy evaluates the fp32 expressions one rounding per operator; keep it so (the including files say the same).
#pragma clang fp contract(off)

namespace pp {

constexpr int PAD = 12;            // x-padding of the LDS map either side: >= the largest radius and a multiple of 4, so that a pixel quad (y, 4 q .. 4 q + 3)
                                   // is a 16-byte aligned slot (ds_write_b128 / ds_read_b128: one conflict-free access per quad)
#ifndef PP_DEC_THREADS
#define PP_DEC_THREADS 256  // dev A/B: 128 (two waves per workgroup, 64 x 48 maps only) measured 53 us against 36: the chain gets longer, nothing is saved
#endif
constexpr int DEC_THREADS = PP_DEC_THREADS;
constexpr int RED_BYTES = 512;  // cross-wave reduction scratch at the head of the dynamic LDS region
constexpr int SMX_CAP = 1024;   // candidates per row the compact threshold search holds (two lists of SMX_CAP floats from the map's first byte)

// i / d for 0 <= i < 2^20, 1 <= d <= 2^12 in three VALU instructions (the integer division is ~25, and the kernel did some forty
// of them per thread): (i + 0.5) / d is at least 0.5 / d away from an integer, the float product is off by < q 2^-22.
struct FastDiv {
    float r;
    __device__ __forceinline__ explicit FastDiv(int d) : r(1.0f / (float)d) {}
    __device__ __forceinline__ int operator()(int i) const { return (int)(((float)i + 0.5f) * r); }
};

// ---- lane exchanges of the xor butterfly (32, 16, 8, 4, 2, 1 - the pairing order __shfl_xor loops have, so sums keep their
// bits) without the LDS queue: the gfx950 row swaps for 32 / 16 (each lane ends up with its own and its partner's value: any
// commutative op takes them in either order), DPP row rotate / shifts / quad permutes below that.
__device__ __forceinline__ int dpp_xor8(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false); }  // row_ror:8
__device__ __forceinline__ int dpp_xor4(int v) {
    const int t = __builtin_amdgcn_update_dpp(0, v, 0x104, 0xf, 0x5, false);  // row_shl:4 into lanes 0-3, 8-11 of a row
    return __builtin_amdgcn_update_dpp(t, v, 0x114, 0xf, 0xa, false);         // row_shr:4 into lanes 4-7, 12-15
}
__device__ __forceinline__ int dpp_xor2(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x4e, 0xf, 0xf, false); }  // quad_perm [2,3,0,1]
__device__ __forceinline__ int dpp_xor1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xb1, 0xf, 0xf, false); }  // quad_perm [1,0,3,2]

template <class T, class Op>
__device__ __forceinline__ T wave_allreduce(T v, Op op) {
    static_assert(sizeof(T) == 4, "one dword");
    auto I = [](T x) { return __builtin_bit_cast(int, x); };
    auto V = [](int x) { return __builtin_bit_cast(T, x); };
    {
        const auto s = __builtin_amdgcn_permlane32_swap((unsigned)I(v), (unsigned)I(v), false, false);
        v = op(V((int)s[0]), V((int)s[1]));
    }
    {
        const auto s = __builtin_amdgcn_permlane16_swap((unsigned)I(v), (unsigned)I(v), false, false);
        v = op(V((int)s[0]), V((int)s[1]));
    }
    v = op(v, V(dpp_xor8(I(v))));
    v = op(v, V(dpp_xor4(I(v))));
    v = op(v, V(dpp_xor2(I(v))));
    v = op(v, V(dpp_xor1(I(v))));
    return v;
}

// ---- block-wide reductions for the in-register Sparsemax (4 waves)
struct SmxStat {
    float s0, s1;
    int n;  // candidates of the two rows, n0 | n1 << 16 (a row has at most 12 288 pixels)
};

__device__ __forceinline__ void block_max2(float& a, float& b, float* scratch) {
    a = wave_allreduce(a, [](float x, float y) { return fmaxf(x, y); });
    b = wave_allreduce(b, [](float x, float y) { return fmaxf(x, y); });
    if (lane_id() == 0) {
        scratch[2 * wave_id()] = a;
        scratch[2 * wave_id() + 1] = b;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < DEC_THREADS / WAVE; ++w) {
        a = fmaxf(a, scratch[2 * w]);
        b = fmaxf(b, scratch[2 * w + 1]);
    }
}

// `quiet`: no lane of this wave has a candidate left (wave-uniform) - its partial sums are zeros without the exchanges
__device__ __forceinline__ SmxStat block_sum_stat(SmxStat v, bool quiet, SmxStat* scratch) {
    if (!quiet) {
        v.s0 = wave_allreduce(v.s0, [](float x, float y) { return x + y; });
        v.s1 = wave_allreduce(v.s1, [](float x, float y) { return x + y; });
        v.n = wave_allreduce(v.n, [](int x, int y) { return x + y; });
    }
    if (lane_id() == 0) scratch[wave_id()] = v;
    __syncthreads();
    SmxStat r = scratch[0];
#pragma unroll
    for (int w = 1; w < DEC_THREADS / WAVE; ++w) {  // fixed order: every thread gets the same bits
        r.s0 += scratch[w].s0;
        r.s1 += scratch[w].s1;
        r.n += scratch[w].n;
    }
    return r;
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

// A thread owns the pixel QUADS q = tid + 256 e (e < NV): pixels (y, x0 .. x0 + 3), y = q / (W / 4), x0 = 4 (q % (W / 4)) - the same
// quads whatever the memory layout of the input, so both layouts give the same bits; a quad is one 16-byte aligned LDS slot.
// (Measured and dropped, round 4: lane pairs (l, l + 32) sharing an octet, numbered row-parity-major, so that a half-wave reads 512
// contiguous bytes of one phase block and two v_permlane32_swap interleave the columns - 39.3 / 37.3 us against 37.8 / 35.8 for the
// two 8-byte loads per quad below: the octet order puts the lanes' 16-byte LDS stores 32 bytes apart, 2-way conflicts.)
struct QuadMap {
    int tid, HW4, W4;
    FastDiv div_w4;
    __device__ __forceinline__ QuadMap(int tid_, int H, int W) : tid(tid_), HW4((H * W) >> 2), W4(W >> 2), div_w4(W >> 2) {}
    __device__ __forceinline__ bool operator()(int e, int& y, int& x0) const {
        const int i4 = tid + e * DEC_THREADS;
        if (i4 >= HW4) return false;
        y = div_w4(i4);
        x0 = (i4 - y * W4) * 4;
        return true;
    }
};

// The quad (y, x0 ..) of a map in memory. Row-major: one 16-byte vector. Phase-separated (the fused deconvolution head
// writes the four 2x2 output phases one after the other, each a (H/2, W/2) row-major block): two 8-byte pairs - columns
// x0 / 2, x0 / 2 + 1 of row y / 2 of the phases (y & 1, 0) and (y & 1, 1) - interleaved.
__device__ __forceinline__ f32x4 load_quad(const f32x4* base, bool ok, int y, int x0, int phased, int HW4, int W4) {
    const float ninf = -__builtin_inff();
    f32x4 r{ninf, ninf, ninf, ninf};
    if (!ok) return r;
    if (!phased) return base[y * W4 + (x0 >> 2)];
    const f32x2* pb = reinterpret_cast<const f32x2*>(base) + ((y & 1) * HW4 + (y >> 1) * W4 + (x0 >> 2));  // (in pairs: a phase block is HW4 / 2 pairs)
    const f32x2 a = pb[0], c = pb[HW4 >> 1];
    return f32x4{a[0], c[0], a[1], c[1]};
}

// ---- Sparsemax of one keypoint's row and (flip test) of its mirror partner's row, both in registers, then the averaged map into
// mapf ([H][W + 2 PAD], data from column PAD). `smem`: the head of the dynamic LDS region (RED_BYTES of scratch); the map region
// doubles as the candidate lists (2 SMX_CAP floats) until the thresholds are known. When a logit is not finite - workgroup-uniform -
// nothing is written, on_bad() runs (the caller's NaN results) and false comes back. The caller puts a barrier between this and its first read of the map.
// Sort-free threshold search (Michelot): candidates z > tau, tau <- tau + (sum_cand (z - tau) - 1) / |cand|,
// starting from tau = max - 1 (a lower bound of the solution), until no candidate is dropped. The
// correction form keeps the sums O(1), so fp32 accumulation loses nothing against the fp32 reference.
// NV = 16-byte vectors of the H*W row per thread (3 for 64x48, 7 for 96x72). Needs W % 4 == 0.
template <bool HAS_FLIP, int NV, class OnBad>
__device__ __forceinline__ bool sparsemax_average(const f32x4* src, const f32x4* srcf, char* smem, float* mapf, int H, int W, float temperature, float normalize,
                                                  int phased, int shift, OnBad&& on_bad) {
    const int tid = threadIdx.x;
    const int Wp = W + 2 * PAD;
    const int HW4 = (H * W) >> 2, W4 = W >> 2;
    const QuadMap quad(tid, H, W);
    float* fscr = reinterpret_cast<float*>(smem);
    SmxStat* sscr = reinterpret_cast<SmxStat*>(smem + 64);
    f32x4 z0[NV], z1[NV];
    float m0 = -__builtin_inff(), m1 = -__builtin_inff(), chk = 0.f;
    // a division costs nine VALU instructions, the row has 24 per thread: multiply when the temperature is a normal power of two
    const unsigned t_bits = __builtin_bit_cast(unsigned, temperature);
    const bool t_pow2 = (t_bits & 0x007fffffu) == 0 && (t_bits >> 23) >= 2 && (t_bits >> 23) <= 252;
    const float t_inv = __builtin_bit_cast(float, (254u << 23) - t_bits);
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        int y = 0, x0 = 0;
        const bool ok = quad(e, y, x0);
        z0[e] = load_quad(src, ok, y, x0, phased, HW4, W4);
        z1[e] = z0[e];
        if (HAS_FLIP) z1[e] = load_quad(srcf, ok, y, x0, phased, HW4, W4);
        if (t_pow2) {  // x / 2^k == x * 2^-k bit for bit (-inf of a lane without a quad stays -inf)
            z0[e] = z0[e] * t_inv;
            if (HAS_FLIP) z1[e] = z1[e] * t_inv;
        } else {
            z0[e] = z0[e] / temperature;
            if (HAS_FLIP) z1[e] = z1[e] / temperature;
        }
        if (!HAS_FLIP) { const float ninf = -__builtin_inff(); z1[e] = f32x4{ninf, ninf, ninf, ninf}; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m0 = fmaxf(m0, z0[e][j]);
            m1 = fmaxf(m1, z1[e][j]);
            if (ok) {  // x * 0 is NaN for x = +-inf / NaN: one fma per logit finds a non-finite input (fmaxf would skip a NaN)
                chk = __builtin_fmaf(z0[e][j], 0.f, chk);
                if (HAS_FLIP) chk = __builtin_fmaf(z1[e][j], 0.f, chk);
            }
        }
    }
    if (chk != chk) m0 = __builtin_inff();
    block_max2(m0, m1, fscr);
    // A non-finite logit (an operand beyond the split-fp16 range upstream - numeric domain, include/probpose_mi355x.h - or a NaN input) must not
    // decode to pixel 0 with a plausible score: the keypoint comes out as NaN, which the host mirror turns into a FloatingPointError.
    if (!(fabsf(m0) < __builtin_inff()) || (HAS_FLIP && !(fabsf(m1) < __builtin_inff()))) {  // (workgroup-uniform)
        on_bad();
        return false;
    }
    // normalize < 0 stands for the head's `normalize=None` (probmap_head.py:249,642-646): no Sparsemax, the map is
    // clamp(x / T, 0, 1) - the same code with threshold 0, no shift and scale 1
    const bool smx = normalize >= 0.f;
    if (!smx) {
        m0 = m1 = 0.f;
        normalize = 1.f;
    }
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        z0[e] -= m0;
        z1[e] -= m1;
    }
    float tau0 = smx ? -1.0f : 0.f, tau1 = tau0;
    int prev = -1;
    bool alive = true;  // the thresholds only rise: a thread without a candidate now has none in any later round
    // COMPACT form of the threshold search (round 6). The search only ever looks at the candidates of its FIRST threshold (z > max - 1: the
    // thresholds rise, nothing comes back) - a few dozen of a row's 3 072 logits on a peaked map - yet every round walked all 24 (48 with
    // the flipped pass) values of every thread and paid a block-wide reduction: ~260 instructions x 4 - 6 rounds of the kernel's ~2 550 per
    // wave. Now the first threshold's candidates are packed into an LDS list once (a block-wide prefix sum of the per-thread counts) and
    // every wave runs the rounds on the list by itself: a lane per candidate, wave reductions, no barrier. Same rounds, same thresholds up
    // to the order of the fp32 sums. Rows with more than SMX_CAP candidates (a flat map) keep the walk below.
    bool compact_done = false;
    if (smx) {
        int c = 0;
#pragma unroll
        for (int e = 0; e < NV; ++e)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c += z0[e][j] > -1.0f ? 1 : 0;
                if (HAS_FLIP) c += z1[e][j] > -1.0f ? (1 << 16) : 0;
            }
        int inc = c;  // inclusive prefix over the wave's lanes (both counts in one word: a row has 3 072 .. 12 288 values)
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int t = __shfl_up(inc, o);
            if (lane_id() >= o) inc += t;
        }
        int* wtot = reinterpret_cast<int*>(smem + 192);
        if (lane_id() == WAVE - 1) wtot[wave_id()] = inc;
        __syncthreads();
        int base = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < DEC_THREADS / WAVE; ++w) {
            const int t = wtot[w];
            base += w < wave_id() ? t : 0;
            tot += t;
        }
        const int n0 = tot & 0xffff, n1 = tot >> 16;
        if (n0 <= SMX_CAP && n1 <= SMX_CAP) {  // (workgroup-uniform)
            float* L0 = mapf;            // the map region is not written before the thresholds are known
            float* L1 = mapf + SMX_CAP;
            const int off = base + inc - c;
            int o0 = off & 0xffff, o1 = off >> 16;
#pragma unroll
            for (int e = 0; e < NV; ++e)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (z0[e][j] > -1.0f) L0[o0++] = z0[e][j];
                    if (HAS_FLIP && z1[e][j] > -1.0f) L1[o1++] = z1[e][j];
                }
            __syncthreads();
            for (int iter = 0; iter < 64; ++iter) {
                float s0 = 0.f, s1 = 0.f;
                int n = 0;
                for (int i = lane_id(); i < n0; i += WAVE) {
                    const float d0 = L0[i] - tau0;
                    if (d0 > 0.f) {
                        s0 += d0;
                        n += 1;
                    }
                }
                if (HAS_FLIP)
                    for (int i = lane_id(); i < n1; i += WAVE) {
                        const float d1 = L1[i] - tau1;
                        if (d1 > 0.f) {
                            s1 += d1;
                            n += 1 << 16;
                        }
                    }
                s0 = wave_allreduce(s0, [](float x, float y) { return x + y; });
                if (HAS_FLIP) s1 = wave_allreduce(s1, [](float x, float y) { return x + y; });
                n = wave_allreduce(n, [](int x, int y) { return x + y; });
                if (n == prev) break;
                prev = n;
                tau0 = tau0 + (s0 - 1.0f) / (float)(n & 0xffff);
                if (HAS_FLIP) tau1 = tau1 + (s1 - 1.0f) / (float)(n >> 16);
            }
            compact_done = true;
            __syncthreads();  // every wave is through with the lists before the map takes their place
        }
    }
    for (int iter = 0; iter < ((smx && !compact_done) ? 64 : 0); ++iter) {
        SmxStat st{0.f, 0.f, 0};
        if (alive) {
#pragma unroll
            for (int e = 0; e < NV; ++e)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d0 = z0[e][j] - tau0;
                    if (d0 > 0.f) {
                        st.s0 += d0;
                        st.n += 1;
                    }
                    if (HAS_FLIP) {
                        const float d1 = z1[e][j] - tau1;
                        if (d1 > 0.f) {
                            st.s1 += d1;
                            st.n += 1 << 16;
                        }
                    }
                }
            alive = st.n != 0;
        }
        st = block_sum_stat(st, __builtin_amdgcn_ballot_w64(alive) == 0, sscr + (iter & 1) * (DEC_THREADS / WAVE));
        if (st.n == prev) break;
        prev = st.n;
        tau0 = tau0 + (st.s0 - 1.0f) / (float)(st.n & 0xffff);
        if (HAS_FLIP) tau1 = tau1 + (st.s1 - 1.0f) / (float)(st.n >> 16);
    }
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        int y, x0;
        if (quad(e, y, x0)) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = clamp01(fmaxf(z0[e][j] - tau0, 0.0f) * normalize);
            *reinterpret_cast<f32x4*>(mapf + y * Wp + PAD + x0) = v;
        }
    }
    if (HAS_FLIP) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            int y, xf;
            if (quad(e, y, xf)) {
                // pixels xf .. xf + 3 of the flipped pass land at W-1-xf .. W-4-xf: the reversed quad at column W-4-xf; exactly
                // one thread owns each cell
                if (!shift) {
                    f32x4* d = reinterpret_cast<f32x4*>(mapf + y * Wp + PAD + (W - 4 - xf));
                    f32x4 v = *d;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[3 - j] = (v[3 - j] + clamp01(fmaxf(z1[e][j] - tau1, 0.0f) * normalize)) * 0.5f;
                    *d = v;
                } else {
                    // shift_heatmap (tta.py:64-66): flipped pixel q lands at column W - q (q >= 1; q = 0 falls off), and the last
                    // one, q = W - 1, also at column 0 - still exactly one thread per cell
                    float* row = mapf + y * Wp + PAD;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int q = xf + j;
                        const float pv = clamp01(fmaxf(z1[e][j] - tau1, 0.0f) * normalize);
                        if (q >= 1) row[W - q] = (row[W - q] + pv) * 0.5f;
                        if (q == W - 1) row[0] = (row[0] + pv) * 0.5f;
                    }
                }
            }
        }
    }
    return true;
}

// ================================================================ UDP argmax + DARK refinement from an averaged map in LDS
constexpr int UDP_THREADS = 256;
constexpr int UDP_MAX_R = PP_MAX_RADIUS;  // blur_kernel_size <= 19
constexpr int UDP_RED_FLOATS = 64;        // cross-wave reduction scratch, from UDP_TAPS_AT the taps of the runtime-radius kernel
constexpr int UDP_TAPS_AT = 32;
// __syncthreads_or (udp_blur) reduces through LDS the compiler allocates statically, 256 bytes per kernel: the dynamic region a launch
// may ask for is one CU's 160 KiB less that (hipFuncSetAttribute refuses more with an error, not with PP_ERR_UNSUPPORTED)
constexpr size_t UDP_STATIC_LDS = 256;
constexpr size_t UDP_MAX_DYNAMIC_LDS = (size_t)160 * 1024 - UDP_STATIC_LDS;

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

__device__ __forceinline__ UdpGeom udp_geom(int H, int W, int R, int phased, int shift) {
    UdpGeom g;
    g.H = H;
    g.W = W;
    g.HW = H * W;
    g.PA = (W + 2 * R) | 1;
    g.qy = UDP_THREADS / W;
    g.rx = UDP_THREADS - g.qy * W;
    g.phased = phased;
    g.shift = shift;
    return g;
}

struct UdpStat {
    float omax;  // maximum of the averaged map (the score)
    int oidx;    // its first flat index
    float bmax;  // maximum of the blurred map
    bool bad;    // a non-finite input value
};

// What a thread knows once it has put its pixels of the averaged map into A: the best of them, and whether one of its inputs was
// not finite.
struct UdpFill {
    UdpBest best;
    bool bad;
};

// Blurs the averaged map in A (pitch PA, data from column R) into A again through Bf ((H + 2 R) rows of W, R zero rows either end)
// and returns the two maxima. The zero halos of A and Bf are the caller's; they are never written here.
// RT >= 0: the radius at compile time, taps from the kernel arguments (SGPRs), loops unrolled - the two kernel sizes the codec is used
// with (11 for sigma 2, 17 for sigma 3). RT < 0: any radius 0 .. 9 at run time, taps from LDS (`tl`, one broadcast read per tap). Both
// forms sum in the same order.
template <int RT>
__device__ __forceinline__ UdpStat udp_blur(UdpFill f, const UdpGeom& g, float* __restrict__ A, float* __restrict__ Bf,
                                            float* __restrict__ scr, const UdpTaps& taps, int R) {
    const int tid = threadIdx.x;
    const float* tl = scr + UDP_TAPS_AT;
    const int W = g.W, HW = g.HW, PA = g.PA;
    UdpStat st;
    st.bad = __syncthreads_or(f.bad) != 0;
    const UdpBest best = udp_block_argmax(f.best, scr);  // (its barriers also publish A)
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

// The taps of a runtime radius into LDS and the zero halos: the columns of A either side of the map, the R rows of Bf above and
// below it (`bf_rows` false: the caller zeroes those itself, its Bf shares LDS with something still in use).
template <int RT>
__device__ __forceinline__ void udp_prepare(const UdpGeom& g, float* A, float* Bf, float* scr, const UdpTaps& taps, int R, bool bf_rows) {
    const int tid = threadIdx.x;
    if constexpr (RT < 0) {  // the taps into LDS (constant indices: the argument block is not indexed at run time)
#pragma unroll
        for (int j = 0; j <= 2 * UDP_MAX_R; ++j)
            if (tid == j) scr[UDP_TAPS_AT + j] = taps.t[j];
    }
    const int nh = g.PA - g.W;
    for (int i = tid; i < g.H * nh; i += UDP_THREADS) {
        const int y = i / nh, c = i - y * nh;
        A[y * g.PA + (c < R ? c : g.W + c)] = 0.f;
    }
    if (bf_rows)
        for (int i = tid; i < R * g.W; i += UDP_THREADS) {
            Bf[i] = 0.f;
            Bf[(g.H + R) * g.W + i] = 0.f;
        }
}

// Everything from the averaged map on, for the workgroup of (crop, keypoint) bk = (b, k). `fill(kk, avg_dst)` puts the averaged
// map of keypoint kk of the same crop into A (and, where avg_dst is given, there) and returns the calling thread's UdpFill; it is
// called for k and, for a map whose maximum is <= 0, for the keypoint before it.
//
// The reference's quirk is kept: a map whose maximum is <= 0 has loc = (-1, -1), and the flat index of refinement.py:137-145
// then reads three of its seven points from the tail of the PREVIOUS keypoint's padded log map (keypoint K - 1 for k = 0:
// a negative index). Such a workgroup blurs that neighbour map as well, in the same LDS, and takes the two pixels it needs.
template <int RT, class Fill>
__device__ __forceinline__ void udp_dark_decode(Fill&& fill, int bk, int k, int K, const UdpGeom& g, float* __restrict__ A,
                                                float* __restrict__ Bf, float* __restrict__ scr, const UdpTaps& taps, int R,
                                                double in_w, double in_h, float* __restrict__ avg_dst,
                                                float* __restrict__ locs, double* __restrict__ keypoints,
                                                float* __restrict__ scores) {
    const int tid = threadIdx.x;
    const int H = g.H, W = g.W;
    const UdpStat st = udp_blur<RT>(fill(k, avg_dst), g, A, Bf, scr, taps, R);

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
        __syncthreads();  // every thread has read pixel (0, 0)
        const UdpStat sn = udp_blur<RT>(fill(kn, nullptr), g, A, Bf, scr, taps, R);
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

// cv2.getGaussianKernel for sigma <= 0: sigma from the kernel size, factors normalised in double, rounded to fp32
inline UdpTaps udp_gaussian_taps(int blur_kernel_size) {
    UdpTaps taps;
    const int r = (blur_kernel_size - 1) / 2;
    const double sigma = 0.3 * ((blur_kernel_size - 1) * 0.5 - 1.0) + 0.8;
    double e[2 * UDP_MAX_R + 1], sum = 0.0;
    for (int j = 0; j <= 2 * r; ++j) {
        const double t = (double)(j - r);
        e[j] = std::exp(-0.5 * t * t / (sigma * sigma));
        sum += e[j];
    }
    for (int j = 0; j <= 2 * UDP_MAX_R; ++j) taps.t[j] = j <= 2 * r ? (float)(e[j] / sum) : 0.f;
    return taps;
}

}  // namespace pp
