// The pieces every attention kernel of the ViT backbone is put together from (gfx950 only): pp_attention.hip (192 / 432 tokens x head dim
// 32 / 64, bf16, fp32 and split-fp16), pp_attention_hd80.hip (192 x 80), pp_attention_dma.hip (432 tokens, split-fp16, K / V by LDS-DMA) and
// the block id of pp_qkv_attn_split.hip. Everything here is forced inline and compiles to the instructions the kernel would otherwise spell out
// by hand (scripts/gfx950_isa.py compares the assembly of two trees); a kernel differs from its neighbours in its LDS layout, its key walk and
// its launch bounds, which stay with the kernel.
//
// The common scheme: S^T = K Q^T with K as the MFMA "A" operand, so that a lane (fr = lane & 15, fg = lane >> 4) ends up with the four
// consecutive keys 16 kt + 4 fg + (0..3) of ONE query (16 qt + fr) in fragment kt. The softmax row reduction is then in-register work plus
// two hops over the four lane groups of a query (lane ^ 16, lane ^ 32), and P in that layout IS the "B" operand of O^T = V^T P^T (the key
// order inside a K-block is a permutation shared by both operands): P never leaves registers. V is staged transposed, [head dim][keys].
//
// Not here, on purpose: the in-layer attention of pp_mlp.hip (pp_vit_layer: its loops are interleaved with ATT_DBG ablations and another
// software pipeline); the score / softmax / P V phase of pp_qkv_attn_split.hip; the permlane-swap row maximum, the ballot-skipped rescale,
// the split_pair packing and the transposing V^T reads of attention_split_dma_kernel, which are deliberately of another shape than the forms
// below. attention_hd80_kernel is not a padded instantiation of attention_kernel, and attention_split_stream_kernel (attn_dma = 0) stays.
#pragma once
#include "pp_common.h"
#include "pp_device.h"
#include "pp_split.h"

namespace pp {
namespace att {

// softmax runs on exp2: the kernels take scale * log2(e), exp(s scale - m scale) = exp2(s scale_log2e - m scale_log2e)
constexpr float kLog2e = 1.44269504088896340736f;

// ---- XCD-aware block id: the hardware round-robins consecutive block ids over the 8 XCDs; remapped, a run of nblk / 8 consecutive ids -
// the heads (and query quarters) of one sequence, adjacent columns of the same qkv rows - lands on one XCD and shares its L2. Grids that
// are no multiple of 8 keep the plain id.
__device__ __forceinline__ int xcd_block_id() {
    int id = blockIdx.x;
    const int nblk = gridDim.x;
    if ((nblk & 7) == 0) id = (id & 7) * (nblk >> 3) + (id >> 3);
    return id;
}

// ---- one 16-byte chunk of K per lane, the MFMA chosen by the operand type (bf16 -> v_mfma_f32_16x16x32_bf16, fp32 -> four
// v_mfma_f32_16x16x4_f32); the split-fp16 kernels call split_mma (pp_split.h)
__device__ __forceinline__ f32x4 mma(const u32x4& a, const u32x4& b, f32x4 c, __bf16) { return mma_bf16(a, b, c); }
__device__ __forceinline__ f32x4 mma(const u32x4& a, const u32x4& b, f32x4 c, float) { return mma_f32(a, b, c); }

// ---- softmax (statistics in fp32 in every precision)
// the closing step of every form: sum <- the sum over the four lane groups of a query (lane ^ 16, lane ^ 32)
__device__ __forceinline__ void quad_sum(float& sum) {
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
}

// exp-and-sum step for one fragment (four keys of this lane's query): s <- 2^(s scale_log2e - mb), sum += the four. mb = (row maximum) *
// scale_log2e, so the argument is <= 0: raw v_exp_f32 (1 ulp), no range reduction. In the online forms the caller skips (and zeroes) the
// fragments of padded key tiles, and adds the lanes of a query up once, at the end (quad_sum).
__device__ __forceinline__ void exp_sum(f32x4& s, float scale_log2e, float mb, float& sum) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], scale_log2e, -mb));
        s[i] = p;
        sum += p;
    }
}

// single pass over the NT key tiles of this lane's query (the whole score row is in registers: no rescaling): s <- p, fragments from NT on
// zeroed; returns the row sum
template <int NT, int N>
__device__ __forceinline__ float softmax_row(f32x4 (&s)[N], float scale_log2e) {
    static_assert(NT <= N, "fragments of the row");
    float mx = -__builtin_inff();
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) mx = fmaxf(mx, s[kt][i]);
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mb = mx * scale_log2e;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) exp_sum(s[kt], scale_log2e, mb, sum);
    quad_sum(sum);
#pragma unroll
    for (int kt = NT; kt < N; ++kt) s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    return sum;
}

// ---- O^T += V^T P^T, one MFMA K-block of one d tile: c += V^T[16 dt + fr][keys] P^T. V^T rows lie at a pitch of SPV = (padded keys) + 8
// elements, 8 * odd, so the 16 rows of a fragment read fall on different banks; vrow points at key 4 fg of the block in row 16 dt + fr.
// bf16, K = 32 = one PAIR of key tiles: keys 4 fg + i from p0 and 16 + 4 fg + i from p1 on both operands
__device__ __forceinline__ bf16x8 pack_p(const f32x4& p0, const f32x4& p1) {
    return bf16x8{(__bf16)p0[0], (__bf16)p0[1], (__bf16)p0[2], (__bf16)p0[3], (__bf16)p1[0], (__bf16)p1[1], (__bf16)p1[2], (__bf16)p1[3]};
}
__device__ __forceinline__ f32x4 pv_mma(const __bf16* vrow, const bf16x8& pf, f32x4 c) {
    const u32x2 lo = *reinterpret_cast<const u32x2*>(vrow);
    const u32x2 hi = *reinterpret_cast<const u32x2*>(vrow + 16);
    const u32x4 vf = {lo[0], lo[1], hi[0], hi[1]};
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vf), pf, c, 0, 0, 0);
}
// split-fp16, the same pair of key tiles: the eight probabilities are split in registers (p in [0, 1]: a subnormal low half is an absolute
// error below 2^-25); the kernels read V^T from a hi and a lo plane of the same layout and call split_mma (three MFMAs)
__device__ __forceinline__ void split_p(const f32x4& p0, const f32x4& p1, f16x8& ph, f16x8& pl) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ph[j] = split_hi(p0[j]);
        pl[j] = split_lo(p0[j], ph[j]);
        ph[4 + j] = split_hi(p1[j]);
        pl[4 + j] = split_lo(p1[j], ph[4 + j]);
    }
}

// ---- Q fragments straight from global memory to registers (each is used by exactly one wave): lane (query fr, chunk 4 g + fg) of K-block g,
// chunks of CH elements. (Parameters by reference here and below: a by-value scalar is `noundef` to the optimiser, which then drops
// freezes the hand-written form keeps, and the schedule moves.)
template <int CH, int NG, typename T>
__device__ __forceinline__ void load_q(u32x4 (&qf)[NG], const T* const& qrow, const int& fg) {
#pragma unroll
    for (int g = 0; g < NG; ++g) qf[g] = *reinterpret_cast<const u32x4*>(qrow + (g * 4 + fg) * CH);
}
// split-fp16: hi and lo chunk fg of each of the row's NB 128-byte blocks
template <int NB>
__device__ __forceinline__ void load_q_split(f16x8 (&qh)[NB], f16x8 (&ql)[NB], const char* const& qrow, const int& fg) {
#pragma unroll
    for (int g = 0; g < NB; ++g) {
        qh[g] = *reinterpret_cast<const f16x8*>(qrow + g * 128 + fg * 16);
        ql[g] = *reinterpret_cast<const f16x8*>(qrow + g * 128 + 64 + fg * 16);
    }
}

// ---- normalise and store: four consecutive d of one query, scaled by 1 / (row sum), as bf16 or fp32 (split-fp16 rows: split_store4)
template <typename T>
__device__ __forceinline__ void store4(T* dst, f32x4 v) {
    if constexpr (sizeof(T) == 2) {
        const bf16x4 ov = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        *reinterpret_cast<bf16x4*>(dst) = ov;
    } else {
        *reinterpret_cast<f32x4*>(dst) = v;
    }
}

// ---- host: raise the kernel's dynamic LDS limit (above 64 KiB it must be asked for), launch, check. The launch is tallied under the
// CALLER's source file (pp_launch_count): a stream converts to LaunchStream at the call site, where __builtin_FILE() is evaluated.
struct LaunchStream {
    hipStream_t stream;
    const char* file;
    LaunchStream(hipStream_t s, const char* f = __builtin_FILE()) : stream(s), file(f) {}
};
template <typename... P, typename... A>
int launch_with_lds(void (*kernel)(P...), dim3 grid, dim3 threads, size_t lds_bytes, LaunchStream at, A... args) {
    PP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(kernel, grid, threads, lds_bytes, at.stream, static_cast<P>(args)...);
    count_launch(at.file);  // PP_LAUNCH_CHECK, for the caller's file instead of this header
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

}  // namespace att
}  // namespace pp
