// Multi-head self-attention at 192 tokens x head dim 80 (ViT-H: 1280 wide, 16 heads) for gfx950. The kernels of
// pp_attention.hip count a head row in whole MFMA K-blocks (32 elements of the 2-byte formats, one 128-byte block of the
// split-fp16 format); 80 = 2.5 of them. Here the q . k contraction runs over the head row ZERO-PADDED TO 96 (three
// K-blocks; fp32, whose K-block is 16 elements, needs no padding: five blocks) - 1.5x the score MFMAs of head dim 64 -
// while P V and the output keep the true 80 columns (five 16-wide d tiles), so QK^T + PV together cost 1.375x head dim 64.
//
// The padding exists in LDS and in registers only. A head's 80 values are ten 16-byte chunks (twenty in fp32; ten hi + ten lo
// in the split format); the chunks 10 and 11 of the padded row are written as zeros and the q fragment of a lane that owns
// one of them is set to zero WITHOUT a load: behind a head's 80 values lie the next head, the k / v parts of the row, the next
// token and finally the end of the tensor - none of it is read.
//
// Split-fp16 addressing: the format blocks a tensor by its FLAT element index (block = idx >> 5, pp_split.h). At ViT-H E = 1280 and
// 3 E are multiples of 32 and rows start on 128-byte blocks, but a head starts at element 80 h, i.e. in the MIDDLE of a block for
// odd h (80 h mod 32 = 16); with an odd head count (3 E = 240 heads is then a multiple of 16 only) so does every other row. Every
// 8-element chunk still lies inside one block (row * 3 E + 80 h + 8 j is a multiple of 8): chunk j of head h is the 16 bytes at
// split_addr(qkv, row * 3 E + 80 h + 8 j), its lo halves 64 bytes on; the kernel addresses every chunk that way.
// In LDS the row is re-blocked from the head's own origin (block b = j / 4: hi chunks 8 b .. 8 b + 3, lo chunks 8 b + 4 .. 8 b + 7),
// which is the layout the score loop of attention_split_kernel reads.
//
// Everything else is the single-pass form of pp_attention.hip: one 256-thread workgroup per (sequence, head), K row-major and
// V transposed in LDS, S^T = K Q^T so that P stays in registers as the B operand of O^T = V^T P^T, softmax statistics in fp32 -
// block id, MFMA overloads, softmax row, packing of P, the bf16 P V step, the bf16 / fp32 store and the launch from pp_attention_core.h.
#include "pp_attention_core.h"

namespace pp {
namespace {

constexpr int H80_THREADS = 256;
constexpr int H80_HD = 80;           // head dim
constexpr int H80_NT = 12;           // 16-token tiles: 192 tokens
constexpr int H80_S = H80_NT * 16;
constexpr int H80_SPV = H80_S + 8;   // V^T row pitch (elements): 8 * odd -> conflict-free reads
constexpr int H80_DT = H80_HD / 16;  // output d tiles
constexpr int H80_QPW = H80_NT / (H80_THREADS / 64);  // query tiles per wave

// ---------------------------------------------------------------------------------------------
// PP_PREC_BF16 (K-block 32: contraction padded to 96) and PP_PREC_F32 (K-block 16: 80, no padding)
template <typename T>
struct H80Cfg {
    static constexpr int CH = 16 / (int)sizeof(T);                  // elements per 16-byte chunk
    static constexpr int KB = 4 * CH;                               // elements per MFMA K-block
    static constexpr int KD = (H80_HD + KB - 1) / KB * KB;          // contraction depth: 96 / 80
    static constexpr int RCG = H80_HD / CH;                         // chunks of a head row in memory: 10 / 20
    static constexpr int RCL = KD / CH;                             // chunks of a K row in LDS: 12 / 20
    static constexpr int NG = KD / KB;                              // K-blocks: 3 / 5
    static constexpr size_t K_BYTES = (size_t)H80_S * KD * sizeof(T);
    static constexpr size_t V_BYTES = (size_t)H80_HD * H80_SPV * sizeof(T);
    static constexpr size_t LDS = K_BYTES + V_BYTES;
};

template <typename T>
__global__ __launch_bounds__(H80_THREADS, (sizeof(T) == 2 ? 2 : 1)) void attention_hd80_kernel(const T* __restrict__ qkv, T* __restrict__ out, int n_seq, int heads,
                                                                      float scale_log2e) {
    using C = H80Cfg<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // [S][RCL chunks], chunk c of row r at c ^ ((r >> 2) & 3): the row pitch is 48 (bf16) / 80 (fp32) dwords, so the rows r, r + 4, r + 8, r + 12 of a
    // fragment read start on one bank; the swizzle moves them to four different 16-byte columns of it
    char* Ks = smem;
    T* Vt = reinterpret_cast<T*>(smem + C::K_BYTES);  // [HD][SPV]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int id = att::xcd_block_id();
    const int seq = id / heads, head = id - seq * heads;
    const int E = heads * H80_HD;
    const size_t row_stride = (size_t)3 * E;
    const T* base = qkv + (size_t)seq * H80_S * row_stride + (size_t)head * H80_HD;

    // ---- Q fragments of this wave's query tiles; a lane whose chunk lies in the padding holds zeros and loads nothing
    u32x4 qf_all[H80_QPW][C::NG];
#pragma unroll
    for (int t = 0; t < H80_QPW; ++t) {
        const T* qrow = base + (size_t)((wave + t * (H80_THREADS / 64)) * 16 + fr) * row_stride;
#pragma unroll
        for (int g = 0; g < C::NG; ++g) {
            u32x4 q = {0, 0, 0, 0};
            if (g * 4 + fg < C::RCG) q = *reinterpret_cast<const u32x4*>(qrow + (g * 4 + fg) * C::CH);
            qf_all[t][g] = q;
        }
    }

    // ---- stage K (row-major, padded chunks zero) and V (transposed)
    for (int i = tid; i < H80_S * C::RCL; i += H80_THREADS) {
        const int r = i / C::RCL, c = i - r * C::RCL;
        u32x4 kv = {0, 0, 0, 0};
        if (c < C::RCG) {
            kv = *reinterpret_cast<const u32x4*>(base + (size_t)r * row_stride + E + c * C::CH);
            const u32x4 vv = *reinterpret_cast<const u32x4*>(base + (size_t)r * row_stride + 2 * E + c * C::CH);
            T ve[C::CH];
            *reinterpret_cast<u32x4*>(ve) = vv;
#pragma unroll
            for (int j = 0; j < C::CH; ++j) Vt[(c * C::CH + j) * H80_SPV + r] = ve[j];
        }
        *reinterpret_cast<u32x4*>(Ks + ((size_t)r * C::RCL + (c ^ ((r >> 2) & 3))) * 16) = kv;
    }
    __syncthreads();

#pragma unroll
    for (int t = 0; t < H80_QPW; ++t) {
        const int qt = wave + t * (H80_THREADS / 64);
        // ---- scores: s[kt][i] = q . k for key 16 kt + 4 fg + i
        f32x4 s[H80_NT];
#pragma unroll
        for (int kt = 0; kt < H80_NT; ++kt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int r = kt * 16 + fr;
#pragma unroll
            for (int g = 0; g < C::NG; ++g) {
                const u32x4 kf = *reinterpret_cast<const u32x4*>(Ks + ((size_t)r * C::RCL + ((g * 4 + fg) ^ ((r >> 2) & 3))) * 16);
                acc = att::mma(kf, qf_all[t][g], acc, T{});
            }
            s[kt] = acc;
        }
        const float sum = att::softmax_row<H80_NT>(s, scale_log2e);

        // ---- O^T = V^T P^T over the 80 true columns
        f32x4 o[H80_DT];
#pragma unroll
        for (int dt = 0; dt < H80_DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int blk = 0; blk < H80_NT / 2; ++blk) {
                const bf16x8 pf = att::pack_p(s[2 * blk], s[2 * blk + 1]);
#pragma unroll
                for (int dt = 0; dt < H80_DT; ++dt) o[dt] = att::pv_mma(Vt + (dt * 16 + fr) * H80_SPV + blk * 32 + 4 * fg, pf, o[dt]);
            }
        } else {
#pragma unroll
            for (int kt = 0; kt < H80_NT; ++kt) {
                const u32x4 pf = __builtin_bit_cast(u32x4, s[kt]);
#pragma unroll
                for (int dt = 0; dt < H80_DT; ++dt) {
                    const u32x4 vf = *reinterpret_cast<const u32x4*>(Vt + (dt * 16 + fr) * H80_SPV + kt * 16 + 4 * fg);
                    o[dt] = att::mma(vf, pf, o[dt], T{});
                }
            }
        }
        // ---- normalise and store: lane holds d = 16 dt + 4 fg + (0..3) of query 16 qt + fr
        const float inv = 1.0f / sum;
        T* orow = out + ((size_t)seq * H80_S + qt * 16 + fr) * E + head * H80_HD;
#pragma unroll
        for (int dt = 0; dt < H80_DT; ++dt) att::store4(orow + dt * 16 + 4 * fg, o[dt] * inv);
        // one query tile's fragments at a time: without it the K reads of all three tiles are hoisted to the top (256 registers, one workgroup
        // per CU: 115 us per bf16 launch at n_seq 128 x 16 heads); with it 149 registers and the two workgroups a CU's LDS holds (69 KiB each)
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---------------------------------------------------------------------------------------------
// PP_PREC_F16X3: split-fp16 operands, three fp16 MFMAs per product (pp_split.h), the row re-blocked to three 128-byte blocks
constexpr int H80_NB = 3;                  // 128-byte blocks of the padded head row
constexpr int H80_RC = H80_NB * 8;         // 16-byte chunks per K row in LDS
constexpr int H80_JC = H80_HD / 8;         // 8-element chunks of the true head row: 10
constexpr size_t H80_SPLIT_K_BYTES = (size_t)H80_S * H80_RC * 16;
constexpr size_t H80_SPLIT_V_BYTES = (size_t)2 * H80_HD * H80_SPV * 2;
constexpr size_t H80_SPLIT_LDS = H80_SPLIT_K_BYTES + H80_SPLIT_V_BYTES;

__global__ __launch_bounds__(H80_THREADS, 1) void attention_hd80_split_kernel(const char* __restrict__ qkv, char* __restrict__ out, int n_seq,
                                                                             int heads, float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                                                             // [S][RC chunks], chunk c of row r at c ^ (r & 7)
    _Float16* Vh = reinterpret_cast<_Float16*>(smem + H80_SPLIT_K_BYTES);        // [HD][SPV] hi halves of V^T
    _Float16* Vl = Vh + H80_HD * H80_SPV;                                        // [HD][SPV] lo halves
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int id = att::xcd_block_id();
    const int seq = id / heads, head = id - seq * heads;
    const int E = heads * H80_HD;
    // the hi halves of chunk j (0 .. 9) of this head in part 0 / 1 / 2 (q / k / v) of token row r of this sequence: flat element index
    auto chunk = [&](int r, int part, int j) {
        return split_addr(qkv, ((size_t)seq * H80_S + r) * 3 * E + (size_t)part * E + head * H80_HD + j * 8);
    };

    f16x8 qh_all[H80_QPW][H80_NB], ql_all[H80_QPW][H80_NB];
#pragma unroll
    for (int t = 0; t < H80_QPW; ++t) {
        const int qr = (wave + t * (H80_THREADS / 64)) * 16 + fr;
#pragma unroll
        for (int g = 0; g < H80_NB; ++g) {
            const int j = g * 4 + fg;
            u32x4 h = {0, 0, 0, 0}, l = {0, 0, 0, 0};
            if (j < H80_JC) {  // (the padding loads nothing)
                const char* p = chunk(qr, 0, j);
                h = *reinterpret_cast<const u32x4*>(p);
                l = *reinterpret_cast<const u32x4*>(p + 64);
            }
            qh_all[t][g] = __builtin_bit_cast(f16x8, h);
            ql_all[t][g] = __builtin_bit_cast(f16x8, l);
        }
    }

    // ---- stage K (re-blocked, swizzled) and V^T (hi / lo planes): one (key, 8-element chunk) per iteration
    for (int i = tid; i < H80_S * H80_JC; i += H80_THREADS) {
        const int r = i / H80_JC, j = i - r * H80_JC;
        const char* pk = chunk(r, 1, j);
        const char* pv = chunk(r, 2, j);
        const u32x4 kh = *reinterpret_cast<const u32x4*>(pk), kl = *reinterpret_cast<const u32x4*>(pk + 64);
        const u32x4 vh = *reinterpret_cast<const u32x4*>(pv), vl = *reinterpret_cast<const u32x4*>(pv + 64);
        const int c = (j >> 2) * 8 + (j & 3);
        *reinterpret_cast<u32x4*>(Ks + ((size_t)r * H80_RC + (c ^ (r & 7))) * 16) = kh;
        *reinterpret_cast<u32x4*>(Ks + ((size_t)r * H80_RC + ((c + 4) ^ (r & 7))) * 16) = kl;
        const f16x8 eh = __builtin_bit_cast(f16x8, vh), el = __builtin_bit_cast(f16x8, vl);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            Vh[(j * 8 + k) * H80_SPV + r] = eh[k];
            Vl[(j * 8 + k) * H80_SPV + r] = el[k];
        }
    }
    // the padding of the third block: chunks 10 and 11, hi and lo, of every key row
    for (int i = tid; i < H80_S * 4; i += H80_THREADS) {
        const int r = i >> 2, c = 16 + 2 + (i & 1) + ((i & 2) ? 4 : 0);
        *reinterpret_cast<u32x4*>(Ks + ((size_t)r * H80_RC + (c ^ (r & 7))) * 16) = u32x4{0, 0, 0, 0};
    }
    __syncthreads();

#pragma unroll
    for (int t = 0; t < H80_QPW; ++t) {
        const int qt = wave + t * (H80_THREADS / 64);
        // ---- scores: s[kt][i] = q . k for key 16 kt + 4 fg + i
        f32x4 s[H80_NT];
#pragma unroll
        for (int kt = 0; kt < H80_NT; ++kt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int r = kt * 16 + fr;
#pragma unroll
            for (int g = 0; g < H80_NB; ++g) {
                const f16x8 kh = *reinterpret_cast<const f16x8*>(Ks + ((size_t)r * H80_RC + ((g * 8 + fg) ^ (r & 7))) * 16);
                const f16x8 kl = *reinterpret_cast<const f16x8*>(Ks + ((size_t)r * H80_RC + ((g * 8 + 4 + fg) ^ (r & 7))) * 16);
                acc = split_mma(kh, kl, qh_all[t][g], ql_all[t][g], acc);
            }
            s[kt] = acc;
        }
        const float sum = att::softmax_row<H80_NT>(s, scale_log2e);

        // ---- O^T = V^T P^T over the 80 true columns; p in [0, 1] is split in registers
        f32x4 o[H80_DT];
#pragma unroll
        for (int dt = 0; dt < H80_DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int blk = 0; blk < H80_NT / 2; ++blk) {
            f16x8 ph, pl;
            att::split_p(s[2 * blk], s[2 * blk + 1], ph, pl);
#pragma unroll
            for (int dt = 0; dt < H80_DT; ++dt) {
                const int off = (dt * 16 + fr) * H80_SPV + blk * 32 + 4 * fg;
                const u32x2 h0 = *reinterpret_cast<const u32x2*>(Vh + off), h1 = *reinterpret_cast<const u32x2*>(Vh + off + 16);
                const u32x2 l0 = *reinterpret_cast<const u32x2*>(Vl + off), l1 = *reinterpret_cast<const u32x2*>(Vl + off + 16);
                const u32x4 vh = {h0[0], h0[1], h1[0], h1[1]}, vl = {l0[0], l0[1], l1[0], l1[1]};
                o[dt] = split_mma(__builtin_bit_cast(f16x8, vh), __builtin_bit_cast(f16x8, vl), ph, pl, o[dt]);
            }
        }
        // ---- normalise and store: lane holds d = 16 dt + 4 fg + (0..3) of query 16 qt + fr (four elements never straddle a block)
        const float inv = 1.0f / sum;
        const size_t oidx = ((size_t)seq * H80_S + qt * 16 + fr) * E + head * H80_HD;
#pragma unroll
        for (int dt = 0; dt < H80_DT; ++dt) split_store4(out, oidx + dt * 16 + 4 * fg, o[dt] * inv);
    }
}

template <typename T>
int launch_hd80(const void* qkv, void* out, int n_seq, int heads, float scale, hipStream_t s) {
    using C = H80Cfg<T>;
    static_assert(C::LDS <= 160 * 1024, "K/V of one head must fit in one CU's LDS");
    return att::launch_with_lds(attention_hd80_kernel<T>, dim3(n_seq * heads), dim3(H80_THREADS), C::LDS, s, reinterpret_cast<const T*>(qkv),
                                reinterpret_cast<T*>(out), n_seq, heads, scale * att::kLog2e);
}

}  // namespace

// 192 tokens x head dim 80 in the three precisions (dispatched from pp_attention)
int attention_hd80(int prec, const void* qkv, void* out, int n_seq, int heads, float scale, hipStream_t s) {
    if (prec == PP_PREC_BF16) return launch_hd80<__bf16>(qkv, out, n_seq, heads, scale, s);
    if (prec == PP_PREC_F32) return launch_hd80<float>(qkv, out, n_seq, heads, scale, s);
    static_assert(H80_SPLIT_LDS <= 160 * 1024, "K/V of one head must fit in one CU's LDS");
    return att::launch_with_lds(attention_hd80_split_kernel, dim3(n_seq * heads), dim3(H80_THREADS), H80_SPLIT_LDS, s,
                                reinterpret_cast<const char*>(qkv), reinterpret_cast<char*>(out), n_seq, heads, scale * att::kLog2e);
}

}  // namespace pp
