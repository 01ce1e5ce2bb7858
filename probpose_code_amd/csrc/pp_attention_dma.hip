// Multi-head self-attention for 432-token sequences (384x288 crops: BASELINE config 4) in the parity precision (PP_PREC_F16X3,
// split-fp16 operands): softmax(q k^T * scale) v per (sequence, head), from the packed (M, 3E) qkv tensor of the split format.
// (mmpretrain MultiheadAttention.forward [3P]: scaled dot-product attention on qkv.reshape(B, N, 3, H, hd); call site
// mmpose/models/pose_estimators/base.py:206; nearest reference config td-hm_ViTPose-base_8xb64-210e_coco-256x192.py:46-61.)
//
// Round 2's kernel for this shape (pp_attention.hip, attention_split_stream_kernel) stages K and V^T of half the keys through
// registers - V with a 2-byte transposing scatter - into 115 KiB of LDS: one workgroup per CU, 337 us per ViT-B layer at bs 32
// for 54 us of MFMA issue. Here K and V stay ROW-MAJOR by key and come in by LDS-DMA:
//   * a workgroup = (sequence, head, query quarter): seven waves, one 16-query tile each (27 tiles = 7 + 7 + 7 + 6); q
//     fragments from global memory once;
//   * the keys stream through a ring of four 32-key stages: per stage K and V as HD / 32 sub-tiles of [32 keys][128 B] (the
//     raw split blocks: 32 hi halves | 32 lo halves, 16-byte chunks XOR-swizzled by key & 7 at the source) = 16 KiB at head
//     dim 64; the stages go in PAIRS (one barrier, one running-maximum update and one rescale of O per 64 keys: 149 -> 145 us),
//     the next pair requested while this one is worked on; 64 KiB of LDS and < 128 registers: two workgroups per CU;
//   * S^T = K Q^T (a query's scores lane-local), online softmax over the stages (running maximum / sum, O rescaled when the
//     maximum moves), P split in registers, O^T = V^T P^T with the V^T fragments read by ds_read_b64_tr_b16 - the gfx950
//     transposing LDS read (within 16 lanes, lane 4 r + q supplies the address of four consecutive halves M[r][4 q ..], lane i
//     receives M[0..3][i]: four keys of one head dim per lane) - for the hi and the lo plane; no register staging, no scatter.
//
// Round 6, measured and NOT adopted (the attempt is kept as scripts/r06/attempts/pp_attention_dma_two_tiles_ring8.hip.txt; ViT-B 384 x 288, bs 64
// + flip, attention ms per step): this kernel 3.55; TWO query tiles per wave on every K / V^T fragment (query halves, 146 registers, or held to
// 128 with six spills) 3.77 / 3.79; the same with a ring of eight stages, three pairs requested ahead (128 KiB: one workgroup per CU) 4.05 /
// 4.72. Neither the LDS reads nor the DMA latency is what the 42 % matrix-pipe share waits for: per wave and 64 keys the online softmax costs
// about as many issue cycles (16 exp2 at quarter rate, the maxima, eight split_pair: ~1.7 k) as the 48 MFMAs do (~1.5 k), and they belong to
// the same wave - the pipe idles while its wave does arithmetic unless ANOTHER wave of the SIMD has MFMAs ready, which is what two workgroups
// per CU (14 waves) provide and what both attempts gave up.
//
// Block id, the exp-and-sum step, the closing row sum and the launch are pp_attention_core.h; the permlane-swap row maximum, the
// ballot-skipped rescale, the split_pair packing and the transposing V^T reads below are this kernel's own.
#include "pp_attention_core.h"

namespace pp {
namespace adma {

constexpr int S = 432, NT = S / 16, QSPLIT = 4, TPW = (NT + QSPLIT - 1) / QSPLIT, THREADS = 64 * TPW;  // 7 waves
constexpr int SK = 32;                         // keys per stage
constexpr int NSTG = (S + SK - 1) / SK;        // 14 stages (the last one holds 16 keys)
constexpr int RING = 4;

template <int HD>
struct Cfg {
    static constexpr int NB = HD / 32;                   // 128-byte blocks per key and operand
    static constexpr int SUB = SK * 128;                 // one sub-tile: 32 keys x 128 B
    static constexpr int STAGE = 2 * NB * SUB;           // K sub-tiles, then V sub-tiles
    static constexpr int PIECES = STAGE / 1024;          // DMA instructions per stage (8 keys x 128 B each)
    static constexpr int LDS = RING * STAGE;
    static constexpr int DT = HD / 16;
};

template <int HD>
__global__ __launch_bounds__(THREADS, 4) void attention_split_dma_kernel(const char* __restrict__ qkv, char* __restrict__ out, int n_seq,
                                                                         int heads, unsigned qkv_bytes, float scale_log2e) {
    using C = Cfg<HD>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;

    int id = att::xcd_block_id();  // the query quarters and heads of a sequence on one XCD
    const int qs = id % QSPLIT;
    id /= QSPLIT;
    const int seq = id / heads, head = id - seq * heads;
    const int E = heads * HD;
    const unsigned row_bytes = (unsigned)(3 * E * 4);
    const unsigned base = (unsigned)(seq * S) * row_bytes + (unsigned)(head * HD * 4);  // q block 0 of the sequence's first token
    const int qt = qs * TPW + wv;       // this wave's query tile
    const bool live = qt < NT;          // (the last quarter has six tiles: its seventh wave only helps with the DMA)

    // ---- DMA: piece j of a stage = sub-tile j / 4 (K blocks 0 .. NB - 1, then V blocks), keys 8 (j % 4) .. + 7; lane (l = lane >> 3,
    // pc = lane & 7) fetches the logical 16-byte chunk pc ^ l of key 8 (j % 4) + l
    const __amdgpu_buffer_rsrc_t rsrc = buffer_rsrc(qkv, qkv_bytes);
    const int d_l = lane >> 3;
    const unsigned d_sw = (unsigned)(((lane & 7) ^ d_l) << 4);
    auto issue_stage = [&](int st) {
        char* dst = smem + (st & (RING - 1)) * C::STAGE;
#pragma unroll
        for (int u = 0; u < (C::PIECES + TPW - 1) / TPW; ++u) {
            const int j = wv + u * TPW;
            if (j < C::PIECES) {
                const int sub = j >> 2, kq = j & 3;
                const int which = sub / C::NB, blk = sub - which * C::NB;  // 0 = K, 1 = V
                const unsigned vo = base + (unsigned)(st * SK + kq * 8 + d_l) * row_bytes + (unsigned)((1 + which) * E * 4 + blk * 128) + d_sw;
                dma16(rsrc, dst + j * 1024, vo);
            }
        }
    };

    // ---- q fragments of this wave's tile: lane (query fr, chunk fg) of block g
    f16x8 qh[C::NB], ql[C::NB];
    {
        const char* qrow = qkv + base + (size_t)((live ? qt : 0) * 16 + fr) * row_bytes;
#pragma unroll
        for (int g = 0; g < C::NB; ++g) {  // (att::load_q_split, spelled out: shared, it moves this kernel's schedule)
            qh[g] = *reinterpret_cast<const f16x8*>(qrow + g * 128 + fg * 16);
            ql[g] = *reinterpret_cast<const f16x8*>(qrow + g * 128 + 64 + fg * 16);
        }
    }
    issue_stage(0);
    issue_stage(1);

    f32x4 o[C::DT];
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -__builtin_inff(), l_run = 0.f;

    const int sw = fr & 7;
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;  // LDS byte address of the dynamic region (0)
    // V^T fragments through the transposing read: lane fr = 4 r + q of the 16-lane group fg addresses key 4 fg + r, halves 4 q ..
    const int tr_r = fr >> 2, tr_q = fr & 3;
    const int vkey = 4 * fg + tr_r;  // (+ 16 for the second read: same key & 7)

    // Two stages (64 keys) between barriers: one running-maximum update, one rescale of O and one barrier per 48 MFMAs instead
    // of per 24. The pair p + 1 is requested at the top of pair p, into the two slots pair p - 1 has just left.
    static_assert(NSTG % 2 == 0 && RING == 4, "stage pairs on a ring of four");
    for (int pr = 0; pr < NSTG / 2; ++pr) {
        __builtin_amdgcn_sched_barrier(0);
        wait_vm<0>();                  // this wave's pieces of the pair are in (nothing younger is in flight)
        __builtin_amdgcn_s_barrier();  // every wave's pieces are in; every wave is done with pair pr - 1
        __builtin_amdgcn_sched_barrier(0);
        if (2 * pr + 2 < NSTG) {
            issue_stage(2 * pr + 2);
            issue_stage(2 * pr + 3);
        }
        if (!live) continue;
        const bool tail = pr == NSTG / 2 - 1 && (S % SK) != 0;  // the last stage holds S % 32 = 16 keys: its second key tile does not exist

        // ---- scores of the pair's four key tiles: s[kt][i] = q . k for key 64 pr + 16 kt + 4 fg + i of query fr
        f32x4 sc[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const char* Ks = smem + ((2 * pr + (kt >> 1)) & (RING - 1)) * C::STAGE;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int r = (kt & 1) * 16 + fr;
#pragma unroll
            for (int g = 0; g < C::NB; ++g) {
                const f16x8 kh = *reinterpret_cast<const f16x8*>(Ks + g * C::SUB + r * 128 + ((fg ^ sw) << 4));
                const f16x8 kl = *reinterpret_cast<const f16x8*>(Ks + g * C::SUB + r * 128 + (((4 + fg) ^ sw) << 4));
                acc = split_mma(kh, kl, qh[g], ql[g], acc);
            }
            sc[kt] = acc;
        }
        if (tail) sc[3] = f32x4{-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        // ---- online softmax
        float mx = m_run;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int i = 0; i < 4; ++i) mx = fmaxf(mx, sc[kt][i]);
        {  // max over the four lane groups of a query: the gfx950 row swaps (plain VALU) instead of two trips through the LDS queue
            const unsigned mu = __builtin_bit_cast(unsigned, mx);
            const auto s16 = __builtin_amdgcn_permlane16_swap(mu, mu, false, false);
            mx = fmaxf(__builtin_bit_cast(float, (unsigned)s16[0]), __builtin_bit_cast(float, (unsigned)s16[1]));
            const unsigned mv = __builtin_bit_cast(unsigned, mx);
            const auto s32 = __builtin_amdgcn_permlane32_swap(mv, mv, false, false);
            mx = fmaxf(__builtin_bit_cast(float, (unsigned)s32[0]), __builtin_bit_cast(float, (unsigned)s32[1]));
        }
        // (the running maximum of a query stops moving after its first few key blocks: when it has not moved for ANY query of the tile -
        //  wave-uniform - alpha is exactly 1 for every lane and the rescale of O, 17 multiplications, is skipped)
        if (__builtin_amdgcn_ballot_w64(mx != m_run) != 0) {
            const float alpha = __builtin_amdgcn_exp2f((m_run - mx) * scale_log2e);  // (first pair: exp2(-inf) = 0, nothing to rescale)
            l_run *= alpha;
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt) o[dt] *= alpha;
            m_run = mx;
        }
        const float mb = mx * scale_log2e;
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) att::exp_sum(sc[kt], scale_log2e, mb, sum);  // masked keys: exp2(-inf) = 0
        l_run += sum;  // this lane's keys only; the four lanes of a query are added up at the end
        // ---- O^T += V^T P^T, one K = 32 block per stage of the pair: keys 4 fg + i and 16 + 4 fg + i per lane on both operands
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int st = 2 * pr + h;
            f16x8 ph, pl;
            {   // (hi, lo) of the eight probabilities in 16 VALU instructions (split_pair) instead of 32
                u32x4 phu, plu;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    unsigned h_, l_;
                    split_pair(sc[2 * h][2 * j], sc[2 * h][2 * j + 1], h_, l_);
                    phu[j] = h_; plu[j] = l_;
                    split_pair(sc[2 * h + 1][2 * j], sc[2 * h + 1][2 * j + 1], h_, l_);
                    phu[2 + j] = h_; plu[2 + j] = l_;
                }
                ph = __builtin_bit_cast(f16x8, phu);
                pl = __builtin_bit_cast(f16x8, plu);
            }
            // two head-dim tiles (16 dims each) per group: eight transposing reads in flight, one wait, six MFMAs.
            // As asm: the BUILTIN carries no memory operand, so the compiler waits for every LDS-DMA in flight (vmcnt(0)) in front of
            // it - the stages ahead included. The explicit lgkmcnt(0) covers the group's reads.
#pragma unroll
            for (int d2 = 0; d2 < C::DT / 2; ++d2) {
                u32x2 h0[2], h1[2], l0[2], l1[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int dt = 2 * d2 + e;
                    const int g = dt >> 1, c0 = 2 * (dt & 1) + (tr_q >> 1);  // logical hi chunk of dims 16 dt + 4 q ..
                    const unsigned vb = lds_base + (unsigned)((st & (RING - 1)) * C::STAGE + C::NB * C::SUB + g * C::SUB + vkey * 128 + (tr_q & 1) * 8);
                    const unsigned a_hi = vb + (unsigned)((c0 ^ (vkey & 7)) << 4), a_lo = vb + (unsigned)(((4 + c0) ^ (vkey & 7)) << 4);
                    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(h0[e]) : "v"(a_hi));
                    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(h1[e]) : "v"(a_hi));
                    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(l0[e]) : "v"(a_lo));
                    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(l1[e]) : "v"(a_lo));
                }
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(h0[0]), "+v"(h1[0]), "+v"(l0[0]), "+v"(l1[0]), "+v"(h0[1]), "+v"(h1[1]), "+v"(l0[1]), "+v"(l1[1]));
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const u32x4 vh = {h0[e][0], h0[e][1], h1[e][0], h1[e][1]}, vl = {l0[e][0], l0[e][1], l1[e][0], l1[e][1]};
                    o[2 * d2 + e] = split_mma(__builtin_bit_cast(f16x8, vh), __builtin_bit_cast(f16x8, vl), ph, pl, o[2 * d2 + e]);
                }
            }
        }
    }
    if (!live) return;
    float sum = l_run;
    att::quad_sum(sum);
    const float inv = 1.0f / sum;
    const size_t oidx = ((size_t)seq * S + qt * 16 + fr) * E + head * HD;
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) split_store4_rowpair(out, oidx + dt * 16 + 4 * fg, o[dt] * inv, true);
}

template <int HD>
static int launch(const void* qkv, void* out, int n_seq, int heads, float scale, hipStream_t s) {
    using C = Cfg<HD>;
    auto kern = attention_split_dma_kernel<HD>;
    const size_t bytes = (size_t)n_seq * S * 3 * heads * HD * 4;
    PP_REQUIRE(bytes < kOob, PP_ERR_UNSUPPORTED, "pp_attention: qkv tensor exceeds 2 GiB (32-bit buffer offsets)");
    return att::launch_with_lds(kern, dim3(n_seq * heads * QSPLIT), dim3(THREADS), C::LDS, s, reinterpret_cast<const char*>(qkv),
                                reinterpret_cast<char*>(out), n_seq, heads, (unsigned)bytes, scale * att::kLog2e);
}

}  // namespace adma

// 432-token sequences in the split format, head dim 32 or 64 (called from pp_attention)
int attention_split_dma(const void* qkv, void* out, int n_seq, int heads, int head_dim, float scale, hipStream_t s) {
    if (head_dim == 64) return adma::launch<64>(qkv, out, n_seq, heads, scale, s);
    if (head_dim == 32) return adma::launch<32>(qkv, out, n_seq, heads, scale, s);
    return fail(PP_ERR_UNSUPPORTED, "pp_attention (LDS-DMA form): head dim 32 or 64");
}

}  // namespace pp
