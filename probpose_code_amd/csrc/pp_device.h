// Device-side primitives shared by the matrix kernels (gfx950 only): vector types, MFMA wrappers, s_waitcnt encodings, buffer
// resources, LDS DMA and the guarded 16-byte buffer store. Everything here is forced inline and compiles to exactly the instruction
// a kernel would otherwise spell out by hand; the three traps of DESIGN.md 4 ("Three traps") are each encoded once, below.
#pragma once
#include <hip/hip_runtime.h>

namespace pp {

constexpr int WAVE = 64;

// ---- register tuples (u32x4 = one 16-byte chunk as loaded; bit-cast to the element type at the MFMA) and LDS pointers
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_t;  // operand of ds_read_tr16_b64

__device__ __forceinline__ int lane_id() { return threadIdx.x & (WAVE - 1); }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }
// the value of lane ^ 16 / lane ^ 32 by v_permlane16_swap / v_permlane32_swap - plain VALU, no trip through the LDS queue (swap(a, a): an
// even-row lane gets (own, partner's), an odd-row lane (partner's, own))
__device__ __forceinline__ float xor16(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto s = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const unsigned own_is_first = ((threadIdx.x >> 4) & 1u) == 0u;
    return __builtin_bit_cast(float, own_is_first ? (unsigned)s[1] : (unsigned)s[0]);
}
__device__ __forceinline__ float xor32(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto s = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const unsigned own_is_first = ((threadIdx.x >> 5) & 1u) == 0u;
    return __builtin_bit_cast(float, own_is_first ? (unsigned)s[1] : (unsigned)s[0]);
}

// ---- MFMA 16x16 over one 16-byte chunk of K per lane: c += a b^T (a, b: lane = row (lane & 15), k-group (lane >> 4))
__device__ __forceinline__ f32x4 mma_bf16(const u32x4& a, const u32x4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma_f16(const u32x4& a, const u32x4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// fp32: the chunk holds four k, one 16x16x4 MFMA each
__device__ __forceinline__ f32x4 mma_f32(const u32x4& a, const u32x4& b, f32x4 c) {
    const f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], bf[j], c, 0, 0, 0);
    return c;
}

// ---- s_waitcnt as a builtin, not inline asm: the compiler's own wait-count bookkeeping sees it and does not wait again for what
// it covers. gfx9 immediate: vmcnt [3:0] + [15:14], expcnt [6:4] (7 = no wait), lgkmcnt [11:8] (15 = no wait).
// wait_vm<N>: at most N of this wave's vector-memory operations (LDS DMA included) are still outstanding.
template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt immediate");
    __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}
// wait_vm_lgkm<N>: the same, and every LDS access and scalar load has returned (vmcnt(N) lgkmcnt(0)); N = 63 waits for those alone
template <int N>
__device__ __forceinline__ void wait_vm_lgkm() {
    static_assert(N >= 0 && N < 64, "vmcnt immediate");
    __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (0 << 8) | ((N >> 4) << 14));
}

// ---- buffer resource over `bytes` bytes at p: base, stride 0 (raw: offsets are bytes), num_records = bytes, and the gfx950
// flags word 0x00020000 = DATA_FORMAT 4, "32" (bits 18:15 of the fourth dword; the field must hold a valid format although raw
// accesses ignore it), everything else 0: no swizzle, no TID add. A lane whose voffset + immediate offset reaches past `bytes` is
// out of bounds.
constexpr unsigned kRsrcFlags = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, kRsrcFlags);
}
// The out-of-bounds voffset: >= num_records of every tensor (the entry points refuse operands of 2 GiB and more), so a buffer load
// with it reads nothing and delivers ZEROS, also into LDS - padding rows, conv borders and dead pipeline slots are DMA'd like data.
constexpr unsigned kOob = 0x7ffffff0u;

// ---- LDS DMA: every lane fetches the 16 bytes at voffset + soffset (soffset wave-uniform), the wave's 1 KiB lands contiguously
// at lds_dst in lane order (lds_dst wave-uniform: it travels in M0). Counts in vmcnt; nothing orders it against LDS reads but
// wait_vm + barrier.
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, void* lds_dst, unsigned voffset, unsigned soffset = 0) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)lds_dst, 16, voffset, soffset, 0, 0);
}

// ---- 16-byte buffer store. buffer_store_dwordx4 reads its data registers a cycle late for lanes 12 - 15 of every row (one wait
// state with an SGPR soffset, two with an immediate one: scripts/micro/mubuf_store_hazard.hip) and the compiler inserts none for
// the SGPR form: a dead value's register reused right behind the store changes what those lanes write. The s_nop takes q as an
// input, so q's registers live through it (tests/test_no_scratch_in_hot_loops.py checks the ISA).
__device__ __forceinline__ void store16_guarded(u32x4 q, __amdgpu_buffer_rsrc_t rsrc, unsigned voffset, unsigned soffset) {
    __builtin_amdgcn_raw_buffer_store_b128(q, rsrc, voffset, soffset, 0);
    asm volatile("s_nop 3" ::"v"(q));
}

// ---- scheduling groups (sched_group_barrier masks): "next, n instructions of this class"
#define HSGB(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0)
constexpr int SG_VALU = 0x002, SG_MFMA = 0x008, SG_VMEM = 0x010, SG_DS_READ = 0x100;

// byte offset of 16-byte chunk `chunk` of row `row` in a tile of 128-byte rows, chunks XOR-swizzled by the row (conflict-free
// fragment reads; the DMA lanes fetch the source chunk that belongs in their slot)
__device__ __forceinline__ int swz(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }

// exact GELU (libdevice erff; the fast forms live with the kernels that use them)
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

}  // namespace pp
