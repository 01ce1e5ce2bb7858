// The code core of the device Huffman coder (csrc/pp_jpeg_entropy.hip), shared with its sequential host restatement
// (scripts/jpeg_entropy_host_check.cpp): the annex K code tables, an image's scratch layout, the addressing of a block and
// its DC predictor, the code walk over a block and the bit packer. Plain C++ that compiles for host and device; nothing
// here touches the GPU.
#pragma once
#include <cstdint>

#include "pp_jpeg_enc_host.h"

namespace pp {

constexpr int ENT_CHUNK = 256;      // blocks per workgroup of jpeg_ent_bits / jpeg_ent_pack: one per thread
constexpr int STUFF_CHUNK = 2048;   // unstuffed bytes per workgroup pass of jpeg_ent_ffcount / jpeg_ent_stuff: eight per thread
constexpr int ENT_BLOCK_BITS = 1665;  // 16 + 11 bits of DC, 63 x (16 + 10) bits of AC

// what probpose_code_amd/jpeg.py mirrors (_ENT_DESC, _ENT_RESULT)
static_assert(sizeof(pp_jpeg_ent_desc) == 64 && sizeof(pp_jpeg_ent_result) == 16, "jpeg.py mirrors these");
static_assert(offsetof(pp_jpeg_ent_desc, capacity) == 32, "four pointers, then the capacity");

// code | size << 16 of every symbol: [0] luma, [1] chroma
struct EntTables {
    uint32_t dc[2][12];
    uint32_t ac[2][256];
};

constexpr void ent_derive(uint32_t* t, const uint8_t* bits, const uint8_t* vals) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k, ++code) t[vals[k]] = code | ((uint32_t)len << 16);
        code <<= 1;
    }
}

constexpr EntTables ent_tables() {
    EntTables t{};
    ent_derive(t.dc[0], jpeg::kDcLumaBits, jpeg::kDcVals);
    ent_derive(t.dc[1], jpeg::kDcChromaBits, jpeg::kDcVals);
    ent_derive(t.ac[0], jpeg::kAcLumaBits, jpeg::kAcLumaVals);
    ent_derive(t.ac[1], jpeg::kAcChromaBits, jpeg::kAcChromaVals);
    return t;
}

// An image's share of scratch (pp_jpeg_entropy_scratch_bytes): byte offsets of its regions, each 16-byte aligned.
struct EntLayout {
    long long nblk, nchunks, nwords, max_bytes, nstuff;
    long long o_len, o_csum, o_coff, o_words, o_sff, o_soff, total;
};

struct EntHeader {  // first 64 bytes of the share
    unsigned long long total_bits, nbytes;
    unsigned int bad, ok;
};

PP_HOST_DEVICE long long ent_align16(long long v) { return (v + 15) / 16 * 16; }

PP_HOST_DEVICE EntLayout ent_layout(long long nblk) {
    EntLayout L;
    L.nblk = nblk;
    L.nchunks = (nblk + ENT_CHUNK - 1) / ENT_CHUNK;
    const long long max_bits = nblk * ENT_BLOCK_BITS + 7;  // (and the padding of the last byte)
    L.max_bytes = (max_bits + 7) / 8;
    L.nwords = (max_bits + 31) / 32 + 4;  // (zeroed sixteen bytes at a time)
    L.nstuff = (L.max_bytes + STUFF_CHUNK - 1) / STUFF_CHUNK;
    L.o_len = 64;
    L.o_csum = ent_align16(L.o_len + 4 * nblk);
    L.o_coff = ent_align16(L.o_csum + 8 * L.nchunks);
    L.o_words = ent_align16(L.o_coff + 8 * L.nchunks);
    L.o_sff = ent_align16(L.o_words + 4 * L.nwords);
    L.o_soff = ent_align16(L.o_sff + 4 * L.nstuff);
    L.total = (L.o_soff + 8 * L.nstuff + 255) / 256 * 256;
    return L;
}

// Blocks of the scan, 0 for a descriptor that holds no pp_jpeg_encode_plan geometry (its status becomes PP_ERR_INVALID_ARG).
PP_HOST_DEVICE long long ent_blocks(const pp_jpeg_ent_desc& d) {
    const bool sampling = (d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2);
    if (!sampling || d.mcus_x < 1 || d.mcus_y < 1 || d.mcus_x > 8192 || d.mcus_y > 8192 || !d.coef || !d.scratch || !d.out || !d.result) return 0;
    return (long long)d.mcus_x * d.mcus_y * (d.hs * d.vs + 2);
}

PP_HOST_DEVICE int ent_category(int v) { return v ? 32 - __builtin_clz((unsigned)(v < 0 ? -v : v)) : 0; }  // bits of |v|

PP_HOST_DEVICE void or_word(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;  // (the sequential restatement of the stand-alone host check)
#endif
}

struct BitCounter {
    uint32_t bits = 0;
    PP_HOST_DEVICE void put(uint32_t, int count) { bits += (uint32_t)count; }
};

// MSB-first bits ORed into zeroed 32-bit words, from bit `start` on; word indices at or past `cap` are dropped.
struct BitPacker {
    uint32_t* words;
    long long widx, cap;
    uint64_t acc = 0;
    int n;  // bits held in acc, < 32 between calls (the first word's leading bits, another thread's, count as held zeros)
    PP_HOST_DEVICE BitPacker(uint32_t* w, unsigned long long start, long long cap_) : words(w), widx((long long)(start >> 5)), cap(cap_), n((int)(start & 31)) {}
    PP_HOST_DEVICE void put(uint32_t bits, int count) {  // count <= 27
        acc = (acc << count) | (bits & ((1u << count) - 1u));
        n += count;
        if (n >= 32) {
            n -= 32;
            if (widx < cap) or_word(words + widx, (uint32_t)(acc >> n));
            ++widx;
        }
    }
    PP_HOST_DEVICE void finish() {
        if (n > 0 && widx < cap) or_word(words + widx, (uint32_t)(acc << (32 - n)));
    }
    PP_HOST_DEVICE int phase() const { return n & 7; }
};

// The codes of one block into `sink`, as entropy_encode writes them. w: its 64 coefficients, two per word, natural order;
// pred: the DC value of the block before it; dc / ac: the component's tables (in LDS). Returns true for a coefficient no
// baseline code expresses (it is coded with its category clamped to 11 resp. 10).
template <class Sink>
PP_HOST_DEVICE bool code_block(const uint32_t (&w)[32], int pred, const uint32_t* dc, const uint32_t* ac, Sink& sink) {
    bool bad = false;
    const int diff = (int)(int16_t)(w[0] & 0xFFFFu) - pred;
    int s = ent_category(diff);
    if (s > 11) {
        bad = true;
        s = 11;
    }
    {
        const uint32_t e = dc[s];
        sink.put((e << s) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u)), (int)(e >> 16) + s);
    }
    const uint32_t zrl = ac[0xF0];
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int i = jpeg::kNatural[k];  // (a constant once the loop is unrolled)
        const int a = (int)(int16_t)((w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
        if (a == 0) {
            ++run;
        } else {
            for (; run > 15; run -= 16) sink.put(zrl, (int)(zrl >> 16));
            s = ent_category(a);
            if (s > 10) {
                bad = true;
                s = 10;
            }
            const uint32_t e = ac[(run << 4) | s];
            sink.put((e << s) | ((uint32_t)(a < 0 ? a - 1 : a) & ((1u << s) - 1u)), (int)(e >> 16) + s);
            run = 0;
        }
    }
    if (run > 0) sink.put(ac[0], (int)(ac[0] >> 16));
    return bad;
}

// sixteen bytes of coefficients, loaded at once
#if defined(__HIPCC__)
using EntQuad = uint4;
#else
struct alignas(16) EntQuad {
    uint32_t x, y, z, w;
};
#endif

// Block s of the scan: loads its coefficients, finds its component (0 luma, 1 chroma tables) and its DC predictor.
PP_HOST_DEVICE void load_block(const pp_jpeg_ent_desc& d, long long s, uint32_t (&w)[32], int& pred, int& chroma) {
    const int lum = d.hs * d.vs, bpm = lum + 2;
    const long long mcu = s / bpm, mcus = (long long)d.mcus_x * d.mcus_y;
    const int j = (int)(s - mcu * bpm);
    const long long my = mcu / d.mcus_x, mx = mcu - my * d.mcus_x;
    const long long bw0 = (long long)d.mcus_x * d.hs;
    long long idx, prev = -1;  // block indices in d.coef
    if (j < lum) {
        chroma = 0;
        idx = (my * d.vs + j / d.hs) * bw0 + mx * d.hs + j % d.hs;
        if (j > 0) prev = (my * d.vs + (j - 1) / d.hs) * bw0 + mx * d.hs + (j - 1) % d.hs;
        else if (mcu > 0) {  // the last luma block of the MCU before
            const long long py = (mcu - 1) / d.mcus_x, px = (mcu - 1) - py * d.mcus_x;
            prev = (py * d.vs + d.vs - 1) * bw0 + px * d.hs + d.hs - 1;
        }
    } else {
        chroma = 1;
        idx = mcus * lum + (long long)(j - lum) * mcus + mcu;  // a chroma plane is one block per MCU, in MCU order
        if (mcu > 0) prev = idx - 1;
    }
    const EntQuad* p = reinterpret_cast<const EntQuad*>(d.coef + idx * 64);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const EntQuad v = p[q];
        w[4 * q] = v.x;
        w[4 * q + 1] = v.y;
        w[4 * q + 2] = v.z;
        w[4 * q + 3] = v.w;
    }
    pred = prev >= 0 ? (int)d.coef[prev * 64] : 0;
}

// Byte k of the unstuffed stream out of its words (word k / 4 holds it at bits 31 - 8 (k % 4) and down).
PP_HOST_DEVICE uint32_t stream_byte(uint32_t word, int k) { return (word >> (24 - 8 * k)) & 255u; }

}  // namespace pp
