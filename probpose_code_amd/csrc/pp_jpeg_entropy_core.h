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
static_assert(offsetof(pp_jpeg_ent_desc, restart_interval) == 56, "the interval in the first four of the eight bytes once reserved");

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

// The restart intervals of an image as the *_restart_batch calls see them. per: MCUs per interval (the whole image for
// interval 0 and for one of at least the MCU count: no marker in the scan); count: intervals; bpi: blocks per interval.
struct EntIntervals {
    long long per, count, bpi;
    int R;  // what load_block takes: the interval, 0 for none
};

PP_HOST_DEVICE bool ent_interval_ok(const pp_jpeg_ent_desc& d) { return d.restart_interval >= 0 && d.restart_interval <= 65535; }

PP_HOST_DEVICE EntIntervals ent_intervals(const pp_jpeg_ent_desc& d) {
    EntIntervals v;
    const long long mcus = (long long)d.mcus_x * d.mcus_y;
    v.R = d.restart_interval;
    v.per = (v.R <= 0 || v.R >= mcus) ? mcus : v.R;
    v.count = v.per > 0 ? (mcus + v.per - 1) / v.per : 0;
    v.bpi = v.per * (d.hs * d.vs + 2);
    return v;
}

// An image's share of scratch with restart intervals (pp_jpeg_entropy_restart_scratch_bytes): ent_layout's regions - the bit
// buffer and what follows it longer by seven padding bits per MCU - and behind them, per interval (at most one per MCU):
// irel[j] (u32: the bit offset of the interval's first block inside its chunk of ENT_CHUNK blocks), ilen[j] (u32: its bytes,
// padding included) and ioff[j] (u64: the byte offset of the interval in the unstuffed stream; ioff[count] is the stream's
// length). ent_layout's own result is not changed by any of this.
struct EntRstLayout : EntLayout {
    long long nint, o_irel, o_ilen, o_ioff;
};

PP_HOST_DEVICE EntRstLayout ent_rst_layout(long long nblk, long long mcus) {
    EntRstLayout L;
    if (nblk <= 0) mcus = 0;
    L.nblk = nblk;
    L.nint = mcus;
    L.nchunks = (nblk + ENT_CHUNK - 1) / ENT_CHUNK;
    const long long max_bits = nblk * ENT_BLOCK_BITS + 7 * (mcus > 0 ? mcus : 1);  // (every interval pads its last byte)
    L.max_bytes = (max_bits + 7) / 8;
    L.nwords = (max_bits + 31) / 32 + 4;
    L.nstuff = (L.max_bytes + STUFF_CHUNK - 1) / STUFF_CHUNK;
    L.o_len = 64;
    L.o_csum = ent_align16(L.o_len + 4 * nblk);
    L.o_coff = ent_align16(L.o_csum + 8 * L.nchunks);
    L.o_words = ent_align16(L.o_coff + 8 * L.nchunks);
    L.o_sff = ent_align16(L.o_words + 4 * L.nwords);
    L.o_soff = ent_align16(L.o_sff + 4 * L.nstuff);
    L.o_irel = ent_align16(L.o_soff + 8 * L.nstuff);
    L.o_ilen = ent_align16(L.o_irel + 4 * L.nint);
    L.o_ioff = ent_align16(L.o_ilen + 4 * L.nint);
    L.total = (L.o_ioff + 8 * (L.nint + 1) + 255) / 256 * 256;
    return L;
}

// The layout a phase runs with: ent_layout without restart handling, ent_rst_layout with it.
template <bool RST>
struct EntPhaseLayout {
    using type = EntLayout;
    static PP_HOST_DEVICE EntLayout of(const pp_jpeg_ent_desc&, long long nblk) { return ent_layout(nblk); }
};
template <>
struct EntPhaseLayout<true> {
    using type = EntRstLayout;
    static PP_HOST_DEVICE EntRstLayout of(const pp_jpeg_ent_desc& d, long long nblk) { return ent_rst_layout(nblk, (long long)d.mcus_x * d.mcus_y); }
};

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
// RST: R is the restart interval in MCUs, 0 for none - the first block of each component in an interval has predictor 0.
template <bool RST = false>
PP_HOST_DEVICE void load_block(const pp_jpeg_ent_desc& d, long long s, uint32_t (&w)[32], int& pred, int& chroma, int R = 0) {
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
    if constexpr (RST) {  // no predictor comes over from the MCU before an interval's first
        if (R > 0 && (j == 0 || j >= lum) && (unsigned)mcu % (unsigned)R == 0u) prev = -1;
    }
    pred = prev >= 0 ? (int)d.coef[prev * 64] : 0;
}

// Byte k of the unstuffed stream out of its words (word k / 4 holds it at bits 31 - 8 (k % 4) and down).
PP_HOST_DEVICE uint32_t stream_byte(uint32_t word, int k) { return (word >> (24 - 8 * k)) & 255u; }

// ------------------------------------------------------------------------------------------------ restart intervals
// With P[s] the exclusive prefix of the block lengths (a chunk's offset + the prefix inside the chunk), interval j holds
// P[start of j + 1] - P[start of j] bits and ilen[j] = ceil(that / 8) bytes; ioff[] is the exclusive prefix of ilen[]. The
// unstuffed stream is the byte-aligned intervals back to back: block s of interval j packs at bit 8 ioff[j] + P[s] -
// P[start of j], and the last block of every interval pads its byte with ones. An interval is at least one byte (three
// blocks of at least two bits), so ioff[] is strictly increasing and a byte lies in exactly one interval.

// P[start of interval j]; j == count: the total.
PP_HOST_DEVICE unsigned long long ent_interval_bits_before(const EntIntervals& iv, long long j, const unsigned long long* coff, const uint32_t* irel,
                                                           unsigned long long total_bits) {
    return j >= iv.count ? total_bits : coff[(j * iv.bpi) / ENT_CHUNK] + irel[j];
}

PP_HOST_DEVICE uint32_t ent_interval_bytes(const EntIntervals& iv, long long j, const unsigned long long* coff, const uint32_t* irel,
                                           unsigned long long total_bits) {
    return (uint32_t)((ent_interval_bits_before(iv, j + 1, coff, irel, total_bits) - ent_interval_bits_before(iv, j, coff, irel, total_bits) + 7) >> 3);
}

// Where block s (bit offset P[s] = `before`) packs, and whether it pads.
PP_HOST_DEVICE unsigned long long ent_pack_start(const EntIntervals& iv, long long s, unsigned long long before, const unsigned long long* coff,
                                                 const uint32_t* irel, const unsigned long long* ioff) {
    const long long j = s / iv.bpi;
    return 8ull * ioff[j] + (before - ent_interval_bits_before(iv, j, coff, irel, 0));
}
PP_HOST_DEVICE bool ent_pads(const EntIntervals& iv, long long s, long long nblk) { return s == nblk - 1 || (s + 1) % iv.bpi == 0; }

// The interval that holds byte `b` of the unstuffed stream (b < ioff[count]): the last j with ioff[j] <= b. It is also the
// number of markers in front of the byte.
PP_HOST_DEVICE long long ent_interval_at(const unsigned long long* ioff, long long count, unsigned long long b) {
    long long lo = 0, hi = count;  // ioff[lo] <= b < ioff[hi]
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (ioff[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A thread's `valid` bytes (v: two words) from byte `byte0` of the unstuffed stream to their places in the output; pos: the
// place of the first with the FF bytes in front of it counted, the markers not. A 00 behind every FF, and FF D0 + (j & 7)
// behind the last byte of interval j unless it is the image's last - eight bytes may cross several interval ends.
PP_HOST_DEVICE void ent_stuff_restart(const uint32_t (&v)[2], int valid, long long byte0, long long pos, const unsigned long long* ioff, long long count,
                                      uint8_t* out, long long capacity) {
    if (valid <= 0) return;
    long long j = ent_interval_at(ioff, count, (unsigned long long)byte0);
    long long end = (long long)ioff[j + 1];
    pos += 2 * j;
    for (int k = 0; k < 8; ++k) {
        if (k >= valid) break;
        const uint32_t b = stream_byte(v[k >> 2], k & 3);
        if (pos < capacity) out[pos] = (uint8_t)b;
        ++pos;
        if (b == 255u) {
            if (pos < capacity) out[pos] = 0;
            ++pos;
        }
        if (byte0 + k + 1 == end && j + 1 < count) {
            if (pos < capacity) out[pos] = 0xFF;
            if (pos + 1 < capacity) out[pos + 1] = (uint8_t)(0xD0 + (j & 7));
            pos += 2;
            ++j;
            end = (long long)ioff[j + 1];
        }
    }
}

}  // namespace pp
