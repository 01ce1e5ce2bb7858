// The core of the device PNG writer (csrc/pp_png.hip), shared with its sequential host form (pp_png_encode, pp_zlib_compress
// and scripts/png_host_check.cpp): the five row filters and the choice rule, the tile constant, the emission rule of the
// run-length tokens with the length symbols, the LSB-first bit packer, a stream's scratch layout, the Adler-32 and CRC-32
// partials with their combination, and - host only - the code builder, the header writer, the framing and the sequential
// coder. Plain C++ that compiles for host and device; nothing here touches the GPU.
//
// The format. A row of W pixels becomes a filter-type byte and 3 W filtered bytes in R, G, B order (bpp 3; what lies above or
// left of the picture counts as 0); of the five filters the row takes the one with the smallest sum of min(b, 256 - b) over
// its bytes, the lowest number on a tie. The filtered stream is cut into tiles of PNG_TILE bytes. A run is a maximal stretch
// of equal bytes inside one tile; byte k of a run of length L emits: k = 0 a literal; else with j = k - 1, g = j / 258,
// m = min(258, L - 1 - 258 g): a literal if m < 3, a match of length m at distance 1 if j % 258 == 0, nothing otherwise. So
// what a byte emits depends on its position, its run's start and its run's end only. One dynamic deflate block per stream:
// the literal/length code from the stream's own histogram (symbol 256 counted once), one distance code of length 1, zlib
// header 78 01 in front, Adler-32 behind.
//
// The second match mode, "lz" (the *_lz entry points; the run rule above stays the default and gives the same bytes as
// before). Filters, tiles, one dynamic block, zlib header and Adler-32 as above. Integers only. s[0, len): the stream;
// E(g) = min(len, PNG_TILE (g / PNG_TILE + 1)): the end of g's tile.
//   m_d(g)   0 if g < d, else the largest m <= min(258, E(g) - g) with s[g + i] == s[g + i - d] for all i < m: a match never
//            covers bytes beyond its tile, its source may lie anywhere earlier in the stream and may overlap its output;
//   N        the near candidates (1, 3); F: the far candidates (P, P - 3, P + 3) in this order, P = 1 + 3 width for a picture
//            and the descriptor's `period` for a raw stream (0: F is empty); members of F below 4 or above 32768 are dropped;
//   Ln(g)    the largest m_d(g) over N if that is >= 3, else 0; dn: the first d of N that attains it;
//   Lf(g)    likewise over F with a minimum of 4; df;
//   reach(g) max(Ln(g), 1 + Ln(g + 1)), the second term only when g + 1 < E(g) and Ln(g + 1) > 0;
//   a position g that starts a token emits the match (Lf, df) if Lf(g) > 0 and Lf(g) >= reach(g) + 3, else the match
//   (Ln, dn) if Ln(g) > 0, else the literal s[g];
//   a tile's first byte starts a token; behind a token at g of length l (1 for a literal) g + l starts one; tiles are
//   independent.
// The literal/length code as above; a distance code over symbols 0 .. 29 built the same way (build_lengths, limit 15; with
// fewer than two used symbols unused ones are added), HDIST the highest symbol with a length; the code-length code still
// avoids symbols 16 .. 18. A match takes up to 15 + 5 + 15 + 13 bits: two put calls. The parse is kept as one uint16 per
// byte: 0 covered by a match, 1 a literal, else length | candidate index << 9 (candidates in the order 1, 3, P, P - 3, P + 3).
//
// The code builder below (build_lengths, canonical_codes, build_code, build_code_lz) is host only; csrc/pp_png_code_core.h
// restates it as steps over fixed-size arrays that a workgroup runs (png_code) and gives the same bytes.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pp_jpeg_entropy_core.h"  // PP_HOST_DEVICE, or_word, ent_align16

namespace pp {
namespace png {

constexpr int PNG_TILE = 4096;  // bytes of the filtered stream per workgroup of png_hist / png_bits / png_pack; runs end at its borders
constexpr int PNG_SPAN = 16;    // bytes per thread
constexpr int DEFLATE_SYMS = 286;
constexpr int DEFLATE_HEADER_BITS = 16 + 3 + 14 + 19 * 3 + 287 * 7;  // the longest header: no length of the code-length code above 7
constexpr int CRC_CHUNK = 4096;  // bytes per workgroup pass of png_crc: sixteen per thread
constexpr uint32_t ADLER_MOD = 65521u;

// what probpose_code_amd/png.py mirrors (_DESC, _RESULT, CODE_BYTES)
static_assert(sizeof(pp_deflate_desc) == 104 && sizeof(pp_deflate_result) == 16 && sizeof(pp_deflate_code) == 1472, "png.py mirrors these");
static_assert(DEFLATE_HEADER_BITS <= 32 * 76, "pp_deflate_code.header holds the longest header");

// ------------------------------------------------------------------------------------------------------------ filters
// Byte i (0 .. 3 W - 1) of a row in R, G, B order; rgb: the order in memory.
PP_HOST_DEVICE int raw_byte(const uint8_t* row, int i, int rgb) {
    const int px = i / 3, ch = i - 3 * px;
    return row[3 * px + (rgb ? ch : 2 - ch)];
}

PP_HOST_DEVICE int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// x filtered by filter `type`; a: the byte three to the left, b: the byte above, c: the byte above a.
PP_HOST_DEVICE uint32_t filter_byte(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : paeth(a, b, c);
    return (uint32_t)(x - pred) & 255u;
}

PP_HOST_DEVICE uint32_t filter_cost(uint32_t f) { return f < 128u ? f : 256u - f; }

PP_HOST_DEVICE int filter_choice(const uint32_t* cost) {
    int best = 0;
    for (int t = 1; t < 5; ++t)
        if (cost[t] < cost[best]) best = t;
    return best;
}

// The filtered bytes of byte i of a row under all five filters. up: the row above, NULL for the first row.
PP_HOST_DEVICE void filter_all(const uint8_t* cur, const uint8_t* up, int i, int rgb, uint32_t (&f)[5]) {
    const int x = raw_byte(cur, i, rgb), a = i >= 3 ? raw_byte(cur, i - 3, rgb) : 0, b = up ? raw_byte(up, i, rgb) : 0,
              c = (up && i >= 3) ? raw_byte(up, i - 3, rgb) : 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) f[t] = filter_byte(t, x, a, b, c);
}

// ------------------------------------------------------------------------------------------------------------- tokens
// What byte k of a run of length L emits: 0 nothing, 1 a literal, otherwise a match of that length (3 .. 258).
PP_HOST_DEVICE int emission(int k, int L) {
    if (k == 0) return 1;
    const int j = k - 1, g = j / 258;
    int m = L - 1 - 258 * g;
    if (m > 258) m = 258;
    if (m < 3) return 1;
    return j - 258 * g == 0 ? m : 0;
}

// Length symbol (257 .. 285), number of extra bits and their value of a match length 3 .. 258.
PP_HOST_DEVICE void length_symbol(int m, int& sym, int& ebits, uint32_t& extra) {
    const int v = m - 3;
    if (m == 258) {
        sym = 285, ebits = 0, extra = 0;
    } else if (v < 8) {
        sym = 257 + v, ebits = 0, extra = 0;
    } else {
        const int e = 29 - __builtin_clz((unsigned)v);  // floor(log2 v) - 2
        sym = 257 + 4 * (e + 1) + ((v >> e) & 3);
        ebits = e;
        extra = (uint32_t)v & ((1u << e) - 1u);
    }
}

PP_HOST_DEVICE uint32_t span_byte(const uint32_t (&w)[4], int i) { return (w[(i >> 2) & 3] >> (8 * (i & 3))) & 255u; }

// The tokens of one span: cnt (1 .. 16) bytes of a tile from position p0 on, held in w (byte i at bits 8 (i % 4) of word
// i / 4). left_start: the start of the run that holds byte p0, right_end: the end of the run that holds byte p0 + cnt - 1
// (positions in the tile). sink.literal(byte) / sink.match(length) in stream order.
template <class Sink>
PP_HOST_DEVICE void span_tokens(const uint32_t (&w)[4], int cnt, int p0, int left_start, int right_end, Sink& sink) {
    int end[PNG_SPAN];
    int e = right_end;
#pragma unroll
    for (int i = PNG_SPAN - 1; i >= 0; --i) {
        if (i < cnt) {
            if (i < cnt - 1 && span_byte(w, i) != span_byte(w, i + 1)) e = p0 + i;
            end[i] = e;
        }
    }
    int s = left_start;
#pragma unroll
    for (int i = 0; i < PNG_SPAN; ++i) {
        if (i < cnt) {
            const uint32_t b = span_byte(w, i);
            if (i > 0 && b != span_byte(w, i - 1)) s = p0 + i;
            const int em = emission(p0 + i - s, end[i] - s + 1);
            if (em == 1) sink.literal(b);
            else if (em >= 3) sink.match(em);
        }
    }
}

PP_HOST_DEVICE void add_word(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;  // (the sequential form)
#endif
}

struct HistSink {  // hist: 286 counts
    uint32_t* hist;
    PP_HOST_DEVICE void literal(uint32_t b) { add_word(hist + b, 1u); }
    PP_HOST_DEVICE void match(int m) {
        int sym, ebits;
        uint32_t extra;
        length_symbol(m, sym, ebits, extra);
        add_word(hist + sym, 1u);
    }
};

struct LsbCounter {
    uint32_t bits = 0;
    PP_HOST_DEVICE void put(uint32_t, int count) { bits += (uint32_t)count; }
};

// LSB-first bits ORed into zeroed little-endian 32-bit words (so the words are the bytes in file order), from bit `start`
// on; word indices at or past `cap` are dropped.
struct LsbPacker {
    uint32_t* words;
    long long widx, cap;
    uint64_t acc = 0;
    int n;  // bits held in acc, < 32 between calls (the first word's low bits, another writer's, count as held zeros)
    PP_HOST_DEVICE LsbPacker(uint32_t* w, unsigned long long start, long long cap_) : words(w), widx((long long)(start >> 5)), cap(cap_), n((int)(start & 31)) {}
    PP_HOST_DEVICE void put(uint32_t bits, int count) {  // count <= 32, no bit of `bits` set at or above count
        acc |= (uint64_t)bits << n;
        n += count;
        if (n >= 32) {
            if (widx < cap) or_word(words + widx, (uint32_t)acc);
            ++widx;
            acc >>= 32;
            n -= 32;
        }
    }
    PP_HOST_DEVICE void finish() {
        if (n > 0 && widx < cap) or_word(words + widx, (uint32_t)acc);
    }
    PP_HOST_DEVICE int phase() const { return n & 7; }
};

// Tokens to code bits. sym: pp_deflate_code.sym. A match is its length code, the extra bits and the one-bit distance code 0.
template <class Put>
struct CodeSink {
    const uint32_t* sym;
    Put& out;
    PP_HOST_DEVICE void literal(uint32_t b) {
        const uint32_t e = sym[b];
        out.put(e & 0xFFFFu, (int)(e >> 16));
    }
    PP_HOST_DEVICE void match(int m) {
        int s, ebits;
        uint32_t extra;
        length_symbol(m, s, ebits, extra);
        const uint32_t e = sym[s];
        const int len = (int)(e >> 16);
        out.put((e & 0xFFFFu) | (extra << len), len + ebits + 1);
    }
};

// What ends a stream behind its last token: the end-of-block code, zeros up to a byte, the Adler-32 big-endian.
template <class Put>
PP_HOST_DEVICE void put_tail(Put& out, const uint32_t* sym, uint32_t adler) {
    out.put(sym[256] & 0xFFFFu, (int)(sym[256] >> 16));
    if (out.phase()) out.put(0u, 8 - out.phase());
    out.put(((adler >> 24) & 255u) | (((adler >> 16) & 255u) << 8) | (((adler >> 8) & 255u) << 16) | ((adler & 255u) << 24), 32);
}

// ------------------------------------------------------------------------------------------------------------ scratch
// A stream's share of scratch (pp_deflate_scratch_bytes): byte offsets of its regions, each 16-byte aligned.
struct DefLayout {
    long long len, ntiles, max_bytes, nwords;
    long long o_tadler, o_tsum, o_toff, o_words, total;
};

struct DefHeader {  // first 64 bytes of the share
    unsigned long long total_bits, nbytes;
    unsigned int adler, ok;
};

PP_HOST_DEVICE long long deflate_bound(long long len) {  // every byte emits at most one token of at most 15 bits, or a third of a match of 21
    return (DEFLATE_HEADER_BITS + 15 * len + 15 + 7) / 8 + 4;
}

PP_HOST_DEVICE DefLayout def_layout(long long len) {
    DefLayout L;
    L.len = len;
    L.ntiles = (len + PNG_TILE - 1) / PNG_TILE;
    L.max_bytes = deflate_bound(len);
    L.nwords = (L.max_bytes + 3) / 4 + 4;  // (zeroed and read sixteen bytes at a time)
    L.o_tadler = 64;
    L.o_tsum = ent_align16(L.o_tadler + 8 * L.ntiles);
    L.o_toff = ent_align16(L.o_tsum + 4 * L.ntiles);
    L.o_words = ent_align16(L.o_toff + 8 * L.ntiles);
    L.total = (L.o_words + 4 * L.nwords + 255) / 256 * 256;
    return L;
}

// The stream a descriptor describes, 0 for one that describes none (its status becomes PP_ERR_INVALID_ARG).
PP_HOST_DEVICE long long def_len(const pp_deflate_desc& d) {
    if (!d.data || !d.hist || !d.scratch || !d.out || !d.result || d.len < 1 || d.len > 0x7FFFFFFFll || d.capacity < 0) return 0;
    if (d.pixels) {
        if (d.width < 1 || d.height < 1 || d.width > 65535 || d.height > 65535 || d.row_stride < 3ll * d.width) return 0;
        if (d.len != (long long)d.height * (1 + 3ll * d.width)) return 0;
    }
    return d.len;
}

// ------------------------------------------------------------------------------------------------------------ Adler-32
// A span's share of its tile's partial: s1 = the sum of its bytes, s2 = the sum of byte x (bytes of the tile from it on).
PP_HOST_DEVICE void adler_span(const uint32_t (&w)[4], int cnt, int from_on, uint32_t& s1, uint32_t& s2) {
    s1 = 0, s2 = 0;
#pragma unroll
    for (int i = 0; i < PNG_SPAN; ++i) {
        if (i < cnt) {
            const uint32_t b = span_byte(w, i);
            s1 += b;
            s2 += b * (uint32_t)(from_on - i);
        }
    }
}

// A tile's term of the high half: its pair weighted by the bytes behind it. adler = ((N + sum of terms) % M) << 16 | (1 + sum of s1) % M.
PP_HOST_DEVICE uint32_t adler_term(uint32_t s1, uint32_t s2, unsigned long long behind) {
    return (uint32_t)((s2 % ADLER_MOD + (unsigned long long)(s1 % ADLER_MOD) * (behind % ADLER_MOD)) % ADLER_MOD);
}

// -------------------------------------------------------------------------------------------------------------- CRC-32
constexpr uint32_t CRC_POLY = 0xEDB88320u;

// a x b modulo the CRC polynomial, both in the register's reflected form (x^0 is 0x80000000).
PP_HOST_DEVICE constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
    }
    return p;
}

struct CrcTables {
    uint32_t byte[256];  // the register after one byte from register 0
    uint32_t x2n[32];    // x^(2^k)
};

constexpr CrcTables crc_tables() {
    CrcTables t{};
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
        t.byte[i] = c;
    }
    uint32_t p = 0x40000000u;
    t.x2n[0] = p;
    for (int k = 1; k < 32; ++k) t.x2n[k] = p = crc_mul(p, p);
    return t;
}

// x^(8 nbytes): a register times this is the register after nbytes zero bytes. So the register after a chunk D from register
// S is crc_mul(crc_shift(|D|), S) ^ (the register after D from 0), and the partials of chunks combine by XOR once each is
// shifted by the bytes behind it.
PP_HOST_DEVICE uint32_t crc_shift(const uint32_t* x2n, unsigned long long nbytes) {
    uint32_t p = 0x80000000u;
    for (unsigned k = 3; nbytes; nbytes >>= 1, ++k)
        if (nbytes & 1u) p = crc_mul(x2n[k & 31u], p);
    return p;
}

PP_HOST_DEVICE uint32_t crc_byte(const uint32_t* tab, uint32_t reg, uint32_t b) { return tab[(reg ^ b) & 255u] ^ (reg >> 8); }

// ------------------------------------------------------------------------------------------------------------- lz mode
constexpr int LZ_CANDS = 5;  // distances 1, 3, P, P - 3, P + 3: the parse's candidate index
constexpr int LZ_NEAR_MIN = 3, LZ_FAR_MIN = 4, LZ_MARGIN = 3;
constexpr int LZ_DIST_SYMS = 30, LZ_DIST_AT = 288, LZ_HIST_WORDS = 320;  // hist: 288 words as in runs mode, then the distance counts
constexpr int DEFLATE_HEADER_BITS_LZ = 16 + 3 + 14 + 19 * 3 + (DEFLATE_SYMS + LZ_DIST_SYMS) * 7;

static_assert(sizeof(pp_deflate_code_lz) == 1600 && offsetof(pp_deflate_code_lz, dist) == sizeof(pp_deflate_code), "png.py mirrors these");
static_assert(DEFLATE_HEADER_BITS_LZ == 2302 && DEFLATE_HEADER_BITS_LZ <= 32 * 76, "pp_deflate_code.header holds the longest lz header");

struct LzDist {
    int d[LZ_CANDS];  // 0: a dropped candidate
};

// The candidates of row period P (0: no far candidates).
PP_HOST_DEVICE LzDist lz_dists(long long P) {
    LzDist r;
    r.d[0] = 1, r.d[1] = 3;
    const long long f[3] = {P, P - 3, P + 3};
#pragma unroll
    for (int k = 0; k < 3; ++k) r.d[2 + k] = (P > 0 && f[k] >= 4 && f[k] <= 32768) ? (int)f[k] : 0;
    return r;
}

PP_HOST_DEVICE long long lz_period(const pp_deflate_desc& d) { return d.pixels ? 1 + 3ll * d.width : d.period; }

// def_len for a descriptor of lz mode.
PP_HOST_DEVICE long long def_len_lz(const pp_deflate_desc& d) {
    if (d.period < 0 || (d.pixels && d.period != 0)) return 0;
    return def_len(d);
}

// Distance symbol (0 .. 29), number of extra bits and their value of a distance 1 .. 32768.
PP_HOST_DEVICE void distance_symbol(int dist, int& sym, int& ebits, uint32_t& extra) {
    const int v = dist - 1;
    if (v < 4) {
        sym = v, ebits = 0, extra = 0;
    } else {
        const int nb = 31 - __builtin_clz((unsigned)v);  // floor(log2 v)
        ebits = nb - 1;
        sym = 2 * nb + ((v >> ebits) & 1);
        extra = (uint32_t)v & ((1u << ebits) - 1u);
    }
}

// What position g emits if it starts a token, as the parse stores it. m: m_d(g) of the five candidates (0 for a dropped
// one); ln_next: Ln(g + 1), 0 where g + 1 is past the tile. ln <- Ln(g).
PP_HOST_DEVICE int lz_token(const int (&m)[LZ_CANDS], int ln_next, int& ln) {
    const int cn = m[0] >= m[1] ? 0 : 1;
    ln = m[cn] >= LZ_NEAR_MIN ? m[cn] : 0;
    int cf = 2;
    if (m[3] > m[cf]) cf = 3;
    if (m[4] > m[cf]) cf = 4;
    const int lf = m[cf] >= LZ_FAR_MIN ? m[cf] : 0;
    const int reach = (ln_next > 0 && 1 + ln_next > ln) ? 1 + ln_next : ln;
    if (lf > 0 && lf >= reach + LZ_MARGIN) return lf | (cf << 9);
    if (ln > 0) return ln | (cn << 9);
    return 1;
}

// A span's view of the candidates. eq[c] bit i: byte p0 + i of the tile equals the byte d_c before it in the stream (clear
// where there is none, for a dropped candidate and at or past the tile's end); nu_next[c]: the first position at or behind
// the span's end (p0 + cnt) whose bit is clear, n where all are set up to the tile's end.
struct LzSpan {
    uint32_t eq[LZ_CANDS];
    int nu_next[LZ_CANDS];
};

// tok[i] <- what byte p0 + i (i < cnt) of a tile of n bytes emits if it starts a token.
PP_HOST_DEVICE void lz_span_tokens(const LzSpan& s, int cnt, int p0, int n, uint16_t (&tok)[PNG_SPAN]) {
    int nu[LZ_CANDS], m[LZ_CANDS], ln_next = 0;
#pragma unroll
    for (int c = 0; c < LZ_CANDS; ++c) {
        nu[c] = s.nu_next[c];
        const int left = nu[c] - (p0 + cnt);
        m[c] = left > 258 ? 258 : left;
    }
    if (p0 + cnt < n) (void)lz_token(m, 0, ln_next);
#pragma unroll
    for (int i = PNG_SPAN - 1; i >= 0; --i) {
        tok[i] = 0;
        if (i < cnt) {
#pragma unroll
            for (int c = 0; c < LZ_CANDS; ++c) {
                if (!((s.eq[c] >> i) & 1u)) nu[c] = p0 + i;
                const int left = nu[c] - (p0 + i);
                m[c] = left > 258 ? 258 : left;
            }
            int ln;
            tok[i] = (uint16_t)lz_token(m, ln_next, ln);
            ln_next = ln;
        }
    }
}

PP_HOST_DEVICE int lz_step(uint32_t tok) { return tok <= 1u ? 1 : (int)(tok & 511u); }

// A stored parse entry to a sink: sink.literal(byte) / sink.match(length, distance).
template <class Sink>
PP_HOST_DEVICE void lz_emit(uint32_t v, uint32_t byte, const LzDist& D, Sink& sink) {
    if (v == 1u) sink.literal(byte);
    else if (v > 1u) sink.match((int)(v & 511u), D.d[(v >> 9) & 7u]);
}

struct LzHistSink {  // hist: LZ_HIST_WORDS counts
    uint32_t* hist;
    PP_HOST_DEVICE void literal(uint32_t b) { add_word(hist + b, 1u); }
    PP_HOST_DEVICE void match(int m, int dist) {
        int sym, ebits;
        uint32_t extra;
        length_symbol(m, sym, ebits, extra);
        add_word(hist + sym, 1u);
        distance_symbol(dist, sym, ebits, extra);
        add_word(hist + LZ_DIST_AT + sym, 1u);
    }
};

// Tokens to code bits in lz mode. sym: pp_deflate_code.sym, dsym: pp_deflate_code_lz.dist. A match is two puts: the length
// code with its extra bits (at most 20 bits), the distance code with its extra bits (at most 28).
template <class Put>
struct LzCodeSink {
    const uint32_t* sym;
    const uint32_t* dsym;
    Put& out;
    PP_HOST_DEVICE void literal(uint32_t b) {
        const uint32_t e = sym[b];
        out.put(e & 0xFFFFu, (int)(e >> 16));
    }
    PP_HOST_DEVICE void match(int m, int dist) {
        int s, ebits;
        uint32_t extra;
        length_symbol(m, s, ebits, extra);
        uint32_t e = sym[s];
        int len = (int)(e >> 16);
        out.put((e & 0xFFFFu) | (extra << len), len + ebits);
        distance_symbol(dist, s, ebits, extra);
        e = dsym[s];
        len = (int)(e >> 16);
        out.put((e & 0xFFFFu) | (extra << len), len + ebits);
    }
};

PP_HOST_DEVICE long long deflate_bound_lz(long long len) {  // a literal takes at most 15 bits; a match of m >= 3 bytes at most 48, never 15 m
    return (DEFLATE_HEADER_BITS_LZ + 15 * len + 15 + 7) / 8 + 4;
}

// A stream's share of scratch in lz mode (pp_deflate_scratch_bytes_lz): the regions of runs mode sized by the lz bound, then
// the parse, PNG_TILE entries a tile.
struct LzLayout : DefLayout {
    long long o_parse, parse_entries;
};

PP_HOST_DEVICE LzLayout def_layout_lz(long long len) {
    LzLayout L;
    L.len = len;
    L.ntiles = (len + PNG_TILE - 1) / PNG_TILE;
    L.max_bytes = deflate_bound_lz(len);
    L.nwords = (L.max_bytes + 3) / 4 + 4;
    L.o_tadler = 64;
    L.o_tsum = ent_align16(L.o_tadler + 8 * L.ntiles);
    L.o_toff = ent_align16(L.o_tsum + 4 * L.ntiles);
    L.o_words = ent_align16(L.o_toff + 8 * L.ntiles);
    L.o_parse = ent_align16(L.o_words + 4 * L.nwords);
    L.parse_entries = L.ntiles * PNG_TILE;
    L.total = (L.o_parse + 2 * L.parse_entries + 255) / 256 * 256;
    return L;
}

// =========================================================================================================== host only
// Code lengths of at most `limit` bits for n symbols with these counts: Huffman's, and where its tree is deeper, the deep
// leaves are lifted to `limit` and the Kraft sum is brought back to 1 by moving leaves down one level. With fewer than two
// used symbols the lowest unused ones are added. Equal counts are ordered by symbol number: the same counts, the same code.
inline void build_lengths(const uint32_t* count, int n, int limit, uint8_t* len) {
    std::vector<int> order;
    for (int s = 0; s < n; ++s) {
        len[s] = 0;
        if (count[s]) order.push_back(s);
    }
    for (int s = 0; (int)order.size() < 2 && s < n; ++s)
        if (std::find(order.begin(), order.end(), s) == order.end()) order.push_back(s);
    const int u = (int)order.size();
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return count[a] != count[b] ? count[a] < count[b] : a < b; });
    // two queues: the leaves in rising order and the inner nodes in the order they are made (rising as well)
    std::vector<unsigned long long> weight(2 * u);
    std::vector<int> parent(2 * u, -1);
    for (int i = 0; i < u; ++i) weight[i] = count[order[i]];
    int leaf = 0, inner = u, made = u;
    auto take = [&]() { return (leaf < u && (inner >= made || weight[leaf] <= weight[inner])) ? leaf++ : inner++; };
    while (made < 2 * u - 1) {
        const int a = take(), b = take();
        weight[made] = weight[a] + weight[b];
        parent[a] = parent[b] = made++;
    }
    std::vector<int> depth(2 * u, 0), per_len(limit + 1, 0);
    for (int i = 2 * u - 3; i >= 0; --i) depth[i] = depth[parent[i]] + 1;
    for (int i = 0; i < u; ++i) ++per_len[depth[i] > limit ? limit : depth[i]];
    unsigned long long kraft = 0;  // in units of 2^-limit
    for (int l = 1; l <= limit; ++l) kraft += (unsigned long long)per_len[l] << (limit - l);
    while (kraft > (1ull << limit)) {
        --per_len[limit];
        for (int l = limit - 1; l >= 1; --l)
            if (per_len[l]) {
                --per_len[l];
                per_len[l + 1] += 2;
                break;
            }
        --kraft;
    }
    int at = u - 1;  // the most frequent symbol takes the shortest length
    for (int l = 1; l <= limit; ++l)
        for (int k = 0; k < per_len[l]; ++k) len[order[at--]] = (uint8_t)l;
}

// Canonical codes of these lengths, bit-reversed for LSB-first packing: code[s] | len[s] << 16, 0 for an unused symbol.
inline void canonical_codes(const uint8_t* len, int n, uint32_t* out) {
    uint32_t next[17] = {0}, per_len[17] = {0};
    for (int s = 0; s < n; ++s) ++per_len[len[s]];
    per_len[0] = 0;
    for (int l = 1; l <= 16; ++l) next[l] = (next[l - 1] + per_len[l - 1]) << 1;
    for (int s = 0; s < n; ++s) {
        out[s] = 0;
        if (!len[s]) continue;
        uint32_t c = next[len[s]]++, r = 0;
        for (int k = 0; k < len[s]; ++k) r |= ((c >> k) & 1u) << (len[s] - 1 - k);
        out[s] = r | ((uint32_t)len[s] << 16);
    }
}

// pp_deflate_build_code. lengths (may be NULL) <- the 286 code lengths.
inline void build_code(const uint32_t* hist, pp_deflate_code* code, uint8_t* lengths = nullptr) {
    static const uint8_t kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t count[DEFLATE_SYMS];
    for (int s = 0; s < DEFLATE_SYMS; ++s) count[s] = hist[s];
    if (!count[256]) count[256] = 1;
    uint8_t len[DEFLATE_SYMS + 1];
    build_lengths(count, DEFLATE_SYMS, 15, len);
    len[DEFLATE_SYMS] = 1;  // the one distance code
    if (lengths) std::memcpy(lengths, len, DEFLATE_SYMS);
    std::memset(code, 0, sizeof(*code));
    canonical_codes(len, DEFLATE_SYMS, code->sym);
    uint32_t cl_count[19] = {0}, cl_code[19];
    uint8_t cl_len[19];
    for (int i = 0; i <= DEFLATE_SYMS; ++i) ++cl_count[len[i]];
    build_lengths(cl_count, 19, 7, cl_len);
    canonical_codes(cl_len, 19, cl_code);
    LsbPacker p(code->header, 0, 76);
    p.put(0x0178u, 16);  // zlib: deflate, 32 KiB window, no dictionary, fastest
    p.put(1u, 1);        // BFINAL
    p.put(2u, 2);        // BTYPE: dynamic
    p.put(DEFLATE_SYMS - 257, 5);
    p.put(0u, 5);   // HDIST: one distance code
    p.put(15u, 4);  // HCLEN: all nineteen
    for (int i = 0; i < 19; ++i) p.put(cl_len[kOrder[i]], 3);
    for (int i = 0; i <= DEFLATE_SYMS; ++i) p.put(cl_code[len[i]] & 0xFFFFu, (int)(cl_code[len[i]] >> 16));
    code->header_bits = (uint32_t)(32 * p.widx + p.n);
    p.finish();
}

// One tile's spans on the host: start[p] / end[p] of every byte's run, then fn(w, cnt, p0, left_start, right_end) span by span.
template <class Fn>
inline void for_spans(const uint8_t* tile, int n, Fn fn) {
    int16_t start[PNG_TILE], end[PNG_TILE];
    for (int p = 0; p < n; ++p) start[p] = (int16_t)((p > 0 && tile[p] == tile[p - 1]) ? start[p - 1] : p);
    for (int p = n - 1; p >= 0; --p) end[p] = (int16_t)((p < n - 1 && tile[p] == tile[p + 1]) ? end[p + 1] : p);
    for (int p0 = 0; p0 < n; p0 += PNG_SPAN) {
        const int cnt = n - p0 < PNG_SPAN ? n - p0 : PNG_SPAN;
        uint32_t w[4] = {0, 0, 0, 0};
        for (int i = 0; i < cnt; ++i) w[i >> 2] |= (uint32_t)tile[p0 + i] << (8 * (i & 3));
        fn(w, cnt, p0, (int)start[p0], (int)end[p0 + cnt - 1]);
    }
}

// pp_zlib_compress: the phases of the kernels one after another.
inline int zlib_compress(const uint8_t* data, long long len, uint8_t* out, size_t capacity, size_t* size_out, long long* tokens_out) {
    const DefLayout L = def_layout(len);
    uint32_t hist[288] = {0};
    std::vector<uint32_t> s1(L.ntiles), s2(L.ntiles);
    for (long long t = 0; t < L.ntiles; ++t) {
        const int n = (int)(len - t * PNG_TILE < PNG_TILE ? len - t * PNG_TILE : PNG_TILE);
        HistSink h{hist};
        uint32_t a = 0, b = 0;
        for_spans(data + t * PNG_TILE, n, [&](const uint32_t (&w)[4], int cnt, int p0, int ls, int re) {
            span_tokens(w, cnt, p0, ls, re, h);
            uint32_t x, y;
            adler_span(w, cnt, n - p0, x, y);
            a += x, b += y;
        });
        s1[t] = a, s2[t] = b;
    }
    if (tokens_out) {
        *tokens_out = 0;
        for (int s = 0; s < DEFLATE_SYMS; ++s) *tokens_out += hist[s];
    }
    hist[256] += 1;
    pp_deflate_code code;
    build_code(hist, &code);
    unsigned long long lo = 1, hi = (unsigned long long)len % ADLER_MOD;
    for (long long t = 0; t < L.ntiles; ++t) {
        const long long behind = len - (t + 1) * PNG_TILE;
        lo += s1[t];
        hi += adler_term(s1[t], s2[t], behind > 0 ? (unsigned long long)behind : 0ull);
    }
    const uint32_t adler = (uint32_t)(hi % ADLER_MOD) << 16 | (uint32_t)(lo % ADLER_MOD);
    std::vector<uint32_t> words((size_t)L.nwords, 0u);
    for (int i = 0; i < (int)((code.header_bits + 31) / 32); ++i) or_word(words.data() + i, code.header[i]);
    unsigned long long at = code.header_bits;
    for (long long t = 0; t < L.ntiles; ++t) {
        const int n = (int)(len - t * PNG_TILE < PNG_TILE ? len - t * PNG_TILE : PNG_TILE);
        for_spans(data + t * PNG_TILE, n, [&](const uint32_t (&w)[4], int cnt, int p0, int ls, int re) {
            LsbCounter c;
            CodeSink<LsbCounter> count{code.sym, c};
            span_tokens(w, cnt, p0, ls, re, count);
            LsbPacker p(words.data(), at, L.nwords);
            CodeSink<LsbPacker> pack{code.sym, p};
            span_tokens(w, cnt, p0, ls, re, pack);
            at += c.bits;
            if (t * PNG_TILE + p0 + cnt == len) {
                put_tail(p, code.sym, adler);
                at = 32ull * (unsigned long long)p.widx + (unsigned)p.n;
            }
            p.finish();
        });
    }
    const size_t nbytes = (size_t)(at / 8);
    *size_out = nbytes;
    if (nbytes > capacity) return PP_ERR_WORKSPACE;
    std::memcpy(out, words.data(), nbytes);  // (little-endian words: the bytes in file order)
    return PP_OK;
}

// pp_deflate_build_code_lz. hist: LZ_HIST_WORDS counts. lengths (may be NULL) <- the 286 + 30 code lengths.
inline void build_code_lz(const uint32_t* hist, pp_deflate_code_lz* code, uint8_t* lengths = nullptr) {
    static const uint8_t kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t count[DEFLATE_SYMS];
    for (int s = 0; s < DEFLATE_SYMS; ++s) count[s] = hist[s];
    if (!count[256]) count[256] = 1;
    uint8_t len[DEFLATE_SYMS + LZ_DIST_SYMS];
    build_lengths(count, DEFLATE_SYMS, 15, len);
    build_lengths(hist + LZ_DIST_AT, LZ_DIST_SYMS, 15, len + DEFLATE_SYMS);
    if (lengths) std::memcpy(lengths, len, sizeof(len));
    int ndist = LZ_DIST_SYMS;
    while (!len[DEFLATE_SYMS + ndist - 1]) --ndist;  // (at least two symbols have a length)
    std::memset(code, 0, sizeof(*code));
    canonical_codes(len, DEFLATE_SYMS, code->base.sym);
    canonical_codes(len + DEFLATE_SYMS, LZ_DIST_SYMS, code->dist);
    uint32_t cl_count[19] = {0}, cl_code[19];
    uint8_t cl_len[19];
    for (int i = 0; i < DEFLATE_SYMS + ndist; ++i) ++cl_count[len[i]];
    build_lengths(cl_count, 19, 7, cl_len);
    canonical_codes(cl_len, 19, cl_code);
    LsbPacker p(code->base.header, 0, 76);
    p.put(0x0178u, 16);
    p.put(1u, 1);
    p.put(2u, 2);
    p.put(DEFLATE_SYMS - 257, 5);
    p.put((uint32_t)(ndist - 1), 5);  // HDIST
    p.put(15u, 4);
    for (int i = 0; i < 19; ++i) p.put(cl_len[kOrder[i]], 3);
    for (int i = 0; i < DEFLATE_SYMS + ndist; ++i) p.put(cl_code[len[i]] & 0xFFFFu, (int)(cl_code[len[i]] >> 16));
    code->base.header_bits = (uint32_t)(32 * p.widx + p.n);
    p.finish();
}

// The parse of one tile on the host: s: the whole stream, t0: the tile's first byte, n: its bytes; parse[0, n).
inline void lz_parse_tile(const uint8_t* s, long long t0, int n, const LzDist& D, uint16_t* parse) {
    std::vector<int16_t> nu((size_t)LZ_CANDS * (PNG_TILE + 1));
    std::vector<uint8_t> eq((size_t)LZ_CANDS * PNG_TILE);
    for (int c = 0; c < LZ_CANDS; ++c) {
        int16_t* u = nu.data() + (size_t)c * (PNG_TILE + 1);
        uint8_t* e = eq.data() + (size_t)c * PNG_TILE;
        u[n] = (int16_t)n;
        for (int p = n - 1; p >= 0; --p) {
            const long long g = t0 + p;
            e[p] = D.d[c] && g >= D.d[c] && s[g] == s[g - D.d[c]];
            u[p] = e[p] ? u[p + 1] : (int16_t)p;
        }
    }
    uint16_t tok[PNG_TILE + PNG_SPAN];
    for (int p0 = 0; p0 < n; p0 += PNG_SPAN) {
        const int cnt = n - p0 < PNG_SPAN ? n - p0 : PNG_SPAN;
        LzSpan sp;
        for (int c = 0; c < LZ_CANDS; ++c) {
            sp.eq[c] = 0;
            for (int i = 0; i < cnt; ++i) sp.eq[c] |= (uint32_t)eq[(size_t)c * PNG_TILE + p0 + i] << i;
            sp.nu_next[c] = nu[(size_t)c * (PNG_TILE + 1) + p0 + cnt];
        }
        lz_span_tokens(sp, cnt, p0, n, *reinterpret_cast<uint16_t(*)[PNG_SPAN]>(tok + p0));
    }
    for (int p = 0; p < n; ++p) parse[p] = 0;
    for (int p = 0; p < n; p += lz_step(tok[p])) parse[p] = tok[p];  // (the chain the kernel resolves by pointer doubling)
}

// pp_zlib_compress_lz: the phases of the kernels one after another.
inline int zlib_compress_lz(const uint8_t* data, long long len, long long period, uint8_t* out, size_t capacity, size_t* size_out, long long* tokens_out) {
    const LzLayout L = def_layout_lz(len);
    const LzDist D = lz_dists(period);
    uint32_t hist[LZ_HIST_WORDS] = {0};
    std::vector<uint16_t> parse((size_t)len);
    unsigned long long lo = 1, hi = (unsigned long long)len % ADLER_MOD;
    LzHistSink h{hist};
    for (long long t = 0; t < L.ntiles; ++t) {
        const long long t0 = t * PNG_TILE;
        const int n = (int)(len - t0 < PNG_TILE ? len - t0 : PNG_TILE);
        lz_parse_tile(data, t0, n, D, parse.data() + t0);
        uint32_t s1 = 0, s2 = 0;
        for (int p = 0; p < n; ++p) {
            lz_emit(parse[t0 + p], data[t0 + p], D, h);
            s1 += data[t0 + p];
            s2 += (uint32_t)data[t0 + p] * (uint32_t)(n - p);
        }
        const long long behind = len - (t + 1) * PNG_TILE;
        lo += s1;
        hi += adler_term(s1, s2, behind > 0 ? (unsigned long long)behind : 0ull);
    }
    if (tokens_out) {
        *tokens_out = 0;
        for (int s = 0; s < DEFLATE_SYMS; ++s) *tokens_out += hist[s];
    }
    hist[256] += 1;
    pp_deflate_code_lz code;
    build_code_lz(hist, &code);
    const uint32_t adler = (uint32_t)(hi % ADLER_MOD) << 16 | (uint32_t)(lo % ADLER_MOD);
    std::vector<uint32_t> words((size_t)L.nwords, 0u);
    for (int i = 0; i < (int)((code.base.header_bits + 31) / 32); ++i) or_word(words.data() + i, code.base.header[i]);
    LsbPacker p(words.data(), code.base.header_bits, L.nwords);
    LzCodeSink<LsbPacker> pack{code.base.sym, code.dist, p};
    for (long long g = 0; g < len; ++g) lz_emit(parse[g], data[g], D, pack);
    put_tail(p, code.base.sym, adler);
    const size_t nbytes = (size_t)((32ull * (unsigned long long)p.widx + (unsigned)p.n) / 8);
    p.finish();
    *size_out = nbytes;
    if (nbytes > capacity) return PP_ERR_WORKSPACE;
    std::memcpy(out, words.data(), nbytes);
    return PP_OK;
}

inline void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

inline uint32_t crc_bytes(uint32_t reg, const uint8_t* p, size_t n) {
    static const CrcTables T = crc_tables();
    for (size_t i = 0; i < n; ++i) reg = crc_byte(T.byte, reg, p[i]);
    return reg;
}

constexpr size_t PNG_HEAD = 41, PNG_TAIL = 16;  // signature, IHDR, IDAT's length and type | IDAT's CRC, IEND

// The filtered stream of a picture: height x (1 + 3 width) bytes.
inline void filter_picture(const uint8_t* pixels, int width, int height, long long row_stride, int rgb, uint8_t* stream) {
    const int nb = 3 * width;
    for (int y = 0; y < height; ++y) {
        const uint8_t* cur = pixels + (long long)y * row_stride;
        const uint8_t* up = y ? cur - row_stride : nullptr;
        uint32_t cost[5] = {0, 0, 0, 0, 0}, f[5];
        for (int i = 0; i < nb; ++i) {
            filter_all(cur, up, i, rgb, f);
            for (int t = 0; t < 5; ++t) cost[t] += filter_cost(f[t]);
        }
        const int type = filter_choice(cost);
        uint8_t* row = stream + (long long)y * (1 + nb);
        row[0] = (uint8_t)type;
        for (int i = 0; i < nb; ++i) {
            filter_all(cur, up, i, rgb, f);
            row[1 + i] = (uint8_t)f[type];
        }
    }
}

// pp_png_encode; lz: pp_png_encode_lz.
inline int encode_file(const uint8_t* pixels, int width, int height, long long row_stride, int rgb, uint8_t* out, size_t capacity, size_t* size_out,
                       bool lz = false) {
    const long long len = (long long)height * (1 + 3ll * width);
    std::vector<uint8_t> stream((size_t)len);
    filter_picture(pixels, width, height, row_stride, rgb, stream.data());
    *size_out = 0;
    if (capacity < PNG_HEAD + PNG_TAIL) return PP_ERR_WORKSPACE;
    size_t z = 0;
    const int st = lz ? zlib_compress_lz(stream.data(), len, 1 + 3ll * width, out + PNG_HEAD, capacity - PNG_HEAD - PNG_TAIL, &z, nullptr)
                      : zlib_compress(stream.data(), len, out + PNG_HEAD, capacity - PNG_HEAD - PNG_TAIL, &z, nullptr);
    *size_out = PNG_HEAD + z + PNG_TAIL;
    if (st != PP_OK) return st;
    static const uint8_t kSig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    std::memcpy(out, kSig, 8);
    put_be32(out + 8, 13);
    std::memcpy(out + 12, "IHDR", 4);
    put_be32(out + 16, (uint32_t)width);
    put_be32(out + 20, (uint32_t)height);
    out[24] = 8, out[25] = 2, out[26] = 0, out[27] = 0, out[28] = 0;  // 8 bits, truecolour, deflate, adaptive filtering, no interlace
    put_be32(out + 29, ~crc_bytes(~0u, out + 12, 17));
    put_be32(out + 33, (uint32_t)z);
    std::memcpy(out + 37, "IDAT", 4);
    uint8_t* tail = out + PNG_HEAD + z;
    put_be32(tail, ~crc_bytes(~0u, out + 37, 4 + z));
    put_be32(tail + 4, 0);
    std::memcpy(tail + 8, "IEND", 4);
    put_be32(tail + 12, ~crc_bytes(~0u, tail + 8, 4));
    return PP_OK;
}

}  // namespace png
}  // namespace pp
