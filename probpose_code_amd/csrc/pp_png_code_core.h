// The code build of the PNG writer as steps that a workgroup can run: what build_lengths, canonical_codes, build_code and
// build_code_lz (csrc/pp_png_core.h) compute with std::vector and std::stable_sort, restated over fixed-size arrays so that
// the same text runs in a kernel (png_code, csrc/pp_png.hip: one workgroup per stream, the work area in LDS) and one step
// after another on the host (pp_deflate_build_code_steps, scripts/png_code_host_check.cpp). The result is the
// pp_deflate_code / pp_deflate_code_lz of the host builders, byte for byte; they stay the reference.
//
// The steps are written once, against an executor that says how a step runs:
//   ex.each(n, f)             f(i) for every i in [0, n), in any order, then a barrier;
//   ex.one(f)                 f() once, then a barrier;
//   ex.offsets(n, bits, put)  put(i, the sum of bits(j) over j < i) for every i in [0, n), then a barrier; returns the total.
// SeqExec below is the host's (plain loops); the kernel's strides the items over its threads and scans by block_scan.
//
// What decides the bytes, as build_lengths states it: the order of the used symbols by (count, symbol number) - here the
// rank of a symbol is the number of keys below its own; the two-queue merge, a leaf taken when weight[leaf] <=
// weight[inner], inner nodes queued in the order they are made (one lane, 64-bit weights: 286 counts of 2^32 - 1 overflow
// 32 bits); the depth of every leaf (a walk up its parents: a parent's index is above its child's), clipped at the limit;
// the Kraft repair loop (one lane; its rounds that take a leaf from the level above the limit are done many at once);
// lengths handed out from the most frequent symbol down, by the prefix of the per-length counts; the canonical code of symbol s: the first code of its length plus the number of lower-numbered symbols of that
// length, bit-reversed.
//
// Bounds that hold whatever the counts are, and would hold if a step were wrong: a stored length is a loop index of at
// most `limit` (15, or 7 for the code-length code), so header_bits is at most 90 + 7 x the lengths written (and clamped to
// the mode's DEFLATE_HEADER_BITS on top); every index into the work area is checked against its array or is one by
// construction (a rank counts other symbols of the alphabet: below n); the header's words go through LsbPacker's cap.
#pragma once
#include "pp_png_core.h"

namespace pp {
namespace png {

constexpr int CODE_WORDS = (int)(sizeof(pp_deflate_code) / 4), CODE_WORDS_LZ = (int)(sizeof(pp_deflate_code_lz) / 4);
constexpr int CODE_FIXED_BITS = 16 + 3 + 14 + 19 * 3;  // the header in front of the lengths

// The work area of one stream's build: the kernel's LDS, the host function's stack.
struct CodeWork {
    unsigned long long weight[2 * DEFLATE_SYMS];  // leaves in rising order, then the inner nodes in the order they are made
    uint32_t count[288];                          // the counts of the alphabet in work
    uint32_t per_len[16];                         // symbols per length (after the repair: of the finished code)
    uint32_t cl_code[20];                         // the code-length code
    uint32_t u;                                   // symbols of the alphabet in work that take part
    uint32_t ndist;                               // distance lengths the header carries (runs mode: 1)
    uint16_t order[288];                          // rank -> symbol
    uint16_t parent[2 * DEFLATE_SYMS];
    uint8_t in_set[288];
    uint8_t len[DEFLATE_SYMS + LZ_DIST_SYMS + 4];  // the literal/length lengths, then the distance lengths (runs mode: the one 1)
    uint8_t cl_len[20];
    pp_deflate_code_lz out;  // built here, its zero words included, and copied whole (runs mode: its base)
};

struct SeqExec {
    template <class F>
    void each(int n, F f) {
        for (int i = 0; i < n; ++i) f(i);
    }
    template <class F>
    void one(F f) {
        f();
    }
    template <class B, class P>
    uint32_t offsets(int n, B bits, P put) {
        uint32_t at = 0;
        for (int i = 0; i < n; ++i) {
            put(i, at);
            at += bits(i);
        }
        return at;
    }
};

// The lowest `len` bits of c in reverse order (len 1 .. 16).
PP_HOST_DEVICE uint32_t reverse_bits(uint32_t c, int len) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(c) >> (32 - len);
#else
    uint32_t r = 0;
    for (int k = 0; k < len; ++k) r |= ((c >> k) & 1u) << (len - 1 - k);
    return r;
#endif
}

// The order in which the header carries the lengths of the code-length code.
PP_HOST_DEVICE int cl_order(int i) {
    constexpr uint8_t kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return kOrder[i];
}

// build_lengths: len[0, n) <- the code lengths of at most `limit` bits for w.count[0, n). n: 2 .. DEFLATE_SYMS; len may
// lie in w. Leaves w.per_len as the symbols per length of the code, which canonical_steps reads.
template <class Exec>
PP_HOST_DEVICE void lengths_steps(Exec& ex, CodeWork& w, int n, int limit, uint8_t* len) {
    ex.one([&] {
        w.u = 0;
        for (int l = 0; l < 16; ++l) w.per_len[l] = 0;
    });
    // a symbol's sort key: count << 9 | symbol number, all ones for a symbol that takes no part (kept in the inner nodes'
    // half of weight[], which the merge overwrites only after the ranks are taken)
    unsigned long long* key = w.weight + DEFLATE_SYMS;
    ex.each(n, [&](int s) {
        len[s] = 0;
        const bool used = w.count[s] != 0;
        w.in_set[s] = used ? 1 : 0;
        key[s] = used ? ((unsigned long long)w.count[s] << 9 | (unsigned)s) : ~0ull;
        if (used) add_word(&w.u, 1u);
    });
    ex.one([&] {  // with fewer than two used symbols the lowest unused ones are added
        for (int s = 0; w.u < 2 && s < n; ++s)
            if (!w.in_set[s]) {
                w.in_set[s] = 1;
                key[s] = (unsigned)s;
                ++w.u;
            }
    });
    ex.each(n, [&](int s) {  // the rank by (count, symbol number): the keys below this one
        if (!w.in_set[s]) return;
        const unsigned long long mine = key[s];
        int r = 0;
#pragma unroll 8
        for (int t = 0; t < n; ++t) r += key[t] < mine ? 1 : 0;
        w.order[r] = (uint16_t)s;
        w.weight[r] = w.count[s];
    });
    ex.one([&] {  // the two queues. Their heads l0, i0 and the weights behind them l1, i1 are held in registers, all ones for
                  // "none" (no weight reaches 2^41), so that a take is one comparison; it is written without branches, and
                  // l1, i1 are reloaded every take, a take before they are needed
        const int u = (int)w.u < n ? (int)w.u : n;
        const unsigned long long none = ~0ull;
        int leaf = 0, inner = u, made = u;
        unsigned long long l0 = w.weight[0], l1 = w.weight[1], i0 = none, i1 = none;
        while (made < 2 * u - 1) {
            unsigned long long sum = 0;
            for (int k = 0; k < 2; ++k) {
                const bool take_leaf = l0 <= i0;
                sum += take_leaf ? l0 : i0;
                w.parent[take_leaf ? leaf : inner] = (uint16_t)made;
                leaf += take_leaf ? 1 : 0;
                inner += take_leaf ? 0 : 1;
                l0 = take_leaf ? l1 : l0;
                i0 = take_leaf ? i0 : i1;
                const unsigned long long lb = w.weight[leaf + 1 < u ? leaf + 1 : 0], ib = w.weight[inner + 1 < made ? inner + 1 : 0];
                l1 = leaf + 1 < u ? lb : none;
                i1 = inner + 1 < made ? ib : none;
            }
            w.weight[made] = sum;
            if (inner == made) i0 = sum;  // the new node joins the queue of inner nodes
            else if (inner + 1 == made) i1 = sum;
            ++made;
        }
    });
    const int u = (int)w.u < n ? (int)w.u : n;
    ex.each(u, [&](int i) {  // a leaf's depth: the parents up to the root
        const int root = 2 * u - 2;
        int depth = 0;
        for (int k = i; k < root && depth < 2 * DEFLATE_SYMS; k = w.parent[k]) ++depth;
        add_word(&w.per_len[depth > limit ? limit : depth], 1u);
    });
    ex.one([&] {  // the Kraft sum in units of 2^-limit, brought back to 1
        unsigned long long kraft = 0;
        for (int l = 1; l <= limit; ++l) kraft += (unsigned long long)w.per_len[l] << (limit - l);
        while (kraft > (1ull << limit)) {
            if (w.per_len[limit - 1]) {  // as long as the level above the limit has leaves the loop below takes them: that many rounds at once
                const unsigned long long over = kraft - (1ull << limit);
                const uint32_t k = over < w.per_len[limit - 1] ? (uint32_t)over : w.per_len[limit - 1];
                w.per_len[limit - 1] -= k;
                w.per_len[limit] += k;
                kraft -= k;
                continue;
            }
            --w.per_len[limit];
            for (int l = limit - 1; l >= 1; --l)
                if (w.per_len[l]) {
                    --w.per_len[l];
                    w.per_len[l + 1] += 2;
                    break;
                }
            --kraft;
        }
    });
    ex.each(u, [&](int r) {  // the most frequent symbol takes the shortest length
        const uint32_t place = (uint32_t)(u - 1 - r);
        uint32_t upto = 0;
        int mine = 0;
        for (int l = 1; l <= limit; ++l) {
            if (!mine && place < upto + w.per_len[l]) mine = l;
            upto += w.per_len[l];
        }
        const int s = w.order[r];
        if (s < n) len[s] = (uint8_t)mine;
    });
}

// canonical_codes: out[s] <- the bit-reversed code of symbol s | len[s] << 16, 0 for an unused symbol; w.per_len: the
// symbols per length of len[0, n).
template <class Exec>
PP_HOST_DEVICE void canonical_steps(Exec& ex, const CodeWork& w, const uint8_t* len, int n, uint32_t* out) {
    ex.each(n, [&](int s) {
        const int l = len[s] < 16 ? len[s] : 0;
        uint32_t v = 0;
        if (l) {
            uint32_t c = 0;  // the first code of length l
            for (int j = 2; j <= l; ++j) c = (c + w.per_len[j - 1]) << 1;
#pragma unroll 8
            for (int t = 0; t < s; ++t) c += len[t] == l ? 1u : 0u;
            v = (reverse_bits(c, l) & 0xFFFFu) | ((uint32_t)l << 16);
        }
        out[s] = v;
    });
}

// build_code (LZ: build_code_lz) of hist (288 words, LZ: LZ_HIST_WORDS) into w.out.
template <bool LZ, class Exec>
PP_HOST_DEVICE void code_steps(Exec& ex, CodeWork& w, const uint32_t* hist) {
    ex.each(CODE_WORDS_LZ, [&](int i) { reinterpret_cast<uint32_t*>(&w.out)[i] = 0; });
    ex.each(DEFLATE_SYMS, [&](int s) {
        const uint32_t c = hist[s];
        w.count[s] = (s == 256 && !c) ? 1u : c;
    });
    lengths_steps(ex, w, DEFLATE_SYMS, 15, w.len);
    canonical_steps(ex, w, w.len, DEFLATE_SYMS, w.out.base.sym);
    if (LZ) {
        ex.each(LZ_DIST_SYMS, [&](int s) { w.count[s] = hist[LZ_DIST_AT + s]; });
        lengths_steps(ex, w, LZ_DIST_SYMS, 15, w.len + DEFLATE_SYMS);
        canonical_steps(ex, w, w.len + DEFLATE_SYMS, LZ_DIST_SYMS, w.out.dist);
        ex.one([&] {  // HDIST: the highest symbol with a length (at least two have one)
            int nd = LZ_DIST_SYMS;
            while (nd > 1 && !w.len[DEFLATE_SYMS + nd - 1]) --nd;
            w.ndist = (uint32_t)nd;
        });
    } else {
        ex.one([&] {
            w.len[DEFLATE_SYMS] = 1;  // the one distance code
            w.ndist = 1;
        });
    }
    const int ndist = (int)w.ndist <= LZ_DIST_SYMS ? (int)w.ndist : LZ_DIST_SYMS, nlen = DEFLATE_SYMS + ndist;
    ex.each(19, [&](int s) { w.count[s] = 0; });
    ex.each(nlen, [&](int i) { add_word(&w.count[w.len[i] & 15], 1u); });
    lengths_steps(ex, w, 19, 7, w.cl_len);
    canonical_steps(ex, w, w.cl_len, 19, w.cl_code);
    ex.one([&] {
        LsbPacker p(w.out.base.header, 0, 76);
        p.put(0x0178u, 16);  // zlib: deflate, 32 KiB window, no dictionary, fastest
        p.put(1u, 1);        // BFINAL
        p.put(2u, 2);        // BTYPE: dynamic
        p.put(DEFLATE_SYMS - 257, 5);
        p.put((uint32_t)(ndist - 1), 5);  // HDIST
        p.put(15u, 4);                    // HCLEN: all nineteen
        for (int i = 0; i < 19; ++i) p.put(w.cl_len[cl_order(i)] & 7u, 3);
        p.finish();
    });
    const uint32_t total = ex.offsets(
        nlen, [&](int i) { return w.cl_code[w.len[i] & 15] >> 16; },
        [&](int i, uint32_t before) {
            const uint32_t e = w.cl_code[w.len[i] & 15];
            LsbPacker p(w.out.base.header, CODE_FIXED_BITS + before, 76);
            p.put(e & 0xFFFFu, (int)(e >> 16));
            p.finish();
        });
    ex.one([&] {
        const uint32_t bits = CODE_FIXED_BITS + total, most = LZ ? DEFLATE_HEADER_BITS_LZ : DEFLATE_HEADER_BITS;
        w.out.base.header_bits = bits < most ? bits : most;
    });
}

// pp_deflate_build_code_steps / pp_deflate_build_code_steps_lz: the steps one after another.
inline void build_code_steps(const uint32_t* hist, pp_deflate_code* code) {
    CodeWork w;
    SeqExec ex;
    code_steps<false>(ex, w, hist);
    std::memcpy(code, &w.out.base, sizeof(*code));
}

inline void build_code_steps_lz(const uint32_t* hist, pp_deflate_code_lz* code) {
    CodeWork w;
    SeqExec ex;
    code_steps<true>(ex, w, hist);
    std::memcpy(code, &w.out, sizeof(*code));
}

}  // namespace png
}  // namespace pp
