// Optimised Huffman tables for the JPEG writer: the symbol histogram of an image and libjpeg's jpeg_gen_optimal_table, in the
// pieces the host form (csrc/pp_jpeg_enc_host.h: pp_jpeg_symbol_histogram, pp_jpeg_optimal_table, pp_jpeg_entropy_encode_opt)
// and the kernels (csrc/pp_jpeg_entropy_opt.hip) share, and which scripts/jpeg_opt_host_check.cpp runs sequentially under
// sanitisers. Plain C++ that compiles for host and device; nothing here touches the GPU.
//
// Histogram: four tables of OPT_BINS = 257 bins in the order OPT_DC_LUMA, OPT_AC_LUMA, OPT_DC_CHROMA, OPT_AC_CHROMA, filled by
// the code walk of code_block (pp_jpeg_entropy_core.h): the DC category of the difference to the block before, (run << 4) |
// size per non-zero AC coefficient, 0xF0 per sixteen zeros in front of one, 0x00 unless zigzag 63 is non-zero. Categories
// are clamped as the coder clamps them (such an image is refused anyway). Bin 256 is libjpeg's pseudo-symbol, which keeps
// the all-ones code free; the builder sets it to 1 itself.
//
// Code lengths, as libjpeg builds them: the two least frequent non-zero entries are merged until one is left. Either search
// prefers, among equal frequencies, the LARGER symbol number (libjpeg scans upward with <=), the second skips the first's
// entry. That order is a total one on the key opt_key = frequency << 9 | (511 - symbol): both searches are minima of it,
// on the device wave reductions. libjpeg walks its others[] chain to lengthen every code of both trees; here every symbol
// carries the id of its tree (the entry that holds the tree's frequency), so the same step is a map over the 257 entries:
// opt_merge_entry. Then the lengths are counted, lengths above 16 are shortened by annex K.3's adjustment, one code is
// taken from the longest length in use (the pseudo-symbol's) and the symbols are ordered by their length BEFORE the
// adjustment, then by value (opt_limit_lengths, opt_rank).
//
// Frequencies are 32-bit: a plan of more than OPT_MAX_BLOCKS blocks (blocks x 64 > 2^32 - 1) is refused, and a table counts
// at most 63 symbols per block, so no bin and no merged sum wraps. (libjpeg ignores entries above 10^9 in its searches, which
// breaks its own tables for such images; that limit is not restated.)
// No optimised table has more symbols than its annex K counterpart: a DC table holds the categories 0..11 (12), an AC table
// the 160 (run, size) pairs with size 1..10, EOB and ZRL (162). So the marker segments stay within ENC_HEADER_BOUND, and with
// every length at most 16 bits ENT_BLOCK_BITS and pp_jpeg_encoded_bound hold as they stand.
#pragma once
#include <cstdint>

#include "pp_jpeg_entropy_core.h"

namespace pp {

constexpr int OPT_BINS = 257;
constexpr int OPT_DC_LUMA = 0, OPT_AC_LUMA = 1, OPT_DC_CHROMA = 2, OPT_AC_CHROMA = 3;
constexpr long long OPT_MAX_BLOCKS = 0xFFFFFFFFll / 64;
constexpr int OPT_MAX_CLEN = 32;  // libjpeg's MAX_CLEN: a deeper tree is an error there and a refusal here
constexpr int OPT_DC_SYMBOLS = 12, OPT_AC_SYMBOLS = 162;

// what probpose_code_amd/jpeg.py mirrors (_OPT_RECORD, _ENT_OPT_DESC)
static_assert(sizeof(pp_jpeg_opt_record) == 9344 && sizeof(pp_jpeg_ent_opt_desc) == 72, "jpeg.py mirrors these");
static_assert(offsetof(pp_jpeg_opt_record, bits) == 4112 && offsetof(pp_jpeg_opt_record, vals) == 4176 &&
                  offsetof(pp_jpeg_opt_record, lookup) == 5200 && offsetof(pp_jpeg_opt_record, status) == 9296,
              "histograms, bits, vals, lookup, status");

// The symbols of one block into `sink` (sink.dc(category), sink.ac(run_size)), in the order code_block codes them. Returns
// true for a coefficient no baseline code expresses (counted with its category clamped, as it is coded).
template <class Sink>
PP_HOST_DEVICE bool block_symbols(const uint32_t (&w)[32], int pred, Sink& sink) {
    bool bad = false;
    int s = ent_category((int)(int16_t)(w[0] & 0xFFFFu) - pred);
    if (s > 11) {
        bad = true;
        s = 11;
    }
    sink.dc(s);
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int i = jpeg::kNatural[k];
        const int a = (int)(int16_t)((w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
        if (a == 0) {
            ++run;
        } else {
            for (; run > 15; run -= 16) sink.ac(0xF0);
            s = ent_category(a);
            if (s > 10) {
                bad = true;
                s = 10;
            }
            sink.ac((run << 4) | s);
            run = 0;
        }
    }
    if (run > 0) sink.ac(0);
    return bad;
}

// The order both minimum searches of a merge use: smaller frequency first, among equals the larger symbol. freq != 0.
PP_HOST_DEVICE unsigned long long opt_key(uint32_t freq, int symbol) { return ((unsigned long long)freq << 9) | (unsigned)(511 - symbol); }
PP_HOST_DEVICE int opt_key_symbol(unsigned long long key) { return 511 - (int)(key & 511u); }
PP_HOST_DEVICE uint32_t opt_key_freq(unsigned long long key) { return (uint32_t)(key >> 9); }
constexpr unsigned long long OPT_NO_KEY = ~0ull;

// Entry i's share of the merge of tree c2 (frequency f2) into tree c1 (frequency f1).
PP_HOST_DEVICE void opt_merge_entry(int i, int c1, int c2, uint32_t f1, uint32_t f2, uint32_t& freq, int& tree, int& size) {
    if (i == c1) freq = f1 + f2;
    if (i == c2) freq = 0;
    if (tree == c1 || tree == c2) {
        ++size;
        tree = c1;
    }
}

// count[l]: symbols of code length l (0..OPT_MAX_CLEN, the pseudo-symbol among them) -> lengths of at most 16 by annex K.3,
// then one code less at the longest length in use.
PP_HOST_DEVICE void opt_limit_lengths(uint32_t (&count)[OPT_MAX_CLEN + 1]) {
    for (int i = OPT_MAX_CLEN; i > 16; --i)
        while (count[i] > 0) {
            int j = i - 2;
            while (j > 0 && count[j] == 0) --j;  // (a prefix of the pair's; j >= 1 while a pair hangs at length i)
            count[i] -= 2;
            count[i - 1] += 1;
            count[j + 1] += 2;
            count[j] -= 1;
        }
    int i = 16;
    while (i > 0 && count[i] == 0) --i;
    if (i > 0) --count[i];
}

// Where symbol i (code length size[i] > 0, i < 256) stands in huffval: behind every symbol with a shorter code and every
// smaller symbol with a code of the same length.
PP_HOST_DEVICE int opt_rank(const uint8_t* size, int i) {
    int r = 0;
    const int mine = size[i];
    for (int j = 0; j < 256; ++j) r += (size[j] != 0 && (size[j] < mine || (size[j] == mine && j < i))) ? 1 : 0;
    return r;
}

// The first code and the first huffval index of every length (1..16) of a table.
struct OptCodeBase {
    uint32_t code[17], first[17];
};

PP_HOST_DEVICE void opt_code_base(const uint8_t* bits, OptCodeBase& b) {
    uint32_t code = 0, k = 0;
    b.code[0] = b.first[0] = 0;
    for (int len = 1; len <= 16; ++len) {
        b.code[len] = code;
        b.first[len] = k;
        code = (code + bits[len - 1]) << 1;
        k += bits[len - 1];
    }
}

// code | length << 16 of huffval entry k.
PP_HOST_DEVICE uint32_t opt_code_of(const OptCodeBase& b, const uint8_t* bits, uint32_t k) {
    int len = 1;
    while (len < 16 && k >= b.first[len] + bits[len - 1]) ++len;
    return (b.code[len] + (k - b.first[len])) | ((uint32_t)len << 16);
}

// The whole builder, sequentially: freq[257] (bin 256 is overwritten with 1) -> bits[16], vals[256] (the first *nvals are
// set, the rest zero). Returns false for a tree deeper than OPT_MAX_CLEN (libjpeg's JERR_HUFF_CLEN_OVERFLOW).
inline bool opt_build_table(const uint32_t* freq_in, uint8_t* bits, uint8_t* vals, int* nvals) {
    uint32_t freq[OPT_BINS];
    int tree[OPT_BINS], size[OPT_BINS];
    for (int i = 0; i < OPT_BINS; ++i) {
        freq[i] = freq_in[i];
        tree[i] = i;
        size[i] = 0;
    }
    freq[256] = 1;
    for (;;) {
        unsigned long long k1 = OPT_NO_KEY, k2 = OPT_NO_KEY;
        for (int i = 0; i < OPT_BINS; ++i)
            if (freq[i] && opt_key(freq[i], i) < k1) k1 = opt_key(freq[i], i);
        const int c1 = opt_key_symbol(k1);
        for (int i = 0; i < OPT_BINS; ++i)
            if (freq[i] && i != c1 && opt_key(freq[i], i) < k2) k2 = opt_key(freq[i], i);
        if (k2 == OPT_NO_KEY) break;
        const int c2 = opt_key_symbol(k2);
        const uint32_t f1 = opt_key_freq(k1), f2 = opt_key_freq(k2);
        for (int i = 0; i < OPT_BINS; ++i) opt_merge_entry(i, c1, c2, f1, f2, freq[i], tree[i], size[i]);
    }
    uint32_t count[OPT_MAX_CLEN + 1] = {};
    uint8_t size8[256];
    for (int i = 0; i < OPT_BINS; ++i) {
        if (size[i] > OPT_MAX_CLEN) return false;
        if (size[i]) ++count[size[i]];
        if (i < 256) size8[i] = (uint8_t)size[i];
    }
    opt_limit_lengths(count);
    int n = 0;
    for (int l = 1; l <= 16; ++l) {
        bits[l - 1] = (uint8_t)count[l];
        n += (int)count[l];
    }
    for (int i = 0; i < 256; ++i) vals[i] = 0;
    for (int i = 0; i < 256; ++i)
        if (size8[i]) vals[opt_rank(size8, i)] = (uint8_t)i;
    *nvals = n;
    return true;
}

// ------------------------------------------------------------------------------------------------ the host form
namespace jpeg {

struct HistSink {
    uint32_t* dc_bins;
    uint32_t* ac_bins;
    void dc(int s) { ++dc_bins[s]; }
    void ac(int rs) { ++ac_bins[rs]; }
};

inline int check_opt_plan(const pp_jpeg_info* info, int restart_interval) {
    if (!plan_consistent(*info)) return enc_fail(PP_ERR_INVALID_ARG, "info is not a pp_jpeg_encode_plan result");
    if (restart_interval < 0 || restart_interval > 65535) return enc_fail(PP_ERR_INVALID_ARG, "restart interval outside 0..65535");
    if (info->coef_count / 64 > OPT_MAX_BLOCKS) return enc_fail(PP_ERR_INVALID_ARG, "too many blocks for 32-bit symbol frequencies");
    return PP_OK;
}

// pp_jpeg_symbol_histogram: the scan of entropy_encode, counted instead of coded (no alignment is asked of coef).
inline int symbol_histogram(const int16_t* coef, const pp_jpeg_info* info, int restart_interval, uint32_t (*hist)[OPT_BINS]) {
    if (!coef || !info || !hist) return enc_fail(PP_ERR_INVALID_ARG, "NULL argument");
    if (const int st = check_opt_plan(info, restart_interval)) return st;
    std::memset(hist, 0, 4 * OPT_BINS * sizeof(uint32_t));
    const int16_t* plane[3];
    long long off = 0;
    for (int c = 0; c < 3; ++c) {
        plane[c] = coef + off;
        off += (long long)info->comp_bw[c] * info->comp_bh[c] * 64;
    }
    int pred[3] = {0, 0, 0};
    long long mcu = 0;
    bool bad = false;
    for (int my = 0; my < info->mcus_y; ++my)
        for (int mx = 0; mx < info->mcus_x; ++mx, ++mcu) {
            if (restart_interval && mcu % restart_interval == 0) pred[0] = pred[1] = pred[2] = 0;
            for (int c = 0; c < 3; ++c) {
                const int h = c ? 1 : info->hs, v = c ? 1 : info->vs;
                HistSink sink{hist[c ? OPT_DC_CHROMA : OPT_DC_LUMA], hist[c ? OPT_AC_CHROMA : OPT_AC_LUMA]};
                for (int bv = 0; bv < v; ++bv)
                    for (int bh = 0; bh < h; ++bh) {
                        const int16_t* blk = plane[c] + ((long long)(my * v + bv) * info->comp_bw[c] + (mx * h + bh)) * 64;
                        uint32_t w[32];
                        for (int i = 0; i < 32; ++i) w[i] = (uint32_t)(uint16_t)blk[2 * i] | ((uint32_t)(uint16_t)blk[2 * i + 1] << 16);
                        bad |= block_symbols(w, pred[c], sink);
                        pred[c] = blk[0];
                    }
            }
        }
    if (bad) return enc_fail(PP_ERR_INVALID_ARG, "a coefficient no baseline code expresses (DC difference beyond 2047 or AC beyond 1023)");
    return PP_OK;
}

// pp_jpeg_optimal_table
inline int optimal_table(const uint32_t* freq, uint8_t* bits, uint8_t* vals, int* nvals) {
    if (!freq || !bits || !vals || !nvals) return enc_fail(PP_ERR_INVALID_ARG, "NULL argument");
    if (!opt_build_table(freq, bits, vals, nvals)) return enc_fail(PP_ERR_INVALID_ARG, "code tree deeper than 32");
    return PP_OK;
}

// The tables of a file as the entry points pass them: bits[4][16], vals[4][256]. False for a table that is no prefix code.
inline bool spec_of(const uint8_t (*bits)[16], const uint8_t (*vals)[256], HuffSpec& spec) {
    for (int t = 0; t < 4; ++t) {
        int n = 0;
        long long room = 1;  // codes left at the current length
        for (int l = 0; l < 16; ++l) {
            room = 2 * room - bits[t][l];
            if (room < 0) return false;
            n += bits[t][l];
        }
        if (n > 256) return false;
        spec.bits[t] = bits[t];
        spec.vals[t] = vals[t];
        spec.nvals[t] = n;
    }
    return true;
}

// pp_jpeg_write_headers_tables
inline int write_headers_tables(const uint16_t* qtables, const pp_jpeg_info* info, int restart_interval, const uint8_t (*bits)[16],
                                const uint8_t (*vals)[256], uint8_t* out, size_t capacity, size_t* size_out) {
    if (!qtables || !info || !bits || !vals || !out || !size_out) return enc_fail(PP_ERR_INVALID_ARG, "NULL argument");
    *size_out = 0;
    HuffSpec spec;
    if (!spec_of(bits, vals, spec)) return enc_fail(PP_ERR_INVALID_ARG, "a Huffman table that is no prefix code of at most 256 symbols");
    return write_headers(qtables, info, restart_interval, out, capacity, size_out, spec);
}

// pp_jpeg_entropy_encode_opt: the histograms, the four tables, then entropy_encode's file with them.
inline int entropy_encode_opt(const int16_t* coef, const uint16_t* qtables, const pp_jpeg_info* info, int restart_interval, uint8_t* out,
                              size_t capacity, size_t* size_out) {
    if (!coef || !qtables || !info || !out || !size_out) return enc_fail(PP_ERR_INVALID_ARG, "NULL argument");
    *size_out = 0;
    if (const int st = check_file_args(qtables, info, restart_interval)) return st;
    uint32_t hist[4][OPT_BINS];
    if (const int st = symbol_histogram(coef, info, restart_interval, hist)) return st;
    uint8_t bits[4][16], vals[4][256];
    HuffSpec spec;
    for (int t = 0; t < 4; ++t) {
        if (const int st = optimal_table(hist[t], bits[t], vals[t], &spec.nvals[t])) return st;
        // the bound of the header segments: no more symbols than the annex K table
        if (spec.nvals[t] > ((t & 1) ? OPT_AC_SYMBOLS : OPT_DC_SYMBOLS)) return enc_fail(PP_ERR_INVALID_ARG, "more symbols than an annex K table");
        spec.bits[t] = bits[t];
        spec.vals[t] = vals[t];
    }
    const EncTables tables(spec);
    return entropy_encode_with(coef, qtables, info, restart_interval, out, capacity, size_out, spec, tables);
}

}  // namespace jpeg
}  // namespace pp
