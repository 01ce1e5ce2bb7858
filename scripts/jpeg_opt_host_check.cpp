// Stand-alone host check of the optimised Huffman tables (csrc/pp_jpeg_opt_core.h): the launches of
// csrc/pp_jpeg_entropy_opt.hip restated sequentially around the shared core - the histogram block by block through load_block
// and block_symbols (what jpeg_opt_hist runs), the table builder as jpeg_opt_build runs it (257 entries spread over 64 lanes,
// both minimum searches as reductions of opt_key, opt_merge_entry as a map, opt_limit_lengths, opt_rank, opt_code_of), and the
// coder's phases with the lookup that gives - compared with the host form: symbol_histogram, opt_build_table and the bytes of
// entropy_encode_opt. Cases: seeded coefficient arrays (sizes x samplings x densities x amplitudes), a 17 x 17 block plan whose
// luma AC table needs the 16-bit limit, and crafted histograms (Fibonacci counts over 24 symbols, equal counts, five-way
// ties, a single symbol, every symbol, sums near 2^32, a tree deeper than 32). What it does not run: the wave shuffles, the
// atomics and the grids - those are the GPU tests' (tests/test_jpeg_opt_gpu.py). A program for a sanitiser build on a CPU
// machine; no GPU is used:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_opt_host_check.cpp -o jpeg_opt_host_check
//   ./jpeg_opt_host_check        ->  "... cases, 0 failures"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../probpose_code_amd/csrc/pp_jpeg_enc_host.h"
#include "../probpose_code_amd/csrc/pp_jpeg_entropy_core.h"
#include "../probpose_code_amd/csrc/pp_jpeg_opt_core.h"

using namespace pp;

constexpr int LANES = 64, PER_LANE = (OPT_BINS + LANES - 1) / LANES;

struct BuiltTable {
    uint8_t bits[16], vals[256];
    uint32_t look[256];
    int nvals;
    bool deep;
};

// jpeg_opt_build, lane by lane.
static BuiltTable build_as_the_kernel(const uint32_t* hist) {
    BuiltTable T{};
    uint32_t freq[LANES][PER_LANE];
    int tree[LANES][PER_LANE], size[LANES][PER_LANE];
    for (int lane = 0; lane < LANES; ++lane)
        for (int e = 0; e < PER_LANE; ++e) {
            const int i = lane + LANES * e;
            freq[lane][e] = i < 256 ? hist[i] : (i == 256 ? 1u : 0u);
            tree[lane][e] = i;
            size[lane][e] = 0;
        }
    for (int merge = 0; merge < OPT_BINS - 1; ++merge) {
        unsigned long long k1 = OPT_NO_KEY, k2 = OPT_NO_KEY;
        for (int lane = 0; lane < LANES; ++lane)
            for (int e = 0; e < PER_LANE; ++e)
                if (freq[lane][e] && opt_key(freq[lane][e], lane + LANES * e) < k1) k1 = opt_key(freq[lane][e], lane + LANES * e);
        const int c1 = opt_key_symbol(k1);
        for (int lane = 0; lane < LANES; ++lane)
            for (int e = 0; e < PER_LANE; ++e) {
                const int i = lane + LANES * e;
                if (freq[lane][e] && i != c1 && opt_key(freq[lane][e], i) < k2) k2 = opt_key(freq[lane][e], i);
            }
        if (k2 == OPT_NO_KEY) break;
        const int c2 = opt_key_symbol(k2);
        for (int lane = 0; lane < LANES; ++lane)
            for (int e = 0; e < PER_LANE; ++e)
                opt_merge_entry(lane + LANES * e, c1, c2, opt_key_freq(k1), opt_key_freq(k2), freq[lane][e], tree[lane][e], size[lane][e]);
    }
    uint32_t count[OPT_MAX_CLEN + 1] = {};
    uint8_t size8[256];
    for (int lane = 0; lane < LANES; ++lane)
        for (int e = 0; e < PER_LANE; ++e) {
            const int i = lane + LANES * e, s = size[lane][e];
            if (i < OPT_BINS && s > 0) {
                if (s > OPT_MAX_CLEN) T.deep = true;
                else ++count[s];
            }
            if (i < 256) size8[i] = (uint8_t)(s > OPT_MAX_CLEN ? OPT_MAX_CLEN + 1 : s);
        }
    if (T.deep) return T;
    opt_limit_lengths(count);
    for (int l = 1; l <= 16; ++l) {
        T.bits[l - 1] = (uint8_t)count[l];
        T.nvals += (int)count[l];
    }
    OptCodeBase base;
    opt_code_base(T.bits, base);
    for (int i = 0; i < 256; ++i)
        if (size8[i]) {
            const int k = opt_rank(size8, i);
            if (k >= T.nvals) { std::printf("rank %d of symbol %d outside %d values\n", k, i, T.nvals); std::exit(1); }
            T.vals[k] = (uint8_t)i;
            T.look[i] = opt_code_of(base, T.bits, (uint32_t)k);
        }
    return T;
}

static int check_table(const char* what, const uint32_t* hist, BuiltTable* out = nullptr) {
    const BuiltTable T = build_as_the_kernel(hist);
    uint8_t bits[16], vals[256];
    int nvals = 0;
    const bool ok = opt_build_table(hist, bits, vals, &nvals);
    if (out) *out = T;
    if (ok == T.deep) { std::printf("%s: depth refusal differs\n", what); return 1; }
    if (!ok) return 0;
    if (nvals != T.nvals || std::memcmp(bits, T.bits, 16) || std::memcmp(vals, T.vals, 256)) { std::printf("%s: tables differ\n", what); return 1; }
    // the lookup is what ent_derive / EncTables::derive give for bits and vals; no code is all ones; Kraft's sum leaves room for one
    uint32_t want[256] = {};
    ent_derive(want, bits, vals);
    if (std::memcmp(want, T.look, sizeof(want))) { std::printf("%s: lookup differs\n", what); return 1; }
    unsigned long long kraft = 0;
    for (int l = 1; l <= 16; ++l) kraft += (unsigned long long)bits[l - 1] << (16 - l);
    if (nvals && kraft >= 65536) { std::printf("%s: no room for the pseudo-symbol\n", what); return 1; }
    for (int k = 0; k < nvals; ++k) {
        const uint32_t e = T.look[vals[k]], len = e >> 16;
        if (len < 1 || len > 16 || (e & 0xFFFFu) == (1u << len) - 1u) { std::printf("%s: bad code of symbol %d\n", what, vals[k]); return 1; }
    }
    int used = 0;
    for (int i = 0; i < 256; ++i) used += hist[i] != 0;
    if (used != nvals) { std::printf("%s: %d symbols, %d codes\n", what, used, nvals); return 1; }
    return 0;
}

struct Bins {
    uint32_t* dc_bins;
    uint32_t* ac_bins;
    void dc(int s) { ++dc_bins[s]; }
    void ac(int rs) { ++ac_bins[rs]; }
};

static int run_image(const pp_jpeg_info& info, const std::vector<int16_t>& coef, bool expect_limit) {
    uint16_t qt[192];
    jpeg::quality_tables(75, qt);
    std::vector<uint8_t> file((size_t)jpeg::encoded_bound(&info));
    size_t fsz = 0;
    if (jpeg::entropy_encode_opt(coef.data(), qt, &info, 0, file.data(), file.size(), &fsz) != PP_OK) { std::printf("host refused: %s\n", jpeg::g_reason); return 1; }
    pp_jpeg_ent_desc d{};
    d.coef = coef.data();
    d.hs = info.hs; d.vs = info.vs; d.mcus_x = info.mcus_x; d.mcus_y = info.mcus_y;
    uint8_t dummy; pp_jpeg_ent_result res;
    d.scratch = &dummy; d.out = &dummy; d.result = &res;
    const long long nblk = ent_blocks(d);
    if (nblk != info.coef_count / 64 || nblk > OPT_MAX_BLOCKS) { std::printf("nblk mismatch\n"); return 1; }
    // jpeg_opt_hist
    uint32_t hist[4][OPT_BINS] = {}, want[4][OPT_BINS];
    for (long long s = 0; s < nblk; ++s) {
        uint32_t w[32]; int pred, chroma;
        load_block(d, s, w, pred, chroma);
        Bins sink{hist[chroma ? OPT_DC_CHROMA : OPT_DC_LUMA], hist[chroma ? OPT_AC_CHROMA : OPT_AC_LUMA]};
        if (block_symbols(w, pred, sink)) { std::printf("bad coefficient\n"); return 1; }
    }
    if (jpeg::symbol_histogram(coef.data(), &info, 0, want) != PP_OK || std::memcmp(hist, want, sizeof(hist))) { std::printf("histogram differs\n"); return 1; }
    // jpeg_opt_build
    BuiltTable T[4];
    uint8_t bits[4][16], vals[4][256];
    for (int t = 0; t < 4; ++t) {
        if (check_table("image table", hist[t], &T[t])) return 1;
        if (T[t].nvals > ((t & 1) ? OPT_AC_SYMBOLS : OPT_DC_SYMBOLS)) { std::printf("more symbols than annex K\n"); return 1; }
        std::memcpy(bits[t], T[t].bits, 16);
        std::memcpy(vals[t], T[t].vals, 256);
    }
    if (expect_limit && T[OPT_AC_LUMA].bits[15] == 0) { std::printf("the case did not reach 16 bits\n"); return 1; }
    std::vector<uint8_t> hdr(2048);
    size_t hsz = 0;
    if (jpeg::write_headers_tables(qt, &info, 0, bits, vals, hdr.data(), hdr.size(), &hsz) != PP_OK || hsz > (size_t)jpeg::ENC_HEADER_BOUND) { std::printf("headers\n"); return 1; }
    if (hsz > fsz || std::memcmp(hdr.data(), file.data(), hsz) != 0) { std::printf("header mismatch\n"); return 1; }
    // the coder's phases with the record's lookup
    const EntLayout L = ent_layout(nblk);
    std::vector<uint32_t> len(nblk);
    unsigned long long tot = 0;
    for (long long s = 0; s < nblk; ++s) {
        uint32_t w[32]; int pred, chroma;
        load_block(d, s, w, pred, chroma);
        BitCounter c;
        if (code_block(w, pred, T[2 * chroma].look, T[2 * chroma + 1].look, c)) return 1;
        len[s] = c.bits;
        if (c.bits > (uint32_t)ENT_BLOCK_BITS) { std::printf("len over bound\n"); return 1; }
        tot += c.bits;
    }
    const unsigned long long nbytes = (tot + 7) >> 3;
    if ((long long)nbytes > L.max_bytes) { std::printf("stream over the scratch bound\n"); return 1; }
    std::vector<uint32_t> words(L.nwords, 0);
    unsigned long long at = 0;
    for (long long s = 0; s < nblk; ++s) {
        uint32_t w[32]; int pred, chroma;
        load_block(d, s, w, pred, chroma);
        BitPacker p(words.data(), at, L.nwords);
        code_block(w, pred, T[2 * chroma].look, T[2 * chroma + 1].look, p);
        if (s == nblk - 1 && p.phase()) p.put(0x7Fu, 8 - p.phase());
        p.finish();
        at += len[s];
    }
    std::vector<uint8_t> out;
    for (unsigned long long k = 0; k < nbytes; ++k) {
        const uint32_t b = stream_byte(words[k >> 2], (int)(k & 3));
        out.push_back((uint8_t)b);
        if (b == 255) out.push_back(0);
    }
    const size_t want_bytes = fsz - hsz - 2;
    if (out.size() != want_bytes || std::memcmp(out.data(), file.data() + hsz, want_bytes) != 0) {
        std::printf("MISMATCH %dx%d: got %zu want %zu\n", info.width, info.height, out.size(), want_bytes);
        return 1;
    }
    return 0;
}

static int run_random(int W, int H, int sub, double density, int amp, unsigned seed) {
    pp_jpeg_info info;
    if (jpeg::encode_plan(W, H, sub, &info) != PP_OK) return 1;
    std::mt19937 rng(seed);
    std::vector<int16_t> coef((size_t)info.coef_count, 0);
    std::uniform_real_distribution<double> u(0, 1);
    for (auto& c : coef)
        if (u(rng) < density) c = (int16_t)((int)(rng() % (2 * amp + 1)) - amp);
    for (size_t b = 0; b < coef.size() / 64; ++b) coef[b * 64] = (int16_t)((int)(rng() % 2001) - 1000);  // (DC differences stay legal)
    return run_image(info, coef, false);
}

// 17 x 17 blocks, 4:4:4: with the pseudo-symbol's 1 and EOB's 289 the luma AC counts are 1, 1, 2, 3, 5 ... 144, 289, 377, 666 ...:
// the unlimited tree is a chain 18 deep (tests/jpeg_opt_ref.length_limited_coefficients).
static int run_limited() {
    static const int counts[17] = {4461, 2752, 1709, 1043, 666, 377, 144, 89, 55, 34, 21, 13, 8, 5, 3, 2, 1};
    pp_jpeg_info info;
    if (jpeg::encode_plan(136, 136, 0, &info) != PP_OK) return 1;
    std::vector<int16_t> coef((size_t)info.coef_count, 0);
    long long b = 0;
    int k = 0, n = 0;
    for (int i = 0; i < 17; ++i) {
        const int run = i / 10, size = i % 10 + 1;  // (run, size) symbols, run 0 first
        for (int c = 0; c < counts[i]; ++c, ++n) {
            if (k + run + 1 > 62) { ++b; k = 0; }
            k += run + 1;
            coef[(size_t)b * 64 + jpeg::kNatural[k]] = (int16_t)((n & 1) ? (1 << size) - 1 : -(1 << (size - 1)));
        }
    }
    if (b >= 289) return 1;
    return run_image(info, coef, true);
}

static int run_histograms() {
    int fails = 0;
    uint32_t f[OPT_BINS];
    auto clear = [&] { std::memset(f, 0, sizeof(f)); };
    clear();  // Fibonacci counts over 24 symbols: 24 deep without the limit
    for (uint32_t i = 0, a = 1, b = 2; i < 24; ++i) { f[1 + 7 * i] = a; const uint32_t c = a + b; a = b; b = c; }
    BuiltTable T;
    fails += check_table("fibonacci", f, &T);
    if (T.bits[15] == 0) { std::printf("fibonacci: not limited\n"); ++fails; }
    clear();
    for (int i = 0; i < 16; ++i) f[3 * i + 1] = 7;
    fails += check_table("equal", f);
    clear();
    for (int i = 0; i < 200; ++i) f[i] = 1 + i / 5;
    fails += check_table("ties", f);
    clear();
    f[0x21] = 1000;
    fails += check_table("one", f, &T);
    if (T.nvals != 1 || T.bits[0] != 1 || T.look[0x21] != (1u << 16)) { std::printf("one: not the code 0\n"); ++fails; }
    clear();
    for (int i = 0; i < 256; ++i) f[i] = 1 + i;
    fails += check_table("full", f);
    for (int i = 0; i < 256; ++i) f[i] = 1;
    fails += check_table("full equal", f);
    clear();
    f[0] = 0xFFFFFFFFu - (1u << 30); f[1] = 1u << 29; f[2] = (1u << 29) - 1; f[0xF0] = 1;
    fails += check_table("near 2^32", f);
    clear();
    fails += check_table("empty", f);
    clear();  // forty Fibonacci counts: deeper than OPT_MAX_CLEN, refused by both forms
    for (uint32_t i = 0, a = 1, b = 2; i < 40; ++i) { f[i] = a; const uint32_t c = a + b; a = b; b = c; }
    fails += check_table("deep", f, &T);
    if (!T.deep) { std::printf("deep: not refused\n"); ++fails; }
    std::mt19937 rng(7);
    for (int r = 0; r < 200; ++r) {  // random histograms, many ties
        clear();
        const int nsym = 1 + (int)(rng() % 256), top = 1 + (int)(rng() % (r % 2 ? 4 : 100000));
        for (int i = 0; i < nsym; ++i) f[rng() % 256] = 1 + rng() % top;
        fails += check_table("random", f);
    }
    return fails;
}

int main() {
    int fails = run_histograms(), n = 210;
    fails += run_limited();
    ++n;
    const int sizes[][2] = {{1, 1}, {8, 8}, {17, 13}, {64, 96}, {250, 187}};
    unsigned seed = 1;
    for (auto& sz : sizes)
        for (int sub = 0; sub < 3; ++sub)
            for (double dens : {0.0, 0.01, 0.1, 1.0})
                for (int amp : {3, 1023}) { fails += run_random(sz[0], sz[1], sub, dens, amp, seed++); ++n; }
    // the oversize refusal, before any coefficient is read
    pp_jpeg_info huge;
    uint32_t hist[4][OPT_BINS];
    int16_t one[64] = {};
    if (jpeg::encode_plan(65535, 65535, 0, &huge) != PP_OK || jpeg::symbol_histogram(one, &huge, 0, hist) != PP_ERR_INVALID_ARG) { std::printf("oversize plan accepted\n"); ++fails; }
    ++n;
    std::printf("%d cases, %d failures\n", n, fails);
    return fails != 0;
}
