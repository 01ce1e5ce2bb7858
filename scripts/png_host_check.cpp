// Stand-alone host check of the device PNG writer (csrc/pp_png.hip): the sequential form of its core (csrc/pp_png_core.h:
// the filters and the choice, the token rule, the bit packer, the code builder and header writer, the Adler-32 and CRC-32
// partials and their combination - the code the kernels run) over seeded streams and pictures, judged by the system zlib:
//   - streams (runs of 1, 2, 3, 4, 258 .. 262, 517 .. 520 and 4096 bytes, a run across a tile border, one byte, one value,
//     all 256 values with every length symbol, noise, sizes around the tile): uncompress() returns the input, the Adler-32
//     is zlib's, the token count is that of a walk over the runs written here, the size stays inside pp_deflate_bound's rule;
//   - pictures (1x1, 1x7, 7x1, 150x201, W = 1365 and 1366, zeros, 255s, noise, ramps, both channel orders, a strided view):
//     every chunk's CRC is crc32()'s, the IDAT inflates to the filtered stream, and that unfilters to the pixels;
//   - histograms (Fibonacci counts, two symbols, one symbol, all 286 equal, no match): lengths of at most 15 bits, Kraft
//     sum exactly 1, the same code twice;
//   - the CRC-32 of a buffer cut into chunks and combined by crc_shift / crc_mul equals crc32();
//   - lz mode (zlib_compress_lz, encode_file with lz, build_code_lz): the same streams with and without a row period, rows
//     that repeat the row above, far sources in earlier tiles (a period of 4096 and of 5000), a distance with 13 extra bits
//     (30300), matches cut at a tile border, a last tile of one byte, positions before the first source; pictures whose
//     filtered rows repeat: uncompress() returns the input, nothing is written behind the size, the size stays inside
//     deflate_bound_lz, a capacity one byte short is refused with the need; both codes complete and at most 15 bits.
// What it does not run: the workgroup scans and the grids - those are the GPU tests' (tests/test_png_gpu.py). A program for a
// sanitiser build on a CPU machine; no GPU is used:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/png_host_check.cpp -lz -o png_host_check
//   ./png_host_check        ->  "609 cases, 0 failures"
#include <zlib.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../probpose_code_amd/csrc/pp_png_core.h"

using namespace pp::png;

static int g_cases = 0, g_fails = 0;

static void fail(const char* what, const char* name) {
    std::printf("FAIL %s: %s\n", name, what);
    ++g_fails;
}

// The tokens of a stream by a walk over its runs.
static long long tokens_by_runs(const std::vector<uint8_t>& d) {
    long long tokens = 0;
    for (size_t t0 = 0; t0 < d.size(); t0 += PNG_TILE) {
        const size_t t1 = std::min(d.size(), t0 + PNG_TILE);
        for (size_t p = t0; p < t1;) {
            size_t q = p;
            while (q + 1 < t1 && d[q + 1] == d[p]) ++q;
            long long rest = (long long)(q - p);  // bytes behind the literal
            ++tokens;
            while (rest > 0) {
                const long long m = std::min(rest, 258ll);
                tokens += m >= 3 ? 1 : m;
                rest -= m;
            }
            p = q + 1;
        }
    }
    return tokens;
}

static void check_stream(const char* name, const std::vector<uint8_t>& d) {
    ++g_cases;
    const long long bound = deflate_bound((long long)d.size());
    std::vector<uint8_t> z((size_t)bound + 16, 0xA5);
    size_t zs = 0;
    long long tokens = -1;
    if (zlib_compress(d.data(), (long long)d.size(), z.data(), (size_t)bound, &zs, &tokens) != PP_OK) return fail("refused", name);
    for (size_t i = zs; i < z.size(); ++i)
        if (z[i] != 0xA5) return fail("wrote behind its size", name);
    std::vector<uint8_t> back(d.size() + 1);
    uLongf n = (uLongf)back.size();
    if (uncompress(back.data(), &n, z.data(), (uLong)zs) != Z_OK) return fail("zlib does not inflate it", name);
    if (n != d.size() || std::memcmp(back.data(), d.data(), d.size()) != 0) return fail("inflates to other bytes", name);
    if (tokens != tokens_by_runs(d)) return fail("token count", name);
    size_t need = 0;
    if (zs > 1 && zlib_compress(d.data(), (long long)d.size(), z.data(), zs - 1, &need, nullptr) != PP_ERR_WORKSPACE) return fail("one byte short accepted", name);
    if (zs > 1 && need != zs) return fail("needed size", name);
}

static void check_stream_lz(const char* name, const std::vector<uint8_t>& d, long long period) {
    ++g_cases;
    const long long bound = deflate_bound_lz((long long)d.size());
    std::vector<uint8_t> z((size_t)bound + 16, 0xA5);
    size_t zs = 0;
    long long tokens = -1;
    if (zlib_compress_lz(d.data(), (long long)d.size(), period, z.data(), (size_t)bound, &zs, &tokens) != PP_OK) return fail("lz: refused", name);
    for (size_t i = zs; i < z.size(); ++i)
        if (z[i] != 0xA5) return fail("lz: wrote behind its size", name);
    std::vector<uint8_t> back(d.size() + 1);
    uLongf n = (uLongf)back.size();
    if (uncompress(back.data(), &n, z.data(), (uLong)zs) != Z_OK) return fail("lz: zlib does not inflate it", name);
    if (n != d.size() || std::memcmp(back.data(), d.data(), d.size()) != 0) return fail("lz: inflates to other bytes", name);
    if (tokens < 1 || tokens > (long long)d.size()) return fail("lz: token count", name);
    if (period == 0 && tokens > tokens_by_runs(d)) return fail("lz: more tokens than the run rule", name);  // (distance 1 is a candidate)
    size_t need = 0;
    if (zs > 1 && zlib_compress_lz(d.data(), (long long)d.size(), period, z.data(), zs - 1, &need, nullptr) != PP_ERR_WORKSPACE) return fail("lz: one byte short accepted", name);
    if (zs > 1 && need != zs) return fail("lz: needed size", name);
}

static void check_histogram_lz(const char* name, const std::vector<uint32_t>& hist) {
    ++g_cases;
    pp_deflate_code_lz a, b;
    uint8_t len[DEFLATE_SYMS + LZ_DIST_SYMS];
    build_code_lz(hist.data(), &a, len);
    build_code_lz(hist.data(), &b);
    if (std::memcmp(&a, &b, sizeof(a)) != 0) return fail("lz: not deterministic", name);
    unsigned long long kraft = 0, dkraft = 0;
    for (int s = 0; s < DEFLATE_SYMS + LZ_DIST_SYMS; ++s) {
        if (len[s] > 15) return fail("lz: length above 15", name);
        if (len[s]) (s < DEFLATE_SYMS ? kraft : dkraft) += 1ull << (15 - len[s]);
        if (s >= DEFLATE_SYMS && hist[LZ_DIST_AT + s - DEFLATE_SYMS] && !len[s]) return fail("lz: used distance without a code", name);
    }
    if (kraft != 1ull << 15 || dkraft != 1ull << 15) return fail("lz: Kraft sum is not 1", name);
    if (a.base.header_bits > (uint32_t)DEFLATE_HEADER_BITS_LZ) return fail("lz: header too long", name);
}

static std::vector<uint8_t> runs_of(std::initializer_list<int> lengths, int lead = 0) {
    std::vector<uint8_t> d((size_t)lead);
    for (size_t i = 0; i < d.size(); ++i) d[i] = (uint8_t)(i * 7 + 1);
    uint8_t v = 200;
    for (int L : lengths) {
        d.insert(d.end(), (size_t)L, v);
        v = (uint8_t)(v + 13);
    }
    return d;
}

static void check_picture(const char* name, const std::vector<uint8_t>& px, int W, int H, long long stride, int rgb, bool lz = false) {
    ++g_cases;
    const long long len = (long long)H * (1 + 3ll * W);
    std::vector<uint8_t> file(PNG_HEAD + PNG_TAIL + (size_t)(lz ? deflate_bound_lz(len) : deflate_bound(len)));
    size_t fs = 0;
    if (encode_file(px.data(), W, H, stride, rgb, file.data(), file.size(), &fs, lz) != PP_OK) return fail("refused", name);
    size_t at = 8;
    std::vector<uint8_t> idat;
    int chunks = 0;
    while (at + 12 <= fs) {
        const uint32_t len = (uint32_t)file[at] << 24 | file[at + 1] << 16 | file[at + 2] << 8 | file[at + 3];
        if (at + 12 + len > fs) return fail("chunk runs over the file", name);
        const uint32_t crc = (uint32_t)file[at + 8 + len] << 24 | file[at + 9 + len] << 16 | file[at + 10 + len] << 8 | file[at + 11 + len];
        if (crc != crc32(0, file.data() + at + 4, 4 + len)) return fail("chunk CRC", name);
        if (std::memcmp(file.data() + at + 4, "IDAT", 4) == 0) idat.assign(file.begin() + at + 8, file.begin() + at + 8 + len);
        at += 12 + len;
        ++chunks;
    }
    if (at != fs || chunks != 3) return fail("framing", name);
    const size_t nb = 3 * (size_t)W;
    std::vector<uint8_t> want((size_t)H * (1 + nb)), got(want.size());
    filter_picture(px.data(), W, H, stride, rgb, want.data());
    uLongf n = (uLongf)got.size();
    if (uncompress(got.data(), &n, idat.data(), (uLong)idat.size()) != Z_OK || n != got.size()) return fail("IDAT does not inflate", name);
    if (got != want) return fail("IDAT is not the filtered stream", name);
    std::vector<uint8_t> prev(nb, 0), row(nb);
    for (int y = 0; y < H; ++y) {  // unfilter, by the specification's rules
        const uint8_t* f = got.data() + (size_t)y * (1 + nb);
        for (size_t i = 0; i < nb; ++i) {
            const int a = i >= 3 ? row[i - 3] : 0, b = prev[i], c = i >= 3 ? prev[i - 3] : 0;
            int pred = 0;
            if (f[0] == 1) pred = a;
            else if (f[0] == 2) pred = b;
            else if (f[0] == 3) pred = (a + b) / 2;
            else if (f[0] == 4) {
                const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
                pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
            } else if (f[0] != 0) return fail("filter type", name);
            row[i] = (uint8_t)(f[1 + i] + pred);
        }
        for (size_t i = 0; i < nb; ++i)
            if (row[i] != px[(size_t)y * stride + i / 3 * 3 + (rgb ? i % 3 : 2 - i % 3)]) return fail("pixels", name);
        prev = row;
    }
}

static void check_histogram(const char* name, const std::vector<uint32_t>& hist) {
    ++g_cases;
    pp_deflate_code a, b;
    uint8_t len[DEFLATE_SYMS];
    build_code(hist.data(), &a, len);
    build_code(hist.data(), &b);
    if (std::memcmp(&a, &b, sizeof(a)) != 0) return fail("not deterministic", name);
    unsigned long long kraft = 0;
    for (int s = 0; s < DEFLATE_SYMS; ++s) {
        if (len[s] > 15) return fail("length above 15", name);
        if (len[s]) kraft += 1ull << (15 - len[s]);
        if ((hist[s] || s == 256) && !len[s]) return fail("used symbol without a code", name);
    }
    if (kraft != 1ull << 15) return fail("Kraft sum is not 1", name);
    if (a.header_bits > (uint32_t)DEFLATE_HEADER_BITS) return fail("header too long", name);
}

int main() {
    std::mt19937 rng(7);
    check_stream("runs 1 2 3 4", runs_of({1, 2, 3, 4}));
    check_stream("runs 258..262", runs_of({258, 259, 260, 261, 262}));
    check_stream("runs 517..520", runs_of({517, 518, 519, 520}));
    check_stream("run 4096", runs_of({4096}));
    check_stream("run 4096 + 1", runs_of({4097}));
    check_stream("run across a tile border", runs_of({600}, 3800));
    check_stream("one byte", {42});
    check_stream("one value", std::vector<uint8_t>(10000, 0));
    {
        std::vector<uint8_t> d;
        for (int v = 0; v < 256; ++v) d.push_back((uint8_t)v);
        for (int m = 3; m <= 258; ++m) {  // a run of 1 + m: every match length, so every length symbol
            d.insert(d.end(), (size_t)m + 1, (uint8_t)(m * 5));
            d.push_back((uint8_t)(m * 5 + 1));
        }
        check_stream("all values, every length", d);
    }
    for (int n : {2, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 70000}) {
        std::vector<uint8_t> d((size_t)n);
        for (auto& b : d) b = (uint8_t)rng();
        check_stream("noise", d);
        for (auto& b : d) b = (uint8_t)((rng() % 16 == 0) ? rng() : 0);
        check_stream("sparse", d);
        for (auto& b : d) b = (uint8_t)(rng() % 3);
        check_stream("three values", d);
    }
    const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {150, 201}, {1365, 3}, {1366, 3}, {64, 48}};
    for (auto& sz : sizes) {
        const int W = sz[0], H = sz[1];
        for (int kind = 0; kind < 7; ++kind) {
            const long long stride = 3ll * W + (kind == 6 ? 9 : 0);
            std::vector<uint8_t> px((size_t)(stride * H));
            for (int y = 0; y < H; ++y)
                for (int i = 0; i < stride; ++i) {
                    uint8_t v = 0;
                    if (kind == 1) v = 255;
                    else if (kind == 2 || kind == 6) v = (uint8_t)rng();
                    else if (kind == 3) v = (uint8_t)(i / 3);
                    else if (kind == 4) v = (uint8_t)(y * 3);
                    else if (kind == 5) v = (uint8_t)(128 + 60 * std::sin(0.05 * i + 0.11 * y) + (int)(rng() % 5));
                    px[(size_t)(y * stride + i)] = v;
                }
            check_picture("picture bgr", px, W, H, stride, 0);
            check_picture("picture rgb", px, W, H, stride, 1);
            check_picture("lz picture rgb", px, W, H, stride, 1, true);
            for (int y = 1; y < H; ++y)  // every row the row above plus 128: the filtered rows repeat (Sub), the far candidates match
                for (int i = 0; i < stride; ++i) px[(size_t)(y * stride + i)] = (uint8_t)(px[(size_t)((y - 1) * stride + i)] + 128);
            check_picture("lz picture of repeating rows", px, W, H, stride, 0, true);
        }
    }
    // lz mode: the streams above again, and what only it can get wrong
    check_stream_lz("runs 258..262", runs_of({258, 259, 260, 261, 262}), 0);
    check_stream_lz("run 4096 + 1", runs_of({4097}), 7);
    check_stream_lz("run across a tile border", runs_of({600}, 3800), 100);
    check_stream_lz("one byte", {42}, 0);
    check_stream_lz("one byte with a period", {42}, 4);
    for (int n : {2, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 70000}) {
        std::vector<uint8_t> d((size_t)n);
        for (long long period : {0ll, 4ll, 100ll, 4096ll, 5000ll, 32768ll, 32771ll, 40000ll}) {
            for (auto& b : d) b = (uint8_t)rng();
            check_stream_lz("noise", d, period);
            for (auto& b : d) b = (uint8_t)((rng() % 16 == 0) ? rng() : 0);
            check_stream_lz("sparse", d, period);
            // rows of `period` bytes that repeat the row above but for a few bytes: far matches, sources in earlier tiles
            for (size_t i = 0; i < d.size(); ++i)
                d[i] = (period > 0 && i >= (size_t)period && rng() % 40) ? d[i - (size_t)period] : (uint8_t)(rng() % 7 ? rng() : d[i ? i - 1 : 0]);
            check_stream_lz("repeating rows", d, period);
            for (size_t i = 3; i < d.size(); ++i)
                if (rng() % 5) d[i] = d[i - 3];  // equal pixels: distance 3
            check_stream_lz("pixel runs", d, period);
        }
    }
    {
        std::vector<uint8_t> d(30300 + 400);  // a repeat 30300 bytes back: distance symbol 29, 13 extra bits
        for (auto& b : d) b = (uint8_t)rng();
        std::memcpy(d.data() + 30300, d.data(), 400);
        check_stream_lz("13 extra bits", d, 30300);
        check_stream_lz("13 extra bits by P - 3", d, 30303);
        check_stream_lz("13 extra bits by P + 3", d, 30297);
        d.resize(2 * PNG_TILE + 1);  // a last tile of one byte; a far match (period 100) that would cross the first border
        std::memcpy(d.data() + PNG_TILE - 10, d.data() + PNG_TILE - 110, 40);
        check_stream_lz("a match at a tile border, a last tile of one byte", d, 100);
    }
    {
        std::vector<uint32_t> h(LZ_HIST_WORDS, 0);
        check_histogram_lz("nothing used", h);
        h[LZ_DIST_AT + 12] = 5;
        check_histogram_lz("one distance", h);
        uint32_t a = 1, b = 1;
        for (int s = 0; s < 30; ++s) {
            h[s] = h[LZ_DIST_AT + s] = a;
            const uint32_t c = a + b;
            a = b, b = c;
        }
        check_histogram_lz("Fibonacci counts in both alphabets", h);
        for (int s = 0; s < DEFLATE_SYMS; ++s) h[s] = 1 + rng() % 1000;
        for (int s = 0; s < LZ_DIST_SYMS; ++s) h[LZ_DIST_AT + s] = 1 + rng() % 1000;
        check_histogram_lz("everything used", h);
    }
    {
        std::vector<uint32_t> h(DEFLATE_SYMS, 0);
        uint32_t a = 1, b = 1;
        for (int s = 0; s < 40; ++s) {
            h[s] = a;
            const uint32_t c = a + b;
            a = b, b = c;
        }
        check_histogram("Fibonacci counts", h);
        h.assign(DEFLATE_SYMS, 0);
        h[65] = 9, h[256] = 1;
        check_histogram("two symbols", h);
        h.assign(DEFLATE_SYMS, 0);
        check_histogram("the end of block alone", h);
        h.assign(DEFLATE_SYMS, 77);
        check_histogram("all equal", h);
        for (int s = 257; s < DEFLATE_SYMS; ++s) h[s] = 0;
        for (int s = 0; s < 256; ++s) h[s] = 1 + rng() % 1000;
        check_histogram("no match", h);
    }
    {
        ++g_cases;
        static const CrcTables T = crc_tables();
        std::vector<uint8_t> d(100003);
        for (auto& b : d) b = (uint8_t)rng();
        const uint32_t init = ~(uint32_t)crc32(0, reinterpret_cast<const Bytef*>("IDAT"), 4);
        uint32_t reg = crc_mul(crc_shift(T.x2n, d.size()), init);
        for (size_t at = 0; at < d.size(); at += 4096) {
            const size_t n = std::min<size_t>(4096, d.size() - at);
            reg ^= crc_mul(crc_shift(T.x2n, d.size() - at - n), crc_bytes(0u, d.data() + at, n));
        }
        if (~reg != (uint32_t)crc32(crc32(0, reinterpret_cast<const Bytef*>("IDAT"), 4), d.data(), (uInt)d.size())) fail("combination", "CRC-32");
    }
    std::printf("%d cases, %d failures\n", g_cases, g_fails);
    return g_fails != 0;
}
