// Stand-alone host check of the PNG writer's device code build (png_code / png_code_lz of csrc/pp_png.hip): the steps of
// csrc/pp_png_code_core.h - the text the kernel runs - one after another on the host (build_code_steps,
// build_code_steps_lz), against the host builders build_code / build_code_lz of csrc/pp_png_core.h. Every byte of the
// pp_deflate_code / pp_deflate_code_lz must be equal:
//   - named histograms: a code-length tree deeper than 7 (lengths 4 .. 15 by counts of 2^(15 - l): the limit-7 repair loop
//     runs), Fibonacci counts on 40 symbols (39 deep), nothing used, the end of block and one other, all 286 equal, all
//     286 at 2^32 - 1 (64-bit weights), 257 used symbols; in lz mode these with distance counts all zero, only symbol 29,
//     Fibonacci over all 30, two equal, random;
//   - 200 000 seeded random histograms per mode, of mixed sparsity and magnitude, geometric ones and ones with many equal
//     counts among them.
// What it does not run: the kernel's executor (the striding over threads, the barriers, the workgroup scan, LDS atomics) -
// those are the GPU tests' (tests/test_png_code_gpu.py). A program for a sanitiser build on a CPU machine; no GPU is used:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/png_code_host_check.cpp -o png_code_host_check
//   ./png_code_host_check        ->  "400042 cases, 0 failures"
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../probpose_code_amd/csrc/pp_png_code_core.h"

using namespace pp::png;

static int g_cases = 0, g_fails = 0;

static void check(const char* name, const std::vector<uint32_t>& hist) {
    ++g_cases;
    pp_deflate_code want, got;
    std::memset(&got, 0xA5, sizeof(got));
    build_code(hist.data(), &want);
    build_code_steps(hist.data(), &got);
    if (std::memcmp(&want, &got, sizeof(want)) != 0) {
        std::printf("FAIL %s: the steps give another code\n", name);
        ++g_fails;
    }
}

static void check_lz(const char* name, const std::vector<uint32_t>& hist) {
    ++g_cases;
    pp_deflate_code_lz want, got;
    std::memset(&got, 0xA5, sizeof(got));
    build_code_lz(hist.data(), &want);
    build_code_steps_lz(hist.data(), &got);
    if (std::memcmp(&want, &got, sizeof(want)) != 0) {
        std::printf("FAIL lz %s: the steps give another code\n", name);
        ++g_fails;
    }
}

// Counts that make build_lengths return the lengths 4 .. 15 below without a repair; their code-length tree is 10 deep.
static std::vector<uint32_t> deep_code_length_tree() {
    static const int per[16] = {0, 0, 0, 0, 1, 13, 24, 3, 23, 9, 15, 12, 5, 1, 0, 116};
    std::vector<uint32_t> h(288, 0);
    int s = 0;
    for (int l = 4; l <= 15; ++l)
        for (int k = 0; k < per[l]; ++k) h[s++] = 1u << (15 - l);  // s ends at 222
    std::swap(h[256], h[221]);  // symbol 256 among the used ones, for one of the l15 symbols
    return h;
}

static std::vector<uint32_t> random_hist(std::mt19937& rng, int n) {
    std::vector<uint32_t> h((size_t)n, 0);
    const int kind = (int)(rng() % 6);
    const uint32_t keep = 1 + rng() % 16;  // one symbol in `keep` is used
    const int shift = (int)(rng() % 32);
    for (int s = 0; s < n; ++s) {
        if (rng() % keep) continue;
        if (kind == 0) h[s] = (uint32_t)rng() >> shift;
        else if (kind == 1) h[s] = 1 + rng() % 4;  // many equal counts
        else if (kind == 2) h[s] = 1u << (rng() % 32);  // geometric
        else if (kind == 3) h[s] = (uint32_t)(1.0 + 1e9 / (1.0 + (double)(rng() % 100000)));
        else if (kind == 4) h[s] = (rng() % 3) ? 7u : (uint32_t)rng();
        else h[s] = 0xFFFFFFFFu - rng() % 3;
    }
    return h;
}

int main() {
    std::mt19937 rng(11);
    std::vector<std::vector<uint32_t>> named;
    named.push_back(deep_code_length_tree());
    {
        std::vector<uint32_t> h(288, 0);
        uint32_t a = 1, b = 1;
        for (int s = 0; s < 40; ++s) {
            h[s] = a;
            const uint32_t c = a + b;
            a = b, b = c;
        }
        named.push_back(h);
        h.assign(288, 0);
        named.push_back(h);  // only 256 is used, symbol 0 is added
        h[256] = 3, h[65] = 9;
        named.push_back(h);
        h.assign(288, 0);
        for (int s = 0; s < DEFLATE_SYMS; ++s) h[s] = 77;
        named.push_back(h);
        for (int s = 0; s < DEFLATE_SYMS; ++s) h[s] = 0xFFFFFFFFu;
        named.push_back(h);
        h.assign(288, 0);
        for (int s = 0; s < 257; ++s) h[s] = 1 + rng() % 100000;
        named.push_back(h);
    }
    for (auto& h : named) check("named", h);
    for (auto& lit : named) {
        for (int kind = 0; kind < 5; ++kind) {
            std::vector<uint32_t> h(LZ_HIST_WORDS, 0);
            std::copy(lit.begin(), lit.end(), h.begin());
            uint32_t a = 1, b = 1;
            for (int s = 0; s < LZ_DIST_SYMS; ++s) {
                uint32_t v = 0;
                if (kind == 1) v = s == 29 ? 5 : 0;
                else if (kind == 2) v = a;
                else if (kind == 3) v = (s == 4 || s == 17) ? 6 : 0;
                else if (kind == 4) v = rng() % 1000;
                h[LZ_DIST_AT + s] = v;
                const uint32_t c = a + b;
                a = b, b = c;
            }
            check_lz("named", h);
        }
    }
    for (int i = 0; i < 200000; ++i) {
        std::vector<uint32_t> h = random_hist(rng, 288);
        h[286] = h[287] = 0;
        check("random", h);
        std::vector<uint32_t> d = random_hist(rng, 32);
        h.resize(LZ_HIST_WORDS, 0);
        for (int s = 0; s < LZ_DIST_SYMS; ++s) h[LZ_DIST_AT + s] = d[s];
        check_lz("random", h);
    }
    std::printf("%d cases, %d failures\n", g_cases, g_fails);
    return g_fails != 0;
}
