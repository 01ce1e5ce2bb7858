// Host memory-safety and round-trip check of the JPEG entropy coder (probpose_code_amd/csrc/pp_jpeg_enc_host.h) against the
// entropy decoder (pp_jpeg_host.h), a stand-alone program for a sanitiser build on a CPU machine:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_enc_host_fuzz.cpp -o jpeg_enc_host_fuzz
//   ./jpeg_enc_host_fuzz [--rounds N] [--seed S]
//
// Every round draws a geometry (sides 1..70, the three samplings), a quality, a restart interval and a coefficient array of
// one of several kinds - sparse, dense, all +-1023 AC with DC steps of +-2047, long zero runs, all zero - codes it into an
// exactly-sized heap buffer (the size the first pass reported, so the sanitiser sees any write past it), decodes the file
// with the host decoder and compares coefficients, tables and geometry. It also codes into a buffer one byte short
// (PP_ERR_WORKSPACE expected), checks the file against pp_jpeg_encoded_bound, and feeds values no baseline code expresses
// (PP_ERR_INVALID_ARG expected). Exit status 0: every round agreed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../probpose_code_amd/csrc/pp_jpeg_enc_host.h"

static uint64_t g_state = 1;
static uint32_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}
static int rnd_range(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static void die(const char* what, int round) {
    std::fprintf(stderr, "round %d: %s (%s)\n", round, what, pp::jpeg::g_reason);
    std::exit(2);
}

int main(int argc, char** argv) {
    int rounds = 2000;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--rounds") && i + 1 < argc) rounds = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) g_state = std::strtoull(argv[++i], nullptr, 10);
        else {
            std::fprintf(stderr, "usage: %s [--rounds N] [--seed S]\n", argv[0]);
            return 1;
        }
    }
    long files = 0, bytes = 0, refused = 0;
    for (int r = 0; r < rounds; ++r) {
        pp_jpeg_info info;
        const int W = rnd_range(1, 70), H = rnd_range(1, 70), sub = rnd_range(0, 2);
        if (pp::jpeg::encode_plan(W, H, sub, &info) != PP_OK) die("encode_plan refused a valid geometry", r);
        const long long n = info.coef_count, blocks = n / 64;
        int16_t* coef = (int16_t*)std::malloc((size_t)n * sizeof(int16_t));
        uint16_t* qt = (uint16_t*)std::malloc(192 * sizeof(uint16_t));
        if (pp::jpeg::quality_tables(rnd_range(1, 100), qt) != PP_OK) die("quality_tables refused a valid quality", r);
        if (rnd() % 4 == 0)
            for (int i = 128; i < 192; ++i) qt[i] = (uint16_t)rnd_range(1, 255);  // a third table of its own
        const int kind = r % 6;
        for (long long b = 0; b < blocks; ++b) {
            int16_t* blk = coef + b * 64;
            for (int k = 0; k < 64; ++k) {
                int v = 0;
                switch (kind) {
                    case 0: v = rnd() % 8 == 0 ? rnd_range(-1023, 1023) : 0; break;            // sparse
                    case 1: v = rnd_range(-1023, 1023); break;                                  // dense
                    case 2: v = (rnd() & 1) ? 1023 : -1023; break;                              // extreme AC
                    case 3: v = (k == 63 || k == 17) ? rnd_range(-3, 3) : 0; break;             // long zero runs (ZRL)
                    case 4: v = 0; break;                                                       // EOB only
                    default: v = rnd() % 3 == 0 ? ((rnd() & 1) ? 1 : -1) * (1 << (rnd() % 10)) : 0;   // every magnitude category
                }
                blk[k] = (int16_t)v;
            }
            // DC: within +-1023 so that any two differ by at most 2046; kind 2 alternates the extremes (-1024, 1023: 2047)
            blk[0] = (int16_t)(kind == 2 ? ((b & 1) ? 1023 : -1024) : (kind == 4 ? 0 : rnd_range(-1023, 1023)));
        }
        const int n_mcus = info.mcus_x * info.mcus_y;
        const int ri_pick[5] = {0, 1, 3, n_mcus, n_mcus + 7};
        const int ri = ri_pick[rnd() % 5];
        const long long bound = pp::jpeg::encoded_bound(&info);
        if (bound <= 0) die("no bound", r);
        uint8_t* big = (uint8_t*)std::malloc((size_t)bound);
        size_t size = 0;
        if (pp::jpeg::entropy_encode(coef, qt, &info, ri, big, (size_t)bound, &size) != PP_OK) die("encode failed inside the bound", r);
        if (size == 0 || (long long)size > bound) die("size outside the bound", r);
        // exactly sized, and one byte short
        uint8_t* exact = (uint8_t*)std::malloc(size);
        size_t size2 = 0;
        if (pp::jpeg::entropy_encode(coef, qt, &info, ri, exact, size, &size2) != PP_OK || size2 != size || std::memcmp(exact, big, size))
            die("exactly-sized buffer: another result", r);
        uint8_t* tight = (uint8_t*)std::malloc(size - 1);
        if (pp::jpeg::entropy_encode(coef, qt, &info, ri, tight, size - 1, &size2) != PP_ERR_WORKSPACE || size2 != 0) die("short buffer accepted", r);
        const size_t cut = rnd() % size;
        uint8_t* shorter = (uint8_t*)std::malloc(cut ? cut : 1);
        if (pp::jpeg::entropy_encode(coef, qt, &info, ri, shorter, cut, &size2) != PP_ERR_WORKSPACE) die("short buffer accepted", r);
        // decode and compare
        pp_jpeg_info back;
        int16_t* coef2 = (int16_t*)std::malloc((size_t)n * sizeof(int16_t));
        uint16_t qt2[192];
        if (pp::jpeg::entropy_decode(exact, size, coef2, n, qt2, &back) != PP_OK) die("the decoder refused the file", r);
        if (back.width != W || back.height != H || back.hs != info.hs || back.vs != info.vs || back.coef_count != n || back.restart_interval != ri)
            die("geometry differs", r);
        if (std::memcmp(coef, coef2, (size_t)n * sizeof(int16_t))) die("coefficients differ", r);
        if (std::memcmp(qt, qt2, sizeof(qt2))) die("tables differ", r);
        // values outside the baseline codes
        if (r % 16 == 0) {
            const long long at = (long long)(rnd() % (uint32_t)blocks) * 64;
            const int16_t keep0 = coef[at], keep5 = coef[at + 5];
            coef[at + 5] = (rnd() & 1) ? 1024 : -32768;
            if (pp::jpeg::entropy_encode(coef, qt, &info, ri, big, (size_t)bound, &size2) != PP_ERR_INVALID_ARG) die("AC 1024 accepted", r);
            coef[at + 5] = keep5;
            coef[at] = (rnd() & 1) ? 32767 : -32768;
            const int st = pp::jpeg::entropy_encode(coef, qt, &info, ri, big, (size_t)bound, &size2);
            if (st != PP_ERR_INVALID_ARG) die("a DC difference above 2047 accepted", r);
            coef[at] = keep0;
            ++refused;
        }
        ++files;
        bytes += (long)size;
        std::free(coef);
        std::free(coef2);
        std::free(qt);
        std::free(big);
        std::free(exact);
        std::free(tight);
        std::free(shorter);
    }
    std::printf("jpeg_enc_host_fuzz: %ld files (%ld bytes) coded, decoded and equal; %ld out-of-range arrays refused; no fault\n", files, bytes, refused);
    return 0;
}
