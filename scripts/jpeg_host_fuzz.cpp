// Host memory-safety check of the JPEG parser and entropy decoder (probpose_code_amd/csrc/pp_jpeg_host.h), a stand-alone
// program for a sanitiser build on a CPU machine:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_host_fuzz.cpp -o jpeg_host_fuzz
//   ./jpeg_host_fuzz [--rounds N] [--seed S] file.jpg ...
//
// Every file is probed and decoded as it is (exactly-sized heap buffers, so the sanitiser sees any access past `size`, the
// coefficient capacity or the 3 x 64 table words), then `rounds` times after seeded mutations: single bytes, short runs,
// truncations, and a capacity one short of what the probe asked for. A call may return PP_OK or an error (an error
// carries a reason, a short capacity is never accepted); the sanitisers judge the rest. Exit status 0: every call returned.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../probpose_code_amd/csrc/pp_jpeg_host.h"

static uint64_t g_state = 1;
static uint32_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static long g_ok = 0, g_refused = 0;

// One probe + decode of `size` bytes held in a heap block of exactly that size.
static void run(const std::vector<uint8_t>& bytes, bool short_capacity) {
    uint8_t* data = (uint8_t*)std::malloc(bytes.size() ? bytes.size() : 1);
    if (!bytes.empty()) std::memcpy(data, bytes.data(), bytes.size());
    pp_jpeg_info info;
    const int ps = pp::jpeg::probe(data, bytes.size(), &info);
    if (ps == PP_OK && info.coef_count > 0 && info.coef_count < (1ll << 26)) {
        const long long cap = info.coef_count - (short_capacity ? 1 : 0);
        int16_t* coef = (int16_t*)std::malloc((size_t)(cap > 0 ? cap : 1) * sizeof(int16_t));
        uint16_t* qt = (uint16_t*)std::malloc(3 * 64 * sizeof(uint16_t));
        pp_jpeg_info info2;
        const int st = pp::jpeg::entropy_decode(data, bytes.size(), coef, cap, qt, &info2);
        if (st == PP_OK) {
            ++g_ok;
            if (short_capacity) {
                std::fprintf(stderr, "decode accepted a short coefficient buffer\n");
                std::exit(2);
            }
            long long sum = 0;  // read every value back: uninitialised or out-of-bounds storage would show
            for (long long i = 0; i < info2.coef_count; ++i) sum += coef[i];
            for (int i = 0; i < 64 * info2.ncomp; ++i) sum += qt[i];
            if (sum == 0x7fffffffffffffffll) std::puts("");
        } else {
            ++g_refused;
            if (!pp::jpeg::g_reason[0]) {
                std::fprintf(stderr, "refusal without a reason\n");
                std::exit(2);
            }
        }
        std::free(coef);
        std::free(qt);
    } else {
        ++g_refused;
    }
    std::free(data);
}

int main(int argc, char** argv) {
    int rounds = 300;
    std::vector<const char*> files;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--rounds") && i + 1 < argc) rounds = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) g_state = std::strtoull(argv[++i], nullptr, 10);
        else files.push_back(argv[i]);
    }
    if (files.empty()) {
        std::fprintf(stderr, "usage: %s [--rounds N] [--seed S] file.jpg ...\n", argv[0]);
        return 1;
    }
    for (const char* path : files) {
        FILE* f = std::fopen(path, "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", path);
            return 1;
        }
        std::vector<uint8_t> orig;
        uint8_t buf[4096];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) orig.insert(orig.end(), buf, buf + n);
        std::fclose(f);
        run(orig, false);
        run(orig, true);
        for (size_t cut = 0; cut < orig.size() && cut < 700; ++cut) run(std::vector<uint8_t>(orig.begin(), orig.begin() + cut), false);  // every short prefix
        for (int r = 0; r < rounds; ++r) {
            std::vector<uint8_t> m = orig;
            if (m.empty()) break;
            switch (rnd() % 5) {
                case 0: m[rnd() % m.size()] = (uint8_t)rnd(); break;                    // one byte
                case 1: m[rnd() % m.size()] ^= (uint8_t)(1u << (rnd() % 8)); break;     // one bit
                case 2: {                                                               // a short run
                    size_t at = rnd() % m.size(), len = 1 + rnd() % 8;
                    for (size_t i = at; i < m.size() && i < at + len; ++i) m[i] = (uint8_t)rnd();
                    break;
                }
                case 3: m.resize(rnd() % m.size()); break;                              // truncation
                default: {                                                              // a marker byte dropped in
                    size_t at = rnd() % m.size();
                    m[at] = 0xFF;
                    if (at + 1 < m.size()) m[at + 1] = (uint8_t)(0xC0 + rnd() % 64);
                }
            }
            run(m, false);
        }
    }
    std::printf("jpeg_host_fuzz: %zu files, %ld decodes OK, %ld refused, no fault\n", files.size(), g_ok, g_refused);
    return 0;
}
