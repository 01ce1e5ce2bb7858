// Stand-alone host check of the device Huffman coder (csrc/pp_jpeg_entropy.hip): its phases restated sequentially on the host
// around the coder's own core (csrc/pp_jpeg_entropy_core.h: block addressing and DC predictor, the code walk, the bit packer,
// the scratch layout, the byte order of the packed words - the code the kernels run), compared byte for byte with
// entropy_encode of csrc/pp_jpeg_enc_host.h on seeded coefficient arrays: seven sizes x three samplings x four densities x
// two amplitudes x three special forms (plain; a last Cr block ending in 1023 at zigzag 63; single AC values at zigzag
// 16 / 17 / 33 / 49 / 63 with DC differences of +-2047). What it does not run: the workgroup scans and the grids - those are
// the GPU tests' (tests/test_jpeg_entropy_gpu.py). A program for a sanitiser build on a CPU machine; no GPU is used:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_entropy_host_check.cpp -o jpeg_entropy_host_check
//   ./jpeg_entropy_host_check        ->  "504 cases, 0 failures"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../probpose_code_amd/csrc/pp_jpeg_enc_host.h"
#include "../probpose_code_amd/csrc/pp_jpeg_entropy_core.h"

using namespace pp;

static int run_case(int W, int H, int sub, double density, int amp, unsigned seed, int special) {
    pp_jpeg_info info;
    if (jpeg::encode_plan(W, H, sub, &info) != PP_OK) return 1;
    std::mt19937 rng(seed);
    std::vector<int16_t> coef((size_t)info.coef_count, 0);
    std::uniform_real_distribution<double> u(0, 1);
    for (auto& c : coef)
        if (u(rng) < density) c = (int16_t)((int)(rng() % (2 * amp + 1)) - amp);
    // keep DC diffs legal: limit DC to +-1000
    for (size_t b = 0; b < coef.size() / 64; ++b) coef[b * 64] = (int16_t)((int)(rng() % 2001) - 1000);
    if (special == 1) coef[coef.size() - 1] = 1023;  // the last Cr block ends with 1023 at zigzag 63
    if (special == 2) {  // one AC value per block at zigzag 16, 17, 33, 49 or 63; DC values 1023 / -1024 alternate
        static const int at[5] = {16, 17, 33, 49, 63};
        for (size_t b = 0; b < coef.size() / 64; ++b) {
            std::memset(&coef[b * 64], 0, 128);
            coef[b * 64 + jpeg::kNatural[at[b % 5]]] = (b & 1) ? -1023 : 1023;
            coef[b * 64] = (b & 1) ? 1023 : -1024;
        }
    }
    uint16_t qt[192];
    jpeg::quality_tables(75, qt);
    std::vector<uint8_t> file((size_t)jpeg::encoded_bound(&info));
    size_t fsz = 0, hsz = 0;
    int st = jpeg::entropy_encode(coef.data(), qt, &info, 0, file.data(), file.size(), &fsz);
    if (st != PP_OK) { std::printf("host refused: %s\n", jpeg::g_reason); return 1; }
    std::vector<uint8_t> hdr(1024);
    if (jpeg::write_headers(qt, &info, 0, hdr.data(), hdr.size(), &hsz) != PP_OK) return 1;
    if (std::memcmp(hdr.data(), file.data(), hsz) != 0) { std::printf("header mismatch\n"); return 1; }

    static const EntTables T = ent_tables();
    pp_jpeg_ent_desc d{};
    d.coef = coef.data();
    d.hs = info.hs; d.vs = info.vs; d.mcus_x = info.mcus_x; d.mcus_y = info.mcus_y;
    uint8_t dummy; pp_jpeg_ent_result res;
    d.scratch = &dummy; d.out = &dummy; d.result = &res;
    const long long nblk = ent_blocks(d);
    if (nblk != info.coef_count / 64) { std::printf("nblk mismatch\n"); return 1; }
    const EntLayout L = ent_layout(nblk);
    std::vector<uint32_t> len(nblk);
    bool bad = false;
    for (long long s = 0; s < nblk; ++s) {
        uint32_t w[32]; int pred, chroma;
        load_block(d, s, w, pred, chroma);
        BitCounter c;
        bad |= code_block(w, pred, T.dc[chroma], T.ac[chroma], c);
        len[s] = c.bits;
        if (c.bits > (uint32_t)ENT_BLOCK_BITS) { std::printf("len over bound\n"); return 1; }
    }
    std::vector<unsigned long long> coff(L.nchunks);
    unsigned long long tot = 0;
    for (long long c = 0; c < L.nchunks; ++c) {
        coff[c] = tot;
        for (long long s = c * ENT_CHUNK; s < nblk && s < (c + 1) * ENT_CHUNK; ++s) tot += len[s];
    }
    const unsigned long long nbytes = (tot + 7) >> 3;
    std::vector<uint32_t> words(L.nwords, 0xDEADBEEF);
    long long quads = (long long)((nbytes + 15) >> 4);
    if (quads > L.nwords / 4) { std::printf("quads over\n"); return 1; }
    for (long long i = 0; i < quads * 4; ++i) words[i] = 0;
    for (long long c = 0; c < L.nchunks; ++c) {
        unsigned long long before = 0;
        for (long long s = c * ENT_CHUNK; s < nblk && s < (c + 1) * ENT_CHUNK; ++s) {
            uint32_t w[32]; int pred, chroma;
            load_block(d, s, w, pred, chroma);
            BitPacker p(words.data(), coff[c] + before, L.nwords);
            code_block(w, pred, T.dc[chroma], T.ac[chroma], p);
            if (s == nblk - 1 && p.phase()) p.put(0x7Fu, 8 - p.phase());
            p.finish();
            if (p.widx >= quads * 4 && p.n > 0) { std::printf("pack beyond zeroed\n"); return 1; }
            before += len[s];
        }
    }
    std::vector<uint8_t> out;
    for (unsigned long long k = 0; k < nbytes; ++k) {
        const uint32_t b = stream_byte(words[k >> 2], (int)(k & 3));
        out.push_back((uint8_t)b);
        if (b == 255) out.push_back(0);
    }
    const size_t want = fsz - hsz - 2;
    if (bad || out.size() != want || std::memcmp(out.data(), file.data() + hsz, want) != 0) {
        std::printf("MISMATCH %dx%d sub %d dens %g: got %zu want %zu bad %d\n", W, H, sub, density, out.size(), want, (int)bad);
        return 1;
    }
    return 0;
}

int main() {
    int fails = 0, n = 0;
    const int sizes[][2] = {{1, 1}, {8, 8}, {9, 17}, {16, 16}, {17, 33}, {250, 130}, {641, 479}};
    unsigned seed = 1;
    for (auto& sz : sizes)
        for (int sub = 0; sub < 3; ++sub)
            for (double dens : {0.0, 0.01, 0.1, 1.0})
                for (int amp : {3, 1023})
                    for (int special = 0; special < 3; ++special) { fails += run_case(sz[0], sz[1], sub, dens, amp, seed++, special); ++n; }
    std::printf("%d cases, %d failures\n", n, fails);
    return fails != 0;
}
