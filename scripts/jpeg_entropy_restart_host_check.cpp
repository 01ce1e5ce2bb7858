// Stand-alone host check of the device Huffman coder with restart intervals (pp_jpeg_entropy_encode_restart_batch,
// csrc/pp_jpeg_entropy.hip): the phases with RST restated sequentially on the host around the coder's own core
// (csrc/pp_jpeg_entropy_core.h: load_block with the interval, ent_intervals, ent_rst_layout, ent_interval_bytes,
// ent_pack_start, ent_pads, ent_interval_at, ent_stuff_restart - the code the kernels run), compared byte for byte with
// entropy_encode of csrc/pp_jpeg_enc_host.h at the same interval. Seeded coefficients: four sizes x three samplings x three
// densities x three special forms (plain; every Cr block ending in 1023 at zigzag 63, so that intervals end in FF bytes, padded
// and whole; single AC values with DC values of 1023 / -1024) x the intervals 1, 2, 3, 7, 8, 9, one MCU row, mcus - 1, mcus,
// mcus + 1 and 65535. Over the run it also counts the forms the streams must show - an interval end at each bit phase, FF 00
// FF Dn from a padded byte and from a whole data byte, marker numbers that wrap, an interval count that does not divide the
// MCU count, an interval of at least the MCU count (the bytes of interval 0), eight bytes holding several markers, a scan
// that differs from interval 0's in the first block of an interval - and fails when one is missing. What it does not run:
// the workgroup scans and the grids - those are the GPU tests' (tests/test_jpeg_entropy_restart_gpu.py). A program for a
// sanitiser build on a CPU machine; no GPU is used:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_entropy_restart_host_check.cpp -o jpeg_entropy_restart_host_check
//   ./jpeg_entropy_restart_host_check        ->  "1188 cases, 0 failures; forms: ... all seen"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../probpose_code_amd/csrc/pp_jpeg_enc_host.h"
#include "../probpose_code_amd/csrc/pp_jpeg_entropy_core.h"

using namespace pp;

struct Forms {
    int phase[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int padded_ff = 0, whole_ff = 0, wrap = 0, ragged = 0, single = 0, crowded = 0, reset_visible = 0;
};
static Forms g_forms;

static int run_case(int W, int H, int sub, double density, unsigned seed, int special, int R) {
    pp_jpeg_info info;
    if (jpeg::encode_plan(W, H, sub, &info) != PP_OK) return 1;
    std::mt19937 rng(seed);
    std::vector<int16_t> coef((size_t)info.coef_count, 0);
    std::uniform_real_distribution<double> u(0, 1);
    for (auto& c : coef)
        if (u(rng) < density) c = (int16_t)((int)(rng() % 2047) - 1023);
    for (size_t b = 0; b < coef.size() / 64; ++b) coef[b * 64] = (int16_t)((int)(rng() % 2001) - 1000);  // (legal DC differences, reset or not)
    const long long mcus = (long long)info.mcus_x * info.mcus_y;
    if (special == 1)  // every Cr block ends with 1023 at zigzag 63: the last bits of every MCU are ten ones
        for (long long m = 0; m < mcus; ++m) coef[coef.size() - 64 * (size_t)(mcus - m) + 63] = 1023;
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
    std::vector<uint8_t> file((size_t)jpeg::encoded_bound(&info)), plain(file.size());
    size_t fsz = 0, hsz = 0, psz = 0, phsz = 0;
    if (jpeg::entropy_encode(coef.data(), qt, &info, R, file.data(), file.size(), &fsz) != PP_OK) { std::printf("host refused: %s\n", jpeg::g_reason); return 1; }
    std::vector<uint8_t> hdr(1024);
    if (jpeg::write_headers(qt, &info, R, hdr.data(), hdr.size(), &hsz) != PP_OK) return 1;
    if (std::memcmp(hdr.data(), file.data(), hsz) != 0) { std::printf("header mismatch\n"); return 1; }
    const bool plain_ok = jpeg::entropy_encode(coef.data(), qt, &info, 0, plain.data(), plain.size(), &psz) == PP_OK;  // (special 2 needs the resets)
    if (jpeg::write_headers(qt, &info, 0, hdr.data(), hdr.size(), &phsz) != PP_OK) return 1;

    static const EntTables T = ent_tables();
    pp_jpeg_ent_desc d{};
    d.coef = coef.data();
    d.hs = info.hs; d.vs = info.vs; d.mcus_x = info.mcus_x; d.mcus_y = info.mcus_y;
    d.restart_interval = R;
    uint8_t dummy; pp_jpeg_ent_result res;
    d.scratch = &dummy; d.out = &dummy; d.result = &res;
    if (!ent_interval_ok(d)) { std::printf("interval refused\n"); return 1; }
    const long long nblk = ent_blocks(d);
    if (nblk != info.coef_count / 64) { std::printf("nblk mismatch\n"); return 1; }
    const EntRstLayout L = ent_rst_layout(nblk, mcus);
    const EntLayout L0 = ent_layout(nblk);
    if (L.total < L0.total || L.nwords < L0.nwords || L.nint != mcus) { std::printf("layout\n"); return 1; }
    const EntIntervals iv = ent_intervals(d);
    if (iv.count < 1 || iv.count > L.nint) { std::printf("interval count\n"); return 1; }
    // ---- jpeg_ent_bits: lengths, chunk sums, an interval's first block leaves its offset inside the chunk
    std::vector<uint32_t> len(nblk), irel(L.nint, 0xDEADBEEF), ilen(L.nint, 0xDEADBEEF);
    std::vector<unsigned long long> coff(L.nchunks), ioff(L.nint + 1, ~0ull);
    bool bad = false;
    unsigned long long tot = 0;
    for (long long c = 0; c < L.nchunks; ++c) {
        coff[c] = tot;
        uint32_t before = 0;
        for (long long s = c * ENT_CHUNK; s < nblk && s < (c + 1) * ENT_CHUNK; ++s) {
            uint32_t w[32]; int pred, chroma;
            load_block<true>(d, s, w, pred, chroma, d.restart_interval);
            BitCounter bc;
            bad |= code_block(w, pred, T.dc[chroma], T.ac[chroma], bc);
            len[s] = bc.bits;
            const long long j = s / iv.bpi;
            if (s == j * iv.bpi && j < L.nint) irel[j] = before;
            before += bc.bits;
        }
        tot += before;
    }
    // ---- jpeg_ent_scan: the intervals
    unsigned long long nbytes = (tot + 7) >> 3;
    if (iv.count > 1) {
        unsigned long long at = 0;
        for (long long j = 0; j < iv.count; ++j) ilen[j] = ent_interval_bytes(iv, j, coff.data(), irel.data(), tot);
        for (long long j = 0; j < iv.count; ++j) {
            if (ilen[j] == 0) { std::printf("empty interval\n"); return 1; }
            ioff[j] = at;
            at += ilen[j];
            const unsigned long long bits = ent_interval_bits_before(iv, j + 1, coff.data(), irel.data(), tot) - ent_interval_bits_before(iv, j, coff.data(), irel.data(), tot);
            ++g_forms.phase[bits & 7];
        }
        nbytes = at;
    } else {
        ioff[0] = 0;
    }
    ioff[iv.count] = nbytes;
    if (nbytes > (unsigned long long)L.max_bytes) { std::printf("bytes over the bound\n"); return 1; }
    // ---- jpeg_ent_zero, jpeg_ent_pack
    std::vector<uint32_t> words(L.nwords, 0xDEADBEEF);
    const long long quads = (long long)((nbytes + 15) >> 4);
    if (quads > L.nwords / 4) { std::printf("quads over\n"); return 1; }
    for (long long i = 0; i < quads * 4; ++i) words[i] = 0;
    for (long long c = 0; c < L.nchunks; ++c) {
        unsigned long long before = 0;
        for (long long s = c * ENT_CHUNK; s < nblk && s < (c + 1) * ENT_CHUNK; ++s) {
            unsigned long long start = coff[c] + before;
            bool pads = s == nblk - 1;
            if (iv.count > 1) {
                start = ent_pack_start(iv, s, start, coff.data(), irel.data(), ioff.data());
                pads = ent_pads(iv, s, nblk);
            }
            uint32_t w[32]; int pred, chroma;
            load_block<true>(d, s, w, pred, chroma, d.restart_interval);
            BitPacker p(words.data(), start, L.nwords);
            code_block(w, pred, T.dc[chroma], T.ac[chroma], p);
            if (pads && p.phase()) p.put(0x7Fu, 8 - p.phase());
            p.finish();
            if (p.widx >= quads * 4 && p.n > 0) { std::printf("pack beyond zeroed\n"); return 1; }
            before += len[s];
        }
    }
    // ---- jpeg_ent_ffcount, jpeg_ent_ffscan, jpeg_ent_stuff: a "thread" is eight bytes
    unsigned long long ff = 0;
    for (unsigned long long k = 0; k < nbytes; ++k) ff += stream_byte(words[k >> 2], (int)(k & 3)) == 255u;
    const long long need = (long long)(nbytes + ff) + 2 * (iv.count - 1);
    std::vector<uint8_t> out((size_t)need, 0xA5);
    long long pos = 0;  // with the FF bytes in front counted, the markers not
    for (long long byte0 = 0; byte0 < (long long)nbytes; byte0 += 8) {
        const long long left = (long long)nbytes - byte0;
        const int valid = left >= 8 ? 8 : (int)left;
        uint32_t v[2] = {words[byte0 >> 2], valid > 4 ? words[(byte0 >> 2) + 1] : 0u};
        if (iv.count > 1) {
            ent_stuff_restart(v, valid, byte0, pos, ioff.data(), iv.count, out.data(), need);
            const long long j0 = ent_interval_at(ioff.data(), iv.count, (unsigned long long)byte0);
            const long long j1 = ent_interval_at(ioff.data(), iv.count, (unsigned long long)(byte0 + valid - 1));
            if (j1 - j0 + ((long long)ioff[j1 + 1] == byte0 + valid && j1 + 1 < iv.count) >= 2) ++g_forms.crowded;
        } else {
            long long q = pos;
            for (int k = 0; k < valid; ++k) {
                const uint32_t b = stream_byte(v[k >> 2], k & 3);
                if (q < need) out[q] = (uint8_t)b;
                ++q;
                if (b == 255u) { if (q < need) out[q] = 0; ++q; }
            }
        }
        for (int k = 0; k < valid; ++k) pos += 1 + (stream_byte(v[k >> 2], k & 3) == 255u);
    }
    const size_t want = fsz - hsz - 2;
    if (bad || (size_t)need != want || std::memcmp(out.data(), file.data() + hsz, want) != 0) {
        size_t first = 0;
        while (first < want && first < (size_t)need && out[first] == file[hsz + first]) ++first;
        std::printf("MISMATCH %dx%d sub %d dens %g special %d R %d: got %lld want %zu bad %d first difference at %zu\n", W, H, sub, density, special, R,
                    need, want, (int)bad, first);
        return 1;
    }
    // ---- the forms, read from the host coder's stream
    const uint8_t* scan = file.data() + hsz;
    long long markers = 0;
    for (size_t i = 0; i + 1 < want; ++i)
        if (scan[i] == 0xFF && scan[i + 1] >= 0xD0 && scan[i + 1] <= 0xD7) {
            if ((int)(scan[i + 1] - 0xD0) != (int)(markers & 7)) { std::printf("marker order\n"); return 1; }
            if (i >= 2 && scan[i - 2] == 0xFF && scan[i - 1] == 0x00) {
                const unsigned long long bits = ent_interval_bits_before(iv, markers + 1, coff.data(), irel.data(), tot) - ent_interval_bits_before(iv, markers, coff.data(), irel.data(), tot);
                ++((bits & 7) ? g_forms.padded_ff : g_forms.whole_ff);
            }
            ++markers;
        }
    if (markers != iv.count - 1) { std::printf("marker count %lld, intervals %lld\n", markers, iv.count); return 1; }
    if (markers > 8) ++g_forms.wrap;
    if (iv.count > 1 && mcus % iv.per != 0) ++g_forms.ragged;
    if (R >= mcus) {
        if (!plain_ok || want != psz - phsz - 2 || std::memcmp(scan, plain.data() + phsz, want) != 0) { std::printf("R >= mcus differs from R = 0\n"); return 1; }
        if (hsz != phsz + 6) { std::printf("no DRI segment\n"); return 1; }
        ++g_forms.single;
    } else if (plain_ok && iv.count > 1 && ilen[0] + 2 < want) {  // the first interval is coded alike; behind the first marker the reset shows
        const uint8_t* a = scan + ilen[0];
        while (a < scan + want && !(a[0] == 0xFF && a[1] == 0xD0)) ++a;
        const uint8_t* b = plain.data() + phsz + (a - scan);
        if ((size_t)(a - scan) + 4 <= want && (size_t)(a - scan) + 2 <= psz - phsz - 2 && std::memcmp(a + 2, b, 2) != 0) ++g_forms.reset_visible;
    }
    return 0;
}

int main() {
    int fails = 0, n = 0;
    const int sizes[][2] = {{8, 8}, {17, 33}, {40, 24}, {250, 130}};
    unsigned seed = 1;
    for (auto& sz : sizes)
        for (int sub = 0; sub < 3; ++sub) {
            pp_jpeg_info info;
            if (jpeg::encode_plan(sz[0], sz[1], sub, &info) != PP_OK) return 2;
            const int mcus = info.mcus_x * info.mcus_y;
            const int intervals[] = {1, 2, 3, 7, 8, 9, info.mcus_x, mcus - 1, mcus, mcus + 1, 65535};
            for (double dens : {0.0, 0.05, 1.0})
                for (int special = 0; special < 3; ++special)
                    for (int R : intervals) { fails += run_case(sz[0], sz[1], sub, dens, seed++, special, R); ++n; }
        }
    const Forms& f = g_forms;
    bool all = f.padded_ff && f.whole_ff && f.wrap && f.ragged && f.single && f.crowded && f.reset_visible;
    for (int p = 0; p < 8; ++p) all = all && f.phase[p];
    std::printf("%d cases, %d failures; forms: end phases %d %d %d %d %d %d %d %d, padded FF %d, whole FF %d, wrap %d, ragged %d, single %d, crowded %d, "
                "reset visible %d: %s\n", n, fails, f.phase[0], f.phase[1], f.phase[2], f.phase[3], f.phase[4], f.phase[5], f.phase[6], f.phase[7], f.padded_ff,
                f.whole_ff, f.wrap, f.ragged, f.single, f.crowded, f.reset_visible, all ? "all seen" : "A FORM IS MISSING");
    return (fails != 0 || !all) ? 1 : 0;
}
