// Stand-alone host check of the device Huffman decoder (csrc/pp_jpeg_huffdec.hip): its phases restated sequentially on the
// host around the decoder's own core (csrc/pp_jpeg_huffdec_core.h: bit reader, state, one subsequence's decode, block
// addressing, scratch layout - the code the kernels run), compared with entropy_decode of csrc/pp_jpeg_host.h. A program
// for a sanitiser build on a CPU machine; no GPU is used:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_huffdec_host_check.cpp -o jpeg_huffdec_host_check
//   ./jpeg_huffdec_host_check [--rounds N] [--seed S] file.jpg ...
//
// Every file runs as it is, after the three truncations of tests/golden/make_golden_jpeg.py (half, the last bytes gone with
// and without EOI), with its entropy-coded segment cut at every one of its last 40 lengths (EOI put back), after each of 32
// single bit flips at fixed places of the segment (the damaged streams the GPU tests run), and `rounds` times after a
// seeded single bit flip or byte deletion inside the segment; a file with a restart interval (taken through
// scan_prepare's restart form) also with a marker deleted, two markers' numbers swapped, a marker doubled (an empty
// interval) and D7 changed to D0, and for every subsequence that holds a marker run() from five entry states must return
// one exit state. Stream, tables, coefficients and scratch live
// in heap blocks of exactly their size, so the sanitiser sees any access outside them. Demanded of every input the
// preparation accepts: the restated device decoder and the host decoder agree on acceptance - except that the device may
// say "not synchronised" - and where the device says PP_OK its coefficients are the host's, byte for byte; at sync_passes
// = 64 every accepted corpus file must synchronise. What it does not run: the workgroup scans and the grids - those are
// the GPU tests' (tests/test_jpeg_huffdec_gpu.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../probpose_code_amd/csrc/pp_jpeg_host.h"
#include "../probpose_code_amd/csrc/pp_jpeg_huffdec_core.h"

using namespace pp;
using namespace pp::hd;

static uint64_t g_state = 1;
static uint32_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static long long end_of(long long i, long long len) { return (i + 1) * HD_S < len ? (i + 1) * HD_S : len; }

// The launches of pp_jpeg_huffman_decode_batch for one image, thread by thread.
static pp_jpeg_hd_result emulate(const pp_jpeg_hd_desc& d, int sync_passes) {
    const Geometry G = geometry(d);
    if (!G.valid) return pp_jpeg_hd_result{PP_ERR_INVALID_ARG, 0, 0, HD_BAD_DESC};
    const Layout L = layout(d.stream_bytes, G.restart != 0);
    const Stream st{d.stream, d.stream_bytes};
    State* entry_g = reinterpret_cast<State*>(d.scratch + L.o_entry);
    State* exit_g = reinterpret_cast<State*>(d.scratch + L.o_exit);
    uint32_t* cnt_g = reinterpret_cast<uint32_t*>(d.scratch + L.o_cnt);
    uint32_t* first_g = reinterpret_cast<uint32_t*>(d.scratch + L.o_first);
    uint32_t* mfirst_g = reinterpret_cast<uint32_t*>(d.scratch + L.o_mfirst);  // (restart files only)
    State* bexit = reinterpret_cast<State*>(d.scratch + L.o_bexit);
    uint32_t* open_g = reinterpret_cast<uint32_t*>(d.scratch + L.o_open);
    Header* hdr = reinterpret_cast<Header*>(d.scratch);
    uint32_t unused = 0;
    // jpeg_hd_sync
    for (int pass = 0; pass < sync_passes; ++pass) {
        for (long long wg = 0; wg < L.nwg; ++wg) {
            if (pass > 0) {  // a workgroup at rest only hands its last exit on
                const long long i0 = wg * HD_WG, i1 = i0 + HD_WG < L.nsub ? i0 + HD_WG : L.nsub;
                const State left0 = wg == 0 ? State{0u, 0u} : bexit[(long long)((pass - 1) & 1) * L.nwg + wg - 1];
                if (!open_g[wg] && same(left0, entry_g[i0])) {
                    bexit[(long long)(pass & 1) * L.nwg + wg] = exit_g[i1 - 1];
                    continue;
                }
            }
            State entry[HD_WG], exit[HD_WG], ex[2][HD_WG], left{0u, 0u};
            uint32_t cnt[HD_WG];
            bool live[HD_WG], dirty[HD_WG];
            for (int t = 0; t < HD_WG; ++t) {
                const long long i = wg * HD_WG + t;
                live[t] = i < L.nsub;
                dirty[t] = false;
                entry[t] = exit[t] = State{0u, 0u};
                cnt[t] = 0;
                if (!live[t]) continue;
                if (pass == 0) {
                    entry[t] = State{canonical(st, (uint32_t)(i * HD_S * 8)), 0u};
                    CountSink c;
                    exit[t] = run(st, d.tables, entry[t], end_of(i, st.len), G, c, unused);
                    cnt[t] = c.blocks | (c.markers << 16);
                } else {
                    entry[t] = entry_g[i];
                    exit[t] = exit_g[i];
                    cnt[t] = cnt_g[i];
                }
            }
            if (pass == 0 && wg == 0) *hdr = Header{0u, 0u, 0u, 0u, 0xFFFFFFFFu, 0u};
            left = entry[0];
            if (wg == 0) left = State{0u, 0u};
            else if (pass > 0) left = bexit[(long long)((pass - 1) & 1) * L.nwg + wg - 1];
            for (int t = 0; t < HD_WG; ++t) ex[0][t] = exit[t];
            bool open = false;
            for (int it = 0; it < HD_INNER; ++it) {
                const int cur = it & 1;
                bool any = false;
                for (int t = 0; t < HD_WG; ++t) {
                    const State want = t == 0 ? left : ex[cur][t - 1];
                    if (live[t] && !same(want, entry[t])) {
                        entry[t] = want;
                        CountSink c;
                        exit[t] = run(st, d.tables, entry[t], end_of(wg * HD_WG + t, st.len), G, c, unused);
                        cnt[t] = c.blocks | (c.markers << 16);
                        dirty[t] = any = true;
                    }
                    ex[cur ^ 1][t] = exit[t];
                }
                open = any;
                if (!any) break;
            }
            open_g[wg] = open ? 1u : 0u;
            for (int t = 0; t < HD_WG; ++t) {
                const long long i = wg * HD_WG + t;
                if (!live[t]) continue;
                entry_g[i] = entry[t];
                exit_g[i] = exit[t];
                cnt_g[i] = cnt[t];
                if (t == HD_WG - 1 || i == L.nsub - 1) bexit[(long long)(pass & 1) * L.nwg + wg] = exit[t];
                if (dirty[t] && pass > 0 && hdr->passes < (uint32_t)pass) hdr->passes = (uint32_t)pass;
            }
        }
    }
    // jpeg_hd_scan
    uint32_t carry = 0, mcarry = 0;
    bool ok = true;
    for (long long i = 0; i < L.nsub; ++i) {
        const State want = i == 0 ? State{0u, 0u} : exit_g[i - 1];
        if (!same(want, entry_g[i])) ok = false;
        first_g[i] = carry;
        carry += cnt_g[i] & 0xFFFFu;
        if (G.restart) mfirst_g[i] = mcarry;
        mcarry += cnt_g[i] >> 16;
    }
    hdr->synced = ok ? 1u : 0u;
    hdr->total = carry;
    hdr->markers = mcarry;
    // jpeg_hd_zero
    std::memset(d.coef, 0, (size_t)G.nblk * 128);
    // jpeg_hd_write
    if (hdr->synced)
        for (long long i = 0; i < L.nsub; ++i) {
            if ((long long)first_g[i] >= G.nblk) continue;
            WriteSink sink(d, G, first_g[i], G.restart ? (long long)mfirst_g[i] : 0);
            uint32_t bad = 0;
            const State out = run(st, d.tables, entry_g[i], end_of(i, st.len), G, sink, bad);
            hdr->flags |= bad;
            if (sink.finished) {
                if (hdr->done) {
                    std::fprintf(stderr, "two subsequences completed the last block\n");
                    std::exit(2);
                }
                hdr->endpos = out.pos;
                hdr->done = 1;
            }
        }
    // jpeg_hd_dc
    bool range_bad = false;
    if (hdr->synced)
        for (int c = 0; c < d.ncomp; ++c) {
            const long long nb = c == 0 ? G.mcus * G.lum : G.mcus;
            const long long per = G.restart ? (long long)G.restart * (c == 0 ? G.lum : 1) : 0;  // blocks of the component per interval
            long long sum = 0;
            for (long long k = 0; k < nb; ++k) {
                const long long at = component_block(d, G, c, k) * 64;
                if (per && k % per == 0) sum = 0;
                sum += d.coef[at];
                if (sum < -32768 || sum > 32767) range_bad = true;
                d.coef[at] = (int16_t)(int32_t)sum;
            }
        }
    return verdict(st, G, *hdr, range_bad);
}

static long g_cases = 0, g_ok = 0, g_refused_prepare = 0, g_refused_both = 0, g_unsync = 0, g_failures = 0, g_marker_subs = 0;
static int g_max_passes = 0;

// A marker is a hard synchronisation point: for every subsequence that holds one (its first FF), run() from five entry
// states in front of it - the subsequence's first bit and three further bit positions, other places in the MCU and the
// block - returns one and the same exit state.
static void marker_exits(const pp_jpeg_hd_desc& d) {
    const Geometry G = geometry(d);
    if (!G.valid) return;
    const Stream st{d.stream, d.stream_bytes};
    const long long nsub = layout(d.stream_bytes, true).nsub;
    for (long long i = 0; i < nsub; ++i) {
        long long m = -1;
        for (long long b = i * HD_S; b < end_of(i, st.len) && m < 0; ++b)
            if (marker_at(st, b)) m = b;
        if (m < 0) continue;
        ++g_marker_subs;
        const uint32_t first = canonical(st, (uint32_t)(i * HD_S * 8)), span = (uint32_t)(m * 8) - first;
        const State in[5] = {State{first, 0u}, State{first + span / 4, (uint32_t)((G.bpm - 1) << 8) | 5u}, State{first + span / 2 + 3, 63u},
                             State{first + span * 3 / 4 + 1, 1u}, State{first + (span > 3 ? 3u : 0u), (uint32_t)((G.bpm / 2) << 8)}};
        State out[5];
        for (int e = 0; e < 5; ++e) {
            CountSink c;
            uint32_t bad = 0;
            out[e] = run(st, d.tables, State{canonical(st, in[e].pos), in[e].bk}, end_of(i, st.len), G, c, bad);
            if (!same(out[e], out[0])) {
                ++g_failures;
                std::printf("MARKER EXIT subsequence %lld: entry %d leaves (%u, %u), entry 0 (%u, %u)\n", i, e, out[e].pos, out[e].bk, out[0].pos, out[0].bk);
            }
        }
    }
}

// One input through the preparation, the restated device decoder and the host decoder.
static void check(const std::vector<uint8_t>& bytes, int sync_passes, bool must_sync, const char* what) {
    ++g_cases;
    uint8_t* data = (uint8_t*)std::malloc(bytes.size() ? bytes.size() : 1);
    if (!bytes.empty()) std::memcpy(data, bytes.data(), bytes.size());
    pp_jpeg_scan* scan = (pp_jpeg_scan*)std::malloc(sizeof(pp_jpeg_scan));
    const int ps = jpeg::scan_prepare(data, bytes.size(), scan, true);
    if (ps != PP_OK) {
        ++g_refused_prepare;
        if (!jpeg::g_reason[0]) {
            std::fprintf(stderr, "%s: refusal without a reason\n", what);
            std::exit(2);
        }
        pp_jpeg_info pi;  // the preparation refuses what the probe refuses, and files with a restart interval
        if (jpeg::probe(data, bytes.size(), &pi) != PP_OK && !scan->info.reason[0]) ++g_failures;
    } else if (scan->info.coef_count < (1ll << 26)) {
        const pp_jpeg_info& info = scan->info;
        const long long len = scan->stream_bytes;
        if (scan->stream_offset < 0 || len < 0 || (size_t)(scan->stream_offset + len) > bytes.size()) {
            std::fprintf(stderr, "%s: segment outside the file\n", what);
            std::exit(2);
        }
        uint8_t* stream = (uint8_t*)std::malloc(len ? (size_t)len : 1);
        std::memcpy(stream, data + scan->stream_offset, (size_t)len);
        pp_jpeg_huff_table* tabs = (pp_jpeg_huff_table*)std::malloc(2 * (size_t)info.ncomp * sizeof(pp_jpeg_huff_table));
        std::memcpy(tabs, scan->tables, 2 * (size_t)info.ncomp * sizeof(pp_jpeg_huff_table));
        int16_t* coef = (int16_t*)std::aligned_alloc(16, (size_t)info.coef_count * 2);
        const Layout L = layout(len, info.restart_interval != 0);
        uint8_t* scratch = (uint8_t*)std::aligned_alloc(16, (size_t)L.total);
        std::memset(scratch, 0xA5, (size_t)L.total);
        pp_jpeg_hd_result slot;
        pp_jpeg_hd_desc d{stream, tabs, coef, scratch, &slot, len, info.hs, info.vs, info.mcus_x, info.mcus_y, info.ncomp, info.restart_interval};
        if (info.restart_interval) marker_exits(d);
        const pp_jpeg_hd_result r = emulate(d, sync_passes);
        std::vector<int16_t> want((size_t)info.coef_count);
        uint16_t qt[192];
        pp_jpeg_info hi;
        const int hs = jpeg::entropy_decode(data, bytes.size(), want.data(), info.coef_count, qt, &hi);
        bool fail = false;
        if (r.status == PP_OK) {
            ++g_ok;
            if (r.passes > g_max_passes) g_max_passes = r.passes;
            fail = hs != PP_OK || std::memcmp(want.data(), coef, (size_t)info.coef_count * 2) != 0 ||
                   std::memcmp(qt, scan->qtables, 128 * (size_t)info.ncomp) != 0;
        } else if (r.reason == HD_NOT_SYNCHRONISED) {
            ++g_unsync;
            fail = must_sync;
        } else {
            ++g_refused_both;
            fail = hs == PP_OK;
        }
        if (fail) {
            ++g_failures;
            std::printf("MISMATCH %s: device status %d reason %d passes %d blocks %d, host status %d (%s)\n", what, r.status, r.reason, r.passes,
                        r.blocks, hs, hs == PP_OK ? "" : jpeg::g_reason);
        }
        std::free(stream);
        std::free(tabs);
        std::free(coef);
        std::free(scratch);
    }
    std::free(scan);
    std::free(data);
}

int main(int argc, char** argv) {
    int rounds = 400;
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
        check(orig, HD_MAX_PASSES, true, path);
        check(orig, 1, false, path);
        check(orig, HD_DEFAULT_PASSES, false, path);
        if (orig.size() < 8) continue;
        check(std::vector<uint8_t>(orig.begin(), orig.begin() + orig.size() / 2), HD_MAX_PASSES, false, "half");
        check(std::vector<uint8_t>(orig.begin(), orig.end() - 6), HD_MAX_PASSES, false, "last_mcu");
        {
            std::vector<uint8_t> m(orig.begin(), orig.end() - 6);
            m.push_back(0xFF);
            m.push_back(0xD9);
            check(m, HD_MAX_PASSES, false, "last_mcu_eoi");
        }
        pp_jpeg_scan scan;
        if (jpeg::scan_prepare(orig.data(), orig.size(), &scan, true) != PP_OK) continue;
        const size_t off = (size_t)scan.stream_offset, len = (size_t)scan.stream_bytes;
        for (size_t cut = 0; cut < 40 && cut < len; ++cut) {  // the segment without its last bytes, EOI put back
            std::vector<uint8_t> m(orig.begin(), orig.begin() + off + len - 1 - cut);
            m.push_back(0xFF);
            m.push_back(0xD9);
            check(m, HD_MAX_PASSES, false, "segment cut");
        }
        for (int k = 0; k < 32 && len > 0; ++k) {  // the fixed bit flips of tests/test_jpeg_huffdec_gpu.py
            std::vector<uint8_t> m = orig;
            m[off + len * k / 32] ^= (uint8_t)(1u << (k % 8));
            check(m, HD_MAX_PASSES, false, "fixed flip");
        }
        if (scan.info.restart_interval) {  // marker damage: one deleted, two numbers swapped, one doubled (an empty interval), D7 -> D0
            std::vector<size_t> at;  // the D0..D7 byte of every marker
            for (size_t b = off; b + 1 < off + len; ++b) {
                if (orig[b] != 0xFF) continue;
                if (orig[b + 1] == 0x00) ++b;
                else if (orig[b + 1] >= 0xD0 && orig[b + 1] <= 0xD7) at.push_back(++b);
            }
            for (size_t q = 0; q < at.size(); q += at.size() > 12 ? at.size() / 12 : 1) {
                std::vector<uint8_t> m = orig;
                m.erase(m.begin() + at[q] - 1, m.begin() + at[q] + 1);
                check(m, HD_MAX_PASSES, false, "marker deleted");
                m = orig;
                m.insert(m.begin() + at[q] + 1, orig.begin() + at[q] - 1, orig.begin() + at[q] + 1);
                check(m, HD_MAX_PASSES, false, "marker doubled");
                if (q + 1 < at.size()) {
                    m = orig;
                    std::swap(m[at[q]], m[at[q + 1]]);
                    check(m, HD_MAX_PASSES, false, "markers swapped");
                }
                if (orig[at[q]] == 0xD7) {
                    m = orig;
                    m[at[q]] = 0xD0;
                    check(m, HD_MAX_PASSES, false, "D7 to D0");
                }
            }
        }
        for (int r = 0; r < rounds && len > 0; ++r) {
            std::vector<uint8_t> m = orig;
            const size_t at = off + rnd() % len;
            if (rnd() & 1) m[at] ^= (uint8_t)(1u << (rnd() % 8));  // one bit
            else m.erase(m.begin() + at);                           // one byte gone
            check(m, (r & 3) == 3 ? HD_DEFAULT_PASSES : HD_MAX_PASSES, false, "mutation");
        }
    }
    std::printf("jpeg_huffdec_host_check: %zu files, %ld cases: %ld decoded equal to the host, %ld refused by the preparation, %ld refused by both decoders, "
                "%ld not synchronised, at most %d passes, %ld subsequences with a marker left alike from 5 entries, %ld failures\n",
                files.size(), g_cases, g_ok, g_refused_prepare, g_refused_both, g_unsync, g_max_passes, g_marker_subs, g_failures);
    return g_failures != 0;
}
