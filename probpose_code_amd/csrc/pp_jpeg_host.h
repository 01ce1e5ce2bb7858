// The serial half of the split JPEG decoder: marker parsing and Huffman decoding on the host. Plain C++ (no HIP, no
// state besides the thread-local reason string), so it also compiles alone into a sanitised test program
// (scripts/jpeg_host_fuzz.cpp). The data-parallel half - dequantisation, inverse DCT, chroma upsampling, colour - is
// csrc/pp_jpeg.hip.
//
// Accepted: baseline / extended sequential Huffman files (SOF0, SOF1) of 8-bit precision with one component, or three
// components whose chroma is sampled 1x1 and whose luma is sampled 1x1, 2x1 or 2x2, in ONE interleaved scan; any DQT / DHT
// tables; restart intervals. Everything else - and every irregularity of the stream - is PP_ERR_UNSUPPORTED with a reason:
// the caller then decodes the file with the host decoder it used before. Nothing is guessed, no partial image is returned.
// Every read of the input is checked against `size`, every write against the caller's capacities.
//
// scan_prepare (pp_jpeg_scan_prepare) is the host's share when the Huffman codes are decoded on the device as well
// (csrc/pp_jpeg_huffdec.hip): the same header parser, the components' tables in the form the device reads, and the bounds of
// the entropy-coded segment by a search for FF bytes - no bit of it is decoded here. It refuses what the parser refuses,
// files with a restart interval and a segment that no EOI marker ends. scan_prepare_restart (pp_jpeg_scan_prepare_restart)
// is the same search that takes a file with a restart interval as well: its RSTn markers, and the fill bytes in front of
// them, belong to the segment, which the first other marker ends. Their order and number are the device decoder's to check.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/probpose_mi355x.h"

// This header itself stays plain host C++. It also carries PP_HOST_DEVICE, because it is the one header both device cores
// (pp_jpeg_entropy_core.h, pp_jpeg_huffdec_core.h) include for jpeg::kNatural: the function qualifier of what they share
// with their sequential host checks - host and device under hipcc, plain inline under a host compiler.
#if defined(__HIPCC__)
#define PP_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define PP_HOST_DEVICE inline
#endif

namespace pp {
namespace jpeg {

inline thread_local char g_reason[96] = "";  // why the last probe / decode of this thread refused a file

inline int refuse(pp_jpeg_info* info, const char* why) {
    std::snprintf(g_reason, sizeof(g_reason), "%s", why);
    if (info) {
        info->supported = 0;
        std::snprintf(info->reason, sizeof(info->reason), "%s", why);
    }
    return PP_ERR_UNSUPPORTED;
}

// zigzag position -> natural (row-major) position
static constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int LOOK_BITS = 9;
constexpr int kMaxMarkerFill = 8;  // FF bytes of a restart marker the device decoder recognises (HD_MAX_FILL): the marker's own and seven fill bytes

struct HuffTable {
    bool present = false;
    uint8_t vals[256];
    int32_t maxcode[18];  // largest code of each length, -1: none
    int32_t valoffset[17];  // vals index of a code = code + valoffset[length]
    uint16_t look[1 << LOOK_BITS];  // (length << 8) | symbol for codes of at most LOOK_BITS bits, 0: longer
};

// Canonical table from the 16 counts and the symbols (ITU T.81 annex C). False: counts that no prefix code has.
inline bool build_huff(HuffTable& h, const uint8_t* counts, const uint8_t* symbols, int n_symbols) {
    std::memset(h.look, 0, sizeof(h.look));
    std::memset(h.vals, 0, sizeof(h.vals));  // (scan_prepare copies the whole table)
    std::memcpy(h.vals, symbols, (size_t)n_symbols);
    int32_t code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        h.valoffset[len] = k - code;
        const int cnt = counts[len - 1];
        if (code + cnt > (1 << len)) return false;
        for (int i = 0; i < cnt; ++i, ++k, ++code)
            if (len <= LOOK_BITS) {
                const int lo = code << (LOOK_BITS - len);
                for (int j = 0; j < (1 << (LOOK_BITS - len)); ++j) h.look[lo + j] = (uint16_t)((len << 8) | symbols[k]);
            }
        h.maxcode[len] = cnt ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    h.present = true;
    return true;
}

struct Component {
    int id, h, v, tq, td, ta;
};

struct Header {
    int width = 0, height = 0, ncomp = 0, precision = 0;
    Component comp[3];
    int restart_interval = 0;
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = 0;
    bool have_q[4] = {false, false, false, false};
    uint16_t q[4][64];  // natural order
    HuffTable dc[4], ac[4];
    size_t scan_pos = 0;  // first byte of the entropy-coded data
};

inline int fill_info(const Header& h, pp_jpeg_info* info) {
    info->width = h.width;
    info->height = h.height;
    info->ncomp = h.ncomp;
    info->precision = h.precision;
    info->hs = h.comp[0].h;
    info->vs = h.comp[0].v;
    info->mcus_x = (h.width + 8 * info->hs - 1) / (8 * info->hs);
    info->mcus_y = (h.height + 8 * info->vs - 1) / (8 * info->vs);
    long long blocks = 0;
    for (int c = 0; c < 3; ++c) {
        info->comp_bw[c] = c < h.ncomp ? info->mcus_x * h.comp[c].h : 0;
        info->comp_bh[c] = c < h.ncomp ? info->mcus_y * h.comp[c].v : 0;
        blocks += (long long)info->comp_bw[c] * info->comp_bh[c];
    }
    info->restart_interval = h.restart_interval;
    info->coef_count = blocks * 64;
    info->supported = 1;
    info->reason[0] = 0;
    return PP_OK;
}

// Markers up to and including SOS. PP_OK: `h` describes a file of the accepted subset and h.scan_pos is its entropy data.
inline int parse_header(const uint8_t* d, size_t size, Header& h, pp_jpeg_info* info) {
    if (size < 4 || d[0] != 0xFF || d[1] != 0xD8) return refuse(info, "not a JPEG file (no SOI)");
    size_t pos = 2;
    for (;;) {
        if (pos + 2 > size) return refuse(info, "file ends inside the headers");
        if (d[pos] != 0xFF) return refuse(info, "marker expected in the headers");
        while (pos < size && d[pos] == 0xFF) ++pos;  // fill bytes
        if (pos >= size) return refuse(info, "file ends inside the headers");
        const int m = d[pos++];
        if (m == 0xD9) return refuse(info, "EOI before any scan");
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) return refuse(info, "stray marker in the headers");
        if (pos + 2 > size) return refuse(info, "file ends inside the headers");
        const size_t len = ((size_t)d[pos] << 8) | d[pos + 1];
        if (len < 2 || pos + len > size) return refuse(info, "marker segment runs past the end of the file");
        const uint8_t* s = d + pos + 2;  // segment payload, n bytes
        const size_t n = len - 2;
        pos += len;
        if (m == 0xC0 || m == 0xC1) {
            if (h.have_sof) return refuse(info, "several frames");
            if (n < 6) return refuse(info, "short SOF segment");
            h.precision = s[0];
            h.height = (s[1] << 8) | s[2];
            h.width = (s[3] << 8) | s[4];
            h.ncomp = s[5];
            if (h.precision != 8) return refuse(info, "sample precision is not 8 bits");
            if (h.ncomp != 1 && h.ncomp != 3) return refuse(info, "neither 1 nor 3 components");
            if (n != 6 + 3 * (size_t)h.ncomp) return refuse(info, "bad SOF length");
            if (h.width == 0 || h.height == 0) return refuse(info, "zero image dimension");
            for (int c = 0; c < h.ncomp; ++c) {
                Component& k = h.comp[c];
                k.id = s[6 + 3 * c];
                k.h = s[7 + 3 * c] >> 4;
                k.v = s[7 + 3 * c] & 15;
                k.tq = s[8 + 3 * c];
                if (k.tq > 3) return refuse(info, "bad quantisation table index");
            }
            const Component* k = h.comp;
            const bool ok = h.ncomp == 1 ? (k[0].h == 1 && k[0].v == 1)
                                         : (k[1].h == 1 && k[1].v == 1 && k[2].h == 1 && k[2].v == 1 &&
                                            ((k[0].h == 1 && k[0].v == 1) || (k[0].h == 2 && k[0].v == 1) || (k[0].h == 2 && k[0].v == 2)));
            if (!ok) return refuse(info, "sampling factors outside 4:4:4 / 4:2:2 / 4:2:0 / grey");
            h.have_sof = true;
        } else if ((m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC)) {
            return refuse(info, m == 0xC2 ? "progressive coding" : "coding process other than sequential Huffman");
        } else if (m == 0xCC) {
            return refuse(info, "arithmetic coding");
        } else if (m == 0xC4) {
            size_t o = 0;
            while (o < n) {
                if (o + 17 > n) return refuse(info, "short DHT segment");
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return refuse(info, "bad Huffman table index");
                int total = 0;
                for (int i = 0; i < 16; ++i) total += s[o + 1 + i];
                if (total > 256 || o + 17 + (size_t)total > n) return refuse(info, "bad Huffman table size");
                if (!build_huff(tc ? h.ac[th] : h.dc[th], s + o + 1, s + o + 17, total)) return refuse(info, "Huffman counts are no prefix code");
                o += 17 + (size_t)total;
            }
        } else if (m == 0xDB) {
            size_t o = 0;
            while (o < n) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (pq > 1 || tq > 3) return refuse(info, "bad quantisation table header");
                const size_t need = 1 + 64 * (size_t)(pq + 1);
                if (o + need > n) return refuse(info, "short DQT segment");
                for (int i = 0; i < 64; ++i)
                    h.q[tq][kNatural[i]] = pq ? (uint16_t)((s[o + 1 + 2 * i] << 8) | s[o + 2 + 2 * i]) : s[o + 1 + i];
                h.have_q[tq] = true;
                o += need;
            }
        } else if (m == 0xDD) {
            if (n != 2) return refuse(info, "bad DRI length");
            h.restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xE0) {
            if (n >= 5 && std::memcmp(s, "JFIF", 5) == 0) h.jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && std::memcmp(s, "Adobe", 5) == 0) {
                h.adobe = true;
                h.adobe_transform = s[11];
            }
        } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE) {
            // application data / comment: skipped
        } else if (m == 0xDA) {
            if (!h.have_sof) return refuse(info, "scan before the frame header");
            if (n < 1 || s[0] != h.ncomp || n != 4 + 2 * (size_t)h.ncomp) return refuse(info, "scan does not hold all components (several scans)");
            for (int c = 0; c < h.ncomp; ++c) {
                Component& k = h.comp[c];
                if (s[1 + 2 * c] != k.id) return refuse(info, "scan components out of frame order");
                k.td = s[2 + 2 * c] >> 4;
                k.ta = s[2 + 2 * c] & 15;
                if (k.td > 3 || k.ta > 3 || !h.dc[k.td].present || !h.ac[k.ta].present) return refuse(info, "missing Huffman table");
                if (!h.have_q[k.tq]) return refuse(info, "missing quantisation table");
            }
            const uint8_t* t = s + 1 + 2 * h.ncomp;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) return refuse(info, "spectral selection / successive approximation");
            if (h.ncomp == 3) {
                if (h.adobe && h.adobe_transform != 1) return refuse(info, "Adobe marker: not YCbCr");
                if (!h.adobe && !h.jfif && h.comp[0].id == 'R' && h.comp[1].id == 'G' && h.comp[2].id == 'B')
                    return refuse(info, "RGB component ids");
            }
            h.scan_pos = pos;
            return PP_OK;
        } else {
            return refuse(info, "marker outside the supported subset");
        }
    }
}

// MSB-first bit reader over entropy-coded data: FF 00 is a data byte FF, any other FF xx ends the segment. Past a marker
// (or the end of the input) it feeds zero bits and counts them (`fake`): whoever consumed one has run past the data.
struct BitReader {
    const uint8_t* d;
    size_t pos, size;
    uint64_t acc = 0;
    int n = 0, fake = 0;
    bool stopped = false;

    inline void fill() {
        while (n <= 56) {
            uint64_t b = 0;
            if (!stopped) {
                if (pos >= size) {
                    stopped = true;
                } else if (d[pos] != 0xFF) {
                    b = d[pos++];
                } else if (pos + 1 < size && d[pos + 1] == 0x00) {
                    b = 0xFF;
                    pos += 2;
                } else {
                    stopped = true;
                }
            }
            if (stopped) fake += 8;
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    inline uint32_t peek(int k) const { return (uint32_t)(acc >> (n - k)) & ((1u << k) - 1u); }
    inline bool overrun() const { return n < fake; }
    inline int real_bits() const { return n - fake; }
};

// One Huffman symbol, -1: no such code.
inline int decode_symbol(BitReader& br, const HuffTable& h) {
    if (br.n < 16) br.fill();
    const uint32_t e = h.look[br.peek(LOOK_BITS)];
    if (e) {
        br.n -= (int)(e >> 8);
        return (int)(e & 255);
    }
    for (int len = LOOK_BITS + 1; len <= 16; ++len) {
        const int32_t code = (int32_t)br.peek(len);
        if (code <= h.maxcode[len]) {
            br.n -= len;
            const int32_t idx = code + h.valoffset[len];
            if (idx < 0 || idx > 255) return -1;
            return h.vals[idx];
        }
    }
    return -1;
}

inline int receive_extend(BitReader& br, int s) {
    if (br.n < s) br.fill();
    const int v = (int)br.peek(s);
    br.n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// pp_jpeg_probe
inline int probe(const uint8_t* data, size_t size, pp_jpeg_info* info) {
    if (!data || !info) {
        std::snprintf(g_reason, sizeof(g_reason), "NULL argument");
        return PP_ERR_INVALID_ARG;
    }
    std::memset(info, 0, sizeof(*info));
    Header h;
    const int st = parse_header(data, size, h, info);
    if (st != PP_OK) {
        if (h.have_sof) {  // geometry of a refused file, as far as it was read
            info->width = h.width;
            info->height = h.height;
            info->ncomp = h.ncomp;
            info->precision = h.precision;
        }
        return st;
    }
    return fill_info(h, info);
}

// pp_jpeg_entropy_decode: coef (coef_capacity int16 values) <- the quantised coefficients, per component
// [block_row][block_col][64] in natural order, padded to whole MCUs; qtables (ncomp x 64 uint16, natural order; room for
// 3 x 64) <- each component's quantisation table.
inline int entropy_decode(const uint8_t* data, size_t size, int16_t* coef, long long coef_capacity, uint16_t* qtables, pp_jpeg_info* info) {
    if (!data || !coef || !qtables || !info) {
        std::snprintf(g_reason, sizeof(g_reason), "NULL argument");
        return PP_ERR_INVALID_ARG;
    }
    std::memset(info, 0, sizeof(*info));
    Header h;
    int st = parse_header(data, size, h, info);
    if (st != PP_OK) return st;
    fill_info(h, info);
    if (coef_capacity < info->coef_count) {
        refuse(info, "coefficient buffer too small");
        return PP_ERR_WORKSPACE;
    }
    std::memset(coef, 0, (size_t)info->coef_count * sizeof(int16_t));
    int16_t* plane[3];
    long long off = 0;
    for (int c = 0; c < h.ncomp; ++c) {
        plane[c] = coef + off;
        off += (long long)info->comp_bw[c] * info->comp_bh[c] * 64;
        std::memcpy(qtables + 64 * c, h.q[h.comp[c].tq], 64 * sizeof(uint16_t));
    }
    BitReader br{data, h.scan_pos, size};
    int pred[3] = {0, 0, 0};
    const int ri = h.restart_interval;
    int next_rst = 0;
    const long long n_mcus = (long long)info->mcus_x * info->mcus_y;
    long long mcu = 0;
    for (int my = 0; my < info->mcus_y; ++my)
        for (int mx = 0; mx < info->mcus_x; ++mx, ++mcu) {
            if (ri > 0 && mcu > 0 && mcu % ri == 0) {
                // the bits left before the marker are padding of the last byte; the marker itself must be the expected RSTn
                if (br.real_bits() >= 8) return refuse(info, "data where a restart marker is due");
                size_t p = br.pos;
                if (p >= size || data[p] != 0xFF) return refuse(info, "missing restart marker");
                while (p < size && data[p] == 0xFF) ++p;
                if (p >= size || data[p] != 0xD0 + next_rst) return refuse(info, "wrong restart marker");
                next_rst = (next_rst + 1) & 7;
                br.pos = p + 1;
                br.acc = 0;
                br.n = br.fake = 0;
                br.stopped = false;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < h.ncomp; ++c) {
                const HuffTable& dc = h.dc[h.comp[c].td];
                const HuffTable& ac = h.ac[h.comp[c].ta];
                for (int v = 0; v < h.comp[c].v; ++v)
                    for (int u = 0; u < h.comp[c].h; ++u) {
                        const long long b = (long long)(my * h.comp[c].v + v) * info->comp_bw[c] + (mx * h.comp[c].h + u);
                        int16_t* blk = plane[c] + b * 64;  // inside coef_count by the block grid above
                        int s = decode_symbol(br, dc);
                        if (s < 0) return refuse(info, "bad Huffman code");
                        if (s > 11) return refuse(info, "DC magnitude category above 11");
                        if (s) pred[c] += receive_extend(br, s);
                        if (pred[c] < -32768 || pred[c] > 32767) return refuse(info, "DC coefficient out of range");
                        blk[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            const int rs = decode_symbol(br, ac);
                            if (rs < 0) return refuse(info, "bad Huffman code");
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;  // end of block
                                k += 16;
                                if (k > 63) return refuse(info, "coefficient index past 63");
                                continue;
                            }
                            k += r;
                            if (k > 63) return refuse(info, "coefficient index past 63");
                            if (s > 10) return refuse(info, "AC magnitude category above 10");
                            blk[kNatural[k]] = (int16_t)receive_extend(br, s);
                            ++k;
                        }
                        if (br.overrun()) return refuse(info, "data ends before the last MCU");
                    }
            }
        }
    (void)n_mcus;
    // after the last MCU: padding of the last byte, then EOI
    if (br.real_bits() >= 8) return refuse(info, "data after the last MCU");
    size_t p = br.pos;
    if (p >= size || data[p] != 0xFF) return refuse(info, "no EOI after the scan");
    while (p < size && data[p] == 0xFF) ++p;
    if (p >= size || data[p] != 0xD9) return refuse(info, "no EOI after the scan (several scans?)");
    return PP_OK;
}

// pp_jpeg_scan_prepare: what the device Huffman decoder (csrc/pp_jpeg_huffdec.hip) needs of a file, read from its headers.
// No bit of the entropy-coded segment is decoded here: its end is the first FF that no 00 follows, and the marker there
// must be EOI (what entropy_decode demands behind the last MCU). restart: a file with a restart interval is taken too; in
// it an FF run that D0..D7 ends is part of the segment. A run of more than kMaxMarkerFill FF bytes there is refused (the
// host decoder takes it, the device decoder's reader looks no further).
inline int scan_prepare(const uint8_t* data, size_t size, pp_jpeg_scan* scan, bool restart = false) {
    if (!data || !scan) {
        std::snprintf(g_reason, sizeof(g_reason), "NULL argument");
        return PP_ERR_INVALID_ARG;
    }
    std::memset(scan, 0, sizeof(*scan));
    pp_jpeg_info* info = &scan->info;
    Header h;
    const int st = parse_header(data, size, h, info);
    if (st != PP_OK) return st;
    fill_info(h, info);
    if (h.restart_interval != 0 && !restart) return refuse(info, "restart interval: the device Huffman decoder takes files without one");
    for (int c = 0; c < h.ncomp; ++c) {
        std::memcpy(scan->qtables + 64 * c, h.q[h.comp[c].tq], 64 * sizeof(uint16_t));
        const HuffTable* src[2] = {&h.dc[h.comp[c].td], &h.ac[h.comp[c].ta]};
        for (int t = 0; t < 2; ++t) {
            pp_jpeg_huff_table& dst = scan->tables[2 * c + t];
            std::memcpy(dst.look, src[t]->look, sizeof(dst.look));
            std::memcpy(dst.vals, src[t]->vals, sizeof(dst.vals));
            for (int len = 1; len <= 17; ++len) dst.maxcode[len] = src[t]->maxcode[len];
            for (int len = 1; len <= 16; ++len) dst.valoffset[len] = src[t]->valoffset[len];
        }
    }
    size_t end = h.scan_pos;
    for (;;) {
        const void* ff = end < size ? std::memchr(data + end, 0xFF, size - end) : nullptr;
        if (!ff) return refuse(info, "no EOI after the scan");
        end = (size_t)(reinterpret_cast<const uint8_t*>(ff) - data);
        if (end + 1 < size && data[end + 1] == 0x00) {  // a stuffed data byte
            end += 2;
            continue;
        }
        if (h.restart_interval == 0) break;
        size_t m = end;
        while (m < size && data[m] == 0xFF) ++m;
        if (m >= size || data[m] < 0xD0 || data[m] > 0xD7) break;
        if (m - end > (size_t)kMaxMarkerFill) return refuse(info, "more than 7 fill bytes in front of a restart marker");
        end = m + 1;
    }
    size_t p = end;
    while (p < size && data[p] == 0xFF) ++p;
    if (p >= size || data[p] != 0xD9) return refuse(info, "no EOI after the scan (several scans?)");
    if (end - h.scan_pos >= ((size_t)1 << 28)) return refuse(info, "entropy-coded segment of 2^28 bytes or more");
    scan->stream_offset = (int64_t)h.scan_pos;
    scan->stream_bytes = (int64_t)(end - h.scan_pos);
    return PP_OK;
}

}  // namespace jpeg
}  // namespace pp
