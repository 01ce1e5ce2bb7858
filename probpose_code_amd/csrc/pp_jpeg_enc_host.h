// The serial half of the split JPEG encoder: quantisation tables from a quality, the block geometry of an image, and the
// baseline Huffman coder that turns the quantised coefficients of csrc/pp_jpeg_enc.hip into a JFIF file. Plain C++ (no HIP,
// no allocation, no state besides the thread-local reason string of pp_jpeg_host.h), so it also compiles alone into a
// sanitised test program (scripts/jpeg_enc_host_fuzz.cpp).
//
// The file: SOI, JFIF APP0, DQT (one segment per distinct table), SOF0, DHT (the four tables of ITU T.81 annex K.3 - K.6),
// DRI when a restart interval is asked for, SOS (one interleaved scan), entropy-coded data with byte stuffing, EOI.
// Quantisation tables follow libjpeg: annex K.1 scaled by jpeg_quality_scaling, clamped to 1..255 (force_baseline).
// Every write is checked against the caller's capacity; every coefficient against what a baseline code can express.
// entropy_encode is also the contract of the device coder (csrc/pp_jpeg_entropy.hip), which writes the bytes between the SOS
// header and EOI bit for bit and derives its code tables from the arrays below; write_headers gives the bytes in front.
// The Huffman tables of a file are a parameter (HuffSpec): annex K's by default, the image's own optimal ones in the host form
// of csrc/pp_jpeg_opt_core.h (entropy_encode_opt), which calls entropy_encode_with and write_headers with the tables it built.
#pragma once
#include "pp_jpeg_host.h"

namespace pp {
namespace jpeg {

// ITU T.81 annex K.1, natural (row-major) order
static const uint8_t kStdLumaQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                      69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                      81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t kStdChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                        99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// ITU T.81 annex K.3 - K.6: code counts per length 1..16, then the symbols in code order
static constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
static constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

inline int enc_fail(int code, const char* why) {
    std::snprintf(g_reason, sizeof(g_reason), "%s", why);
    return code;
}

// pp_jpeg_quality_tables: qtables (3 x 64 uint16, natural order: luma, chroma, chroma) of libjpeg's jpeg_set_quality(quality,
// force_baseline = TRUE).
inline int quality_tables(int quality, uint16_t* qtables) {
    if (!qtables) return enc_fail(PP_ERR_INVALID_ARG, "NULL argument");
    if (quality < 1 || quality > 100) return enc_fail(PP_ERR_INVALID_ARG, "quality outside 1..100");
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 64; ++i) {
            int v = ((c ? kStdChromaQ[i] : kStdLumaQ[i]) * scale + 50) / 100;
            qtables[64 * c + i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    return PP_OK;
}

// pp_jpeg_encode_plan: the pp_jpeg_info of a width x height YCbCr file. subsampling: 0 4:4:4, 1 4:2:2, 2 4:2:0.
inline int encode_plan(int width, int height, int subsampling, pp_jpeg_info* info) {
    if (!info) return enc_fail(PP_ERR_INVALID_ARG, "NULL argument");
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return enc_fail(PP_ERR_INVALID_ARG, "image sides outside 1..65535");
    if (subsampling < 0 || subsampling > 2) return enc_fail(PP_ERR_INVALID_ARG, "subsampling is none of 0 (4:4:4), 1 (4:2:2), 2 (4:2:0)");
    std::memset(info, 0, sizeof(*info));
    Header h;
    h.width = width;
    h.height = height;
    h.ncomp = 3;
    h.precision = 8;
    h.comp[0] = Component{1, subsampling ? 2 : 1, subsampling == 2 ? 2 : 1, 0, 0, 0};
    h.comp[1] = Component{2, 1, 1, 1, 1, 1};
    h.comp[2] = Component{3, 1, 1, 1, 1, 1};
    return fill_info(h, info);
}

// True: `info` is what encode_plan gives for its own width, height and sampling (so coef_count bounds every block index).
inline bool plan_consistent(const pp_jpeg_info& i) {
    if (i.ncomp != 3 || i.precision != 8 || i.width < 1 || i.height < 1 || i.width > 65535 || i.height > 65535) return false;
    if (!((i.hs == 1 && i.vs == 1) || (i.hs == 2 && i.vs == 1) || (i.hs == 2 && i.vs == 2))) return false;
    pp_jpeg_info want;
    if (encode_plan(i.width, i.height, i.hs == 1 ? 0 : (i.vs == 1 ? 1 : 2), &want) != PP_OK) return false;
    if (i.mcus_x != want.mcus_x || i.mcus_y != want.mcus_y || i.coef_count != want.coef_count) return false;
    for (int c = 0; c < 3; ++c)
        if (i.comp_bw[c] != want.comp_bw[c] || i.comp_bh[c] != want.comp_bh[c]) return false;
    return true;
}

constexpr long long ENC_HEADER_BOUND = 1024;  // all marker segments of a file (698 bytes with three tables and DRI) and EOI

// pp_jpeg_encoded_bound: a capacity no file of this geometry exceeds, whatever its coefficients and restart interval.
// A block is at most a 16-bit DC code + 11 bits and 63 x (16-bit AC code + 10 bits) = 1665 bits, every byte may be stuffed
// (x 2), and every MCU may end a restart interval: up to a stuffed padding byte and a two-byte marker.
inline long long encoded_bound(const pp_jpeg_info* info) {
    if (!info) return enc_fail(PP_ERR_INVALID_ARG, "NULL argument");
    if (!plan_consistent(*info)) return enc_fail(PP_ERR_INVALID_ARG, "info is not a pp_jpeg_encode_plan result");
    return ENC_HEADER_BOUND + (info->coef_count / 64) * 420 + (long long)info->mcus_x * info->mcus_y * 4;
}

// The four Huffman tables of a file, in the order of its DHT segments: DC luma, AC luma, DC chroma, AC chroma.
struct HuffSpec {
    const uint8_t* bits[4];
    const uint8_t* vals[4];
    int nvals[4];
};

inline const HuffSpec& annex_k_spec() {
    static const HuffSpec spec = {{kDcLumaBits, kAcLumaBits, kDcChromaBits, kAcChromaBits}, {kDcVals, kAcLumaVals, kDcVals, kAcChromaVals}, {12, 162, 12, 162}};
    return spec;
}

struct EncTable {
    uint16_t code[256];
    uint8_t size[256];  // 0: the symbol has no code
};

struct EncTables {
    EncTable dc[2], ac[2];
    uint8_t zigzag_of[64];  // natural position -> zigzag position
    static void derive(EncTable& t, const uint8_t* bits, const uint8_t* vals) {
        std::memset(&t, 0, sizeof(t));
        int code = 0, k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < bits[len - 1]; ++i, ++k, ++code) {
                t.code[vals[k]] = (uint16_t)code;
                t.size[vals[k]] = (uint8_t)len;
            }
            code <<= 1;
        }
    }
    explicit EncTables(const HuffSpec& spec = annex_k_spec()) {
        derive(dc[0], spec.bits[0], spec.vals[0]);
        derive(ac[0], spec.bits[1], spec.vals[1]);
        derive(dc[1], spec.bits[2], spec.vals[2]);
        derive(ac[1], spec.bits[3], spec.vals[3]);
        for (int k = 0; k < 64; ++k) zigzag_of[kNatural[k]] = (uint8_t)k;
    }
};

// MSB-first bit writer into [p, end): a data byte FF is followed by 00. `full` once a byte did not fit. Bits leave four
// bytes at a time - in one store where eight bytes of room are left and none of the four is FF, bytewise otherwise.
struct BitWriter {
    uint8_t* p;
    uint8_t* end;
    uint64_t acc = 0;
    int n = 0;  // bits held in acc, < 32 between calls
    bool full = false;

    inline void byte(uint8_t b) {
        if (p < end) *p++ = b;
        else full = true;
    }
    inline void data_byte(uint8_t b) {
        byte(b);
        if (b == 0xFF) byte(0);
    }
    inline void put(uint32_t bits, int count) {  // count <= 27
        acc = (acc << count) | (bits & ((1u << count) - 1u));
        n += count;
        if (n >= 32) {
            n -= 32;
            const uint32_t w = (uint32_t)(acc >> n), inv = ~w;
            if ((size_t)(end - p) >= 8 && ((inv - 0x01010101u) & w & 0x80808080u) == 0) {  // (no byte of inv is zero: no FF in w)
                const uint8_t b[4] = {(uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w};
                std::memcpy(p, b, 4);
                p += 4;
            } else {
                data_byte((uint8_t)(w >> 24));
                data_byte((uint8_t)(w >> 16));
                data_byte((uint8_t)(w >> 8));
                data_byte((uint8_t)w);
            }
        }
    }
    inline void flush() {  // pad the last byte with ones and write what is held
        if (n & 7) put(0x7F, 8 - (n & 7));
        for (; n >= 8; n -= 8) data_byte((uint8_t)(acc >> (n - 8)));
        acc = 0;
        n = 0;
    }
    inline void raw(const void* src, size_t count) {
        if ((size_t)(end - p) < count) {
            full = true;
            return;
        }
        std::memcpy(p, src, count);
        p += count;
    }
    inline void marker(int m) {
        const uint8_t b[2] = {0xFF, (uint8_t)m};
        raw(b, 2);
    }
    inline void u16(int v) {
        const uint8_t b[2] = {(uint8_t)(v >> 8), (uint8_t)v};
        raw(b, 2);
    }
};

inline int bit_size(int v) {  // magnitude category of |v|
    int s = 0;
    for (unsigned a = (unsigned)(v < 0 ? -v : v); a; a >>= 1) ++s;
    return s;
}

inline void write_dht(BitWriter& w, int tc_th, const uint8_t* bits, const uint8_t* vals, int nvals) {
    w.marker(0xC4);
    w.u16(2 + 1 + 16 + nvals);
    const uint8_t id = (uint8_t)tc_th;
    w.raw(&id, 1);
    w.raw(bits, 16);
    w.raw(vals, (size_t)nvals);
}

// The marker segments SOI .. SOS of a file into w (the caller checks w.full). Cr gets a table of its own where it differs from Cb's.
// One DHT segment per table of `spec`, immediately before DRI / SOS.
inline void put_headers(BitWriter& w, const uint16_t* qtables, const pp_jpeg_info* info, int restart_interval, const HuffSpec& spec = annex_k_spec()) {
    w.marker(0xD8);
    static const uint8_t app0[16] = {0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    w.marker(0xE0);
    w.raw(app0, 16);
    int tq[3] = {0, 1, 1};
    if (std::memcmp(qtables + 64, qtables + 128, 64 * sizeof(uint16_t)) != 0) tq[2] = 2;
    for (int t = 0; t <= tq[2]; ++t) {
        uint8_t seg[65];
        seg[0] = (uint8_t)t;
        for (int i = 0; i < 64; ++i) seg[1 + i] = (uint8_t)qtables[64 * t + kNatural[i]];
        w.marker(0xDB);
        w.u16(67);
        w.raw(seg, 65);
    }
    w.marker(0xC0);
    w.u16(17);
    {
        const uint8_t p = 8;
        w.raw(&p, 1);
        w.u16(info->height);
        w.u16(info->width);
        const uint8_t sof[10] = {3, 1, (uint8_t)((info->hs << 4) | info->vs), (uint8_t)tq[0], 2, 0x11, (uint8_t)tq[1], 3, 0x11, (uint8_t)tq[2]};
        w.raw(sof, 10);
    }
    static const int tc_th[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) write_dht(w, tc_th[t], spec.bits[t], spec.vals[t], spec.nvals[t]);
    if (restart_interval) {
        w.marker(0xDD);
        w.u16(4);
        w.u16(restart_interval);
    }
    static const uint8_t sos[12] = {0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    w.marker(0xDA);
    w.raw(sos, 12);
}

// The argument checks pp_jpeg_entropy_encode and pp_jpeg_write_headers share.
inline int check_file_args(const uint16_t* qtables, const pp_jpeg_info* info, int restart_interval) {
    if (!plan_consistent(*info)) return enc_fail(PP_ERR_INVALID_ARG, "info is not a pp_jpeg_encode_plan result");
    if (restart_interval < 0 || restart_interval > 65535) return enc_fail(PP_ERR_INVALID_ARG, "restart interval outside 0..65535");
    for (int i = 0; i < 192; ++i)
        if (qtables[i] < 1 || qtables[i] > 255) return enc_fail(PP_ERR_INVALID_ARG, "quantisation value outside 1..255 (baseline)");
    return PP_OK;
}

// pp_jpeg_write_headers: the bytes SOI .. SOS of the file entropy_encode writes for these tables, geometry and restart
// interval, into out[0, capacity); *size_out <- their length. The device coder's stream and FF D9 complete the file.
inline int write_headers(const uint16_t* qtables, const pp_jpeg_info* info, int restart_interval, uint8_t* out, size_t capacity,
                         size_t* size_out, const HuffSpec& spec = annex_k_spec()) {
    if (!qtables || !info || !out || !size_out) return enc_fail(PP_ERR_INVALID_ARG, "NULL argument");
    *size_out = 0;
    if (const int st = check_file_args(qtables, info, restart_interval)) return st;
    BitWriter w{out, out + capacity};
    put_headers(w, qtables, info, restart_interval, spec);
    if (w.full) return enc_fail(PP_ERR_WORKSPACE, "output buffer too small");
    *size_out = (size_t)(w.p - out);
    return PP_OK;
}

// pp_jpeg_entropy_encode: coef (info->coef_count int16, the layout of pp_jpeg_entropy_decode) + qtables (3 x 64 uint16,
// natural order, values 1..255) -> a baseline JFIF file in out[0, capacity); *size_out <- its length. spec / tables: the
// file's Huffman tables and the codes derived from them (pp_jpeg_entropy_encode: annex K's).
inline int entropy_encode_with(const int16_t* coef, const uint16_t* qtables, const pp_jpeg_info* info, int restart_interval, uint8_t* out,
                               size_t capacity, size_t* size_out, const HuffSpec& spec, const EncTables& tables) {
    if (!coef || !qtables || !info || !out || !size_out) return enc_fail(PP_ERR_INVALID_ARG, "NULL argument");
    *size_out = 0;
    if (const int st = check_file_args(qtables, info, restart_interval)) return st;
    BitWriter w{out, out + capacity};
    put_headers(w, qtables, info, restart_interval, spec);
    if (w.full) return enc_fail(PP_ERR_WORKSPACE, "output buffer too small");
    // ---- the scan
    const int16_t* plane[3];
    long long off = 0;
    for (int c = 0; c < 3; ++c) {
        plane[c] = coef + off;
        off += (long long)info->comp_bw[c] * info->comp_bh[c] * 64;
    }
    int pred[3] = {0, 0, 0}, next_rst = 0;
    long long mcu = 0;
    for (int my = 0; my < info->mcus_y; ++my) {
        for (int mx = 0; mx < info->mcus_x; ++mx, ++mcu) {
            if (restart_interval && mcu > 0 && mcu % restart_interval == 0) {
                w.flush();
                w.marker(0xD0 + next_rst);
                next_rst = (next_rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < 3; ++c) {
                const int h = c ? 1 : info->hs, v = c ? 1 : info->vs;
                const EncTable& dc = tables.dc[c ? 1 : 0];
                const EncTable& ac = tables.ac[c ? 1 : 0];
                for (int bv = 0; bv < v; ++bv)
                    for (int bh = 0; bh < h; ++bh) {
                        const int16_t* blk = plane[c] + ((long long)(my * v + bv) * info->comp_bw[c] + (mx * h + bh)) * 64;
                        const int diff = (int)blk[0] - pred[c];
                        pred[c] = blk[0];
                        int s = bit_size(diff);
                        if (s > 11) return enc_fail(PP_ERR_INVALID_ARG, "DC difference outside -2047..2047 (baseline)");
                        w.put(dc.code[s], dc.size[s]);
                        if (s) w.put((uint32_t)(diff < 0 ? diff - 1 : diff), s);
                        // the nonzero AC positions in zigzag order, as a bit mask: most rows of most blocks are all zero
                        uint64_t nz = 0;
                        for (int r = 0; r < 8; ++r) {
                            uint64_t half[2];
                            std::memcpy(half, blk + 8 * r, 16);
                            if (half[0] | half[1])
                                for (int i = 8 * r; i < 8 * r + 8; ++i) nz |= (uint64_t)(blk[i] != 0) << tables.zigzag_of[i];
                        }
                        nz &= ~1ull;
                        int prev = 0;
                        while (nz) {
                            const int k = __builtin_ctzll(nz);
                            nz &= nz - 1;
                            int run = k - prev - 1;
                            prev = k;
                            for (; run > 15; run -= 16) w.put(ac.code[0xF0], ac.size[0xF0]);
                            const int a = blk[kNatural[k]];
                            s = bit_size(a);
                            if (s > 10) return enc_fail(PP_ERR_INVALID_ARG, "AC coefficient outside -1023..1023 (baseline)");
                            const int rs = (run << 4) | s;
                            w.put(ac.code[rs], ac.size[rs]);
                            w.put((uint32_t)(a < 0 ? a - 1 : a), s);
                        }
                        if (prev != 63) w.put(ac.code[0], ac.size[0]);
                    }
            }
            if (w.full) return enc_fail(PP_ERR_WORKSPACE, "output buffer too small");
        }
    }
    w.flush();
    w.marker(0xD9);
    if (w.full) return enc_fail(PP_ERR_WORKSPACE, "output buffer too small");
    *size_out = (size_t)(w.p - out);
    return PP_OK;
}

inline int entropy_encode(const int16_t* coef, const uint16_t* qtables, const pp_jpeg_info* info, int restart_interval, uint8_t* out,
                          size_t capacity, size_t* size_out) {
    static const EncTables tables;
    return entropy_encode_with(coef, qtables, info, restart_interval, out, capacity, size_out, annex_k_spec(), tables);
}

}  // namespace jpeg
}  // namespace pp
