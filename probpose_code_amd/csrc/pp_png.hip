// PNG files written from the device: 8-bit truecolour, non-interlaced, one IDAT chunk; per row the cheapest of the five
// filters, then run-length tokens (matches at distance 1 only) in one dynamic deflate block whose Huffman code comes from
// the stream's own histogram. The format, the filters, the token rule, the packer, the checksums and the scratch layout are
// csrc/pp_png_core.h, which the sequential host form (pp_png_encode, pp_zlib_compress, scripts/png_host_check.cpp) runs as
// well; here are the kernels. A batch of streams of any mix of sizes per call, driven by a device table of pp_deflate_desc;
// the deflate stage takes a byte stream and a length, so a descriptor without pixels compresses its bytes as they stand.
//
// What a byte emits depends on its position, its run's start and its run's end: a map, a prefix sum and a scatter, like the
// JPEG coder (csrc/pp_jpeg_entropy.hip), with the code built in between. Eight launches, each the barrier between two
// phases; no workgroup ever waits for another:
//   pp_png_tokens_batch
//     png_filter   a workgroup per row: the five filter costs summed, the choice, the filtered row -> data;
//     png_clear    the 288 histogram words of every stream zeroed;
//     png_hist     a workgroup per tile of PNG_TILE bytes, sixteen bytes a thread: run starts and ends by two scans over the
//                  workgroup, the tokens counted into a histogram in LDS, that added to hist[] with integer atomics; the
//                  tile's Adler-32 pair -> tadler[];
//   the host reads the histograms of the batch in one copy, builds every code and header (pp_deflate_build_code) and uploads
//   them in one copy: the one synchronisation this path adds;
//   pp_png_deflate_batch
//     png_bits     a workgroup per tile: its tokens' bit count -> tsum[];
//     png_scan     one workgroup per stream: exclusive 64-bit prefix sums of tsum[] -> toff[], the Adler-32 combination,
//                  the stream's size and status -> the result slot, whose CRC word starts as crc_init shifted over the stream;
//     png_zero     zeroes the words the bits will be ORed into (only those the size needs);
//     png_pack     a workgroup per tile again: a thread's bit offset is the header's length + toff[tile] + the prefix inside
//                  the tile; it codes its span a second time and ORs the bits into little-endian 32-bit words. Tile 0 ORs the
//                  header in, the thread of the last byte the end-of-block code, the padding and the Adler-32;
//     png_crc      sixteen bytes a thread: copied to out, their CRC-32 partial shifted by the bytes behind them and XORed
//                  into the slot.
// Integer add, OR and XOR into zeroed words commute, every other store has one writer: the bytes are the same from launch to
// launch. Every store into scratch or output is checked against the size of its region. A stream that does not fit its
// capacity is PP_ERR_WORKSPACE with the needed size in the slot and no byte of out written.
//
// The lz match mode (pp_png_tokens_batch_lz, pp_png_deflate_batch_lz; the rule is stated in pp_png_core.h) keeps the eight
// launches and every property above. What changes: which positions start a token depends on the chain of tokens before
// them in the tile, so png_hist gives way to
//     png_parse_lz  a workgroup per tile: the five candidates' equality masks, their first differences by a running minimum
//                   over the workgroup, the choice of every position, the token starts by twelve rounds of pointer doubling
//                   in LDS; the parse (one uint16 per byte) -> scratch, both histograms -> hist[], the Adler-32 pair;
// and png_bits_lz / png_pack_lz read the stored parse in place of the run scans; png_clear, png_scan, png_zero and png_crc
// are instantiated a second time for the mode's layout (tags png_clear_lz, png_scan_lz, png_zero_lz, png_crc_lz).
#include "pp_common.h"
#include "pp_png_code_core.h"
#include "pp_png_core.h"

#include <cstdint>

namespace pp {

using namespace png;

constexpr int PNG_STRIDE_WGS = 256;  // workgroups per stream of the grid-stride launches

__constant__ const CrcTables kCrcTables = crc_tables();

// What the launches both match modes share (png_clear, png_scan, png_zero, png_crc) take from the mode: which descriptors
// count, the scratch layout with its bound, and the histogram's size.
template <bool LZ>
__device__ __forceinline__ long long mode_len(const pp_deflate_desc& d) {
    return LZ ? def_len_lz(d) : def_len(d);
}

template <bool LZ>
__device__ __forceinline__ DefLayout mode_layout(long long len) {
    if constexpr (LZ) return def_layout_lz(len);
    else return def_layout(len);
}

// blockIdx.y: stream; blockIdx.x: row.
__global__ __launch_bounds__(256) void png_filter_kernel(const pp_deflate_desc* __restrict__ descs) {
    __shared__ uint32_t cost[5];
    const pp_deflate_desc d = descs[blockIdx.y];
    if (!d.pixels || def_len(d) == 0 || (int)blockIdx.x >= d.height) return;
    const int nb = 3 * d.width, rgb = d.rgb;
    const uint8_t* cur = d.pixels + (long long)blockIdx.x * d.row_stride;
    const uint8_t* up = blockIdx.x ? cur - d.row_stride : nullptr;
    if (threadIdx.x < 5) cost[threadIdx.x] = 0;
    __syncthreads();
    uint32_t sum[5] = {0, 0, 0, 0, 0}, f[5];
    for (int i = threadIdx.x; i < nb; i += 256) {
        filter_all(cur, up, i, rgb, f);
#pragma unroll
        for (int t = 0; t < 5; ++t) sum[t] += filter_cost(f[t]);
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        uint32_t v = sum[t];
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o);
        if (lane_id() == 0) atomicAdd(&cost[t], v);
    }
    __syncthreads();
    const int type = filter_choice(cost);
    const long long row0 = (long long)blockIdx.x * (1 + nb);
    if (threadIdx.x == 0 && row0 < d.len) d.data[row0] = (uint8_t)type;
    for (int i = threadIdx.x; i < nb; i += 256) {
        filter_all(cur, up, i, rgb, f);
        if (row0 + 1 + i < d.len) d.data[row0 + 1 + i] = (uint8_t)f[type];
    }
}

// blockIdx.x: stream.
template <bool LZ>
__global__ __launch_bounds__(256) void png_clear_kernel(const pp_deflate_desc* __restrict__ descs) {
    const pp_deflate_desc d = descs[blockIdx.x];
    if (mode_len<LZ>(d) == 0) return;
    for (int i = threadIdx.x; i < (LZ ? LZ_HIST_WORDS : 288); i += 256) d.hist[i] = 0;
}

// A thread's span of its tile and the ends of the runs that reach beyond it.
struct Span {
    uint32_t w[4];
    int cnt, p0, n, left_start, right_end;
};

struct SpanLds {
    int16_t last_head[256], first_tail[256];
    uint8_t first[256], last[256];
};

// The bytes of this thread's span of tile `tile` of d's stream (left_start and right_end stay unset).
__device__ __forceinline__ Span load_bytes(const pp_deflate_desc& d, long long tile) {
    Span sp;
    const long long left = d.len - tile * PNG_TILE;
    sp.n = left < PNG_TILE ? (int)left : PNG_TILE;
    sp.p0 = PNG_SPAN * (int)threadIdx.x;
    sp.cnt = sp.n - sp.p0 >= PNG_SPAN ? PNG_SPAN : (sp.n > sp.p0 ? sp.n - sp.p0 : 0);
    const uint8_t* src = d.data + tile * PNG_TILE + sp.p0;
    sp.w[0] = sp.w[1] = sp.w[2] = sp.w[3] = 0;
    if (sp.cnt == PNG_SPAN) {
        const uint4 v = *reinterpret_cast<const uint4*>(src);
        sp.w[0] = v.x, sp.w[1] = v.y, sp.w[2] = v.z, sp.w[3] = v.w;
    } else {
#pragma unroll
        for (int i = 0; i < PNG_SPAN; ++i)
            if (i < sp.cnt) sp.w[i >> 2] |= (uint32_t)src[i] << (8 * (i & 3));
    }
    return sp;
}

// The span of this thread in tile `tile` of d's stream. left_start: the last run start at or before the span's first byte,
// by a running maximum over the threads before it; right_end: the first run end at or behind its last byte, by a running
// minimum over the threads behind it.
__device__ __forceinline__ Span load_span(const pp_deflate_desc& d, long long tile, SpanLds& s) {
    Span sp = load_bytes(d, tile);
    const int t = threadIdx.x, cnt = sp.cnt;
    s.first[t] = (uint8_t)span_byte(sp.w, 0);
    s.last[t] = (uint8_t)span_byte(sp.w, cnt > 0 ? cnt - 1 : 0);
    __syncthreads();
    const bool head0 = cnt > 0 && (t == 0 || span_byte(sp.w, 0) != s.last[t - 1]);
    const bool tail_last = cnt > 0 && (sp.p0 + cnt == sp.n || span_byte(sp.w, cnt - 1) != s.first[t + 1]);  // (then t < 255: the span ends before the tile)
    int lh = head0 ? sp.p0 : -1, ft = 32767;
#pragma unroll
    for (int i = 1; i < PNG_SPAN; ++i)
        if (i < cnt && span_byte(sp.w, i) != span_byte(sp.w, i - 1)) lh = sp.p0 + i;
    if (tail_last) ft = sp.p0 + cnt - 1;
#pragma unroll
    for (int i = PNG_SPAN - 2; i >= 0; --i)
        if (i < cnt - 1 && span_byte(sp.w, i) != span_byte(sp.w, i + 1)) ft = sp.p0 + i;
    s.last_head[t] = (int16_t)lh;
    s.first_tail[t] = (int16_t)ft;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int a = t >= o ? (int)s.last_head[t - o] : -1, b = t + o < 256 ? (int)s.first_tail[t + o] : 32767;
        __syncthreads();
        if (a > (int)s.last_head[t]) s.last_head[t] = (int16_t)a;
        if (b < (int)s.first_tail[t]) s.first_tail[t] = (int16_t)b;
        __syncthreads();
    }
    sp.left_start = (head0 || t == 0) ? sp.p0 : (int)s.last_head[t - 1];
    sp.right_end = (tail_last || t == 255) ? sp.p0 + cnt - 1 : (int)s.first_tail[t + 1];
    __syncthreads();  // (s is free for the next call)
    return sp;
}

// blockIdx.y: stream; blockIdx.x: tile.
__global__ __launch_bounds__(256) void png_hist_kernel(const pp_deflate_desc* __restrict__ descs) {
    __shared__ SpanLds lds;
    __shared__ uint32_t hist[288];
    __shared__ uint32_t red[4];
    const pp_deflate_desc d = descs[blockIdx.y];
    if (def_len(d) == 0) return;
    const DefLayout L = def_layout(d.len);
    if ((long long)blockIdx.x >= L.ntiles) return;
    for (int i = threadIdx.x; i < 288; i += 256) hist[i] = 0;
    const Span sp = load_span(d, blockIdx.x, lds);
    uint32_t s1 = 0, s2 = 0;
    if (sp.cnt > 0) {
        HistSink h{hist};
        span_tokens(sp.w, sp.cnt, sp.p0, sp.left_start, sp.right_end, h);
        adler_span(sp.w, sp.cnt, sp.n - sp.p0, s1, s2);
    }
    uint32_t t1, t2;
    block_scan(s1, red, t1);
    block_scan(s2, red, t2);  // (at most 255 x 4096 x 4097 / 2 < 2^32)
    for (int i = threadIdx.x; i < DEFLATE_SYMS; i += 256)
        if (hist[i]) atomicAdd(d.hist + i, hist[i]);
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) atomicAdd(d.hist + 256, 1u);  // the end of the block
        reinterpret_cast<uint2*>(d.scratch + L.o_tadler)[blockIdx.x] = make_uint2(t1, t2);
    }
}

__device__ __forceinline__ void code_to_lds(const pp_deflate_desc& d, uint32_t* sym) {
    for (int i = threadIdx.x; i < 288; i += 256) sym[i] = d.code->sym[i];
    __syncthreads();
}

// blockIdx.y: stream; blockIdx.x: tile.
__global__ __launch_bounds__(256) void png_bits_kernel(const pp_deflate_desc* __restrict__ descs) {
    __shared__ SpanLds lds;
    __shared__ uint32_t sym[288];
    __shared__ uint32_t red[4];
    const pp_deflate_desc d = descs[blockIdx.y];
    if (def_len(d) == 0 || !d.code) return;
    const DefLayout L = def_layout(d.len);
    if ((long long)blockIdx.x >= L.ntiles) return;
    code_to_lds(d, sym);
    const Span sp = load_span(d, blockIdx.x, lds);
    LsbCounter c;
    if (sp.cnt > 0) {
        CodeSink<LsbCounter> sink{sym, c};
        span_tokens(sp.w, sp.cnt, sp.p0, sp.left_start, sp.right_end, sink);
    }
    uint32_t total;
    block_scan(c.bits, red, total);
    if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(d.scratch + L.o_tsum)[blockIdx.x] = total;
}

// blockIdx.x: stream.
template <bool LZ>
__global__ __launch_bounds__(256) void png_scan_kernel(const pp_deflate_desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const pp_deflate_desc d = descs[blockIdx.x];
    if (mode_len<LZ>(d) == 0 || !d.code) {
        if (threadIdx.x == 0 && d.result) {
            d.result->bytes = 0;
            d.result->status = PP_ERR_INVALID_ARG;
            d.result->crc = 0;
        }
        return;
    }
    const DefLayout L = mode_layout<LZ>(d.len);
    const unsigned long long token_bits = scan_u32_to_u64(reinterpret_cast<const uint32_t*>(d.scratch + L.o_tsum), 1, L.ntiles,
                                                          reinterpret_cast<unsigned long long*>(d.scratch + L.o_toff), red);
    const uint2* tadler = reinterpret_cast<const uint2*>(d.scratch + L.o_tadler);
    uint32_t lo = 1u, hi = (uint32_t)((unsigned long long)d.len % ADLER_MOD);
    for (long long base = 0; base < L.ntiles; base += 256) {
        const long long t = base + threadIdx.x;
        uint32_t a = 0, b = 0;
        if (t < L.ntiles) {
            const uint2 v = tadler[t];
            const long long behind = d.len - (t + 1) * PNG_TILE;
            a = v.x % ADLER_MOD;
            b = adler_term(v.x, v.y, behind > 0 ? (unsigned long long)behind : 0ull);
        }
        uint32_t ta, tb;
        block_scan(a, red, ta);
        block_scan(b, red, tb);
        lo = (lo + ta) % ADLER_MOD;
        hi = (hi + tb) % ADLER_MOD;
    }
    if (threadIdx.x == 0) {
        const uint32_t eob = d.code->sym[256] >> 16;
        const unsigned long long bits = d.code->header_bits + token_bits + eob;
        const unsigned long long nbytes = ((bits + 7) >> 3) + 4;
        const bool ok = (long long)nbytes <= d.capacity && (long long)nbytes <= L.max_bytes;
        DefHeader* h = reinterpret_cast<DefHeader*>(d.scratch);
        h->total_bits = bits;
        h->nbytes = nbytes;
        h->adler = (hi << 16) | lo;
        h->ok = ok ? 1u : 0u;
        d.result->bytes = (long long)nbytes;
        d.result->status = ok ? PP_OK : PP_ERR_WORKSPACE;
        d.result->crc = ok ? crc_mul(crc_shift(kCrcTables.x2n, nbytes), d.crc_init) : 0u;
    }
}

// blockIdx.y: stream; the workgroups of a row stride over the words in use, sixteen bytes a thread.
template <bool LZ>
__global__ __launch_bounds__(256) void png_zero_kernel(const pp_deflate_desc* __restrict__ descs) {
    const pp_deflate_desc d = descs[blockIdx.y];
    if (mode_len<LZ>(d) == 0 || !d.code) return;
    const DefLayout L = mode_layout<LZ>(d.len);
    const DefHeader* h = reinterpret_cast<const DefHeader*>(d.scratch);
    if (!h->ok) return;
    long long quads = (long long)((h->nbytes + 15) >> 4);
    if (quads > L.nwords / 4) quads = L.nwords / 4;
    uint4* q = reinterpret_cast<uint4*>(d.scratch + L.o_words);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long long)gridDim.x * 256) q[i] = make_uint4(0u, 0u, 0u, 0u);
}

// blockIdx.y: stream; blockIdx.x: tile.
__global__ __launch_bounds__(256) void png_pack_kernel(const pp_deflate_desc* __restrict__ descs) {
    __shared__ SpanLds lds;
    __shared__ uint32_t sym[288];
    __shared__ uint32_t red[4];
    const pp_deflate_desc d = descs[blockIdx.y];
    if (def_len(d) == 0 || !d.code) return;
    const DefLayout L = def_layout(d.len);
    if ((long long)blockIdx.x >= L.ntiles) return;
    const DefHeader* h = reinterpret_cast<const DefHeader*>(d.scratch);
    if (!h->ok) return;
    code_to_lds(d, sym);
    const Span sp = load_span(d, blockIdx.x, lds);
    LsbCounter c;
    if (sp.cnt > 0) {
        CodeSink<LsbCounter> sink{sym, c};
        span_tokens(sp.w, sp.cnt, sp.p0, sp.left_start, sp.right_end, sink);
    }
    uint32_t total;
    const uint32_t before = block_scan(c.bits, red, total);
    uint32_t* words = reinterpret_cast<uint32_t*>(d.scratch + L.o_words);
    const uint32_t header_bits = d.code->header_bits;
    if (blockIdx.x == 0 && threadIdx.x < (header_bits + 31) / 32 && threadIdx.x < 76 && (long long)threadIdx.x < L.nwords)
        atomicOr(words + threadIdx.x, d.code->header[threadIdx.x]);
    if (sp.cnt == 0) return;
    const unsigned long long start = header_bits + reinterpret_cast<const unsigned long long*>(d.scratch + L.o_toff)[blockIdx.x] + before;
    LsbPacker p(words, start, L.nwords);
    CodeSink<LsbPacker> sink{sym, p};
    span_tokens(sp.w, sp.cnt, sp.p0, sp.left_start, sp.right_end, sink);
    if ((long long)blockIdx.x * PNG_TILE + sp.p0 + sp.cnt == d.len) put_tail(p, sym, h->adler);
    p.finish();
}

// blockIdx.y: stream; the workgroups of a row stride over the chunks of CRC_CHUNK bytes in use.
template <bool LZ>
__global__ __launch_bounds__(256) void png_crc_kernel(const pp_deflate_desc* __restrict__ descs) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t part[4];
    const pp_deflate_desc d = descs[blockIdx.y];
    if (mode_len<LZ>(d) == 0 || !d.code) return;
    const DefLayout L = mode_layout<LZ>(d.len);
    const DefHeader* h = reinterpret_cast<const DefHeader*>(d.scratch);
    if (!h->ok) return;
    const long long nbytes = (long long)h->nbytes;  // (ok: at most the capacity and the words' size)
    tab[threadIdx.x] = kCrcTables.byte[threadIdx.x];
    __syncthreads();
    const long long chunks = (nbytes + CRC_CHUNK - 1) / CRC_CHUNK;
    const uint4* quads = reinterpret_cast<const uint4*>(d.scratch + L.o_words);
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long byte0 = c * CRC_CHUNK + 16 * (long long)threadIdx.x;
        const long long left = nbytes - byte0;
        const int valid = left >= 16 ? 16 : (left > 0 ? (int)left : 0);
        const long long chunk_end = (c + 1) * CRC_CHUNK < nbytes ? (c + 1) * CRC_CHUNK : nbytes;
        uint32_t r = 0;
        if (valid > 0) {
            const uint4 v = quads[byte0 >> 4];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < valid) r = crc_byte(tab, r, span_byte(w, k));
            if (valid == 16) {
                if (byte0 + 16 <= d.capacity) *reinterpret_cast<uint4*>(d.out + byte0) = v;
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k < valid && byte0 + k < d.capacity) d.out[byte0 + k] = (uint8_t)span_byte(w, k);
            }
            r = crc_mul(crc_shift(kCrcTables.x2n, (unsigned long long)(chunk_end - byte0 - valid)), r);
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) r ^= __shfl_xor(r, o);
        if (lane_id() == 0) part[wave_id()] = r;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t all = part[0] ^ part[1] ^ part[2] ^ part[3];
            atomicXor(&d.result->crc, crc_mul(crc_shift(kCrcTables.x2n, (unsigned long long)(nbytes - chunk_end)), all));
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------- lz mode
struct LzLds {
    int16_t jump[PNG_TILE + 16];  // the chain: position -> the position 2^round tokens on, PNG_TILE for "past the tile" (read sixteen bytes at a time)
    uint8_t mark[PNG_TILE + 16];  // 1: a token starts here (likewise)
    int16_t fu[LZ_CANDS][4];      // per candidate and wave: the first position in the wave's spans whose byte differs from its source
};

// Bit i: byte g0 + i of the stream (i < cnt, held in w) equals the byte `dist` before it; clear where g0 + i < dist.
__device__ __forceinline__ uint32_t lz_eq_mask(const uint8_t* __restrict__ data, long long g0, int dist, const uint32_t (&w)[4], int cnt) {
    if (dist == 0 || cnt == 0) return 0u;
    const long long o = g0 - dist;
    uint32_t h[4] = {0u, 0u, 0u, 0u}, valid = 0u;
    if (dist >= 4 && cnt == PNG_SPAN && o >= 0) {
        // five aligned words around the sixteen source bytes, none past the span's own last byte (dist >= 4), shifted into place
        const uint32_t* a = reinterpret_cast<const uint32_t*>(data + (o & ~3ll));
        const int sh = 8 * (int)(o & 3);
        const uint32_t v[5] = {a[0], a[1], a[2], a[3], sh ? a[4] : 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) h[k] = (uint32_t)((((uint64_t)v[k + 1] << 32) | v[k]) >> sh);
        valid = 0xFFFFu;
    } else {
#pragma unroll
        for (int i = 0; i < PNG_SPAN; ++i) {
            if (i < cnt && g0 + i >= dist) {
                const uint32_t b = i >= dist ? span_byte(w, i - dist) : (uint32_t)data[o + i];
                h[i >> 2] |= b << (8 * (i & 3));
                valid |= 1u << i;
            }
        }
    }
    uint32_t eq = 0u;
#pragma unroll
    for (int i = 0; i < PNG_SPAN; ++i) eq |= (uint32_t)(span_byte(w, i) == span_byte(h, i)) << i;
    return eq & valid;
}

__device__ __forceinline__ uint32_t parse_entry(const uint32_t (&pv)[8], int i) { return (pv[i >> 1] >> (16 * (i & 1))) & 0xFFFFu; }

// blockIdx.y: stream; blockIdx.x: tile. The candidates' equality masks, their first differences by a running minimum over
// the threads behind (load_span's scan, five at once and by wave shuffles), every position's token, then the token starts: the chain
// next(p) = p + step(p) from position 0, by twelve rounds of pointer doubling (a round: every reached q marks jump[q], then
// jump[q] <- jump[jump[q]]; reads, barrier, writes, barrier). A mark is the store of a 1: the set is the same every launch.
__global__ __launch_bounds__(256) void png_parse_lz_kernel(const pp_deflate_desc* __restrict__ descs) {
    __shared__ __attribute__((aligned(16))) LzLds lds;
    __shared__ uint32_t hist[LZ_HIST_WORDS];
    __shared__ uint32_t red[4];
    const pp_deflate_desc d = descs[blockIdx.y];
    if (def_len_lz(d) == 0) return;
    const LzLayout L = def_layout_lz(d.len);
    if ((long long)blockIdx.x >= L.ntiles) return;
    const int t = threadIdx.x;
    for (int i = t; i < LZ_HIST_WORDS; i += 256) hist[i] = 0;
    const Span sp = load_bytes(d, blockIdx.x);
    const int cnt = sp.cnt, p0 = sp.p0, n = sp.n;
    const long long g0 = (long long)blockIdx.x * PNG_TILE + p0;
    const LzDist D = lz_dists(lz_period(d));
    LzSpan ls;
    int fu[LZ_CANDS];  // the first position at or behind this span's first byte whose byte differs from its source
#pragma unroll
    for (int c = 0; c < LZ_CANDS; ++c) {
        ls.eq[c] = lz_eq_mask(d.data, g0, D.d[c], sp.w, cnt);
        const int f = __builtin_ctz(~ls.eq[c]);  // (bits at and above cnt are clear: f <= cnt)
        fu[c] = f < cnt ? p0 + f : (cnt == PNG_SPAN ? 32767 : n);
    }
    // the running minimum over the threads behind: inside the wave by shuffles, across the four waves through LDS
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
#pragma unroll
        for (int c = 0; c < LZ_CANDS; ++c) {
            const int b = __shfl_down(fu[c], o);
            if (lane_id() + o < WAVE && b < fu[c]) fu[c] = b;
        }
    }
#pragma unroll
    for (int c = 0; c < LZ_CANDS; ++c) {
        ls.nu_next[c] = __shfl_down(fu[c], 1);  // (the last lane's comes from the waves behind)
        if (lane_id() == 0) lds.fu[c][wave_id()] = (int16_t)fu[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < LZ_CANDS; ++c) {
        int v = lane_id() < WAVE - 1 ? ls.nu_next[c] : 32767;
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (w > wave_id() && (int)lds.fu[c][w] < v) v = (int)lds.fu[c][w];
        ls.nu_next[c] = v < n ? v : n;
    }
    uint16_t tok[PNG_SPAN];
    lz_span_tokens(ls, cnt, p0, n, tok);
    // the chain
    int j[PNG_SPAN];
    uint32_t jw[8], mk[4] = {t == 0 ? 1u : 0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < PNG_SPAN; ++i) j[i] = i < cnt ? p0 + i + lz_step(tok[i]) : PNG_TILE;  // (at most n)
#pragma unroll
    for (int i = 0; i < PNG_SPAN; ++i)
        if (j[i] >= n) j[i] = PNG_TILE;
#pragma unroll
    for (int k = 0; k < 8; ++k) jw[k] = (uint32_t)j[2 * k] | ((uint32_t)j[2 * k + 1] << 16);
    uint4* my_jump = reinterpret_cast<uint4*>(lds.jump + p0);
    uint4* my_mark = reinterpret_cast<uint4*>(lds.mark + p0);
    my_jump[0] = make_uint4(jw[0], jw[1], jw[2], jw[3]);
    my_jump[1] = make_uint4(jw[4], jw[5], jw[6], jw[7]);
    *my_mark = make_uint4(mk[0], mk[1], mk[2], mk[3]);
    if (t < 16) {
        lds.jump[PNG_TILE + t] = (int16_t)PNG_TILE;  // the fixed point
        lds.mark[PNG_TILE + t] = 0;
    }
    __syncthreads();
#pragma unroll 1
    for (int round = 0; round < 12; ++round) {
        const uint4 m4 = *my_mark;
        mk[0] = m4.x, mk[1] = m4.y, mk[2] = m4.z, mk[3] = m4.w;
        int j2[PNG_SPAN];
#pragma unroll
        for (int i = 0; i < PNG_SPAN; ++i) j2[i] = (int)lds.jump[j[i]];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PNG_SPAN; ++i) {
            if (span_byte(mk, i)) lds.mark[j[i]] = 1;
            j[i] = j2[i];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) jw[k] = (uint32_t)j[2 * k] | ((uint32_t)j[2 * k + 1] << 16);
        my_jump[0] = make_uint4(jw[0], jw[1], jw[2], jw[3]);
        my_jump[1] = make_uint4(jw[4], jw[5], jw[6], jw[7]);
        __syncthreads();
    }
    const uint4 m4 = *my_mark;
    mk[0] = m4.x, mk[1] = m4.y, mk[2] = m4.z, mk[3] = m4.w;
    uint32_t pv[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, s1 = 0, s2 = 0;
    if (cnt > 0) {
        LzHistSink h{hist};
#pragma unroll
        for (int i = 0; i < PNG_SPAN; ++i) {
            const uint32_t v = (i < cnt && span_byte(mk, i)) ? (uint32_t)tok[i] : 0u;
            pv[i >> 1] |= v << (16 * (i & 1));
            lz_emit(v, span_byte(sp.w, i), D, h);
        }
        adler_span(sp.w, cnt, n - p0, s1, s2);
        const long long at = (long long)blockIdx.x * PNG_TILE + p0;
        if (at + PNG_SPAN <= L.parse_entries) {
            uint4* q = reinterpret_cast<uint4*>(d.scratch + L.o_parse) + at / 8;
            q[0] = make_uint4(pv[0], pv[1], pv[2], pv[3]);
            q[1] = make_uint4(pv[4], pv[5], pv[6], pv[7]);
        }
    }
    uint32_t t1, t2;
    block_scan(s1, red, t1);
    block_scan(s2, red, t2);
    for (int i = t; i < LZ_DIST_AT + LZ_DIST_SYMS; i += 256)
        if (hist[i]) atomicAdd(d.hist + i, hist[i]);
    if (t == 0) {
        if (blockIdx.x == 0) atomicAdd(d.hist + 256, 1u);  // the end of the block
        reinterpret_cast<uint2*>(d.scratch + L.o_tadler)[blockIdx.x] = make_uint2(t1, t2);
    }
}

// What png_bits_lz and png_pack_lz read: the span's bytes, its share of the stored parse, both codes in LDS.
struct LzCoded {
    Span sp;
    uint32_t pv[8];
};

__device__ __forceinline__ LzCoded load_coded(const pp_deflate_desc& d, const LzLayout& L, long long tile, uint32_t* sym) {
    const pp_deflate_code_lz* code = reinterpret_cast<const pp_deflate_code_lz*>(d.code);
    for (int i = threadIdx.x; i < LZ_HIST_WORDS; i += 256) sym[i] = i < LZ_DIST_AT ? code->base.sym[i] : code->dist[i - LZ_DIST_AT];
    __syncthreads();
    LzCoded c;
    c.sp = load_bytes(d, tile);
#pragma unroll
    for (int k = 0; k < 8; ++k) c.pv[k] = 0u;
    const long long at = tile * PNG_TILE + c.sp.p0;
    if (c.sp.cnt > 0 && at + PNG_SPAN <= L.parse_entries) {
        const uint4* q = reinterpret_cast<const uint4*>(d.scratch + L.o_parse) + at / 8;
        const uint4 a = q[0], b = q[1];
        c.pv[0] = a.x, c.pv[1] = a.y, c.pv[2] = a.z, c.pv[3] = a.w, c.pv[4] = b.x, c.pv[5] = b.y, c.pv[6] = b.z, c.pv[7] = b.w;
    }
    return c;
}

template <class Put>
__device__ __forceinline__ void code_span(const LzCoded& c, const LzDist& D, const uint32_t* sym, Put& out) {
    LzCodeSink<Put> sink{sym, sym + LZ_DIST_AT, out};
#pragma unroll
    for (int i = 0; i < PNG_SPAN; ++i)
        if (i < c.sp.cnt) lz_emit(parse_entry(c.pv, i), span_byte(c.sp.w, i), D, sink);
}

// blockIdx.y: stream; blockIdx.x: tile.
__global__ __launch_bounds__(256) void png_bits_lz_kernel(const pp_deflate_desc* __restrict__ descs) {
    __shared__ uint32_t sym[LZ_HIST_WORDS];
    __shared__ uint32_t red[4];
    const pp_deflate_desc d = descs[blockIdx.y];
    if (def_len_lz(d) == 0 || !d.code) return;
    const LzLayout L = def_layout_lz(d.len);
    if ((long long)blockIdx.x >= L.ntiles) return;
    const LzCoded c = load_coded(d, L, blockIdx.x, sym);
    LsbCounter count;
    code_span(c, lz_dists(lz_period(d)), sym, count);
    uint32_t total;
    block_scan(count.bits, red, total);
    if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(d.scratch + L.o_tsum)[blockIdx.x] = total;
}

// blockIdx.y: stream; blockIdx.x: tile.
__global__ __launch_bounds__(256) void png_pack_lz_kernel(const pp_deflate_desc* __restrict__ descs) {
    __shared__ uint32_t sym[LZ_HIST_WORDS];
    __shared__ uint32_t red[4];
    const pp_deflate_desc d = descs[blockIdx.y];
    if (def_len_lz(d) == 0 || !d.code) return;
    const LzLayout L = def_layout_lz(d.len);
    if ((long long)blockIdx.x >= L.ntiles) return;
    const DefHeader* h = reinterpret_cast<const DefHeader*>(d.scratch);
    if (!h->ok) return;
    const LzCoded c = load_coded(d, L, blockIdx.x, sym);
    const LzDist D = lz_dists(lz_period(d));
    LsbCounter count;
    code_span(c, D, sym, count);
    uint32_t total;
    const uint32_t before = block_scan(count.bits, red, total);
    uint32_t* words = reinterpret_cast<uint32_t*>(d.scratch + L.o_words);
    const uint32_t header_bits = d.code->header_bits;
    if (blockIdx.x == 0 && threadIdx.x < (header_bits + 31) / 32 && threadIdx.x < 76 && (long long)threadIdx.x < L.nwords)
        atomicOr(words + threadIdx.x, d.code->header[threadIdx.x]);
    if (c.sp.cnt == 0) return;
    const unsigned long long start = header_bits + reinterpret_cast<const unsigned long long*>(d.scratch + L.o_toff)[blockIdx.x] + before;
    LsbPacker p(words, start, L.nwords);
    code_span(c, D, sym, p);
    if ((long long)blockIdx.x * PNG_TILE + c.sp.p0 + c.sp.cnt == d.len) put_tail(p, sym, h->adler);
    p.finish();
}

// The executor of the code build's steps (csrc/pp_png_code_core.h) for a workgroup of 256 threads. red: four words.
struct WgExec {
    uint32_t* red;
    template <class F>
    __device__ __forceinline__ void each(int n, F f) {
        for (int i = threadIdx.x; i < n; i += 256) f(i);
        __syncthreads();
    }
    template <class F>
    __device__ __forceinline__ void one(F f) {
        if (threadIdx.x == 0) f();
        __syncthreads();
    }
    template <class B, class P>
    __device__ __forceinline__ uint32_t offsets(int n, B bits, P put) {  // two items a thread: n <= 512
        const int i = 2 * (int)threadIdx.x;
        const uint32_t b0 = i < n ? bits(i) : 0u, b1 = i + 1 < n ? bits(i + 1) : 0u;
        uint32_t total;
        const uint32_t before = block_scan(b0 + b1, red, total);
        if (i < n) put(i, before);
        if (i + 1 < n) put(i + 1, before + b0);
        __syncthreads();
        return total;
    }
};

static_assert(DEFLATE_SYMS + LZ_DIST_SYMS <= 512, "WgExec::offsets takes two items a thread");

// blockIdx.x: stream. Reads hist, writes the whole *code (LZ: the pp_deflate_code_lz whose base it names).
template <bool LZ>
__global__ __launch_bounds__(256) void png_code_kernel(const pp_deflate_desc* __restrict__ descs) {
    __shared__ CodeWork work;
    __shared__ uint32_t red[4];
    const pp_deflate_desc d = descs[blockIdx.x];
    if (mode_len<LZ>(d) == 0 || !d.code) return;
    WgExec ex{red};
    code_steps<LZ>(ex, work, d.hist);
    uint32_t* dst = reinterpret_cast<uint32_t*>(const_cast<pp_deflate_code*>(d.code));
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&work.out);
    for (int i = threadIdx.x; i < (LZ ? CODE_WORDS_LZ : CODE_WORDS); i += 256) dst[i] = src[i];
}

static bool batch_args_ok(const char* fn, const void* descriptors, int n, long long max_len) {
    if (n < 0 || (n > 0 && !descriptors) || n > 65535 || (n > 0 && (max_len < 1 || max_len > 0x7FFFFFFFll))) {
        set_error("%s: at most 65535 descriptors of streams of 1 .. 2^31 - 1 bytes", fn);
        return false;
    }
    return true;
}

}  // namespace pp

extern "C" long long pp_deflate_bound(long long len) {
    if (len < 1 || len > 0x7FFFFFFFll || pp::png::deflate_bound(len) > 0x7FFFFFFFll) {
        pp::set_error("pp_deflate_bound: a stream of 1 .. 2^31 - 1 bytes whose bound stays below 2^31");
        return PP_ERR_INVALID_ARG;
    }
    return pp::png::deflate_bound(len);
}

extern "C" long long pp_png_encoded_bound(int width, int height) {
    if (width < 1 || height < 1 || width > 65535 || height > 65535) {
        pp::set_error("pp_png_encoded_bound: a PNG file holds 1..65535 pixels a side");
        return PP_ERR_INVALID_ARG;
    }
    const long long bound = pp_deflate_bound((long long)height * (1 + 3ll * width));
    return bound < 0 ? bound : bound + (long long)(pp::png::PNG_HEAD + pp::png::PNG_TAIL);
}

extern "C" long long pp_deflate_scratch_bytes(long long len) {
    if (pp_deflate_bound(len) < 0) return PP_ERR_INVALID_ARG;
    return pp::png::def_layout(len).total;
}

extern "C" int pp_deflate_build_code(const uint32_t* hist_host, pp_deflate_code* code_host) {
    if (!hist_host || !code_host) {
        pp::set_error("pp_deflate_build_code: NULL argument");
        return PP_ERR_INVALID_ARG;
    }
    pp::png::build_code(hist_host, code_host);
    return PP_OK;
}

extern "C" int pp_deflate_build_code_steps(const uint32_t* hist_host, pp_deflate_code* code_host) {
    if (!hist_host || !code_host) {
        pp::set_error("pp_deflate_build_code_steps: NULL argument");
        return PP_ERR_INVALID_ARG;
    }
    pp::png::build_code_steps(hist_host, code_host);
    return PP_OK;
}

extern "C" int pp_zlib_compress(const void* data_host, long long len, void* out_host, size_t capacity, size_t* size_out, long long* tokens_out) {
    if (!data_host || !out_host || !size_out || pp_deflate_bound(len) < 0) {
        pp::set_error("pp_zlib_compress: NULL argument, or a stream outside 1 .. 2^31 - 1 bytes");
        return PP_ERR_INVALID_ARG;
    }
    const int st = pp::png::zlib_compress(static_cast<const uint8_t*>(data_host), len, static_cast<uint8_t*>(out_host), capacity, size_out, tokens_out);
    if (st != PP_OK) pp::set_error("pp_zlib_compress: the stream needs %zu bytes, %zu were given", *size_out, capacity);
    return st;
}

extern "C" int pp_png_encode(const uint8_t* pixels_host, int width, int height, long long row_stride, int rgb, void* out_host, size_t capacity,
                             size_t* size_out) {
    if (!pixels_host || !out_host || !size_out || pp_png_encoded_bound(width, height) < 0 || row_stride < 3ll * width) {
        pp::set_error("pp_png_encode: NULL argument, a side outside 1..65535, a row stride below 3 x width or a picture too large for one stream");
        return PP_ERR_INVALID_ARG;
    }
    const int st = pp::png::encode_file(pixels_host, width, height, row_stride, rgb ? 1 : 0, static_cast<uint8_t*>(out_host), capacity, size_out);
    if (st != PP_OK) pp::set_error("pp_png_encode: the file needs %zu bytes, %zu were given", *size_out, capacity);
    return st;
}

extern "C" int pp_png_tokens_batch(const pp_deflate_desc* descriptors, int n, int max_height, long long max_len, void* stream) {
    using namespace pp;
    if (!batch_args_ok("pp_png_tokens_batch", descriptors, n, max_len) || max_height < 0 || max_height > 65535) {
        if (max_height < 0 || max_height > 65535) set_error("pp_png_tokens_batch: max_height outside 0..65535");
        return PP_ERR_INVALID_ARG;
    }
    if (n == 0) return PP_OK;
    (void)hipGetLastError();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 tpb(256), per_tile((unsigned)def_layout(max_len).ntiles, n);
    if (max_height > 0) {
        hipLaunchKernelGGL(png_filter_kernel, dim3(max_height, n), tpb, 0, s, descriptors);
        PP_LAUNCH_CHECK_AS("png_filter");
    }
    hipLaunchKernelGGL(png_clear_kernel<false>, dim3(n), tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_clear");
    hipLaunchKernelGGL(png_hist_kernel, per_tile, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_hist");
    return PP_OK;
}

extern "C" int pp_png_deflate_batch(const pp_deflate_desc* descriptors, int n, long long max_len, void* stream) {
    using namespace pp;
    if (!batch_args_ok("pp_png_deflate_batch", descriptors, n, max_len)) return PP_ERR_INVALID_ARG;
    if (n == 0) return PP_OK;
    (void)hipGetLastError();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const DefLayout L = def_layout(max_len);
    const dim3 tpb(256), per_tile((unsigned)L.ntiles, n), per_stream(n);
    const long long quads = (L.nwords / 4 + 255) / 256, chunks = (L.max_bytes + CRC_CHUNK - 1) / CRC_CHUNK;
    const dim3 zero_grid((unsigned)(quads < PNG_STRIDE_WGS ? quads : PNG_STRIDE_WGS), n);
    const dim3 crc_grid((unsigned)(chunks < PNG_STRIDE_WGS ? chunks : PNG_STRIDE_WGS), n);
    hipLaunchKernelGGL(png_bits_kernel, per_tile, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_bits");
    hipLaunchKernelGGL(png_scan_kernel<false>, per_stream, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_scan");
    hipLaunchKernelGGL(png_zero_kernel<false>, zero_grid, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_zero");
    hipLaunchKernelGGL(png_pack_kernel, per_tile, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_pack");
    hipLaunchKernelGGL(png_crc_kernel<false>, crc_grid, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_crc");
    return PP_OK;
}

extern "C" int pp_png_code_batch(const pp_deflate_desc* descriptors, int n, void* stream) {
    using namespace pp;
    if (!batch_args_ok("pp_png_code_batch", descriptors, n, 1)) return PP_ERR_INVALID_ARG;
    if (n == 0) return PP_OK;
    (void)hipGetLastError();
    hipLaunchKernelGGL(png_code_kernel<false>, dim3(n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), descriptors);
    PP_LAUNCH_CHECK_AS("png_code");
    return PP_OK;
}

// ------------------------------------------------------------------------------------------------------------- lz mode
extern "C" long long pp_deflate_bound_lz(long long len) {
    if (len < 1 || len > 0x7FFFFFFFll || pp::png::deflate_bound_lz(len) > 0x7FFFFFFFll) {
        pp::set_error("pp_deflate_bound_lz: a stream of 1 .. 2^31 - 1 bytes whose bound stays below 2^31");
        return PP_ERR_INVALID_ARG;
    }
    return pp::png::deflate_bound_lz(len);
}

extern "C" long long pp_deflate_scratch_bytes_lz(long long len) {
    if (pp_deflate_bound_lz(len) < 0) return PP_ERR_INVALID_ARG;
    return pp::png::def_layout_lz(len).total;
}

extern "C" int pp_deflate_build_code_lz(const uint32_t* hist_host, pp_deflate_code_lz* code_host) {
    if (!hist_host || !code_host) {
        pp::set_error("pp_deflate_build_code_lz: NULL argument");
        return PP_ERR_INVALID_ARG;
    }
    pp::png::build_code_lz(hist_host, code_host);
    return PP_OK;
}

extern "C" int pp_deflate_build_code_steps_lz(const uint32_t* hist_host, pp_deflate_code_lz* code_host) {
    if (!hist_host || !code_host) {
        pp::set_error("pp_deflate_build_code_steps_lz: NULL argument");
        return PP_ERR_INVALID_ARG;
    }
    pp::png::build_code_steps_lz(hist_host, code_host);
    return PP_OK;
}

extern "C" int pp_zlib_compress_lz(const void* data_host, long long len, long long period, void* out_host, size_t capacity, size_t* size_out,
                                   long long* tokens_out) {
    if (!data_host || !out_host || !size_out || period < 0 || pp_deflate_bound_lz(len) < 0) {
        pp::set_error("pp_zlib_compress_lz: NULL argument, a negative period, or a stream outside 1 .. 2^31 - 1 bytes");
        return PP_ERR_INVALID_ARG;
    }
    const int st = pp::png::zlib_compress_lz(static_cast<const uint8_t*>(data_host), len, period, static_cast<uint8_t*>(out_host), capacity, size_out, tokens_out);
    if (st != PP_OK) pp::set_error("pp_zlib_compress_lz: the stream needs %zu bytes, %zu were given", *size_out, capacity);
    return st;
}

extern "C" int pp_png_encode_lz(const uint8_t* pixels_host, int width, int height, long long row_stride, int rgb, void* out_host, size_t capacity,
                                size_t* size_out) {
    if (!pixels_host || !out_host || !size_out || pp_png_encoded_bound(width, height) < 0 || row_stride < 3ll * width ||
        pp_deflate_bound_lz((long long)height * (1 + 3ll * width)) < 0) {
        pp::set_error("pp_png_encode_lz: NULL argument, a side outside 1..65535, a row stride below 3 x width or a picture too large for one stream");
        return PP_ERR_INVALID_ARG;
    }
    const int st = pp::png::encode_file(pixels_host, width, height, row_stride, rgb ? 1 : 0, static_cast<uint8_t*>(out_host), capacity, size_out, true);
    if (st != PP_OK) pp::set_error("pp_png_encode_lz: the file needs %zu bytes, %zu were given", *size_out, capacity);
    return st;
}

extern "C" int pp_png_tokens_batch_lz(const pp_deflate_desc* descriptors, int n, int max_height, long long max_len, void* stream) {
    using namespace pp;
    if (!batch_args_ok("pp_png_tokens_batch_lz", descriptors, n, max_len) || max_height < 0 || max_height > 65535) {
        if (max_height < 0 || max_height > 65535) set_error("pp_png_tokens_batch_lz: max_height outside 0..65535");
        return PP_ERR_INVALID_ARG;
    }
    if (n == 0) return PP_OK;
    (void)hipGetLastError();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 tpb(256), per_tile((unsigned)def_layout_lz(max_len).ntiles, n);
    if (max_height > 0) {
        hipLaunchKernelGGL(png_filter_kernel, dim3(max_height, n), tpb, 0, s, descriptors);
        PP_LAUNCH_CHECK_AS("png_filter");
    }
    hipLaunchKernelGGL(png_clear_kernel<true>, dim3(n), tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_clear_lz");
    hipLaunchKernelGGL(png_parse_lz_kernel, per_tile, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_parse_lz");
    return PP_OK;
}

extern "C" int pp_png_deflate_batch_lz(const pp_deflate_desc* descriptors, int n, long long max_len, void* stream) {
    using namespace pp;
    if (!batch_args_ok("pp_png_deflate_batch_lz", descriptors, n, max_len)) return PP_ERR_INVALID_ARG;
    if (n == 0) return PP_OK;
    (void)hipGetLastError();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const LzLayout L = def_layout_lz(max_len);
    const dim3 tpb(256), per_tile((unsigned)L.ntiles, n), per_stream(n);
    const long long quads = (L.nwords / 4 + 255) / 256, chunks = (L.max_bytes + CRC_CHUNK - 1) / CRC_CHUNK;
    const dim3 zero_grid((unsigned)(quads < PNG_STRIDE_WGS ? quads : PNG_STRIDE_WGS), n);
    const dim3 crc_grid((unsigned)(chunks < PNG_STRIDE_WGS ? chunks : PNG_STRIDE_WGS), n);
    hipLaunchKernelGGL(png_bits_lz_kernel, per_tile, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_bits_lz");
    hipLaunchKernelGGL(png_scan_kernel<true>, per_stream, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_scan_lz");
    hipLaunchKernelGGL(png_zero_kernel<true>, zero_grid, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_zero_lz");
    hipLaunchKernelGGL(png_pack_lz_kernel, per_tile, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_pack_lz");
    hipLaunchKernelGGL(png_crc_kernel<true>, crc_grid, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("png_crc_lz");
    return PP_OK;
}

extern "C" int pp_png_code_batch_lz(const pp_deflate_desc* descriptors, int n, void* stream) {
    using namespace pp;
    if (!batch_args_ok("pp_png_code_batch_lz", descriptors, n, 1)) return PP_ERR_INVALID_ARG;
    if (n == 0) return PP_OK;
    (void)hipGetLastError();
    hipLaunchKernelGGL(png_code_kernel<true>, dim3(n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), descriptors);
    PP_LAUNCH_CHECK_AS("png_code_lz");
    return PP_OK;
}
