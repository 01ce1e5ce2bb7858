// The seven phases of the device Huffman coder (see csrc/pp_jpeg_entropy.hip for what each does) as kernel templates over
// a table source, so that the coder with annex K's tables (pp_jpeg_entropy.hip) and the one with an image's own optimal tables
// (pp_jpeg_entropy_opt.hip) are one body. A source gives:
//   Desc                      the element of the descriptor table the launches read;
//   ent(desc)                 its pp_jpeg_ent_desc;
//   blocks(desc)              the blocks of the scan, 0 for an image to refuse (jpeg_ent_ffscan then reports PP_ERR_INVALID_ARG);
//   tables_to_lds(desc, lds)  code | size << 16 of every symbol into 536 words: AC luma (256), AC chroma (256), DC luma (12),
//                             DC chroma (12), and the barrier behind it.
// RST, the second template argument: the image's restart interval (pp_jpeg_ent_desc.restart_interval) is honoured - the
// *_restart_batch calls. The phases then run in ent_rst_layout, the DC prediction restarts with every interval
// (load_block), jpeg_ent_scan lays the intervals out behind its chunk scan (ilen[], ioff[]), jpeg_ent_pack places every
// block inside its byte-aligned interval and pads every interval's last byte, jpeg_ent_ffscan counts the markers into the
// need and jpeg_ent_stuff writes them (ent_stuff_restart). Without RST every body is what it was before the argument existed.
#pragma once
#include "pp_common.h"
#include "pp_jpeg_entropy_core.h"

namespace pp {

constexpr int ENT_STRIDE_WGS = 256;   // workgroups per image of the grid-stride launches

// The blocks a phase sees: the source's, and none for an interval outside 0..65535 where intervals are honoured.
template <class Src, bool RST>
__device__ __forceinline__ long long phase_blocks(const typename Src::Desc& src) {
    if constexpr (RST) {
        if (!ent_interval_ok(Src::ent(src))) return 0;
    }
    return Src::blocks(src);
}

// blockIdx.y: image; blockIdx.x: chunk of ENT_CHUNK blocks.
template <class Src, bool RST = false>
__global__ __launch_bounds__(256) void jpeg_ent_bits_kernel(const typename Src::Desc* __restrict__ descs) {
    __shared__ uint32_t tab[536];
    __shared__ uint32_t red[4];
    const typename Src::Desc src = descs[blockIdx.y];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const auto L = EntPhaseLayout<RST>::of(d, phase_blocks<Src, RST>(src));
    if ((long long)blockIdx.x >= L.nchunks) return;
    Src::tables_to_lds(src, tab);
    const long long s = (long long)blockIdx.x * ENT_CHUNK + threadIdx.x;
    uint32_t bits = 0, bad = 0;
    if (s < L.nblk) {
        uint32_t w[32];
        int pred, chroma;
        load_block<RST>(d, s, w, pred, chroma, d.restart_interval);
        BitCounter c;
        bad = code_block(w, pred, tab + 512 + 12 * chroma, tab + 256 * chroma, c) ? 1u : 0u;
        bits = c.bits;
        reinterpret_cast<uint32_t*>(d.scratch + L.o_len)[s] = bits;
    }
    uint32_t total;
    [[maybe_unused]] const uint32_t before = block_scan(bits, red, total);
    if constexpr (RST) {  // an interval's first block leaves its bit offset inside the chunk for jpeg_ent_scan
        const EntIntervals iv = ent_intervals(d);
        const long long j = s / iv.bpi;
        if (s < L.nblk && s == j * iv.bpi && j < L.nint) reinterpret_cast<uint32_t*>(d.scratch + L.o_irel)[j] = before;
    }
    const uint32_t any_bad = __syncthreads_or((int)bad) ? 1u : 0u;
    if (threadIdx.x == 0) reinterpret_cast<uint2*>(d.scratch + L.o_csum)[blockIdx.x] = make_uint2(total, any_bad);
}

// blockIdx.x: image.
template <class Src, bool RST = false>
__global__ __launch_bounds__(256) void jpeg_ent_scan_kernel(const typename Src::Desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const typename Src::Desc src = descs[blockIdx.x];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const auto L = EntPhaseLayout<RST>::of(d, phase_blocks<Src, RST>(src));
    if (L.nblk == 0) return;
    const uint32_t* csum = reinterpret_cast<const uint32_t*>(d.scratch + L.o_csum);
    const unsigned long long bits = scan_u32_to_u64(csum, 2, L.nchunks, reinterpret_cast<unsigned long long*>(d.scratch + L.o_coff), red);
    [[maybe_unused]] unsigned long long nbytes = (bits + 7) >> 3;
    if constexpr (RST) {  // the intervals: bytes of each, then their offsets in the unstuffed stream
        const EntIntervals iv = ent_intervals(d);
        const long long count = iv.count < L.nint ? iv.count : L.nint;
        unsigned long long* ioff = reinterpret_cast<unsigned long long*>(d.scratch + L.o_ioff);
        if (count > 1) {
            const unsigned long long* coff = reinterpret_cast<const unsigned long long*>(d.scratch + L.o_coff);
            const uint32_t* irel = reinterpret_cast<const uint32_t*>(d.scratch + L.o_irel);
            uint32_t* ilen = reinterpret_cast<uint32_t*>(d.scratch + L.o_ilen);
            __syncthreads();  // (coff[] of the scan above is read by other threads than wrote it)
            for (long long j = threadIdx.x; j < count; j += 256) ilen[j] = ent_interval_bytes(iv, j, coff, irel, bits);
            __syncthreads();
            nbytes = scan_u32_to_u64(ilen, 1, count, ioff, red);
        } else if (threadIdx.x == 0) {
            ioff[0] = 0;  // (a single interval may hold more bytes than ilen's 32 bits count: it is not scanned)
        }
        if (threadIdx.x == 0) ioff[count] = nbytes;
    }
    uint32_t bad = 0;
    for (long long i = threadIdx.x; i < L.nchunks; i += 256) bad |= csum[2 * i + 1];
    bad = __syncthreads_or((int)bad) ? 1u : 0u;
    if (threadIdx.x == 0) {
        EntHeader* h = reinterpret_cast<EntHeader*>(d.scratch);
        h->total_bits = bits;
        h->nbytes = RST ? nbytes : (bits + 7) >> 3;
        h->bad = bad;
        h->ok = 0;
    }
}

// blockIdx.y: image; the workgroups of a row stride over the words in use, sixteen bytes a thread.
template <class Src, bool RST = false>
__global__ __launch_bounds__(256) void jpeg_ent_zero_kernel(const typename Src::Desc* __restrict__ descs) {
    const typename Src::Desc src = descs[blockIdx.y];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const auto L = EntPhaseLayout<RST>::of(d, phase_blocks<Src, RST>(src));
    if (L.nblk == 0) return;
    const unsigned long long nbytes = reinterpret_cast<const EntHeader*>(d.scratch)->nbytes;
    long long quads = (long long)((nbytes + 15) >> 4);
    if (quads > L.nwords / 4) quads = L.nwords / 4;
    uint4* q = reinterpret_cast<uint4*>(d.scratch + L.o_words);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long long)gridDim.x * 256) q[i] = make_uint4(0u, 0u, 0u, 0u);
}

// blockIdx.y: image; blockIdx.x: chunk of ENT_CHUNK blocks.
template <class Src, bool RST = false>
__global__ __launch_bounds__(256) void jpeg_ent_pack_kernel(const typename Src::Desc* __restrict__ descs) {
    __shared__ uint32_t tab[536];
    __shared__ uint32_t red[4];
    const typename Src::Desc src = descs[blockIdx.y];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const auto L = EntPhaseLayout<RST>::of(d, phase_blocks<Src, RST>(src));
    if ((long long)blockIdx.x >= L.nchunks) return;
    Src::tables_to_lds(src, tab);
    const long long s = (long long)blockIdx.x * ENT_CHUNK + threadIdx.x;
    const bool live = s < L.nblk;
    const uint32_t len = live ? reinterpret_cast<const uint32_t*>(d.scratch + L.o_len)[s] : 0u;
    uint32_t total;
    const uint32_t before = block_scan(len, red, total);
    if (!live) return;
    unsigned long long start = reinterpret_cast<const unsigned long long*>(d.scratch + L.o_coff)[blockIdx.x] + before;
    bool pads = s == L.nblk - 1;
    if constexpr (RST) {  // the block's place inside its byte-aligned interval; every interval pads
        const EntIntervals iv = ent_intervals(d);
        if (iv.count > 1 && iv.count <= L.nint) {
            start = ent_pack_start(iv, s, start, reinterpret_cast<const unsigned long long*>(d.scratch + L.o_coff),
                                   reinterpret_cast<const uint32_t*>(d.scratch + L.o_irel), reinterpret_cast<const unsigned long long*>(d.scratch + L.o_ioff));
            pads = ent_pads(iv, s, L.nblk);
        }
    }
    uint32_t w[32];
    int pred, chroma;
    load_block<RST>(d, s, w, pred, chroma, d.restart_interval);
    BitPacker p(reinterpret_cast<uint32_t*>(d.scratch + L.o_words), start, L.nwords);
    code_block(w, pred, tab + 512 + 12 * chroma, tab + 256 * chroma, p);
    if (pads && p.phase()) p.put(0x7Fu, 8 - p.phase());  // the last byte is padded with ones
    p.finish();
}

// A thread's eight bytes of chunk c (two words) and how many of them lie inside the stream.
__device__ __forceinline__ int load_stream(const uint32_t* words, long long c, unsigned long long nbytes, uint32_t (&v)[2], long long& byte0) {
    byte0 = c * STUFF_CHUNK + 8 * (long long)threadIdx.x;
    const long long left = (long long)nbytes - byte0;
    const int valid = left >= 8 ? 8 : (left > 0 ? (int)left : 0);
    v[0] = valid > 0 ? words[byte0 >> 2] : 0u;
    v[1] = valid > 4 ? words[(byte0 >> 2) + 1] : 0u;
    return valid;
}

__device__ __forceinline__ uint32_t count_ff(const uint32_t (&v)[2], int valid) {
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) n += (k < valid && stream_byte(v[k >> 2], k & 3) == 255u) ? 1u : 0u;
    return n;
}

// blockIdx.y: image; the workgroups of a row stride over the chunks of STUFF_CHUNK bytes in use.
template <class Src, bool RST = false>
__global__ __launch_bounds__(256) void jpeg_ent_ffcount_kernel(const typename Src::Desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const typename Src::Desc src = descs[blockIdx.y];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const auto L = EntPhaseLayout<RST>::of(d, phase_blocks<Src, RST>(src));
    if (L.nblk == 0) return;
    const unsigned long long nbytes = reinterpret_cast<const EntHeader*>(d.scratch)->nbytes;
    long long chunks = (long long)((nbytes + STUFF_CHUNK - 1) / STUFF_CHUNK);
    if (chunks > L.nstuff) chunks = L.nstuff;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(d.scratch + L.o_words);
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        uint32_t v[2];
        long long byte0;
        const int valid = load_stream(words, c, nbytes, v, byte0);
        uint32_t total;
        block_scan(count_ff(v, valid), red, total);
        if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(d.scratch + L.o_sff)[c] = total;
    }
}

// blockIdx.x: image.
template <class Src, bool RST = false>
__global__ __launch_bounds__(256) void jpeg_ent_ffscan_kernel(const typename Src::Desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const typename Src::Desc src = descs[blockIdx.x];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const auto L = EntPhaseLayout<RST>::of(d, phase_blocks<Src, RST>(src));
    if (L.nblk == 0) {
        if (threadIdx.x == 0 && d.result) {
            d.result->bytes = 0;
            d.result->status = PP_ERR_INVALID_ARG;
            d.result->reserved = 0;
        }
        return;
    }
    EntHeader* h = reinterpret_cast<EntHeader*>(d.scratch);
    const unsigned long long nbytes = h->nbytes;
    const uint32_t bad = h->bad;
    long long chunks = (long long)((nbytes + STUFF_CHUNK - 1) / STUFF_CHUNK);
    if (chunks > L.nstuff) chunks = L.nstuff;
    const unsigned long long ff = scan_u32_to_u64(reinterpret_cast<const uint32_t*>(d.scratch + L.o_sff), 1, chunks,
                                                  reinterpret_cast<unsigned long long*>(d.scratch + L.o_soff), red);
    if (threadIdx.x == 0) {
        long long need = (long long)(nbytes + ff);
        if constexpr (RST) need += 2 * (ent_intervals(d).count - 1);  // the markers between the intervals
        const int status = bad ? PP_ERR_INVALID_ARG : (need > d.capacity ? PP_ERR_WORKSPACE : PP_OK);
        d.result->bytes = need;
        d.result->status = status;
        d.result->reserved = 0;
        h->ok = status == PP_OK ? 1u : 0u;
    }
}

// blockIdx.y: image; the workgroups of a row stride over the chunks of STUFF_CHUNK bytes in use.
template <class Src, bool RST = false>
__global__ __launch_bounds__(256) void jpeg_ent_stuff_kernel(const typename Src::Desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const typename Src::Desc src = descs[blockIdx.y];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const auto L = EntPhaseLayout<RST>::of(d, phase_blocks<Src, RST>(src));
    if (L.nblk == 0) return;
    const EntHeader* h = reinterpret_cast<const EntHeader*>(d.scratch);
    if (!h->ok) return;
    const unsigned long long nbytes = h->nbytes;
    long long chunks = (long long)((nbytes + STUFF_CHUNK - 1) / STUFF_CHUNK);
    if (chunks > L.nstuff) chunks = L.nstuff;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(d.scratch + L.o_words);
    const unsigned long long* soff = reinterpret_cast<const unsigned long long*>(d.scratch + L.o_soff);
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        uint32_t v[2];
        long long byte0;
        const int valid = load_stream(words, c, nbytes, v, byte0);
        uint32_t total;
        const uint32_t before = block_scan(count_ff(v, valid), red, total);
        long long pos = byte0 + (long long)soff[c] + before;
        if constexpr (RST) {
            const EntIntervals iv = ent_intervals(d);
            if (iv.count > 1 && iv.count <= L.nint) {
                ent_stuff_restart(v, valid, byte0, pos, reinterpret_cast<const unsigned long long*>(d.scratch + L.o_ioff), iv.count, d.out, d.capacity);
                continue;
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < valid) {
                const uint32_t b = stream_byte(v[k >> 2], k & 3);
                if (pos < d.capacity) d.out[pos] = (uint8_t)b;
                ++pos;
                if (b == 255u) {
                    if (pos < d.capacity) d.out[pos] = 0;
                    ++pos;
                }
            }
        }
    }
}

// The grids of the seven launches for n images of at most max_blocks blocks.
struct EntGrids {
    dim3 per_chunk, per_image, zero, stuff;
    // restart: the launches of a *_restart_batch call (ent_rst_layout; an image has at most a third as many MCUs as blocks)
    EntGrids(long long max_blocks, int n, bool restart = false) {
        const EntLayout L = restart ? (EntLayout)ent_rst_layout(max_blocks, max_blocks / 3) : ent_layout(max_blocks);
        const long long quads = (L.nwords / 4 + 255) / 256;
        per_chunk = dim3((unsigned)L.nchunks, n);
        per_image = dim3(n);
        zero = dim3((unsigned)(quads < ENT_STRIDE_WGS ? quads : ENT_STRIDE_WGS), n);
        stuff = dim3((unsigned)(L.nstuff < ENT_STRIDE_WGS ? L.nstuff : ENT_STRIDE_WGS), n);
    }
};

}  // namespace pp
