// The seven phases of the device Huffman coder (see csrc/pp_jpeg_entropy.hip for what each does) as kernel templates over
// a table source, so that the coder with annex K's tables (pp_jpeg_entropy.hip) and the one with an image's own optimal tables
// (pp_jpeg_entropy_opt.hip) are one body. A source gives:
//   Desc                      the element of the descriptor table the launches read;
//   ent(desc)                 its pp_jpeg_ent_desc;
//   blocks(desc)              the blocks of the scan, 0 for an image to refuse (jpeg_ent_ffscan then reports PP_ERR_INVALID_ARG);
//   tables_to_lds(desc, lds)  code | size << 16 of every symbol into 536 words: AC luma (256), AC chroma (256), DC luma (12),
//                             DC chroma (12), and the barrier behind it.
#pragma once
#include "pp_common.h"
#include "pp_jpeg_entropy_core.h"

namespace pp {

constexpr int ENT_STRIDE_WGS = 256;   // workgroups per image of the grid-stride launches

// blockIdx.y: image; blockIdx.x: chunk of ENT_CHUNK blocks.
template <class Src>
__global__ __launch_bounds__(256) void jpeg_ent_bits_kernel(const typename Src::Desc* __restrict__ descs) {
    __shared__ uint32_t tab[536];
    __shared__ uint32_t red[4];
    const typename Src::Desc src = descs[blockIdx.y];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const EntLayout L = ent_layout(Src::blocks(src));
    if ((long long)blockIdx.x >= L.nchunks) return;
    Src::tables_to_lds(src, tab);
    const long long s = (long long)blockIdx.x * ENT_CHUNK + threadIdx.x;
    uint32_t bits = 0, bad = 0;
    if (s < L.nblk) {
        uint32_t w[32];
        int pred, chroma;
        load_block(d, s, w, pred, chroma);
        BitCounter c;
        bad = code_block(w, pred, tab + 512 + 12 * chroma, tab + 256 * chroma, c) ? 1u : 0u;
        bits = c.bits;
        reinterpret_cast<uint32_t*>(d.scratch + L.o_len)[s] = bits;
    }
    uint32_t total;
    block_scan(bits, red, total);
    const uint32_t any_bad = __syncthreads_or((int)bad) ? 1u : 0u;
    if (threadIdx.x == 0) reinterpret_cast<uint2*>(d.scratch + L.o_csum)[blockIdx.x] = make_uint2(total, any_bad);
}

// blockIdx.x: image.
template <class Src>
__global__ __launch_bounds__(256) void jpeg_ent_scan_kernel(const typename Src::Desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const typename Src::Desc src = descs[blockIdx.x];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const EntLayout L = ent_layout(Src::blocks(src));
    if (L.nblk == 0) return;
    const uint32_t* csum = reinterpret_cast<const uint32_t*>(d.scratch + L.o_csum);
    const unsigned long long bits = scan_u32_to_u64(csum, 2, L.nchunks, reinterpret_cast<unsigned long long*>(d.scratch + L.o_coff), red);
    uint32_t bad = 0;
    for (long long i = threadIdx.x; i < L.nchunks; i += 256) bad |= csum[2 * i + 1];
    bad = __syncthreads_or((int)bad) ? 1u : 0u;
    if (threadIdx.x == 0) {
        EntHeader* h = reinterpret_cast<EntHeader*>(d.scratch);
        h->total_bits = bits;
        h->nbytes = (bits + 7) >> 3;
        h->bad = bad;
        h->ok = 0;
    }
}

// blockIdx.y: image; the workgroups of a row stride over the words in use, sixteen bytes a thread.
template <class Src>
__global__ __launch_bounds__(256) void jpeg_ent_zero_kernel(const typename Src::Desc* __restrict__ descs) {
    const typename Src::Desc src = descs[blockIdx.y];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const EntLayout L = ent_layout(Src::blocks(src));
    if (L.nblk == 0) return;
    const unsigned long long nbytes = reinterpret_cast<const EntHeader*>(d.scratch)->nbytes;
    long long quads = (long long)((nbytes + 15) >> 4);
    if (quads > L.nwords / 4) quads = L.nwords / 4;
    uint4* q = reinterpret_cast<uint4*>(d.scratch + L.o_words);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long long)gridDim.x * 256) q[i] = make_uint4(0u, 0u, 0u, 0u);
}

// blockIdx.y: image; blockIdx.x: chunk of ENT_CHUNK blocks.
template <class Src>
__global__ __launch_bounds__(256) void jpeg_ent_pack_kernel(const typename Src::Desc* __restrict__ descs) {
    __shared__ uint32_t tab[536];
    __shared__ uint32_t red[4];
    const typename Src::Desc src = descs[blockIdx.y];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const EntLayout L = ent_layout(Src::blocks(src));
    if ((long long)blockIdx.x >= L.nchunks) return;
    Src::tables_to_lds(src, tab);
    const long long s = (long long)blockIdx.x * ENT_CHUNK + threadIdx.x;
    const bool live = s < L.nblk;
    const uint32_t len = live ? reinterpret_cast<const uint32_t*>(d.scratch + L.o_len)[s] : 0u;
    uint32_t total;
    const uint32_t before = block_scan(len, red, total);
    if (!live) return;
    const unsigned long long start = reinterpret_cast<const unsigned long long*>(d.scratch + L.o_coff)[blockIdx.x] + before;
    uint32_t w[32];
    int pred, chroma;
    load_block(d, s, w, pred, chroma);
    BitPacker p(reinterpret_cast<uint32_t*>(d.scratch + L.o_words), start, L.nwords);
    code_block(w, pred, tab + 512 + 12 * chroma, tab + 256 * chroma, p);
    if (s == L.nblk - 1 && p.phase()) p.put(0x7Fu, 8 - p.phase());  // the last byte is padded with ones
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
template <class Src>
__global__ __launch_bounds__(256) void jpeg_ent_ffcount_kernel(const typename Src::Desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const typename Src::Desc src = descs[blockIdx.y];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const EntLayout L = ent_layout(Src::blocks(src));
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
template <class Src>
__global__ __launch_bounds__(256) void jpeg_ent_ffscan_kernel(const typename Src::Desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const typename Src::Desc src = descs[blockIdx.x];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const EntLayout L = ent_layout(Src::blocks(src));
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
        const long long need = (long long)(nbytes + ff);
        const int status = bad ? PP_ERR_INVALID_ARG : (need > d.capacity ? PP_ERR_WORKSPACE : PP_OK);
        d.result->bytes = need;
        d.result->status = status;
        d.result->reserved = 0;
        h->ok = status == PP_OK ? 1u : 0u;
    }
}

// blockIdx.y: image; the workgroups of a row stride over the chunks of STUFF_CHUNK bytes in use.
template <class Src>
__global__ __launch_bounds__(256) void jpeg_ent_stuff_kernel(const typename Src::Desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const typename Src::Desc src = descs[blockIdx.y];
    const pp_jpeg_ent_desc& d = Src::ent(src);
    const EntLayout L = ent_layout(Src::blocks(src));
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
    EntGrids(long long max_blocks, int n) {
        const EntLayout L = ent_layout(max_blocks);
        const long long quads = (L.nwords / 4 + 255) / 256;
        per_chunk = dim3((unsigned)L.nchunks, n);
        per_image = dim3(n);
        zero = dim3((unsigned)(quads < ENT_STRIDE_WGS ? quads : ENT_STRIDE_WGS), n);
        stuff = dim3((unsigned)(L.nstuff < ENT_STRIDE_WGS ? L.nstuff : ENT_STRIDE_WGS), n);
    }
};

}  // namespace pp
