// The Huffman coder of the split JPEG encoder on the device: from the quantised coefficients pp_jpeg_forward_batch leaves
// (per component [block_row][block_col][64], natural order) to the entropy-coded bytes entropy_encode of
// csrc/pp_jpeg_enc_host.h writes between the SOS header and the EOI marker - one interleaved scan, annex K tables, ZRL for
// runs above 15, EOB unless zigzag position 63 is non-zero, bits MSB first, the last byte padded with ones, every data byte
// FF followed by 00. Restart interval 0 only. A batch of images of any mix of sizes and sampling per call, driven by a
// device table of pp_jpeg_ent_desc.
//
// Encoding has no serial dependency: a block's code depends on its own 64 coefficients and on the DC value of the block
// before it in scan order, which is read in place. So it is a map, a prefix sum and a scatter, twice - once for the bits,
// once for the stuffed bytes. Seven launches, each the barrier between two phases; no workgroup ever waits for another:
//   jpeg_ent_bits     a thread per block (scan order): its code length in bits -> len[]; a workgroup's 256 blocks are one
//                     chunk (ENT_CHUNK), whose sum and invalid-coefficient flag go to csum[];
//   jpeg_ent_scan     one workgroup per image: exclusive 64-bit prefix sums of csum[] -> coff[], the total -> hdr;
//   jpeg_ent_zero     zeroes the words the bits will be ORed into (only those the total needs);
//   jpeg_ent_pack     a thread per block again: its bit offset is coff[chunk] + the prefix of len[] inside the chunk; it
//                     codes the block a second time and ORs the bits into 32-bit words (word w holds stream bits
//                     32 w .. 32 w + 31, most significant first). The thread of the image's last block pads with ones;
//   jpeg_ent_ffcount  FF bytes per STUFF_CHUNK bytes of the unstuffed stream -> sff[];
//   jpeg_ent_ffscan   one workgroup per image: prefix sums of sff[] -> soff[]; byte count and status -> the result slot;
//   jpeg_ent_stuff    every byte to its place in the output, a 00 behind every FF.
// Integer OR into zeroed words commutes, every other store has one writer: the bytes are the same from launch to launch.
// Bit and byte offsets are 64-bit (a 65535 x 65535 plan has 2.0e8 blocks of up to 1665 bits). The coefficients are only
// read. A coefficient outside what a baseline code expresses is coded with its category clamped (so every length stays
// inside the bound the scratch is sized for) and flags the image: status PP_ERR_INVALID_ARG, stream undefined.
// Every store into scratch or output is checked against the size of its region.
// The tables, the scratch layout, the block addressing, the code walk and the bit packer are csrc/pp_jpeg_entropy_core.h,
// which the sequential host check (scripts/jpeg_entropy_host_check.cpp) runs as well; here are the kernels.
#include "pp_common.h"
#include "pp_jpeg_entropy_core.h"

#include <cstdint>

namespace pp {

constexpr int ENT_STRIDE_WGS = 256;   // workgroups per image of the grid-stride launches

__constant__ const EntTables kEntTables = ent_tables();

__device__ __forceinline__ void tables_to_lds(uint32_t* lds) {  // 2 x (256 AC + 12 DC) words
    for (int i = threadIdx.x; i < 512; i += blockDim.x) lds[i] = kEntTables.ac[i >> 8][i & 255];
    if (threadIdx.x < 24) lds[512 + threadIdx.x] = kEntTables.dc[threadIdx.x / 12][threadIdx.x % 12];
    __syncthreads();
}

// blockIdx.y: image; blockIdx.x: chunk of ENT_CHUNK blocks.
__global__ __launch_bounds__(256) void jpeg_ent_bits_kernel(const pp_jpeg_ent_desc* __restrict__ descs) {
    __shared__ uint32_t tab[536];
    __shared__ uint32_t red[4];
    const pp_jpeg_ent_desc d = descs[blockIdx.y];
    const EntLayout L = ent_layout(ent_blocks(d));
    if ((long long)blockIdx.x >= L.nchunks) return;
    tables_to_lds(tab);
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
__global__ __launch_bounds__(256) void jpeg_ent_scan_kernel(const pp_jpeg_ent_desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const pp_jpeg_ent_desc d = descs[blockIdx.x];
    const EntLayout L = ent_layout(ent_blocks(d));
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
__global__ __launch_bounds__(256) void jpeg_ent_zero_kernel(const pp_jpeg_ent_desc* __restrict__ descs) {
    const pp_jpeg_ent_desc d = descs[blockIdx.y];
    const EntLayout L = ent_layout(ent_blocks(d));
    if (L.nblk == 0) return;
    const unsigned long long nbytes = reinterpret_cast<const EntHeader*>(d.scratch)->nbytes;
    long long quads = (long long)((nbytes + 15) >> 4);
    if (quads > L.nwords / 4) quads = L.nwords / 4;
    uint4* q = reinterpret_cast<uint4*>(d.scratch + L.o_words);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long long)gridDim.x * 256) q[i] = make_uint4(0u, 0u, 0u, 0u);
}

// blockIdx.y: image; blockIdx.x: chunk of ENT_CHUNK blocks.
__global__ __launch_bounds__(256) void jpeg_ent_pack_kernel(const pp_jpeg_ent_desc* __restrict__ descs) {
    __shared__ uint32_t tab[536];
    __shared__ uint32_t red[4];
    const pp_jpeg_ent_desc d = descs[blockIdx.y];
    const EntLayout L = ent_layout(ent_blocks(d));
    if ((long long)blockIdx.x >= L.nchunks) return;
    tables_to_lds(tab);
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
__global__ __launch_bounds__(256) void jpeg_ent_ffcount_kernel(const pp_jpeg_ent_desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const pp_jpeg_ent_desc d = descs[blockIdx.y];
    const EntLayout L = ent_layout(ent_blocks(d));
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
__global__ __launch_bounds__(256) void jpeg_ent_ffscan_kernel(const pp_jpeg_ent_desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const pp_jpeg_ent_desc d = descs[blockIdx.x];
    const EntLayout L = ent_layout(ent_blocks(d));
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
__global__ __launch_bounds__(256) void jpeg_ent_stuff_kernel(const pp_jpeg_ent_desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const pp_jpeg_ent_desc d = descs[blockIdx.y];
    const EntLayout L = ent_layout(ent_blocks(d));
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

}  // namespace pp

extern "C" long long pp_jpeg_entropy_scratch_bytes(const pp_jpeg_info* infos_host, int n) {
    if (!infos_host || n < 0) {
        pp::set_error("pp_jpeg_entropy_scratch_bytes: bad argument");
        return PP_ERR_INVALID_ARG;
    }
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        if (!pp::jpeg::plan_consistent(infos_host[i])) {
            pp::set_error("pp_jpeg_entropy_scratch_bytes: entry %d is not a pp_jpeg_encode_plan result", i);
            return PP_ERR_INVALID_ARG;
        }
        total += pp::ent_layout(infos_host[i].coef_count / 64).total;
    }
    return total;
}

extern "C" int pp_jpeg_entropy_encode_batch(const pp_jpeg_ent_desc* descriptors, int n, long long max_blocks, void* stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0, PP_ERR_INVALID_ARG, "pp_jpeg_entropy_encode_batch: n < 0");
    if (n == 0) return PP_OK;
    PP_REQUIRE(descriptors, PP_ERR_INVALID_ARG, "pp_jpeg_entropy_encode_batch: NULL argument");
    PP_REQUIRE(max_blocks > 0, PP_ERR_INVALID_ARG, "pp_jpeg_entropy_encode_batch: bad shape");
    PP_REQUIRE(n <= 65535 && max_blocks <= 3ll * 8192 * 8192, PP_ERR_INVALID_ARG,
               "pp_jpeg_entropy_encode_batch: at most 65535 images of sides up to 65535");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const EntLayout L = ent_layout(max_blocks);
    const dim3 per_chunk((unsigned)L.nchunks, n), per_image(n), tpb(256);
    const long long quads = (L.nwords / 4 + 255) / 256;
    const dim3 zero_grid((unsigned)(quads < ENT_STRIDE_WGS ? quads : ENT_STRIDE_WGS), n);
    const dim3 stuff_grid((unsigned)(L.nstuff < ENT_STRIDE_WGS ? L.nstuff : ENT_STRIDE_WGS), n);
    hipLaunchKernelGGL(jpeg_ent_bits_kernel, per_chunk, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_bits");
    hipLaunchKernelGGL(jpeg_ent_scan_kernel, per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_scan");
    hipLaunchKernelGGL(jpeg_ent_zero_kernel, zero_grid, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_zero");
    hipLaunchKernelGGL(jpeg_ent_pack_kernel, per_chunk, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_pack");
    hipLaunchKernelGGL(jpeg_ent_ffcount_kernel, stuff_grid, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_ffcount");
    hipLaunchKernelGGL(jpeg_ent_ffscan_kernel, per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_ffscan");
    hipLaunchKernelGGL(jpeg_ent_stuff_kernel, stuff_grid, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_stuff");
    return PP_OK;
}
