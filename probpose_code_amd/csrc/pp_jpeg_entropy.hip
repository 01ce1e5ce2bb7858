// The Huffman coder of the split JPEG encoder on the device: from the quantised coefficients pp_jpeg_forward_batch leaves
// (per component [block_row][block_col][64], natural order) to the entropy-coded bytes entropy_encode of
// csrc/pp_jpeg_enc_host.h writes between the SOS header and the EOI marker - one interleaved scan, annex K tables, ZRL for
// runs above 15, EOB unless zigzag position 63 is non-zero, bits MSB first, the last byte padded with ones, every data byte
// FF followed by 00. A batch of images of any mix of sizes and sampling per call, driven by a device table of
// pp_jpeg_ent_desc. pp_jpeg_entropy_encode_batch codes without restart intervals; pp_jpeg_entropy_encode_restart_batch (at
// the end of this comment) honours every image's own.
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
// which the sequential host check (scripts/jpeg_entropy_host_check.cpp) runs as well. The kernels are the templates of
// csrc/pp_jpeg_entropy_phases.h, instantiated here with annex K's tables (csrc/pp_jpeg_entropy_opt.hip instantiates them
// with an image's own).
//
// Restart intervals (pp_jpeg_entropy_encode_restart_batch; every image its own interval R, 0 included) keep that shape and
// add a second, segmented level. The same seven launches, the phase templates instantiated with RST:
//   jpeg_ent_rst_bits     load_block returns predictor 0 for the first block of each component of an interval; the thread of
//                         an interval's first block also leaves its bit offset inside the chunk in irel[];
//   jpeg_ent_rst_scan     behind the chunk scan, still one workgroup per image: interval j has P[start j+1] - P[start j]
//                         bits (P: chunk offset + irel), ilen[j] = its bytes rounded up, ioff[] = their prefix sums - the
//                         unstuffed stream is the byte-aligned intervals back to back;
//   jpeg_ent_rst_pack     block s of interval j packs at bit 8 ioff[j] + P[s] - P[start j]; the last block of EVERY interval
//                         pads with ones;
//   jpeg_ent_rst_ffcount  as before: a padding byte FF is a data byte and is stuffed;
//   jpeg_ent_rst_ffscan   need = unstuffed bytes + FF bytes + 2 (intervals - 1);
//   jpeg_ent_rst_stuff    a byte's place grows by 2 x (intervals before it) - one binary search in ioff[] per thread - and the
//                         thread that holds the last byte of interval j < last writes FF, D0 + (j & 7) behind it, unstuffed
//                         (ent_stuff_restart: a thread's eight bytes may cross several interval ends).
// ioff[] is strictly increasing (an interval holds three blocks of two bits at least), so every byte has one interval.
// The scratch share is ent_rst_layout's (pp_jpeg_entropy_restart_scratch_bytes): ent_layout's regions, the bit buffer longer
// by seven padding bits per MCU, and sixteen bytes of interval table per MCU - any interval down to one MCU fits. The
// instantiations without RST compile to the instructions they had before the argument existed.
#include "pp_common.h"
#include "pp_jpeg_entropy_core.h"
#include "pp_jpeg_entropy_phases.h"

#include <cstdint>

namespace pp {

__constant__ const EntTables kEntTables = ent_tables();

__device__ __forceinline__ void tables_to_lds(uint32_t* lds) {  // 2 x (256 AC + 12 DC) words
    for (int i = threadIdx.x; i < 512; i += blockDim.x) lds[i] = kEntTables.ac[i >> 8][i & 255];
    if (threadIdx.x < 24) lds[512 + threadIdx.x] = kEntTables.dc[threadIdx.x / 12][threadIdx.x % 12];
    __syncthreads();
}

// The coder's own table source: annex K's codes out of constant memory, every descriptor taken as it is.
struct AnnexKSource {
    using Desc = pp_jpeg_ent_desc;
    static __device__ __forceinline__ const pp_jpeg_ent_desc& ent(const Desc& d) { return d; }
    static __device__ __forceinline__ long long blocks(const Desc& d) { return ent_blocks(d); }
    static __device__ __forceinline__ void tables_to_lds(const Desc&, uint32_t* lds) { pp::tables_to_lds(lds); }
};

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
    const EntGrids g(max_blocks, n);
    const dim3 tpb(256);
    hipLaunchKernelGGL(jpeg_ent_bits_kernel<AnnexKSource>, g.per_chunk, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_bits");
    hipLaunchKernelGGL(jpeg_ent_scan_kernel<AnnexKSource>, g.per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_scan");
    hipLaunchKernelGGL(jpeg_ent_zero_kernel<AnnexKSource>, g.zero, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_zero");
    hipLaunchKernelGGL(jpeg_ent_pack_kernel<AnnexKSource>, g.per_chunk, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_pack");
    hipLaunchKernelGGL(jpeg_ent_ffcount_kernel<AnnexKSource>, g.stuff, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_ffcount");
    hipLaunchKernelGGL(jpeg_ent_ffscan_kernel<AnnexKSource>, g.per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_ffscan");
    hipLaunchKernelGGL(jpeg_ent_stuff_kernel<AnnexKSource>, g.stuff, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_stuff");
    return PP_OK;
}

extern "C" long long pp_jpeg_entropy_restart_scratch_bytes(const pp_jpeg_info* infos_host, int n) {
    if (!infos_host || n < 0) {
        pp::set_error("pp_jpeg_entropy_restart_scratch_bytes: bad argument");
        return PP_ERR_INVALID_ARG;
    }
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        if (!pp::jpeg::plan_consistent(infos_host[i])) {
            pp::set_error("pp_jpeg_entropy_restart_scratch_bytes: entry %d is not a pp_jpeg_encode_plan result", i);
            return PP_ERR_INVALID_ARG;
        }
        total += pp::ent_rst_layout(infos_host[i].coef_count / 64, (long long)infos_host[i].mcus_x * infos_host[i].mcus_y).total;
    }
    return total;
}

extern "C" int pp_jpeg_entropy_encode_restart_batch(const pp_jpeg_ent_desc* descriptors, int n, long long max_blocks, void* stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0, PP_ERR_INVALID_ARG, "pp_jpeg_entropy_encode_restart_batch: n < 0");
    if (n == 0) return PP_OK;
    PP_REQUIRE(descriptors, PP_ERR_INVALID_ARG, "pp_jpeg_entropy_encode_restart_batch: NULL argument");
    PP_REQUIRE(max_blocks > 0, PP_ERR_INVALID_ARG, "pp_jpeg_entropy_encode_restart_batch: bad shape");
    PP_REQUIRE(n <= 65535 && max_blocks <= 3ll * 8192 * 8192, PP_ERR_INVALID_ARG,
               "pp_jpeg_entropy_encode_restart_batch: at most 65535 images of sides up to 65535");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const EntGrids g(max_blocks, n, true);
    const dim3 tpb(256);
    hipLaunchKernelGGL((jpeg_ent_bits_kernel<AnnexKSource, true>), g.per_chunk, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_rst_bits");
    hipLaunchKernelGGL((jpeg_ent_scan_kernel<AnnexKSource, true>), g.per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_rst_scan");
    hipLaunchKernelGGL((jpeg_ent_zero_kernel<AnnexKSource, true>), g.zero, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_rst_zero");
    hipLaunchKernelGGL((jpeg_ent_pack_kernel<AnnexKSource, true>), g.per_chunk, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_rst_pack");
    hipLaunchKernelGGL((jpeg_ent_ffcount_kernel<AnnexKSource, true>), g.stuff, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_rst_ffcount");
    hipLaunchKernelGGL((jpeg_ent_ffscan_kernel<AnnexKSource, true>), g.per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_rst_ffscan");
    hipLaunchKernelGGL((jpeg_ent_stuff_kernel<AnnexKSource, true>), g.stuff, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_ent_rst_stuff");
    return PP_OK;
}
