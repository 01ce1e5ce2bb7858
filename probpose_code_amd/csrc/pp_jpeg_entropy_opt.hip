// The JPEG writer's optimised Huffman tables, built and used on the device: pp_jpeg_entropy_encode_opt_batch gives the bytes
// pp_jpeg_entropy_encode_opt (the host form, csrc/pp_jpeg_opt_core.h) writes between the SOS header and EOI, bit for bit, and
// leaves every image's tables in its pp_jpeg_opt_record for the host to put into the DHT segments. No host round trip sits
// between the statistics and the coding. Ten launches, each the barrier between two phases:
//   jpeg_opt_clear    one workgroup per image: its four histograms to zero, its status to PP_OK;
//   jpeg_opt_hist     a thread per block in scan order, 256 blocks per workgroup (the chunks of jpeg_ent_bits): the symbols
//                     of the block (block_symbols: the coder's walk) are counted in LDS, the workgroup's non-zero bins are
//                     added to the record with integer atomicAdd - addition commutes, the sums are the same every launch;
//   jpeg_opt_build    one wave per (image, table), the 257 entries spread over the lanes (five registers each): libjpeg's
//                     merge loop with both minimum searches as wave reductions of opt_key and the lengthening of both trees
//                     as a map over a per-symbol tree id (opt_merge_entry); then the counts per length, annex K.3
//                     (opt_limit_lengths, one lane: a few dozen steps), huffval by rank (opt_rank, a lane per symbol) and
//                     code | length << 16 of every symbol -> bits, vals, nvals, lookup of the record;
//   jpeg_opt_bits .. jpeg_opt_stuff
//                     the coder's seven phases (csrc/pp_jpeg_entropy_phases.h, the bodies pp_jpeg_entropy.hip runs) with the
//                     record's lookup staged in LDS at kernel start in place of annex K's tables.
// An image is refused - result slot PP_ERR_INVALID_ARG, nothing coded - for what pp_jpeg_entropy_encode_batch refuses, for a
// record pointer that is NULL or not 16-byte aligned, for more than OPT_MAX_BLOCKS blocks (32-bit frequencies would not be
// exact) and for a code tree deeper than 32 (the record's status says so too). Every store goes to a fixed place of the
// image's record or, in the phases, is checked against its region as before.
// pp_jpeg_entropy_encode_opt_restart_batch honours every image's restart interval (see csrc/pp_jpeg_entropy.hip): the same ten
// launches with jpeg_opt_hist counting the restarted DC differences (what pp_jpeg_symbol_histogram(..., restart_interval)
// counts on the host) and the seven phases instantiated with RST.
#include "pp_common.h"
#include "pp_jpeg_entropy_phases.h"
#include "pp_jpeg_opt_core.h"

#include <cstdint>

namespace pp {

// The table source of the phases: the image's own lookup. An image whose record was refused has no blocks.
struct OptSource {
    using Desc = pp_jpeg_ent_opt_desc;
    static __device__ __forceinline__ const pp_jpeg_ent_desc& ent(const Desc& d) { return d.ent; }
    // what the plan and the record pointer allow, whatever the record holds
    static __device__ __forceinline__ long long plan_blocks(const Desc& d) {
        const long long n = ent_blocks(d.ent);
        return (d.record && (reinterpret_cast<uintptr_t>(d.record) & 15) == 0 && n <= OPT_MAX_BLOCKS) ? n : 0;
    }
    static __device__ __forceinline__ long long blocks(const Desc& d) {
        const long long n = plan_blocks(d);
        return (n && d.record->status == PP_OK) ? n : 0;
    }
    static __device__ __forceinline__ void tables_to_lds(const Desc& d, uint32_t* lds) {  // the layout of annex K's: AC, AC, DC, DC
        for (int i = threadIdx.x; i < 512; i += blockDim.x) lds[i] = d.record->lookup[(i >> 8) ? OPT_AC_CHROMA : OPT_AC_LUMA][i & 255];
        if (threadIdx.x < 24) lds[512 + threadIdx.x] = d.record->lookup[threadIdx.x / 12 ? OPT_DC_CHROMA : OPT_DC_LUMA][threadIdx.x % 12];
        __syncthreads();
    }
};

// blockIdx.x: image.
__global__ __launch_bounds__(256) void jpeg_opt_clear_kernel(const pp_jpeg_ent_opt_desc* __restrict__ descs) {
    const pp_jpeg_ent_opt_desc src = descs[blockIdx.x];
    if (OptSource::plan_blocks(src) == 0) return;
    uint32_t* hist = &src.record->hist[0][0];
    for (int i = threadIdx.x; i < 4 * OPT_BINS; i += 256) hist[i] = 0u;
    if (threadIdx.x == 0) src.record->status = PP_OK;
    if (threadIdx.x < 7) src.record->reserved[threadIdx.x] = 0;
}

struct LdsHistSink {
    uint32_t* dc_bins;
    uint32_t* ac_bins;
    __device__ __forceinline__ void dc(int s) { atomicAdd(dc_bins + s, 1u); }
    __device__ __forceinline__ void ac(int rs) { atomicAdd(ac_bins + rs, 1u); }
};

// blockIdx.y: image; blockIdx.x: chunk of ENT_CHUNK blocks. RST: the DC prediction restarts with the image's interval.
template <bool RST>
__device__ __forceinline__ void opt_hist_body(const pp_jpeg_ent_opt_desc* __restrict__ descs) {
    __shared__ uint32_t bins[536];  // AC luma (256), AC chroma (256), DC luma (12), DC chroma (12)
    const pp_jpeg_ent_opt_desc src = descs[blockIdx.y];
    const EntLayout L = ent_layout(OptSource::plan_blocks(src));
    if ((long long)blockIdx.x >= L.nchunks) return;
    for (int i = threadIdx.x; i < 536; i += 256) bins[i] = 0u;
    __syncthreads();
    const long long s = (long long)blockIdx.x * ENT_CHUNK + threadIdx.x;
    if (s < L.nblk) {
        uint32_t w[32];
        int pred, chroma;
        load_block<RST>(src.ent, s, w, pred, chroma, src.ent.restart_interval);
        LdsHistSink sink{bins + 512 + 12 * chroma, bins + 256 * chroma};
        block_symbols(w, pred, sink);  // (a coefficient outside the codes is the coder's to report)
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 536; i += 256) {
        const uint32_t v = bins[i];
        if (v == 0u) continue;
        const int j = i - 512;
        uint32_t* bin = i < 512 ? &src.record->hist[(i >> 8) ? OPT_AC_CHROMA : OPT_AC_LUMA][i & 255]
                                : &src.record->hist[j / 12 ? OPT_DC_CHROMA : OPT_DC_LUMA][j % 12];
        atomicAdd(bin, v);
    }
}

__global__ __launch_bounds__(256) void jpeg_opt_hist_kernel(const pp_jpeg_ent_opt_desc* __restrict__ descs) { opt_hist_body<false>(descs); }
__global__ __launch_bounds__(256) void jpeg_opt_hist_rst_kernel(const pp_jpeg_ent_opt_desc* __restrict__ descs) { opt_hist_body<true>(descs); }

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o);
        v = other < v ? other : v;
    }
    return v;
}

constexpr int OPT_PER_LANE = (OPT_BINS + WAVE - 1) / WAVE;  // entries lane + 64 e

// blockIdx.y: image; blockIdx.x: table. One wave.
__global__ __launch_bounds__(64) void jpeg_opt_build_kernel(const pp_jpeg_ent_opt_desc* __restrict__ descs) {
    __shared__ uint32_t count[OPT_MAX_CLEN + 1];
    __shared__ uint8_t size8[256], bits[16], vals[256];
    __shared__ uint32_t look[256];
    __shared__ OptCodeBase base;
    __shared__ int deep, nvals;
    const pp_jpeg_ent_opt_desc src = descs[blockIdx.y];
    if (OptSource::plan_blocks(src) == 0) return;
    pp_jpeg_opt_record* rec = src.record;
    const int t = blockIdx.x, lane = threadIdx.x;
    uint32_t freq[OPT_PER_LANE];
    int tree[OPT_PER_LANE], size[OPT_PER_LANE];
#pragma unroll
    for (int e = 0; e < OPT_PER_LANE; ++e) {
        const int i = lane + WAVE * e;
        freq[e] = i < 256 ? rec->hist[t][i] : (i == 256 ? 1u : 0u);
        tree[e] = i;
        size[e] = 0;
    }
    for (int merge = 0; merge < OPT_BINS - 1; ++merge) {  // (every merge empties one of 257 entries)
        unsigned long long k1 = OPT_NO_KEY, k2 = OPT_NO_KEY;
#pragma unroll
        for (int e = 0; e < OPT_PER_LANE; ++e) {
            const unsigned long long k = freq[e] ? opt_key(freq[e], lane + WAVE * e) : OPT_NO_KEY;
            k1 = k < k1 ? k : k1;
        }
        k1 = wave_min(k1);
        const int c1 = opt_key_symbol(k1);
#pragma unroll
        for (int e = 0; e < OPT_PER_LANE; ++e) {
            const int i = lane + WAVE * e;
            const unsigned long long k = (freq[e] && i != c1) ? opt_key(freq[e], i) : OPT_NO_KEY;
            k2 = k < k2 ? k : k2;
        }
        k2 = wave_min(k2);
        if (k2 == OPT_NO_KEY) break;  // (the same in every lane)
        const int c2 = opt_key_symbol(k2);
        const uint32_t f1 = opt_key_freq(k1), f2 = opt_key_freq(k2);
#pragma unroll
        for (int e = 0; e < OPT_PER_LANE; ++e) opt_merge_entry(lane + WAVE * e, c1, c2, f1, f2, freq[e], tree[e], size[e]);
    }
    if (lane <= OPT_MAX_CLEN) count[lane] = 0u;
    if (lane == 0) deep = 0;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < OPT_PER_LANE; ++e) {
        const int i = lane + WAVE * e;
        if (i < OPT_BINS && size[e] > 0) {
            if (size[e] > OPT_MAX_CLEN) deep = 1;
            else atomicAdd(&count[size[e]], 1u);
        }
        if (i < 256) size8[i] = (uint8_t)(size[e] > OPT_MAX_CLEN ? OPT_MAX_CLEN + 1 : size[e]);
    }
    __syncthreads();
    if (deep) {
        if (lane == 0) rec->status = PP_ERR_INVALID_ARG;
        return;
    }
    if (lane == 0) {
        opt_limit_lengths(count);
        int n = 0;
        for (int l = 1; l <= 16; ++l) {
            bits[l - 1] = (uint8_t)count[l];
            n += (int)count[l];
        }
        nvals = n;
        opt_code_base(bits, base);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        vals[lane + WAVE * e] = 0;
        look[lane + WAVE * e] = 0u;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = lane + WAVE * e;
        if (size8[i]) {
            const int k = opt_rank(size8, i);  // (< nvals <= 256: one place per coded symbol)
            vals[k] = (uint8_t)i;
            look[i] = opt_code_of(base, bits, (uint32_t)k);
        }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = lane + WAVE * e;
        rec->vals[t][i] = vals[i];
        rec->lookup[t][i] = look[i];
    }
    if (lane < 16) rec->bits[t][lane] = bits[lane];
    if (lane == 0) rec->nvals[t] = nvals;
}

}  // namespace pp

extern "C" long long pp_jpeg_entropy_opt_scratch_bytes(const pp_jpeg_info* infos_host, int n) {
    if (!infos_host || n < 0) {
        pp::set_error("pp_jpeg_entropy_opt_scratch_bytes: bad argument");
        return PP_ERR_INVALID_ARG;
    }
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        if (pp::jpeg::check_opt_plan(&infos_host[i], 0) != PP_OK) {
            pp::set_error("pp_jpeg_entropy_opt_scratch_bytes: entry %d: %s", i, pp::jpeg::g_reason);
            return PP_ERR_INVALID_ARG;
        }
        total += pp::ent_layout(infos_host[i].coef_count / 64).total;
    }
    return total;
}

extern "C" int pp_jpeg_entropy_encode_opt_batch(const pp_jpeg_ent_opt_desc* descriptors, int n, long long max_blocks, void* stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0, PP_ERR_INVALID_ARG, "pp_jpeg_entropy_encode_opt_batch: n < 0");
    if (n == 0) return PP_OK;
    PP_REQUIRE(descriptors, PP_ERR_INVALID_ARG, "pp_jpeg_entropy_encode_opt_batch: NULL argument");
    PP_REQUIRE(max_blocks > 0, PP_ERR_INVALID_ARG, "pp_jpeg_entropy_encode_opt_batch: bad shape");
    PP_REQUIRE(n <= 65535 && max_blocks <= OPT_MAX_BLOCKS, PP_ERR_INVALID_ARG,
               "pp_jpeg_entropy_encode_opt_batch: at most 65535 images of at most 2^32 / 64 blocks");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const EntGrids g(max_blocks, n);
    const dim3 tpb(256);
    hipLaunchKernelGGL(jpeg_opt_clear_kernel, g.per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_clear");
    hipLaunchKernelGGL(jpeg_opt_hist_kernel, g.per_chunk, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_hist");
    hipLaunchKernelGGL(jpeg_opt_build_kernel, dim3(4, n), dim3(WAVE), 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_build");
    hipLaunchKernelGGL(jpeg_ent_bits_kernel<OptSource>, g.per_chunk, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_bits");
    hipLaunchKernelGGL(jpeg_ent_scan_kernel<OptSource>, g.per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_scan");
    hipLaunchKernelGGL(jpeg_ent_zero_kernel<OptSource>, g.zero, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_zero");
    hipLaunchKernelGGL(jpeg_ent_pack_kernel<OptSource>, g.per_chunk, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_pack");
    hipLaunchKernelGGL(jpeg_ent_ffcount_kernel<OptSource>, g.stuff, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_ffcount");
    hipLaunchKernelGGL(jpeg_ent_ffscan_kernel<OptSource>, g.per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_ffscan");
    hipLaunchKernelGGL(jpeg_ent_stuff_kernel<OptSource>, g.stuff, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_stuff");
    return PP_OK;
}

extern "C" int pp_jpeg_entropy_encode_opt_restart_batch(const pp_jpeg_ent_opt_desc* descriptors, int n, long long max_blocks, void* stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0, PP_ERR_INVALID_ARG, "pp_jpeg_entropy_encode_opt_restart_batch: n < 0");
    if (n == 0) return PP_OK;
    PP_REQUIRE(descriptors, PP_ERR_INVALID_ARG, "pp_jpeg_entropy_encode_opt_restart_batch: NULL argument");
    PP_REQUIRE(max_blocks > 0, PP_ERR_INVALID_ARG, "pp_jpeg_entropy_encode_opt_restart_batch: bad shape");
    PP_REQUIRE(n <= 65535 && max_blocks <= OPT_MAX_BLOCKS, PP_ERR_INVALID_ARG,
               "pp_jpeg_entropy_encode_opt_restart_batch: at most 65535 images of at most 2^32 / 64 blocks");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const EntGrids g(max_blocks, n, true);
    const dim3 tpb(256);
    hipLaunchKernelGGL(jpeg_opt_clear_kernel, g.per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_clear");
    hipLaunchKernelGGL(jpeg_opt_hist_rst_kernel, g.per_chunk, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_rst_hist");
    hipLaunchKernelGGL(jpeg_opt_build_kernel, dim3(4, n), dim3(WAVE), 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_build");
    hipLaunchKernelGGL((jpeg_ent_bits_kernel<OptSource, true>), g.per_chunk, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_rst_bits");
    hipLaunchKernelGGL((jpeg_ent_scan_kernel<OptSource, true>), g.per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_rst_scan");
    hipLaunchKernelGGL((jpeg_ent_zero_kernel<OptSource, true>), g.zero, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_rst_zero");
    hipLaunchKernelGGL((jpeg_ent_pack_kernel<OptSource, true>), g.per_chunk, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_rst_pack");
    hipLaunchKernelGGL((jpeg_ent_ffcount_kernel<OptSource, true>), g.stuff, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_rst_ffcount");
    hipLaunchKernelGGL((jpeg_ent_ffscan_kernel<OptSource, true>), g.per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_rst_ffscan");
    hipLaunchKernelGGL((jpeg_ent_stuff_kernel<OptSource, true>), g.stuff, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_opt_rst_stuff");
    return PP_OK;
}

extern "C" int pp_jpeg_symbol_histogram(const int16_t* coef_host, const pp_jpeg_info* info, int restart_interval, uint32_t hist[4][257]) {
    const int st = pp::jpeg::symbol_histogram(coef_host, info, restart_interval, hist);
    if (st != PP_OK) pp::set_error("pp_jpeg_symbol_histogram: %s", pp::jpeg::g_reason);
    return st;
}

extern "C" int pp_jpeg_optimal_table(const uint32_t freq[257], uint8_t bits[16], uint8_t vals[256], int* nvals) {
    const int st = pp::jpeg::optimal_table(freq, bits, vals, nvals);
    if (st != PP_OK) pp::set_error("pp_jpeg_optimal_table: %s", pp::jpeg::g_reason);
    return st;
}

extern "C" int pp_jpeg_write_headers_tables(const uint16_t* qtables_host, const pp_jpeg_info* info, int restart_interval, const uint8_t bits[4][16],
                                            const uint8_t vals[4][256], void* out_host, size_t capacity, size_t* size_out) {
    const int st = pp::jpeg::write_headers_tables(qtables_host, info, restart_interval, bits, vals, static_cast<uint8_t*>(out_host), capacity, size_out);
    if (st != PP_OK) pp::set_error("pp_jpeg_write_headers_tables: %s", pp::jpeg::g_reason);
    return st;
}

extern "C" int pp_jpeg_entropy_encode_opt(const int16_t* coef_host, const uint16_t* qtables_host, const pp_jpeg_info* info,
                                          int restart_interval, void* out_host, size_t capacity, size_t* size_out) {
    const int st = pp::jpeg::entropy_encode_opt(coef_host, qtables_host, info, restart_interval, static_cast<uint8_t*>(out_host), capacity, size_out);
    if (st != PP_OK) pp::set_error("pp_jpeg_entropy_encode_opt: %s", pp::jpeg::g_reason);
    return st;
}
