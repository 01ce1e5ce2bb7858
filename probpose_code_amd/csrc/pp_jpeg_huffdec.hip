// The Huffman decoder of the split JPEG decoder on the device: from a file's own entropy-coded bytes (byte stuffing
// included, as pp_jpeg_scan_prepare and pp_jpeg_scan_prepare_restart bound them) to the quantised coefficients
// pp_jpeg_entropy_decode of csrc/pp_jpeg_host.h gives, bit for bit, in the layout pp_jpeg_reconstruct_bgr_batch reads. Files
// with and without a restart interval; the file's own DHT tables. A batch of images of any mix of sizes and sampling per call, driven by a device
// table of pp_jpeg_hd_desc.
//
// A Huffman stream has a serial dependency, but a weak one: a decoder started at a wrong bit position (or a wrong place in
// the MCU) falls into step with the true decoder after a short distance (Klein and Wiseman; Weissenberger and Schmidt,
// "Accelerating JPEG decompression on GPUs"). So the stream is cut into subsequences of HD_S = 128 raw bytes, one per
// thread, and decoding becomes maps, prefix sums and a scatter. sync_passes + 4 launches, each the barrier between two
// phases; no workgroup ever waits for another:
//   jpeg_hd_sync   (sync_passes times) launch 0 decodes every subsequence from the state (its first bit, block 0, DC due)
//                  to the first symbol boundary at or behind its end and keeps entry, exit and the blocks completed. Then,
//                  and in every later launch, a workgroup iterates over its 256 subsequences, at most HD_INNER = 32 times
//                  between barriers and until none changes: a thread whose predecessor's exit (of the iteration before, in
//                  LDS) differs from the entry it last used decodes again from there. Thread 0 of a workgroup takes the
//                  last exit of the workgroup before it as the launch before left it (two slots per workgroup, used in
//                  turn), subsequence 0 the true start. p launches carry a state over 32 (p - 1) + 2 subsequences at least;
//   jpeg_hd_scan   one workgroup per image. Verify: the image is synchronised if and only if every entry equals its
//                  predecessor's exit in the final states - by induction from subsequence 0 every entry is then the true
//                  decoder's. Otherwise its status is PP_ERR_UNSUPPORTED, "not synchronised", and nothing below decodes
//                  it. Scan: exclusive prefix sums of the block counts give every subsequence its first block;
//   jpeg_hd_zero   zeroes coef[0, 64 blocks);
//   jpeg_hd_write  every thread decodes its subsequence a last time from its (true) entry and stores every coefficient
//                  at its natural position of its block; DC values are stored as differences. Decoding stops behind the
//                  image's last block, whose end position is kept. What no valid stream holds flags the image;
//   jpeg_hd_dc     one workgroup per image: inclusive prefix sums of the DC differences of each component over its blocks in
//                  scan order, in place (the host's int32 predictor truncated to int16; a value outside int16 flags the
//                  image as it makes the host refuse it); then the result slot.
// The status equals the host's verdict: PP_OK only if the chain is proven, all blocks were decoded from real bits, fewer
// than 8 bits are left in front of the EOI marker and nothing was flagged. More blocks than the image holds cannot be
// told by their count (the padding of the last byte may decode to anything), so the count only proves too few; too many
// show as data behind the last block.
// A restart interval (pp_jpeg_hd_desc.restart_interval > 0) adds no launch. An RSTn marker is plain in the raw bytes, and a
// decoder that reaches one leaves it in the true decoder's state (the byte behind it, block 0, DC due) whatever its entry
// was (pp_jpeg_huffdec_core.h): markers are hard synchronisation points inside the same passes, and a subsequence behind
// a marker of its workgroup is true after the speculative launch. jpeg_hd_sync also counts the markers each subsequence
// jumps (in the upper half of its block count), jpeg_hd_scan sums them next to the blocks, so that jpeg_hd_write knows
// every marker's ordinal j and demands of it the number D0 + (j - 1) mod 8 and the block j * interval * blocks-per-MCU;
// the verdict demands ceil(mcus / interval) - 1 of them (reason 7 otherwise). jpeg_hd_dc's sums are segmented: they start
// anew where the MCU index is a multiple of the interval.
// The tables lie in LDS (random 16-bit lookups: bank conflicts among the lanes of a wave are inherent, as is their
// divergence - they decode unrelated data); the stream is read from global memory a byte at a time through the caches.
// All loops are bounded by construction: a decode makes at most 8 HD_S + 64 symbol steps, the reader supplies zeros past the
// stream, every store is checked against the size of its region. Integer maxima and ORs commute and every other store
// has one writer: the bytes are the same from launch to launch.
#include "pp_common.h"
#include "pp_jpeg_host.h"
#include "pp_jpeg_huffdec_core.h"

#include <cstdint>

namespace pp {

using namespace hd;

constexpr int HD_STRIDE_WGS = 256;  // workgroups per image of the grid-stride launch
constexpr int HD_DC_ITEMS = 8;      // blocks per thread and round of the DC prefix sums

// The image's 2 x ncomp tables from the descriptor into LDS (each workgroup keeps its own copy for its random lookups).
__device__ __forceinline__ const pp_jpeg_huff_table* tables_to_lds(const pp_jpeg_hd_desc& d, uint32_t* lds) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(d.tables);
    const int words = 2 * d.ncomp * HD_TABLE_WORDS;
    for (int i = threadIdx.x; i < words; i += blockDim.x) lds[i] = src[i];
    __syncthreads();
    return reinterpret_cast<const pp_jpeg_huff_table*>(lds);
}

__device__ __forceinline__ long long end_of(long long i, long long len) {
    const long long e = (i + 1) * HD_S;
    return e < len ? e : len;
}

// A workgroup's share of a synchronisation launch. RST: the image has a restart interval - a template argument, so that
// the code of an image without one holds no test for a marker (the kernels branch once, uniformly, per workgroup).
template <bool RST>
__device__ __forceinline__ void sync_body(const pp_jpeg_hd_desc& d, const Geometry& G, int pass, uint32_t* tab, State (*ex)[HD_WG]) {
    const Layout L = layout(d.stream_bytes, RST);
    if ((long long)blockIdx.x >= L.nwg) return;
    State* entry_g = reinterpret_cast<State*>(d.scratch + L.o_entry);
    State* exit_g = reinterpret_cast<State*>(d.scratch + L.o_exit);
    uint32_t* cnt_g = reinterpret_cast<uint32_t*>(d.scratch + L.o_cnt);
    State* bexit = reinterpret_cast<State*>(d.scratch + L.o_bexit);  // [2][nwg]
    uint32_t* open_g = reinterpret_cast<uint32_t*>(d.scratch + L.o_open);  // [nwg]: the workgroup was still changing when its launch ended
    Header* hdr = reinterpret_cast<Header*>(d.scratch);
    if (pass > 0) {
        // Nothing can change in a workgroup that came to rest and whose border state is the one its thread 0 used: it only
        // hands its last exit on (the same values for every thread: the branch is uniform).
        const long long i0 = (long long)blockIdx.x * HD_WG, i1 = i0 + HD_WG < L.nsub ? i0 + HD_WG : L.nsub;
        const State left0 = blockIdx.x == 0 ? State{0u, 0u} : bexit[(long long)((pass - 1) & 1) * L.nwg + blockIdx.x - 1];
        if (!open_g[blockIdx.x] && same(left0, entry_g[i0])) {
            if (threadIdx.x == 0) bexit[(long long)(pass & 1) * L.nwg + blockIdx.x] = exit_g[i1 - 1];
            return;
        }
    }
    const Stream st{d.stream, d.stream_bytes};
    const pp_jpeg_huff_table* T = tables_to_lds(d, tab);
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * HD_WG + tid;
    const bool live = i < L.nsub;
    State entry{0u, 0u}, exit{0u, 0u};
    uint32_t cnt = 0, unused = 0;
    bool dirty = false;
    if (live) {
        if (pass == 0) {
            entry = State{canonical(st, (uint32_t)(i * HD_S * 8)), 0u};
            CountSink c;
            exit = run_as<RST>(st, T, entry, end_of(i, st.len), G, c, unused);
            cnt = c.blocks | (c.markers << 16);
        } else {
            entry = entry_g[i];
            exit = exit_g[i];
            cnt = cnt_g[i];
        }
    }
    if (pass == 0 && i == 0) {
        hdr->passes = 0;
        hdr->flags = 0;
        hdr->synced = 0;
        hdr->total = 0;
        hdr->endpos = 0xFFFFFFFFu;
        hdr->done = 0;
    }
    // what thread 0 takes for its predecessor's exit: the true start, or the border state the launch before left
    State left = entry;
    if (tid == 0 && live) {
        if (i == 0) left = State{0u, 0u};
        else if (pass > 0) left = bexit[(long long)((pass - 1) & 1) * L.nwg + blockIdx.x - 1];
    }
    ex[0][tid] = exit;
    __syncthreads();
    bool open = false;
    for (int it = 0; it < HD_INNER; ++it) {
        const int cur = it & 1;
        const State want = tid == 0 ? left : ex[cur][tid - 1];
        const bool redo = live && !same(want, entry);
        if (redo) {
            entry = want;
            CountSink c;
            exit = run_as<RST>(st, T, entry, end_of(i, st.len), G, c, unused);
            cnt = c.blocks | (c.markers << 16);
            dirty = true;
        }
        ex[cur ^ 1][tid] = exit;
        open = __syncthreads_or(redo ? 1 : 0) != 0;
        if (!open) break;
    }
    if (tid == 0) open_g[blockIdx.x] = open ? 1u : 0u;
    if (live) {
        entry_g[i] = entry;
        exit_g[i] = exit;
        cnt_g[i] = cnt;
        if (tid == HD_WG - 1 || i == L.nsub - 1) bexit[(long long)(pass & 1) * L.nwg + blockIdx.x] = exit;
        if (dirty && pass > 0) atomicMax(&hdr->passes, (uint32_t)pass);
    }
}

// blockIdx.y: image; blockIdx.x: HD_WG subsequences. pass: 0 for the speculative launch.
__global__ __launch_bounds__(256) void jpeg_hd_sync_kernel(const pp_jpeg_hd_desc* __restrict__ descs, int pass) {
    __shared__ uint32_t tab[6 * HD_TABLE_WORDS];
    __shared__ State ex[2][HD_WG];
    const pp_jpeg_hd_desc d = descs[blockIdx.y];
    const Geometry G = geometry(d);
    if (!G.valid) return;
    if (G.restart) sync_body<true>(d, G, pass, tab, ex);
    else sync_body<false>(d, G, pass, tab, ex);
}

// blockIdx.x: image.
__global__ __launch_bounds__(256) void jpeg_hd_scan_kernel(const pp_jpeg_hd_desc* __restrict__ descs) {
    __shared__ uint32_t red[4];
    const pp_jpeg_hd_desc d = descs[blockIdx.x];
    const Geometry G = geometry(d);
    if (!G.valid) return;
    const Layout L = layout(d.stream_bytes, G.restart != 0);
    const State* entry_g = reinterpret_cast<const State*>(d.scratch + L.o_entry);
    const State* exit_g = reinterpret_cast<const State*>(d.scratch + L.o_exit);
    const uint32_t* cnt_g = reinterpret_cast<const uint32_t*>(d.scratch + L.o_cnt);
    uint32_t* first_g = reinterpret_cast<uint32_t*>(d.scratch + L.o_first);
    uint32_t* mfirst_g = reinterpret_cast<uint32_t*>(d.scratch + L.o_mfirst);  // (restart files only)
    uint32_t carry = 0, mcarry = 0;
    int ok = 1;
    for (long long base = 0; base < L.nsub; base += HD_WG) {
        const long long i = base + threadIdx.x;
        uint32_t v = 0;
        if (i < L.nsub) {
            v = cnt_g[i];  // blocks | markers << 16: a subsequence holds fewer than 2^16 of either
            const State want = i == 0 ? State{0u, 0u} : exit_g[i - 1];
            if (!same(want, entry_g[i])) ok = 0;
        }
        uint32_t total;
        const uint32_t before = block_scan(v & 0xFFFFu, red, total);
        if (i < L.nsub) first_g[i] = carry + before;
        carry += total;
        if (G.restart) {  // the markers the chain jumped in front of each subsequence
            const uint32_t mbefore = block_scan(v >> 16, red, total);
            if (i < L.nsub) mfirst_g[i] = mcarry + mbefore;
            mcarry += total;
        }
    }
    ok = __syncthreads_and(ok);
    if (threadIdx.x == 0) {
        Header* hdr = reinterpret_cast<Header*>(d.scratch);
        hdr->synced = ok ? 1u : 0u;
        hdr->total = carry;
        hdr->markers = mcarry;
    }
}

// blockIdx.y: image; the workgroups of a row stride over the coefficients, sixteen bytes a thread.
__global__ __launch_bounds__(256) void jpeg_hd_zero_kernel(const pp_jpeg_hd_desc* __restrict__ descs) {
    const pp_jpeg_hd_desc d = descs[blockIdx.y];
    const Geometry G = geometry(d);
    if (!G.valid) return;
    const long long quads = G.nblk * 8;  // 64 int16 a block
    uint4* q = reinterpret_cast<uint4*>(d.coef);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long long)gridDim.x * 256) q[i] = make_uint4(0u, 0u, 0u, 0u);
}

template <bool RST>
__device__ __forceinline__ void write_body(const pp_jpeg_hd_desc& d, const Geometry& G, uint32_t* tab) {
    const Layout L = layout(d.stream_bytes, RST);
    if ((long long)blockIdx.x >= L.nwg) return;
    Header* hdr = reinterpret_cast<Header*>(d.scratch);
    if (!hdr->synced) return;
    const Stream st{d.stream, d.stream_bytes};
    const pp_jpeg_huff_table* T = tables_to_lds(d, tab);
    const long long i = (long long)blockIdx.x * HD_WG + threadIdx.x;
    if (i >= L.nsub) return;
    const State entry = reinterpret_cast<const State*>(d.scratch + L.o_entry)[i];
    const long long first = reinterpret_cast<const uint32_t*>(d.scratch + L.o_first)[i];
    if (first >= G.nblk) return;  // behind the image's last block: padding
    const long long ordinal = RST ? (long long)reinterpret_cast<const uint32_t*>(d.scratch + L.o_mfirst)[i] : 0;
    WriteSink sink(d, G, first, ordinal);
    uint32_t bad = 0;
    const State out = run_as<RST>(st, T, entry, end_of(i, st.len), G, sink, bad);
    if (bad) atomicOr(&hdr->flags, bad);
    if (sink.finished) {  // (one thread per image completes its last block)
        hdr->endpos = out.pos;
        hdr->done = 1;
    }
}

// blockIdx.y: image; blockIdx.x: HD_WG subsequences.
__global__ __launch_bounds__(256) void jpeg_hd_write_kernel(const pp_jpeg_hd_desc* __restrict__ descs) {
    __shared__ uint32_t tab[6 * HD_TABLE_WORDS];
    const pp_jpeg_hd_desc d = descs[blockIdx.y];
    const Geometry G = geometry(d);
    if (!G.valid) return;
    if (G.restart) write_body<true>(d, G, tab);
    else write_body<false>(d, G, tab);
}

// Segmented prefix sums over the 256 threads of a workgroup. sum: the thread's items since its last segment start; flag: it
// holds one. Returns what the items in front of the thread's first segment start take from before the thread: the sums of
// the threads back to the last one with a flag, and `carry` (what the round before left) if there is none. last <- the same
// for the thread behind the last one.
struct SegLds {
    int32_t sum[4], flag[4];
    long long last;
};
__device__ __forceinline__ long long block_seg_scan(int32_t sum, bool flag, long long carry, SegLds& lds, long long& last) {
    int32_t s = sum, f = flag ? 1 : 0;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int32_t us = __shfl_up(s, o), uf = __shfl_up(f, o);
        if (lane_id() >= o) {
            if (!f) s += us;
            f |= uf;
        }
    }
    if (lane_id() == WAVE - 1) {
        lds.sum[wave_id()] = s;
        lds.flag[wave_id()] = f;
    }
    int32_t es = __shfl_up(s, 1), ef = __shfl_up(f, 1);  // exclusive inside the wave
    if (lane_id() == 0) es = ef = 0;
    __syncthreads();
    long long ws = 0;
    int32_t wf = 0;
#pragma unroll
    for (int w = 0; w < 3; ++w)
        if (w < wave_id()) {
            ws = lds.flag[w] ? (long long)lds.sum[w] : ws + lds.sum[w];
            wf |= lds.flag[w];
        }
    const long long before = ef ? (long long)es : es + ws + (wf ? 0ll : carry);
    if (threadIdx.x == 255) lds.last = flag ? (long long)sum : before + sum;
    __syncthreads();  // (the next call writes sum / flag behind this barrier and last behind its own first)
    last = lds.last;
    return before;
}

// blockIdx.x: image.
__global__ __launch_bounds__(256) void jpeg_hd_dc_kernel(const pp_jpeg_hd_desc* __restrict__ descs) {
    __shared__ SegLds seg;
    const pp_jpeg_hd_desc d = descs[blockIdx.x];
    const Geometry G = geometry(d);
    if (!G.valid) {
        if (threadIdx.x == 0 && d.result) *d.result = pp_jpeg_hd_result{PP_ERR_INVALID_ARG, 0, 0, HD_BAD_DESC};
        return;
    }
    const Header* hdr = reinterpret_cast<const Header*>(d.scratch);
    const bool decoded = hdr->synced != 0;
    int range_bad = 0;
    if (decoded) {
        for (int c = 0; c < d.ncomp; ++c) {
            const long long nb = c == 0 ? G.mcus * G.lum : G.mcus;
            // The predictor starts anew at every restart interval: block k of the component opens a segment where it is the
            // first of an MCU whose index is a multiple of the interval (geometry alone says so; the chain's checks have
            // proven that the markers stand there).
            const long long per = G.restart ? (long long)G.restart * (c == 0 ? G.lum : 1) : 0;  // blocks of the component per interval
            long long carry = 0;
            for (long long base = 0; base < nb; base += 256 * HD_DC_ITEMS) {
                const long long k0 = base + (long long)threadIdx.x * HD_DC_ITEMS;
                long long at[HD_DC_ITEMS];
                int32_t v[HD_DC_ITEMS];
                int32_t sum = 0;
                int opened = 0;  // items of this thread in front of its first segment start take the sums before it
#pragma unroll
                for (int j = 0; j < HD_DC_ITEMS; ++j) {
                    at[j] = k0 + j < nb ? component_block(d, G, c, k0 + j) * 64 : -1;
                    if (per && (k0 + j) % per == 0) {
                        sum = 0;
                        opened |= 1 << j;
                    }
                    if (opened) opened |= 1 << j;
                    if (at[j] >= 0 && at[j] < G.nblk * 64) sum += (int32_t)d.coef[at[j]];
                    else at[j] = -1;
                    v[j] = sum;  // inclusive inside the thread and its segment
                }
                long long last;
                const long long before = block_seg_scan(sum, opened != 0, carry, seg, last);  // (a round's sums stay far inside int32)
#pragma unroll
                for (int j = 0; j < HD_DC_ITEMS; ++j)
                    if (at[j] >= 0) {
                        const long long p = v[j] + ((opened >> j) & 1 ? 0ll : before);
                        if (p < -32768 || p > 32767) range_bad = 1;
                        d.coef[at[j]] = (int16_t)(int32_t)p;
                    }
                carry = last;
            }
        }
    }
    range_bad = __syncthreads_or(range_bad);
    if (threadIdx.x == 0) {
        *d.result = verdict(Stream{d.stream, d.stream_bytes}, G, *hdr, range_bad != 0);
    }
}

}  // namespace pp

extern "C" int pp_jpeg_scan_prepare(const void* data_host, size_t size, pp_jpeg_scan* scan) {
    const int st = pp::jpeg::scan_prepare(reinterpret_cast<const uint8_t*>(data_host), size, scan);
    if (st != PP_OK) pp::set_error("pp_jpeg_scan_prepare: %s", pp::jpeg::g_reason);
    return st;
}

extern "C" int pp_jpeg_scan_prepare_restart(const void* data_host, size_t size, pp_jpeg_scan* scan) {
    const int st = pp::jpeg::scan_prepare(reinterpret_cast<const uint8_t*>(data_host), size, scan, true);
    if (st != PP_OK) pp::set_error("pp_jpeg_scan_prepare_restart: %s", pp::jpeg::g_reason);
    return st;
}

extern "C" long long pp_jpeg_huffman_scratch_bytes(const pp_jpeg_info* infos_host, const long long* stream_bytes_host, int n) {
    if (!infos_host || !stream_bytes_host || n < 0) {
        pp::set_error("pp_jpeg_huffman_scratch_bytes: bad argument");
        return PP_ERR_INVALID_ARG;
    }
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        if (!infos_host[i].supported || stream_bytes_host[i] < 0 || stream_bytes_host[i] >= pp::hd::HD_MAX_STREAM) {
            pp::set_error("pp_jpeg_huffman_scratch_bytes: entry %d describes no supported file or a segment of 2^28 bytes or more", i);
            return PP_ERR_INVALID_ARG;
        }
        total += pp::hd::layout(stream_bytes_host[i], infos_host[i].restart_interval != 0).total;
    }
    return total;
}

extern "C" int pp_jpeg_huffman_decode_batch(const pp_jpeg_hd_desc* descriptors, int n, long long max_stream_bytes, long long max_blocks,
                                            int sync_passes, void* stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0, PP_ERR_INVALID_ARG, "pp_jpeg_huffman_decode_batch: n < 0");
    if (n == 0) return PP_OK;
    PP_REQUIRE(descriptors, PP_ERR_INVALID_ARG, "pp_jpeg_huffman_decode_batch: NULL argument");
    PP_REQUIRE(max_blocks > 0 && max_stream_bytes >= 0, PP_ERR_INVALID_ARG, "pp_jpeg_huffman_decode_batch: bad shape");
    PP_REQUIRE(n <= 65535 && max_blocks <= 3ll * 8192 * 8192 && max_stream_bytes < HD_MAX_STREAM, PP_ERR_INVALID_ARG,
               "pp_jpeg_huffman_decode_batch: at most 65535 images of sides up to 65535 and segments below 2^28 bytes");
    PP_REQUIRE(sync_passes >= 1 && sync_passes <= HD_MAX_PASSES, PP_ERR_INVALID_ARG, "pp_jpeg_huffman_decode_batch: sync_passes outside 1..64");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const Layout L = layout(max_stream_bytes);
    const dim3 per_sub((unsigned)L.nwg, n), per_image(n), tpb(256);
    const long long quads = (max_blocks * 8 + 255) / 256;
    const dim3 zero_grid((unsigned)(quads < HD_STRIDE_WGS ? quads : HD_STRIDE_WGS), n);
    for (int pass = 0; pass < sync_passes; ++pass) {
        hipLaunchKernelGGL(jpeg_hd_sync_kernel, per_sub, tpb, 0, s, descriptors, pass);
        PP_LAUNCH_CHECK_AS("jpeg_hd_sync");
    }
    hipLaunchKernelGGL(jpeg_hd_scan_kernel, per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_hd_scan");
    hipLaunchKernelGGL(jpeg_hd_zero_kernel, zero_grid, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_hd_zero");
    hipLaunchKernelGGL(jpeg_hd_write_kernel, per_sub, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_hd_write");
    hipLaunchKernelGGL(jpeg_hd_dc_kernel, per_image, tpb, 0, s, descriptors);
    PP_LAUNCH_CHECK_AS("jpeg_hd_dc");
    return PP_OK;
}
