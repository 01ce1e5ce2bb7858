/*
 * probpose_mi355x.h -- C ABI of libprobpose_mi355x.so
 *
 * MI355X (gfx950 / CDNA4) implementation of the ProbPose top-down inference hot path:
 * ViT backbone forward -> ProbMapHead (deconv heatmap branch + Sparsemax, four scalar
 * towers, flip-test averaging) -> ProbMap decode (OKS-kernel convolution, argmax,
 * sub-pixel step). Each entry point replaces one stage of the reference's Python path;
 * the reference line range it stands in for is cited above the declaration (paths are
 * relative to the reference tree, MiraPurkrabek/ProbPose_code).
 *
 * Conventions:
 *   - plain C: raw device pointers + explicit sizes, no framework types;
 *   - every function returns an int status: PP_OK (0) or a negative PP_ERR_* code;
 *     pp_last_error() gives the thread-local message of the last failure;
 *   - the library never allocates or frees device memory, never synchronises the
 *     stream and never throws; outputs and workspaces are caller-allocated;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); kernels are
 *     enqueued on it and the call returns immediately;
 *   - all pointers are DEVICE pointers unless the parameter is named *_host.
 */
#ifndef PROBPOSE_MI355X_H_
#define PROBPOSE_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 (later, additive): + pp_relu_operand, pp_taps_upsample4_conv3x3 (the ViTPose "-simple" head, csrc/pp_simple_head.hip).
 * 4 (round 6): + pp_warp_affine_u8_batch (additive); + pp_parea_scratch_bytes, pp_parea_thresholds, pp_parea_compose, pp_draw_poses, pp_resize_bilinear_u8 (the --draw-heatmap
 *    picture, csrc/pp_render.hip; added later under the same version: purely additive); + pp_render_batch_scratch_bytes, pp_render_samples_batch (the pictures of a batch of samples in one
 *    set of launches, csrc/pp_render_batch.hip; additive); the numeric domain of PP_PREC_F16X3 stated and guarded (below); power-of-two WEIGHT SCALES: + pp_gemm_ws, pp_linear_ln_folded_ws,
 *    pp_qkv_attention_split_ws, pp_gemm_residual_layernorm_ws, pp_ffn_split_residual_layernorm_ws, pp_proj_ffn_split_residual_layernorm_ws (the unsuffixed entry points = scale 1);
 *    CHANGED signatures: pp_qkv_attention_split_folded (centered rows, no column sums, + w_inv_scale), pp_proj_ffn_split_folded (+ residual_stats,
 *    + three weight scales; the rows it leaves are centered); pp_probmap_decode_flags writes NaN results for a map with a non-finite logit;
 *    + pp_skinny_linear / pp_skinny_linear_tile / pp_skinny_deconv / pp_skinny_conv1x1_planar (the launch plan of small batches); REMOVED: the eight-wave feed-forward kernel, the overlapped-epilogue Linear kernel and the
 *    head-pair qkv + attention kernel with their options "ffn_dma_waves" / "linear_ovl" / "qkv_attn_pair".
 * 3: + pp_launch_count / pp_reset_launch_counts (diagnostics: which kernels a launch plan really ran); pp_linear_ln_folded, the *_folded launches
 *    and PP_WS_LN_STATS (round 5).
 * 2: + pp_clock_probe, pp_conv3x3_splitk_slices, pp_conv3x3_winograd_maxpool_relu, pp_winograd_scratch_bytes, pp_probmap_decode_flags, option "ksplit9_below"; PP_WS_TOWER_PARTIAL sized for the slice count the
 *    library itself picks (round 3 added pp_workspace_bytes / pp_set_option / the split-fp16 layer kernels under version 1). */
#define PP_ABI_VERSION 4

/* NUMERIC DOMAIN of PP_PREC_F16X3 (the parity mode: every parity figure of the repo is taken in it).
 * An operand x is carried as hi = fp16(x), lo = fp16(x - hi) (csrc/pp_split.h); a product is three fp16 MFMAs with fp32 accumulation.
 *   range      |x| <= 65504 for EVERY MFMA operand: activations (LayerNorm outputs, q / k / v, the FFN's hidden activation, features, deconvolution
 *              maps) and - since the LayerNorm fold - the residual rows themselves (centered per row in the ViT-S chain, raw in ViT-B's
 *              pp_linear_ln_folded plan). Beyond it hi = inf, the product NaN: it reaches the heatmap logits as NaN / inf, pp_probmap_decode_flags
 *              then writes NaN keypoints / scores (never "pixel 0 with a score"), and the host mirror raises FloatingPointError.
 *              The same holds in the four scalar towers (features, every stage's pooled output): their pooling max and ReLU keep a NaN
 *              (pp_maxpool_relu_nhwc, pp_sum_maxpool_relu_nhwc, the pooled epilogues of pp_conv3x3_winograd_maxpool_relu and
 *              pp_conv3x3_maxpool_relu, pp_tower_final's error tower), so an overflowing tower yields NaN scalars for its crops - never a
 *              window pooled to a clean 0 - and the record check of the host mirror raises. (PP_PREC_BF16 has fp32's range; its halo-pooled
 *              epilogue keeps a NaN too, its ReLU epilogues of pp_conv_gemm do not.)
 *   precision  hi + lo has 22 significant bits while lo is a NORMAL fp16 number: |x| >= 2^-3. Below that lo is subnormal and the pair is exact
 *              to an ABSOLUTE 2^-25 only (no bits at all below 2^-25). Harmless for activations next to O(1) neighbours, fatal for weights,
 *              which are small numbers throughout (trained ViT weights ~ 0.02: 17 bits; rows of 1e-3: 13 bits - measured, tests/
 *              test_trained_stats.py). Linear weights are therefore stored SCALED by a power of two, the tensor's largest element in
 *              [2^12, 2^13) (probpose_code_amd/weights.py), and the kernels multiply their accumulators by the inverse (the *_ws entry points,
 *              `w_inv_scale`: exact). Elements down to 2^-16 of a tensor's largest keep all 22 bits.
 *   weights    a weight (after the BatchNorm / LayerNorm-gamma folds) with |w| > 65504 or non-finite is refused at load (weights.check_split_range).
 *   LayerNorm fold   ViT-S chain: rows travel CENTERED, the folded projection is rstd * ((x - mean) W'^T) + b' - the accuracy of a plain LayerNorm.
 *              ViT-B plan (pp_linear_ln_folded): rstd * (x W'^T - mean * colsum) + b' on raw rows loses ~ log2(1 + |mean| / std) bits of the fp32
 *              accumulator: 2 - 5e-6 relative at |mean| / std <= 1 (a trained ViT's rows), 3e-5 at 10, 5e-4 at 150; engine plan ln_fold=False
 *              applies the LayerNorm before the split instead.
 *   diagnosis  probpose_code_amd.domain_report(state_dict, crops, heads) runs a checkpoint once in fp32 and reports every operand's range and the
 *              rows' |mean| / std per layer.
 * PP_PREC_F32 has fp32's range and no such limits (16x slower MFMA); PP_PREC_BF16 has fp32's range and 8 bits. */

enum {
    PP_OK = 0,
    PP_ERR_INVALID_ARG = -1, /* NULL pointer, non-positive size, inconsistent shapes        */
    PP_ERR_UNSUPPORTED = -2, /* shape / option outside what the kernels were built for      */
    PP_ERR_HIP = -3,         /* a HIP runtime call failed (message has hipGetErrorString)   */
    PP_ERR_WORKSPACE = -4    /* caller-provided workspace too small                          */
};

/* Largest OKS-kernel radius the decode kernels support (reference clips the kernel
 * variance to 3.0 => radius ceil(3*3.0) = 9, post_processing.py:23-24). */
#define PP_MAX_RADIUS 9
#define PP_MAX_TAPS (2 * PP_MAX_RADIUS + 1)

int pp_abi_version(void);
const char* pp_last_error(void);
const char* pp_status_string(int status);

/* Number of compute units of the current device (for callers sizing batches); <0 on error. */
int pp_device_cu_count(void);

/* A HIP stream of the caller's own (non-blocking), and its end. For hosts that fork work to a second stream INSIDE a stream capture: on ROCm 7.0 a
 * stream that took part in a capture whose graph has since been destroyed must not be forked to in a later capture (the first launch of the new
 * graph crashes inside hipGraphLaunch) - a stream per captured graph, destroyed with it, is the safe pattern (probpose_code_amd/engine.py, capture). */
int pp_stream_create(void** stream_out);
int pp_stream_destroy(void* stream);

/* Explicit process-wide options. The library NEVER reads the environment: kernel selection depends only on the arguments of a
 * call and on these switches, which exist for A/B timing and default to the shipped plan:
 *   "panel" (1)              0: every GEMM / convolution on the 128 x 128-tile kernel
 *   "conv_halo" (1)          0: first tower convolution (bf16) on the implicit-GEMM kernel
 *   "psplit_nst" (0)         2 / 3: force the two- / three-stage form of the wide-tile split kernel
 *   "panel_linear_mink" (0)  > 0: shortest K of a bf16 Linear layer that takes the wide-tile kernel
 *   "psplit_bf16_conv" (0)   1: bf16 convolutions through the split kernel's bf16 instantiation
 *   "psplit_tap_inner" (1)          K walk of the gathered split-fp16 convolutions: 1 = 3x3 convolutions channel-block-major
 *                                   (the nine shifted re-reads of a block hit L2), 2 = deconvolutions too, 0 = tap-major
 *   "psplit_conv_weight_major" (1)  tiles of those 3x3 convolutions weight-set-major (with taps inner only): half the HBM-side fetch
 *   "attn_dma" (1)           0: split-fp16 attention of 432-token sequences with the register-staged kernel
 *   "conv_pool_split" (1)    0: split-fp16 first tower stage as two launches (conv, then pooling)
 *   "decode_wgs_per_cu" (3)  pp_probmap_(head_)decode: workgroups per CU its LDS band buffer is sized for (5 .. 1)
 *   "ksplit9_below" (1024)   pp_conv3x3_splitk_slices: output rows under which a small tower stage is cut into nine K-slices
 *   "linear_dma" (1)         0: large split-fp16 Linear layers (pp_gemm, N % 192 == 0, >= 512 tiles) stay on the wide-tile kernel instead of the
 *                            twelve-wave 192 x 192 kernel (pp_linear_dma.hip: eight computing + four DMA-only waves)
 *   "linear_loop" (1)        twelve-wave Linear kernel: one workgroup per CU walks a column of tiles, the next tile's first stages requested
 *                            under this tile's epilogue; 0: a workgroup per tile
 *   "psplit_deconv_weight_major" (0)  dev A/B: 1 = deconvolution tiles weight-set(phase)-major per XCD instead of row panel -> phase
 *   "ffn_pair" (1)           twelve-wave feed-forward launch: hidden chunks in pairs that share every streamed x k-block (x rows streamed 6 instead of 12
 *                            times per launch; taken when F / 128 is even); 0: one chunk at a time
 *   "psplit_tail" (1)        0: split-fp16 Linear layers never send the rows of a ragged last round to a second launch on 128 x 192 tiles
 *   "wino_order" (8)         pp_conv3x3_winograd_maxpool_relu: column tiles per 32-workgroup super tile (0: column tiles fastest)
 *   "qkv_attn_deep" (1)      pp_qkv_attention_split(_ws) of a small launch (<= 2 workgroups per CU): ring of four stages, one workgroup per CU (0: always two stages)
 *   "qkv_attn_qsplit" (1)    ... and while 2 x sequences x heads <= 0.8 x CUs: two workgroups per (sequence, head), each attends for half of the query tiles
 *   "skinny_tile" (0)        pp_skinny_linear: 10 RT + CT (11, 22, 33, 13, 12, 23) forces a tile of 32 RT rows x 32 CT columns (0: the cost rule of pp_skinny.hip)
 *   "skinny_xcd_order" (1)   pp_skinny_linear launches with a LayerNorm tail and >= 2 048 rows: tiles ordered so that an XCD touches 1 / xr of the row
 *                            blocks and 1 / xc of the column tiles (xr xc = 8; 0: row-major)
 *   "ksplit_channels" (1)    pp_conv3x3_splitk_slices: 0 = whole-tap slices only (never the four channel ranges of the wide-tile kernel)
 * Unknown names return PP_ERR_INVALID_ARG. Not thread-safe against concurrent launches (set them before the first call).
 * (probpose_code_amd/_lib.py forwards PP_OPT_<NAME>=<int> environment variables here at import - host-side convenience.) */
int pp_set_option(const char* name, int value);
int pp_get_option(const char* name, int* value);

/* Diagnostics: kernel launches since the last reset, tallied on the host at launch time (a captured hipGraph counts once, at capture) under
 * the launching source file's name - "pp_winograd.hip", "pp_ffn_dma.hip", "pp_qkv_attn_split.hip", "pp_linear_dma.hip", "pp_gemm.hip" ... - and
 * for kernels that share a file under their own tag: "linear_dma_tile" (twelve-wave Linear kernel under pp_gemm), "linear_dma_fold" (the same
 * kernel under pp_linear_ln_folded), "ffn_dma_pair" / "ffn_dma_single" / "ffn_dma_fold" (the twelve-wave feed-forward launch in its
 * paired-chunk / one-chunk form / under pp_proj_ffn_split_folded), "winograd_input_transform", "winograd_gemm_pool", "layernorm". Lets a test
 * assert WHICH kernels a launch plan ran (the reference has no counterpart: kernel selection there is cuDNN's, mmpose/models/heads/
 * hybrid_heads/probmap_head.py:261-294 and mmpretrain's VisionTransformer only name the layers). Unknown (and NULL) names count 0. Thread-safe (a mutex around the tally). */
long long pp_launch_count(const char* kernel);
int pp_reset_launch_counts(void);

/* Bytes of the caller-allocated buffers of one step of the launch plan (the library never allocates). `shape`
 * describes the step: prec = PP_PREC_*; n_img = crops x flip passes; n_tokens per image; embed / ffn widths; patch_k = 3 * patch
 * * patch; feat_h x feat_w = the backbone's output grid; heat_h x heat_w = the heatmap; deconv_channels = channels of the
 * deconvolution outputs. `buffer` = PP_WS_*; `index` selects the deconvolution (PP_WS_DECONV: 0, 1 ...) or the tower stage
 * (PP_WS_TOWER*: 0..2), 0 otherwise. Operand-format buffers are 2 bytes per element in PP_PREC_BF16 and 4 in PP_PREC_F32 /
 * PP_PREC_F16X3 (the split format is a 4-byte container). Returns < 0 (PP_ERR_INVALID_ARG) for an unknown buffer / bad shape. */
typedef struct {
    int prec, n_img, n_tokens, embed, ffn, patch_k, n_keypoints, feat_h, feat_w, heat_h, heat_w, deconv_channels;
} pp_plan_shape;
enum {
    PP_WS_PATCHES = 0,       /* (M, patch_k) operand format: im2col of the preprocessed crops, M = n_img * n_tokens        */
    PP_WS_X = 1,             /* (M, embed) fp32: the residual stream                                                       */
    PP_WS_H = 2,             /* (M, embed) operand format: LayerNorm output feeding qkv                                    */
    PP_WS_QKV = 3,           /* (M, 3 embed) operand format (unfused qkv + attention only)                                 */
    PP_WS_ATT = 4,           /* (M, embed) operand format: attention output of pp_qkv_attention_split                      */
    PP_WS_LN2 = 5,           /* (M, embed) operand format: ln2 rows parked by pp_proj_ffn_split_residual_layernorm         */
    PP_WS_FFN = 6,           /* (M, ffn) operand format: hidden activation (unfused FFN only)                              */
    PP_WS_FEAT = 7,          /* (M, embed) operand format: final LayerNorm = NHWC feature map                              */
    PP_WS_LOGITS = 8,        /* (n_img, K, heat_h * heat_w) fp32                                                           */
    PP_WS_DECONV = 9,        /* output of deconvolution `index`, NHWC operand format                                       */
    PP_WS_TOWER = 10,        /* (4, n_img, h, w, embed) operand format: convolution output of tower stage `index`         */
    PP_WS_TOWER_PARTIAL = 11,/* (slices, 4, n_img, h, w, embed) fp32: split-K partial sums of tower stage `index`, slices =
                              * pp_conv3x3_splitk_slices(prec, n_img, h, w, embed, embed, 4)                                                    */
    PP_WS_TOWER_POOLED = 12, /* (4, n_img, h / ph, w / pw, embed) operand format: pooled output of tower stage `index`     */
    PP_WS_WINOGRAD = 13,     /* pp_conv3x3_winograd_maxpool_relu's scratch for the first tower stage (pp_winograd_scratch_bytes)  */
    PP_WS_LN_STATS = 14      /* (n_img * n_tokens, embed / 96, 2) fp32: row statistics between two pp_linear_ln_folded launches   */
};
long long pp_workspace_bytes(int buffer, int index, const pp_plan_shape* shape);

/* K-slices of pp_conv3x3_splitk for a small tower stage (probmap_head.py:261-294, the 4 x 4 and 2 x 2 stages; `groups` = the four
 * towers): 3 = one kernel row of taps per slice, 9 = one tap per slice when the stage has fewer than option "ksplit9_below" output
 * rows B * H * W (too few tiles to fill the chip otherwise); 4 = four CHANNEL ranges (all nine taps each) on the split-fp16
 * wide-tile kernel, when the stage has enough rows for its 256 x 192 tiles to fill the chip (PP_PREC_F16X3, Cin % 128 == 0,
 * Cout % 192 == 0; option "ksplit_channels"). The caller passes this count to pp_conv3x3_splitk / pp_sum_maxpool_relu_nhwc;
 * PP_WS_TOWER_PARTIAL is sized for it. */
int pp_conv3x3_splitk_slices(int prec, int B, int H, int W, int Cin, int Cout, int groups);

/* Measurement aid (bench hygiene, no reference counterpart): one wavefront that sleeps on `stream` until *stop_flag becomes
 * non-zero (stop_flag: a word both sides can address - pinned host memory the caller sets with a plain store; NULL = no flag) or
 * `max_microseconds` (<= 5 000 000) of wall time have passed, then writes out[0] = shader-clock cycles (s_memtime) and out[1] =
 * ticks of the constant 100 MHz counter (s_memrealtime) it saw meanwhile: out[0] / out[1] * 100 = the average shader clock in
 * MHz over that window. Launched on a side stream beside a timed loop it records the clock the loop actually ran at (box-to-box
 * spread is clock spread). `out` may be pinned host memory too. */
int pp_clock_probe(unsigned long long* out_cycles_ticks, const unsigned long long* stop_flag, unsigned int max_microseconds, void* stream);

/* ------------------------------------------------------------------------------------
 * ProbMap decode, fused with the flip-test average.
 *
 * Replaces, per batch, the reference's per-sample Python loop
 *   flip_heatmaps(...)            mmpose/models/utils/tta.py:35-39
 *   (_htm + _htm_flip) * 0.5      mmpose/models/heads/hybrid_heads/probmap_head.py:763
 *   BaseHead.decode               mmpose/models/heads/base_head.py:33-86
 *   ProbMap.decode                mmpose/codecs/probmap.py:170-220
 *   get_heatmap_expected_value    mmpose/codecs/utils/post_processing.py:308-381
 *   _get_subpixel_maximums        mmpose/codecs/utils/post_processing.py:384-430
 *
 * hm          (B,K,H,W) f32 probability maps of the un-flipped pass.
 * hm_flip     (B,K,H,W) f32 maps of the horizontally flipped pass, or NULL (no flip test).
 *             When given, the map decoded for (b,k) is
 *             (hm[b,k,y,x] + hm_flip[b,flip_indices[k],y,W-1-x]) * 0.5f.
 * flip_indices (K) i32; required iff hm_flip != NULL.
 * taps        (K, PP_MAX_TAPS) f64: row k holds the 2*radius[k]+1 normalised 1-D factors
 *             of keypoint k's OKS kernel (the 2-D kernel of post_processing.py:13-39 is the
 *             outer product of this vector with itself up to f64 rounding), rest ignored.
 * radius      (K) i32, each in [0, PP_MAX_RADIUS].
 * in_w, in_h  codec input_size; keypoints = locs / (W-1, H-1) * (in_w, in_h) in f64.
 * avg_out     optional (B,K,H,W) f32: the averaged map that was decoded (pred_fields.heatmaps).
 * conv_out    optional (B,K,H,W) f32: the OKS-convolved map (f64 accumulate, rounded once).
 * locs        (B,K,2) f32 heatmap-space (x,y) after the sub-pixel step.
 * keypoints   (B,K,2) f64 input-pixel space (what ProbMap.decode returns, probmap.py:218).
 * scores      (B,K) f32: the un-convolved map at the integer argmax (keypoints_conf).
 * ---------------------------------------------------------------------------------- */
int pp_probmap_decode(const float* hm, const float* hm_flip, const int32_t* flip_indices,
                      const double* taps, const int32_t* radius,
                      int B, int K, int H, int W, double in_w, double in_h,
                      float* avg_out, float* conv_out,
                      float* locs, double* keypoints, float* scores, void* stream);

/* Same as pp_probmap_decode but starting from the LOGITS of the head's final 1x1 conv: the
 * kernel first applies  x / temperature -> Sparsemax over the H*W pixels of each (b, k) row ->
 * * normalize -> clamp(0, 1)  (probmap_head.py:637-646; Sparsemax = PyPI `sparsemax` [3P],
 * probmap_head.py:11,251), to the row itself and -- under the flip test -- to the mirror
 * partner's row, then averages and decodes as above. Logits are read from HBM once; the
 * probability maps only leave the CU when avg_out is requested. H*W <= 12288 (both decode entry points): a larger map,
 * or one too wide for a CU's LDS (e.g. 11 x 652), is refused with PP_ERR_UNSUPPORTED before anything is launched.
 * normalize < 0 stands for the head's `normalize=None` (probmap_head.py:249: normalize_layer = Identity): no Sparsemax,
 * the map is clamp(x / temperature, 0, 1). */
int pp_probmap_head_decode(const float* logits, const float* logits_flip, const int32_t* flip_indices,
                           const double* taps, const int32_t* radius,
                           int B, int K, int H, int W, double in_w, double in_h,
                           float temperature, float normalize,
                           float* avg_out, float* conv_out,
                           float* locs, double* keypoints, float* scores, void* stream);

/* ------------------------------------------------------------------------------------
 * Operand precision of the MFMA kernels.
 *   PP_PREC_BF16: bf16 operands, fp32 accumulate (v_mfma_f32_16x16x32_bf16) -- throughput mode.
 *   PP_PREC_F32 : fp32 operands, fp32 accumulate (v_mfma_f32_16x16x4_f32, exact fp32
 *                 products) -- bit-for-bit an fp32 fmaf chain, at 1/16 of the bf16 MFMA rate.
 *   PP_PREC_F16X3: split-fp16 operands (x = hi + lo, both fp16; a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on
 *                 v_mfma_f32_16x16x32_f16, fp32 accumulate): operand error ~2^-23, fp32's own rounding step --
 *                 the mode that meets the reference's 1e-3 tolerance at MFMA fp16 rate. Operand tensors are 4 bytes
 *                 per element in blocks of 32 elements along the contiguous axis: 32 hi halves (64 B) then 32 lo
 *                 halves (64 B); every row pitch / channel count must be a multiple of 32. Host-side packing:
 *                 probpose_code_amd/weights.py::to_split.
 * Output-format flags (`out_bf16`, `h_bf16`, `in_bf16`, `feat_bf16` arguments below): PP_OUT_F32 = fp32,
 * PP_OUT_BF16 = bf16 (with PP_PREC_BF16), PP_OUT_SPLIT = split fp16 (with PP_PREC_F16X3).
 * ---------------------------------------------------------------------------------- */
enum { PP_PREC_BF16 = 0, PP_PREC_F32 = 1, PP_PREC_F16X3 = 2 };
enum { PP_OUT_F32 = 0, PP_OUT_BF16 = 1, PP_OUT_SPLIT = 2 };
enum { PP_ACT_NONE = 0, PP_ACT_GELU = 1, PP_ACT_RELU = 2 };
enum { PP_CONV3X3 = 1, PP_DECONV4X4S2 = 2 };

/* Dense layer  out[m, n] = act_fn(sum_k act[m, k] * weight[n, k] + bias[n]) + residual[r(m), n].
 *
 * Stands in for every nn.Linear of the backbone (mmpretrain VisionTransformer [3P]; call site
 * mmpose/models/pose_estimators/base.py:206, ctor args config :56-67): qkv, proj, FFN.
 * act/weight are bf16 or fp32 according to `prec`; bias and residual are fp32 (or NULL);
 * `out` is bf16 when out_bf16 != 0 else fp32. K must be a multiple of 64 (bf16) / 32 (fp32);
 * lda/ldw multiples of 8 elements; ldc a multiple of 4. act_fn: PP_ACT_GELU is the exact erf form
 * (nn.GELU()). residual may alias out (in-place residual stream); r(m) = m, or m % res_mod when
 * res_mod > 0 (a (res_mod, N) table broadcast over the batch: the ViT pos_embed added to the
 * patch-embed output). planar_P > 0 stores fp32 planes out[((m / P) * N + n) * P + m % P]
 * instead of rows: the final 1x1 conv of the heatmap branch (probmap_head.py:244-249) emits
 * (B, K, H*W) logits, the layout the Sparsemax/decode kernel streams. */
int pp_gemm(int prec, const void* act, const void* weight, const float* bias, const float* residual,
            int res_mod, void* out, int M, int N, int K, int lda, int ldw, int ldc, int act_fn,
            int out_bf16, int planar_P, void* stream);
/* ... with PP_PREC_F16X3 weights stored as W * 2^e (numeric domain above): w_inv_scale = 2^-e multiplies the sums in front of the bias. A power
 * of two in [2^-40, 2^40]; 1 for the other precisions. */
int pp_gemm_ws(int prec, const void* act, const void* weight, const float* bias, const float* residual,
               int res_mod, void* out, int M, int N, int K, int lda, int ldw, int ldc, int act_fn,
               int out_bf16, int planar_P, float w_inv_scale, void* stream);

/* Dense layer of a ViT block (PP_PREC_F16X3 operands) with the LayerNorm in FRONT of it folded into the layer and the statistics of the
 * LayerNorm BEHIND it emitted with the output rows: a block of mmpretrain's TransformerEncoderLayer [3P] (x = x + attn(ln1(x));
 * x = ffn(ln2(x)) + x; call site mmpose/models/pose_estimators/base.py:206) then runs without a LayerNorm launch and with its residual
 * stream in the operand format (the path ViT-B - BASELINE config 4 - takes; ViT-S at 192 tokens has its two-launch layer kernels).
 *   out[m, n] = act_fn(sum_k a_hat[m, k] * weight[n, k] + bias[n]) + residual[m, n]
 *   a_hat[m, :] = act[m, :]                                  without ln_stats
 *               = (act[m, :] - mean[m]) * rstd[m]            with ln_stats: evaluated as rstd * (sum_k act weight - mean * ln_colsum[n]);
 *                 the CALLER folds the affine part into the layer: weight[n, k] = W[n, k] * gamma[k], ln_colsum[n] = sum_k weight[n, k]
 *                 (of the split-rounded weights), bias[n] = b[n] + sum_k W[n, k] * beta[k] (probpose_code_amd/weights.py::fold_layernorm)
 * ln_stats : (M, K / 96, 2) fp32, per row and 96-column part (mean, sum of squared deviations from it) of the act rows - what the layer
 *            that PRODUCED those rows left in its stats_out (its N = this K); mean / rstd (biased variance + ln_eps, as nn.LayerNorm)
 *            are combined from the parts here. K % 192 == 0.
 * stats_out: (M, N / 96, 2) fp32 or NULL: the same statistics of the OUTPUT rows (after activation and residual).
 * residual : NULL, fp32 rows (residual_format PP_OUT_F32) or operand-format rows (PP_OUT_SPLIT: hi + lo, 22 significant bits; may alias
 *            out - the residual stream updated in place). out_format PP_OUT_SPLIT or PP_OUT_F32. act must not alias out.
 * Shapes: K % 32 == 0, K >= 64, N % 192 == 0 (192 x 192 tiles, twelve-wave kernel of pp_linear_dma.hip); ln_stats excludes residual and
 * stats_out (the block has no such layer: qkv / fc1 take statistics, proj / fc2 make them); PP_ERR_UNSUPPORTED otherwise.
 * pp_linear_ln_folded_supported: 0 = shape not served, 1 = served, 2 = served with at least two rounds of tiles on the chip (the size from
 * which pp_gemm itself picks this kernel; callers use the folded plan from there and pp_gemm + pp_layernorm below). */
int pp_linear_ln_folded(const void* act, const void* weight, const float* bias, const void* residual, int residual_format,
                        void* out, int out_format, int M, int N, int K, int act_fn, const float* ln_stats,
                        const float* ln_colsum, float ln_eps, float* stats_out, void* stream);
/* ... with the weights stored as W' * 2^e (ln_colsum then sums the STORED weights): w_inv_scale = 2^-e. */
int pp_linear_ln_folded_ws(const void* act, const void* weight, const float* bias, const void* residual, int residual_format,
                           void* out, int out_format, int M, int N, int K, int act_fn, const float* ln_stats,
                           const float* ln_colsum, float ln_eps, float* stats_out, float w_inv_scale, void* stream);
int pp_linear_ln_folded_supported(int M, int N, int K, int with_ln_stats);

/* Dense layer of a SMALL batch (PP_PREC_F16X3), column-parallel: the launch plan of the one-image / few-person callers
 * (mmpose/apis/inference.py:161-196: one batch per image, B = number of boxes; demo/image_demo.py:36-61: one crop;
 * demo/topdown_demo_with_mmdet.py:35-41), where the layer kernels of the headline plan - 96 complete rows per workgroup, the layer's whole weight
 * set streamed through each - would run 4 workgroups on 256 CUs:
 *   out[m, n] = act_fn((sum_k act[m, k] weight[n, k]) * w_inv_scale + bias[n]) + residual[r(m), n]
 *   ln_out[m, :] = LayerNorm(out[m, :]; ln_gamma, ln_beta, ln_eps)                       when ln_out != NULL
 * act (M, K), weight (N, K) PP_OUT_SPLIT; bias fp32 or NULL; residual fp32 (M, N) - it may be `out` (fp32), the residual stream updated in place -
 * or a (res_mod, N) table (r(m) = m % res_mod: pos_embed) or NULL; out fp32 or PP_OUT_SPLIT. Tiles of 32 / 64 / 96 rows x 32 / 64 / 96 columns, the
 * shape a measured cost rule prices cheapest (rounds of one workgroup per CU x the time of a round + the LayerNorm tail of its row block;
 * pp_skinny_linear_tile returns rows * 1000 + columns). N % 32 == 0, K % 64 == 0.
 * The LayerNorm tail needs no second launch and no grid barrier: the workgroup that stores the LAST tile of a row block (a counter per block in
 * ln_counters: ceil(M / 32) int32, zero before the first launch, left at zero) normalises the block's rows - out must be fp32 then, N <= 1024, and
 * ln_out (M, N) PP_OUT_SPLIT distinct from out and act. The result does not depend on which workgroup arrives last.
 * Stands in for attn.proj / ffn.layers.0.0 / ffn.layers.1 of mmpretrain's TransformerEncoderLayer [3P] and the patch-embed projection (call site
 * mmpose/models/pose_estimators/base.py:206) at small M. */
int pp_skinny_linear(const void* act, const void* weight, const float* bias, const float* residual, int res_mod, void* out, int out_format,
                     int M, int N, int K, int act_fn, float w_inv_scale, const float* ln_gamma, const float* ln_beta, float ln_eps,
                     void* ln_out, int* ln_counters, void* stream);
int pp_skinny_linear_tile(int M, int N, int K, int with_layernorm);
/* 1x1 convolution to a few channels, planar fp32 out, of a SMALL batch on pp_skinny_linear's 32 x 32 tiles (the final layer of the heatmap branch,
 * mmpose/models/heads/hybrid_heads/probmap_head.py:244-249, 471-472): out[i, c, p] = sum_k act[i * P + p, k] weight[c, k] * w_inv_scale + bias[c],
 * c < n_valid. act (n_img * P, K) PP_OUT_SPLIT (an NHWC map); weight_padded (32 * ceil(n_valid / 32), K) PP_OUT_SPLIT with ZERO rows past n_valid,
 * bias_padded of the same padded length; out fp32 (n_img, n_valid, P). K % 64 == 0. */
int pp_skinny_conv1x1_planar(const void* act, const void* weight_padded, const float* bias_padded, float* out, int n_img, int P, int K,
                             int n_valid, float w_inv_scale, void* stream);
/* ConvTranspose2d(Cin -> Cout, k4, s2, p1, bias=False) + folded BatchNorm + ReLU of a SMALL batch (mmpose/models/heads/hybrid_heads/
 * probmap_head.py:435-472): act_nhwc (B, H, W, Cin), out_nhwc (B, 2H, 2W, Cout) PP_OUT_SPLIT; weight / bias as PP_DECONV4X4S2 of pp_conv_gemm
 * with py < 0 (four phase matrices (Cout, 4 Cin), BatchNorm folded). The four output phases are four column-parallel GEMMs of one launch on
 * pp_skinny_linear's tiles, the taps gathered by LDS-DMA (zeros outside the map); same sums in the same order as pp_conv_gemm.
 * Cin % 32 == 0 and Cin >= 64 (a stage of two 32-channel blocks stays within one tap or steps into the next one once), Cout % 32 == 0, else
 * PP_ERR_UNSUPPORTED: pp_conv_gemm serves every other width. */
int pp_skinny_deconv(const void* act_nhwc, const void* weight, const float* bias, void* out_nhwc, int B, int H, int W, int Cin, int Cout,
                     void* stream);

/* Residual dense layer fused with the LayerNorm that follows it in the ViT block
 * (mmpretrain TransformerEncoderLayer [3P]: x = x + attn(ln1(x)); x = ffn(ln2(x)) + x; final ln1):
 *   x_out[m, :] = sum_k act[m, k] * weight[:, k] + bias + residual[r(m), :]        (fp32 residual stream)
 *   h_out[m, :] = LayerNorm(x_out[m, :]; gamma, beta, eps)                          (bf16 or fp32 operand of the next GEMM)
 * One workgroup owns 96 (N = 384, ViT-S) or 112 (N = 768, ViT-B) complete rows, so the row statistics never
 * leave the CU and the separate LayerNorm pass over the stream disappears. N must be 384 or 768; callers fall
 * back to pp_gemm + pp_layernorm otherwise. residual may alias x_out; act may alias h_out (a workgroup
 * has consumed its own rows of act before it writes them). r(m) as in pp_gemm (res_mod). */
int pp_gemm_residual_layernorm(int prec, const void* act, const void* weight, const float* bias,
                               const float* residual, int res_mod, float* x_out, const float* gamma,
                               const float* beta, float eps, void* h_out, int h_bf16, int M, int N, int K,
                               int lda, int ldw, void* stream);
/* ... with the PP_PREC_F16X3 weights stored as W * 2^e: w_inv_scale = 2^-e (residual + bias enter the accumulators times 2^e, exact). */
int pp_gemm_residual_layernorm_ws(int prec, const void* act, const void* weight, const float* bias,
                               const float* residual, int res_mod, float* x_out, const float* gamma,
                               const float* beta, float eps, void* h_out, int h_bf16, int M, int N, int K,
                               int lda, int ldw, float w_inv_scale, void* stream);

/* Whole feed-forward block of a ViT layer fused with the LayerNorm that follows it (bf16 operands):
 *   x_out = residual + GELU(h_in W1^T + b1) W2^T + b2 ;  h_out = LayerNorm(x_out; gamma, beta, eps)
 * (mmpretrain TransformerEncoderLayer.ffn [3P] = mmcv FFN: Linear(E, F) - GELU - Linear(F, E) + identity).
 * The F-wide hidden activation stays on the CU. h_in, w1 (F, E), w2 (E, F), h_out are bf16; b1, b2,
 * residual, x_out, gamma, beta fp32. E must be 384, F a multiple of 128. residual may alias x_out
 * and h_in may alias h_out. */
int pp_mlp_residual_layernorm(const void* h_in, const void* w1, const float* b1, const void* w2,
                              const float* b2, const float* residual, float* x_out, const float* gamma,
                              const float* beta, float eps, void* h_out, int M, int E, int F, void* stream);

/* Second half of a ViT layer in one launch (bf16 operands): attention output projection + residual, the LayerNorm
 * in front of the FFN, the FFN + residual, and the LayerNorm that follows the layer
 *   x1    = residual + attn Wp^T + bp ;          h  = LayerNorm(x1; gamma2, beta2, eps)
 *   x_out = x1 + GELU(h W1^T + b1) W2^T + b2 ;   h_out = LayerNorm(x_out; gamma, beta, eps)
 * (mmpretrain TransformerEncoderLayer.forward [3P]: x = x + attn(ln1(x)); x = ffn(ln2(x), identity=x), here from
 * the point where the per-head attention outputs exist; ln1 of the NEXT layer / the final norm is the trailing
 * LayerNorm). x1 and h never leave the CU. attn (M, E), wp (E, E), w1 (F, E), w2 (E, F), h_out are bf16; the
 * rest fp32. E must be 384, F a multiple of 128. residual may alias x_out.
 * With wqkv != NULL the next layer's qkv Linear (nn.Linear(E, 3E), weight (3E, E) bf16, bias fp32) is applied to
 * h_out in the same launch:  qkv_out (M, 3E) bf16 = h_out wqkv^T + bqkv ; h_out may then be NULL (not stored). */
int pp_proj_mlp_residual_layernorm(const void* attn, const void* wp, const float* bp, const float* residual,
                                   const float* gamma2, const float* beta2, const void* w1, const float* b1,
                                   const void* w2, const float* b2, float* x_out, const float* gamma,
                                   const float* beta, float eps, void* h_out, const void* wqkv, const float* bqkv,
                                   void* qkv_out, int M, int E, int F, void* stream);

/* Convolutions of ProbMapHead as implicit GEMMs on NHWC activations (no im2col buffer):
 *   PP_CONV3X3     : Conv2d(Cin->Cout, k3, s1, p1) of the scalar towers
 *                    (mmpose/models/heads/hybrid_heads/probmap_head.py:261-410);
 *                    weight[n, (ky*3+kx)*Cin + c] = w_torch[n, c, ky, kx]; out NHWC (B,H,W,Cout).
 *   PP_DECONV4X4S2 : one output phase (py, px) of ConvTranspose2d(Cin->Cout, k4, s2, p1)
 *                    (probmap_head.py:435-472): writes out[b, 2y+py, 2x+px, :] of a (B,2H,2W,Cout)
 *                    tensor; weight[n, (ty*2+tx)*Cin + c] = w_torch[c, n, 3-2ty-py, 3-2tx-px].
 *                    py < 0 runs all four phases in one launch: `weight` then holds the four phase
 *                    matrices back to back, order (py, px) = (0,0), (0,1), (1,0), (1,1).
 * BatchNorm is folded into weight/bias by the caller; act_fn applies after bias. `groups`
 * launches several independent convolutions at once (the four towers): operand g is at
 * base + g * stride_*_g elements. ldc = row stride of out in elements. Cin must be a multiple of the
 * precision's K-tile - 64 channels (bf16), 32 (fp32, split fp16): a K-tile never straddles two taps - else
 * PP_ERR_UNSUPPORTED. */
int pp_conv_gemm(int prec, int kind, const void* act_nhwc, const void* weight, const float* bias, void* out,
                 int B, int H, int W, int Cin, int Cout, int py, int px, int groups,
                 long long stride_act_g, long long stride_w_g, long long stride_out_g,
                 long long stride_bias_g, int ldc, int act_fn, int out_bf16, void* stream);

/* Multi-head self-attention of the backbone (mmpretrain MultiheadAttention [3P]:
 * softmax(q k^T * scale) v per head). qkv: (n_seq * seq_len, 3 * heads * head_dim) rows as the
 * qkv Linear emits them ([q | k | v], head-major inside each); out: (n_seq * seq_len, heads *
 * head_dim). Both bf16, fp32 or split fp16 per `prec`. Supported (seq_len, head_dim): {192, 432} x
 * {32, 64} (fp32 432 x 64 exceeds one CU's LDS) and 192 x 80 (ViT-H; all three precisions: the
 * q . k contraction runs over the head row zero-padded to 96 on chip, nothing is read or written
 * beyond a head's 80 columns). Any other shape: PP_ERR_UNSUPPORTED. */
int pp_attention(int prec, const void* qkv, void* out, int n_seq, int seq_len, int heads, int head_dim,
                 float scale, void* stream);

/* Input side of the backbone: PoseDataPreprocessor (mmpose/models/data_preprocessors/
 * data_preprocessor.py:79-104 + mmengine ImgDataPreprocessor [3P]: BGR->RGB, float, (x-mean)/std),
 * the flip-test copy `inputs.flip(-1)` (mmpose/models/pose_estimators/topdown.py:109-112) and the
 * im2col of the ViT patch-embed Conv2d(3->E, k16, s16, zero pad `pad`) in one pass.
 * img: (B, 3, H, W) CHW, uint8 (raw crops; normalised here) or -- img_is_f32 != 0 -- fp32 that is
 * already preprocessed (the reference backbone's own input contract; mean/std/bgr_to_rgb ignored).
 * patches: (passes * B * Hp * Wp, 768) bf16/fp32, row order (pass, b, py, px), column order
 * (c, i, j); pass 1 is the horizontally flipped crop.
 * mean_host / std_host: 3 floats each, HOST pointers, in output-channel (RGB) order. */
int pp_preproc_im2col(int prec, const void* img, int img_is_f32, void* patches, int B, int passes, int H,
                      int W, int patch, int pad, const float* mean_host, const float* std_host,
                      int bgr_to_rgb, void* stream);

/* LayerNorm over the last dim of an fp32 (M, E) matrix (nn.LayerNorm(E, eps) of the ViT, eps 1e-6);
 * output bf16 or fp32. E in {384, 768, 1024, 1280}. */
int pp_layernorm(const float* x, const float* gamma, const float* beta, void* y, int M, int E, float eps,
                 int out_bf16, void* stream);

/* MaxPool2d(kernel = stride = (ph, pw)) + ReLU on an NHWC tensor (the towers' pooling,
 * probmap_head.py:264,277-278): (N, H, W, C) -> (N, H/ph, W/pw, C). */
int pp_maxpool_relu_nhwc(const void* in, int in_bf16, void* out, int out_bf16, int N, int H, int W, int C,
                         int ph, int pw, void* stream);

/* First stage of the four scalar towers in one launch: Conv2d(Cin->Cout, k3, p1) + folded BN -> MaxPool2d(ph, pw) -> ReLU
 * (probmap_head.py:261-278), i.e. PP_CONV3X3 of pp_conv_gemm followed by pp_maxpool_relu_nhwc with the full-resolution
 * tensor never stored: out_pooled (groups, B, H/ph, W/pw, Cout). One launch for bf16 operands on 16x12 feature maps with
 * (4, 3) windows (the halo-staged kernel holds whole images per tile); every other shape / precision runs the two entry points
 * through scratch_full (groups, B, H, W, Cout), which may be NULL only when the fused form applies. fmt: PP_OUT_*. */
int pp_conv3x3_maxpool_relu(int prec, const void* act_nhwc, const void* weight, const float* bias, void* out_pooled,
                            void* scratch_full, int B, int H, int W, int Cin, int Cout, int ph, int pw, int groups,
                            long long stride_act_g, long long stride_w_g, long long stride_bias_g, int fmt, void* stream);

/* A whole ViT-S encoder layer in one launch (bf16 operands), from the qkv of this layer to the qkv of the next:
 *   a     = softmax(q k^T * scale) v per head                  (mmpretrain MultiheadAttention [3P], as pp_attention)
 *   x1    = residual + a Wp^T + bp ;          h  = LayerNorm(x1; gamma2, beta2, eps)
 *   x_out = x1 + GELU(h W1^T + b1) W2^T + b2 ;   h_out = LayerNorm(x_out; gamma, beta, eps)
 *   qkv_out = h_out wqkv^T + bqkv                               (when wqkv != NULL; h_out may then be NULL)
 * i.e. pp_attention followed by pp_proj_mlp_residual_layernorm with neither the attention output nor anything between
 * the two residual adds leaving the CU. qkv_in (M, 3E) bf16 row-major [q | k | v] as the qkv Linear emits it; rows
 * [s * seq_len, (s + 1) * seq_len) are sequence s. Built for E = 384, heads * 32 = E, seq_len = 192 (256x192 input);
 * other shapes take the separate entry points. qkv_out must not alias qkv_in; scale must be positive and finite. */
int pp_vit_layer(const void* qkv_in, int seq_len, int heads, float scale, const void* wp, const float* bp,
                 const float* residual, const float* gamma2, const float* beta2, const void* w1, const float* b1,
                 const void* w2, const float* b2, float* x_out, const float* gamma, const float* beta, float eps,
                 void* h_out, const void* wqkv, const float* bqkv, void* qkv_out, int M, int E, int F, void* stream);

/* Whole feed-forward block of a ViT layer fused with the LayerNorm that follows it, in the parity precision
 * (PP_PREC_F16X3: split-fp16 operands, three fp16 MFMAs per product):
 *   x_out = residual + GELU(h_in W1^T + b1) W2^T + b2 ;  h_out = LayerNorm(x_out; gamma, beta, eps)
 * (mmpretrain TransformerEncoderLayer.ffn [3P] = mmcv FFN: Linear(E, F) - GELU - Linear(F, E) + identity; call site
 * mmpose/models/pose_estimators/base.py:206, ctor args td-pm_ProbPose-small_8xb64-210e_coco-256x192.py:56-67).
 * The F-wide hidden activation stays on the CU. h_in, h_out (M, E) are PP_OUT_SPLIT tensors; b1, b2, residual, x_out,
 * gamma, beta fp32. The weights come as ONE buffer in the kernel's consumption order, produced once per layer by
 * pp_ffn_split_pack_weights from w1 (F, E) and w2 (E, F) in the split format (pp_ffn_split_packed_bytes(E, F) bytes;
 * -1 for an unsupported shape). E must be 384, F a multiple of 128. residual may alias x_out, h_in may alias h_out
 * (a workgroup has consumed its own rows before it writes them). */
long long pp_ffn_split_packed_bytes(int E, int F);
int pp_ffn_split_pack_weights(const void* w1_split, const void* w2_split, void* packed, int E, int F, void* stream);
int pp_ffn_split_residual_layernorm(const void* h_in, const void* w_packed, const float* b1, const float* b2,
                                    const float* residual, float* x_out, const float* gamma, const float* beta,
                                    float eps, void* h_out, int M, int E, int F, void* stream);
/* ... with W1 / W2 packed from tensors stored as W * 2^e: their inverse scales (powers of two). */
int pp_ffn_split_residual_layernorm_ws(const void* h_in, const void* w_packed, const float* b1, const float* b2,
                                       const float* residual, float* x_out, const float* gamma, const float* beta,
                                       float eps, void* h_out, int M, int E, int F, float w1_inv_scale, float w2_inv_scale, void* stream);

/* The first half of a ViT layer in ONE launch in the parity precision (PP_PREC_F16X3): the qkv Linear layer and the
 * multi-head self-attention behind it; the (M, 3E) qkv tensor never reaches HBM:
 *   qkv = h_in Wqkv^T + bqkv ;  out[:, head] = softmax(q_head k_head^T * scale) v_head   per sequence
 * (mmpretrain MultiheadAttention.forward [3P]: self.qkv(x).reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4), scaled dot-product
 * attention, heads concatenated; call site mmpose/models/pose_estimators/base.py:206, ctor args
 * td-pm_ProbPose-small_8xb64-210e_coco-256x192.py:56-67). One workgroup per (sequence, head). h_in, out (n_seq * seq_len, E)
 * PP_OUT_SPLIT; wqkv (3E, E) in the split format, rows [q | k | v] as mmpretrain packs them; bqkv (3E) fp32 or NULL.
 * Built for seq_len 192, head_dim 32, heads * head_dim = 384 (ViT-S at 256x192); PP_ERR_UNSUPPORTED otherwise (callers then
 * use pp_gemm + pp_attention). out must not alias h_in. */
int pp_qkv_attention_split(const void* h_in, const void* wqkv, const float* bqkv, void* out, int n_seq, int seq_len, int heads,
                           int head_dim, float scale, void* stream);
/* ... with Wqkv stored as W * 2^e: w_inv_scale = 2^-e. */
int pp_qkv_attention_split_ws(const void* h_in, const void* wqkv, const float* bqkv, void* out, int n_seq, int seq_len, int heads,
                              int head_dim, float scale, float w_inv_scale, void* stream);

/* The same launch with the LayerNorm in front of it (ln1 of the block; mmpretrain TransformerEncoderLayer [3P]: x + attn(ln1(x))) folded into the
 * projection: x_centered holds the residual rows MINUS THEIR ROW MEAN in the operand format, wqkv_folded / bqkv_folded carry gamma / beta
 * (probpose_code_amd/weights.py::fold_layernorm: W' = W gamma * 2^e, b' = b + W beta), and ln_stats holds (mean, rstd) of every row -
 * (n_seq * seq_len, 2) fp32, as pp_proj_ffn_split_folded leaves both. q / k / v are evaluated as  rstd * w_inv_scale * ((x - mean) W'^T) + b'
 * where the unfolded launch adds its bias: no  mean * colsum  correction, hence the accuracy of a LayerNorm applied before the split (ABI 3 took raw
 * rows and column sums: 2 - 5x the error at |mean| / std <= 1, a digit more per decade beyond). Same shapes and restrictions as
 * pp_qkv_attention_split. */
int pp_qkv_attention_split_folded(const void* x_centered, const void* wqkv_folded, const float* bqkv_folded, const float* ln_stats, void* out,
                                  int n_seq, int seq_len, int heads, int head_dim, float scale, float w_inv_scale, void* stream);

/* The second half of a ViT layer in ONE launch in the parity precision (PP_PREC_F16X3): attention output projection +
 * residual, ln2, the feed-forward block + residual, and the LayerNorm that follows the layer:
 *   x_mid = residual + att Wp^T + bp ;  h = LayerNorm(x_mid; gamma2, beta2, eps)
 *   x_out = x_mid + GELU(h W1^T + b1) W2^T + b2 ;  h_out = LayerNorm(x_out; gamma, beta, eps)
 * (mmpretrain TransformerEncoderLayer.forward [3P]: x = x + attn(ln1(x)); x = ffn(ln2(x), identity=x); call site
 * mmpose/models/pose_estimators/base.py:206, ctor args td-pm_ProbPose-small_8xb64-210e_coco-256x192.py:56-67).
 * x_mid and the hidden activation never leave the CU; h (the ln2 rows) passes through h_scratch (M, E; PP_OUT_SPLIT), which
 * each workgroup writes and streams back for its own 96 rows (it stays in L2) - h_scratch must not alias att or h_out.
 * att, h_out (M, E) PP_OUT_SPLIT; wproj_packed from pp_proj_split_pack_weights (Wp (E, E) in the split format;
 * pp_proj_split_packed_bytes(E) bytes, -1 if unsupported), w_packed from pp_ffn_split_pack_weights. E must be 384, F a
 * multiple of 128. residual may alias x_out, att may alias h_out. */
long long pp_proj_split_packed_bytes(int E);
int pp_proj_split_pack_weights(const void* wp_split, void* packed, int E, void* stream);
int pp_proj_ffn_split_residual_layernorm(const void* att, const void* wproj_packed, const float* bproj,
                                         const float* gamma2, const float* beta2, void* h_scratch, const void* w_packed,
                                         const float* b1, const float* b2, const float* residual, float* x_out,
                                         const float* gamma, const float* beta, float eps, void* h_out, int M, int E,
                                         int F, void* stream);
/* ... with Wp / W1 / W2 packed from tensors stored as W * 2^e: their inverse scales (powers of two). */
int pp_proj_ffn_split_residual_layernorm_ws(const void* att, const void* wproj_packed, const float* bproj,
                                            const float* gamma2, const float* beta2, void* h_scratch, const void* w_packed,
                                            const float* b1, const float* b2, const float* residual, float* x_out,
                                            const float* gamma, const float* beta, float eps, void* h_out, int M, int E,
                                            int F, float wp_inv_scale, float w1_inv_scale, float w2_inv_scale, void* stream);

/* The same launch inside a chain of layers whose ln1 is folded into the qkv projection (pp_qkv_attention_split_folded). Rows that travel between
 * the launches of the chain are CENTERED rows: x - mean(x) in the operand format, with (mean, rstd) per row beside them.
 *   residual_format PP_OUT_SPLIT: `residual` holds centered rows, residual_stats ((M, 2) fp32: mean, rstd) their means - x = (hi + lo) + mean;
 *                   PP_OUT_F32: fp32 rows (the first layer: the patch embedding's), residual_stats unused;
 *   fold_out != 0: the LayerNorm behind the FFN is NOT applied - the new rows leave ONCE, centered, in the operand format, to h_out (which may alias
 *                  `residual`), with (mean, rstd) of every row in stats_out ((M, 2) fp32; may alias residual_stats: a workgroup owns its rows);
 *                  x_out, gamma, beta are not used. A workgroup writes 288 KiB less per 96 rows (the store path is what the epilogue waits for);
 *   fold_out == 0: x_out (fp32) and h_out = LayerNorm(x_out; gamma, beta) as in the plain launch (the last layer: ln_f).
 *   w*_inv_scale:  inverse power-of-two scales of Wp / W1 / W2 (1 for unscaled weights).
 * Paired kernel only: F / 128 even - PP_ERR_UNSUPPORTED otherwise (callers keep the plain launches). Tallied as "ffn_dma_fold". */
int pp_proj_ffn_split_folded(const void* att, const void* wproj_packed, const float* bproj, const float* gamma2, const float* beta2,
                             void* h_scratch, const void* w_packed, const float* b1, const float* b2, const void* residual,
                             int residual_format, const float* residual_stats, int fold_out, float* x_out, const float* gamma,
                             const float* beta, float eps, void* h_out, float* stats_out, int M, int E, int F, float wp_inv_scale,
                             float w1_inv_scale, float w2_inv_scale, void* stream);

/* Last deconvolution of the heatmap branch fused with the 1x1 convolution that follows it (bf16 operands):
 *   ConvTranspose2d(Cin -> 256, k4, s2, p1) + BN + ReLU  ->  Conv2d(256 -> K, k1)
 * (probmap_head.py:435-472 and :244-249; reshaped to (B, K, H'W') at :627-648). weight / bias as PP_DECONV4X4S2 of
 * pp_conv_gemm with py < 0 (four phase matrices, folded BatchNorm); head_w (32, 256) bf16 = the 1x1 kernel, rows >= K
 * zero; head_b (K) fp32, K <= 28 (the kernel keeps both biases in the unused weight rows of its LDS image). The 256-channel
 * feature map is never stored. logits_phased (B, K, 4, H*W) fp32: output pixel
 * (2y + py, 2x + px) of map (b, k) sits at [b, k, 2 py + px, y W + x] - the layout pp_probmap_head_decode_phased reads.
 * Cout == 256, Cin % 64 == 0 (the kernel's stages are 64 channels of one tap) and H * W % 4 == 0, else PP_ERR_UNSUPPORTED: use
 * pp_conv_gemm + pp_gemm. */
int pp_deconv_head(const void* act_nhwc, const void* weight, const float* bias, const void* head_w, const float* head_b,
                   float* logits_phased, int B, int H, int W, int Cin, int Cout, int K, void* stream);

/* pp_deconv_head in the parity precision (PP_PREC_F16X3): act_nhwc, weight in the split format; head_w_packed = the 1x1
 * kernel (K <= 28 maps x 256 channels, zero-padded to 32 rows) as the 32 KiB register image the kernel's waves load
 * (probpose_code_amd/weights.py::pack_head_split: [column group 4][K block 2][map fragment 2][hi | lo][lane 64][8 halves]).
 * The ReLU'd tile is split in registers and contracted with it in the epilogue; same logits_phased layout. Needs
 * 4 * ceil(B H W / 192) >= 192 tiles (PP_ERR_UNSUPPORTED below that: use pp_conv_gemm + pp_gemm). */
int pp_deconv_head_split(const void* act_nhwc, const void* weight, const float* bias, const void* head_w_packed,
                         const float* head_b, float* logits_phased, int B, int H, int W, int Cin, int Cout, int K, void* stream);

/* pp_probmap_head_decode for logits in the phase-separated layout of pp_deconv_head (H, W = the heatmap size). */
int pp_probmap_head_decode_phased(const float* logits, const float* logits_flip, const int32_t* flip_indices,
                                  const double* taps, const int32_t* radius, int B, int K, int H, int W, double in_w,
                                  double in_h, float temperature, float normalize, float* avg_out, float* conv_out,
                                  float* locs, double* keypoints, float* scores, void* stream);

/* The three decode entry points above as one, with flags: PP_DECODE_LOGITS (input = logits of the final 1x1 conv: temperature,
 * Sparsemax, normalize, clamp first, as pp_probmap_head_decode; otherwise probability maps as pp_probmap_decode and temperature /
 * normalize are ignored), PP_DECODE_PHASED (logits in the phase-separated layout of pp_deconv_head), PP_DECODE_SHIFT_HEATMAP
 * (flip_heatmaps(..., shift_heatmap=True), mmpose/models/utils/tta.py:64-66: the flipped-back map is moved one pixel to the right
 * before the average - column x takes the flipped pass's column W - x, column 0 its column W - 1; ignored without a flipped pass). */
#define PP_DECODE_LOGITS 1
#define PP_DECODE_PHASED 2
#define PP_DECODE_SHIFT_HEATMAP 4
int pp_probmap_decode_flags(const float* maps, const float* maps_flip, const int32_t* flip_indices, const double* taps,
                            const int32_t* radius, int B, int K, int H, int W, double in_w, double in_h, float temperature,
                            float normalize, float* avg_out, float* conv_out, float* locs, double* keypoints, float* scores,
                            int flags, void* stream);

/* UDP heatmap decode with DARK refinement (mmpose/codecs/udp_heatmap.py:146-196, heatmap_type "gaussian": the ViTPose baseline's
 * codec), csrc/pp_udp_decode.hip; added under version 4, purely additive. maps / maps_flip / flip_indices as pp_probmap_decode_flags
 * takes them - fp32 maps (B, K, H*W) of the final 1x1 conv, row-major or (PP_DECODE_PHASED; even H and W) in the phase-separated
 * layout of pp_deconv_head, the flipped pass optional, PP_DECODE_SHIFT_HEATMAP honoured; no other flag. The average
 * (a + flip_back(b)) * 0.5 is taken in fp32; `scores` (B, K) is its maximum and `locs` (B, K, 2) the first row-major index of that
 * maximum as (x, y) - (-1, -1) where the maximum is <= 0 - both bit-equal to numpy on the same map. The map is then blurred with
 * the separable Gaussian cv2.GaussianBlur(ks, sigma 0) uses (sigma = 0.3 ((ks - 1) / 2 - 1) + 0.8, taps normalised in double and
 * rounded to fp32, fp32 sums, zero border), rescaled to its original maximum, clipped to [1e-3, 50] and logged; one Newton step
 * from the seven-point fp32 derivative / Hessian, (H + eps32 I)^+ in fp64, the result rounded to fp32 and rescaled:
 * `keypoints` (B, K, 2) f64 = loc / (W - 1, H - 1) * (in_w, in_h). A map with maximum <= 0 takes three of its seven points from the
 * map of keypoint k - 1 (K - 1 for k = 0) of the same sample, as the reference's flat index does. blur_kernel_size odd, 1 .. 19;
 * H, W >= 2, H * W <= 12288 and the two LDS images ((W + ks) H + (H + ks - 1) W floats) within 160 KiB less
 * the 256 bytes the kernel holds statically, else PP_ERR_UNSUPPORTED.
 * avg_out (optional) takes the averaged maps, row-major (B, K, H, W). A map with a non-finite value (or, for a map with maximum
 * <= 0, such a neighbour) yields NaN locs / keypoints / scores. */
int pp_udp_heatmap_decode(const float* maps, const float* maps_flip, const int32_t* flip_indices, int B, int K, int H, int W,
                          double in_w, double in_h, int blur_kernel_size, float* avg_out, float* locs, double* keypoints,
                          float* scores, int flags, void* stream);

/* The other two codecs of the reference's head x decode table (mmpose/codecs/udp_expmax_heatmap.py, argmax_probmap.py); added under
 * version 4, purely additive: no existing entry point changes.
 *
 * pp_expmax_heatmap_decode = UDPExpMaxHeatmap.decode, heatmap_type "gaussian" (udp_expmax_heatmap.py:165-206:
 * get_heatmap_expected_value, post_processing.py:308-381, then / (W - 1, H - 1) * input_size): the expected-OKS decode of
 * pp_probmap_decode on the RAW fp32 maps of the final 1x1 conv - no temperature, no Sparsemax, no clamp: values below 0 and above 1
 * pass through unchanged. A load mode of pp_probmap_decode's kernel (csrc/pp_decode.hip), the same arithmetic from the averaged map
 * on: flip-back, channel permutation and fp32 average; separable OKS-kernel convolution in fp64, one rounding to fp32; first-occurrence
 * argmax; one fp32 sub-pixel step; rescale in fp64; `scores` = the raw averaged map at the integer argmax. Row-major maps, or with
 * PP_DECODE_PHASED the phase-separated layout of pp_deconv_head (even H, W % 8 == 0); PP_DECODE_SHIFT_HEATMAP honoured; any other
 * flag is PP_ERR_INVALID_ARG. conv_out against scipy.ndimage.convolve (a raster sum over the 2-D kernel, a product and a sum per tap): both
 * are fp64 sums rounded once to fp32, and differ in fp64 by at most (d^2 + 2 d + 130) 2^-53 times the same convolution of |map|
 * (d = 2 r + 1: the two orders of summation, and the 1-D taps against the 2-D weights). On a result that does not cancel that is far
 * below half an fp32 spacing and the bits are equal; on a signed map whose result is a cancellation residue (or an exact 0.0 of
 * scipy's) conv_out is within that bound, not equal, and the argmax may move between pixels scipy ties to within it. locs,
 * keypoints and scores are always the reference's steps applied to conv_out as returned. taps / radius as pp_probmap_decode takes them; K <= 17 (the reference's table of sigmas), else
 * PP_ERR_UNSUPPORTED. Shape limits are pp_probmap_decode's. A map holding a non-finite value (in either pass) gives NaN locs /
 * keypoints / scores (and NaN avg_out / conv_out maps) for that (crop, keypoint) only. Tallied as "pp_expmax_heatmap_decode". */
int pp_expmax_heatmap_decode(const float* maps, const float* maps_flip, const int32_t* flip_indices, const double* taps,
                             const int32_t* radius, int B, int K, int H, int W, double in_w, double in_h, float* avg_out,
                             float* conv_out, float* locs, double* keypoints, float* scores, int flags, void* stream);

/* pp_argmax_probmap_decode = ProbMapHead's map construction (probmap_head.py:637-646: x / T, Sparsemax over the H*W pixels,
 * * normalize, clamp(0, 1) per pass; normalize < 0 = the head's normalize=None, as in pp_probmap_decode_flags), the flip-test
 * average, then ArgMaxProbMap.decode, heatmap_type "gaussian" (argmax_probmap.py:150-196: get_heatmap_maximum +
 * refine_keypoints_dark_udp + / (W - 1, H - 1) * input_size - the steps of UDPHeatmap.decode), csrc/pp_argmax_decode.hip. ONE
 * launch, one 256-thread workgroup per (crop, keypoint); the averaged map stays in LDS unless avg_out is given. Its results are bit
 * for bit those of pp_probmap_decode_flags(PP_DECODE_LOGITS | flags, avg_out = maps) followed by pp_udp_heatmap_decode(maps): both
 * halves are the same device code (csrc/pp_decode_stages.h). logits row-major or PP_DECODE_PHASED (even H, W % 8 == 0);
 * PP_DECODE_SHIFT_HEATMAP honoured; any other flag is PP_ERR_INVALID_ARG. W % 4 == 0, H * W <= 12288, blur_kernel_size odd,
 * 1 .. 19, and the LDS above (512 B + max(H (W + 24) + 32, 2048, (H + ks - 1) W) + H ((W + ks - 1) | 1) floats) within 160 KiB less the 256 bytes the kernel holds statically, else
 * PP_ERR_UNSUPPORTED. A non-finite logit gives NaN locs / keypoints / scores (and a NaN avg_out map) for that (crop, keypoint), and
 * for one whose map has maximum <= 0 and takes points from that neighbour (see pp_udp_heatmap_decode). Tallied as
 * "pp_argmax_probmap_decode". */
int pp_argmax_probmap_decode(const float* logits, const float* logits_flip, const int32_t* flip_indices, int B, int K, int H, int W,
                             double in_w, double in_h, float temperature, float normalize, int blur_kernel_size, float* avg_out,
                             float* locs, double* keypoints, float* scores, int flags, void* stream);

/* ------------------------------------------------------------------------------------
 * The head of the ViTPose "-simple" variants (csrc/pp_simple_head.hip): FeatureMapProcessor(scale_factor=4.0, apply_relu=True)
 * (mmpose/models/necks/fmap_proc_neck.py:52-92; resize = F.interpolate(x, None, 4.0, "bilinear", align_corners=False),
 * mmpose/models/utils/ops.py:60) in front of HeatmapHead(deconv_out_channels=[], final_layer=dict(kernel_size=3, padding=1))
 * (heatmap_head.py:198-213). Behind the ReLU everything is linear, so the 3x3 convolution runs at the backbone's resolution as nine
 * 1x1 "tap" convolutions - ONE pp_gemm_ws with the (9 K, E) tap matrix and planar_P = h * w - and the upsampling gathers from the tap
 * planes; the (n_img, 4h, 4w, E) upsampled map is never built. Three launches: pp_relu_operand, pp_gemm_ws, pp_taps_upsample4_conv3x3.
 *
 * pp_relu_operand: out = relu(in) for n_rows x row_len elements of an activation tensor in the operand format `format` (PP_OUT_F32,
 *   PP_OUT_BF16, PP_OUT_SPLIT), dense rows, row_len % 32 == 0, both buffers 16-byte aligned, out distinct from in (the input stays as it
 *   is). fp32 / bf16: an element becomes +0 unless it is > 0 or NaN. Split fp16: an element becomes (+0, +0)
 *   unless float(hi) + float(lo) > 0 or that sum is NaN. Every other element is copied bit for bit - a NaN (an out-of-range operand,
 *   "numeric domain" above) reaches the logits and the decode behind them writes NaN results. n_rows == 0 returns PP_OK at once.
 *
 * pp_taps_upsample4_conv3x3:
 *   out[i, k, Y, X] = bias[k] + sum over dy, dx in {-1, 0, 1} with 0 <= Y + dy < 4h and 0 <= X + dx < 4w
 *                               of bil(taps[i, (3 (dy + 1) + dx + 1) K + k], Y + dy, X + dx)
 *   bil(P, Y', X'): sy = max((Y' + 0.5) / 4 - 0.5, 0), y0 = floor(sy), y1 = min(y0 + 1, h - 1), ly = sy - y0; x likewise;
 *                   = (1 - ly) ((1 - lx) P[y0, x0] + lx P[y0, x1]) + ly ((1 - lx) P[y1, x0] + lx P[y1, x1])
 *   taps (n_img, 9 K, h * w) fp32: plane t K + k = tap t = 3 (dy + 1) + (dx + 1) of keypoint k WITHOUT bias - what
 *        pp_gemm_ws(act = relu'd NHWC features (n_img h w, E), weight row t K + k = W[k, :, dy + 1, dx + 1], bias = NULL, N = 9 K,
 *        planar_P = h * w) stores; bias (K) fp32; out (n_img, K, 4h * 4w) fp32, plain planar (not PP_DECODE_PHASED): what
 *        pp_udp_heatmap_decode / pp_expmax_heatmap_decode read.
 *   A tap outside the upsampled map is the convolution's zero padding: it is left out by selection (not sampled at a clamped position, not
 *   multiplied by zero). The weights ly, lx and their products are exact in fp32; the sum is fp32 in a fixed order (bit-identical from
 *   launch to launch), within 41 * 2^-24 * (|bias| + sum of weight * |tap|) of the exact value.
 *   K >= 1, h, w >= 1 (at most 2^20 each), n_img >= 0 (0 returns PP_OK at once; n_img K ceil(h / 16) ceil(w / 16) < 2^31 workgroups, else
 *   PP_ERR_UNSUPPORTED). 16-byte stores when out is 16-byte aligned, scalar ones otherwise.
 * Both are tallied under "pp_simple_head.hip" (pp_launch_count).
 * ---------------------------------------------------------------------------------- */
int pp_relu_operand(int format, const void* in, void* out, int n_rows, int row_len, void* stream);
int pp_taps_upsample4_conv3x3(const float* taps, const float* bias, float* out, int n_img, int K, int h, int w, void* stream);

/* Split-K form of the towers' 3x3 convolution for stages with few output pixels: the contraction is cut into ksplit slices -
 * 1, 3 or 9: whole taps (any precision); any other count with Cin % (32 ksplit) == 0: channel ranges [s Cin / ksplit, ...) of all nine
 * taps (PP_PREC_F16X3 on the wide-tile kernel only, needs >= 192 tiles of 256 x 192; pp_conv3x3_splitk_slices returns such a
 * count only where it applies) - every (slice, group) pair is its own set of output tiles, and the fp32 partial sums go to
 * partials (ksplit, groups, B*H*W, Cout) WITHOUT bias. Weight layout as PP_CONV3X3 of pp_conv_gemm. Followed by
 * pp_sum_maxpool_relu_nhwc, which reduces the slices, adds the (folded BatchNorm) bias, pools and applies ReLU
 * (probmap_head.py:261-294). */
int pp_conv3x3_splitk(int prec, const void* act_nhwc, const void* weight, float* partials, int B, int H, int W, int Cin,
                      int Cout, int groups, long long stride_act_g, long long stride_w_g, int ksplit, void* stream);
int pp_sum_maxpool_relu_nhwc(const float* partials, int nsplit, long long split_stride, const float* bias,
                             int images_per_group, void* out, int out_bf16, int N, int H, int W, int C, int ph, int pw,
                             void* stream);

/* First stage of the scalar towers in its Winograd F(2x2, 3x3) form (PP_PREC_F16X3 only; split-fp16 operands):
 *     Conv2d(Cin -> Cout, k3, p1) + folded BatchNorm -> MaxPool2d(pool_h, pool_w) -> ReLU      (probmap_head.py:261-294)
 * for `groups` towers that SHARE the input act_nhwc (B, H, W, Cin), in two launches: the input transform (every 4 x 4 patch ->
 * 16 planes [p][B * 48 tiles][Cin] in v_scratch, pp_winograd_scratch_bytes) and 16 position GEMMs with the output transform,
 * pooling, bias and ReLU in the epilogue - 2.25x fewer MFMAs than the implicit GEMM (pp_conv3x3_maxpool_relu), only the pooled
 * map is stored. u_packed: (groups, 16, Cout, Cin) split format, U_p = (G g G^T)_p of the BatchNorm-folded 3 x 3 weights
 * g (Cout, Cin, 3, 3), G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1], p = 4 a + b (probpose_code_amd/weights.py computes it in
 * fp64). bias (groups, Cout) fp32; out_pooled (groups, B, H / pool_h, W / pool_w, Cout) split format. Built for H % 4 == 0, W % 6 == 0
 * (16 x 12, 24 x 18), pooling (4, 3), Cin % 128 == 0, Cout % 96 == 0; anything else returns PP_ERR_UNSUPPORTED (use pp_conv3x3_maxpool_relu). */
long long pp_winograd_scratch_bytes(int B, int H, int W, int Cin);
int pp_conv3x3_winograd_maxpool_relu(const void* act_nhwc, const void* u_packed, const float* bias, void* v_scratch,
                                     void* out_pooled, int B, int H, int W, int Cin, int Cout, int pool_h, int pool_w, int groups,
                                     void* stream);

/* Last layer of the four scalar towers (Conv1x1 -> Sigmoid; ReLU for the error tower,
 * probmap_head.py:280-290,405) on the 1x1 pooled feature, fused with the flip-test average of the
 * scalars (probmap_head.py:766-774). feat: (4, passes * B, C); w: (4, K, C) fp32; bias: (4, K);
 * out: (4, B, K) fp32 in tower order probability, visibility, oks, error; the error row is divided
 * by err_div (pass 1 to keep it raw). */
int pp_tower_final(const void* feat, int feat_bf16, const float* w, const float* bias,
                   const int32_t* flip_indices, float* out, int B, int passes, int C, int K, float err_div,
                   void* stream);

/* Ex-OKS similarity of one (image, category) cell (COCOeval.computeExtendedOks,
 * mmpose/evaluation/metrics/_cocoeval.py:540-707, iouType "keypoints"; window from fix_bbox_aspect_ratio,
 * mmpose/structures/keypoint/keypoints_min_padding.py:68-133). float64 device arrays: gt_kpts (G, K, 3) = x, y, v with
 * v = 3 for keypoints outside the activation window; gt_bbox (G, 4) xywh; gt_area (G); dt_kpts (D, K, 3) = x, y, presence
 * probability, ALREADY in evaluation order (stable descending score, at most maxDets = 20); sigmas (K);
 * gt_visibilities (n_vis) int32 = the visibility value of levels 1..n_vis (level 0 is v > 0).
 * confidence_thr = NaN stands for the reference's None. out (n_vis + 1, D, G) float64. */
int pp_extended_oks(const double* gt_kpts, const double* gt_bbox, const double* gt_area, const double* dt_kpts,
                    const double* sigmas, const int* gt_visibilities, int G, int D, int K, int n_vis,
                    double confidence_thr, double padding, int use_area, int original, double* out, void* stream);

/* Result record of the multi-GPU exchange: records[i] = [x, y, conf, prob, vis, oks, err] (float64 x 7) for the n =
 * crops x keypoints outputs - keypoints (n, 2) float64, scores (n) float32 from the decode, scalars (4, n) float32 from
 * pp_tower_final. One fixed-layout all_gather of this replaces mmengine's pickled collect_results. */
int pp_pack_records(const double* keypoints, const float* scores, const float* scalars, double* records, int n, void* stream);

/* Person heatmaps back on the image, merged: out[k, y, x] = max over the n persons of cv2.warpAffine(heatmap_n[k], M_n,
 * (img_w, img_h), INTER_LINEAR) with zero border (revert_heatmap + the np.max of merge_data_samples,
 * mmpose/structures/utils.py:105-123, 146-175) in one launch. heatmaps (n, K <= 32, hm_h, hm_w) float32; inverse_maps
 * (n, 2, 3) float64 = the image -> heatmap maps (warpAffine inverts M itself); out (K, img_h, img_w) float32. */
int pp_revert_heatmaps_max(const float* heatmaps, const double* inverse_maps, float* out, int n, int K, int hm_h, int hm_w,
                           int img_h, int img_w, void* stream);

/* In place heatmaps[k] = heatmaps[k] / sum(heatmaps[k]) * presence[k] - the posterior the visualiser draws
 * (mmpose/visualization/local_visualizer.py:827-837). heatmaps (K, H, W) float32, presence (K) float32, scratch: K * 64
 * float64. */
int pp_heatmap_posterior(float* heatmaps, const float* presence, double* scratch, int K, int H, int W, void* stream);

/* pp_extended_oks for every (image, category) cell of a dataset in one launch. Instances / detections of cell c are rows
 * [cell_gt_off[c], cell_gt_off[c + 1]) / [cell_dt_off[c], cell_dt_off[c + 1]) of the flat arrays (detections of a cell in
 * evaluation order, at most maxDets); its (n_vis + 1, Dc, Gc) float64 block is written at out + cell_out_off[c]. */
int pp_exoks_cells(const double* gt_kpts, const double* gt_bbox, const double* gt_area, const double* dt_kpts,
                   const double* sigmas, const int* gt_visibilities, const int* cell_gt_off, const int* cell_dt_off,
                   const long long* cell_out_off, int n_cells, int K, int n_vis, double confidence_thr, double padding,
                   int use_area, int original, double* out, void* stream);

/* Greedy detection <-> instance matching of every (cell, visibility level, area range) at every similarity threshold
 * (COCOeval.evaluateImg, mmpose/evaluation/metrics/_cocoeval.py:709-887, the return_matching=False branch: by similarity,
 * or by nearest box centre when match_by_bbox). ious / offsets as written by pp_exoks_cells; gt_ignore (N_gt, L) uint8 =
 * gt["ignore"][level]; gt_area (N_gt) = the area of the range test (:729-733); boxes xywh float64; area_rng (A, 2);
 * iou_thrs (T <= 64). max_gt_per_cell sizes the LDS. Outputs: dt_match (L, A, T, N_dt) int32 = row of the matched instance
 * or -1; dt_ignore (L, A, T, N_dt) uint8; gt_match (L, A, T, N_gt) int32 = row of the matching detection or -1;
 * gt_ignore_out (L, A, N_gt) uint8 = the cell's _ignore flag; sim_sum / sim_cnt (L, A, n_cells) = sum / number of the
 * similarities of the matches made over all thresholds (COCOeval.loc_similarities, :857). */
int pp_exoks_match(const double* ious, const int* cell_gt_off, const int* cell_dt_off, const long long* cell_iou_off,
                   const unsigned char* gt_ignore, const unsigned char* gt_iscrowd, const double* gt_area,
                   const double* gt_bbox, const double* dt_area, const double* dt_bbox, const double* area_rng,
                   const double* iou_thrs, int n_cells, int max_gt_per_cell, int N_gt, int N_dt, int L, int A, int T,
                   int match_by_bbox, int* dt_match, unsigned char* dt_ignore, int* gt_match,
                   unsigned char* gt_ignore_out, double* sim_sum, int* sim_cnt, void* stream);

/* Precision / recall / score tables of the dataset (COCOeval.accumulate, _cocoeval.py:889-1009; one category, one maxDets).
 * order (N_dt) int32 = np.argsort(-score, kind="mergesort") over all detections in cell order; rec_thrs (R <= 128);
 * chunk_scratch: int32 (L * A * T, ceil(N_dt / 256), 2). precision / scores (T, L, R, A) and recall (T, L, A) float64 must be
 * pre-filled with -1 by the caller: entries of rows without a counted instance are left untouched (:941-943, :955-956). */
int pp_exmap_accumulate(const int* dt_match, const unsigned char* dt_ignore, const unsigned char* gt_ignore,
                        const int* order, const double* dt_score, const double* rec_thrs, int n_cells, int N_gt, int N_dt,
                        int L, int A, int T, int R, int* chunk_scratch, double* precision, double* recall, double* scores,
                        void* stream);

/* Person crops of the top-down pipeline: n times cv2.warpAffine(img, M_i, (out_w, out_h), flags=INTER_LINEAR), zero border
 * (TopdownAffine.transform, mmpose/datasets/transforms/topdown_transforms.py:118-126), written as the CHW uint8 tensors
 * PackPoseInputs emits (mmpose/datasets/transforms/formatting.py:14-36,195). img_hwc: (img_h, img_w, channels) uint8 on
 * the device; inverse_maps: (n, 2, 3) float64 on the device, the dst -> src maps (warpAffine inverts M itself - so does
 * probpose_code_amd.transforms.invert_affine); crops_chw: (n, channels, out_h, out_w) uint8. OpenCV's fixed-point
 * bilinear arithmetic restated from its source; cv2 is not available in the build image: parity unpinned. */
int pp_warp_affine_u8(const void* img_hwc, int img_h, int img_w, int channels, const double* inverse_maps, void* crops_chw,
                      int n, int out_h, int out_w, void* stream);
/* The same crops cut from many images in one launch (the batches of a test loop): crop i is cut from image crop_image[i]
 * (n int32 on the device) with inverse_maps[i]; image j is the HWC uint8 buffer images[j] (a device table of device
 * pointers) of image_hw[2 j] rows and image_hw[2 j + 1] columns (int32 on the device); every image has `channels` channels.
 * max_img_h / max_img_w bound the sides in the table (checked here: below 32768, as pp_warp_affine_u8). Bytes equal to
 * pp_warp_affine_u8 on each image alone. */
int pp_warp_affine_u8_batch(const void* const* images, const int* image_hw, int channels, const int* crop_image,
                            const double* inverse_maps, int max_img_h, int max_img_w, void* crops_chw, int n, int out_h,
                            int out_w, void* stream);

/* The --draw-heatmap picture (mmpose/visualization/local_visualizer.py:215-343, 520-585, 796-865), csrc/pp_render.hip; the
 * drawing rules are stated there. K <= 22 (the reference's colour table); maps (K, H, W) < 2^29 values per map.
 * pp_parea_thresholds: per keypoint the probability-area threshold thr (K) float32 - the largest value v of maps[k] with
 * mass{x >= v} >= 0.75 * total, fp64 masses - and draw (K) int32 = 0 when a value is negative or non-finite or total < 0.75
 * (:560-568). Deterministic radix select, no sort; scratch: pp_parea_scratch_bytes(K, H, W) bytes (< 0: error). */
long long pp_parea_scratch_bytes(int K, int H, int W);
int pp_parea_thresholds(const float* maps, int K, int H, int W, void* scratch, float* thr, int* draw, void* stream);
/* The heatmap panel canvas_rgb (canvas_h, canvas_w, 3) uint8: image_rgb (img_h, img_w, 3) uint8 placed at (pad_left, pad_top)
 * inside an (80, 80, 80) border, the areas maps[k] > thr[k] of every drawn keypoint blended 0.7 / 0.3 with its colour and
 * outlined (:570-583), then 1-px green rectangles boxes (n_boxes, 4) int32 x1, y1, x2, y2 in canvas pixels (:844-858). */
int pp_parea_compose(const void* image_rgb, int img_h, int img_w, int pad_left, int pad_top, const float* maps, int K,
                     const float* thr, const int* draw, const int* boxes, int n_boxes, void* canvas_rgb, int canvas_h,
                     int canvas_w, void* stream);
/* The pose panel out_rgb (img_h, img_w, 3) uint8 from image_rgb: per instance its box (boxes (n, 4) int32 or NULL), its links
 * (skeleton (n_links, 2) int32, link_rgb (n_links, 3) uint8) and its points (keypoints (n, K, 2) float32, visible (n, K) float32,
 * kpt_rgb (K, 3) uint8) - _draw_instances_kpts + _draw_instances_bbox (:215-343) with integer rules of our own. */
int pp_draw_poses(const void* image_rgb, int img_h, int img_w, const float* keypoints, const float* visible, const int* boxes,
                  int n, int K, const int* skeleton, const void* link_rgb, const void* kpt_rgb, int n_links, double kpt_thr,
                  float radius, float thickness, float alpha, void* out_rgb, void* stream);
/* cv2.resize(src, (dst_w, dst_h), INTER_LINEAR) of an RGB uint8 image, restated in fp32 (half-pixel centres, edge clamp). */
int pp_resize_bilinear_u8(const void* src_rgb, int src_h, int src_w, void* dst_rgb, int dst_h, int dst_w, void* stream);

/* The pictures of many samples in one set of launches (added under version 4: purely additive), csrc/pp_render_batch.hip:
 * what pp_revert_heatmaps_max, pp_heatmap_posterior, pp_parea_thresholds, pp_parea_compose, pp_draw_poses and
 * pp_resize_bilinear_u8 give picture by picture, byte for byte (the same per-pixel and per-part bodies, the same
 * partitions per picture), in a number of launches that does not depend on the number of pictures: one - the pose panel -
 * when no picture has a heatmap panel, twelve otherwise. */
#define PP_RENDER_MAX_KEYPOINTS 32
#define PP_RENDER_MAX_INSTANCES 255 /* per picture (the presence mean restates a reduction order that holds below 256) */
/* One picture. image: (height, width, 3) uint8, R G B or (bgr != 0) B G R; out: (height, width, 3) uint8 RGB, with heatmap
 * != 0 (2 height, width, 3): the pose panel over the probability-area panel resized to the image. pad: left, top, right,
 * bottom border of the canvas, canvas_h = height + top + bottom, canvas_w = width + left + right (heatmap pictures; else
 * ignored). Its instances are rows first .. first + count - 1 of the instance table. scratch_offset: where its share of
 * the scratch starts (bytes, a multiple of 256; pp_render_batch_scratch_bytes of it; the share begins with its (K,
 * canvas_h, canvas_w) float32 posterior maps). The shares of a call must not overlap, nor its outputs. */
typedef struct {
    const uint8_t* image;
    uint8_t* out;
    int64_t scratch_offset;
    int32_t height, width, bgr, heatmap;
    int32_t pad[4];
    int32_t canvas_h, canvas_w;
    int32_t first, count;
} pp_render_picture;
/* One instance. maps: its un-reverted (K, hm_h, hm_w) float32 maps (heatmap pictures; else ignored); inverse: the inverse
 * warp (canvas -> map, six doubles, as pp_revert_heatmaps_max takes it); keypoints (K, 2), visible (K), presence (K): the
 * first K entries; box: its int pose box x1, y1, x2, y2 in image pixels, drawn when box_valid != 0; rect: its aspect-fixed
 * rectangle in canvas pixels, drawn on the heatmap panel when rect_valid != 0. */
typedef struct {
    const float* maps;
    double inverse[6];
    float keypoints[2 * PP_RENDER_MAX_KEYPOINTS];
    float visible[PP_RENDER_MAX_KEYPOINTS];
    float presence[PP_RENDER_MAX_KEYPOINTS];
    int32_t box[4];
    int32_t rect[4];
    int32_t box_valid, rect_valid;
} pp_render_instance;
/* Host only: bytes of scratch of one heatmap picture with K keypoints and a (canvas_h, canvas_w) canvas, a multiple of 256:
 * its posterior maps, its canvas, the partial sums, the histogram partials, states, thresholds. < 0: error. */
long long pp_render_batch_scratch_bytes(int K, int canvas_h, int canvas_w);
/* pictures / instances / tiles: the tables on the device; *_host: the same bytes in host memory (the caller's staging
 * buffer), read here for the argument checks - all of which run before any HIP call - and the grid sizes. tiles: 2
 * (n_pictures + 1) int32, two exclusive prefixes over the pictures with the total last: of the canvas row tiles
 * canvas_h * ceil(canvas_w / 256) (0 for a picture without heatmap), then of the image row tiles height * ceil(width / 256);
 * a workgroup finds its picture by a search in them. K keypoints (<= 32; <= 22 when a picture has a heatmap panel) and
 * (hm_h, hm_w) maps for every instance of the call. skeleton (n_links, 2) int32, link_rgb (n_links, 3), kpt_rgb (K, 3)
 * uint8, on the device, and kpt_thr, radius, thickness, alpha: as pp_draw_poses takes them. scratch: scratch_bytes bytes on
 * the device (may be NULL when no picture has a heatmap panel). A picture with no instance and no heatmap panel is legal:
 * its output is its image, as RGB. */
int pp_render_samples_batch(const pp_render_picture* pictures_host, const pp_render_instance* instances_host, const int* tiles_host,
                            const pp_render_picture* pictures, const pp_render_instance* instances, const int* tiles,
                            int n_pictures, int n_instances, int K, int hm_h, int hm_w, const int* skeleton, const void* link_rgb,
                            const void* kpt_rgb, int n_links, double kpt_thr, float radius, float thickness, float alpha,
                            void* scratch, long long scratch_bytes, void* stream);

/* Split JPEG decoder (added under version 4: purely additive). The serial part - markers and Huffman codes - runs on host
 * threads (csrc/pp_jpeg_host.h), the data-parallel rest - dequantisation, 8x8 inverse DCT, chroma upsampling, YCbCr -> BGR,
 * HWC packing - in csrc/pp_jpeg.hip. The pixels are those of libjpeg-turbo's default decoder (islow IDCT, fancy upsampling)
 * as mmcv.imread / cv2.imdecode / Pillow return them, bit for bit; the integer rules are stated in csrc/pp_jpeg.hip.
 * Accepted: SOF0 / SOF1, 8 bits, Huffman coding, one interleaved scan, 1 component or 3 components with chroma sampled 1x1
 * and luma 1x1, 2x1 or 2x2, any DQT / DHT tables, restart intervals. Everything else, and every irregular stream (bad code,
 * wrong or missing RSTn, data ending early, coefficient index past 63, missing table, zero dimension), is
 * PP_ERR_UNSUPPORTED with a reason: the caller decodes such a file on the host as before. No partial images. */
typedef struct {
    int32_t width, height, ncomp, precision;
    int32_t hs, vs;                 /* luma sampling factors (chroma is 1x1)                              */
    int32_t mcus_x, mcus_y;         /* MCU grid                                                          */
    int32_t comp_bw[3], comp_bh[3]; /* 8x8 blocks per row / block rows of each component, whole MCUs    */
    int32_t restart_interval;       /* MCUs between RSTn markers, 0: none                                */
    int32_t supported;              /* 1: inside the accepted subset                                      */
    int64_t coef_count;             /* int16 coefficients of all components = 64 x blocks                */
    char reason[96];                /* why the file was refused ("" when supported)                      */
} pp_jpeg_info;

/* One image of a batched reconstruct (a device table of these drives both launches). coef: info.coef_count int16, per
 * component [block_row][block_col][64] in natural order; qtables: ncomp x 64 uint16, natural order; planes:
 * info.coef_count bytes of scratch (the component planes, 8-byte aligned); out: (height, width, 3) uint8 BGR. */
typedef struct {
    const int16_t* coef;
    const uint16_t* qtables;
    uint8_t* planes;
    uint8_t* out;
    int32_t width, height, ncomp, hs, vs, mcus_x, mcus_y, reserved;
} pp_jpeg_desc;

/* Host only, re-entrant, no HIP call. data_host: the file's bytes. PP_OK: *info describes a file pp_jpeg_entropy_decode
 * accepts as far as its headers tell; PP_ERR_UNSUPPORTED: info->reason (and pp_last_error) say why. */
int pp_jpeg_probe(const void* data_host, size_t size, pp_jpeg_info* info);
/* Host only, re-entrant, no HIP call: the quantised coefficients of the file into coef_host (coef_capacity int16 values,
 * PP_ERR_WORKSPACE when that is fewer than info->coef_count) and each component's quantisation table into qtables_host
 * (3 x 64 uint16). On any status but PP_OK the buffers hold no image. */
int pp_jpeg_entropy_decode(const void* data_host, size_t size, int16_t* coef_host, long long coef_capacity,
                           uint16_t* qtables_host, pp_jpeg_info* info);
/* Bytes of plane scratch for n images (infos_host: n pp_jpeg_info), each image's share rounded up to 256: image i's planes
 * start at the sum of the shares before it. < 0: error. */
long long pp_jpeg_scratch_bytes(const pp_jpeg_info* infos_host, int n);
/* Pixels of n images of any mix of sizes and sampling in two launches ("jpeg_idct", "jpeg_color" of pp_launch_count):
 * descriptors: n pp_jpeg_desc on the device; max_blocks / max_height / max_width: the largest block count
 * (coef_count / 64), height and width in the table - they size the launch grids, every image is bounded by its own entry. */
int pp_jpeg_reconstruct_bgr_batch(const pp_jpeg_desc* descriptors, int n, long long max_blocks, int max_height, int max_width,
                                  void* stream);

/* Split JPEG encoder (added under version 4: purely additive), the decoder's counterpart: colour conversion, edge
 * expansion, chroma downsampling, 8x8 forward DCT and quantisation in csrc/pp_jpeg_enc.hip, Huffman coding and the marker
 * segments on host threads (csrc/pp_jpeg_enc_host.h). The file holds the quantised coefficients, tables and sampling
 * libjpeg-turbo's default compressor writes for the same pixels, quality and subsampling (islow FDCT, no smoothing, the
 * annex K Huffman tables), so it decodes to the same pixels; the integer rules are stated in csrc/pp_jpeg_enc.hip.
 * Written: baseline (SOF0) YCbCr JFIF files, 4:4:4 / 4:2:2 / 4:2:0, optional restart intervals. */

/* One image of a batched forward transform (a device table of these drives both launches). src: height rows of width
 * 3-byte pixels, row_stride bytes apart, B G R or (rgb != 0) R G B; qtables: 3 x 64 uint16, natural order, one table per
 * component; planes: info.coef_count bytes of scratch, 8-byte aligned (pp_jpeg_scratch_bytes sizes a batch's);
 * coef: info.coef_count int16 out, 16-byte aligned, in the layout of pp_jpeg_desc.coef. hs / vs / mcus_x / mcus_y: as
 * pp_jpeg_encode_plan gives them. */
typedef struct {
    const uint8_t* src;
    const uint16_t* qtables;
    uint8_t* planes;
    int16_t* coef;
    int32_t width, height, row_stride, rgb, hs, vs, mcus_x, mcus_y;
} pp_jpeg_enc_desc;

/* Host only. qtables_host (3 x 64 uint16, natural order: luma, chroma, chroma) <- the tables of libjpeg's
 * jpeg_set_quality(quality, force_baseline): annex K.1 scaled, clamped to 1..255. quality: 1..100. */
int pp_jpeg_quality_tables(int quality, uint16_t* qtables_host);
/* Host only. *info <- geometry of a width x height (1..65535) three-component file: MCU grid, comp_bw / comp_bh, coef_count.
 * subsampling: 0 4:4:4, 1 4:2:2, 2 4:2:0. */
int pp_jpeg_encode_plan(int width, int height, int subsampling, pp_jpeg_info* info);
/* Quantised coefficients of n images of any mix of sizes and sampling in two launches ("jpeg_enc_color", "jpeg_enc_fdct" of
 * pp_launch_count). descriptors: n pp_jpeg_enc_desc on the device; max_blocks / max_height / max_width: the largest block
 * count (coef_count / 64), height and width in the table - they size the launch grids, every image is bounded by its own
 * entry. The source pixels are only read. n == 0: PP_OK, nothing is launched. */
int pp_jpeg_forward_batch(const pp_jpeg_enc_desc* descriptors, int n, long long max_blocks, int max_height, int max_width,
                          void* stream);
/* Host only. A capacity no file of this geometry exceeds, whatever its coefficients and restart interval. < 0: error. */
long long pp_jpeg_encoded_bound(const pp_jpeg_info* info);
/* Host only, re-entrant, no HIP call, no allocation: the file of coef_host (info->coef_count int16) and qtables_host
 * (3 x 64 uint16, values 1..255) into out_host[0, capacity); *size_out <- its length. restart_interval: MCUs between RSTn
 * markers, 0: none. PP_ERR_WORKSPACE: capacity too small; PP_ERR_INVALID_ARG: a coefficient no baseline code expresses (a DC
 * difference outside -2047..2047, an AC value outside -1023..1023), an info that is no pp_jpeg_encode_plan result. */
int pp_jpeg_entropy_encode(const int16_t* coef_host, const uint16_t* qtables_host, const pp_jpeg_info* info, int restart_interval,
                           void* out_host, size_t capacity, size_t* size_out);
/* Host only, re-entrant: the bytes SOI .. SOS of the file pp_jpeg_entropy_encode writes for these tables, geometry and
 * restart interval (the same code writes both) into out_host[0, capacity); *size_out <- their length. A file is these
 * headers, the stream of pp_jpeg_entropy_encode_batch, then FF D9. */
int pp_jpeg_write_headers(const uint16_t* qtables_host, const pp_jpeg_info* info, int restart_interval, void* out_host,
                          size_t capacity, size_t* size_out);

/* Huffman coding on the device (csrc/pp_jpeg_entropy.hip; added under version 4: purely additive): the bytes
 * pp_jpeg_entropy_encode writes between the SOS header and the EOI marker, bit for bit, from coefficients that stay where
 * pp_jpeg_forward_batch left them. pp_jpeg_entropy_encode_batch and pp_jpeg_entropy_encode_opt_batch code without restart
 * intervals; the *_restart_batch calls further down honour every image's own. */

/* What the coder leaves per image: the length of the stream in bytes (also when it did not fit: the capacity it needs) and
 * PP_OK, PP_ERR_INVALID_ARG (a DC difference outside -2047..2047 or an AC value outside -1023..1023: the stream is
 * undefined; or a descriptor without a plan's geometry) or PP_ERR_WORKSPACE (capacity below the need: nothing written). */
typedef struct {
    int64_t bytes;
    int32_t status;
    int32_t reserved;
} pp_jpeg_ent_result;

/* One image of a batched entropy coding (a device table of these drives every launch). coef: info.coef_count int16 in the
 * layout of pp_jpeg_desc.coef, 16-byte aligned, only read; scratch: the image's share of pp_jpeg_entropy_scratch_bytes,
 * 16-byte aligned, contents undefined before and after; out / capacity: where the stream goes and how many bytes fit;
 * result: the image's slot; hs / vs / mcus_x / mcus_y: as pp_jpeg_encode_plan gives them; restart_interval: MCUs between
 * RSTn markers, 0: none - read by the *_restart_batch calls only (the calls without "restart" in their name code without
 * intervals whatever it holds). */
typedef struct {
    const int16_t* coef;
    uint8_t* scratch;
    uint8_t* out;
    pp_jpeg_ent_result* result;
    int64_t capacity;
    int32_t hs, vs, mcus_x, mcus_y;
    int32_t restart_interval;
    int32_t reserved;
} pp_jpeg_ent_desc;

/* Host only. Bytes of scratch for n images (infos_host: n pp_jpeg_encode_plan results), each image's share a multiple of
 * 256: image i's share starts at the sum of the shares before it. < 0: error. */
long long pp_jpeg_entropy_scratch_bytes(const pp_jpeg_info* infos_host, int n);
/* The streams of n images of any mix of sizes and sampling in seven launches ("jpeg_ent_bits", "jpeg_ent_scan",
 * "jpeg_ent_zero", "jpeg_ent_pack", "jpeg_ent_ffcount", "jpeg_ent_ffscan", "jpeg_ent_stuff" of pp_launch_count).
 * descriptors: n pp_jpeg_ent_desc on the device; max_blocks: the largest block count (coef_count / 64) in the table - it
 * sizes the grids, every image is bounded by its own entry. No allocation, no synchronisation, no read-back: the caller
 * reads the result slots after the stream has run. An image's failure leaves the others untouched; nothing is written
 * outside an image's scratch share, out[0, capacity) and result slot. n == 0: PP_OK, nothing is launched. */
int pp_jpeg_entropy_encode_batch(const pp_jpeg_ent_desc* descriptors, int n, long long max_blocks, void* stream);

/* Optimised Huffman tables (csrc/pp_jpeg_opt_core.h; added under version 4: purely additive): a file coded with the tables
 * libjpeg's jpeg_gen_optimal_table builds from the image's own symbol statistics - what Pillow's save(optimize=True) writes
 * for the same coefficients: the same pixels in fewer bytes. Tables are always in the order of the file's DHT segments: DC
 * luma, AC luma, DC chroma, AC chroma. Code lengths stay at most 16 bits and no table has more symbols than its annex K
 * counterpart (12 DC, 162 AC), so pp_jpeg_encoded_bound holds for these files as well. A plan of more than 2^32 / 64 blocks
 * is refused (PP_ERR_INVALID_ARG): 32-bit frequencies are then exact. */

/* Host only, re-entrant. hist[t][s] <- how often the scan of coef_host codes symbol s with table t: the DC categories,
 * (run << 4) | size per non-zero AC coefficient, 0xF0 per sixteen zeros in front of one, 0x00 per block whose zigzag position
 * 63 is zero; hist[t][256] <- 0. restart_interval: the DC prediction restarts with every interval. PP_ERR_INVALID_ARG as
 * pp_jpeg_entropy_encode. */
int pp_jpeg_symbol_histogram(const int16_t* coef_host, const pp_jpeg_info* info, int restart_interval, uint32_t hist[4][257]);
/* Host only, re-entrant. bits[l - 1] (codes of length l = 1..16) and vals (the symbols in code order; *nvals of them, the
 * rest zero) of libjpeg's optimal table for freq (freq[256] is taken as 1: the pseudo-symbol that keeps the all-ones code
 * free). PP_ERR_INVALID_ARG: a code tree deeper than 32 (frequencies that grow like the Fibonacci numbers over more than 32
 * symbols; libjpeg refuses them too). */
int pp_jpeg_optimal_table(const uint32_t freq[257], uint8_t bits[16], uint8_t vals[256], int* nvals);
/* pp_jpeg_write_headers with the file's four Huffman tables passed in (bits[t], vals[t]; table t has the sum of bits[t]
 * symbols): the same segments in the same order, one DHT segment per table immediately in front of DRI / SOS.
 * PP_ERR_INVALID_ARG also for a table that is no prefix code of at most 256 symbols. */
int pp_jpeg_write_headers_tables(const uint16_t* qtables_host, const pp_jpeg_info* info, int restart_interval, const uint8_t bits[4][16],
                                 const uint8_t vals[4][256], void* out_host, size_t capacity, size_t* size_out);
/* pp_jpeg_entropy_encode with the image's own optimal tables in the DHT segments and in the scan: same arguments, same
 * error contract, any restart interval. */
int pp_jpeg_entropy_encode_opt(const int16_t* coef_host, const uint16_t* qtables_host, const pp_jpeg_info* info, int restart_interval,
                               void* out_host, size_t capacity, size_t* size_out);

/* What pp_jpeg_entropy_encode_opt_batch keeps per image on the device (16-byte aligned, contents undefined before): the
 * histograms, the tables built from them (the host reads bits / vals back with the result slots and writes them into the
 * DHT segments), code | length << 16 of every symbol, and PP_OK or PP_ERR_INVALID_ARG (too many blocks, a tree deeper
 * than 32). */
typedef struct {
    uint32_t hist[4][257];
    uint8_t bits[4][16];
    uint8_t vals[4][256];
    uint32_t lookup[4][256];
    int32_t status;
    int32_t nvals[4];
    int32_t reserved[7];
} pp_jpeg_opt_record;

/* One image of pp_jpeg_entropy_encode_opt_batch: pp_jpeg_ent_desc and the image's record. */
typedef struct {
    pp_jpeg_ent_desc ent;
    pp_jpeg_opt_record* record;
} pp_jpeg_ent_opt_desc;

/* Host only. As pp_jpeg_entropy_scratch_bytes (the records are the caller's own); PP_ERR_INVALID_ARG for a plan of too many
 * blocks. */
long long pp_jpeg_entropy_opt_scratch_bytes(const pp_jpeg_info* infos_host, int n);
/* pp_jpeg_entropy_encode_batch with every image's own optimal tables, built and used on the device
 * (csrc/pp_jpeg_entropy_opt.hip): the streams are those of pp_jpeg_entropy_encode_opt, bit for bit. Ten launches:
 * "jpeg_opt_clear" (the histograms), "jpeg_opt_hist", "jpeg_opt_build" (one wave per image and table), then the coder's
 * seven phases reading the record's lookup: "jpeg_opt_bits", "jpeg_opt_scan", "jpeg_opt_zero", "jpeg_opt_pack",
 * "jpeg_opt_ffcount", "jpeg_opt_ffscan", "jpeg_opt_stuff". The rules of pp_jpeg_entropy_encode_batch: no allocation, no
 * synchronisation, no read-back; an image's failure (its slot's status, PP_ERR_INVALID_ARG also for a refused record) leaves
 * the others untouched; nothing is written outside an image's scratch share, out[0, capacity), result slot and record. */
int pp_jpeg_entropy_encode_opt_batch(const pp_jpeg_ent_opt_desc* descriptors, int n, long long max_blocks, void* stream);

/* The device coder with restart intervals (added under version 4: purely additive). Every image of a batch has its own
 * descriptor field restart_interval, 0 included: the stream is what pp_jpeg_entropy_encode resp. pp_jpeg_entropy_encode_opt
 * writes between the SOS header and the EOI marker for that interval, bit for bit - the DC prediction restarts with every
 * interval, every interval is padded with ones to a whole byte (a padding byte FF gets its 00), and FF D0 .. FF D7, never
 * stuffed, stand between the intervals. An image with interval 0, or one of at least its MCU count, gets the bytes of the
 * calls above. An interval outside 0..65535 fails that image alone (PP_ERR_INVALID_ARG). result->bytes counts the markers,
 * also when the stream does not fit (PP_ERR_WORKSPACE, nothing written). */

/* Host only. As pp_jpeg_entropy_scratch_bytes, for the two calls below: an image's share for any interval (sized for one MCU
 * per interval: sixteen bytes per MCU for the interval table, seven padding bits per MCU in the bit buffer). Never below
 * pp_jpeg_entropy_scratch_bytes of the same plans. < 0: error. */
long long pp_jpeg_entropy_restart_scratch_bytes(const pp_jpeg_info* infos_host, int n);
/* pp_jpeg_entropy_encode_batch with the intervals of the descriptors, its rules and its arguments; scratch shares of
 * pp_jpeg_entropy_restart_scratch_bytes. Seven launches: "jpeg_ent_rst_bits", "jpeg_ent_rst_scan" (which also lays the
 * intervals out: one workgroup per image), "jpeg_ent_rst_zero", "jpeg_ent_rst_pack", "jpeg_ent_rst_ffcount",
 * "jpeg_ent_rst_ffscan", "jpeg_ent_rst_stuff" of pp_launch_count. */
int pp_jpeg_entropy_encode_restart_batch(const pp_jpeg_ent_desc* descriptors, int n, long long max_blocks, void* stream);
/* pp_jpeg_entropy_encode_opt_batch with the intervals of the descriptors (descriptors[i].ent.restart_interval): the tables
 * are built from the statistics of the restarted DC differences, as pp_jpeg_symbol_histogram counts them. Ten launches:
 * "jpeg_opt_clear", "jpeg_opt_rst_hist", "jpeg_opt_build", "jpeg_opt_rst_bits", "jpeg_opt_rst_scan", "jpeg_opt_rst_zero",
 * "jpeg_opt_rst_pack", "jpeg_opt_rst_ffcount", "jpeg_opt_rst_ffscan", "jpeg_opt_rst_stuff". */
int pp_jpeg_entropy_encode_opt_restart_batch(const pp_jpeg_ent_opt_desc* descriptors, int n, long long max_blocks, void* stream);

/* Huffman decoding on the device (csrc/pp_jpeg_huffdec.hip; added under version 4: purely additive): the coefficients
 * pp_jpeg_entropy_decode gives, bit for bit, from the file's own entropy-coded bytes, by self-synchronising passes. The
 * stream is cut into subsequences of 128 raw bytes, each decoded by one thread from a guessed state (bit position, block
 * inside the MCU, zigzag index); a decoder started wrongly falls into step with the true one after a short distance, so
 * passes that hand every subsequence its predecessor's exit state converge, and a final check proves it: an image is
 * accepted only if every subsequence's entry equals its predecessor's exit. An image the passes did not synchronise is
 * PP_ERR_UNSUPPORTED, never wrong data. A file with a restart interval decodes as well: a decoder that reaches an RSTn
 * marker leaves it in the true decoder's state whatever its own entry was, so inside such a file the synchronisation
 * distance is bounded by the interval's length; the markers' numbers, their count and the blocks between them are checked
 * on the proven chain (reason 7). */

/* One Huffman table in the form the device reads (the host decoder's own lookup): look[next 9 bits] = length << 8 | symbol
 * for codes of at most 9 bits (0: longer); maxcode[len] the largest code of a length (-1: none; [17] = INT32_MAX);
 * vals[code + valoffset[len]] the symbol of a longer code. */
typedef struct {
    uint16_t look[512];
    int32_t maxcode[18];
    int32_t valoffset[18];
    uint8_t vals[256];
} pp_jpeg_huff_table;

/* What pp_jpeg_scan_prepare reads from a file's headers: geometry, each component's quantisation table (natural order, as
 * pp_jpeg_entropy_decode returns them), each component's tables (tables[2 c] DC, tables[2 c + 1] AC) and where the
 * entropy-coded segment lies in the file: from behind the SOS header to the first marker, which must be EOI. */
typedef struct {
    pp_jpeg_info info;
    uint16_t qtables[3 * 64];
    pp_jpeg_huff_table tables[6];
    int64_t stream_offset, stream_bytes;
} pp_jpeg_scan;

/* What the decoder leaves per image. status: PP_OK, PP_ERR_UNSUPPORTED (reason 1: not synchronised within sync_passes;
 * 2: data ends before the last block; 3: a bit pattern that is no code, a category or a zigzag index no baseline stream
 * holds; 4: a DC coefficient outside int16; 5: data after the last block; 7: a restart marker missing, out of order, in
 * excess, inside a block or an MCU, or not behind the interval's last MCU) or PP_ERR_INVALID_ARG (reason 6: the
 * descriptor describes no file of the subset). On any status but PP_OK the coefficients are undefined. passes: the
 * synchronisation launches that were needed (1 + the last one in which a subsequence was decoded again); blocks: the
 * blocks counted along the chain. */
typedef struct {
    int32_t status, passes, blocks, reason;
} pp_jpeg_hd_result;

/* One image of a batched Huffman decode (a device table of these drives every launch). stream / stream_bytes: the
 * entropy-coded segment, byte stuffing included, only read (fewer than 2^28 bytes); tables: its 2 x ncomp
 * pp_jpeg_huff_table, 4-byte aligned; coef: mcus_x * mcus_y * blocks-per-MCU * 64 int16 out in the layout of
 * pp_jpeg_desc.coef, 16-byte aligned; scratch: the image's share of pp_jpeg_huffman_scratch_bytes, 16-byte aligned,
 * contents undefined before and after; result: the image's slot; restart_interval: the file's (pp_jpeg_info's), 0: none -
 * then no byte of the stream is taken for a marker. */
typedef struct {
    const uint8_t* stream;
    const pp_jpeg_huff_table* tables;
    int16_t* coef;
    uint8_t* scratch;
    pp_jpeg_hd_result* result;
    int64_t stream_bytes;
    int32_t hs, vs, mcus_x, mcus_y, ncomp, restart_interval;
} pp_jpeg_hd_desc;

/* Host only, re-entrant, no HIP call, no per-bit work: the headers of a file through the parser of pp_jpeg_probe, and the
 * bounds of its entropy-coded segment by a search for FF bytes. PP_ERR_UNSUPPORTED with scan->info.reason: everything
 * pp_jpeg_probe refuses, a file with a restart interval (it keeps the host Huffman decoder), a segment that no EOI marker
 * ends, a segment of 2^28 bytes or more. */
int pp_jpeg_scan_prepare(const void* data_host, size_t size, pp_jpeg_scan* scan);
/* The same (added under version 4 as well), but a file with a restart interval is accepted: scan->info.restart_interval is
 * set and the segment runs from behind the SOS header to the first marker that is no RSTn, which must be EOI - FF D0..D7
 * and the FF fill bytes in front of them belong to it. Still a search for FF bytes: the markers' order and number are the
 * device decoder's to check. More than 7 fill bytes in front of an RSTn are PP_ERR_UNSUPPORTED (the device decoder looks
 * no further; the host decoder takes such a file). Without a restart interval: status, reason and every byte of *scan are
 * pp_jpeg_scan_prepare's. */
int pp_jpeg_scan_prepare_restart(const void* data_host, size_t size, pp_jpeg_scan* scan);
/* Host only. Bytes of scratch for n images with segments of stream_bytes_host[i] bytes (infos_host: their pp_jpeg_info),
 * each image's share a multiple of 256: image i's share starts at the sum of the shares before it; a file with a restart
 * interval has a larger one. < 0: error. */
long long pp_jpeg_huffman_scratch_bytes(const pp_jpeg_info* infos_host, const long long* stream_bytes_host, int n);
/* The coefficients of n images of any mix of sizes and sampling in sync_passes + 4 launches (sync_passes x "jpeg_hd_sync",
 * "jpeg_hd_scan", "jpeg_hd_zero", "jpeg_hd_write", "jpeg_hd_dc" of pp_launch_count). descriptors: n pp_jpeg_hd_desc on
 * the device; max_stream_bytes / max_blocks: the longest segment and the largest block count in the table - they size the
 * grids, every image is bounded by its own entry. sync_passes: 1 .. 64; a launch carries states 32 subsequences on inside
 * a workgroup's 256 and one across its border, so p launches cover a synchronisation distance of 128 (32 (p - 1) + 2)
 * bytes (p = 3: 8448). No allocation, no synchronisation, no read-back: the caller reads the result slots after the
 * stream has run. An image's failure leaves the others untouched; nothing is written outside an image's scratch share,
 * its coefficients and its result slot; the same input gives the same bytes launch after launch. n == 0: PP_OK, nothing
 * is launched. */
int pp_jpeg_huffman_decode_batch(const pp_jpeg_hd_desc* descriptors, int n, long long max_stream_bytes, long long max_blocks,
                                 int sync_passes, void* stream);

/* PNG files written from the device (csrc/pp_png.hip, csrc/pp_png_core.h; added under version 4: purely additive). 8-bit
 * truecolour, non-interlaced, one IDAT chunk, no ancillary chunk. Each row takes, of the five PNG filters, the one with the
 * smallest sum of min(b, 256 - b) over its bytes (ties: the lowest number). The filtered stream is cut into tiles of 4096
 * bytes; a run of equal bytes inside a tile becomes a literal and matches of length 3..258 at distance 1; the tokens are
 * coded in ONE dynamic deflate block with a Huffman code built from the stream's own histogram - on the host by default
 * (pp_deflate_build_code, between the two halves), or on the device by one launch more (pp_png_code_batch, opt-in: the
 * same code, byte for byte, without the round trip). The deflate stage takes any byte stream: a descriptor without pixels compresses `data` as it stands into a zlib stream.
 *
 * A second match mode, "lz" (the *_lz functions; opt-in, the unsuffixed ones are unchanged): beside runs (distance 1) a
 * position may copy from one pixel back (distance 3) and from the row above (distance P = 1 + 3 * width, P - 3, P + 3; for a
 * raw stream P is the descriptor's `period`, 0 for none), chosen by a greedy rule with a one-byte lookahead; the tokens of a
 * tile form a chain that the device resolves by pointer doubling. Two Huffman codes, literal/length and distance, both
 * from the stream's own histograms. csrc/pp_png_core.h states the rule in full. */

/* A stream's Huffman code as the device reads it. sym[s]: the bit-reversed code of literal/length symbol s | its length << 16
 * (0: unused); header: the first header_bits bits of the zlib stream, LSB first in little-endian words (78 01, BFINAL,
 * BTYPE, HLIT, HDIST, HCLEN, the code-length code and the lengths). */
typedef struct {
    uint32_t sym[288];
    uint32_t header_bits;
    uint32_t reserved[3];
    uint32_t header[76];
} pp_deflate_code;

/* The code of a stream in lz mode: `base` as above (its header then holds both codes' lengths: at most 2302 bits), and
 * dist[s]: the bit-reversed code of distance symbol s (0 .. 29) | its length << 16 (0: unused). */
typedef struct {
    pp_deflate_code base;
    uint32_t dist[32];
} pp_deflate_code_lz;

/* What the coder leaves per stream: the length of the zlib stream in bytes (also when it did not fit: the capacity it
 * needs), PP_OK, PP_ERR_INVALID_ARG (a descriptor that describes nothing) or PP_ERR_WORKSPACE (capacity below the need:
 * nothing written), and the CRC-32 register after crc_init and the stream's bytes (the chunk's CRC is its complement). */
typedef struct {
    int64_t bytes;
    int32_t status;
    uint32_t crc;
} pp_deflate_result;

/* One stream of a batch (a device table of these drives every launch). pixels: NULL, or the picture's top-left byte -
 * (height, width, 3) uint8 with row_stride bytes between rows, rgb: 1 for R,G,B in memory, 0 for B,G,R - only read; then
 * len = height * (1 + 3 * width) and pp_png_tokens_batch writes the filtered stream to data. Without pixels data is only
 * read. data: 16-byte aligned; hist: 288 uint32 (the histogram of the 286 symbols, symbol 256 counted once); code: what
 * pp_deflate_build_code made of hist, read by pp_png_deflate_batch only - and written by pp_png_code_batch(_lz), the one
 * call that stores through this pointer (the whole struct, in lz mode the whole pp_deflate_code_lz); scratch: the stream's share of
 * pp_deflate_scratch_bytes, 16-byte aligned, contents undefined before and after; out / capacity: where the zlib stream
 * goes (16-byte aligned) and how many bytes fit; crc_init: the CRC-32 register in front of the stream's first byte.
 * period: read in lz mode only - the row period P of a raw stream (0: no far candidates); with pixels it must be 0, P is
 * 1 + 3 * width. In lz mode hist holds 320 uint32 (the 288 as above, then the counts of the 30 distance symbols), code
 * points at the `base` of a pp_deflate_code_lz, and scratch is the share pp_deflate_scratch_bytes_lz gives. */
typedef struct {
    const uint8_t* pixels;
    uint8_t* data;
    uint32_t* hist;
    const pp_deflate_code* code;
    uint8_t* scratch;
    uint8_t* out;
    pp_deflate_result* result;
    int64_t len;
    int64_t capacity;
    int32_t width, height;
    int64_t row_stride;
    int32_t rgb;
    uint32_t crc_init;
    int64_t period;
} pp_deflate_desc;

/* Host only. A capacity no zlib stream of this coder exceeds for len (1 .. 2^31 - 1) input bytes: 15 bits a byte, header,
 * end-of-block and Adler-32. PP_ERR_INVALID_ARG: len out of range or a bound of 2^31 bytes or more. */
long long pp_deflate_bound(long long len);
/* Host only. A capacity no file of a width x height picture exceeds: pp_deflate_bound of its filtered stream and 57 bytes
 * of framing. PP_ERR_INVALID_ARG: a side outside 1..65535, or a stream bound of 2^31 bytes or more. */
long long pp_png_encoded_bound(int width, int height);
/* Host only. Bytes of scratch for one stream of len bytes, a multiple of 256. < 0: error. */
long long pp_deflate_scratch_bytes(long long len);
/* Host only, re-entrant: the code of a histogram (hist_host: 286 counts; symbol 256 is taken as used whatever its count).
 * Lengths of at most 15 bits, a complete code (Kraft sum 1; with fewer than two used symbols an unused one is added), one
 * distance code of length 1, a code-length code of at most 7 bits that does not use symbols 16..18. The same histogram
 * gives the same code. */
int pp_deflate_build_code(const uint32_t* hist_host, pp_deflate_code* code_host);
/* Host only, re-entrant, no HIP call: the zlib stream of data_host[0, len) into out_host[0, capacity) by the sequential
 * form of the core the kernels run (the same bytes); *size_out <- its length, *tokens_out (may be NULL) <- the literals and
 * matches in it. PP_ERR_WORKSPACE: capacity too small (*size_out <- the need). */
int pp_zlib_compress(const void* data_host, long long len, void* out_host, size_t capacity, size_t* size_out, long long* tokens_out);
/* Host only, re-entrant, no HIP call: the whole file of a picture in host memory (arguments as pp_deflate_desc's) into
 * out_host[0, capacity); *size_out <- its length. The sequential form of the same core: the file pp_png_tokens_batch,
 * pp_deflate_build_code and pp_png_deflate_batch give, byte for byte. */
int pp_png_encode(const uint8_t* pixels_host, int width, int height, long long row_stride, int rgb, void* out_host, size_t capacity,
                  size_t* size_out);
/* The first half on the device, in three launches ("png_filter": a workgroup per row, only with max_height > 0 and only for
 * descriptors with pixels; "png_clear": the histograms zeroed; "png_hist": a workgroup per tile - the tokens counted into
 * hist, the tile's Adler-32 partial into scratch). descriptors: n pp_deflate_desc on the device; max_height / max_len: the
 * largest height and stream length in the table - they size the grids, every stream is bounded by its own entry. The
 * caller then reads the histograms, builds the codes and uploads them. No allocation, no synchronisation. */
int pp_png_tokens_batch(const pp_deflate_desc* descriptors, int n, int max_height, long long max_len, void* stream);
/* The second half, in five launches ("png_bits": a tile's bit count; "png_scan": one workgroup per stream - 64-bit prefix
 * sums, the Adler-32 combination, size and status into the result slot; "png_zero": the words in use; "png_pack": header,
 * tokens, end-of-block, padding, Adler-32 ORed into the words; "png_crc": the bytes copied to out and their CRC-32 XORed
 * into the slot). A stream that does not fit leaves out untouched; one stream's failure leaves the others alone; nothing
 * is written outside a stream's scratch share, out[0, capacity) and result slot; the same input gives the same bytes
 * launch after launch. n == 0: PP_OK, nothing is launched. */
int pp_png_deflate_batch(const pp_deflate_desc* descriptors, int n, long long max_len, void* stream);
/* The code build on the device, in one launch ("png_code": one workgroup per stream), called between pp_png_tokens_batch
 * and pp_png_deflate_batch on the same stream in place of the histogram download, pp_deflate_build_code and the code
 * upload. It reads each descriptor's hist (288 words) and writes *code: every byte of the pp_deflate_code that
 * pp_deflate_build_code gives for the same histogram. A descriptor that describes no stream or whose code is NULL is
 * skipped (pp_png_deflate_batch refuses it into its result slot); nothing else is written. No stored length exceeds 15
 * and header_bits stays within what pp_deflate_bound counts. No allocation, no synchronisation. n == 0: PP_OK, nothing is
 * launched. */
int pp_png_code_batch(const pp_deflate_desc* descriptors, int n, void* stream);
/* Host only, re-entrant, no HIP call: the steps of the device build (csrc/pp_png_code_core.h) one after another - the code
 * pp_deflate_build_code gives, byte for byte. For tests of the kernel's logic without a GPU. */
int pp_deflate_build_code_steps(const uint32_t* hist_host, pp_deflate_code* code_host);

/* lz mode. The host queries, as their unsuffixed counterparts: the bound holds the longer header (both codes), the scratch
 * share also holds the parse (one uint16 per input byte). */
long long pp_deflate_bound_lz(long long len);
long long pp_deflate_scratch_bytes_lz(long long len);
/* Host only, re-entrant: both codes of a histogram of 320 words (286 literal/length counts at 0, 30 distance counts at 288).
 * The literal/length code as pp_deflate_build_code's; the distance code likewise at most 15 bits and complete (with fewer
 * than two used symbols unused ones are added), HDIST the highest symbol with a length. */
int pp_deflate_build_code_lz(const uint32_t* hist_host, pp_deflate_code_lz* code_host);
/* Host only, re-entrant, no HIP call: pp_zlib_compress in lz mode with row period `period` (>= 0; 0: near candidates
 * only), pp_png_encode in lz mode. The sequential run of the same core: the bytes the *_lz kernels give. */
int pp_zlib_compress_lz(const void* data_host, long long len, long long period, void* out_host, size_t capacity, size_t* size_out,
                        long long* tokens_out);
int pp_png_encode_lz(const uint8_t* pixels_host, int width, int height, long long row_stride, int rgb, void* out_host, size_t capacity,
                     size_t* size_out);
/* The two halves in lz mode: every stream of the call is coded in lz mode. Arguments, guarantees and error reporting as
 * pp_png_tokens_batch / pp_png_deflate_batch; eight launches per batch together, no workgroup waits for another. First half:
 * "png_filter" (as above), "png_clear_lz" (320 histogram words), "png_parse_lz" (a workgroup per tile: the candidates'
 * match lengths by a running minimum over the workgroup, the choice, the token starts by twelve rounds of pointer doubling
 * in LDS, the parse - one uint16 per byte - into scratch, both histograms, the tile's Adler-32 partial). Second half:
 * "png_bits_lz", "png_scan_lz", "png_zero_lz", "png_pack_lz", "png_crc_lz": as above, reading the stored parse. */
int pp_png_tokens_batch_lz(const pp_deflate_desc* descriptors, int n, int max_height, long long max_len, void* stream);
int pp_png_deflate_batch_lz(const pp_deflate_desc* descriptors, int n, long long max_len, void* stream);
/* pp_png_code_batch and pp_deflate_build_code_steps in lz mode ("png_code_lz"): hist holds 320 words, and the whole
 * pp_deflate_code_lz whose `base` the descriptor's code names is written - what pp_deflate_build_code_lz gives. */
int pp_png_code_batch_lz(const pp_deflate_desc* descriptors, int n, void* stream);
int pp_deflate_build_code_steps_lz(const uint32_t* hist_host, pp_deflate_code_lz* code_host);

/* Greedy OKS suppression (oks_nms with oks_iou, mmpose/evaluation/functional/nms.py:58-170, no vis_thr) of every image of a
 * dataset at once (csrc/pp_oks_nms.hip; added under version 4: purely additive). The instances of image i are rows
 * [img_off_host[i], img_off_host[i + 1]) of the flat arrays, ALREADY in that image's suppression order (descending score as
 * the caller's sort gives it: the tie order is the caller's). img_off_host (n_images + 1) is a HOST array: it starts at 0,
 * never decreases and ends at n_instances (checked). Device arrays: kpts (n_instances, K, 3) float64 = x, y and a third value
 * that is not read; areas (n_instances) float64; sigmas (K) float64. Per pair, in fp64 and numpy's operation order,
 *   e = (dx^2 + dy^2) / (2 sigma)^2 / ((a_i + a_j) / 2 + spacing(1)) / 2,   oks = sum_k exp(-e) / K
 * (area_f32 != 0: the areas are float32 values and (a_i + a_j) / 2 is formed in float32, as numpy does for a float32 area
 * array), and a kept row i removes every later row j with float32(oks) > float32(thr); a NaN oks removes.
 * keep (n_instances) uint8: 1 = kept. status (n_images) int32:
 *   PP_OKS_NMS_DECIDED    keep is the reference's;
 *   PP_OKS_NMS_UNDECIDED  some pair's fp64 oks lies within `guard` of the float32 rounding midpoint above float32(thr), where
 *                         the last bits of exp() decide: the caller runs the image on the host (its keep bytes are a valid
 *                         greedy result of the device's own values, not relied upon);
 *   PP_OKS_NMS_HOST       the image holds more than PP_OKS_NMS_MAX_PER_IMAGE instances (its keep bytes are 0).
 * workspace: pp_oks_nms_workspace_bytes(...) bytes, 8-byte aligned. Two launches (oks_nms_pairs, oks_nms_sweep) behind one
 * small table upload that is complete when the call returns; the same bytes launch after launch. */
#define PP_OKS_NMS_MAX_PER_IMAGE 4096
#define PP_OKS_NMS_DECIDED 0
#define PP_OKS_NMS_UNDECIDED 1
#define PP_OKS_NMS_HOST 2
long long pp_oks_nms_workspace_bytes(const long long* img_off_host, long long n_instances, int n_images);
int pp_oks_nms_batch(const double* kpts, const double* areas, const long long* img_off_host, const double* sigmas,
                     long long n_instances, int n_images, int K, double thr, double guard, int area_f32, void* workspace,
                     long long workspace_bytes, unsigned char* keep, int* status, void* stream);

/* ---- Loss mode: ProbMap targets and the OKS map loss (csrc/pp_probmap_encode.hip, csrc/pp_probmap_loss.hip; added under
 * version 4: purely additive). Evaluation-mode forward losses only: no gradients.
 *
 * pp_probmap_encode: ProbMap.encode (mmpose/codecs/probmap.py:98-168, codecs/utils/oks_map.py) for a batch in one launch
 * ("probmap_encode", one workgroup per map). keypoints (B, K, 2) float32 in input-pixel space, visible (B, K) float32. Per map:
 * the coordinates are divided by (in_w - 1) / (W - 1) and (in_h - 1) / (H - 1) in float32, then every pixel gets
 *   float32(exp(-(sqrt(dx^2 + dy^2))^2 / (2 s)))      in fp64, one rounding per operator,
 * s = clip((2 sigma_k)^2 sqrt(H / 1.25 * W / 1.25) 2, 0.55, 3.0) with the 17 COCO sigmas, or `sigma` when that is > 0.
 * visible < 0.5: a zero map, weight = visible. Otherwise weight = (some fp64 value of the map > 0) - decided before the rounding
 * to float32, so a keypoint far outside the map gets weight 0. annotated = visible > 0; in_image = 0 <= x < in_w and
 * 0 <= y < in_h on the unscaled coordinates. Outputs: heatmaps (B, K, H, W) float32, keypoint_weights (B, K) float32, annotated
 * and in_image (B, K) uint8. Status instead of a launch: NULL pointers, B < 0, K/H/W <= 0, in_w/in_h <= 0 (INVALID_ARG);
 * K != 17 with sigma <= 0 (INVALID_ARG: the sigma table is COCO's). A 1-pixel axis has scale factor (in - 1) / 0 = inf as in
 * numpy: every finite coordinate lands on 0. B = 0 returns PP_OK untouched.
 * pp_probmap_encode_s: the K values of s the launch would use, to a HOST array (the same checks; no device call). */
int pp_probmap_encode(const float* keypoints, const float* visible, int B, int K, int H, int W, double in_w, double in_h,
                      double sigma, float* heatmaps, float* keypoint_weights, unsigned char* annotated,
                      unsigned char* in_image, void* stream);
int pp_probmap_encode_s(int K, int H, int W, double sigma, double* s_host);

/* pp_probmap_loss_maps: OKSHeatmapLoss.forward(per_pixel=True), oks_type "minus" (mmpose/models/losses/heatmap_loss.py:552-638),
 * reduced to its mean, plus the argmax pixels pose_pck_accuracy(method="argmax") reads. pred, target (B, K, H, W) float32,
 * weights (B, K) float32 (the mask of _get_mask: the keypoint's weight over its whole map). Launch one ("probmap_loss_maps"), one
 * workgroup per map, the map staged once in LDS with a one-pixel zero halo: per map
 *   map_sums[b, k] = w[b, k] * sum_pixels( smoothing_weight (Gx^2 + Gy^2) + (1 - smoothing_weight - gaussian_weight) p (1 - t)
 *                                          + gaussian_weight (p - t)^2 )                                    in fp64,
 * Gx, Gy the 3x3 Sobel responses of p with zero "same" padding; argmax (B, K, 2) int32 = row-major index of the maximum of p and
 * of t (numpy's argmax: the first on ties, the first NaN if there is one) and maxval (B, K, 2) float32 those maxima. Launch two
 * ("probmap_loss_mean", one workgroup, a fixed tree): loss[0] = float32(loss_weight * sum(map_sums) / (B K H W)). No atomics:
 * the same bits launch after launch. map_sums (B, K) float64 is an output and the second launch's input.
 * Status instead of a launch: NULL pointers, B < 0, K/H/W <= 0 (INVALID_ARG); (H + 2) (W + 2) > PP_PROBMAP_LOSS_MAX_TILE floats,
 * the LDS stage (UNSUPPORTED). B = 0 returns PP_OK untouched. */
#define PP_PROBMAP_LOSS_MAX_TILE 15360
int pp_probmap_loss_maps(const float* pred, const float* target, const float* weights, int B, int K, int H, int W,
                         double smoothing_weight, double gaussian_weight, double loss_weight, double* map_sums, int32_t* argmax,
                         float* maxval, float* loss, void* stream);

/* pp_probmap_loss_scalars: the scalar targets and the four scalar losses of ProbMapHead.loss (probmap_head.py:830-941) in ONE launch
 * ("probmap_loss_scalars", one workgroup, fixed trees). Inputs on the device: scalars (4, B, K) float32 = the predicted probability,
 * visibility, oks and error; in_image, annotated (keypoints_visible.astype(int)) and visibility (keypoints_visibility.astype(int))
 * (B, K) uint8, each 0 or 1; kp_gt and kp_dt (B, K, 2) float64 = the target and the predicted maps decoded by pp_udp_heatmap_decode
 * (ArgMaxProbMap.decode, the head's fast_decoder). loss_weights_host: four doubles on the HOST (probability, visibility, oks, error).
 * Outputs on the device:
 *   gt_oks (B, K) float32   _oks_from_heatmaps: NaN target coordinates -> 0, both coordinate sets times w = in_image & annotated,
 *                           exp(-(dx^2 + dy^2) / (2 sigma_k)^2 / (64 * 48 * 0.53 + spacing(1)) / 2) (compute_oks, use_area=False,
 *                           per_kpt=True, the sigmas / 10), 0 where w = 0; an instance without any w = 1 gets zeros and
 *   oks_weight (B) float32  0, every other 1. PP_LOSS_FREEZE_OKS: all zeros.
 *   gt_errs (B, K) float32  _error_from_heatmaps: ||gt - dt||, NaN target coordinates -> -1; PP_LOSS_FREEZE_ERROR: zeros.
 *   vis_weights (B, K) float32  the class-balanced weights of :883-889 (1 / count of annotated invisible resp. visible keypoints,
 *                           formed in float32, divided by the smallest positive one; 0 where not annotated).
 *   out[6] float32          loss_probability = mean(BCE(p, in_image) * annotated), loss_visibility = mean(BCE(v, visibility) *
 *                           vis_weights), loss_oks = mean((o w - gt_oks w)^2), loss_error = mean(smooth_l1(log(1 + e) w,
 *                           log(1 + gt_errs) w)) - means over B K, times their loss weights -, mae_oks, mae_err = mean |.| over w = 1
 *                           (NaN when no keypoint has w = 1). BCE is torch's binary_cross_entropy (logs clamped at -100), with
 *                           PP_LOSS_PROB_LOGITS / PP_LOSS_VIS_LOGITS binary_cross_entropy_with_logits. Elementwise values and sums
 *                           are fp64 from the float32 inputs. A batch without any annotated keypoint has loss_visibility 0 (the
 *                           reference raises on the empty minimum).
 * Status instead of a launch: NULL pointers, B < 0, K <= 0, unknown flags, K != 17 (INVALID_ARG). B = 0 returns PP_OK untouched. */
#define PP_LOSS_FREEZE_OKS 1
#define PP_LOSS_FREEZE_ERROR 2
#define PP_LOSS_PROB_LOGITS 4
#define PP_LOSS_VIS_LOGITS 8
int pp_probmap_loss_scalars(const float* scalars, const unsigned char* in_image, const unsigned char* annotated,
                            const unsigned char* visibility, const double* kp_gt, const double* kp_dt, int B, int K, int flags,
                            const double* loss_weights_host, float* gt_oks, float* oks_weight, float* gt_errs, float* vis_weights,
                            float* out, void* stream);

/* ---- following persons through a video (csrc/pp_track.hip, csrc/pp_track_core.h; probpose_code_amd/tracking.py) ------------------------
 * pp_track_update: the person boxes of the next frame from this frame's poses, in ONE launch ("track_update") of one 64-lane
 * workgroup, lane i = track i. Inputs on the device: records (n, K, 7) float64 = x, y, conf, prob, vis, oks, err in crop space as
 * pp_pack_records leaves them; centers, scales (n, 2) float32 the crops were cut with; sigmas (K) float64 of the dataset; the track
 * state boxes_in (n, 4) float32 xyxy, alive_in, lost_in (n) int32. Per alive track: keypoints to image space as
 * TopdownPoseEstimator.add_pred_to_datasample maps them, x / input_w * scale + centre - 0.5 * scale in float64 (0.5 * scale a float32
 * product); a keypoint is selected when its gate - the prob column (PP_TRACK_GATE_PROB) or the conf column (PP_TRACK_GATE_CONF) - is
 * finite and >= kpt_thr and its coordinates are finite. With at least min_keypoints selected: the min/max box of the selected
 * keypoints, grown about its centre by expand with each side at least min_side, smooth * old + (1 - smooth) * new (smooth = 0: the
 * new box itself), rounded to float32; lost = 0. Otherwise the box is kept, lost + 1, and beyond max_lost alive = 0 for good.
 * Duplicates: every two tracks updated in this frame whose image-space poses have an OKS (mmpose/evaluation/functional/nms.py
 * oks_iou, all K keypoints, the mean area of the two new boxes) above dup_oks_thr, visited in the order (0,1) (0,2) .. (1,2) ..: of
 * two tracks still alive the one with the lower mean gate over its selected keypoints dies, the higher index on a tie. Dead and free
 * slots keep box and lost count. Outputs boxes_out, alive_out, lost_out may be the inputs (a lane touches its own rows only).
 * next_centers, next_scales (n, 2) float32 and next_maps (n, 2, 3) float64, given together or all NULL: pp_track_affine_params of
 * boxes_out, fused into the launch; they may be centers / scales.
 * Float64 throughout, one rounding per operator, sums over K through one fixed tree, no atomics: the same bits launch after launch,
 * and the host form's bits up to exp() (an OKS within a few ulp of dup_oks_thr may be decided either way).
 * Status instead of a launch (PP_ERR_INVALID_ARG): NULL pointers, n outside 1..PP_TRACK_MAX_TRACKS, K outside
 * 1..PP_TRACK_MAX_KEYPOINTS, an input side outside 2..32767, an unknown gate, NaN thresholds, min_keypoints < 1, expand or min_side or
 * input_padding not positive and finite, smooth outside [0, 1), max_lost < 0.
 *
 * pp_track_affine_params ("track_affine_params", the same kernel without the update): for boxes (n, 4) float32 xyxy the centres and
 * scales (n, 2) float32 of bbox_xyxy2cs(padding = input_padding) + TopdownAffine._fix_aspect_ratio(w / h) and the dst -> src maps
 * (n, 2, 3) float64 pp_warp_affine_u8 reads: get_udp_warp_matrix at rot = 0 in float32 as numpy promotes it, inverted in float64 as
 * cv2.warpAffine does - bit for bit transforms.topdown_affine_params + transforms.invert_affine. use_udp = True pipelines only. */
#define PP_TRACK_MAX_TRACKS 64
#define PP_TRACK_MAX_KEYPOINTS 256
#define PP_TRACK_GATE_PROB 0
#define PP_TRACK_GATE_CONF 1
int pp_track_update(const double* records, const float* centers, const float* scales, int n, int K, int input_w, int input_h,
                    int gate, const double* sigmas, const float* boxes_in, const int32_t* alive_in, const int32_t* lost_in,
                    double kpt_thr, int min_keypoints, double expand, double min_side, double smooth, int max_lost,
                    double dup_oks_thr, float* boxes_out, int32_t* alive_out, int32_t* lost_out, double input_padding,
                    float* next_centers, float* next_scales, double* next_maps, void* stream);
int pp_track_affine_params(const float* boxes, int n, int input_w, int input_h, double input_padding, float* centers, float* scales,
                           double* maps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PROBPOSE_MI355X_H_ */
