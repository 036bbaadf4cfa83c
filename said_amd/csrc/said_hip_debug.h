/*
 * said_hip_debug.h — development / test entry points of libsaid_hip.so.  NOT part of the reference-facing boundary (include/said_hip.h): nothing in
 * said_amd/model, script/ or bench.py's measured path needs them; tests/ and scripts/ use them to pin a schedule, read internal buffers, stamp clocks.
 * Same conventions as said_hip.h (0 = success, said_last_error for the message).
 */
#ifndef SAID_HIP_DEBUG_H
#define SAID_HIP_DEBUG_H

#include "../../include/said_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test-only switches of one context (the library reads no environment variables; an unknown name fails):
 *   "unet_tgemm_min_tokens"  tokens per launch from which the UNet takes the token-major GEMM path, both precisions
 *                            (< 0: restore the measured defaults 3000 bf16 / 10000 fp32)
 *   "audio_chunk"            clips per audio-encoder pass (default 32)
 *   "audio_train_sites"      said_audio_encode_train: bit mask of the kinds of dropout site that draw a mask (1 feature projection, 2 encoder front, 4 attention probabilities,
 *                            8 attention output, 16 activation, 32 FFN output); the others run with p = 0.  < 0 (default): all.  The three sites of p_hidden can be told apart this way.
 *   "audio_stop_after"       n >= 0 makes said_audio_encode (and said_audio_extract_features) issue only the first n stages of each pass and return 0 (the output is then
 *                            undefined; the buffers hold the intermediates: said_debug_audio_copy); < 0 (default): everything.  Host side only; said_audio_encode_train ignores
 *                            it.  A stage is one launch site, asked whether or not it launches.  bf16 mode, the bf16 branch's sites in order:
 *                              0 conv0 + GroupNorm + GELU, 1-6 the strided convolutions, 7 interpolation + LayerNorm, 8 feature projection, 9 tm_to_group_bf16,
 *                              10 positional convolution, 11 encoder LayerNorm; layer l from 12 + 8 l: +0 q/k/v, +1 attention, +2 cm_to_tm_bf16 (a stage of its own also where the
 *                              key-split-free attention stores token-major itself and nothing is launched), +3 out_proj, +4 LayerNorm, +5 ff1, +6 ff2, +7 final LayerNorm;
 *                              then audio_proj_layer.  (Without the packed positional weights: 9 tm_to_cm, 10 the grouped fp32 convolution + cm_to_tm, 11 LayerNorm.)
 *                            fp32 modes, the fp32 branch's sites in order:
 *                              0 conv0, 1 per-channel GroupNorm + GELU, 2-7 the strided convolutions, 8 interpolation (a stage of its own also where no frame count is given and
 *                              nothing is launched), 9 feature projection (LayerNorm in its operand transform), 10 positional convolution, 11 encoder LayerNorm; layer l from
 *                              12 + 7 l: +0 q/k/v, +1 attention, +2 out_proj + residual, +3 LayerNorm, +4 ff1, +5 ff2 + residual, +6 final LayerNorm; then audio_proj_layer (only
 *                              with apply_proj), then the final cm_to_tm.  said_audio_extract_features: its cm_to_tm store is stage 9, and the last.
 *   "steps_per_graph"        denoise steps captured per hipGraph in loops of >= 400 steps (default 50; until round 6: 10); shorter loops: min(this, 10)
 *   "tm_acts"                bf16 mode, large batches: token-major bf16 activations between the UNet kernels, GroupNorm / LayerNorm applied inside the consuming
 *                            GEMMs (-1 / 1, default); 0: channel-major fp32 activations with preparation kernels (round 2).  (The fp32 twin of the schedule, measured
 *                            slower in round 3, was removed in round 6.)
 *   "tgemm_direct"           0: the bf16 audio encoder's projections on tgemm_kernel<128, 128> (rounds 2-5); -1 / 1 (default): on tgemm256d_kernel — 256 x 256 x 64 tile, operand tiles
 *                            loaded global -> LDS directly, XOR-swizzled chunks, one barrier per k-tile (round 6; bit-identical)
 *   "out_tm"                 0: bf16 large batches end the step with round 3's channel-major out conv + scheduler kernel (default -1: out_sched_tm_kernel)
 *   "gemm_presplit"          fp32 mode, large batches: 0 = fgemm_kernel splits fp32 operands in its k loop (round 5); -1 / 1 (default): the ResBlock convolutions' and q / k / v's
 *                            operands arrive split (prep_kernel packs h | l pairs, packed weight copies; bit-identical, round 6)
 *   "gemm_split"             fp32 mode, large batches: 0 puts fgemm_kernel back on v_mfma_f32_32x32x2_f32 (default -1 / 1: split-fp16 products)
 *   "attn_split"             fp32 mode: 0 puts both self-attention products back on fp32 MFMAs (default -1 / 1: split-fp16 products)
 *   "ugemm_split"            fp32 mode, channel-major GEMMs (ugemm_kernel): 0 = fp32 MFMAs (default -1 / 1: split-fp16 products, round 5)
 *   "chain_coef"             fp32 mode, small batch: 0 = stchain_kernel finalises the block input's GroupNorm coefficients from the partials itself; -1 / 1 (default): it reads the
 *                            coefficients the q/k/v GEMM of the same block finalised and left behind (GemmCommon::gn_coef_out, round 6)
 *   "kconv"                  fp32 mode, small batch: 0 = the K-long ResBlock convolutions of the up path (two / three K segments) keep ugemm_body's block loop; -1 / 1 (default):
 *                            kconv_body's straight-line blocks (round 6; bit-identical); 2: also under concurrent clip groups where the chosen column-tile count has no split shape
 *                            (4 / 5 / 6 / 7 / 8 clips: -0.3 / -1.1 / +4.6 / -0.1 / +0.2 %: not the default)
 *   "attn_2q"                fp32 mode, pre-split K / V, four key slices: 0 = one query tile per wave always; 1 = three always; -1 (default) = three from 512 (sample, head, query tile)
 *                            triples per launch on (attn2q_kernel: long sequences at small batch; bit-identical)
 *   "attn_presplit"          fp32 small batch: 0 = attention splits K / V itself (default -1 / 1: the q/k/v GEMM stores them pre-split, attn_kernel<PM = 3>)
 *   "out_split"              out_sched_kernel's convolution: 0 = fp32 MFMAs (default -1 / 1: split-fp16 products, round 5)
 *   "st_chain"               fp32 mode: 0 runs everything behind a SpatialTransformer's self-attention as five launches (rounds 1-4); default -1 / 1:
 *                            one launch per block (stchain_kernel, round 5)
 *   "st_chain_slices"        fp32 mode, fused tail: 1 = always one workgroup per token tile; -1 / 3 (default) = launches of at most 85 (sample, tile) pairs run three
 *                            workgroups per tile, each with a third of the GEGLU / folded proj_out weight stream, partial sums met in memory in a fixed order (round 6)
 *   "st_chain_bf16"          bf16 mode, large batches: 0 = rgemm's six launches behind self-attention; -1 / 1 (default) = stchain_kernel<bf16>, one token tile per workgroup,
 *                            two workgroups per CU
 *   "xgemm_clk"              1: shader-clock stamps of the token-major schedule's kernels (-DSAID_CLK_STAMPS builds; read with said_debug_clocks)
 * said_debug_get additionally knows "n_set_weight" (said_set_weight calls so far), "n_stchain" / "n_rgemm" / "n_xgemm" (launches issued through those kernels)
 * and "n_out_sched" / "n_out_sched_tm" / "n_sched_step" (the same for the step's last kernel: out_sched_kernel, out_sched_tm_kernel, sched_step_kernel);
 * of the bf16 audio encoder: "n_tgemm_128" / "n_tgemm_128sb" / "n_tgemm_128x64" / "n_tgemm_256" / "n_tgemm_256x192" / "n_tgemm_256d" (its GEMM launches per kernel: tgemm.h
 * TGemmVariant) and "n_audio_attn_ks8" / "n_audio_attn_tm" (attention launches with eight key slices / without key split and with the token-major bf16 store);
 * of the fp32 audio encoder: "n_audio_attn_f32_ks8" / "n_audio_attn_f32_ks4" / "n_audio_attn_f32_ks1" (attention launches with eight / four key slices / without key split:
 * audio_plan.h attn_slices). */
int said_debug_option(said_ctx* ctx, const char* name, long long value);
long long said_debug_get(const said_ctx* ctx, const char* name);
/* Stop the UNet schedule after `n_launches` kernel launches, counted from the start of each said_unet_forward / said_denoise_loop call (< 0: run
 * everything).  In a loop call only the eager warm-up step then runs (its first n launches); the workspace afterwards holds that step's intermediates
 * (tests/test_gpu_round5.py reads the last hidden state this way). */
int said_debug_stop_after(said_ctx* ctx, int n_launches);
/* Enable/disable per-phase shader-clock stamps in the GEMM kernels of the next UNet evaluations and
 * (if out_host != NULL) read back the [64 launches][8 waves][8 slots] stamp table. */
int said_debug_clocks(said_ctx* ctx, int enable, long long* out_host);
/* Synchronously copy `n` floats from the start of the named internal buffer
 * ("H0","H1","P","Q","M","X1","X2","X3","O","QK","VT","F","KV","CTX","EO","E0","E1","E2",
 *  "x","eps","stH0","stP","stM", ...) to host memory. */
int said_debug_read(said_ctx* ctx, const char* name, float* out_host, int64_t n);
/* Workspace inspection (race hunting, round 5): the context's (max_batch_eff, max_frames)-sized buffers by allocation index.
 * _info: device pointer, size in bytes and a short name ("H0", "uPA", ..., "?" if unnamed) of buffer `idx`;
 * _fill: synchronises the device and sets EVERY byte of every workspace buffer to `byte_value` (0xFF: NaN patterns; drops the step graph
 *        and the cached band tables) — a result that changes with the fill value is a read of memory nobody wrote;
 * _copy: enqueues a device-to-device copy of the first `bytes` bytes of buffer `idx` to `dst_dev` on `stream`. */
int said_debug_ws_count(const said_ctx* ctx);
int said_debug_ws_info(said_ctx* ctx, int idx, void** ptr_out, long long* bytes_out, const char** name_out);
int said_debug_ws_fill(said_ctx* ctx, int byte_value);
int said_debug_ws_copy(said_ctx* ctx, int idx, void* dst_dev, long long bytes, void* stream);
/* The audio encoder's lazily sized buffers are not in that list.  Enqueues a device-to-device copy of the first `bytes` bytes of the named one — bf16 mode's token-major
 * buffers "bA0" "bA1" (feature-extractor ping-pong, bf16) "bX" (interpolated + normalised features, bf16) "bXg" (per-group positional-conv operand, bf16) "bH" (hidden state, fp32)
 * "bHb" (its bf16 copy) "bT" (GEMM results before LayerNorm, fp32) "bF" (feed-forward activation, bf16) "bO" (attention output, bf16) "bPosT", and the attention buffers "aQK"
 * "aVT" "aO" (fp32), and fp32 mode's channel-major buffers (fp32, [clip][channel][pitch], pitch = frames rounded up to 32): "abufA" "abufB" (feature-extractor ping-pong) "aX"
 * (interpolated features) "aH" (hidden state) "aT" (GEMM results before LayerNorm; the audio_proj_layer output) "aF" (feed-forward activation) "aPOS" (positional convolution) — to
 * `dst_dev` on `stream`.  Fails on an unknown name, a buffer no call has allocated yet, or more bytes than it holds. */
int said_debug_audio_copy(said_ctx* ctx, const char* name, void* dst_dev, long long bytes, void* stream);
/* Synchronises the device and sets EVERY byte of every allocated audio-encoder buffer (all the names above, fp32 and bf16 set alike) to `byte_value`: what said_debug_ws_fill
 * is for the workspace.  An encode whose result changes with the fill value reads memory nobody wrote (pad rows frames .. pitch, or what an earlier, larger encode left). */
int said_debug_audio_fill(said_ctx* ctx, int byte_value);

#ifdef __cplusplus
}
#endif
#endif /* SAID_HIP_DEBUG_H */
