/*
 * said_unet_finetune.h — fine-tuning the Wav2Vec2 transformer together with the denoiser: the entry points that a said_unet_train context
 * (include/said_unet_train.h, whose conventions hold here) gains for it.  Kernels: said_amd/csrc/audio_ft.hip; host: unet_trainer.cpp.
 *
 * The reference leaves one training variant open: beside the loop that freezes every encoder parameter, its script/train.py holds the commented
 * `said_model.audio_encoder.freeze_feature_encoder()`, which freezes the seven convolutions and trains the feature projection, the positional
 * convolution and the transformer layers with the denoiser (the paper's "finetune_wav2vec" ablation).
 *
 * A context made by said_unet_train_create_ft with finetune_layers = L >= 1 trains an L-layer wav2vec2-base encoder that way.  Its table is the
 * one of said_unet_train_create_dim followed by "audio_encoder.*" without "audio_encoder.feature_extractor.*", in state-dict order with the
 * transformers 4.30.2 key layout: masked_spec_embed, feature_projection.layer_norm.*, feature_projection.projection.*,
 * encoder.pos_conv_embed.conv.{bias, weight_g, weight_v}, encoder.layer_norm.*, then the 16 tensors of each layer.  They live in the context's
 * one store: the gradient norm and the clip run over denoiser and encoder jointly, as clip_grad_norm_(said_model.parameters(), 1.0) does, and
 * AdamW, the EMA, the stash, set_tensor, get_tensor, copy and reset_optimizer cover them with the rest.
 *
 * Such a context takes `features` (B, T, 512), the frozen extractor's output after the interpolation to T frames (said_audio_extract_features,
 * said_amd/csrc/said_audio_features.h), through the _ft entry points below; the entry points of said_unet_train.h that take an audio embedding refuse
 * it, and the _ft ones refuse a context without a fine-tuned encoder.  The encoder runs in fp32, token-major.  Its forward is that of
 * said_audio_encode_train (include/said_audio_train.h), in that order and with the same Philox key, counters and sites, so the same
 * (seed, mask, skip_layers) give the same masks.  Then audio_proj_layer when feature_dim > 0, the select against null_cond_emb, and the UNet's
 * forward, loss and backward; then the conditional samples' rows of the context gradient (through W_proj when feature_dim > 0) go back through the
 * encoder down to feature_projection.layer_norm.  Nothing flows into `features`.  A skipped layer's gradients are exact zeros; an unconditional
 * sample sends exact zeros into the encoder (its rows still run the forward); masked_spec_embed's gradient is exact zeros without a mask; no
 * gradient is accumulated across steps.  One update (clip, AdamW, EMA) over everything follows.  Every sum runs in a fixed order: equal inputs
 * give equal bits.
 *
 * finetune_layers <= 0 is said_unet_train_create_dim: the same tables, the same launches, the same bits.
 */
#ifndef SAID_UNET_FINETUNE_H
#define SAID_UNET_FINETUNE_H

#include "../../include/said_audio_train.h"
#include "../../include/said_unet_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the width of `features` and the largest finetune_layers (said_audio_train_params.skip_layers holds 32 layers) */
enum { SAID_UT_FEATURE_WIDTH = 512, SAID_UT_MAX_FINETUNE_LAYERS = 32 };

/* said_unet_train_create_dim with a fine-tuned encoder of finetune_layers layers; above SAID_UT_MAX_FINETUNE_LAYERS fails with a message */
int said_unet_train_create_ft(said_unet_train** out, int device, int max_batch, int max_frames, int feature_dim, int finetune_layers);
/* the table of (feature_dim, finetune_layers) without a context or a device: its size (-1 above either maximum), the i-th name and count */
int said_unet_train_table_size_ft(int feature_dim, int finetune_layers);
const char* said_unet_train_table_name_ft(int feature_dim, int finetune_layers, int i);
long long said_unet_train_table_numel_ft(int feature_dim, int finetune_layers, int i);
/* a context's fine-tuned layer count (0: the encoder is frozen and its output an input) */
int said_unet_train_finetune_layers(const said_unet_train* t);

/* said_unet_train_step / _eval_loss / _forward_only for a fine-tuning context.  `features` (B, T, 512) fp32 token-major, in host memory or, when
 * features_on_device, in device memory, replaces the audio embedding.  params (nullable): the encoder's train mode as said_audio_encode_train
 * takes it (time_mask_dev (B, T) is copied before the call returns); null: eval mode.  eval_loss_ft and forward_only_ft always run the encoder in
 * eval mode, whatever params holds, and with ema != 0 on the EMA copy of encoder and denoiser. */
int said_unet_train_step_ft(said_unet_train* t, int B, int T, const float* coeffs_host, const float* noise_host, const long long* timesteps_host,
                            const int* cond_host, const void* features, int features_on_device, const said_audio_train_params* params,
                            unsigned long long dropout_seed, const float* scalars_host, const float* std_host, const float* deltas_host, int V);
int said_unet_train_eval_loss_ft(said_unet_train* t, int B, int T, const float* coeffs_host, const float* noise_host, const long long* timesteps_host,
                                 const int* cond_host, const void* features, int features_on_device, const said_audio_train_params* params,
                                 const float* scalars_host, const float* std_host, const float* deltas_host, int V, int ema);
int said_unet_train_forward_only_ft(said_unet_train* t, int B, int T, const float* sample_host, const long long* timesteps_host, const int* cond_host,
                                    const void* features, int features_on_device, const said_audio_train_params* params, int ema, float* out_host);
/* the conditioning (B, T, context width) that the denoiser saw in the last _ft call, which had this shape: the encoder's output (projected when
 * feature_dim > 0) in the conditional samples' rows, null_cond_emb in the others */
int said_unet_train_last_conditioning(said_unet_train* t, int B, int T, float* out_host);

#ifdef __cplusplus
}
#endif
#endif /* SAID_UNET_FINETUNE_H */
