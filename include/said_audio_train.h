/*
 * said_audio_train.h — C ABI of the audio encoder's train mode (said_amd/csrc/audio_train.hip, audio_enc.cpp), in libsaid_hip.so beside said_hip.h.
 *
 * The reference trains its denoiser with the frozen Wav2Vec2 left in train() mode (script/train.py:204), so the conditioning passes through
 * SpecAugment time masking, four dropouts and LayerDrop (transformers 4.30.2, post-LN encoder).  said_audio_encode_train is said_audio_encode's
 * fp32 channel-major route with those steps added, in this order:
 *   h = dropout(Linear(LN(x)), p_feat_proj);  h[b, t, :] = masked_spec_embed where time_mask[b, t];  h = dropout(LN(h + pos_conv(h)), p_hidden);
 *   per layer l unless bit l of skip_layers is set:
 *     a = out_proj(softmax(q k^T scale) * keep / (1 - p_attention) . v)          (the softmax denominator sums the undropped terms)
 *     h = LN1(h + dropout(a, p_hidden));  f = W2 dropout(GELU(W1 h + b1), p_activation) + b2;  h = LN2(h + dropout(f, p_hidden))
 * then audio_proj_layer with apply_proj != 0.  The span mask and the skip decisions are the host's draws; the dropout masks are generated on the
 * device: Philox4x32-10, key = seed, u = (word >> 8) 2^-24, kept iff u >= p, a kept element multiplied by the fp32 value of 1 / (1 - p).
 *   element-wise sites: e = logical index in (B, T, C); counter (site, e >> 2, 0, 0), word e & 3
 *   attention probabilities: counter (site, (b 12 + head) T + i, j >> 2, 0), word j & 3 (query i, key j)
 *   site: 0 feature projection, 1 encoder front, 16 + 4 l + {0 probabilities, 1 attention output, 2 activation, 3 FFN output} for layer l
 * A mask depends on (seed, site, logical index) only: not on the audio chunk size, the key split or any tiling.  Calls whose indices would need
 * 2^32 or more are refused.  A context in SAID_PREC_BF16 refuses the call; under SAID_PREC_FP32 / _STRICT the products multiply as in
 * said_audio_encode.  Conventions are those of said_hip.h.
 */
#ifndef SAID_AUDIO_TRAIN_H
#define SAID_AUDIO_TRAIN_H

#include <stdint.h>

#include "said_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    float p_feat_proj, p_hidden, p_attention, p_activation;   /* each in [0, 1) */
    uint64_t seed;
    const uint8_t* time_mask_dev;   /* (B, frames), non-zero = masked; may be null.  Needs audio_encoder.masked_spec_embed */
    uint32_t skip_layers;           /* bit l set: layer l skipped */
} said_audio_train_params;

int said_audio_encode_train(said_ctx* ctx, const float* waveform_dev, int batch, int num_samples, int num_frames, int apply_proj,
                            const said_audio_train_params* params, float* out_dev, int* out_frames, void* stream);

#ifdef __cplusplus
}
#endif
#endif
