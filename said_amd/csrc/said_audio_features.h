/*
 * said_audio_features.h — the audio encoder's frozen front end as a callable (said_amd/csrc/audio_enc.cpp), in libsaid_hip.so beside include/said_hip.h,
 * whose conventions hold.  What a trainer context that fine-tunes the Wav2Vec2 transformer takes as its input (said_amd/csrc/said_unet_finetune.h).
 */
#ifndef SAID_AUDIO_FEATURES_H
#define SAID_AUDIO_FEATURES_H

#include "../../include/said_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The seven convolutions and the interpolation to num_frames (<= 0: none) of said_audio_encode's fp32 route, then a transposing store:
 * out_dev (batch, frames, 512) fp32 token-major; *out_frames (nullable) = frames.  A context in SAID_PREC_BF16 refuses the call, as
 * said_audio_encode_train does. */
int said_audio_extract_features(said_ctx* ctx, const float* waveform_dev, int batch, int num_samples, int num_frames, float* out_dev,
                                int* out_frames, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAID_AUDIO_FEATURES_H */
