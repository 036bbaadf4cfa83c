// audio_train.h — launch-level interface of audio_train.hip: the kernels that said_audio_encode_train adds to the fp32 channel-major
// audio encoder (include/said_audio_train.h states the semantics, the Philox counters and the site ids).
#pragma once
#include "kernels.h"

namespace said {

// site ids of the dropout masks
constexpr int AT_SITE_FEAT_PROJ = 0, AT_SITE_FRONT = 1;
constexpr int at_site_layer(int l, int which) { return 16 + 4 * l + which; }   // which: 0 probabilities, 1 attention output, 2 activation, 3 FFN output

// One dropout mask: the Philox key, the site, p and the fp32 value of 1 / (1 - p).  p == 0: no mask is drawn.
struct DropSite {
    unsigned long long seed;
    int site;
    float p, keep;
};
inline DropSite drop_site(unsigned long long seed, int site, float p) { return DropSite{seed, site, p, 1.0f / (1.0f - p)}; }

// Self-attention of the audio encoder (head_dim 64) with dropout on the normalised probabilities: launch_attn's operand layouts and
// key split (KS = 8 or 4), mode 0 (fp32 MFMAs) or 2 (split-fp16 operands); channel-major fp32 output.  b_global: the call-wide index
// of the launch's first clip (a.b0 must be 0).
void launch_attn_drop(const AttnArgs& a, int batch, int KS, hipStream_t s, int mode, int b_global, const DropSite& d);
void configure_audio_train_kernels();

// y[b][c][t] = post(LN_c(res[b][c][t] + pre(x[b][c][t]))) on channel-major tensors; pre / post are dropout masks over the logical
// (B, T, C) index (either may have p == 0).  C % 4 == 0.
void launch_ln_drop_cm(const float* x, const float* res, float* y, const float* gamma, const float* beta, int B, int C, int T, int pitch,
                       long long bstride, float eps, int b_global, const DropSite& pre, const DropSite& post, hipStream_t s);

// In place on a channel-major tensor: x = dropout(x), then x[b][:][t] = embed[:] wherever mask[b][t] != 0 (mask: (B, T) bytes of THIS
// launch's clips, or null).  C % 4 == 0.
void launch_drop_cm(float* x, int B, int C, int T, int pitch, long long bstride, int b_global, const DropSite& d, const unsigned char* mask,
                    const float* embed, hipStream_t s);

}  // namespace said
