// audio_ft.h — launchers of the kernels that fine-tuning the Wav2Vec2 transformer adds to the UNet trainer (audio_ft.hip): the encoder's
// forward in fp32, token-major, saving what its backward needs, and that backward.  The matrix products are ut::gemm's (unet_train.h).
// The dropout masks are those of include/said_audio_train.h (same key, counters and sites), recomputed in the backward and never stored.
// No kernel uses atomics; every sum runs in a fixed order, so equal inputs give equal bits.
#pragma once
#include <hip/hip_runtime.h>

namespace said {
namespace aft __attribute__((visibility("hidden"))) {

// one dropout mask: the Philox key, the site, p and the fp32 value of 1 / (1 - p); p == 0: no mask is drawn
struct Drop { unsigned k0, k1; int site; float p, keep; };
inline Drop drop(unsigned long long seed, int site, float p) {
    return Drop{(unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32), site, p, 1.0f / (1.0f - p)};
}

// LayerNorm over the C (512 or 768) channels of each of M rows of v = res + pre(x) (res nullable), y = post(xhat gamma + beta); pre / post
// are element-wise dropout masks over the logical index m C + c.  Saves xhat (M, C) and rstd (M).
void ln_fwd(hipStream_t s, int M, int C, const float* x, const float* res, const float* gamma, const float* beta, const Drop& pre, const Drop& post,
            float* xhat, float* rstd, float* y);
// The backward: du = post(dy) (nullable; the caller's column sums give dgamma = sum du xhat and dbeta = sum du), dres (+)= the gradient at v,
// dpre (nullable) = pre(that gradient), the gradient at x.
void ln_bwd(hipStream_t s, int M, int C, const float* dy, const float* xhat, const float* rstd, const float* gamma, const Drop& pre, const Drop& post,
            float* du, float* dres, int accumulate, float* dpre);
// u[m][c] += bias[c] over (M, C): where the GEMM's epilogue cannot add it (the grouped positional convolution)
void add_bias(hipStream_t s, int M, int C, const float* bias, float* u);
// y = drop(gelu(u)) (erf GELU) over n elements, n % 4 == 0
void gelu_drop_fwd(hipStream_t s, long long n, const float* u, const Drop& d, float* y);
// du = drop(dy) gelu'(u)
void gelu_drop_bwd(hipStream_t s, long long n, const float* u, const float* dy, const Drop& d, float* du);
// Pd = P * keep factors of the attention probabilities: row r = (b heads + head) T + i, key j is word j & 3 of counter (site, r, j >> 2, 0).
// In place when Pd == P.
void prob_drop(hipStream_t s, long long rows, int T, const float* P, const Drop& d, float* Pd);
// h[m][:] = mask[m] ? embed[:] : drop(x[m][:]) over (M, C) (mask nullable)
void mask_drop_fwd(hipStream_t s, int M, int C, const float* x, const unsigned char* mask, const float* embed, const Drop& d, float* h);
// dx[m][:] = mask[m] ? 0 : drop(dh[m][:]); dmasked[m][:] = mask[m] ? dh[m][:] : 0 (mask and dmasked nullable together)
void mask_drop_bwd(hipStream_t s, int M, int C, const float* dh, const unsigned char* mask, const Drop& d, float* dx, float* dmasked);
// weight_norm(dim = 2) of v (O, I, K) with g (K): norm[k] = |v[:, :, k]|, w = g v / norm.  O I % WN_SEG == 0; part: WN_SEG K floats of scratch
constexpr int WN_SEG = 64;
void weight_norm_fwd(hipStream_t s, int OI, int K, const float* g, const float* v, float* part, float* norm, float* w);
// dg[k] = <dw, v> / norm; dv = g / norm (dw - dg v / norm); dot: K floats of scratch
void weight_norm_bwd(hipStream_t s, int OI, int K, const float* g, const float* v, const float* norm, const float* dw, float* part, float* dot,
                     float* dg, float* dv);

}  // namespace aft
}  // namespace said
