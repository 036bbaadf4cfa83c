// vae_train.h — launchers of the BCVAE training kernels (vae_train.hip), called by the trainer context (vae_trainer.cpp).
// Every launcher enqueues on `s` and only enqueues (no allocation, no copy, no sync): a step is captured into a hipGraph as it is.
// Activations are fp32; an activation element (b, c, t) lives at b * sb + c * sc + t * st.
#pragma once
#include <hip/hip_runtime.h>

namespace said {
namespace vt __attribute__((visibility("hidden"))) {

// per-step scalars, written by the host into the step record before each step (include/said_train.h SAID_TRAIN_S_*)
enum { S_LR = 0, S_WD_FACTOR, S_STEP_SIZE, S_BC2_SQRT, S_EMA_OMD, S_BETA, S_WVEL, S_OMB1, S_B2, S_OMB2, S_EPS, S_USE_EMA, S_USE_STD, NSCAL = 16 };
// accumulated losses (double): reconst * B, regularize * B, velocity * B, total * B, samples, non-finite steps
enum { A_RECONST = 0, A_REG, A_VEL, A_TOTAL, A_COUNT, A_BAD, NACC = 8 };
constexpr int C = 32, T = 120, Z = 64, ITEM = 4;   // channels, window, latent, ints per batch item (seq, bdx, flip, zero)

struct TAct { const float* p; int sb, sc, st; };
struct TActW { float* p; int sb, sc, st; };

// x[b][t][c] = data[off[seq] + clamp(bdx + t, 0, len[seq] - 1)][flip ? mirror[c] : c], or 0 when the item's zero flag is set
void gather(hipStream_t s, int B, const float* data, const long long* off, const int* len, const int* items, const int* mirror, float* x);
// Conv1d (W [Co][Ci][K], stride S) or, transposed != 0, ConvTranspose1d with stride 1 (W [Ci][Co][K]); y = bias + sum, fixed order
void conv_fwd(hipStream_t s, int transposed, int B, int Ci, int Co, int K, int S, int Lin, int Lout, TAct x, const float* W, const float* bias, TActW y);
// dx of the same layers (dy -> dx)
void conv_bwd_data(hipStream_t s, int transposed, int B, int Ci, int Co, int K, int S, int Lin, int Lout, TAct dy, const float* W, TActW dx);
// dW and dbias: one wave per weight, its B x L products summed lane-strided and then by a fixed butterfly
void conv_bwd_weight(hipStream_t s, int transposed, int B, int Ci, int Co, int K, int S, int Lin, int Lout, TAct x, TAct dy, float* dW, float* dbias);
// y[b][o] = bias[o] + sum_i W[o][i] x[b][i]
void linear_fwd(hipStream_t s, int B, int In, int Out, const float* x, const float* W, const float* bias, float* y);
// dx[b][i] = sum_o W[o][i] dy[b][o] (+ sum_o W2[o][i] dy2[b][o] when W2 is given)
void linear_bwd_data(hipStream_t s, int B, int In, int Out, const float* dy, const float* W, const float* dy2, const float* W2, float* dx);
// dW[o][i] = sum_b dy[b][o] x[b][i], dbias[o] = sum_b dy[b][o]
void linear_bwd_weight(hipStream_t s, int B, int In, int Out, const float* x, const float* dy, float* dW, float* dbias);
// BatchNorm1d + LeakyReLU(slope) over B x L per channel.  train: batch statistics (biased variance), running stats updated with momentum 0.1
// and the unbiased variance; stats[0..Cn) mean, [Cn..2Cn) invstd.  eval: running statistics.  xhat and h are written in the layout of `a`.
void bn_fwd(hipStream_t s, int train, int B, int Cn, int L, TAct a, const float* gamma, const float* beta, float* rmean, float* rvar, float* stats,
            float slope, float* xhat, float* h);
// the backward of the above (training mode): dgamma, dbeta and da from dh
void bn_bwd(hipStream_t s, int B, int Cn, int L, TAct dh, TAct h, TAct xhat, const float* gamma, const float* stats, float slope, float* dgamma,
            float* dbeta, TActW da);
// z = mu + exp(0.5 lv) eps
void reparam(hipStream_t s, int B, const float* mu, const float* lv, const float* eps, float* z);
// ELBO losses of the batch (rec: x, u time-major (B, 120, 32); y = tanh(relu(u))); du (nullable) = d total / d u.  The four losses of the step go
// to last[0..4) and, times B, into acc.
void loss(hipStream_t s, int B, const float* x, const float* u, const float* mu, const float* lv, const float* rec, float* du, float* last, double* acc);
// dmu, dlv of beta * kld and of the reparametrisation, from dz
void kl_reparam_bwd(hipStream_t s, int B, const float* mu, const float* lv, const float* eps, const float* dz, const float* rec, float* dmu, float* dlv);

}  // namespace vt
}  // namespace said
