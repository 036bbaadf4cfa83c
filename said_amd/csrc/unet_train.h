// unet_train.h — launchers of the UNet denoiser's training kernels (unet_train.hip), called by the trainer context (unet_trainer.cpp).
// Every launcher only enqueues on `s`.  Activations are fp32 and token-major: element (b, t, c) of a (B, T, C) tensor lives at
// ((b T) + t) ld + c.  No kernel uses atomics; every sum runs in a fixed order (unet_train.hip's header), so equal inputs give equal bits.
#pragma once
#include <hip/hip_runtime.h>

namespace said {
namespace ut __attribute__((visibility("hidden"))) {

// per-step scalars (include/said_unet_train.h SAID_UT_S_*)
enum { S_LR = 0, S_WD_FACTOR, S_STEP_SIZE, S_BC2_SQRT, S_EMA_OMD, S_WVEL, S_WVERTEX, S_OMB1, S_B2, S_OMB2, S_EPS, S_USE_EMA, S_PRED_TYPE, S_DROPOUT,
       S_USE_STD, NSCAL = 16 };   // the record holds the scalars and then std[32]
// accumulated losses (double): predict * B, velocity * B, vertex * B, total * B, samples, non-finite steps
enum { A_PREDICT = 0, A_VEL, A_VERTEX, A_TOTAL, A_COUNT, A_BAD, NACC = 8 };
constexpr int XC = 32;   // blendshape coefficients per frame

// One operand of the GEMM, read as f(r, k): r the row (of A: m, of B: n), k the reduction index.  One of the two indices is the operand's
// "line" index rho, the other its "column" index q (swap != 0: rho = k, q = r).  q decodes to (tap j, channel c): J == 1: (0, q);
// cmajor: (q % J, q / J); else (q / Cn, q % Cn).
//   T == 1 (a plain matrix): element at rho sr + c sc + j sj.
//   T > 1 (the rows of a (B, T, ld) activation, shifted by the tap): rho = b T + t, t' = t + sh0 + dj j; 0 outside [0, T), else the
//   element at (b T + t') ld + c.  This is how the k = 3 convolutions run as GEMMs (forward, data gradient and weight gradient).
struct UOp {
    const float* p;
    long long zb, zh;   // offsets of batch entry z: (z / ZH) zb + (z % ZH) zh
    int swap, T, ld, sr, sc, sj, Cn, J, cmajor, sh0, dj;
};
// C[z][m][n] = alpha sum_k A(m, k) B(n, k) (+ bias[n]) (+ rowb[(m / rbT) N + n]) (+ res[m ldr + n]) (+ C[z][m][n] when accumulate)
struct UGemm {
    UOp A, B;
    float* C;
    long long czb, czh;
    int ldc, M, N, K, Z, ZH;
    float alpha;
    const float* bias;
    const float* rowb;
    int rbT;
    const float* res;
    int ldr, accumulate;
    // K split: KS > 1 runs KS workgroups per tile on k chunks of kchunk (a multiple of 16); their partial tiles go to part[ks][z][m][n] and
    // gemm_reduce adds them in the order ks = 0, 1, ... before the epilogue
    int KS, kchunk;
    float* part;
};
void gemm(hipStream_t s, const UGemm& g);
// the second launch of a K-split gemm alone: C = epilogue(sum over ks of part[ks]) in ascending chunk order; for a kernel that wrote the
// partial tiles itself (enc_gemm.hip)
void gemm_reduce(hipStream_t s, const UGemm& g);

// out[seg][n] (+)= sum over the rows r of segment seg (rows seg * rows .. seg * rows + rows - 1) of x[r ld + n] (* mul[r ldm + n])
void colsum(hipStream_t s, const float* x, int ld, const float* mul, int ldm, int rows, int nseg, int N, float* out, int accumulate);
// GroupNorm(32 groups) over (T, C / 32) per sample, then optionally SiLU, then optionally dropout(p) with the Philox mask of (seed, layer).
// Saves xhat (B T C) and rstd (B 32).  x has row stride ldx; y and xhat are dense (B T, C).
void gn_fwd(hipStream_t s, int B, int T, int C, const float* x, int ldx, const float* gamma, const float* beta, float eps, int silu, float p,
            unsigned long long seed, int layer, float* xhat, float* rstd, float* y);
// backward: du = gradient at the normalisation's output (B T, C, dense, written), dx (+)= gradient at x
void gn_bwd(hipStream_t s, int B, int T, int C, const float* dy, const float* xhat, const float* rstd, const float* gamma, const float* beta, int silu,
            float p, unsigned long long seed, int layer, float* du, float* dx, int lddx, int accumulate);
// LayerNorm over C = 192 per row; saves xhat and rstd
void ln_fwd(hipStream_t s, int M, const float* x, const float* gamma, const float* beta, float* xhat, float* rstd, float* y);
// dx (+)= backward of the above; dgamma = colsum(dy xhat), dbeta = colsum(dy) are the caller's
void ln_bwd(hipStream_t s, int M, const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dx, int accumulate);
// rows of S (rows x Tk, row r is query r % Tq): P = softmax(scale S) over the keys [lo[i], hi[i]) (all keys when lo is null), 0 elsewhere; in place
void softmax_fwd(hipStream_t s, long long rows, int Tq, int Tk, float scale, const int* lo, const int* hi, float* S);
// dS = scale P (dP - sum_j dP P), in place on dP
void softmax_bwd(hipStream_t s, long long rows, int Tk, float scale, const float* P, float* dP);
// GEGLU: y[m][i] = u[m][i] gelu(u[m][F + i]) (erf GELU), u (M, 2F)
void geglu_fwd(hipStream_t s, int M, int F, const float* u, float* y);
void geglu_bwd(hipStream_t s, int M, int F, const float* u, const float* dy, float* du);
void silu_fwd(hipStream_t s, long long n, const float* x, float* y);
// dx (+)= dy silu'(x)
void silu_bwd(hipStream_t s, long long n, const float* x, const float* dy, float* dx);
// dst[m ldd + n] (+)= src[m lds + n]
void copy2d(hipStream_t s, int M, int N, const float* src, int lds, float* dst, int ldd, int accumulate);
// ctx[b][t][:] = cond[b] ? audio[b][t][:] : null[:]   (Cc channels)
void select_ctx(hipStream_t s, int B, int T, int Cc, const float* audio, const float* null_emb, const int* cond, float* ctx);
// zero the rows of the samples whose cond is set
void mask_cond_rows(hipStream_t s, int B, int T, int Cc, const int* cond, float* d);
// dc = d with the rows of the samples whose cond is not set zeroed; those rows stay in d, whose other rows become zero
void split_cond_rows(hipStream_t s, int B, int T, int Cc, const int* cond, float* d, float* dc);
// e[b][:] = [cos(t_b f_i), sin(t_b f_i)], f_i = exp(-ln(10000) i / (dim / 2)), fp32 as the reference computes it
void timestep_embedding(hipStream_t s, int B, int dim, const float* tsteps, float* e);
// noisy = sa x0 + sb noise; answer = noise | x0 | sa noise - sb x0 by prediction type (rec[S_PRED_TYPE]); sasb (B, 2)
void add_noise(hipStream_t s, int B, int T, const float* x0, const float* noise, const float* sasb, const float* rec, float* noisy, float* answer);
// the objective (see unet_train.hip): r = (pred - answer) / std -> R
void loss_residual(hipStream_t s, int n, const float* pred, const float* ans, const float* rec, float* R);
// vertex term: E (n elements) -> block partial sums of |E| (nblk doubles), E <- sign(E)
void vertex_abs(hipStream_t s, long long n, float* E, double* part, int nblk);
// losses and d total / d pred; GV (nullable) = sign(E) D^T; part / nblk / nvert the vertex partial sums and element count
void loss_final(hipStream_t s, int B, int T, const float* R, const float* GV, const double* part, int nblk, long long nvert, const float* rec,
                float* dpred, float* last, double* acc);

}  // namespace ut
}  // namespace said
