// audio_ft.hip — the kernels that fine-tuning the Wav2Vec2 transformer adds to the UNet trainer (audio_ft.h): LayerNorm over 512 / 768
// channels with a residual and the dropouts in front of and behind it, erf GELU with the activation dropout, the dropout of the attention
// probabilities, the SpecAugment substitution, weight_norm(dim = 2), each with its backward.  fp32, token-major (B T, C).
//
// Dropout masks are never stored: Philox4x32-10 (sched_math.h) with key = the step's seed, one call per four elements, the rule of
// include/said_audio_train.h: u = (word >> 8) 2^-24, kept iff u >= p, a kept element times the fp32 value of 1 / (1 - p).
//   element-wise sites: e = m C + c; counter (site, e >> 2, 0, 0), word e & 3
//   probabilities:      counter (site, (b 12 + head) T + i, j >> 2, 0), word j & 3
// Sums: a lane's own in index order, a wave's by train_dev.h's butterfly, columns by ut::colsum.  No atomics.
#include "audio_ft.h"

#include <math.h>

#include "sched_math.h"
#include "train_dev.h"
#include "unet_train.h"

namespace said {
namespace aft {
namespace {

__device__ __forceinline__ void drop4(const Drop& d, unsigned c1, unsigned c2, float (&f)[4]) {
    if (!(d.p > 0.f)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = 1.f;
        return;
    }
    unsigned r[4];
    philox4x32_10((unsigned)d.site, c1, c2, 0u, d.k0, d.k1, r);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = ((float)(r[e] >> 8) * 5.9604644775390625e-8f >= d.p) ? d.keep : 0.f;
}

// one wave per row of C = 256 Q channels; lane l owns the channel quadruples l, l + 64, ...
template <int Q>
__global__ void __launch_bounds__(NT) ln_fwd_kernel(int M, const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, const Drop pre, const Drop post, float* __restrict__ xhat,
                                                    float* __restrict__ rstd, float* __restrict__ y) {
    constexpr int C = 256 * Q;
    const int r = blockIdx.x * (NT / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (r >= M) return;
    const long long o = (long long)r * C;
    float v[Q][4], s = 0.f;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const int c4 = lane + 64 * i;
        float f[4];
        drop4(pre, (unsigned)r * (unsigned)(C / 4) + (unsigned)c4, 0u, f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t = x[o + 4 * c4 + e] * f[e];
            if (res) t = res[o + 4 * c4 + e] + t;
            v[i][e] = t;
            s += t;
        }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < Q; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) q += (v[i][e] - mean) * (v[i][e] - mean);
    const float rs = 1.f / sqrtf(wave_sum(q) / (float)C + 1e-5f);
    if (lane == 0) rstd[r] = rs;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const int c4 = lane + 64 * i;
        float f[4];
        drop4(post, (unsigned)r * (unsigned)(C / 4) + (unsigned)c4, 0u, f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * c4 + e;
            const float xh = (v[i][e] - mean) * rs;
            xhat[o + c] = xh;
            y[o + c] = (xh * gamma[c] + beta[c]) * f[e];
        }
    }
}

// (a lane reads its own elements of dy before it writes them anywhere: dres or dpre may be dy)
template <int Q>
__global__ void __launch_bounds__(NT) ln_bwd_kernel(int M, const float* dy, const float* __restrict__ xhat, const float* __restrict__ rstd,
                                                    const float* __restrict__ gamma, const Drop pre, const Drop post, float* du, float* dres,
                                                    int accumulate, float* dpre) {
    constexpr int C = 256 * Q;
    const int r = blockIdx.x * (NT / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (r >= M) return;
    const long long o = (long long)r * C;
    float g[Q][4], xh[Q][4], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const int c4 = lane + 64 * i;
        float f[4];
        drop4(post, (unsigned)r * (unsigned)(C / 4) + (unsigned)c4, 0u, f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * c4 + e;
            const float d = dy[o + c] * f[e];
            if (du) du[o + c] = d;
            g[i][e] = d * gamma[c];
            xh[i][e] = xhat[o + c];
            s1 += g[i][e];
            s2 += g[i][e] * xh[i][e];
        }
    }
    s1 = wave_sum(s1) / (float)C;
    s2 = wave_sum(s2) / (float)C;
    const float rs = rstd[r];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const int c4 = lane + 64 * i;
        float f[4];
        drop4(pre, (unsigned)r * (unsigned)(C / 4) + (unsigned)c4, 0u, f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * c4 + e;
            const float v = (g[i][e] - s1 - xh[i][e] * s2) * rs;
            if (dpre) dpre[o + c] = v * f[e];
            dres[o + c] = accumulate ? dres[o + c] + v : v;
        }
    }
}

__device__ __forceinline__ float gelu_f(float u) { return 0.5f * u * (1.f + erff(u * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_d(float u) {
    return 0.5f * (1.f + erff(u * 0.70710678118654752f)) + u * (0.3989422804014327f * expf(-0.5f * u * u));
}

__global__ void __launch_bounds__(NT) add_bias_kernel(long long n, int C, const float* __restrict__ bias, float* __restrict__ u) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i < n) u[i] += bias[i % C];
}
// one thread per four consecutive elements
__global__ void __launch_bounds__(NT) gelu_drop_fwd_kernel(long long n4, const float* __restrict__ u, const Drop d, float* __restrict__ y) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n4) return;
    float f[4];
    drop4(d, (unsigned)i, 0u, f);
#pragma unroll
    for (int e = 0; e < 4; ++e) y[4 * i + e] = gelu_f(u[4 * i + e]) * f[e];
}
__global__ void __launch_bounds__(NT) gelu_drop_bwd_kernel(long long n4, const float* __restrict__ u, const float* dy, const Drop d, float* du) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n4) return;
    float f[4];
    drop4(d, (unsigned)i, 0u, f);
#pragma unroll
    for (int e = 0; e < 4; ++e) du[4 * i + e] = dy[4 * i + e] * f[e] * gelu_d(u[4 * i + e]);
}

// one thread per (row, four consecutive keys)
__global__ void __launch_bounds__(NT) prob_drop_kernel(long long rows, int T, int nq, const float* P, const Drop d, float* Pd) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= rows * nq) return;
    const long long r = i / nq;
    const int jq = (int)(i % nq);
    float f[4];
    drop4(d, (unsigned)r, (unsigned)jq, f);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = 4 * jq + e;
        if (j < T) Pd[r * T + j] = P[r * T + j] * f[e];
    }
}

__global__ void __launch_bounds__(NT) mask_drop_fwd_kernel(long long n4, int C4, const float* __restrict__ x, const unsigned char* __restrict__ mask,
                                                           const float* __restrict__ embed, const Drop d, float* __restrict__ h) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n4) return;
    const long long m = i / C4;
    const int c4 = (int)(i % C4);
    const bool masked = mask && mask[m] != 0;
    float f[4];
    drop4(d, (unsigned)i, 0u, f);
#pragma unroll
    for (int e = 0; e < 4; ++e) h[4 * i + e] = masked ? embed[4 * c4 + e] : x[4 * i + e] * f[e];
}
__global__ void __launch_bounds__(NT) mask_drop_bwd_kernel(long long n4, int C4, const float* __restrict__ dh, const unsigned char* __restrict__ mask,
                                                           const Drop d, float* __restrict__ dx, float* __restrict__ dmasked) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n4) return;
    const bool masked = mask && mask[i / C4] != 0;
    float f[4];
    drop4(d, (unsigned)i, 0u, f);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float v = dh[4 * i + e];
        dx[4 * i + e] = masked ? 0.f : v * f[e];
        if (dmasked) dmasked[4 * i + e] = masked ? v : 0.f;
    }
}

__global__ void __launch_bounds__(NT) sqrt_kernel(int n, const float* __restrict__ x, float* __restrict__ y) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) y[i] = sqrtf(x[i]);
}
__global__ void __launch_bounds__(NT) wn_fwd_kernel(long long n, int K, const float* __restrict__ g, const float* __restrict__ v,
                                                    const float* __restrict__ norm, float* __restrict__ w) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int k = (int)(i % K);
    w[i] = v[i] * (g[k] / norm[k]);
}
// dot[k] = <dw, v> over (O, I): dg = dot / norm in place; dv = g / norm (dw - dg v / norm)
__global__ void __launch_bounds__(NT) wn_bwd_kernel(long long n, int K, const float* __restrict__ g, const float* __restrict__ v,
                                                    const float* __restrict__ norm, const float* __restrict__ dw, const float* __restrict__ dot,
                                                    float* __restrict__ dv) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int k = (int)(i % K);
    const float dg = dot[k] / norm[k];
    dv[i] = (g[k] / norm[k]) * (dw[i] - dg * (v[i] / norm[k]));
}
__global__ void __launch_bounds__(NT) div_kernel(int n, const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) y[i] = a[i] / b[i];
}

}  // namespace

void ln_fwd(hipStream_t s, int M, int C, const float* x, const float* res, const float* gamma, const float* beta, const Drop& pre, const Drop& post,
            float* xhat, float* rstd, float* y) {
    if (C == 768) ln_fwd_kernel<3><<<nblk(M, NT / 64), NT, 0, s>>>(M, x, res, gamma, beta, pre, post, xhat, rstd, y);
    else ln_fwd_kernel<2><<<nblk(M, NT / 64), NT, 0, s>>>(M, x, res, gamma, beta, pre, post, xhat, rstd, y);
}
void ln_bwd(hipStream_t s, int M, int C, const float* dy, const float* xhat, const float* rstd, const float* gamma, const Drop& pre, const Drop& post,
            float* du, float* dres, int accumulate, float* dpre) {
    if (C == 768) ln_bwd_kernel<3><<<nblk(M, NT / 64), NT, 0, s>>>(M, dy, xhat, rstd, gamma, pre, post, du, dres, accumulate, dpre);
    else ln_bwd_kernel<2><<<nblk(M, NT / 64), NT, 0, s>>>(M, dy, xhat, rstd, gamma, pre, post, du, dres, accumulate, dpre);
}
void add_bias(hipStream_t s, int M, int C, const float* bias, float* u) {
    add_bias_kernel<<<nblk((long long)M * C), NT, 0, s>>>((long long)M * C, C, bias, u);
}
void gelu_drop_fwd(hipStream_t s, long long n, const float* u, const Drop& d, float* y) {
    gelu_drop_fwd_kernel<<<nblk(n / 4), NT, 0, s>>>(n / 4, u, d, y);
}
void gelu_drop_bwd(hipStream_t s, long long n, const float* u, const float* dy, const Drop& d, float* du) {
    gelu_drop_bwd_kernel<<<nblk(n / 4), NT, 0, s>>>(n / 4, u, dy, d, du);
}
void prob_drop(hipStream_t s, long long rows, int T, const float* P, const Drop& d, float* Pd) {
    const int nq = (T + 3) / 4;
    prob_drop_kernel<<<nblk(rows * nq), NT, 0, s>>>(rows, T, nq, P, d, Pd);
}
void mask_drop_fwd(hipStream_t s, int M, int C, const float* x, const unsigned char* mask, const float* embed, const Drop& d, float* h) {
    const long long n4 = (long long)M * (C / 4);
    mask_drop_fwd_kernel<<<nblk(n4), NT, 0, s>>>(n4, C / 4, x, mask, embed, d, h);
}
void mask_drop_bwd(hipStream_t s, int M, int C, const float* dh, const unsigned char* mask, const Drop& d, float* dx, float* dmasked) {
    const long long n4 = (long long)M * (C / 4);
    mask_drop_bwd_kernel<<<nblk(n4), NT, 0, s>>>(n4, C / 4, dh, mask, d, dx, dmasked);
}
// the sums over (O, I) per tap run as two column sums: WN_SEG segments of rows, then the segments in order
void weight_norm_fwd(hipStream_t s, int OI, int K, const float* g, const float* v, float* part, float* norm, float* w) {
    ut::colsum(s, v, K, v, K, OI / WN_SEG, WN_SEG, K, part, 0);
    ut::colsum(s, part, K, nullptr, 0, WN_SEG, 1, K, norm, 0);
    sqrt_kernel<<<nblk(K), NT, 0, s>>>(K, norm, norm);
    wn_fwd_kernel<<<nblk((long long)OI * K), NT, 0, s>>>((long long)OI * K, K, g, v, norm, w);
}
void weight_norm_bwd(hipStream_t s, int OI, int K, const float* g, const float* v, const float* norm, const float* dw, float* part, float* dot,
                     float* dg, float* dv) {
    ut::colsum(s, dw, K, v, K, OI / WN_SEG, WN_SEG, K, part, 0);
    ut::colsum(s, part, K, nullptr, 0, WN_SEG, 1, K, dot, 0);
    wn_bwd_kernel<<<nblk((long long)OI * K), NT, 0, s>>>((long long)OI * K, K, g, v, norm, dw, dot, dv);
    div_kernel<<<nblk(K), NT, 0, s>>>(K, dot, norm, dg);
}

}  // namespace aft
}  // namespace said
