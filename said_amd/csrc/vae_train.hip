// vae_train.hip — the BCVAE training step (said/model/vae.py, script/train_vae.py): training-mode forward with batch statistics, the ELBO
// loss and its gradient, the backward of every layer.  fp32 throughout.  The update that follows (clip, AdamW, EMA) is train_opt.hip.
//
// Every reduction runs in a fixed order and no kernel uses atomics: a thread's own sum runs in index order, a wave's lanes are combined by a
// fixed xor butterfly, a workgroup's waves by a fixed LDS tree.  Equal inputs give bit-identical outputs, launched directly or from a graph.
// The step is a chain of small dependent launches (vae_trainer.cpp): one per layer and per BatchNorm seam, forward then backward.
#include "vae_train.h"

#include <math.h>

#include "train_dev.h"

namespace said {
namespace vt {
namespace {

__global__ void __launch_bounds__(NT) gather_kernel(int B, const float* __restrict__ data, const long long* __restrict__ off,
                                                    const int* __restrict__ len, const int* __restrict__ items, const int* __restrict__ mirror,
                                                    float* __restrict__ x) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= B * T * C) return;
    const int c = i % C, t = (i / C) % T, b = i / (T * C);
    const int* it = items + b * ITEM;
    const int sq = it[0], n = len[sq];
    // F.pad(seq, (0, 0, 60, 120), "replicate")[bdx + 60 + t]: the padded frame is the sequence's frame clamped into [0, n)
    const int f = min(max(it[1] + t, 0), n - 1);
    const int cs = it[2] ? mirror[c] : c;
    x[i] = it[3] ? 0.f : data[(off[sq] + f) * C + cs];
}

__global__ void __launch_bounds__(NT) conv_fwd_kernel(int transposed, int B, int Ci, int Co, int K, int S, int Lin, int Lout, TAct x,
                                                      const float* __restrict__ W, const float* __restrict__ bias, TActW y) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= B * Co * Lout) return;
    const int t = i % Lout, co = (i / Lout) % Co, b = i / (Lout * Co);
    const float* xb = x.p + (long long)b * x.sb;
    float acc = 0.f;
    if (!transposed) {
        for (int ci = 0; ci < Ci; ++ci)
            for (int j = 0; j < K; ++j) acc += W[(co * Ci + ci) * K + j] * xb[ci * x.sc + (t * S + j) * x.st];
    } else {   // y[t] = sum_j W[ci][co][j] x[t - j]
        for (int ci = 0; ci < Ci; ++ci)
            for (int j = 0; j < K; ++j) {
                const int p = t - j;
                if (p >= 0 && p < Lin) acc += W[(ci * Co + co) * K + j] * xb[ci * x.sc + p * x.st];
            }
    }
    y.p[(long long)b * y.sb + co * y.sc + t * y.st] = acc + bias[co];
}

__global__ void __launch_bounds__(NT) conv_bwd_data_kernel(int transposed, int B, int Ci, int Co, int K, int S, int Lin, int Lout, TAct dy,
                                                           const float* __restrict__ W, TActW dx) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= B * Ci * Lin) return;
    const int p = i % Lin, ci = (i / Lin) % Ci, b = i / (Lin * Ci);
    const float* g = dy.p + (long long)b * dy.sb;
    float acc = 0.f;
    for (int co = 0; co < Co; ++co)
        for (int j = 0; j < K; ++j) {
            if (!transposed) {   // x[p] fed y[t] through tap j when p = t S + j
                const int q = p - j;
                if (q < 0 || q % S) continue;
                const int t = q / S;
                if (t < Lout) acc += W[(co * Ci + ci) * K + j] * g[co * dy.sc + t * dy.st];
            } else {             // x[p] fed y[p + j]
                acc += W[(ci * Co + co) * K + j] * g[co * dy.sc + (p + j) * dy.st];
            }
        }
    dx.p[(long long)b * dx.sb + ci * dx.sc + p * dx.st] = acc;
}

// waves [0, Co Ci K): dW; waves [Co Ci K, + Co): dbias.  The B x Lout products of one weight are split over the lanes by their flat index.
__global__ void __launch_bounds__(NT) conv_bwd_weight_kernel(int transposed, int B, int Ci, int Co, int K, int S, int Lout, TAct x, TAct dy,
                                                             float* __restrict__ dW, float* __restrict__ dbias) {
    const int w = blockIdx.x * (NT / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    const int nw = Co * Ci * K;
    if (w >= nw + Co) return;
    const int N = B * Lout;
    float acc = 0.f;
    if (w < nw) {
        int co, ci, j;
        if (!transposed) { j = w % K; ci = (w / K) % Ci; co = w / (K * Ci); }
        else { j = w % K; co = (w / K) % Co; ci = w / (K * Co); }
        for (int n = lane; n < N; n += 64) {
            const int b = n / Lout, t = n % Lout;
            const float g = dy.p[(long long)b * dy.sb + co * dy.sc + t * dy.st];
            if (!transposed) acc += g * x.p[(long long)b * x.sb + ci * x.sc + (t * S + j) * x.st];
            else {
                const int p = t - j;   // y[t] += W[ci][co][j] x[t - j]
                if (p >= 0 && p < Lout - (K - 1)) acc += g * x.p[(long long)b * x.sb + ci * x.sc + p * x.st];
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) dW[w] = acc;
    } else {
        const int co = w - nw;
        for (int n = lane; n < N; n += 64) {
            const int b = n / Lout, t = n % Lout;
            acc += dy.p[(long long)b * dy.sb + co * dy.sc + t * dy.st];
        }
        acc = wave_sum(acc);
        if (lane == 0) dbias[co] = acc;
    }
}

// one wave per (b, o)
__global__ void __launch_bounds__(NT) linear_fwd_kernel(int B, int In, int Out, const float* __restrict__ x, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ y) {
    const int w = blockIdx.x * (NT / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (w >= B * Out) return;
    const int o = w % Out, b = w / Out;
    const float* wr = W + (long long)o * In;
    const float* xr = x + (long long)b * In;
    float acc = 0.f;
    for (int i = lane; i < In; i += 64) acc += wr[i] * xr[i];
    acc = wave_sum(acc);
    if (lane == 0) y[w] = acc + bias[o];
}

__global__ void __launch_bounds__(NT) linear_bwd_data_kernel(int B, int In, int Out, const float* __restrict__ dy, const float* __restrict__ W,
                                                             const float* __restrict__ dy2, const float* __restrict__ W2, float* __restrict__ dx) {
    const int k = blockIdx.x * NT + threadIdx.x;
    if (k >= B * In) return;
    const int i = k % In, b = k / In;
    float acc = 0.f;
    for (int o = 0; o < Out; ++o) acc += W[(long long)o * In + i] * dy[b * Out + o];
    if (W2) {
        float acc2 = 0.f;
        for (int o = 0; o < Out; ++o) acc2 += W2[(long long)o * In + i] * dy2[b * Out + o];
        acc += acc2;
    }
    dx[k] = acc;
}

__global__ void __launch_bounds__(NT) linear_bwd_weight_kernel(int B, int In, int Out, const float* __restrict__ x, const float* __restrict__ dy,
                                                               float* __restrict__ dW, float* __restrict__ dbias) {
    const long long k = (long long)blockIdx.x * NT + threadIdx.x;
    const long long nw = (long long)Out * In;
    if (k < nw) {
        const int i = (int)(k % In), o = (int)(k / In);
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += dy[b * Out + o] * x[(long long)b * In + i];
        dW[k] = acc;
    } else if (k < nw + Out) {
        const int o = (int)(k - nw);
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += dy[b * Out + o];
        dbias[o] = acc;
    }
}

// one workgroup per channel; element n of the channel is (b, t) = (n / L, n % L)
__global__ void __launch_bounds__(NT) bn_fwd_kernel(int train, int B, int Cn, int L, TAct a, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar,
                                                    float* __restrict__ stats, float slope, float* __restrict__ xhat, float* __restrict__ h) {
    __shared__ float sh[NT];
    const int c = blockIdx.x, N = B * L;
    auto at = [&](int n) { return (long long)(n / L) * a.sb + (long long)c * a.sc + (long long)(n % L) * a.st; };
    float mean, invstd;
    if (train) {
        float s = 0.f;
        for (int n = threadIdx.x; n < N; n += NT) s += a.p[at(n)];
        mean = block_sum(s, sh) / (float)N;
        float q = 0.f;
        for (int n = threadIdx.x; n < N; n += NT) {
            const float d = a.p[at(n)] - mean;
            q += d * d;
        }
        const float var = block_sum(q, sh) / (float)N;
        invstd = 1.f / sqrtf(var + 1e-5f);
        if (threadIdx.x == 0) {
            stats[c] = mean;
            stats[Cn + c] = invstd;
            rmean[c] = 0.1f * mean + 0.9f * rmean[c];
            rvar[c] = 0.1f * (var * ((float)N / (float)(N - 1))) + 0.9f * rvar[c];
        }
    } else {
        mean = rmean[c];
        invstd = 1.f / sqrtf(rvar[c] + 1e-5f);
    }
    const float g = gamma[c], bt = beta[c];
    for (int n = threadIdx.x; n < N; n += NT) {
        const long long e = at(n);
        const float xh = (a.p[e] - mean) * invstd;
        const float v = xh * g + bt;
        xhat[e] = xh;
        h[e] = v > 0.f ? v : v * slope;
    }
}

__global__ void __launch_bounds__(NT) bn_bwd_kernel(int B, int Cn, int L, TAct dh, TAct h, TAct xhat, const float* __restrict__ gamma,
                                                    const float* __restrict__ stats, float slope, float* __restrict__ dgamma,
                                                    float* __restrict__ dbeta, TActW da) {
    __shared__ float sh[NT];
    const int c = blockIdx.x, N = B * L;
    auto at = [&](const TAct& q, int n) { return (long long)(n / L) * q.sb + (long long)c * q.sc + (long long)(n % L) * q.st; };
    // LeakyReLU (in place in the reference): its backward reads the sign of the output
    auto grad = [&](int n) { const float g = dh.p[at(dh, n)]; return h.p[at(h, n)] > 0.f ? g : g * slope; };
    float s = 0.f, sx = 0.f;
    for (int n = threadIdx.x; n < N; n += NT) {
        const float g = grad(n);
        s += g;
        sx += g * xhat.p[at(xhat, n)];
    }
    s = block_sum(s, sh);
    sx = block_sum(sx, sh);
    if (threadIdx.x == 0) {
        dgamma[c] = sx;
        dbeta[c] = s;
    }
    const float k = gamma[c] * stats[Cn + c], ms = s / (float)N, msx = sx / (float)N;
    for (int n = threadIdx.x; n < N; n += NT) {
        const float g = grad(n);
        da.p[(long long)(n / L) * da.sb + (long long)c * da.sc + (long long)(n % L) * da.st] = (g - ms - xhat.p[at(xhat, n)] * msx) * k;
    }
}

__global__ void __launch_bounds__(NT) reparam_kernel(int n, const float* __restrict__ mu, const float* __restrict__ lv, const float* __restrict__ eps,
                                                     float* __restrict__ z) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) z[i] = mu[i] + expf(0.5f * lv[i]) * eps[i];
}

// one workgroup: reconstruction and velocity terms over the whole batch, the KL term, du
__global__ void __launch_bounds__(NT) loss_kernel(int B, const float* __restrict__ x, const float* __restrict__ u, const float* __restrict__ mu,
                                                  const float* __restrict__ lv, const float* __restrict__ rec, float* __restrict__ du,
                                                  float* __restrict__ last, double* __restrict__ acc) {
    __shared__ float sh[NT];
    const float* std_ = rec + NSCAL;
    const bool use_std = rec[S_USE_STD] != 0.f;
    const float beta = rec[S_BETA], wvel = rec[S_WVEL], fB = (float)B;
    // reweighted answer / prediction at (b, t, c): x / std, tanh(relu(u)) / std (out of place)
    auto ans = [&](int e) { return use_std ? x[e] / std_[e % C] : x[e]; };
    auto prd = [&](int e) { const float y = tanhf(fmaxf(u[e], 0.f)); return use_std ? y / std_[e % C] : y; };
    const int n = B * T * C;
    float sr = 0.f, sv = 0.f;
    for (int e = threadIdx.x; e < n; e += NT) {
        const int t = (e / C) % T;
        const float a = ans(e), p = prd(e);
        const float r = a - p;
        sr += r * r;
        float v = 0.f, vn = 0.f;   // velocity residuals (pred diff - answer diff) ending at t and at t + 1
        if (t > 0) {
            v = (p - prd(e - C)) - (a - ans(e - C));
            sv += v * v;
        }
        if (du) {
            if (t + 1 < T) vn = (prd(e + C) - p) - (ans(e + C) - a);
            const float gp = (-r) / fB + wvel * ((v - vn) / fB);       // d total / d prediction
            const float y = tanhf(fmaxf(u[e], 0.f));
            const float gy = use_std ? gp / std_[e % C] : gp;
            du[e] = u[e] > 0.f ? gy * (1.f - y * y) : 0.f;
        }
    }
    float sk = 0.f;
    for (int e = threadIdx.x; e < B * Z; e += NT) sk += mu[e] * mu[e] + expf(lv[e]) - lv[e] - 1.f;
    sr = block_sum(sr, sh);
    sv = block_sum(sv, sh);
    sk = block_sum(sk, sh);
    if (threadIdx.x == 0) {
        const float reconst = 0.5f * sr / fB, kld = 0.5f * (sk / fB), vel = 0.5f * sv / fB;
        const float total = reconst + beta * kld + wvel * vel;
        last[0] = reconst;
        last[1] = kld;
        last[2] = vel;
        last[3] = total;
        acc[A_RECONST] += (double)reconst * B;
        acc[A_REG] += (double)kld * B;
        acc[A_VEL] += (double)vel * B;
        acc[A_TOTAL] += (double)total * B;
        acc[A_COUNT] += (double)B;
        if (!isfinite(total)) acc[A_BAD] += 1.0;
    }
}

__global__ void __launch_bounds__(NT) kl_reparam_bwd_kernel(int n, int B, const float* __restrict__ mu, const float* __restrict__ lv,
                                                            const float* __restrict__ eps, const float* __restrict__ dz, const float* __restrict__ rec,
                                                            float* __restrict__ dmu, float* __restrict__ dlv) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const float kb = rec[S_BETA] * (0.5f / (float)B);   // d (beta kld) = beta 0.5 / B d sum
    const float e = expf(lv[i]);
    dmu[i] = kb * (2.f * mu[i]) + dz[i];
    dlv[i] = kb * (e - 1.f) + dz[i] * eps[i] * (0.5f * expf(0.5f * lv[i]));
}

}  // namespace

void gather(hipStream_t s, int B, const float* data, const long long* off, const int* len, const int* items, const int* mirror, float* x) {
    gather_kernel<<<nblk((long long)B * T * C), NT, 0, s>>>(B, data, off, len, items, mirror, x);
}
void conv_fwd(hipStream_t s, int transposed, int B, int Ci, int Co, int K, int S, int Lin, int Lout, TAct x, const float* W, const float* bias, TActW y) {
    conv_fwd_kernel<<<nblk((long long)B * Co * Lout), NT, 0, s>>>(transposed, B, Ci, Co, K, S, Lin, Lout, x, W, bias, y);
}
void conv_bwd_data(hipStream_t s, int transposed, int B, int Ci, int Co, int K, int S, int Lin, int Lout, TAct dy, const float* W, TActW dx) {
    conv_bwd_data_kernel<<<nblk((long long)B * Ci * Lin), NT, 0, s>>>(transposed, B, Ci, Co, K, S, Lin, Lout, dy, W, dx);
}
void conv_bwd_weight(hipStream_t s, int transposed, int B, int Ci, int Co, int K, int S, int Lin, int Lout, TAct x, TAct dy, float* dW, float* dbias) {
    (void)Lin;
    conv_bwd_weight_kernel<<<nblk((long long)(Co * Ci * K + Co), NT / 64), NT, 0, s>>>(transposed, B, Ci, Co, K, S, Lout, x, dy, dW, dbias);
}
void linear_fwd(hipStream_t s, int B, int In, int Out, const float* x, const float* W, const float* bias, float* y) {
    linear_fwd_kernel<<<nblk((long long)B * Out, NT / 64), NT, 0, s>>>(B, In, Out, x, W, bias, y);
}
void linear_bwd_data(hipStream_t s, int B, int In, int Out, const float* dy, const float* W, const float* dy2, const float* W2, float* dx) {
    linear_bwd_data_kernel<<<nblk((long long)B * In), NT, 0, s>>>(B, In, Out, dy, W, dy2, W2, dx);
}
void linear_bwd_weight(hipStream_t s, int B, int In, int Out, const float* x, const float* dy, float* dW, float* dbias) {
    linear_bwd_weight_kernel<<<nblk((long long)Out * In + Out), NT, 0, s>>>(B, In, Out, x, dy, dW, dbias);
}
void bn_fwd(hipStream_t s, int train, int B, int Cn, int L, TAct a, const float* gamma, const float* beta, float* rmean, float* rvar, float* stats,
            float slope, float* xhat, float* h) {
    bn_fwd_kernel<<<Cn, NT, 0, s>>>(train, B, Cn, L, a, gamma, beta, rmean, rvar, stats, slope, xhat, h);
}
void bn_bwd(hipStream_t s, int B, int Cn, int L, TAct dh, TAct h, TAct xhat, const float* gamma, const float* stats, float slope, float* dgamma,
            float* dbeta, TActW da) {
    bn_bwd_kernel<<<Cn, NT, 0, s>>>(B, Cn, L, dh, h, xhat, gamma, stats, slope, dgamma, dbeta, da);
}
void reparam(hipStream_t s, int B, const float* mu, const float* lv, const float* eps, float* z) {
    reparam_kernel<<<nblk((long long)B * Z), NT, 0, s>>>(B * Z, mu, lv, eps, z);
}
void loss(hipStream_t s, int B, const float* x, const float* u, const float* mu, const float* lv, const float* rec, float* du, float* last, double* acc) {
    loss_kernel<<<1, NT, 0, s>>>(B, x, u, mu, lv, rec, du, last, acc);
}
void kl_reparam_bwd(hipStream_t s, int B, const float* mu, const float* lv, const float* eps, const float* dz, const float* rec, float* dmu, float* dlv) {
    kl_reparam_bwd_kernel<<<nblk((long long)B * Z), NT, 0, s>>>(B * Z, B, mu, lv, eps, dz, rec, dmu, dlv);
}

}  // namespace vt
}  // namespace said
