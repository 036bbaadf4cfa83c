// unet_train.hip — the kernels of the UNet denoiser's training step (said/model/unet_1d_condition.py, script/train.py): a training-mode forward
// that keeps what the backward needs, the backward of every layer, the objective of random_noise_loss and its gradient.  fp32 throughout;
// activations are token-major (B T, C).  The update that follows (clip, AdamW, EMA) is train_opt.hip.
//
// Matrix products (linear layers, the k = 3 / k = 1 convolutions as shifted-operand GEMMs, the attention products) all run on ONE kernel,
// gemm_kernel, on v_mfma_f32_32x32x2_f32.  Reduction orders: a GEMM element is summed over k in ascending 16-wide tiles, each tile in ascending
// k pairs inside the matrix instruction; a K-split GEMM adds its chunk sums in ascending chunk order (gemm_reduce_kernel); a thread's own sum runs
// in index order, a wave's lanes are combined by a fixed xor butterfly, a workgroup's threads by a fixed LDS tree.  No atomics anywhere.
#include "unet_train.h"

#include <math.h>

#include "sched_math.h"
#include "train_dev.h"
#include "vec_types.h"

namespace said {
namespace ut {
namespace {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- GEMM
struct Part { long long off; int t; };
__device__ __forceinline__ Part part_rho(const UOp& o, int rho) {
    if (o.T > 1) {
        const int t = rho % o.T;
        return Part{(long long)(rho - t) * o.ld, t};
    }
    return Part{(long long)rho * o.sr, 0};
}
__device__ __forceinline__ Part part_q(const UOp& o, int q) {
    int c = q, j = 0;
    if (o.J > 1) {
        if (o.cmajor) { c = q / o.J; j = q - c * o.J; }
        else { j = q / o.Cn; c = q - j * o.Cn; }
    }
    return Part{(long long)c * o.sc + (long long)j * o.sj, o.T > 1 ? o.sh0 + o.dj * j : 0};
}
__device__ __forceinline__ Part part_r(const UOp& o, int r) { return o.swap ? part_q(o, r) : part_rho(o, r); }
__device__ __forceinline__ Part part_k(const UOp& o, int k) { return o.swap ? part_rho(o, k) : part_q(o, k); }
__device__ __forceinline__ float fetch(const UOp& o, const float* p, const Part& a, const Part& b) {
    const int t = a.t + b.t;
    if ((unsigned)t >= (unsigned)o.T) return 0.f;
    return p[a.off + b.off + (o.T > 1 ? (long long)t * o.ld : 0)];
}

constexpr int BM = 64, BN = 64, BK = 16, LP = BM + 4;

__device__ __forceinline__ void epilogue(const UGemm& g, float* C, int m, int n, float v) {
    v *= g.alpha;
    if (g.bias) v += g.bias[n];
    if (g.rowb) v += g.rowb[(long long)(m / g.rbT) * g.N + n];
    if (g.res) v += g.res[(long long)m * g.ldr + n];
    float* c = C + (long long)m * g.ldc + n;
    if (g.accumulate) v += *c;
    *c = v;
}

__global__ void __launch_bounds__(NT) gemm_kernel(const UGemm g) {
    __shared__ float As[BK][LP], Bs[BK][LP];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wm = wave & 1, wn = wave >> 1;
    const int z = blockIdx.z / g.KS, ks = blockIdx.z % g.KS;
    const int zb = z / g.ZH, zh = z % g.ZH;
    const float* Ap = g.A.p + zb * g.A.zb + zh * g.A.zh;
    const float* Bp = g.B.p + zb * g.B.zb + zh * g.B.zh;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    // staging: element e = tid + 256 i of a 64 x 16 tile; row = e / 16, k = e % 16 when k is the operand's contiguous index, else row = e % 64
    const bool akf = g.A.swap ? false : (g.A.sc == 1), bkf = g.B.swap ? false : (g.B.sc == 1);
    Part ra[4], rb[4];
    int am[4], ak[4], bn[4], bk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = tid + NT * i;
        am[i] = akf ? (e >> 4) : (e & 63);
        ak[i] = akf ? (e & 15) : (e >> 6);
        bn[i] = bkf ? (e >> 4) : (e & 63);
        bk[i] = bkf ? (e & 15) : (e >> 6);
        ra[i] = part_r(g.A, min(m0 + am[i], g.M - 1));
        rb[i] = part_r(g.B, min(n0 + bn[i], g.N - 1));
    }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int kbeg = ks * g.kchunk, kend = min(g.K, kbeg + g.kchunk);
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        float va[4], vb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + ak[i];
            va[i] = (m0 + am[i] < g.M && k < kend) ? fetch(g.A, Ap, ra[i], part_k(g.A, k)) : 0.f;
            const int k2 = k0 + bk[i];
            vb[i] = (n0 + bn[i] < g.N && k2 < kend) ? fetch(g.B, Bp, rb[i], part_k(g.B, k2)) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            As[ak[i]][am[i]] = va[i];
            Bs[bk[i]][bn[i]] = vb[i];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const float a = As[kk * 2 + (lane >> 5)][wm * 32 + (lane & 31)];
            const float b = Bs[kk * 2 + (lane >> 5)][wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    // lane l, register v: row 8 (v / 4) + 4 (l / 32) + v % 4, column l % 32
    const int n = n0 + wn * 32 + (lane & 31);
    if (n >= g.N) return;
    float* C = g.C + zb * g.czb + zh * g.czh;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int m = m0 + wm * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
        if (m >= g.M) continue;
        if (g.KS > 1) g.part[(((long long)ks * g.Z + z) * g.M + m) * g.N + n] = acc[v];
        else epilogue(g, C, m, n, acc[v]);
    }
}

__global__ void __launch_bounds__(NT) gemm_reduce_kernel(const UGemm g) {
    const long long per = (long long)g.M * g.N, total = per * g.Z;
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int z = (int)(i / per), m = (int)((i % per) / g.N), n = (int)(i % g.N);
    float v = 0.f;
    for (int ks = 0; ks < g.KS; ++ks) v += g.part[(long long)ks * total + i];
    epilogue(g, g.C + (z / g.ZH) * g.czb + (z % g.ZH) * g.czh, m, n, v);
}

// ---------------------------------------------------------------------------------------------------------------- column sums
// workgroup: 16 columns x 16 row lanes; row lane q sums rows q, q + 16, ... in order, the 16 lane sums are added in order 0 .. 15
__global__ void __launch_bounds__(NT) colsum_kernel(const float* __restrict__ x, int ld, const float* __restrict__ mul, int ldm, int rows, int N,
                                                    float* __restrict__ out, int accumulate) {
    __shared__ float sh[16][17];
    const int c = threadIdx.x & 15, q = threadIdx.x >> 4, n = blockIdx.x * 16 + c, seg = blockIdx.y;
    float s = 0.f;
    if (n < N)
        for (int r = q; r < rows; r += 16) {
            const long long row = (long long)seg * rows + r;
            const float v = x[row * ld + n];
            s += mul ? v * mul[row * ldm + n] : v;
        }
    sh[q][c] = s;
    __syncthreads();
    if (q == 0 && n < N) {
        float t = 0.f;
        for (int i = 0; i < 16; ++i) t += sh[i][c];
        float* o = out + (long long)seg * N + n;
        *o = accumulate ? *o + t : t;
    }
}

// ---------------------------------------------------------------------------------------------------------------- norms
__device__ __forceinline__ float silu_f(float u) { return u / (1.f + expf(-u)); }
__device__ __forceinline__ float silu_d(float u) {
    const float sg = 1.f / (1.f + expf(-u));
    return sg * (1.f + u * (1.f - sg));
}
// dropout keep factor of element `elem` of layer `layer`: Philox4x32-10, key = seed, counter = (layer, elem, 0, 0); u = (r0 >> 8) 2^-24; keep iff u >= p
__device__ __forceinline__ float drop_factor(unsigned long long seed, int layer, unsigned elem, float p) {
    unsigned r[4];
    philox4x32_10((unsigned)layer, elem, 0u, 0u, (unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32), r);
    const float u = (float)(r[0] >> 8) * 5.9604644775390625e-8f;
    return u >= p ? 1.f / (1.f - p) : 0.f;
}

// one workgroup per (sample, group)
__global__ void __launch_bounds__(NT) gn_fwd_kernel(int T, int C, const float* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float eps, int silu, float p, unsigned long long seed, int layer,
                                                    float* __restrict__ xhat, float* __restrict__ rstd, float* __restrict__ y) {
    __shared__ float sh[NT];
    const int b = blockIdx.x / 32, gi = blockIdx.x % 32, cpg = C / 32, n = T * cpg;
    const float* xb = x + (long long)b * T * ldx + gi * cpg;
    float s = 0.f;
    for (int e = threadIdx.x; e < n; e += NT) s += xb[(long long)(e / cpg) * ldx + e % cpg];
    const float mean = block_sum(s, sh) / (float)n;
    float q = 0.f;
    for (int e = threadIdx.x; e < n; e += NT) {
        const float d = xb[(long long)(e / cpg) * ldx + e % cpg] - mean;
        q += d * d;
    }
    const float rs = 1.f / sqrtf(block_sum(q, sh) / (float)n + eps);
    if (threadIdx.x == 0) rstd[blockIdx.x] = rs;
    for (int e = threadIdx.x; e < n; e += NT) {
        const int t = e / cpg, c = gi * cpg + e % cpg;
        const float xh = (xb[(long long)t * ldx + e % cpg] - mean) * rs;
        const long long o = ((long long)b * T + t) * C + c;
        float v = xh * gamma[c] + beta[c];
        if (silu) v = silu_f(v);
        if (p > 0.f) v *= drop_factor(seed, layer, (unsigned)o, p);
        xhat[o] = xh;
        y[o] = v;
    }
}

__global__ void __launch_bounds__(NT) gn_bwd_kernel(int T, int C, const float* __restrict__ dy, const float* __restrict__ xhat,
                                                    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    int silu, float p, unsigned long long seed, int layer, float* __restrict__ du,
                                                    float* __restrict__ dx, int lddx, int accumulate) {
    __shared__ float sh[NT];
    const int b = blockIdx.x / 32, gi = blockIdx.x % 32, cpg = C / 32, n = T * cpg;
    float s1 = 0.f, s2 = 0.f;
    for (int e = threadIdx.x; e < n; e += NT) {
        const int t = e / cpg, c = gi * cpg + e % cpg;
        const long long o = ((long long)b * T + t) * C + c;
        float g = dy[o];
        if (p > 0.f) g *= drop_factor(seed, layer, (unsigned)o, p);
        const float xh = xhat[o];
        if (silu) g *= silu_d(xh * gamma[c] + beta[c]);
        du[o] = g;
        const float gg = g * gamma[c];
        s1 += gg;
        s2 += gg * xh;
    }
    s1 = block_sum(s1, sh) / (float)n;
    s2 = block_sum(s2, sh) / (float)n;
    const float rs = rstd[blockIdx.x];
    for (int e = threadIdx.x; e < n; e += NT) {
        const int t = e / cpg, c = gi * cpg + e % cpg;
        const long long o = ((long long)b * T + t) * C + c;
        const float v = (du[o] * gamma[c] - s1 - xhat[o] * s2) * rs;
        float* d = dx + ((long long)b * T + t) * lddx + c;
        *d = accumulate ? *d + v : v;
    }
}

// one wave per row of 192
__global__ void __launch_bounds__(NT) ln_fwd_kernel(int M, const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float* __restrict__ xhat, float* __restrict__ rstd, float* __restrict__ y) {
    const int r = blockIdx.x * (NT / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (r >= M) return;
    const float* xr = x + (long long)r * 192;
    float v[3];
    for (int i = 0; i < 3; ++i) v[i] = xr[lane + 64 * i];
    const float mean = wave_sum((v[0] + v[1]) + v[2]) / 192.f;
    float q = 0.f;
    for (int i = 0; i < 3; ++i) q += (v[i] - mean) * (v[i] - mean);
    const float rs = 1.f / sqrtf(wave_sum(q) / 192.f + 1e-5f);
    if (lane == 0) rstd[r] = rs;
    for (int i = 0; i < 3; ++i) {
        const int c = lane + 64 * i;
        const float xh = (v[i] - mean) * rs;
        xhat[(long long)r * 192 + c] = xh;
        y[(long long)r * 192 + c] = xh * gamma[c] + beta[c];
    }
}
__global__ void __launch_bounds__(NT) ln_bwd_kernel(int M, const float* __restrict__ dy, const float* __restrict__ xhat, const float* __restrict__ rstd,
                                                    const float* __restrict__ gamma, float* __restrict__ dx, int accumulate) {
    const int r = blockIdx.x * (NT / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (r >= M) return;
    float g[3], xh[3], s1 = 0.f, s2 = 0.f;
    for (int i = 0; i < 3; ++i) {
        const int c = lane + 64 * i;
        g[i] = dy[(long long)r * 192 + c] * gamma[c];
        xh[i] = xhat[(long long)r * 192 + c];
        s1 += g[i];
        s2 += g[i] * xh[i];
    }
    s1 = wave_sum(s1) / 192.f;
    s2 = wave_sum(s2) / 192.f;
    const float rs = rstd[r];
    for (int i = 0; i < 3; ++i) {
        float* d = dx + (long long)r * 192 + lane + 64 * i;
        const float v = (g[i] - s1 - xh[i] * s2) * rs;
        *d = accumulate ? *d + v : v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- softmax
// one wave per row
__global__ void __launch_bounds__(NT) softmax_fwd_kernel(long long rows, int Tq, int Tk, float scale, const int* __restrict__ lo,
                                                         const int* __restrict__ hi, float* __restrict__ S) {
    const long long r = (long long)blockIdx.x * (NT / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;
    float* row = S + r * Tk;
    const int i = (int)(r % Tq), j0 = lo ? lo[i] : 0, j1 = lo ? hi[i] : Tk;
    float m = -3.4028234663852886e38f;
    for (int j = j0 + lane; j < j1; j += 64) m = fmaxf(m, row[j] * scale);
    m = wave_max(m);
    float s = 0.f;
    for (int j = j0 + lane; j < j1; j += 64) s += expf(row[j] * scale - m);
    s = wave_sum(s);
    for (int j = lane; j < Tk; j += 64) row[j] = (j >= j0 && j < j1) ? expf(row[j] * scale - m) / s : 0.f;
}
__global__ void __launch_bounds__(NT) softmax_bwd_kernel(long long rows, int Tk, float scale, const float* __restrict__ P, float* __restrict__ dP) {
    const long long r = (long long)blockIdx.x * (NT / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;
    const float* p = P + r * Tk;
    float* d = dP + r * Tk;
    float s = 0.f;
    for (int j = lane; j < Tk; j += 64) s += d[j] * p[j];
    s = wave_sum(s);
    for (int j = lane; j < Tk; j += 64) d[j] = scale * (p[j] * (d[j] - s));
}

// ---------------------------------------------------------------------------------------------------------------- element-wise
__global__ void __launch_bounds__(NT) geglu_fwd_kernel(long long n, int F, const float* __restrict__ u, float* __restrict__ y) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const long long m = i / F;
    const int c = (int)(i % F);
    const float a = u[m * 2 * F + c], g = u[m * 2 * F + F + c];
    y[i] = a * (0.5f * g * (1.f + erff(g * 0.70710678118654752f)));
}
__global__ void __launch_bounds__(NT) geglu_bwd_kernel(long long n, int F, const float* __restrict__ u, const float* __restrict__ dy, float* __restrict__ du) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const long long m = i / F;
    const int c = (int)(i % F);
    const float a = u[m * 2 * F + c], g = u[m * 2 * F + F + c], d = dy[i];
    const float cdf = 0.5f * (1.f + erff(g * 0.70710678118654752f));
    du[m * 2 * F + c] = d * (g * cdf);
    du[m * 2 * F + F + c] = d * a * (cdf + g * (0.3989422804014327f * expf(-0.5f * g * g)));
}
__global__ void __launch_bounds__(NT) silu_fwd_kernel(long long n, const float* __restrict__ x, float* __restrict__ y) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i < n) y[i] = silu_f(x[i]);
}
__global__ void __launch_bounds__(NT) silu_bwd_kernel(long long n, const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i < n) dx[i] = dy[i] * silu_d(x[i]);
}
__global__ void __launch_bounds__(NT) copy2d_kernel(long long n, int N, const float* __restrict__ src, int lds, float* __restrict__ dst, int ldd, int accumulate) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const long long m = i / N;
    const int c = (int)(i % N);
    const float v = src[m * lds + c];
    float* d = dst + m * ldd + c;
    *d = accumulate ? *d + v : v;
}
__global__ void __launch_bounds__(NT) select_ctx_kernel(long long n, int T, int Cc, const float* __restrict__ audio, const float* __restrict__ null_emb,
                                                        const int* __restrict__ cond, float* __restrict__ ctx) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int b = (int)(i / ((long long)T * Cc));
    ctx[i] = cond[b] ? audio[i] : null_emb[i % Cc];
}
__global__ void __launch_bounds__(NT) mask_cond_rows_kernel(long long n, int T, int Cc, const int* __restrict__ cond, float* __restrict__ d) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    if (cond[(int)(i / ((long long)T * Cc))]) d[i] = 0.f;
}
__global__ void __launch_bounds__(NT) split_cond_rows_kernel(long long n, int T, int Cc, const int* __restrict__ cond, float* __restrict__ d,
                                                             float* __restrict__ dc) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const bool c = cond[(int)(i / ((long long)T * Cc))] != 0;
    const float v = d[i];
    dc[i] = c ? v : 0.f;
    d[i] = c ? 0.f : v;
}
__global__ void __launch_bounds__(NT) timestep_embedding_kernel(int B, int dim, const float* __restrict__ ts, float* __restrict__ e) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= B * dim) return;
    const int b = i / dim, c = i % dim, half = dim / 2, f = c % half;
    const float freq = expf(-9.210340371976184f * (float)f / (float)half);
    const float a = ts[b] * freq;
    e[i] = c < half ? cosf(a) : sinf(a);
}
__global__ void __launch_bounds__(NT) add_noise_kernel(int n, int T, const float* __restrict__ x0, const float* __restrict__ noise,
                                                       const float* __restrict__ sasb, const float* __restrict__ rec, float* __restrict__ noisy,
                                                       float* __restrict__ answer) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int b = i / (T * XC), type = (int)rec[S_PRED_TYPE];
    const float sa = sasb[2 * b], sb = sasb[2 * b + 1];
    noisy[i] = sa * x0[i] + sb * noise[i];
    answer[i] = type == 0 ? noise[i] : type == 1 ? x0[i] : sa * noise[i] - sb * x0[i];
}

// ---------------------------------------------------------------------------------------------------------------- objective
// random_noise_loss (script/train.py:112-149).  With a coefficient std, answer /= std and pred /= std are in place in the reference, so the
// vertex term sees the reweighted tensors too and the gradient flows through the division: everything below is in terms of
// R = pred / std - answer / std.  predict = mean |R|; velocity = mean |R[t] - R[t - 1]|; vertex = mean |R D| (the difference of the two
// reference products, by linearity).  sign(0) = 0.
__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : v < 0.f ? -1.f : 0.f; }
__global__ void __launch_bounds__(NT) loss_residual_kernel(int n, const float* __restrict__ pred, const float* __restrict__ ans, const float* __restrict__ rec,
                                                           float* __restrict__ R) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const float* std_ = rec + NSCAL;
    R[i] = rec[S_USE_STD] != 0.f ? pred[i] / std_[i % XC] - ans[i] / std_[i % XC] : pred[i] - ans[i];
}
__global__ void __launch_bounds__(NT) vertex_abs_kernel(long long n, float* __restrict__ E, double* __restrict__ part) {
    __shared__ double sh[NT];
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
        const float v = E[i];
        s += (double)fabsf(v);
        E[i] = sgn(v);
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ void __launch_bounds__(NT) loss_final_kernel(int B, int T, const float* __restrict__ R, const float* __restrict__ GV,
                                                        const double* __restrict__ part, int nblk, long long nvert, const float* __restrict__ rec,
                                                        float* __restrict__ dpred, float* __restrict__ last, double* __restrict__ acc) {
    __shared__ double sh[NT];
    const float* std_ = rec + NSCAL;
    const bool use_std = rec[S_USE_STD] != 0.f;
    const float wvel = rec[S_WVEL], wvtx = rec[S_WVERTEX];
    const int n = B * T * XC;
    const float n1 = (float)n, n2 = (float)(B * (T - 1) * XC);
    double sp = 0.0, sv = 0.0;
    for (int e = threadIdx.x; e < n; e += NT) {
        const int t = (e / XC) % T;
        const float r = R[e];
        sp += (double)fabsf(r);
        float v = 0.f, vn = 0.f;
        if (t > 0) {
            v = r - R[e - XC];
            sv += (double)fabsf(v);
        }
        if (dpred) {
            if (t + 1 < T) vn = R[e + XC] - r;
            float g = sgn(r) / n1 + wvel * ((sgn(v) - sgn(vn)) / n2);
            if (GV) g += wvtx * (GV[e] / (float)nvert);
            dpred[e] = use_std ? g / std_[e % XC] : g;
        }
    }
    sp = block_sum(sp, sh);
    sv = block_sum(sv, sh);
    if (threadIdx.x == 0) {
        double vx = 0.0;
        for (int i = 0; i < nblk; ++i) vx += part[i];
        const float predict = (float)(sp / (double)n1), vel = (float)(sv / (double)n2), vertex = GV ? (float)(vx / (double)nvert) : 0.f;
        const float total = predict + wvel * vel + (GV ? wvtx * vertex : 0.f);
        last[0] = predict;
        last[1] = vel;
        last[2] = vertex;
        last[3] = total;
        acc[A_PREDICT] += (double)predict * B;
        acc[A_VEL] += (double)vel * B;
        acc[A_VERTEX] += (double)vertex * B;
        acc[A_TOTAL] += (double)total * B;
        acc[A_COUNT] += (double)B;
        if (!isfinite(total)) acc[A_BAD] += 1.0;
    }
}

}  // namespace

void gemm(hipStream_t s, const UGemm& g) {
    dim3 grid((g.M + BM - 1) / BM, (g.N + BN - 1) / BN, g.Z * g.KS);
    gemm_kernel<<<grid, NT, 0, s>>>(g);
    if (g.KS > 1) gemm_reduce(s, g);
}
void gemm_reduce(hipStream_t s, const UGemm& g) { gemm_reduce_kernel<<<nblk((long long)g.M * g.N * g.Z), NT, 0, s>>>(g); }
void colsum(hipStream_t s, const float* x, int ld, const float* mul, int ldm, int rows, int nseg, int N, float* out, int accumulate) {
    colsum_kernel<<<dim3((N + 15) / 16, nseg), NT, 0, s>>>(x, ld, mul, ldm, rows, N, out, accumulate);
}
void gn_fwd(hipStream_t s, int B, int T, int C, const float* x, int ldx, const float* gamma, const float* beta, float eps, int silu, float p,
            unsigned long long seed, int layer, float* xhat, float* rstd, float* y) {
    gn_fwd_kernel<<<B * 32, NT, 0, s>>>(T, C, x, ldx, gamma, beta, eps, silu, p, seed, layer, xhat, rstd, y);
}
void gn_bwd(hipStream_t s, int B, int T, int C, const float* dy, const float* xhat, const float* rstd, const float* gamma, const float* beta, int silu,
            float p, unsigned long long seed, int layer, float* du, float* dx, int lddx, int accumulate) {
    gn_bwd_kernel<<<B * 32, NT, 0, s>>>(T, C, dy, xhat, rstd, gamma, beta, silu, p, seed, layer, du, dx, lddx, accumulate);
}
void ln_fwd(hipStream_t s, int M, const float* x, const float* gamma, const float* beta, float* xhat, float* rstd, float* y) {
    ln_fwd_kernel<<<nblk(M, NT / 64), NT, 0, s>>>(M, x, gamma, beta, xhat, rstd, y);
}
void ln_bwd(hipStream_t s, int M, const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dx, int accumulate) {
    ln_bwd_kernel<<<nblk(M, NT / 64), NT, 0, s>>>(M, dy, xhat, rstd, gamma, dx, accumulate);
}
void softmax_fwd(hipStream_t s, long long rows, int Tq, int Tk, float scale, const int* lo, const int* hi, float* S) {
    softmax_fwd_kernel<<<nblk(rows, NT / 64), NT, 0, s>>>(rows, Tq, Tk, scale, lo, hi, S);
}
void softmax_bwd(hipStream_t s, long long rows, int Tk, float scale, const float* P, float* dP) {
    softmax_bwd_kernel<<<nblk(rows, NT / 64), NT, 0, s>>>(rows, Tk, scale, P, dP);
}
void geglu_fwd(hipStream_t s, int M, int F, const float* u, float* y) { geglu_fwd_kernel<<<nblk((long long)M * F), NT, 0, s>>>((long long)M * F, F, u, y); }
void geglu_bwd(hipStream_t s, int M, int F, const float* u, const float* dy, float* du) {
    geglu_bwd_kernel<<<nblk((long long)M * F), NT, 0, s>>>((long long)M * F, F, u, dy, du);
}
void silu_fwd(hipStream_t s, long long n, const float* x, float* y) { silu_fwd_kernel<<<nblk(n), NT, 0, s>>>(n, x, y); }
void silu_bwd(hipStream_t s, long long n, const float* x, const float* dy, float* dx) { silu_bwd_kernel<<<nblk(n), NT, 0, s>>>(n, x, dy, dx); }
void copy2d(hipStream_t s, int M, int N, const float* src, int lds, float* dst, int ldd, int accumulate) {
    copy2d_kernel<<<nblk((long long)M * N), NT, 0, s>>>((long long)M * N, N, src, lds, dst, ldd, accumulate);
}
void select_ctx(hipStream_t s, int B, int T, int Cc, const float* audio, const float* null_emb, const int* cond, float* ctx) {
    const long long n = (long long)B * T * Cc;
    select_ctx_kernel<<<nblk(n), NT, 0, s>>>(n, T, Cc, audio, null_emb, cond, ctx);
}
void mask_cond_rows(hipStream_t s, int B, int T, int Cc, const int* cond, float* d) {
    const long long n = (long long)B * T * Cc;
    mask_cond_rows_kernel<<<nblk(n), NT, 0, s>>>(n, T, Cc, cond, d);
}
void split_cond_rows(hipStream_t s, int B, int T, int Cc, const int* cond, float* d, float* dc) {
    const long long n = (long long)B * T * Cc;
    split_cond_rows_kernel<<<nblk(n), NT, 0, s>>>(n, T, Cc, cond, d, dc);
}
void timestep_embedding(hipStream_t s, int B, int dim, const float* tsteps, float* e) {
    timestep_embedding_kernel<<<nblk((long long)B * dim), NT, 0, s>>>(B, dim, tsteps, e);
}
void add_noise(hipStream_t s, int B, int T, const float* x0, const float* noise, const float* sasb, const float* rec, float* noisy, float* answer) {
    add_noise_kernel<<<nblk((long long)B * T * XC), NT, 0, s>>>(B * T * XC, T, x0, noise, sasb, rec, noisy, answer);
}
void loss_residual(hipStream_t s, int n, const float* pred, const float* ans, const float* rec, float* R) {
    loss_residual_kernel<<<nblk(n), NT, 0, s>>>(n, pred, ans, rec, R);
}
void vertex_abs(hipStream_t s, long long n, float* E, double* part, int nb) { vertex_abs_kernel<<<nb, NT, 0, s>>>(n, E, part); }
void loss_final(hipStream_t s, int B, int T, const float* R, const float* GV, const double* part, int nb, long long nvert, const float* rec,
                float* dpred, float* last, double* acc) {
    loss_final_kernel<<<1, NT, 0, s>>>(B, T, R, GV, part, nb, nvert, rec, dpred, last, acc);
}

}  // namespace ut
}  // namespace said
