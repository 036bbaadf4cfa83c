// metrics.hip — the per-point passes of the evaluation metrics (said/metric/{frechet_distance,wind}.py as run by
// script/test_evaluate.py): weighted moments, the full-covariance GMM E-step, k-means assignment and k-means++ seeding,
// over fp32 (N, 64) latents with float64 products and accumulation (scikit-learn computes all of it in float64).
//
// Determinism: every sum runs in a fixed order.  A workgroup reduces its own points into one partial per output (LDS tree
// or a sequential loop, fixed by the launch shape), and reduce_parts_kernel adds the partials of all workgroups in block
// order, one thread per output.  No atomics.  The launch shape depends on N only, so equal inputs give equal bits.
//
// Precision: fp64 VALU FMAs throughout.  On gfx950 the fp64 matrix and vector rates are the same, and
// the passes here are short dot products of 64 per point, so the v_mfma_f64 layout would buy nothing but a transpose.
//
// The K x 64 x 64 algebra (Cholesky, triangular inverse, log-determinants) and the convergence tests stay on the host
// (said_amd/metric/_gmm.py); the entry points below copy their small parameters in and their results out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/said_metrics.h"
#include "engine_internal.h"

namespace {

constexpr int D = SAID_METRICS_DIM;      // latent width (BCVAE z_dim)
constexpr int KMAX = SAID_METRICS_MAX_K; // mixture components / k-means centres
constexpr int TMAX = 2 + 2;              // k-means++ local trials: 2 + floor(ln K) <= 4 for K <= 8
constexpr int PT = 256;                  // points per workgroup of the per-point kernels (one thread each)
constexpr int MOM_BLOCKS = 512;          // workgroups of the moment passes (fewer at small N)

__device__ __forceinline__ double weight_of(int wsrc, const int* __restrict__ labels, const double* __restrict__ resp, long long p, int k,
                                            int K) {
    if (wsrc == SAID_METRICS_W_UNIT) return 1.0;
    if (wsrc == SAID_METRICS_W_LABELS) return labels[p] == k ? 1.0 : 0.0;
    return resp[p * K + k];
}

// LDS tree over the PT threads of a workgroup in a fixed order; thread 0 returns the total.
__device__ __forceinline__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = PT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// Pass 1: per workgroup, n_k = sum r and s_k = sum r x over the points [b * chunk, min(N, (b + 1) * chunk)).
// 256 threads = 4 point lanes x 64 dimensions; part[b] = [K n_k | K x 64 s_k].
__global__ __launch_bounds__(256) void moments1_kernel(const float* __restrict__ X, long long N, long long chunk, int K, int wsrc,
                                                       const int* __restrict__ labels, const double* __restrict__ resp,
                                                       double* __restrict__ part) {
    __shared__ double red[4][KMAX][D + 1];
    const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long long p0 = (long long)blockIdx.x * chunk, p1 = std::min(N, p0 + chunk);
    double n[KMAX], s[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) n[k] = s[k] = 0.0;
    for (long long p = p0 + g; p < p1; p += 4) {
        const double x = (double)X[p * D + j];
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                const double w = weight_of(wsrc, labels, resp, p, k, K);
                n[k] += w;
                s[k] = fma(w, x, s[k]);
            }
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        red[g][k][j] = s[k];
        if (j == 0) red[g][k][D] = n[k];
    }
    __syncthreads();
    double* out = part + (long long)blockIdx.x * K * (D + 1);
    for (int i = threadIdx.x; i < K * (D + 1); i += 256) {
        const int k = i / (D + 1), c = i % (D + 1);
        const double v = ((red[0][k][c] + red[1][k][c]) + red[2][k][c]) + red[3][k][c];
        if (c == D) out[k] = v;
        else out[K + k * D + c] = v;
    }
}

// Pass 2: per workgroup and component, the centred scatter sum r (x - mu_k)(x - mu_k)^T over the same point ranges.
// Thread t owns the 4 x 4 tile (rows 4 (t / 16), columns 4 (t % 16)) of the 64 x 64 matrix; points are staged in LDS,
// centred, 32 at a time.  part[b] = K x 64 x 64 row-major.
constexpr int TP = 32;
__global__ __launch_bounds__(256) void moments2_kernel(const float* __restrict__ X, long long N, long long chunk, int K, int wsrc,
                                                       const int* __restrict__ labels, const double* __restrict__ resp,
                                                       const double* __restrict__ means, double* __restrict__ part) {
    __shared__ double xs[TP][D + 1];
    __shared__ double ws[TP];
    const int r0 = (threadIdx.x >> 4) * 4, c0 = (threadIdx.x & 15) * 4;
    const long long p0 = (long long)blockIdx.x * chunk, p1 = std::min(N, p0 + chunk);
    for (int k = 0; k < K; ++k) {
        double acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
        for (long long t0 = p0; t0 < p1; t0 += TP) {
            const int nt = (int)std::min<long long>(TP, p1 - t0);
            __syncthreads();
            for (int i = threadIdx.x; i < TP * D; i += 256) {
                const int pp = i / D, c = i % D;
                xs[pp][c] = pp < nt ? (double)X[(t0 + pp) * D + c] - means[k * D + c] : 0.0;
            }
            if ((int)threadIdx.x < TP) ws[threadIdx.x] = (int)threadIdx.x < nt ? weight_of(wsrc, labels, resp, t0 + threadIdx.x, k, K) : 0.0;
            __syncthreads();
            for (int pp = 0; pp < nt; ++pp) {
                const double w = ws[pp];
                double a[4], b[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    a[q] = w * xs[pp][r0 + q];
                    b[q] = xs[pp][c0 + q];
                }
#pragma unroll
                for (int qa = 0; qa < 4; ++qa)
#pragma unroll
                    for (int qb = 0; qb < 4; ++qb) acc[qa][qb] = fma(a[qa], b[qb], acc[qa][qb]);
            }
        }
        double* out = part + ((long long)blockIdx.x * K + k) * D * D;
#pragma unroll
        for (int qa = 0; qa < 4; ++qa)
#pragma unroll
            for (int qb = 0; qb < 4; ++qb) out[(r0 + qa) * D + c0 + qb] = acc[qa][qb];
    }
}

// out[m] = sum over blocks b (in order) of part[b * M + m]
__global__ __launch_bounds__(256) void reduce_parts_kernel(const double* __restrict__ part, int nblk, int M, double* __restrict__ out) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(long long)b * M + m];
    out[m] = s;
}

// GaussianMixture._estimate_log_prob_resp for covariance_type="full", one thread per point:
//   y = x U_k - (mu_k U_k);  log N_k = -0.5 (d log 2 pi + sum y^2) + log_det_k;  + log w_k;  logsumexp over k.
// U_k (upper triangular, row-major [i][j]) is read at wave-uniform addresses (scalar loads).  Writes log_resp and resp =
// exp(log_resp) (N, K), log_prob_norm (N) and one partial sum of log_prob_norm per workgroup.
__global__ __launch_bounds__(256) void estep_kernel(const float* __restrict__ X, long long N, int K, const double* __restrict__ prm,
                                                    double* __restrict__ log_resp, double* __restrict__ resp, double* __restrict__ lpn,
                                                    double* __restrict__ part) {
    __shared__ double red[PT];
    // prm: U [K][D][D] | muU [K][D] | log_det [K] | log_w [K] | d log(2 pi)
    const double* U = prm;
    const double* muU = prm + K * D * D;
    const double* logdet = muU + K * D;
    const double* logw = logdet + K;
    const double c0 = logw[K];
    const long long p = (long long)blockIdx.x * PT + threadIdx.x;
    const bool live = p < N;
    double x[D];
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = live ? (double)X[p * D + i] : 0.0;
    // log_resp[p] holds the weighted log-probabilities until the normaliser is known (no per-thread array indexed by k)
    double* lrow = log_resp + (live ? p : 0) * K;
    double mx = -INFINITY;
    for (int k = 0; k < K; ++k) {
        const double* Uk = U + k * D * D;
        double sq = 0.0;
#pragma unroll
        for (int jj = 0; jj < D; ++jj) {
            double y = 0.0;
#pragma unroll
            for (int i = 0; i <= jj; ++i) y = fma(x[i], Uk[i * D + jj], y);
            y -= muU[k * D + jj];
            sq = fma(y, y, sq);
        }
        const double lp = (-0.5 * (c0 + sq) + logdet[k]) + logw[k];
        if (live) lrow[k] = lp;
        mx = fmax(mx, lp);
    }
    double se = 0.0;
    if (live)
        for (int k = 0; k < K; ++k) se += exp(lrow[k] - mx);
    const double norm = live ? log(se) + mx : 0.0;
    if (live) {
        for (int k = 0; k < K; ++k) {
            const double lr = lrow[k] - norm;
            lrow[k] = lr;
            resp[p * K + k] = exp(lr);
        }
        lpn[p] = norm;
    }
    const double tot = block_sum(norm, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// k-means assignment as in scikit-learn's _update_chunk_dense: d_k = |c_k|^2 - 2 x.c_k, the first minimum wins (ties go to
// the lower index).  Also the exact squared distance to the chosen centre and, per workgroup, [changed labels, sum of
// those distances] (labels_old null: nothing is compared).  prm: C [K][D] | |c_k|^2 [K].
__global__ __launch_bounds__(256) void assign_kernel(const float* __restrict__ X, long long N, int K, const double* __restrict__ prm,
                                                     int* __restrict__ labels, const int* __restrict__ labels_old, double* __restrict__ mind,
                                                     double* __restrict__ part) {
    __shared__ double red[PT];
    const double* C = prm;
    const double* cn = prm + K * D;
    const long long p = (long long)blockIdx.x * PT + threadIdx.x;
    const bool live = p < N;
    double x[D];
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = live ? (double)X[p * D + i] : 0.0;
    double best = INFINITY;
    int lab = 0;
    for (int k = 0; k < K; ++k) {
        double dot = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) dot = fma(x[i], C[k * D + i], dot);
        const double dk = cn[k] - 2.0 * dot;
        if (dk < best) { best = dk; lab = k; }
    }
    double dist = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const double e = x[i] - C[lab * D + i];
        dist = fma(e, e, dist);
    }
    double changed = 0.0;
    if (live) {
        if (labels_old) changed = labels_old[p] != lab ? 1.0 : 0.0;
        labels[p] = lab;
        mind[p] = dist;
    }
    const double c = block_sum(changed, red);
    const double s = block_sum(live ? dist : 0.0, red);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = c;
        part[2 * blockIdx.x + 1] = s;
    }
}

// k-means++ (scikit-learn's _kmeans_plusplus): for each of T candidate points, dist[t][p] = min(closest[p], |x_p - x_cand|^2)
// (closest null: no minimum, the first centre) and one partial sum of dist[t] per workgroup: part[b * T + t].
__global__ __launch_bounds__(256) void kpp_dist_kernel(const float* __restrict__ X, long long N, int T, const long long* __restrict__ cand,
                                                       const double* __restrict__ closest, double* __restrict__ dist, double* __restrict__ part) {
    __shared__ double red[PT];
    const long long p = (long long)blockIdx.x * PT + threadIdx.x;
    const bool live = p < N;
    double x[D];
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = live ? (double)X[p * D + i] : 0.0;
    for (int t = 0; t < T; ++t) {
        const float* c = X + cand[t] * D;
        double d2 = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double e = x[i] - (double)c[i];
            d2 = fma(e, e, d2);
        }
        if (closest && live) d2 = fmin(closest[p], d2);
        if (live) dist[(long long)t * N + p] = d2;
        const double s = block_sum(live ? d2 : 0.0, red);
        if (threadIdx.x == 0) part[(long long)blockIdx.x * T + t] = s;
    }
}

// np.searchsorted(cumsum(closest), r) for T values r, one thread each: walk the workgroup partials (kpp_dist_kernel's
// column `col` of `part`, nblk x stride), then the points of the block found, in order.  The first index whose running sum
// reaches r; clipped to the block's last point (and to N - 1) when rounding leaves the sum short.
__global__ void kpp_search_kernel(const double* __restrict__ closest, long long N, const double* __restrict__ part, int nblk, int stride,
                                  int col, const double* __restrict__ rvals, int T, long long* __restrict__ cand) {
    const int t = threadIdx.x;
    if (t >= T) return;
    const double r = rvals[t];
    double acc = 0.0;
    int b = 0;
    for (; b < nblk - 1; ++b) {
        const double v = part[(long long)b * stride + col];
        if (acc + v >= r) break;
        acc += v;
    }
    const long long p0 = (long long)b * PT, p1 = std::min(N, p0 + PT);
    long long id = p1 - 1;
    for (long long p = p0; p < p1; ++p) {
        acc += closest[p];
        if (acc >= r) { id = p; break; }
    }
    cand[t] = id;
}

}  // namespace

struct said_metrics {
    HostCtx c;
    long long maxN = 0;
    int pblk = 0;                   // ceil(maxN / PT)
    double *log_resp = nullptr, *resp = nullptr, *lpn = nullptr, *mind = nullptr, *closest = nullptr, *kdist = nullptr;
    int* labels[2] = {nullptr, nullptr};
    int cur = 0;                    // labels[cur] holds the last assignment
    bool have_labels = false, have_resp = false, have_closest = false;
    int resp_k = 0, labels_k = 0;
    double *part = nullptr, *red = nullptr, *prm = nullptr, *cpart = nullptr;   // partials, reduced values, parameters, closest's partials
    long long* cand = nullptr;
};

namespace {
int mom_blocks(long long n) { return (int)std::min<long long>(MOM_BLOCKS, (n + PT - 1) / PT); }
long long mom_chunk(long long n) { const int b = mom_blocks(n); return (n + b - 1) / b; }

int check_x(said_metrics* m, const float* x_dev, long long n, int k, const char* what) {
    HostCtx* ctx = &m->c;
    if (!x_dev || n < 1) return fail(ctx, "%s: need a device buffer of n >= 1 points", what);
    if (n > m->maxN) return fail(ctx, "%s: %lld points exceed this context's max_points %lld", what, n, m->maxN);
    if (k < 1 || k > KMAX) return fail(ctx, "%s: k = %d outside [1, %d]", what, k, KMAX);
    return 0;
}

int check_wsrc(said_metrics* m, int wsrc, int k, const char* what) {
    HostCtx* ctx = &m->c;
    if (wsrc == SAID_METRICS_W_UNIT && k != 1) return fail(ctx, "%s: unit weights need k = 1", what);
    if (wsrc == SAID_METRICS_W_LABELS && (!m->have_labels || m->labels_k != k))
        return fail(ctx, "%s: no k-means labels for k = %d (run said_metrics_kmeans_assign first)", what, k);
    if (wsrc == SAID_METRICS_W_RESP && (!m->have_resp || m->resp_k != k))
        return fail(ctx, "%s: no responsibilities for k = %d (run said_metrics_gmm_estep first)", what, k);
    if (wsrc < 0 || wsrc > SAID_METRICS_W_RESP) return fail(ctx, "%s: unknown weight source %d", what, wsrc);
    return 0;
}

// reduce nblk x M partials in block order and copy the M sums to the host (synchronises the stream)
int reduce_to_host(said_metrics* m, const double* part, int nblk, int M, double* out_host, hipStream_t s) {
    HostCtx* ctx = &m->c;
    reduce_parts_kernel<<<(M + 255) / 256, 256, 0, s>>>(part, nblk, M, m->red);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_host, m->red, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}
}  // namespace

extern "C" {

int said_metrics_create(said_metrics** out, int device, long long max_points) {
    DeviceRestore restore_device;
    said_metrics* m = new_ctx("said_metrics_create", out, device);
    if (!m) return -1;
    if (max_points < 1 || max_points > (1LL << 30)) { delete m; return fail(nullptr, "said_metrics_create: max_points %lld outside [1, 2^30]", max_points); }
    HostCtx* ctx = &m->c;
    m->maxN = max_points;
    m->pblk = (int)((max_points + PT - 1) / PT);
    const size_t N = (size_t)max_points;
    const size_t part_n = std::max({(size_t)MOM_BLOCKS * KMAX * D * D, (size_t)m->pblk * 2, (size_t)m->pblk * TMAX});
    const size_t prm_n = (size_t)KMAX * D * D + KMAX * D + 2 * KMAX + 1;
    if (dalloc(ctx, &m->log_resp, N * KMAX, false) || dalloc(ctx, &m->resp, N * KMAX, false) || dalloc(ctx, &m->lpn, N, false) ||
        dalloc(ctx, &m->mind, N, false) || dalloc(ctx, &m->closest, N, false) || dalloc(ctx, &m->kdist, N * TMAX, false) ||
        dalloc(ctx, &m->labels[0], N, false) || dalloc(ctx, &m->labels[1], N, false) || dalloc(ctx, &m->part, part_n, false) ||
        dalloc(ctx, &m->red, (size_t)KMAX * D * D, false) || dalloc(ctx, &m->prm, prm_n, false) || dalloc(ctx, &m->cpart, (size_t)m->pblk, false) ||
        dalloc(ctx, &m->cand, (size_t)TMAX, false)) {
        g_create_err = ctx->err;
        said_metrics_destroy(m);
        return -1;
    }
    *out = m;
    return 0;
}

int said_metrics_destroy(said_metrics* m) { return delete_ctx(m); }

const char* said_metrics_last_error(const said_metrics* m) { return ctx_error(m); }

long long said_metrics_max_points(const said_metrics* m) { return m ? m->maxN : 0; }

int said_metrics_weighted_sums(said_metrics* m, const float* x_dev, long long n, int k, int wsrc, double* nk_host, double* sum_host, void* stream) {
    if (!m) return -1;
    HostCtx* ctx = &m->c;
    if (check_x(m, x_dev, n, k, "said_metrics_weighted_sums") || check_wsrc(m, wsrc, k, "said_metrics_weighted_sums")) return -1;
    if (!nk_host || !sum_host) return fail(ctx, "said_metrics_weighted_sums: null output");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    const int nb = mom_blocks(n);
    moments1_kernel<<<nb, 256, 0, s>>>(x_dev, n, mom_chunk(n), k, wsrc, m->labels[m->cur], m->resp, m->part);
    HIPCHK(hipGetLastError());
    std::vector<double> r((size_t)k * (D + 1));
    if (reduce_to_host(m, m->part, nb, k * (D + 1), r.data(), s)) return -1;
    std::copy(r.begin(), r.begin() + k, nk_host);
    std::copy(r.begin() + k, r.end(), sum_host);
    return 0;
}

int said_metrics_weighted_scatter(said_metrics* m, const float* x_dev, long long n, int k, int wsrc, const double* means_host, double* scatter_host,
                                  void* stream) {
    if (!m) return -1;
    HostCtx* ctx = &m->c;
    if (check_x(m, x_dev, n, k, "said_metrics_weighted_scatter") || check_wsrc(m, wsrc, k, "said_metrics_weighted_scatter")) return -1;
    if (!means_host || !scatter_host) return fail(ctx, "said_metrics_weighted_scatter: null argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(m->prm, means_host, (size_t)k * D * sizeof(double), hipMemcpyHostToDevice, s));
    const int nb = mom_blocks(n);
    moments2_kernel<<<nb, 256, 0, s>>>(x_dev, n, mom_chunk(n), k, wsrc, m->labels[m->cur], m->resp, m->prm, m->part);
    HIPCHK(hipGetLastError());
    return reduce_to_host(m, m->part, nb, k * D * D, scatter_host, s);
}

int said_metrics_gmm_estep(said_metrics* m, const float* x_dev, long long n, int k, const double* prec_chol_host, const double* mean_prec_host,
                           const double* log_det_host, const double* log_weights_host, double* lower_bound_host, double* log_resp_dev,
                           double* log_prob_norm_dev, void* stream) {
    if (!m) return -1;
    HostCtx* ctx = &m->c;
    if (check_x(m, x_dev, n, k, "said_metrics_gmm_estep")) return -1;
    if (!prec_chol_host || !mean_prec_host || !log_det_host || !log_weights_host || !lower_bound_host)
        return fail(ctx, "said_metrics_gmm_estep: null argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<double> prm((size_t)k * D * D + k * D + 2 * k + 1);
    std::copy(prec_chol_host, prec_chol_host + (size_t)k * D * D, prm.begin());
    std::copy(mean_prec_host, mean_prec_host + (size_t)k * D, prm.begin() + (size_t)k * D * D);
    std::copy(log_det_host, log_det_host + k, prm.begin() + (size_t)k * D * D + k * D);
    std::copy(log_weights_host, log_weights_host + k, prm.begin() + (size_t)k * D * D + k * D + k);
    prm.back() = D * std::log(2 * M_PI);   // scikit-learn: n_features * np.log(2 * np.pi)
    HIPCHK(hipMemcpyAsync(m->prm, prm.data(), prm.size() * sizeof(double), hipMemcpyHostToDevice, s));
    const int nb = (int)((n + PT - 1) / PT);
    estep_kernel<<<nb, PT, 0, s>>>(x_dev, n, k, m->prm, m->log_resp, m->resp, m->lpn, m->part);
    HIPCHK(hipGetLastError());
    m->have_resp = true;
    m->resp_k = k;
    if (log_resp_dev) HIPCHK(hipMemcpyAsync(log_resp_dev, m->log_resp, (size_t)n * k * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (log_prob_norm_dev) HIPCHK(hipMemcpyAsync(log_prob_norm_dev, m->lpn, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    double tot = 0.0;
    if (reduce_to_host(m, m->part, nb, 1, &tot, s)) return -1;
    *lower_bound_host = tot / (double)n;
    return 0;
}

int said_metrics_kmeans_assign(said_metrics* m, const float* x_dev, long long n, int k, const double* centres_host, int compare,
                               long long* n_changed_host, double* inertia_host, void* stream) {
    if (!m) return -1;
    HostCtx* ctx = &m->c;
    if (check_x(m, x_dev, n, k, "said_metrics_kmeans_assign")) return -1;
    if (!centres_host) return fail(ctx, "said_metrics_kmeans_assign: null centres");
    if (compare && (!m->have_labels || m->labels_k != k)) return fail(ctx, "said_metrics_kmeans_assign: no earlier labels to compare with");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<double> prm((size_t)k * D + k);
    for (int c = 0; c < k; ++c) {
        double sq = 0.0;   // scikit-learn: row_norms(centers, squared=True)
        for (int i = 0; i < D; ++i) {
            prm[(size_t)c * D + i] = centres_host[(size_t)c * D + i];
            sq += centres_host[(size_t)c * D + i] * centres_host[(size_t)c * D + i];
        }
        prm[(size_t)k * D + c] = sq;
    }
    HIPCHK(hipMemcpyAsync(m->prm, prm.data(), prm.size() * sizeof(double), hipMemcpyHostToDevice, s));
    const int nb = (int)((n + PT - 1) / PT);
    const int nxt = compare ? 1 - m->cur : m->cur;
    assign_kernel<<<nb, PT, 0, s>>>(x_dev, n, k, m->prm, m->labels[nxt], compare ? m->labels[m->cur] : nullptr, m->mind, m->part);
    HIPCHK(hipGetLastError());
    m->cur = nxt;
    m->have_labels = true;
    m->labels_k = k;
    double r[2] = {0.0, 0.0};
    if (reduce_to_host(m, m->part, nb, 2, r, s)) return -1;
    if (n_changed_host) *n_changed_host = compare ? (long long)r[0] : n;
    if (inertia_host) *inertia_host = r[1];
    return 0;
}

int said_metrics_kmeans_read(said_metrics* m, long long n, int* labels_host, double* dist_host, void* stream) {
    if (!m) return -1;
    HostCtx* ctx = &m->c;
    if (!m->have_labels || n < 1 || n > m->maxN) return fail(ctx, "said_metrics_kmeans_read: no labels of %lld points", n);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    if (labels_host) HIPCHK(hipMemcpyAsync(labels_host, m->labels[m->cur], (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    if (dist_host) HIPCHK(hipMemcpyAsync(dist_host, m->mind, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int said_metrics_kmeans_set_labels(said_metrics* m, long long n, int k, const int* labels_host, void* stream) {
    if (!m) return -1;
    HostCtx* ctx = &m->c;
    if (!labels_host || n < 1 || n > m->maxN || k < 1 || k > KMAX) return fail(ctx, "said_metrics_kmeans_set_labels: bad arguments");
    for (long long p = 0; p < n; ++p)
        if (labels_host[p] < 0 || labels_host[p] >= k) return fail(ctx, "said_metrics_kmeans_set_labels: label %d at %lld outside [0, %d)", labels_host[p], p, k);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(m->labels[m->cur], labels_host, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    m->have_labels = true;
    m->labels_k = k;
    return 0;
}

int said_metrics_kmeanspp_first(said_metrics* m, const float* x_dev, long long n, long long centre_id, double* pot_host, void* stream) {
    if (!m) return -1;
    HostCtx* ctx = &m->c;
    if (check_x(m, x_dev, n, 1, "said_metrics_kmeanspp_first")) return -1;
    if (centre_id < 0 || centre_id >= n || !pot_host) return fail(ctx, "said_metrics_kmeanspp_first: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(m->cand, &centre_id, sizeof(long long), hipMemcpyHostToDevice, s));
    const int nb = (int)((n + PT - 1) / PT);
    kpp_dist_kernel<<<nb, PT, 0, s>>>(x_dev, n, 1, m->cand, nullptr, m->closest, m->cpart);
    HIPCHK(hipGetLastError());
    m->have_closest = true;
    return reduce_to_host(m, m->cpart, nb, 1, pot_host, s);
}

int said_metrics_kmeanspp_step(said_metrics* m, const float* x_dev, long long n, const double* rand_host, int trials, long long* centre_id_host,
                               double* pot_host, void* stream) {
    if (!m) return -1;
    HostCtx* ctx = &m->c;
    if (check_x(m, x_dev, n, 1, "said_metrics_kmeanspp_step")) return -1;
    if (!m->have_closest) return fail(ctx, "said_metrics_kmeanspp_step: run said_metrics_kmeanspp_first first");
    if (trials < 1 || trials > TMAX || !rand_host || !centre_id_host || !pot_host) return fail(ctx, "said_metrics_kmeanspp_step: bad arguments (trials in [1, %d])", TMAX);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    const int nb = (int)((n + PT - 1) / PT);
    HIPCHK(hipMemcpyAsync(m->prm, rand_host, (size_t)trials * sizeof(double), hipMemcpyHostToDevice, s));
    kpp_search_kernel<<<1, 64, 0, s>>>(m->closest, n, m->cpart, nb, 1, 0, m->prm, trials, m->cand);
    kpp_dist_kernel<<<nb, PT, 0, s>>>(x_dev, n, trials, m->cand, m->closest, m->kdist, m->part);
    HIPCHK(hipGetLastError());
    std::vector<double> pots(trials);
    if (reduce_to_host(m, m->part, nb, trials, pots.data(), s)) return -1;
    long long ids[TMAX];
    HIPCHK(hipMemcpyAsync(ids, m->cand, (size_t)trials * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int best = 0;   // np.argmin: the first minimum
    for (int t = 1; t < trials; ++t)
        if (pots[t] < pots[best]) best = t;
    HIPCHK(hipMemcpyAsync(m->closest, m->kdist + (size_t)best * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    // the chosen candidate's partials become closest's (column `best` of the nb x trials partials)
    HIPCHK(hipMemcpy2DAsync(m->cpart, sizeof(double), m->part + best, (size_t)trials * sizeof(double), sizeof(double), nb, hipMemcpyDeviceToDevice, s));
    *centre_id_host = ids[best];
    *pot_host = pots[best];
    return 0;
}

}  // extern "C"
