// beat.hip — beat consistency and vertex error on the device (C ABI: include/said_beat.h; host side: beat_ctx.cpp).
// Everything is float64.  Every sum runs in a fixed order (ascending within a thread, then one fixed tree over the workgroup's threads), there
// are no atomics, and sin / cos never run here: the window, the twiddles and the mel bank are host tables.
#include "beat_kernels.h"

#include <cfloat>

namespace said {
namespace beat {

namespace {

constexpr int NT = 256;
constexpr int FRAME_BLOCK = VERTEX_FRAME_BLOCK;   // frames of a pair one workgroup of the vertex error takes
constexpr int MAC_TILE = 2048;    // doubles of per-sequence means coeff_mac_kernel stages at a time (at least 8 sequences of 256 channels)

// one fixed tree over the workgroup's NT values; `red` holds NT doubles and may be reused after the call
template <typename Op>
__device__ inline double block_reduce(double v, double* red, Op op) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = op(red[tid], red[tid + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
struct OpSum { __device__ double operator()(double a, double b) const { return a + b; } };
struct OpMax { __device__ double operator()(double a, double b) const { return a > b ? a : b; } };
struct OpMin { __device__ double operator()(double a, double b) const { return a < b ? a : b; } };

// the segment of x in start[0 .. n] (ascending, start[0] = 0 <= x < start[n]): the last i with start[i] <= x
__device__ inline int find_segment(const int* start, int n, int x) {
    int lo = 0, hi = n;   // start[lo] <= x < start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// One STFT frame per workgroup: the 2048 windowed samples as 1024 complex points z[n] = x[2 n] + i x[2 n + 1], a radix-2 transform in LDS
// (bit-reversed load, ten in-place stages), the real-transform split into 1025 powers, and the 128 mel bands.
__global__ __launch_bounds__(NT) void mel_power_kernel(const float* __restrict__ wave, int n_clips, int total_frames, const Tables* __restrict__ t, ClipWork w) {
    __shared__ double re[HALF], im[HALF], pw[N_BINS];
    const int tid = threadIdx.x, f = blockIdx.x;
    if (f >= total_frames) return;
    const int c = find_segment(w.frame_start, n_clips, f);
    const long long base = w.clip_off[c], len = w.clip_off[c + 1] - base;
    const long long p0 = (long long)HOP * (f - w.frame_start[c]) - HALF;   // centred: 1024 zeros before the clip
    for (int n = tid; n < HALF; n += NT) {
        const long long p = p0 + 2 * n;
        const double a = (p >= 0 && p < len) ? (double)wave[base + p] * t->window[2 * n] : 0.0;
        const double b = (p + 1 >= 0 && p + 1 < len) ? (double)wave[base + p + 1] * t->window[2 * n + 1] : 0.0;
        const int r = (int)(__brev((unsigned)n) >> 22);
        re[r] = a;
        im[r] = b;
    }
    __syncthreads();
    for (int s = 0; s < 10; ++s) {
        const int half = 1 << s;
        for (int j = tid; j < HALF / 2; j += NT) {
            const int pos = j & (half - 1), i0 = ((j >> s) << (s + 1)) + pos, i1 = i0 + half, k = pos << (9 - s);
            const double wr = t->tw_re[k], wi = t->tw_im[k];
            const double xr = re[i1], xi = im[i1], ur = re[i0], ui = im[i0];
            const double vr = xr * wr - xi * wi, vi = xr * wi + xi * wr;
            re[i0] = ur + vr;
            im[i0] = ui + vi;
            re[i1] = ur - vr;
            im[i1] = ui - vi;
        }
        __syncthreads();
    }
    // X[k] = E[k] + W^k O[k], E = (Z[k] + conj Z[-k]) / 2, O = -i (Z[k] - conj Z[-k]) / 2, indices mod 1024
    for (int k = tid; k < N_BINS; k += NT) {
        const int a = k & (HALF - 1), b = (HALF - k) & (HALF - 1);
        const double zr = re[a], zi = im[a], cr = re[b], ci = -im[b];
        const double er = (zr + cr) * 0.5, ei = (zi + ci) * 0.5, dr = (zr - cr) * 0.5, di = (zi - ci) * 0.5;
        const double o_r = di, o_i = -dr, wr = t->sp_re[k], wi = t->sp_im[k];
        const double xr = er + (wr * o_r - wi * o_i), xi = ei + (wr * o_i + wi * o_r);
        pw[k] = xr * xr + xi * xi;
    }
    __syncthreads();
    if (tid < N_MELS) {
        const int first = t->mel_first[tid], last = t->mel_last[tid];
        const double* wt = t->weights + t->mel_woff[tid];
        double acc = 0.0;
        for (int b = first; b < last; ++b) acc += wt[b - first] * pw[b];
        w.mel[(size_t)f * N_MELS + tid] = acc;
    }
}

// One clip per workgroup: dB with the 80 dB floor under the clip's maximum, the flux envelope, its normalisation, the two window tests of
// every frame, and the greedy pass over `wait` by one thread.
__global__ __launch_bounds__(NT) void onset_pick_kernel(int n_clips, PeakPick pp, ClipWork w) {
    __shared__ double red[NT];
    const int tid = threadIdx.x, c = blockIdx.x;
    if (c >= n_clips) return;
    const int f0 = w.frame_start[c], nf = w.frame_start[c + 1] - f0;
    const double* mel = w.mel + (size_t)f0 * N_MELS;
    double* db = w.db + (size_t)f0 * N_MELS;
    double* env = w.env + f0;
    double* xn = w.xn + f0;
    int* flag = w.flag + f0;

    double m = -DBL_MAX;
    for (size_t i = tid; i < (size_t)nf * N_MELS; i += NT) {
        const double v = mel[i];
        const double d = 10.0 * log10(v > 1e-10 ? v : 1e-10);
        db[i] = d;
        m = d > m ? d : m;
    }
    const double floor_db = block_reduce(m, red, OpMax()) - 80.0;   // (its barriers also publish db to the workgroup)

    // envelope: three zeros, then the flux of frame i - 2 against frame i - 3; one wave per frame, two bands per lane, one shuffle tree
    const int wave = tid >> 6, lane = tid & 63;
    for (int i = wave; i < nf; i += NT / 64) {
        double v = 0.0;
        if (i >= 3) {
            const double* cur = db + (size_t)(i - 2) * N_MELS;
            const double* prev = cur - N_MELS;
            double a0 = cur[lane], b0 = prev[lane], a1 = cur[lane + 64], b1 = prev[lane + 64];
            a0 = a0 > floor_db ? a0 : floor_db;
            b0 = b0 > floor_db ? b0 : floor_db;
            a1 = a1 > floor_db ? a1 : floor_db;
            b1 = b1 > floor_db ? b1 : floor_db;
            const double d0 = a0 - b0, d1 = a1 - b1;
            v = (d0 > 0.0 ? d0 : 0.0) + (d1 > 0.0 ? d1 : 0.0);
            for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
            v = v / (double)N_MELS;
        }
        if (lane == 0) env[i] = v;
    }
    __syncthreads();

    double mx = -DBL_MAX, mn = DBL_MAX;
    for (int i = tid; i < nf; i += NT) {
        const double v = env[i];
        mx = v > mx ? v : mx;
        mn = v < mn ? v : mn;
    }
    mx = block_reduce(mx, red, OpMax());
    mn = block_reduce(mn, red, OpMin());
    if (!(mx != 0.0 || mn != 0.0)) {   // no non-zero value: no onsets (uniform over the workgroup)
        if (tid == 0) w.onset_count[c] = 0;
        return;
    }
    const double scale = (mx - mn) + DBL_MIN;
    for (int i = tid; i < nf; i += NT) xn[i] = (env[i] - mn) / scale;
    __syncthreads();

    for (int n = tid; n < nf; n += NT) {
        const double x = xn[n];
        int lo = n - pp.pre_max, hi = n + pp.post_max;
        lo = lo < 0 ? 0 : lo;
        hi = hi > nf ? nf : hi;
        bool is_max = true;
        for (int i = lo; i < hi; ++i) is_max = is_max && x >= xn[i];
        lo = n - pp.pre_avg;
        hi = n + pp.post_avg;
        lo = lo < 0 ? 0 : lo;
        hi = hi > nf ? nf : hi;
        double sum = 0.0;
        for (int i = lo; i < hi; ++i) sum += xn[i];
        flag[n] = (is_max && x >= sum / (double)(hi - lo) + pp.delta) ? 1 : 0;
    }
    __syncthreads();

    if (tid == 0) {
        int* out = w.onsets + f0;
        int count = 0;
        long long last = -(1LL << 40);
        for (int n = 0; n < nf; ++n)
            if (flag[n] && n > last + pp.wait) {
                out[count++] = n;
                last = n;
            }
        w.onset_count[c] = count;
    }
}

// seq_mean[s, ch] = mean over t of |c[t + 1, ch] - c[t, ch]|, t ascending; one sequence per workgroup, one channel per thread
__global__ __launch_bounds__(NT) void coeff_mean_diff_kernel(const float* __restrict__ coeffs, int n_seq, int channels, SeqWork w) {
    const int s = blockIdx.x, ch = threadIdx.x;
    if (s >= n_seq || ch >= channels) return;
    const long long o = w.seq_off[s];
    const int T = (int)(w.seq_off[s + 1] - o);
    const float* c = coeffs + o * channels + ch;
    double acc = 0.0, prev = (double)c[0];
    for (int t = 1; t < T; ++t) {
        const double cur = (double)c[(size_t)t * channels];
        acc += fabs(cur - prev);
        prev = cur;
    }
    w.seq_mean[(size_t)s * channels + ch] = acc / (double)(T - 1);
}

// mac[ch] = mean over the sequences, ascending; one workgroup
// (all threads stage MAC_TILE / channels sequences' means in LDS at a time, so that the ascending sum of a channel does not wait for one
// memory round trip per sequence)
__global__ __launch_bounds__(NT) void coeff_mac_kernel(int n_seq, int channels, SeqWork w) {
    __shared__ double tile[MAC_TILE];
    const int tid = threadIdx.x, rows = MAC_TILE / channels;
    double acc = 0.0;
    for (int s0 = 0; s0 < n_seq; s0 += rows) {
        const int nr = n_seq - s0 < rows ? n_seq - s0 : rows;
        const double* src = w.seq_mean + (size_t)s0 * channels;
        for (int i = tid; i < nr * channels; i += NT) tile[i] = src[i];
        __syncthreads();
        if (tid < channels)
            for (int r = 0; r < nr; ++r) acc += tile[r * channels + tid];
        __syncthreads();
    }
    if (tid < channels) w.mac[tid] = acc / (double)n_seq;
}

// One sequence per workgroup: r[t] = mean over the channels (ascending) of |difference| / mac, then the local minima of r by scipy's
// find_peaks rule on -r (a plateau's middle, rounded down; the ends are never peaks), kept when one side rises by more than `threshold`.
__global__ __launch_bounds__(NT) void coeff_rate_kernel(const float* __restrict__ coeffs, int n_seq, int channels, double threshold, SeqWork w) {
    __shared__ double mac[256];
    const int s = blockIdx.x, tid = threadIdx.x;
    if (s >= n_seq) return;
    const long long o = w.seq_off[s];
    const int n = (int)(w.seq_off[s + 1] - o) - 1;   // rates of this sequence
    if (tid < channels) mac[tid] = w.mac[tid];
    __syncthreads();
    double* r = w.rates + o;
    int* mark = w.minima + o;   // first 0 / 1 per index, compacted in place below (a kept index is never below its position in the list)
    for (int t = tid; t < n; t += NT) {
        const float* c0 = coeffs + (o + t) * channels;
        const float* c1 = c0 + channels;
        double acc = 0.0;
        for (int ch = 0; ch < channels; ++ch) acc += fabs((double)c1[ch] - (double)c0[ch]) / mac[ch];
        r[t] = acc / (double)channels;
    }
    if (tid == 0) r[n] = 0.0;   // the unused last slot of the sequence
    __syncthreads();
    for (int t = tid; t <= n; t += NT) mark[t] = 0;
    __syncthreads();
    for (int i = tid + 1; i < n - 1; i += NT) {   // i: the first index of a run of equal values that was entered downwards
        if (!(r[i - 1] > r[i])) continue;
        int j = i;
        while (j + 1 < n && r[j + 1] == r[j]) ++j;
        if (j + 1 >= n || !(r[j + 1] > r[j])) continue;
        const int p = (i + j) / 2;
        if (r[p - 1] - r[p] > threshold || r[p + 1] - r[p] > threshold) mark[p] = 1;
    }
    __syncthreads();
    if (tid == 0) {
        int count = 0;
        for (int t = 0; t < n; ++t)
            if (mark[t]) mark[count++] = t;
        w.min_count[s] = count;
    }
}

// One sequence per workgroup: mean over its clip's onsets a of exp(-min_k (a - k)^2 / (2 sigma^2)); 0 without a kinematic beat, 0 / 0 = NaN
// without an onset.
__global__ __launch_bounds__(NT) void beat_score_kernel(int n_seq, const int* __restrict__ clip_index, ClipWork cw, SeqWork sw, double sampling_rate, double fps,
                                                        double sigma, double* __restrict__ scores) {
    __shared__ double red[NT];
    const int s = blockIdx.x, tid = threadIdx.x;
    if (s >= n_seq) return;
    const int nk = sw.min_count[s];
    if (nk == 0) {
        if (tid == 0) scores[s] = 0.0;
        return;
    }
    const int c = clip_index[s], na = cw.onset_count[c];
    const int* onsets = cw.onsets + cw.frame_start[c];
    const int* minima = sw.minima + sw.seq_off[s];
    const double denom = 2.0 * (sigma * sigma);
    double acc = 0.0;
    for (int a = tid; a < na; a += NT) {
        const double ta = (double)(onsets[a] * HOP) / sampling_rate;
        double best = DBL_MAX;
        for (int k = 0; k < nk; ++k) {
            const double d = ta - (double)minima[k] / fps, d2 = d * d;
            best = d2 < best ? d2 : best;
        }
        acc += exp(-best / denom);
    }
    acc = block_reduce(acc, red, OpSum());
    if (tid == 0) scores[s] = acc / (double)na;
}

// FRAME_BLOCK consecutive frames of one pair per workgroup (a delta is read once for all of them; a frame's result does not depend on the
// block it is in): e = sqrt(sum over the 3V columns of (sum over c of (real - eval)[c] delta[c, column])^2), c ascending, columns strided over
// the threads and then one fixed tree.
__global__ __launch_bounds__(NT) void vertex_frame_kernel(const float* __restrict__ coeffs, int n_pairs, int total_blocks, const int* __restrict__ block_start,
                                                          const int* __restrict__ pair_start, const long long* __restrict__ real_off,
                                                          const long long* __restrict__ eval_off, const int* __restrict__ person,
                                                          const double* __restrict__ deltas, int channels, int n3v, double* __restrict__ frame_err) {
    __shared__ double red[NT];
    __shared__ double diff[FRAME_BLOCK][256];
    const int blk = blockIdx.x, tid = threadIdx.x;
    if (blk >= total_blocks) return;
    const int p = find_segment(block_start, n_pairs, blk), t0 = (blk - block_start[p]) * FRAME_BLOCK;
    const int len = pair_start[p + 1] - pair_start[p];
    const int nf = len - t0 < FRAME_BLOCK ? len - t0 : FRAME_BLOCK;   // frames of this block; the rows past them are zero
    for (int i = tid; i < FRAME_BLOCK * channels; i += NT) {
        const int f = i / channels, c = i - f * channels;
        diff[f][c] = f < nf ? (double)coeffs[(real_off[p] + t0 + f) * channels + c] - (double)coeffs[(eval_off[p] + t0 + f) * channels + c] : 0.0;
    }
    __syncthreads();
    const double* d = deltas + (size_t)person[p] * channels * n3v;
    double acc[FRAME_BLOCK];
#pragma unroll
    for (int f = 0; f < FRAME_BLOCK; ++f) acc[f] = 0.0;
    for (int j = tid; j < n3v; j += NT) {
        double v[FRAME_BLOCK];
#pragma unroll
        for (int f = 0; f < FRAME_BLOCK; ++f) v[f] = 0.0;
        for (int c = 0; c < channels; ++c) {
            const double w = d[(size_t)c * n3v + j];
#pragma unroll
            for (int f = 0; f < FRAME_BLOCK; ++f) v[f] += diff[f][c] * w;
        }
#pragma unroll
        for (int f = 0; f < FRAME_BLOCK; ++f) acc[f] += v[f] * v[f];
    }
#pragma unroll
    for (int f = 0; f < FRAME_BLOCK; ++f) {
        const double e = block_reduce(acc[f], red, OpSum());
        if (tid == 0 && f < nf) frame_err[pair_start[p] + t0 + f] = sqrt(e);
    }
}

// the maximum over a pair's frames; one pair per workgroup
__global__ __launch_bounds__(NT) void vertex_max_kernel(int n_pairs, const int* __restrict__ pair_start, const double* __restrict__ frame_err, double* __restrict__ out) {
    __shared__ double red[NT];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (p >= n_pairs) return;
    double m = -DBL_MAX;
    for (int f = pair_start[p] + tid; f < pair_start[p + 1]; f += NT) m = frame_err[f] > m ? frame_err[f] : m;
    m = block_reduce(m, red, OpMax());
    if (tid == 0) out[p] = m;
}

}  // namespace

void launch_mel_power(const float* wave, int n_clips, int total_frames, const Tables* t, const ClipWork& w, hipStream_t s) {
    hipLaunchKernelGGL(mel_power_kernel, dim3(total_frames), dim3(NT), 0, s, wave, n_clips, total_frames, t, w);
}

void launch_onset_pick(int n_clips, const PeakPick& pp, const ClipWork& w, hipStream_t s) {
    hipLaunchKernelGGL(onset_pick_kernel, dim3(n_clips), dim3(NT), 0, s, n_clips, pp, w);
}

void launch_coeff_rates(const float* coeffs, int n_seq, int channels, double threshold, const SeqWork& w, hipStream_t s) {
    hipLaunchKernelGGL(coeff_mean_diff_kernel, dim3(n_seq), dim3(NT), 0, s, coeffs, n_seq, channels, w);
    hipLaunchKernelGGL(coeff_mac_kernel, dim3(1), dim3(NT), 0, s, n_seq, channels, w);
    hipLaunchKernelGGL(coeff_rate_kernel, dim3(n_seq), dim3(NT), 0, s, coeffs, n_seq, channels, threshold, w);
}

void launch_beat_score(int n_seq, const int* clip_index, const ClipWork& cw, const SeqWork& sw, double sampling_rate, double fps, double sigma,
                       double* scores, hipStream_t s) {
    hipLaunchKernelGGL(beat_score_kernel, dim3(n_seq), dim3(NT), 0, s, n_seq, clip_index, cw, sw, sampling_rate, fps, sigma, scores);
}

void launch_vertex_error(const float* coeffs, int n_pairs, int total_blocks, const int* block_start, const int* pair_start, const long long* real_off,
                         const long long* eval_off, const int* person, const double* deltas, int channels, int n3v, double* frame_err, double* out, hipStream_t s) {
    hipLaunchKernelGGL(vertex_frame_kernel, dim3(total_blocks), dim3(NT), 0, s, coeffs, n_pairs, total_blocks, block_start, pair_start, real_off, eval_off, person,
                       deltas, channels, n3v, frame_err);
    hipLaunchKernelGGL(vertex_max_kernel, dim3(n_pairs), dim3(NT), 0, s, n_pairs, pair_start, frame_err, out);
}

}  // namespace beat
}  // namespace said
