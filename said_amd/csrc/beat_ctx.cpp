// beat_ctx.cpp — host side of the beat-consistency and vertex-error passes (C ABI: include/said_beat.h; kernels: beat.hip; DESIGN.md section
// 12.1): the context, the float64 tables of a sampling rate (window, twiddles, Slaney mel bank, peak-pick windows), the checks of every
// offset table before a kernel indexes with it, and the launches.
#include "engine_internal.h"
#include "beat_kernels.h"
#include "../../include/said_beat.h"

#include <cmath>

using namespace said::beat;

struct said_beat {
    HostCtx c;
    int sampling_rate = 0;
    PeakPick pp{};
    Tables* tables = nullptr;   // device
    // the last said_beat_clips
    int n_clips = 0, total_frames = 0;
    size_t cap_clips = 0, cap_frames = 0;
    int* frame_start = nullptr;
    long long* clip_off = nullptr;
    ClipWork cw{};
    // the last said_beat_coeffs
    int n_seq = 0, channels = 0;
    long long total_rows = 0;
    size_t cap_seq = 0, cap_rows = 0, cap_mean = 0;
    long long* seq_off = nullptr;
    SeqWork sw{};
    int* clip_index = nullptr;
    double* scores = nullptr;
    // vertex error
    double* deltas = nullptr;
    int n_person = 0, delta_channels = 0, n3v = 0;
    size_t cap_pairs = 0, cap_pair_frames = 0;
    int *pair_start = nullptr, *pair_blocks = nullptr, *pair_person = nullptr;
    long long *pair_real = nullptr, *pair_eval = nullptr;
    double *frame_err = nullptr, *pair_out = nullptr;
};

namespace {

template <typename T>
int grow(HostCtx* ctx, T** p, size_t n) { return drealloc(ctx, p, n, false); }

// Slaney's mel scale (htk = False): 200 / 3 Hz per mel below 1000 Hz, logarithmic above with 27 mels per factor 6.4
const double F_SP = 200.0 / 3.0, MIN_LOG_HZ = 1000.0, MIN_LOG_MEL = MIN_LOG_HZ / F_SP;
double logstep() { return std::log(6.4) / 27.0; }
double hz_to_mel(double f) { return f >= MIN_LOG_HZ ? MIN_LOG_MEL + std::log(f / MIN_LOG_HZ) / logstep() : f / F_SP; }
double mel_to_hz(double m) { return m >= MIN_LOG_MEL ? MIN_LOG_HZ * std::exp(logstep() * (m - MIN_LOG_MEL)) : F_SP * m; }

// numpy's linspace: start + i * ((stop - start) / (n - 1)), the last point set to stop
std::vector<double> linspace(double start, double stop, int n) {
    std::vector<double> v((size_t)n);
    const double step = (stop - start) / (double)(n - 1);
    for (int i = 0; i < n; ++i) v[(size_t)i] = start + (double)i * step;
    v[(size_t)n - 1] = stop;
    return v;
}

// false when the bank has more non-zero weights than Tables holds (cannot happen: a bin lies under at most two triangles)
bool make_tables(int sr, Tables* t) {
    const double pi = 3.14159265358979323846;
    for (int n = 0; n < N_FFT; ++n) t->window[n] = 0.5 - 0.5 * std::cos(2.0 * pi * (double)n / (double)N_FFT);
    for (int k = 0; k < HALF / 2; ++k) {
        t->tw_re[k] = std::cos(2.0 * pi * (double)k / (double)HALF);
        t->tw_im[k] = -std::sin(2.0 * pi * (double)k / (double)HALF);
    }
    for (int k = 0; k < N_BINS; ++k) {
        t->sp_re[k] = std::cos(2.0 * pi * (double)k / (double)N_FFT);
        t->sp_im[k] = -std::sin(2.0 * pi * (double)k / (double)N_FFT);
    }
    const double nyquist = (double)sr / 2.0;
    const std::vector<double> freqs = linspace(0.0, nyquist, N_BINS);
    std::vector<double> pts = linspace(hz_to_mel(0.0), hz_to_mel(nyquist), N_MELS + 2);
    for (double& m : pts) m = mel_to_hz(m);
    int used = 0;
    std::vector<double> row((size_t)N_BINS);
    for (int i = 0; i < N_MELS; ++i) {
        const double lo = pts[(size_t)i], mid = pts[(size_t)i + 1], hi = pts[(size_t)i + 2], norm = 2.0 / (hi - lo);
        int first = N_BINS, last = 0;
        for (int b = 0; b < N_BINS; ++b) {
            const double f = freqs[(size_t)b], w = std::max(0.0, std::min((f - lo) / (mid - lo), (hi - f) / (hi - mid)));
            row[(size_t)b] = w * norm;
            if (w > 0.0) {
                first = std::min(first, b);
                last = b + 1;
            }
        }
        if (last <= first) first = last = 0;
        if (used + (last - first) > MAX_WEIGHTS) return false;
        t->mel_first[i] = first;
        t->mel_last[i] = last;
        t->mel_woff[i] = used;
        for (int b = first; b < last; ++b) t->weights[used++] = row[(size_t)b];
    }
    for (int i = used; i < MAX_WEIGHTS; ++i) t->weights[i] = 0.0;
    return true;
}

// librosa's defaults in frames: int(seconds * sr // hop), with Python's float floor division (CPython's float_floor_div for positive
// operands): the quotient of the operand less its remainder, floored, and rounded up where that quotient lies within a half of the next integer
int frames_of(double seconds, int sr) {
    const double vx = seconds * (double)sr, wx = (double)HOP;
    const double div = (vx - std::fmod(vx, wx)) / wx;
    if (div == 0.0) return 0;
    double fl = std::floor(div);
    if (div - fl > 0.5) fl += 1.0;
    return (int)fl;
}

}  // namespace

extern "C" {

int said_beat_create(said_beat** out, int device) {
    DeviceRestore restore_device;
    said_beat* b = new_ctx("said_beat_create", out, device);
    if (!b) return -1;
    *out = b;
    return 0;
}

int said_beat_destroy(said_beat* b) { return delete_ctx(b); }

const char* said_beat_last_error(const said_beat* b) { return ctx_error(b); }

int said_beat_set_sampling_rate(said_beat* b, int sampling_rate, int* pick_host) {
    if (!b) return -1;
    HostCtx* ctx = &b->c;
    if (sampling_rate < 1) return fail(ctx, "said_beat_set_sampling_rate: sampling rate %d (at least 1)", sampling_rate);
    b->sampling_rate = 0;   // a refused rate leaves none
    b->n_clips = 0;
    std::vector<Tables> t(1);
    if (!make_tables(sampling_rate, t.data())) return fail(ctx, "said_beat_set_sampling_rate: the mel bank of %d Hz has more than %d weights", sampling_rate, (int)MAX_WEIGHTS);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    if (!b->tables && dalloc(ctx, &b->tables, 1, false)) return -1;
    HIPCHK(hipMemcpy(b->tables, t.data(), sizeof(Tables), hipMemcpyHostToDevice));
    PeakPick pp{};
    pp.pre_max = frames_of(0.03, sampling_rate);
    pp.post_max = frames_of(0.00, sampling_rate) + 1;
    pp.pre_avg = frames_of(0.10, sampling_rate);
    pp.post_avg = frames_of(0.10, sampling_rate) + 1;
    pp.wait = frames_of(0.03, sampling_rate);
    pp.delta = 0.07;
    b->pp = pp;
    b->sampling_rate = sampling_rate;
    if (pick_host) {
        const int v[5] = {pp.pre_max, pp.post_max, pp.pre_avg, pp.post_avg, pp.wait};
        std::memcpy(pick_host, v, sizeof(v));
    }
    return 0;
}

int said_beat_clips(said_beat* b, const float* wave_dev, int n_clips, const long long* offsets_host, void* stream) {
    if (!b) return -1;
    HostCtx* ctx = &b->c;
    b->n_clips = 0;
    if (!b->sampling_rate) return fail(ctx, "said_beat_clips: no sampling rate (said_beat_set_sampling_rate)");
    if (!wave_dev || !offsets_host || n_clips < 1) return fail(ctx, "said_beat_clips: null waveforms or offsets, or n_clips %d below 1", n_clips);
    if (offsets_host[0] != 0) return fail(ctx, "said_beat_clips: offsets start at %lld, not 0", offsets_host[0]);
    std::vector<int> start((size_t)n_clips + 1, 0);
    for (int i = 0; i < n_clips; ++i) {
        const long long len = offsets_host[i + 1] - offsets_host[i];
        if (len < 1) return fail(ctx, "said_beat_clips: clip %d has %lld samples (at least 1)", i, len);
        const long long frames = (long long)start[(size_t)i] + 1 + len / HOP;
        if (frames > SAID_BEAT_MAX_FRAMES) return fail(ctx, "said_beat_clips: more than %d frames in one call", (int)SAID_BEAT_MAX_FRAMES);
        start[(size_t)i + 1] = (int)frames;
    }
    const int total = start[(size_t)n_clips];
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    if ((size_t)n_clips > b->cap_clips) {
        b->cap_clips = 0;
        if (grow(ctx, &b->frame_start, (size_t)n_clips + 1) || grow(ctx, &b->clip_off, (size_t)n_clips + 1) || grow(ctx, &b->cw.onset_count, (size_t)n_clips)) return -1;
        b->cap_clips = (size_t)n_clips;
    }
    if ((size_t)total > b->cap_frames) {
        b->cap_frames = 0;
        const size_t n = (size_t)total;
        if (grow(ctx, &b->cw.mel, n * N_MELS) || grow(ctx, &b->cw.db, n * N_MELS) || grow(ctx, &b->cw.env, n) || grow(ctx, &b->cw.xn, n) || grow(ctx, &b->cw.flag, n) ||
            grow(ctx, &b->cw.onsets, n))
            return -1;
        b->cap_frames = n;
    }
    b->cw.frame_start = b->frame_start;
    b->cw.clip_off = b->clip_off;
    HIPCHK(hipMemcpy(b->frame_start, start.data(), sizeof(int) * start.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->clip_off, offsets_host, sizeof(long long) * ((size_t)n_clips + 1), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(b->cw.onsets, 0, sizeof(int) * (size_t)total, s));
    launch_mel_power(wave_dev, n_clips, total, b->tables, b->cw, s);
    HIPCHK(hipGetLastError());
    launch_onset_pick(n_clips, b->pp, b->cw, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    b->n_clips = n_clips;
    b->total_frames = total;
    return 0;
}

int said_beat_coeffs(said_beat* b, const float* coeffs_dev, int n_seq, const long long* offsets_host, int channels, double threshold, void* stream) {
    if (!b) return -1;
    HostCtx* ctx = &b->c;
    b->n_seq = 0;
    if (!coeffs_dev || !offsets_host || n_seq < 1) return fail(ctx, "said_beat_coeffs: null coefficients or offsets, or n_seq %d below 1", n_seq);
    if (channels < 1 || channels > SAID_BEAT_MAX_CHANNELS) return fail(ctx, "said_beat_coeffs: %d channels (1 .. %d)", channels, (int)SAID_BEAT_MAX_CHANNELS);
    if (offsets_host[0] != 0) return fail(ctx, "said_beat_coeffs: offsets start at %lld, not 0", offsets_host[0]);
    for (int i = 0; i < n_seq; ++i) {
        const long long T = offsets_host[i + 1] - offsets_host[i];
        if (T < 2 || T > (1LL << 30)) return fail(ctx, "said_beat_coeffs: sequence %d has %lld frames (at least 2)", i, T);
    }
    const long long rows = offsets_host[n_seq];
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    if ((size_t)n_seq > b->cap_seq) {
        b->cap_seq = 0;
        if (grow(ctx, &b->seq_off, (size_t)n_seq + 1) || grow(ctx, &b->sw.min_count, (size_t)n_seq) || grow(ctx, &b->clip_index, (size_t)n_seq) || grow(ctx, &b->scores, (size_t)n_seq))
            return -1;
        b->cap_seq = (size_t)n_seq;
    }
    if ((size_t)rows > b->cap_rows) {
        b->cap_rows = 0;
        if (grow(ctx, &b->sw.rates, (size_t)rows) || grow(ctx, &b->sw.minima, (size_t)rows)) return -1;
        b->cap_rows = (size_t)rows;
    }
    if ((size_t)n_seq * channels > b->cap_mean) {
        b->cap_mean = 0;
        if (grow(ctx, &b->sw.seq_mean, (size_t)n_seq * channels)) return -1;
        b->cap_mean = (size_t)n_seq * channels;
    }
    if (!b->sw.mac && dalloc(ctx, &b->sw.mac, (size_t)SAID_BEAT_MAX_CHANNELS, false)) return -1;
    b->sw.seq_off = b->seq_off;
    HIPCHK(hipMemcpy(b->seq_off, offsets_host, sizeof(long long) * ((size_t)n_seq + 1), hipMemcpyHostToDevice));
    launch_coeff_rates(coeffs_dev, n_seq, channels, threshold, b->sw, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    b->n_seq = n_seq;
    b->channels = channels;
    b->total_rows = rows;
    return 0;
}

int said_beat_score(said_beat* b, const int* clip_index_host, double fps, double sigma, double* scores_host, void* stream) {
    if (!b) return -1;
    HostCtx* ctx = &b->c;
    if (!b->n_clips || !b->n_seq) return fail(ctx, "said_beat_score: needs the clips and the coefficients first (said_beat_clips, said_beat_coeffs)");
    if (!clip_index_host || !scores_host) return fail(ctx, "said_beat_score: null clip indices or scores");
    for (int i = 0; i < b->n_seq; ++i)
        if (clip_index_host[i] < 0 || clip_index_host[i] >= b->n_clips)
            return fail(ctx, "said_beat_score: sequence %d names clip %d of %d", i, clip_index_host[i], b->n_clips);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(b->clip_index, clip_index_host, sizeof(int) * (size_t)b->n_seq, hipMemcpyHostToDevice));
    launch_beat_score(b->n_seq, b->clip_index, b->cw, b->sw, (double)b->sampling_rate, fps, sigma, b->scores, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(scores_host, b->scores, sizeof(double) * (size_t)b->n_seq, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int said_beat_set_deltas(said_beat* b, int n_person, int channels, int n3v, const double* deltas_host, void* stream) {
    if (!b) return -1;
    HostCtx* ctx = &b->c;
    b->n_person = 0;
    if (!deltas_host || n_person < 1 || n3v < 1 || channels < 1 || channels > SAID_BEAT_MAX_CHANNELS)
        return fail(ctx, "said_beat_set_deltas: null deltas, or %d persons, %d channels (1 .. %d), %d columns", n_person, channels, (int)SAID_BEAT_MAX_CHANNELS, n3v);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    const size_t n = (size_t)n_person * channels * n3v;
    if (grow(ctx, &b->deltas, n)) return -1;
    HIPCHK(hipMemcpy(b->deltas, deltas_host, sizeof(double) * n, hipMemcpyHostToDevice));
    b->n_person = n_person;
    b->delta_channels = channels;
    b->n3v = n3v;
    return 0;
}

int said_beat_vertex_error(said_beat* b, const float* coeffs_dev, long long total_frames, int n_pairs, const long long* real_off_host,
                           const long long* eval_off_host, const int* length_host, const int* person_host, double* out_host, void* stream) {
    if (!b) return -1;
    HostCtx* ctx = &b->c;
    if (!b->n_person) return fail(ctx, "said_beat_vertex_error: no blendshape deltas (said_beat_set_deltas)");
    if (!coeffs_dev || !real_off_host || !eval_off_host || !length_host || !person_host || !out_host || n_pairs < 1)
        return fail(ctx, "said_beat_vertex_error: a null argument, or n_pairs %d below 1", n_pairs);
    std::vector<int> start((size_t)n_pairs + 1, 0), blocks((size_t)n_pairs + 1, 0);
    for (int p = 0; p < n_pairs; ++p) {
        const long long L = length_host[p];
        if (L < 1 || real_off_host[p] < 0 || eval_off_host[p] < 0 || real_off_host[p] + L > total_frames || eval_off_host[p] + L > total_frames)
            return fail(ctx, "said_beat_vertex_error: pair %d compares %lld frames at %lld and %lld of %lld", p, L, real_off_host[p], eval_off_host[p], total_frames);
        if (person_host[p] < 0 || person_host[p] >= b->n_person) return fail(ctx, "said_beat_vertex_error: pair %d names person %d of %d", p, person_host[p], b->n_person);
        const long long sum = (long long)start[(size_t)p] + L;
        if (sum > (1LL << 30)) return fail(ctx, "said_beat_vertex_error: more than 2^30 compared frames in one call");
        start[(size_t)p + 1] = (int)sum;
        blocks[(size_t)p + 1] = blocks[(size_t)p] + (int)((L + VERTEX_FRAME_BLOCK - 1) / VERTEX_FRAME_BLOCK);
    }
    const int total = start[(size_t)n_pairs];
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    if ((size_t)n_pairs > b->cap_pairs) {
        b->cap_pairs = 0;
        const size_t n = (size_t)n_pairs;
        if (grow(ctx, &b->pair_start, n + 1) || grow(ctx, &b->pair_blocks, n + 1) || grow(ctx, &b->pair_person, n) || grow(ctx, &b->pair_real, n) || grow(ctx, &b->pair_eval, n) || grow(ctx, &b->pair_out, n)) return -1;
        b->cap_pairs = n;
    }
    if ((size_t)total > b->cap_pair_frames) {
        b->cap_pair_frames = 0;
        if (grow(ctx, &b->frame_err, (size_t)total)) return -1;
        b->cap_pair_frames = (size_t)total;
    }
    HIPCHK(hipMemcpy(b->pair_start, start.data(), sizeof(int) * start.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->pair_blocks, blocks.data(), sizeof(int) * blocks.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->pair_person, person_host, sizeof(int) * (size_t)n_pairs, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->pair_real, real_off_host, sizeof(long long) * (size_t)n_pairs, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->pair_eval, eval_off_host, sizeof(long long) * (size_t)n_pairs, hipMemcpyHostToDevice));
    launch_vertex_error(coeffs_dev, n_pairs, blocks[(size_t)n_pairs], b->pair_blocks, b->pair_start, b->pair_real, b->pair_eval, b->pair_person, b->deltas, b->delta_channels, b->n3v, b->frame_err,
                        b->pair_out, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_host, b->pair_out, sizeof(double) * (size_t)n_pairs, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

#define BEAT_READ(what, need, src, count, T)                                                                        \
    if (!b) return -1;                                                                                              \
    HostCtx* ctx = &b->c;                                                                                           \
    if (!(need) || !out_host) return fail(ctx, "%s: nothing to read, or a null buffer", what);                      \
    hipStream_t s = (hipStream_t)stream;                                                                            \
    HIPCHK(hipSetDevice(ctx->device));                                                                              \
    HIPCHK(hipMemcpyAsync(out_host, src, sizeof(T) * (size_t)(count), hipMemcpyDeviceToHost, s));

int said_beat_read_mel(said_beat* b, double* out_host, void* stream) {
    BEAT_READ("said_beat_read_mel", b->n_clips, b->cw.mel, (size_t)b->total_frames * N_MELS, double)
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int said_beat_read_envelope(said_beat* b, double* out_host, void* stream) {
    BEAT_READ("said_beat_read_envelope", b->n_clips, b->cw.env, b->total_frames, double)
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int said_beat_read_onsets(said_beat* b, int* count_host, int* frames_host, void* stream) {
    int* out_host = frames_host;
    BEAT_READ("said_beat_read_onsets", b->n_clips && count_host, b->cw.onsets, b->total_frames, int)
    HIPCHK(hipMemcpyAsync(count_host, b->cw.onset_count, sizeof(int) * (size_t)b->n_clips, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int said_beat_read_rates(said_beat* b, double* out_host, void* stream) {
    BEAT_READ("said_beat_read_rates", b->n_seq, b->sw.rates, b->total_rows, double)
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int said_beat_read_minima(said_beat* b, int* count_host, int* index_host, void* stream) {
    int* out_host = index_host;
    BEAT_READ("said_beat_read_minima", b->n_seq && count_host, b->sw.minima, b->total_rows, int)
    HIPCHK(hipMemcpyAsync(count_host, b->sw.min_count, sizeof(int) * (size_t)b->n_seq, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
