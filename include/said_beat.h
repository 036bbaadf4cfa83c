/*
 * said_beat.h — C ABI of the beat-consistency and vertex-error passes (said_amd/csrc/beat.hip, beat_ctx.cpp), in libsaid_hip.so beside
 * said_metrics.h.
 *
 * DESIGN.md section 12.1 is the specification.  The audio side restates librosa.onset.onset_detect with its defaults: a centred, zero-padded
 * STFT (n_fft 2048, hop 512, periodic Hann), the power spectrum, 128 Slaney mel bands, dB with an 80 dB floor, the spectral-flux onset
 * envelope and librosa's peak pick.  The kinematic side is said/metric/beat_consistency.py: the coefficients' change rate, its local minima by
 * scipy's find_peaks rule, and the score.  The vertex error is the reference's evaluate_vertex_error.
 *
 * Everything is computed in float64, every sum has a fixed order and no kernel uses atomics: equal inputs give bit-identical outputs.  The
 * window, the twiddle factors and the mel bank are float64 tables formed on the host.
 *
 * Conventions are those of said_metrics.h: 0 on success, said_beat_last_error(ctx) (NULL for create failures) gives the message; `*_dev` are
 * device pointers, `*_host` host memory; `stream` is a hipStream_t.  Nothing aborts.  Every call but create / destroy / last_error
 * synchronises `stream` before it returns.
 */
#ifndef SAID_BEAT_H
#define SAID_BEAT_H

#ifdef __cplusplus
extern "C" {
#endif

enum { SAID_BEAT_N_FFT = 2048, SAID_BEAT_HOP = 512, SAID_BEAT_N_MELS = 128, SAID_BEAT_MAX_CHANNELS = 256, SAID_BEAT_MAX_FRAMES = 1 << 20 };

typedef struct said_beat said_beat;
int said_beat_create(said_beat** out, int device);
int said_beat_destroy(said_beat* b);
const char* said_beat_last_error(const said_beat* b);

/* The sampling rate of the clips that follow: forms the mel bank (128 Slaney bands from 0 to rate / 2) and librosa's peak-pick windows
 * (pre_max, post_max, pre_avg, post_avg, wait: pick_host[5] receives them when it is not NULL).  Fails when rate < 1. */
int said_beat_set_sampling_rate(said_beat* b, int sampling_rate, int* pick_host);

/* n_clips waveforms, concatenated fp32 on the device; offsets_host has n_clips + 1 sample offsets (clip i is wave_dev[offsets[i] ..
 * offsets[i + 1]), at least one sample each).  Clip i has 1 + length / 512 frames; the frames of all clips are numbered consecutively.
 * Computes the mel power of every frame, and per clip its onset envelope and onset frames.  wave_dev is not used after the call. */
int said_beat_clips(said_beat* b, const float* wave_dev, int n_clips, const long long* offsets_host, void* stream);

/* n_seq coefficient sequences, concatenated as (frames, channels) fp32 on the device; offsets_host has n_seq + 1 frame offsets, at least two
 * frames each.  Computes the change rates r_s (frames - 1 per sequence, stored at the sequence's frame offset) and their local minima
 * under `threshold`.  coeffs_dev is not used after the call. */
int said_beat_coeffs(said_beat* b, const float* coeffs_dev, int n_seq, const long long* offsets_host, int channels, double threshold, void* stream);

/* The score of every sequence of the last said_beat_coeffs against the onsets of clip clip_index_host[s] of the last said_beat_clips:
 * scores_host receives n_seq float64 values (0 without a kinematic beat, NaN without an audio beat); their mean is the beat consistency. */
int said_beat_score(said_beat* b, const int* clip_index_host, double fps, double sigma, double* scores_host, void* stream);

/* Blendshape deltas of n_person persons, (n_person, channels, n3v) float64 on the host (n3v = 3 x vertices): uploaded once. */
int said_beat_set_deltas(said_beat* b, int n_person, int channels, int n3v, const double* deltas_host, void* stream);

/* n_pairs (real, generated) pairs out of coeffs_dev, (frames, channels) fp32 on the device with total_frames rows: pair p compares rows
 * real_off_host[p] + t and eval_off_host[p] + t for t < length_host[p] (>= 1) under the deltas of person_host[p].  out_host receives per
 * pair the maximum over t of the Euclidean norm of the vertex difference. */
int said_beat_vertex_error(said_beat* b, const float* coeffs_dev, long long total_frames, int n_pairs, const long long* real_off_host,
                           const long long* eval_off_host, const int* length_host, const int* person_host, double* out_host, void* stream);

/* What the last said_beat_clips left, for tests: the mel power (frames, 128) and the onset envelope (frames) of all clips' frames; per clip
 * the number of onsets (count_host[n_clips]) and, at the clip's first frame number, that many ascending frame indices (frames_host[frames]). */
int said_beat_read_mel(said_beat* b, double* out_host, void* stream);
int said_beat_read_envelope(said_beat* b, double* out_host, void* stream);
int said_beat_read_onsets(said_beat* b, int* count_host, int* frames_host, void* stream);
/* What the last said_beat_coeffs left: the change rates (one per frame of the input; the last of each sequence is unused), per sequence the
 * number of minima (count_host[n_seq]) and, at the sequence's frame offset, that many ascending indices (index_host[frames]). */
int said_beat_read_rates(said_beat* b, double* out_host, void* stream);
int said_beat_read_minima(said_beat* b, int* count_host, int* index_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAID_BEAT_H */
