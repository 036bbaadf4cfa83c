// beat_kernels.h — launchers of beat.hip for beat_ctx.cpp.
#pragma once
#include <hip/hip_runtime.h>

namespace said {
namespace beat __attribute__((visibility("hidden"))) {

constexpr int N_FFT = 2048, HOP = 512, N_MELS = 128, N_BINS = N_FFT / 2 + 1;
constexpr int HALF = N_FFT / 2;          // points of the complex transform a real frame is packed into
constexpr int MAX_WEIGHTS = 2304;        // non-zero mel weights: a bin lies under at most two triangles (2 x 1025, rounded up)

struct Tables {                           // one device copy per sampling rate; all float64, formed on the host
    double window[N_FFT];                 // periodic Hann
    double tw_re[HALF / 2], tw_im[HALF / 2];   // exp(-2 pi i k / 1024), k < 512: the complex transform's twiddles
    double sp_re[N_BINS], sp_im[N_BINS];       // exp(-2 pi i k / 2048), k <= 1024: the real-transform split
    int mel_first[N_MELS], mel_last[N_MELS];   // bins [first, last) with a non-zero weight
    int mel_woff[N_MELS];                 // where the band's weights start in `weights`
    double weights[MAX_WEIGHTS];
};

struct PeakPick {
    int pre_max, post_max, pre_avg, post_avg, wait;
    double delta;
};

struct ClipWork {                         // per frame of all clips, frames numbered consecutively
    const int* frame_start;               // (n_clips + 1)
    const long long* clip_off;            // (n_clips + 1) sample offsets
    double* mel;                          // (frames, 128)
    double* db;                           // (frames, 128)
    double* env;                          // (frames)
    double* xn;                           // (frames) the normalised envelope
    int* flag;                            // (frames) both window tests hold
    int* onsets;                          // (frames) a clip's onset frames, at its first frame number
    int* onset_count;                     // (n_clips)
};

struct SeqWork {                          // per frame of all sequences
    const long long* seq_off;             // (n_seq + 1) frame offsets
    double* seq_mean;                     // (n_seq, channels) mean over t of |difference|
    double* mac;                          // (channels)
    double* rates;                        // (frames)
    int* minima;                          // (frames) a sequence's minima, at its frame offset
    int* min_count;                       // (n_seq)
};

void launch_mel_power(const float* wave, int n_clips, int total_frames, const Tables* t, const ClipWork& w, hipStream_t s);
void launch_onset_pick(int n_clips, const PeakPick& pp, const ClipWork& w, hipStream_t s);
void launch_coeff_rates(const float* coeffs, int n_seq, int channels, double threshold, const SeqWork& w, hipStream_t s);
void launch_beat_score(int n_seq, const int* clip_index, const ClipWork& cw, const SeqWork& sw, double sampling_rate, double fps, double sigma,
                       double* scores, hipStream_t s);
constexpr int VERTEX_FRAME_BLOCK = 16;   // frames of a pair per workgroup of the vertex error: block_start counts ceil(length / 16) per pair
void launch_vertex_error(const float* coeffs, int n_pairs, int total_blocks, const int* block_start, const int* pair_start, const long long* real_off,
                         const long long* eval_off, const int* person, const double* deltas, int channels, int n3v, double* frame_err, double* out, hipStream_t s);

}  // namespace beat
}  // namespace said
