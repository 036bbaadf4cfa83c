"""A float64 restatement of DESIGN.md section 12.1 (beat consistency and vertex error, said_amd/csrc/beat.hip) in numpy: librosa's default
onset detection step by step (np.fft.rfft, plain loops for the peak pick), the kinematic beats with scipy.signal.find_peaks, the score and
the vertex error.  Every decision that compares two floats also reports its margin, so that a test can demand bit-equal indices from the
device only on inputs where no decision is closer than rounding could move it.  Shared by tests/test_beat_cpu.py, tests/test_gpu_beat.py
and scripts/bench_beat.py; nothing here imports said_amd."""
import math
import statistics
import sys
import warnings

import numpy as np
from scipy.signal import find_peaks, get_window

N_FFT, HOP, N_MELS, DELTA = 2048, 512, 128, 0.07
DBL_MIN = sys.float_info.min


# ---------------------------------------------------------------- audio beats
def hz_to_mel(f):
    """Slaney's scale (htk=False): 200 / 3 Hz per mel below 1000 Hz, 27 mels per factor 6.4 above."""
    f = float(f)
    return 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0) if f >= 1000.0 else f / (200.0 / 3.0)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((math.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_points(sr):
    return mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), N_MELS + 2))


def mel_bank(sr):
    """(128, 1025) float64: Slaney-normalised triangles at the bins of a 2048-point transform."""
    m, f = mel_points(sr), np.linspace(0.0, sr / 2.0, N_FFT // 2 + 1)
    bank = np.zeros((N_MELS, f.shape[0]))
    for i in range(N_MELS):
        tri = np.maximum(0.0, np.minimum((f - m[i]) / (m[i + 1] - m[i]), (m[i + 2] - f) / (m[i + 2] - m[i + 1])))
        bank[i] = tri * (2.0 / (m[i + 2] - m[i]))
    return bank


def n_frames(n_samples):
    return 1 + n_samples // HOP


def power_spectrum(y):
    """(frames, 1025): |rfft|^2 of the centred, zero-padded, Hann-windowed frames."""
    y = np.asarray(y, dtype=np.float64)
    ypad = np.concatenate([np.zeros(N_FFT // 2), y, np.zeros(N_FFT // 2)])
    win = get_window("hann", N_FFT, fftbins=True)
    frames = np.stack([ypad[HOP * t:HOP * t + N_FFT] * win for t in range(n_frames(y.shape[0]))])
    return np.abs(np.fft.rfft(frames, axis=1)) ** 2


def mel_power(y, sr):
    return power_spectrum(y) @ mel_bank(sr).T


def envelope(melp):
    """(frames,) spectral flux of the dB mel spectrogram (80 dB under the clip's maximum at most), three zeros first."""
    db = 10.0 * np.log10(np.maximum(1e-10, melp))
    db = np.maximum(db, db.max() - 80.0)
    flux = np.maximum(0.0, db[1:] - db[:-1]).mean(axis=1)
    return np.concatenate([np.zeros(3), flux])[:melp.shape[0]]


def peak_params(sr):
    """(pre_max, post_max, pre_avg, post_avg, wait) in frames: librosa's defaults."""
    return (int(0.03 * sr // HOP), int(0.00 * sr // HOP + 1), int(0.10 * sr // HOP), int(0.10 * sr // HOP + 1), int(0.03 * sr // HOP))


def peak_pick(env, sr):
    """(onset frames, decisions): a decision is (frame, x - (mean + delta), gap to another value of the max window or None)."""
    n = env.shape[0]
    if not np.any(env != 0):
        return np.zeros(0, dtype=np.int64), []
    x = env - env.min()
    x = x / (x.max() + DBL_MIN)
    pre_max, post_max, pre_avg, post_avg, wait = peak_params(sr)
    onsets, decisions, last = [], [], -math.inf
    for i in range(n):
        win = x[max(0, i - pre_max):min(n, i + post_max)]
        others = np.delete(win, i - max(0, i - pre_max))
        gap = None if others.shape[0] == 0 else float(x[i] - others.max())
        lo, hi = max(0, i - pre_avg), min(n, i + post_avg)
        total = 0.0
        for v in x[lo:hi]:
            total += v
        margin = float(x[i] - (total / (hi - lo) + DELTA))
        decisions.append((i, margin, gap))
        if x[i] == win.max() and margin >= 0 and i > last + wait:
            onsets.append(i)
            last = i
    return np.asarray(onsets, dtype=np.int64), decisions


def onset_margin(decisions):
    """The smallest |margin| among the decisions that can change a frame's flag: a test's margin counts unless the other test fails clearly."""
    worst = math.inf
    for _, margin, gap in decisions:
        if gap is None or gap > -1e-3:
            worst = min(worst, abs(margin))
        if gap is not None and margin > -1e-3 and gap != 0.0:
            worst = min(worst, abs(gap))
    return worst


def audio_beats(y, sr):
    """dict(mel, env, onsets, times, decisions) of one clip."""
    melp = mel_power(y, sr)
    env = envelope(melp)
    onsets, decisions = peak_pick(env, sr)
    return dict(mel=melp, env=env, onsets=onsets, times=onsets * HOP / float(sr), decisions=decisions)


# ---------------------------------------------------------------- kinematic beats
def change_rates(seqs):
    diffs = [np.abs(np.asarray(c, dtype=np.float64)[1:] - np.asarray(c, dtype=np.float64)[:-1]) for c in seqs]
    if any(d.shape[0] < 1 for d in diffs):
        raise ValueError("a coefficient sequence has fewer than 2 frames")
    mac = np.mean([d.mean(0) for d in diffs], axis=0, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return [np.mean(d / mac, axis=1) for d in diffs]


def minima(r, threshold):
    """(indices, margins): the reference's find_peaks(-r, threshold=0) filtered by left / right > threshold; margins are |threshold - side|
    of every candidate and the non-zero |differences| of neighbouring rates."""
    idx, props = find_peaks(-r, threshold=0)
    left, right = props["left_thresholds"], props["right_thresholds"]
    keep = np.logical_or(left > threshold, right > threshold)
    step = np.abs(np.diff(r))
    margins = [abs(threshold - v) for v in np.concatenate([left, right])] + [float(v) for v in step[(step > 0) & np.isfinite(step)]]
    return idx[keep].astype(np.int64), margins


def minima_loop(r, threshold):
    """The same indices by the plain rule of DESIGN.md 12.1: the middle (rounded down) of every run of equal values entered and left upwards."""
    out, n, i = [], len(r), 1
    while i < n - 1:
        if not r[i - 1] > r[i]:
            i += 1
            continue
        j = i
        while j + 1 < n and r[j + 1] == r[j]:
            j += 1
        if j + 1 < n and r[j + 1] > r[j]:
            p = (i + j) // 2
            if r[p - 1] - r[p] > threshold or r[p + 1] - r[p] > threshold:
                out.append(p)
        i = j + 1
    return np.asarray(out, dtype=np.int64)


def sequence_scores(audio_times, kin_times, sigma):
    out = []
    for a, k in zip(audio_times, kin_times):
        if len(k) == 0:
            out.append(0.0)
            continue
        with np.errstate(invalid="ignore"), warnings.catch_warnings():   # the mean of no audio beat is NaN, as in the reference
            warnings.simplefilter("ignore")
            out.append(float(np.mean(np.exp(-np.power(np.asarray(a)[:, None] - np.asarray(k)[None, :], 2).min(axis=1) / (2 * sigma ** 2)))))
    return np.asarray(out)


def beat_consistency(waves, seqs, clip_index, sr, fps, threshold, sigma=0.1):
    """dict(clips=[audio_beats], rates, minima, scores, score) for sequences seqs[s] against clip waves[clip_index[s]]."""
    clips = [audio_beats(w, sr) for w in waves]
    rates = change_rates(seqs)
    mins = [minima(r, threshold) for r in rates]
    scores = sequence_scores([clips[c]["times"] for c in clip_index], [m[0] / fps for m in mins], sigma)
    return dict(clips=clips, rates=rates, minima=[m[0] for m in mins], minima_margins=[m[1] for m in mins], scores=scores, score=float(np.mean(scores)))


# ---------------------------------------------------------------- vertex error
def vertex_error(real, gen, delta):
    """max over t < min length of |(real - gen)[t] @ delta|, delta (C, V, 3), float64."""
    n = min(real.shape[0], gen.shape[0])
    d = np.asarray(real[:n], dtype=np.float64) - np.asarray(gen[:n], dtype=np.float64)
    v = np.einsum("tc,cvi->tvi", d, np.asarray(delta, dtype=np.float64))
    return float(np.sqrt(np.sum(np.square(v), axis=(1, 2))).max())


def mean_vertex_error(pairs, deltas):
    return statistics.mean(vertex_error(r, g, deltas[p]) for r, g, p in pairs)


# ---------------------------------------------------------------- seeded fixtures
SEED = 7
LENGTHS_16K = (800, 2048, 2049, 8209, 24000)
SEQ_FRAMES = (2, 3, 4, 61, 64, 65, 127, 241)


def burst_clip(n, sr, rng):
    """Decaying tone bursts about every 0.2 s over a 0.003 noise floor, fp32."""
    t = np.arange(n) / sr
    y = 0.003 * rng.standard_normal(n)
    start = 0.02
    while start < n / sr:
        tt = t - start
        y += np.where(tt >= 0, rng.uniform(0.3, 0.8) * np.sin(2 * np.pi * rng.uniform(200.0, 3000.0) * tt) * np.exp(-np.maximum(tt, 0) / 0.03), 0.0)
        start += rng.uniform(0.15, 0.3)
    return y.astype(np.float32)


def clips_16k(seed=SEED):
    rng = np.random.default_rng(seed)
    return [burst_clip(n, 16000, rng) for n in LENGTHS_16K] + [np.zeros(4096, dtype=np.float32)]


def clip_44k(seed=SEED):
    return burst_clip(22050, 44100, np.random.default_rng(seed + 1))


def smooth_coeffs(frames, rng, channels=32):
    """Smoothed random coefficients clipped to [0, 1], fp32."""
    raw = rng.standard_normal((frames + 4, channels))
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    sm = sum(k[i] * raw[i:i + frames] for i in range(5))
    return np.clip(0.35 + 0.45 * sm, 0.0, 1.0).astype(np.float32)


def sequences(seed=SEED):
    """(sequences, clip of each): the frames of SEQ_FRAMES; the 65- and 127-frame ones hold rows copied over 3 and 4 frames (exact plateaus
    of the change rate); several sequences share a clip."""
    rng = np.random.default_rng(seed + 2)
    seqs = [smooth_coeffs(T, rng) for T in SEQ_FRAMES]
    seqs[5][20:23] = seqs[5][20]
    seqs[5][40:44] = seqs[5][40]
    seqs[6][70:74] = seqs[6][70]
    seqs[6][100:103] = seqs[6][100]
    return seqs, [0, 1, 2, 3, 4, 4, 3, 4]


def constant_channel_sequences(seed=SEED):
    """A group whose channel 5 never moves: mac = 0 there, every rate is NaN."""
    rng = np.random.default_rng(seed + 3)
    seqs = [smooth_coeffs(T, rng) for T in (30, 47)]
    for c in seqs:
        c[:, 5] = 0.25
    return seqs, [4, 3]


def vertex_case(n_vertices, seed=SEED):
    """(pairs [(real, generated, person)], deltas [(32, V, 3)] x 2): lengths differ, and one pair compares a single frame."""
    rng = np.random.default_rng(seed + 4 + n_vertices)
    deltas = [(0.01 * rng.standard_normal((32, n_vertices, 3))).astype(np.float32) for _ in range(2)]
    shapes = [(40, 37, 0), (1, 12, 1), (33, 33, 1), (20, 64, 0), (300, 290, 1)]
    return [(smooth_coeffs(a, rng), smooth_coeffs(b, rng), p) for a, b, p in shapes], deltas
