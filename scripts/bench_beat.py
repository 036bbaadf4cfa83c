"""Device time of beat consistency and vertex error at the BlendVOCA test set's shape: 80 clips of 4 s at 16 kHz,
5760 coefficient sequences of 240 x 32 (72 repeats of each sentence), and for the vertex error each of them against its sentence's real
sequence under the ARKit head's vertex count and two persons' deltas.

Per pass (the audio pass: mel power and onsets of all clips; the kinematic and score pass; the vertex error): one warm-up, then the median
of `--repeats` calls, each timed by a host clock between two device synchronisations, with the inputs already on the device.  Beside them
the same work in tests/beat_ref.py (numpy, float64) on `--host-procs` host processes; `--host-sequences` bounds how many sequences the host
does (its time is scaled to all of them and both figures are reported).  Prints one JSON line.

Usage:  python scripts/bench_beat.py [--repeats 5] [--host-procs 16] [--host-sequences 576] [--no-host]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beat_ref as br  # noqa: E402

SR, FPS, THRESHOLD, SIGMA = 16000, 60, 0.1, 0.1
N_CLIPS, CLIP_SAMPLES, REPEATS_PER_CLIP, FRAMES = 80, 4 * 16000, 72, 240


def workload(seed=0):
    rng = np.random.default_rng(seed)
    waves = [br.burst_clip(CLIP_SAMPLES, SR, rng) for _ in range(N_CLIPS)]
    n_seq = N_CLIPS * REPEATS_PER_CLIP
    coeffs = np.stack([br.smooth_coeffs(FRAMES, rng) for _ in range(64)])   # 64 distinct sequences, cycled: the kernels' time does not depend on values
    coeffs = coeffs[np.arange(n_seq) % 64].reshape(n_seq * FRAMES, 32)
    real = np.stack([br.smooth_coeffs(FRAMES, rng) for _ in range(N_CLIPS)]).reshape(N_CLIPS * FRAMES, 32)
    clip_index = np.repeat(np.arange(N_CLIPS), REPEATS_PER_CLIP).astype(np.int32)
    return waves, coeffs, real, clip_index


def n_vertices():
    return int(np.load(os.path.join(ROOT, "tests", "golden", "g13_blendshape_qp.npz"))["neutral"].shape[0])


def median_ms(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), ts


def _host_clip(y):
    return br.audio_beats(y, SR)["times"]


def _host_vertex(args):
    real, gens, delta = args
    return [br.vertex_error(real, g, delta) for g in gens]


def host_times(waves, coeffs, real, clip_index, deltas, procs, n_host):
    """Seconds of the restatement on `procs` processes: (audio pass, kinematic + score pass over n_host sequences, vertex error over n_host)."""
    seqs = [coeffs[s * FRAMES:(s + 1) * FRAMES] for s in range(n_host)]
    with ProcessPoolExecutor(procs) as ex:
        list(ex.map(_host_clip, waves[:procs]))   # start the workers
        t = time.perf_counter()
        times = list(ex.map(_host_clip, waves, chunksize=max(1, len(waves) // procs)))
        t_audio = time.perf_counter() - t
        t = time.perf_counter()
        rates = br.change_rates(seqs)   # mac couples all sequences: one process, as the reference runs it
        mins = [br.minima(r, THRESHOLD)[0] / FPS for r in rates]
        br.sequence_scores([times[c] for c in clip_index[:n_host]], mins, SIGMA)
        t_kin = time.perf_counter() - t
        per_clip = {}
        for s in range(n_host):
            per_clip.setdefault(int(clip_index[s]), []).append(seqs[s])
        jobs = [(real[c * FRAMES:(c + 1) * FRAMES], g, deltas[c % 2]) for c, g in per_clip.items()]
        t = time.perf_counter()
        list(ex.map(_host_vertex, jobs))
        t_vertex = time.perf_counter() - t
    return t_audio, t_kin, t_vertex


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-procs", type=int, default=16)
    ap.add_argument("--host-sequences", type=int, default=576)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_beat.py needs the MI355X"
    from said_amd import _engine
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    waves, coeffs, real, clip_index = workload()
    n_seq, V = clip_index.shape[0], n_vertices()
    rng = np.random.default_rng(1)
    deltas = [(0.01 * rng.standard_normal((32, V, 3))).astype(np.float32) for _ in range(2)]

    eng = _engine.BeatEngine(device, SR)
    wave_dev = torch.from_numpy(np.concatenate(waves)).to(device)
    wave_off = np.arange(N_CLIPS + 1, dtype=np.int64) * CLIP_SAMPLES
    coeffs_dev = torch.from_numpy(coeffs).to(device)
    seq_off = np.arange(n_seq + 1, dtype=np.int64) * FRAMES
    both_dev = torch.cat([torch.from_numpy(real).to(device), coeffs_dev])
    real_off = clip_index.astype(np.int64) * FRAMES
    eval_off = N_CLIPS * FRAMES + seq_off[:-1]
    length = np.full(n_seq, FRAMES, dtype=np.int32)
    person = (clip_index % 2).astype(np.int32)
    eng.set_deltas(np.stack([d.reshape(32, -1) for d in deltas]).astype(np.float64))

    scores = {}

    def kinematic():
        eng.coeffs(coeffs_dev, seq_off, THRESHOLD)
        scores["s"] = eng.score(clip_index, FPS, SIGMA)

    audio_ms, audio_all = median_ms(lambda: eng.clips(wave_dev, wave_off), args.repeats)
    kin_ms, kin_all = median_ms(kinematic, args.repeats)
    vert_ms, vert_all = median_ms(lambda: eng.vertex_error(both_dev, real_off, eval_off, length, person), args.repeats)
    result = {"clips": N_CLIPS, "clip_seconds": CLIP_SAMPLES / SR, "sequences": n_seq, "frames": FRAMES, "vertices": V,
              "stft_frames": int(eng.frame_start[-1]), "onsets": int(sum(len(o) for o in eng.read_onsets())),
              "beat_consistency": float(np.mean(scores["s"])),
              "device_ms": {"audio": audio_ms, "kinematic_and_score": kin_ms, "vertex_error": vert_ms},
              "device_ms_all": {"audio": audio_all, "kinematic_and_score": kin_all, "vertex_error": vert_all}}
    if not args.no_host:
        n_host = min(n_seq, args.host_sequences)
        t_audio, t_kin, t_vertex = host_times(waves, coeffs, real, clip_index, deltas, args.host_procs, n_host)
        scale = n_seq / n_host
        result["host"] = {"procs": args.host_procs, "sequences_run": n_host, "audio_s": t_audio, "kinematic_and_score_s_run": t_kin,
                          "kinematic_and_score_s_scaled": t_kin * scale, "vertex_error_s_run": t_vertex, "vertex_error_s_scaled": t_vertex * scale}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
