"""GPU tests of beat consistency and vertex error (said_amd/csrc/beat.hip, include/said_beat.h, said_amd.metric.beat_consistency /
.vertex_error, script/evaluate_extra.py) against the float64 restatement of DESIGN.md section 12.1 in tests/beat_ref.py.

Tolerances: a float64 radix-2 transform of 2048 points leaves about 1e-15 of the frame's largest power on every bin, so the mel power is
held to 1e-12 of the clip's maximum; a band 80 dB under that maximum then carries about 1e-12 relative, 4.3e-12 dB, and the envelope (values
of order 10) is held to 1e-9 absolute.  Onset and minima indices must be EQUAL: tests/test_beat_cpu.py shows that on these seeded inputs the
restatement decides nothing within 1e-6.  Scores are held to 1e-12."""
import importlib.util
import os
import pickle
import re
import statistics
import subprocess
import sys

import numpy as np
import pytest
import torch

import beat_ref as br

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(0.1, 0.1), (0.5, 0.02)]   # (threshold, sigma); the second makes the score sensitive to every beat time


@pytest.fixture(scope="module")
def ref16():
    """The restatement of the 16 kHz group, computed once: per (threshold, sigma) the whole result, the clips analysed once."""
    waves = br.clips_16k()
    seqs, clip_index = br.sequences()
    out = {pair: br.beat_consistency(waves, seqs, clip_index, 16000, 60, *pair) for pair in PAIRS}
    return waves, seqs, clip_index, out


def _engine(sr):
    from said_amd import _engine
    return _engine.BeatEngine(torch.device("cuda:0"), sr)


def _upload_clips(eng, waves):
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    return eng.clips(torch.from_numpy(np.concatenate(waves)).cuda(), offsets)


def _upload_seqs(eng, seqs, threshold):
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in seqs])]).astype(np.int64)
    eng.coeffs(torch.from_numpy(np.concatenate(seqs)).cuda(), offsets, threshold)


def _check_clips(eng, waves, start, beats):
    mel, env, onsets = eng.read_mel(), eng.read_envelope(), eng.read_onsets()
    assert start.tolist() == np.concatenate([[0], np.cumsum([br.n_frames(len(w)) for w in waves])]).tolist()
    worst_mel = worst_env = 0.0
    for i, b in enumerate(beats):
        m, e = mel[start[i]:start[i + 1]], env[start[i]:start[i + 1]]
        assert m.shape == b["mel"].shape
        scale = b["mel"].max()
        err_mel = float(np.abs(m - b["mel"]).max() / scale) if scale > 0 else float(np.abs(m).max())
        err_env = float(np.abs(e - b["env"]).max())
        print(f"clip {i} ({len(waves[i])} samples): mel {err_mel:.3e} of its maximum, envelope {err_env:.3e}, onsets {onsets[i].tolist()}")
        worst_mel, worst_env = max(worst_mel, err_mel), max(worst_env, err_env)
        assert err_mel <= 1e-12, i
        assert err_env <= 1e-9, i
        assert onsets[i].tolist() == b["onsets"].tolist(), i
    return worst_mel, worst_env


def test_clips_16k_in_one_call(ref16):
    waves, _, _, out = ref16
    eng = _engine(16000)
    assert eng.peak_pick == br.peak_params(16000) == (0, 1, 3, 4, 0)
    start = _upload_clips(eng, waves)
    _check_clips(eng, waves, start, out[PAIRS[0]]["clips"])
    assert eng.read_onsets()[-1].shape == (0,) and not eng.read_envelope()[start[-2]:].any()   # the silent clip


def test_clip_44k():
    y = br.clip_44k()
    eng = _engine(44100)
    assert eng.peak_pick == br.peak_params(44100) == (2, 1, 8, 9, 2)
    start = _upload_clips(eng, [y])
    want = br.audio_beats(y, 44100)
    _check_clips(eng, [y], start, [want])
    from said_amd.util.audio import compute_audio_beat_time
    got = compute_audio_beat_time(y, 44100)
    assert got.tolist() == want["times"].tolist() and len(got) >= 1


def _same(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all(np.abs(a - b)[~np.isnan(a)] <= tol))


@pytest.mark.parametrize("threshold,sigma", PAIRS)
def test_minima_and_scores(ref16, threshold, sigma):
    waves, seqs, clip_index, out = ref16
    want = out[(threshold, sigma)]
    eng = _engine(16000)
    _upload_clips(eng, waves)
    _upload_seqs(eng, seqs, threshold)
    rates, minima = eng.read_rates(), eng.read_minima()
    for s, (r, m) in enumerate(zip(rates, minima)):
        assert r.shape == want["rates"][s].shape and np.abs(r - want["rates"][s]).max() <= 1e-12 * max(1.0, want["rates"][s].max()), s
        assert m.tolist() == want["minima"][s].tolist(), s
    scores = eng.score(clip_index, 60, sigma)
    print("scores", scores.tolist(), "restatement", want["scores"].tolist())
    assert _same(scores, want["scores"], 1e-12) and not np.isnan(scores).any()
    assert abs(float(np.mean(scores)) - want["score"]) <= 1e-12

    # the public function: the repeats of a clip are the same object and are analysed once
    from said_amd.metric.beat_consistency import beat_consistency_score, beat_consistency_scores
    per_seq = beat_consistency_scores([waves[c] for c in clip_index], seqs, 16000, 60, threshold, sigma)
    assert per_seq.tolist() == scores.tolist()
    from said_amd.metric import beat_consistency as bc
    assert len(bc.engine_for(None, 16000).frame_start) - 1 == len(set(clip_index))
    assert abs(beat_consistency_score([waves[c] for c in clip_index], seqs, 16000, 60, threshold, sigma) - want["score"]) <= 1e-12

    # a sequence with kinematic beats against the silent clip: NaN, here and in the restatement
    silent = list(clip_index)
    silent[-1] = len(waves) - 1
    want_nan = br.sequence_scores([want["clips"][c]["times"] for c in silent], [m / 60 for m in want["minima"]], sigma)
    got_nan = eng.score(silent, 60, sigma)
    assert np.isnan(want_nan[-1]) and _same(got_nan, want_nan, 1e-12)

    # two runs are bit-identical
    eng2 = _engine(16000)
    _upload_clips(eng2, waves)
    _upload_seqs(eng2, seqs, threshold)
    assert eng2.read_mel().tobytes() == eng.read_mel().tobytes() and eng2.read_envelope().tobytes() == eng.read_envelope().tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(eng2.read_rates(), rates))
    assert eng2.score(clip_index, 60, sigma).tobytes() == scores.tobytes()


def test_constant_channel_gives_nan_rates(ref16):
    waves = ref16[0]
    seqs, clip_index = br.constant_channel_sequences()
    want = br.beat_consistency(waves, seqs, clip_index, 16000, 60, 0.1)
    eng = _engine(16000)
    _upload_clips(eng, waves)
    _upload_seqs(eng, seqs, 0.1)
    assert all(np.isnan(r).all() for r in eng.read_rates()) and all(np.isnan(r).all() for r in want["rates"])
    assert [m.tolist() for m in eng.read_minima()] == [m.tolist() for m in want["minima"]] == [[], []]
    assert _same(eng.score(clip_index, 60, 0.1), want["scores"], 1e-12)


def test_short_sequence_is_refused():
    from said_amd import _engine as E
    from said_amd.metric.beat_consistency import beat_consistency_score
    with pytest.raises(ValueError, match="fewer than 2 frames"):
        beat_consistency_score([np.zeros(800, dtype=np.float32)], [np.zeros((1, 32), dtype=np.float32)], 16000, 60, 0.1)
    eng = _engine(16000)
    with pytest.raises(E.EngineError, match="at least 2"):
        eng.coeffs(torch.zeros(3, 32, device="cuda"), [0, 1, 3], 0.1)
    with pytest.raises(E.EngineError, match="needs clips"):
        eng.score([0], 60, 0.1)
    with pytest.raises(E.EngineError, match="needs set_deltas"):
        eng.vertex_error(torch.zeros(3, 32, device="cuda"), [0], [1], [1], [0])


@pytest.mark.parametrize("n_vertices", [37, 1000])
def test_vertex_error(n_vertices):
    from said_amd.metric.vertex_error import mean_vertex_error, vertex_error, vertex_errors
    pairs, deltas = br.vertex_case(n_vertices)
    assert any(len(r) != len(g) for r, g, _ in pairs) and any(min(len(r), len(g)) == 1 for r, g, _ in pairs) and {p for _, _, p in pairs} == {0, 1}
    want = np.array([br.vertex_error(r, g, deltas[p]) for r, g, p in pairs])
    got = vertex_errors(pairs, deltas)
    print("vertex errors", got.tolist(), "relative difference", (np.abs(got - want) / want).max())
    assert (np.abs(got - want) <= 1e-12 * want).all() and (want > 0).all()
    assert mean_vertex_error(pairs, deltas) == statistics.mean(float(e) for e in got)
    assert abs(mean_vertex_error(pairs, deltas) - br.mean_vertex_error(pairs, deltas)) <= 1e-12 * br.mean_vertex_error(pairs, deltas)
    assert vertex_error(pairs[0][0], pairs[0][1], deltas[0]) == got[0]
    assert vertex_errors(pairs, deltas).tobytes() == got.tobytes()


def _write_wav(path, y, sr):
    from scipy.io import wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, sr, np.round(np.clip(y, -1, 1) * 32767).astype(np.int16))


def _write_csv(path, coeffs):
    from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, save_blendshape_coeffs
    os.makedirs(os.path.dirname(path), exist_ok=True)
    save_blendshape_coeffs(coeffs, DEFAULT_BLENDSHAPE_CLASSES, path)


def test_driver_prints_extra_metrics(tmp_path):
    """script/evaluate_extra.py --beat_consistency --vertex_error in a child process: script/test_evaluate.py's EvalMetrics line as ever, then ExtraMetrics with the
    restatement's beat consistency and vertex error of what the driver loads (the WAV and CSV files as written, read back through the package's loaders)."""
    from said_amd.util.audio import load_audio
    from said_amd.util.blendshape import load_blendshape_coeffs
    spec = importlib.util.spec_from_file_location("said_test_evaluate_beat", os.path.join(ROOT, "script", "test_evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES
    rng = np.random.default_rng(11)
    audio, gen, real = tmp_path / "audio", tmp_path / "gen", tmp_path / "real"
    pid = ev.PERSON_IDS_TEST[0]
    delta = (0.01 * rng.standard_normal((32, 37, 3))).astype(np.float32)
    with open(tmp_path / "residuals.pickle", "wb") as f:
        pickle.dump({pid: {name: delta[i] for i, name in enumerate(DEFAULT_BLENDSHAPE_CLASSES)}}, f)
    for sid in (1, 2):
        _write_wav(str(audio / pid / f"sentence{sid:02}.wav"), br.burst_clip(16000, 16000, rng), 16000)
        _write_csv(str(real / pid / f"sentence{sid:02}.csv"), br.smooth_coeffs(200, rng))
        for r in range(2):
            _write_csv(str(gen / pid / f"sentence{sid:02}-{r}.csv"), br.smooth_coeffs(200 + 4 * r, rng))
    cmd = [sys.executable, os.path.join(ROOT, "script", "evaluate_extra.py"), "--audio_dir", str(audio), "--coeffs_dir", str(gen),
           "--coeffs_real_dir", str(real), "--vae_weights_path", "synthetic", "--wind_num_clusters", "2", "--wind_num_repeats", "2", "--seed", "5",
           "--beat_consistency", "--vertex_error", "--blendshape_residuals_path", str(tmp_path / "residuals.pickle")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert re.fullmatch(r"EvalMetrics\(frechet_distance=\S+, multimodality=\S+, wind=StatisticMetric\(mean=\S+, std=\S+\)\)", lines[-2]), r.stdout
    m = re.fullmatch(r"ExtraMetrics\(beat_consistency=(\S+), vertex_error=(\S+)\)", lines[-1])
    assert m, r.stdout
    paths = ev.get_data_paths(str(audio), str(gen))
    waves = {sid: load_audio(str(audio / pid / f"sentence{sid:02}.wav"), 16000).numpy() for sid in (1, 2)}
    want = br.beat_consistency([waves[1], waves[2]], [load_blendshape_coeffs(p).numpy() for _, _, p in paths], [sid - 1 for _, sid, _ in paths],
                               16000, 60, 0.1)
    assert len(paths) == 4 and all(len(c["onsets"]) for c in want["clips"]) and any(len(k) for k in want["minima"])
    assert abs(float(m.group(1)) - want["score"]) <= 1e-12
    reals = {sid: load_blendshape_coeffs(str(real / pid / f"sentence{sid:02}.csv")).numpy() for sid in (1, 2)}
    want_ve = br.mean_vertex_error([(reals[sid], load_blendshape_coeffs(p).numpy(), 0) for _, sid, p in paths], [delta])
    assert abs(float(m.group(2)) - want_ve) <= 1e-12 * want_ve and want_ve > 0
