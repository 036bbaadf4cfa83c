"""Host halves of the evaluation metrics (said_amd.metric, script/test_evaluate.py): the Frechet distance restatement, the WInD
transport LP, multimodality against golden G12, the evaluation driver's file enumeration and grouping, and its parser.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
from scipy import linalg
from scipy.optimize import linprog

from said_amd.metric.frechet_distance import frechet_distance
from said_amd.metric.multimodality import multimodality
from said_amd.metric.wind import StatisticGMM, transport_lp, wind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _driver():
    spec = importlib.util.spec_from_file_location("said_test_evaluate", os.path.join(ROOT, "script", "test_evaluate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _spd(rng, d):
    a = rng.normal(size=(d, d))
    return a @ a.T / d + 0.1 * np.eye(d)


def _fd_eig(mu1, s1, mu2, s2):
    """tr sqrt(S1 S2) = sum sqrt(eig(S1^1/2 S2 S1^1/2)): an independent form of the Frechet distance."""
    w, v = np.linalg.eigh(s1)
    r = (v * np.sqrt(w)) @ v.T
    lam = np.linalg.eigvalsh(r @ s2 @ r)
    return float(np.sum((mu1 - mu2) ** 2) + np.trace(s1) + np.trace(s2) - 2 * np.sum(np.sqrt(np.clip(lam, 0, None))))


@pytest.mark.parametrize("d", [2, 8, 64])
def test_frechet_distance_matches_eigenvalue_form(d):
    rng = np.random.default_rng(d)
    for _ in range(3):
        mu1, mu2, s1, s2 = rng.normal(size=d), rng.normal(size=d), _spd(rng, d), _spd(rng, d)
        got, want = frechet_distance(mu1, s1, mu2, s2), _fd_eig(mu1, s1, mu2, s2)
        assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (got, want)
    mu, s = rng.normal(size=d), _spd(rng, d)
    assert abs(frechet_distance(mu, s, mu, s)) < 1e-9


def test_frechet_distance_singular_product_takes_the_offset_path():
    s = np.zeros((4, 4))
    s[0, 0] = 1.0
    got = frechet_distance(np.zeros(4), s, np.ones(4), s)
    assert np.isfinite(got) and abs(got - 4.0) < 1e-2


def _stat(rng, d, w):
    return StatisticGMM(mean=rng.normal(size=d) * 3, cov=_spd(rng, d), weight=w)


def test_wind_single_component_is_the_frechet_distance():
    rng = np.random.default_rng(1)
    a, b = _stat(rng, 6, 1.0), _stat(rng, 6, 1.0)
    assert abs(wind([a], [b]) - frechet_distance(a.mean, a.cov, b.mean, b.cov)) < 1e-9


@pytest.mark.parametrize("k", [2, 3])
def test_wind_identical_and_permuted_mixtures(k):
    rng = np.random.default_rng(k)
    w = rng.dirichlet(np.ones(k))
    s1 = [_stat(rng, 5, w[i]) for i in range(k)]
    perm = list(reversed(range(k)))
    assert abs(wind(s1, s1)) < 1e-8
    assert abs(wind(s1, [s1[i] for i in perm])) < 1e-8
    # mixture 2 = mixture 1 with its means shifted: the plan is the identity, the cost the weighted shift
    shift = rng.normal(size=5)
    s2 = [StatisticGMM(s.mean + shift, s.cov, s.weight) for s in s1]
    assert abs(wind(s1, s2) - float(shift @ shift)) < 1e-6


def test_wind_matches_equality_form_lp():
    rng = np.random.default_rng(5)
    k = 4
    w1, w2 = rng.dirichlet(np.ones(k)), rng.dirichlet(np.ones(k))
    s1 = [_stat(rng, 4, w1[i]) for i in range(k)]
    s2 = [_stat(rng, 4, w2[i]) for i in range(k)]
    c, _, _, _, _ = transport_lp(s1, s2)
    # weights summing to 1: the inequalities are tight at any plan of total mass 1, i.e. the classic transport equalities
    A = np.vstack([np.kron(np.eye(k), np.ones((1, k))), np.kron(np.ones((1, k)), np.eye(k))])
    ref = linprog(c, A_eq=A, b_eq=np.concatenate([w1, w2]), bounds=(0, None), method="highs")
    assert ref.status == 0
    assert abs(wind(s1, s2) - ref.fun) <= 1e-7 * max(1.0, abs(ref.fun))


def test_multimodality_matches_golden(golden):
    g = golden("g12_metrics")
    spec = importlib.util.spec_from_file_location("make_golden_g12", os.path.join(ROOT, "tests", "golden", "make_golden_g12.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    B = mk.mixture(int(g["seed_b"]), int(g["n_b"]))
    h = B.shape[0] // 2
    assert abs(multimodality(list(B[:h]), list(B[h:2 * h])) - float(g["multimodality_b"])) <= 1e-6 * float(g["multimodality_b"])
    assert multimodality([], list(B[:1])) == 0


def _touch(path, text=""):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def test_file_enumeration_filter_and_grouping(tmp_path):
    ev = _driver()
    pid, other = ev.PERSON_IDS_TEST
    audio, gen, real = tmp_path / "audio", tmp_path / "gen", tmp_path / "real"
    for s in (1, 2):
        _touch(str(audio / pid / f"sentence{s:02}.wav"))
    _touch(str(audio / other / "sentence03.wav"))
    for r in (10, 2, 0, 1):
        _touch(str(gen / pid / f"sentence01-{r}.csv"))
    _touch(str(gen / pid / "sentence02.csv"))
    _touch(str(gen / pid / "sentence05-0.csv"))        # no audio: dropped
    _touch(str(gen / pid / "sentence01-x.txt"))        # not a CSV of the pattern
    _touch(str(gen / "FaceTalk_other_TA" / "sentence01-0.csv"))   # not a test speaker
    _touch(str(real / pid / "sentence01.csv"))
    paths = ev.get_data_paths(str(audio), str(gen))
    assert [(p, s, os.path.basename(f)) for p, s, f in paths] == [
        (pid, 1, "sentence01-0.csv"), (pid, 1, "sentence01-1.csv"), (pid, 1, "sentence01-2.csv"), (pid, 1, "sentence01-10.csv"),
        (pid, 2, "sentence02.csv")]
    assert [os.path.basename(f) for _, _, f in ev.get_data_paths(str(audio), str(real))] == ["sentence01.csv"]

    import torch
    keys = [(pid, 1, 0), (pid, 1, 1), (pid, 1, 0), (pid, 1, 1), (pid, 1, 0), (pid, 2, 0), (pid, 1, 0)]
    lat = torch.arange(len(keys), dtype=torch.float32)[:, None].repeat(1, 64)
    fk, fl = ev.filter_latents(keys, lat, [(pid, 1, 0), (pid, 2, 0)])
    assert fk == [(pid, 1, 0), (pid, 1, 0), (pid, 1, 0), (pid, 2, 0), (pid, 1, 0)]
    assert fl[:, 0].tolist() == [0, 2, 4, 5, 6]
    a, b = ev.multimodality_pairs(fk)
    assert (a, b) == ([0, 1], [2, 4])   # group (pid, 1, 0): rows 0, 1, 2, 4 -> halves [0, 1] | [2, 4]; (pid, 2, 0): one repeat, no pair


def test_parser_accepts_every_reference_flag():
    ev = _driver()
    argv = ["--audio_dir", "a", "--coeffs_dir", "b", "--coeffs_real_dir", "c", "--vae_weights_path", "synthetic", "--blendshape_residuals_path", "d",
            "--sampling_rate", "16000", "--fps", "60", "--bc_threshold", "0.1", "--wind_num_clusters", "5", "--wind_num_repeats", "3",
            "--window_step_size", "2", "--device", "cuda:0", "--seed", "4"]
    a = ev.build_parser().parse_args(argv)
    assert (a.wind_num_repeats, a.window_step_size, a.seed, a.vae_weights_path) == (3, 2, 4, "synthetic")
    d = ev.build_parser().parse_args(["--vae_weights_path", "x"])
    assert (d.wind_num_clusters, d.wind_num_repeats, d.window_step_size, d.seed) == (5, 10, 1, None)
    with pytest.raises(SystemExit):
        ev.build_parser().parse_args([])   # --vae_weights_path is required


def test_no_gpu_means_no_cpu_path():
    import torch
    from said_amd import _engine
    from said_amd.metric.frechet_distance import get_statistic
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_engine.NoCpuPathError):
        get_statistic(np.zeros((4, 64), dtype=np.float32))
