"""Evaluation metrics on the MI355X (include/said_metrics.h, said_amd/csrc/metrics.hip; said_amd.metric; script/test_evaluate.py) against
float64 numpy restatements and golden G12 (scikit-learn 1.x GaussianMixture / KMeans and the reference's said.metric, captured by
tests/golden/make_golden_g12.py; the data are regenerated here from its seeded generator)."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MK = _load("make_golden_g12", os.path.join(ROOT, "tests", "golden", "make_golden_g12.py"))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


@pytest.mark.parametrize("n", [2, 1000, 4099, 1_000_003])
def test_moments_match_numpy(n):
    from said_amd.metric import _gmm
    from said_amd.metric.frechet_distance import get_statistic
    rng = np.random.default_rng(n)
    x = (rng.normal(size=(n, 64)) * rng.uniform(0.1, 3.0, size=64) + rng.normal(size=64) * 5).astype(np.float32)
    st = get_statistic(_dev(x))
    x64 = x.astype(np.float64)
    mean, cov = np.mean(x64, axis=0), np.cov(x64, rowvar=False)
    scale = np.abs(cov).max()
    assert np.abs(st.mean - mean).max() <= 1e-12 * np.abs(mean).max()
    assert np.abs(st.cov - cov).max() <= 1e-12 * scale
    # list-of-rows input (the reference's form) gives the same bits as the device tensor
    if n <= 1000:
        st2 = get_statistic(list(x))
        assert np.array_equal(st2.mean, st.mean) and np.array_equal(st2.cov, st.cov)
    # bit-identical run to run
    nk, mu, sc = _gmm.moments(_dev(x))
    nk2, mu2, sc2 = _gmm.moments(_dev(x))
    assert nk[0] == n and np.array_equal(mu, mu2) and np.array_equal(sc, sc2)


def _numpy_estep(X, weights, means, prec_chol):
    d = X.shape[1]
    log_det = np.array([np.sum(np.log(np.diag(p))) for p in prec_chol])
    lp = np.empty((X.shape[0], len(means)))
    for k, (mu, pc) in enumerate(zip(means, prec_chol)):
        y = X @ pc - mu @ pc
        lp[:, k] = np.sum(y * y, axis=1)
    w = -0.5 * (d * np.log(2 * np.pi) + lp) + log_det + np.log(weights)
    m = w.max(axis=1, keepdims=True)
    norm = np.log(np.exp(w - m).sum(axis=1)) + m[:, 0]
    return w - norm[:, None], norm


def test_estep_matches_numpy(golden):
    from said_amd.metric import _gmm
    g = golden("g12_metrics")
    X = MK.mixture(int(g["seed_em"]), int(g["n_a"]), sep=float(g["sep_em"]))
    weights, means, cov = g["em_weights"], g["em_means"], g["em_covariances"]
    prec = _gmm.precision_cholesky(cov)
    x = _dev(X)
    eng = _gmm.engine_for(x)
    lb, lr, lpn = _gmm.estep(eng, x, weights, means, prec, want_resp=True)
    ref_lr, ref_norm = _numpy_estep(X.astype(np.float64), weights, means, prec)
    assert np.abs(lr.cpu().numpy() - ref_lr).max() <= 1e-9 * np.abs(ref_norm).max()
    assert np.abs(lpn.cpu().numpy() - ref_norm).max() <= 1e-11 * np.abs(ref_norm).max()
    assert abs(lb - ref_norm.mean()) <= 1e-12 * abs(ref_norm.mean())


def test_em_from_kmeans_labels_matches_sklearn(golden):
    from said_amd.metric import _gmm
    g = golden("g12_metrics")
    X = MK.mixture(int(g["seed_em"]), int(g["n_a"]), sep=float(g["sep_em"]))
    fit = _gmm.gmm_fit_from_labels(_dev(X), g["em_labels"], int(g["k"]))
    assert fit.converged and fit.n_iter == int(g["em_n_iter"])
    assert abs(fit.lower_bound - float(g["em_lower_bound"])) <= 1e-9 * abs(float(g["em_lower_bound"]))
    for got, want in ((fit.weights, g["em_weights"]), (fit.means, g["em_means"]), (fit.covariances, g["em_covariances"])):
        assert np.abs(got - want).max() <= 1e-7 * (want.max() - want.min())


def test_lloyd_from_explicit_centres_matches_sklearn(golden):
    from said_amd.metric import _gmm
    g = golden("g12_metrics")
    A = MK.mixture(int(g["seed_a"]), int(g["n_a"]))
    x = _dev(A)
    eng = _gmm.engine_for(x)
    centres, n_iter, _ = _gmm.kmeans_lloyd(x, A[g["lloyd_init_idx"]].astype(np.float64), eng)
    labels, _ = eng.kmeans_read(A.shape[0])
    assert n_iter == int(g["lloyd_n_iter"])
    assert np.array_equal(labels, g["lloyd_labels"])
    assert np.abs(centres - g["lloyd_centres"]).max() <= 1e-9


def test_kmeanspp_properties():
    from said_amd.metric import _gmm
    A = MK.mixture(3, 20000)
    x = _dev(A)
    c1, i1 = _gmm.kmeans_plusplus(x, 5, 11)
    c2, i2 = _gmm.kmeans_plusplus(x, 5, 11)
    c3, i3 = _gmm.kmeans_plusplus(x, 5, 12)
    assert len(set(i1.tolist())) == 5
    assert np.array_equal(c1, A[i1].astype(np.float64))
    assert np.array_equal(c1, c2) and np.array_equal(i1, i2)
    assert not np.array_equal(i1, i3)


def test_wind_of_gmm_fits_matches_golden(golden):
    from said_amd.metric.frechet_distance import frechet_distance
    from said_amd.metric.wind import get_statistic_gmm, wind
    g = golden("g12_metrics")
    k = int(g["k"])
    A, B = MK.mixture(int(g["seed_a"]), int(g["n_a"])), MK.mixture(int(g["seed_b"]), int(g["n_b"]))
    xa, xb = _dev(A), _dev(B)
    np.random.seed(int(g["wind_seed"]))
    s1, s2 = get_statistic_gmm(xa, k), get_statistic_gmm(list(B), k)
    w = wind(s1, s2)
    assert abs(w - float(g["wind"])) <= 1e-6 * abs(float(g["wind"]))
    assert np.allclose(sorted(s.weight for s in s1), sorted(g["wind_weights_a"]), rtol=0, atol=1e-9)
    # fixed seed: bit-identical
    r1 = [get_statistic_gmm(xa, k, random_state=3) for _ in range(2)]
    for a, b in zip(*r1):
        assert np.array_equal(a.mean, b.mean) and np.array_equal(a.cov, b.cov) and a.weight == b.weight
    # K = 1: the FD of the biased covariances + reg_covar
    one_a, one_b = get_statistic_gmm(xa, 1, random_state=0), get_statistic_gmm(xb, 1, random_state=0)
    ca = np.cov(A.astype(np.float64), rowvar=False, bias=True) + 1e-6 * np.eye(64)
    cb = np.cov(B.astype(np.float64), rowvar=False, bias=True) + 1e-6 * np.eye(64)
    want = frechet_distance(A.astype(np.float64).mean(0), ca, B.astype(np.float64).mean(0), cb)
    assert abs(wind(one_a, one_b) - want) <= 1e-8 * want


def _write_wav(path):
    from scipy.io import wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, 16000, np.zeros(1600, dtype=np.int16))


def _write_csv(path, coeffs):
    from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, save_blendshape_coeffs
    os.makedirs(os.path.dirname(path), exist_ok=True)
    save_blendshape_coeffs(coeffs, DEFAULT_BLENDSHAPE_CLASSES, path)


def test_test_evaluate_end_to_end(tmp_path):
    from oracle import vae as ov
    from said_amd.metric.wind import get_statistic_gmm, wind
    from said_amd.model.vae import BCVAE
    from said_amd.util import synth
    ev = _load("said_test_evaluate", os.path.join(ROOT, "script", "test_evaluate.py"))
    rng = np.random.default_rng(0)
    audio, gen, real = tmp_path / "audio", tmp_path / "gen", tmp_path / "real"

    def walk(T):
        return np.clip(0.5 + np.cumsum(rng.normal(scale=0.05, size=(T, 32)), axis=0), 0, 1).astype(np.float32)

    for pid in ev.PERSON_IDS_TEST:
        for sid, T in ((1, 300), (2, 360), (4, 250)):
            _write_wav(str(audio / pid / f"sentence{sid:02}.wav"))
            _write_csv(str(real / pid / f"sentence{sid:02}.csv"), walk(T))
            for r in range(4):
                _write_csv(str(gen / pid / f"sentence{sid:02}-{r}.csv"), walk(T + 3 * r))
    seed, repeats, k = 5, 2, 2
    cmd = [sys.executable, os.path.join(ROOT, "script", "test_evaluate.py"), "--audio_dir", str(audio), "--coeffs_dir", str(gen),
           "--coeffs_real_dir", str(real), "--vae_weights_path", "synthetic", "--wind_num_clusters", str(k), "--wind_num_repeats", str(repeats),
           "--seed", str(seed)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    m = re.search(r"EvalMetrics\(frechet_distance=(\S+), multimodality=(\S+), wind=StatisticMetric\(mean=(\S+), std=(\S+)\)\)", r.stdout)
    assert m, r.stdout
    fd, mm, wmean, wstd = (float(v) for v in m.groups())

    # CPU: oracle/vae.py latents, numpy / scipy metrics
    sd = synth.vae_state_dict()
    def cpu_latents(paths, padding):
        from said_amd.util.blendshape import load_blendshape_coeffs
        keys, lats = [], []
        for pid, sid, path in paths:
            lat = ov.window_latents(sd, load_blendshape_coeffs(path), 1, padding).numpy().astype(np.float64)
            keys += [(pid, sid, w) for w in range(lat.shape[0])]
            lats.append(lat)
        return keys, np.concatenate(lats)
    ek, el = cpu_latents(ev.get_data_paths(str(audio), str(gen)), 0)
    rk, rl = cpu_latents(ev.get_data_paths(str(audio), str(real)), 2)
    keep = [i for i, key in enumerate(ek) if key in set(rk)]
    ek, el = [ek[i] for i in keep], el[keep]
    from scipy import linalg
    mu1, mu2, s1, s2 = el.mean(0), rl.mean(0), np.cov(el, rowvar=False), np.cov(rl, rowvar=False)
    covmean = linalg.sqrtm(s1 @ s2).real
    fd_cpu = float(((mu1 - mu2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean))
    a, b = ev.multimodality_pairs(ek)
    mm_cpu = float(np.linalg.norm(el[a] - el[b], axis=1).mean())
    # The HIP encoder is within 1e-4 of the latents' range of the oracle (tests/test_gpu_vae.py).  FD and multimodality are sums of
    # 64 terms, each moved by at most about that relative amount by such an error, so 1e-3 relative bounds the difference with margin.
    assert abs(fd - fd_cpu) <= 1e-3 * abs(fd_cpu), (fd, fd_cpu)
    assert abs(mm - mm_cpu) <= 1e-3 * abs(mm_cpu), (mm, mm_cpu)

    # WInD: said_amd.metric with the same seed on the same (HIP) latents
    vae = BCVAE()
    vae.load_state_dict(sd, strict=True)
    vae.to("cuda:0").eval()
    ek2, el2 = ev.generate_latents(vae, ev.get_data_paths(str(audio), str(gen)), 1, torch.device("cuda:0"))
    rk2, rl2 = ev.generate_latents(vae, ev.get_data_paths(str(audio), str(real)), 1, torch.device("cuda:0"), padding=2)
    ek2, el2 = ev.filter_latents(ek2, el2, rk2)
    np.random.seed(seed)
    scores = [wind(get_statistic_gmm(el2, k), get_statistic_gmm(rl2, k)) for _ in range(repeats)]
    import statistics
    assert abs(wmean - statistics.mean(scores)) <= 1e-9 * abs(wmean)
    assert abs(wstd - statistics.stdev(scores)) <= 1e-9 * max(abs(wmean), 1e-30)
