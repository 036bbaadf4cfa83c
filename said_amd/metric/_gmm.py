"""k-means and full-covariance Gaussian mixtures over (N, 64) latents on the MI355X (include/said_metrics.h).

scikit-learn's ``GaussianMixture(n_components=K).fit`` as called by the reference's ``get_statistic_gmm`` (said/metric/wind.py:35),
with its defaults: ``covariance_type="full"``, ``tol=1e-3``, ``reg_covar=1e-6``, ``max_iter=100``, ``n_init=1``, responsibilities
initialised one-hot from ``KMeans(n_clusters=K, n_init=1)`` (k-means++ seeding with 2 + floor(ln K) local trials, Lloyd, ``max_iter=300``,
``tol=1e-4`` scaled by the mean per-feature variance).  Every pass over the N points runs in HIP (float64 accumulation); the K x 64 x 64
algebra (Cholesky, triangular inverse, log-determinants), the draws of the seeded generator and the convergence tests run here, in
scikit-learn's order of operations.

Differences from scikit-learn, all at rounding level: sums run in the kernels' fixed order rather than numpy's; KMeans here does not
subtract the data mean before clustering (scikit-learn does, for numerical accuracy, and adds it back to the centres).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch
from scipy import linalg

from .. import _engine

D = _engine.METRICS_DIM
REG_COVAR, TOL, MAX_ITER = 1e-6, 1e-3, 100
KMEANS_MAX_ITER, KMEANS_TOL = 300, 1e-4

_engines: Dict[int, _engine.MetricsEngine] = {}


def device_latents(data) -> torch.Tensor:
    """(N, 64) float32 contiguous latents on the current CUDA device.  `data` is a list of (64,) arrays (the reference's form), an (N, 64) array
    or tensor; host data is uploaded once.  There is no CPU path."""
    if isinstance(data, torch.Tensor):
        t = data
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(data, dtype=np.float32)))
    if t.dim() != 2 or t.shape[1] != D:
        raise ValueError(f"latents must be (N, {D}), got {tuple(t.shape)}")
    if t.shape[0] < 1:
        raise ValueError("no latents")
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise _engine.NoCpuPathError("said_amd.metric computes on the MI355X only: no CUDA device is visible")
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return t.to(torch.float32).contiguous()


def engine_for(x: torch.Tensor) -> _engine.MetricsEngine:
    """The metrics context of x's device, with workspace for at least x.shape[0] points (grown by re-creation)."""
    idx = x.device.index if x.device.index is not None else torch.cuda.current_device()
    e = _engines.get(idx)
    if e is None or e.max_points < x.shape[0]:
        if e is not None:
            e.close()
        e = _engine.MetricsEngine(torch.device("cuda", idx), max(int(x.shape[0]), 1024))
        _engines[idx] = e
    return e


def moments(x: torch.Tensor, k: int = 1, wsrc: int = _engine.W_UNIT, eng: Optional[_engine.MetricsEngine] = None, nk_offset: float = 0.0):
    """(n_k, means, scatter) in float64: n_k = sum r (+ nk_offset), means = sum r x / n_k, scatter = sum r (x - mu)(x - mu)^T (two passes)."""
    eng = eng or engine_for(x)
    nk, sx = eng.weighted_sums(x, k, wsrc)
    nk = nk + nk_offset
    means = sx / nk[:, np.newaxis]
    return nk, means, eng.weighted_scatter(x, k, wsrc, means)


# ---------------------------------------------------------------- host algebra (sklearn.mixture._gaussian_mixture, full covariances)
def precision_cholesky(covariances: np.ndarray) -> np.ndarray:
    """_compute_precision_cholesky(covariances, "full")."""
    out = np.empty_like(covariances)
    for k, cov in enumerate(covariances):
        try:
            chol = linalg.cholesky(cov, lower=True)
        except linalg.LinAlgError:
            raise ValueError("Fitting the mixture model failed because some components have ill-defined empirical covariance "
                             "(for instance caused by singleton or collapsed samples). Try to decrease the number of components, or increase reg_covar.")
        out[k] = linalg.solve_triangular(chol, np.eye(cov.shape[0]), lower=True).T
    return out


def log_det_cholesky(prec_chol: np.ndarray) -> np.ndarray:
    """_compute_log_det_cholesky(prec_chol, "full", d)."""
    n, d, _ = prec_chol.shape
    return np.sum(np.log(prec_chol.reshape(n, -1)[:, :: d + 1]), 1)


@dataclass
class GMMFit:
    weights: np.ndarray        # (K,)
    means: np.ndarray          # (K, 64)
    covariances: np.ndarray    # (K, 64, 64)
    precisions_cholesky: np.ndarray
    lower_bound: float
    n_iter: int
    converged: bool


def _m_step(eng, x, k, wsrc, reg_covar):
    """_estimate_gaussian_parameters(X, resp, reg_covar, "full"): (nk, means, covariances)."""
    nk, means, scatter = moments(x, k, wsrc, eng, nk_offset=10 * np.finfo(np.float64).eps)
    cov = scatter / nk[:, np.newaxis, np.newaxis]
    for c in cov:
        c.flat[:: D + 1] += reg_covar
    return nk, means, cov


def estep(eng, x, weights, means, prec_chol, want_resp=False):
    """GaussianMixture._e_step on the device: the mean log_prob_norm (and, with want_resp, log_resp and log_prob_norm)."""
    mean_prec = np.stack([np.dot(mu, pc) for mu, pc in zip(means, prec_chol)])
    return eng.gmm_estep(x, prec_chol, mean_prec, log_det_cholesky(prec_chol), np.log(weights), want_resp=want_resp)


def gmm_fit_from_labels(x: torch.Tensor, labels: Optional[np.ndarray], k: int, eng=None, tol: float = TOL, reg_covar: float = REG_COVAR,
                        max_iter: int = MAX_ITER) -> GMMFit:
    """GaussianMixture.fit_predict's single initialisation from one-hot responsibilities of `labels` (None: the context's last k-means labels)."""
    eng = eng or engine_for(x)
    n = x.shape[0]
    if labels is not None:
        eng.kmeans_set_labels(labels, k)
    nk, means, cov = _m_step(eng, x, k, _engine.W_LABELS, reg_covar)   # _initialize
    weights = nk / n
    prec = precision_cholesky(cov)
    lower_bound, converged, n_iter = -np.inf, False, 0
    for n_iter in range(1, max_iter + 1):
        prev = lower_bound
        lower_bound = estep(eng, x, weights, means, prec)
        nk, means, cov = _m_step(eng, x, k, _engine.W_RESP, reg_covar)
        weights = nk / nk.sum()
        prec = precision_cholesky(cov)
        if abs(lower_bound - prev) < tol:
            converged = True
            break
    return GMMFit(weights, means, cov, prec, float(lower_bound), n_iter, converged)


# ---------------------------------------------------------------- k-means (sklearn.cluster._kmeans)
def _rng(random_state) -> np.random.RandomState:
    """check_random_state: None -> numpy's global RandomState, an int -> a fresh seeded one."""
    if random_state is None:
        return np.random.mtrand._rand
    if isinstance(random_state, np.random.RandomState):
        return random_state
    return np.random.RandomState(random_state)


def _row(x: torch.Tensor, i: int) -> np.ndarray:
    return x[i].double().cpu().numpy()


def kmeans_plusplus(x: torch.Tensor, k: int, random_state, eng=None, n_local_trials: Optional[int] = None):
    """_kmeans_plusplus(X, k, random_state): (centres (k, 64) float64, indices (k,))."""
    eng = eng or engine_for(x)
    rs = _rng(random_state)
    n = x.shape[0]
    if n_local_trials is None:
        n_local_trials = 2 + int(np.log(k))
    w = np.ones(n)
    centre_id = rs.choice(n, p=w / w.sum())
    idx = [int(centre_id)]
    pot = eng.kmeanspp_first(x, centre_id)
    for _ in range(1, k):
        rand_vals = rs.uniform(size=n_local_trials) * pot
        cid, pot = eng.kmeanspp_step(x, rand_vals)
        idx.append(cid)
    return np.stack([_row(x, i) for i in idx]), np.array(idx)


def _variance_tol(eng, x, tol):
    """_tolerance(X, tol) = mean(var(X, axis=0)) * tol."""
    n = x.shape[0]
    _, _, sc = moments(x, 1, _engine.W_UNIT, eng)
    return float(np.mean(np.diag(sc[0]) / n)) * tol


def kmeans_lloyd(x: torch.Tensor, centres: np.ndarray, eng=None, max_iter: int = KMEANS_MAX_ITER, tol: float = KMEANS_TOL):
    """_kmeans_single_lloyd from `centres`: (centres, n_iter, inertia); the final labels stay in the context (W_LABELS)."""
    eng = eng or engine_for(x)
    k = centres.shape[0]
    abs_tol = _variance_tol(eng, x, tol)
    centres = np.array(centres, dtype=np.float64)
    strict, i = False, 0
    for i in range(max_iter):
        changed, _ = eng.kmeans_assign(x, centres, compare=i > 0)
        cnt, sums = eng.weighted_sums(x, k, _engine.W_LABELS)
        empty = np.where(cnt == 0)[0]
        if empty.size:   # _relocate_empty_clusters_dense: the farthest points from their old centres
            labels, dist = eng.kmeans_read(x.shape[0])
            far = np.argsort(-dist, kind="stable")[: empty.size]
            for new_c, p in zip(empty, far):
                xp = _row(x, int(p))
                old_c = labels[p]
                sums[old_c] -= xp
                sums[new_c] = xp
                cnt[new_c] = 1.0
                cnt[old_c] -= 1.0
        new = sums / np.where(cnt > 0, cnt, 1.0)[:, np.newaxis]
        shift = np.sqrt(((new - centres) ** 2).sum(axis=1))
        centres = new
        if i > 0 and changed == 0:
            strict = True
            break
        if (shift ** 2).sum() <= abs_tol:
            break
    inertia = None
    if not strict:   # relabel from the final centres (strict convergence: the labels already match them)
        _, inertia = eng.kmeans_assign(x, centres, compare=False)
    return centres, i + 1, inertia


def kmeans(x: torch.Tensor, k: int, random_state, eng=None):
    """KMeans(n_clusters=k, n_init=1, random_state).fit(X): (centres, n_iter, inertia); labels in the context."""
    eng = eng or engine_for(x)
    c0, _ = kmeans_plusplus(x, k, random_state, eng)
    return kmeans_lloyd(x, c0, eng)


def gmm_fit(data, k: int, random_state=None) -> GMMFit:
    """GaussianMixture(n_components=k, random_state=random_state).fit(data)."""
    if not 1 <= k <= _engine.METRICS_MAX_K:
        raise ValueError(f"num_clusters must be in [1, {_engine.METRICS_MAX_K}], got {k}")
    x = device_latents(data)
    if x.shape[0] < k:
        raise ValueError(f"n_samples={x.shape[0]} should be >= n_clusters={k}.")
    eng = engine_for(x)
    rs = _rng(random_state)
    kmeans(x, k, rs, eng)
    return gmm_fit_from_labels(x, None, k, eng)
