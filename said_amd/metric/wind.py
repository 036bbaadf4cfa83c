"""WInD, the Wasserstein distance between two Gaussian mixtures (said/metric/wind.py), the mixtures fitted on the MI355X.

``get_statistic_gmm`` fits ``GaussianMixture(n_components=K)`` with scikit-learn's defaults (said_amd/metric/_gmm.py: every pass over the
latents in HIP, float64).  ``wind`` solves the reference's transport LP over the pairwise Frechet distances of the components: minimise
sum d_jk p_jk subject to sum_k p_jk <= w1_j, sum_j p_jk <= w2_k, p >= 0, sum p = 1, with ``scipy.optimize.linprog`` (HiGHS) in place of
cvxopt's GLPK.  The optimum's value is unique, so the solver does not change the result beyond its tolerance.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
from scipy import sparse as sp
from scipy.optimize import linprog

from . import _gmm
from .frechet_distance import frechet_distance


@dataclass
class StatisticGMM:
    """Dataclass for the statistic of each modal of GMM"""

    mean: np.ndarray
    cov: np.ndarray
    weight: float


def get_statistic_gmm(data, num_clusters: int, random_state: Optional[int] = None) -> List[StatisticGMM]:
    """Means, covariances and weights of a num_clusters-component GMM fitted to the latents (a list of (64,) arrays, an (N, 64) array or an
    (N, 64) CUDA tensor).  random_state None draws from numpy's global generator, as scikit-learn does: np.random.seed makes it reproducible."""
    fit = _gmm.gmm_fit(data, num_clusters, random_state)
    return [StatisticGMM(mean=fit.means[c], cov=fit.covariances[c], weight=fit.weights[c]) for c in range(num_clusters)]


def transport_lp(stats1: List[StatisticGMM], stats2: List[StatisticGMM]):
    """(c, G, h, A, b) of the reference's LP (wind.py:69-100), dense."""
    k = len(stats1)
    d = np.zeros((k, k))
    for j in range(k):
        for m in range(k):
            d[j, m] = frechet_distance(stats1[j].mean, stats1[j].cov, stats2[m].mean, stats2[m].cov)
    h = np.array([s.weight for s in stats1] + [s.weight for s in stats2] + [0] * (k * k), dtype=np.float64)
    ineq1 = sp.block_diag([[[1] * k] for _ in range(k)], format="coo")
    eye = sp.identity(k, dtype="int", format="coo")
    ineq2 = sp.bmat([[eye for _ in range(k)]], dtype="int", format="coo")
    G = sp.bmat([[ineq1], [ineq2], [-sp.identity(k * k, dtype="int", format="coo")]], dtype="int", format="coo").toarray().astype(np.float64)
    return d.reshape(-1), G, h, np.ones((1, k * k)), np.ones(1)


def wind(stats1: List[StatisticGMM], stats2: List[StatisticGMM]) -> float:
    """WInD between the mixtures stats1 and stats2: the optimum of the transport LP."""
    c, G, h, A, b = transport_lp(stats1, stats2)
    res = linprog(c, A_ub=G, b_ub=h, A_eq=A, b_eq=b, bounds=(None, None), method="highs")
    if res.status != 0:
        raise RuntimeError(f"WInD transport LP failed: {res.message}")
    return float(res.fun)
