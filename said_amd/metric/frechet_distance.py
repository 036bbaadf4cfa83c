"""Frechet distance of latent sets (said/metric/frechet_distance.py), the moments computed on the MI355X.

``get_statistic`` is the reference's ``np.mean`` / ``np.cov(rowvar=False)`` (ddof = 1) over (N, 64) latents: both passes over the
points run in HIP in float64 (said_metrics_weighted_sums / _scatter); the 1 / (N - 1) is applied here.  ``frechet_distance`` restates
pytorch-fid's ``calculate_frechet_distance`` on the host in float64 with ``scipy.linalg.sqrtm``, including its 1e-6 diagonal offset when
the product's square root is not finite and its error when the imaginary diagonal exceeds 1e-3.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np
from scipy import linalg

from . import _gmm


@dataclass
class Statistic:
    """Dataclass for the statistic"""

    mean: np.ndarray
    cov: np.ndarray


def get_statistic(data) -> Statistic:
    """Mean (64,) and covariance (64, 64) of the latents.  `data`: a list of (64,) arrays, an (N, 64) array, or an (N, 64) CUDA tensor."""
    x = _gmm.device_latents(data)
    n = x.shape[0]
    nk, mean, scatter = _gmm.moments(x)
    cov = scatter[0] / (n - 1) if n > 1 else np.full((x.shape[1], x.shape[1]), np.nan)   # np.cov of one sample: nan (ddof = 1)
    return Statistic(mean=mean[0], cov=cov)


def _sqrtm(a: np.ndarray) -> np.ndarray:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            return linalg.sqrtm(a, disp=False)[0]
        except TypeError:   # scipy without the disp argument
            return linalg.sqrtm(a)


def frechet_distance(mu1: np.ndarray, sigma1: np.ndarray, mu2: np.ndarray, sigma2: np.ndarray, eps: float = 1e-6) -> float:
    """d^2 = |mu1 - mu2|^2 + Tr(sigma1 + sigma2 - 2 sqrt(sigma1 sigma2)) of X1 ~ N(mu1, sigma1), X2 ~ N(mu2, sigma2)."""
    mu1, mu2 = np.atleast_1d(mu1).astype(np.float64), np.atleast_1d(mu2).astype(np.float64)
    sigma1, sigma2 = np.atleast_2d(sigma1).astype(np.float64), np.atleast_2d(sigma2).astype(np.float64)
    if mu1.shape != mu2.shape:
        raise ValueError("Training and test mean vectors have different lengths")
    if sigma1.shape != sigma2.shape:
        raise ValueError("Training and test covariances have different dimensions")
    diff = mu1 - mu2
    covmean = _sqrtm(sigma1.dot(sigma2))
    if not np.isfinite(covmean).all():
        print(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = _sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))
