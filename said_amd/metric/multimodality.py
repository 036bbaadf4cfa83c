"""Multimodality (said/metric/multimodality.py): the mean distance between aligned pairs of latents."""
from typing import List

import numpy as np
from numpy import linalg as LA


def multimodality(latents_subset1: List[np.ndarray], latents_subset2: List[np.ndarray]) -> float:
    """Mean of |l1_i - l2_i| over aligned lists of latent vectors; 0 when either is empty."""
    if len(latents_subset1) == 0 or len(latents_subset2) == 0:
        return 0
    return np.mean(LA.norm(np.array(latents_subset1) - np.array(latents_subset2), axis=1))
