"""Schedules of the BCVAE training (said/util/scheduler.py)."""
import numpy as np


def frange_cycle_linear(
    n_iter: int,
    start: float = 0.0,
    stop: float = 1.0,
    n_cycle: int = 10,
    ratio: float = 0.5,
) -> np.ndarray:
    """Linear cyclical schedule (https://github.com/haofuml/cyclical_annealing): `n_cycle` periods of `n_iter / n_cycle` values, each rising
    linearly from `start` for `ratio` of the period and then holding `stop`.

    Parameters
    ----------
    n_iter : int
        The number of iterations
    start : float
        Starting value, by default 0.0
    stop : float
        Ending value, by default 1.0
    n_cycle : int
        The number of cycles, by default 10
    ratio : float
        Ratio of the linear increasing part, by default 0.5

    Returns
    -------
    np.ndarray
        (n_iter,), scheduled values
    """
    values = np.ones(n_iter) * stop
    period = n_iter / n_cycle
    step = (stop - start) / (period * ratio)
    for c in range(n_cycle):
        v, i = start, 0
        while v <= stop and int(i + c * period) < n_iter:
            values[int(i + c * period)] = v
            v += step
            i += 1
    return values


def constant_with_warmup_lambda(num_warmup_steps: float):
    """The LR factor of optimizer step k (0-based) under diffusers' get_scheduler("constant_with_warmup"): k / max(1, W) while k < W, then 1."""

    def lr_lambda(current_step: int) -> float:
        if current_step < num_warmup_steps:
            return float(current_step) / float(max(1.0, num_warmup_steps))
        return 1.0

    return lr_lambda


def ema_decay(optimization_step: int, decay: float = 0.99) -> float:
    """The decay of EMA step n (1-based) of diffusers' EMAModel with its defaults (update_after_step 0, no warmup, min_decay 0):
    0 for n <= 1, else min((1 + s) / (10 + s), decay) with s = n - 1."""
    s = max(0, optimization_step - 1)
    if s <= 0:
        return 0.0
    return max(min((1 + s) / (10 + s), decay), 0.0)
