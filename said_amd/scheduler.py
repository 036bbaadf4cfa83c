"""Host side of the noise schedulers: DDIM, DDPM and DPM-Solver++(2M).

Mirrors the slice of ``diffusers==0.19.*`` ``DDIMScheduler`` that the reference
touches (/root/reference/said/model/diffusion.py:100-104, 179, 247, 271-272,
361, 370, 378, 404, 413, 424-426, 441-443, 451-454): same constructor
arguments, ``config``, ``timesteps``, ``alphas_cumprod``, ``init_noise_sigma``,
``set_timesteps``, ``scale_model_input``, ``step``, ``add_noise``,
``get_velocity``.  Only the *tables* are computed here (fp32 torch ops on the
CPU, in that library's op order); every elementwise tensor update runs in the
HIP engine (``said_ddim_step`` / ``said_axpby`` / the fused loop).

``DDPMScheduler`` and ``DPMSolverMultistepScheduler`` restate the same library's
classes of those names with their 0.19 defaults, for the swappable
``noise_scheduler`` slot of the reference's ``SAID`` (diffusion.py:100-104).
Their rows carry a solver code in coefficient column 7 (``SAID_COEF_SOLVER``);
the update runs inside the same fused step (``said_solver_step`` on its own).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Union

import numpy as np
import torch

from . import _engine

NCOEF = _engine.NCOEF
COEF_SOLVER = _engine.COEF_SOLVER


def _betas_squaredcos_cap_v2(n: int, max_beta: float = 0.999) -> torch.Tensor:
    def alpha_bar(t: float) -> float:
        return math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2

    return torch.tensor([min(1 - alpha_bar((i + 1) / n) / alpha_bar(i / n), max_beta) for i in range(n)], dtype=torch.float32)


@dataclass
class DDIMSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: Optional[torch.Tensor] = None


class DDIMScheduler:
    """DDIM scheduler with diffusers-0.19 defaults: clip_sample=True (range 1.0),
    set_alpha_to_one=True, steps_offset=0, timestep_spacing="leading"."""

    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_schedule: str = "squaredcos_cap_v2",
                 prediction_type: str = "epsilon", **kwargs):
        if beta_schedule != "squaredcos_cap_v2":
            raise NotImplementedError(f"beta_schedule={beta_schedule!r}: the SAiD path only uses 'squaredcos_cap_v2'")
        if prediction_type not in _engine.PRED:
            raise ValueError(f"prediction_type must be one of {list(_engine.PRED)}")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_schedule=beta_schedule,
                                      prediction_type=prediction_type, clip_sample=True, clip_sample_range=1.0,
                                      set_alpha_to_one=True, steps_offset=0, timestep_spacing="leading", **kwargs)
        self.betas = _betas_squaredcos_cap_v2(num_train_timesteps)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0)
        self.init_noise_sigma = 1.0
        self.num_inference_steps: Optional[int] = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self._engine: Optional[_engine.Engine] = None  # attached by the owning SAID model

    # ---- tables -------------------------------------------------------------
    def set_timesteps(self, num_inference_steps: int, device: Union[str, torch.device, None] = None) -> None:
        if num_inference_steps > self.config.num_train_timesteps:
            raise ValueError("`num_inference_steps` cannot be larger than `num_train_timesteps`")
        self.num_inference_steps = num_inference_steps
        step_ratio = self.config.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64)
        ts += self.config.steps_offset
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def draws_step_noise(self, eta: float) -> bool:
        """Whether ``step`` adds fresh noise on every step (diffusion.py:441-443): DDIM only for eta > 0."""
        return eta > 0

    def _coef_row(self, timestep: int, eta: float, next_timestep: Optional[int]) -> np.ndarray:
        """One row of the engine's coefficient table (include/said_hip.h SAID_COEF_*),
        each entry a 0-dim fp32 tensor op in DDIMScheduler.step's order."""
        prev_t = timestep - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[timestep]
        a_p = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t = 1 - a_t
        b_p = 1 - a_p
        variance = (b_p / b_t) * (1 - a_t / a_p)
        std_dev_t = eta * variance ** (0.5)
        row = np.zeros(NCOEF, dtype=np.float32)
        row[0] = float(a_t ** (0.5))
        row[1] = float(b_t ** (0.5))
        row[2] = float(a_p ** (0.5))
        row[3] = float((1 - a_p - std_dev_t ** 2) ** (0.5))
        row[4] = float(std_dev_t)
        if next_timestep is None:
            row[5], row[6] = 1.0, 0.0
        else:
            a_n = self.alphas_cumprod[next_timestep]
            row[5] = float(a_n ** 0.5)
            row[6] = float((1 - a_n) ** 0.5)
        return row

    def coef_table(self, timesteps: np.ndarray, eta: float) -> np.ndarray:
        """Rows for consecutive loop steps; the mask-blend columns use the *next*
        loop timestep (diffusion.py:449-454), identity on the last step.

        One batched fp32 expression over all steps: every element goes through the same fp32 ops in the same
        order as ``_coef_row`` (0-dim tensor ops, DDIMScheduler.step's order), so the table is bit-identical to the
        row-wise form (tests/test_host_cpu.py asserts it) — and a 1000-step table costs ~0.2 ms of host time
        instead of ~25 ms, which a single-clip caller would otherwise pay before the first kernel."""
        n = len(timesteps)
        if n == 0:
            return np.zeros((0, NCOEF), np.float32)
        ts = torch.as_tensor(np.asarray(timesteps, dtype=np.int64))
        ac = self.alphas_cumprod
        prev = ts - self.config.num_train_timesteps // self.num_inference_steps
        a_t = ac[ts]
        a_p = torch.where(prev >= 0, ac[prev.clamp(min=0)], self.final_alpha_cumprod.to(ac.dtype))
        b_t = 1 - a_t
        b_p = 1 - a_p
        variance = (b_p / b_t) * (1 - a_t / a_p)
        std_dev_t = eta * variance ** (0.5)
        tab = torch.zeros(n, NCOEF, dtype=torch.float32)
        tab[:, 0] = a_t ** (0.5)
        tab[:, 1] = b_t ** (0.5)
        tab[:, 2] = a_p ** (0.5)
        tab[:, 3] = (1 - a_p - std_dev_t ** 2) ** (0.5)
        tab[:, 4] = std_dev_t
        tab[:, 5], tab[:, 6] = 1.0, 0.0
        if n > 1:
            a_n = ac[ts[1:]]
            tab[:-1, 5] = a_n ** 0.5
            tab[:-1, 6] = (1 - a_n) ** 0.5
        return tab.numpy()

    def coef_table_rowwise(self, timesteps: np.ndarray, eta: float) -> np.ndarray:
        """The same table built row by row with 0-dim tensor ops (reference form; used by the tests)."""
        n = len(timesteps)
        return np.stack([self._coef_row(int(timesteps[k]), eta, int(timesteps[k + 1]) if k + 1 < n else None)
                         for k in range(n)]) if n else np.zeros((0, NCOEF), np.float32)

    # ---- tensor updates (HIP engine) ------------------------------------------
    def _need_engine(self) -> _engine.Engine:
        if self._engine is None:
            raise _engine.EngineError("scheduler is not attached to a HIP engine (construct it through SAID_UNet1D on an MI355X)")
        return self._engine

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, eta: float = 0.0,
             use_clipped_model_output: bool = False, generator=None, variance_noise: Optional[torch.Tensor] = None,
             return_dict: bool = True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if use_clipped_model_output:
            raise NotImplementedError("use_clipped_model_output=True is not used by the SAiD path")
        row = self._coef_row(int(timestep), float(eta), None)
        noise = None
        if eta > 0:
            noise = variance_noise if variance_noise is not None else torch.randn(
                model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
        prev = self._need_engine().ddim_step(model_output, sample, row, self.config.prediction_type, step_noise=noise)
        return DDIMSchedulerOutput(prev_sample=prev) if return_dict else (prev,)

    def _sqrt_pair(self, timesteps: torch.Tensor):
        ts = torch.as_tensor(timesteps).to("cpu").reshape(-1)
        ac = self.alphas_cumprod
        sa = (ac[ts] ** 0.5).flatten()
        sb = ((1 - ac[ts]) ** 0.5).flatten()
        return sa.tolist(), sb.tolist()

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        sa, sb = self._sqrt_pair(timesteps)
        B = original_samples.shape[0]
        if len(sa) == 1 and B > 1:
            sa, sb = sa * B, sb * B
        return self._need_engine().axpby(sa, original_samples, sb, noise)

    def get_velocity(self, sample: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        sa, sb = self._sqrt_pair(timesteps)
        B = sample.shape[0]
        if len(sa) == 1 and B > 1:
            sa, sb = sa * B, sb * B
        return self._need_engine().axpby(sa, noise, [-v for v in sb], sample)


# ---------------------------------------------------------------------------------------------------------------------------------
# DDPM and DPM-Solver++ (diffusers 0.19).  Their tables are built row by row from 0-dim fp32 tensor ops in the library's own op order
# (a batched form could round torch.exp differently from the scalar one), so given the same model output the engine's update is
# bit-exact against a CPU restatement of the library.  The mask-blend columns 5 / 6 are add_noise(init, noise, t_next) as for DDIM.
# ---------------------------------------------------------------------------------------------------------------------------------
def _add_noise_cols(alphas_cumprod: torch.Tensor, row: np.ndarray, next_timestep: Optional[int]) -> None:
    if next_timestep is None:
        row[5], row[6] = 1.0, 0.0
    else:
        a_n = alphas_cumprod[next_timestep]
        row[5] = float(a_n ** 0.5)
        row[6] = float((1 - a_n) ** 0.5)


class _EngineScheduler:
    """What DDPM and DPM-Solver++ share with DDIMScheduler: the beta schedule, add_noise / get_velocity (the same formula in all
    three schedulers of diffusers 0.19) and the engine attachment."""

    order = 1

    def _init_common(self, num_train_timesteps: int, beta_schedule: str, prediction_type: str):
        if beta_schedule != "squaredcos_cap_v2":
            raise NotImplementedError(f"beta_schedule={beta_schedule!r}: the SAiD path only uses 'squaredcos_cap_v2'")
        if prediction_type not in _engine.PRED:
            raise ValueError(f"prediction_type must be one of {list(_engine.PRED)}")
        self.betas = _betas_squaredcos_cap_v2(num_train_timesteps)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.init_noise_sigma = 1.0
        self.num_inference_steps: Optional[int] = None
        self._engine: Optional[_engine.Engine] = None  # attached by the owning SAID model
        # Rows are a pure function of a few integers: kept, so that a repeated call (SAID.inference sets the timesteps afresh each time)
        # does not pay the 0-dim tensor ops again (~50 us per row: 50 ms before a 1000-step loop's first kernel).
        self._rows = {}

    def _cached_row(self, key, make) -> np.ndarray:
        row = self._rows.get(key)
        if row is None:
            row = self._rows[key] = make()
        return row.copy()

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def coef_table_rowwise(self, timesteps: np.ndarray, eta: float = 0.0) -> np.ndarray:
        return self.coef_table(timesteps, eta)

    _need_engine = DDIMScheduler._need_engine
    _sqrt_pair = DDIMScheduler._sqrt_pair
    add_noise = DDIMScheduler.add_noise
    get_velocity = DDIMScheduler.get_velocity


class DDPMScheduler(_EngineScheduler):
    """DDPM scheduler (diffusers 0.19 ``DDPMScheduler``) with that version's defaults: variance_type="fixed_small", clip_sample=True
    (range 1.0), timestep_spacing="leading", steps_offset=0, thresholding=False; alpha_prod_t_prev = 1 below t = 0.  ``step`` takes
    no ``eta`` (so the reference's loop passes none, diffusion.py:403-405) and draws noise on every step with t > 0.

    Row (SAID_COEF_SOLVER = 1): sqrt(alpha_prod_t), sqrt(1 - alpha_prod_t) (x0 from the model output), pred_original_sample_coeff,
    current_sample_coeff, std = _get_variance(t) ** 0.5 (0 at t = 0); prev = c_x0 * clip(x0) + c_x * x + std * z."""

    solver = "ddpm"

    def __init__(self, num_train_timesteps: int = 1000, beta_schedule: str = "squaredcos_cap_v2",
                 prediction_type: str = "epsilon", **kwargs):
        self._init_common(num_train_timesteps, beta_schedule, prediction_type)
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_schedule=beta_schedule, prediction_type=prediction_type,
                                      variance_type="fixed_small", clip_sample=True, clip_sample_range=1.0, thresholding=False,
                                      timestep_spacing="leading", steps_offset=0, **kwargs)
        self.one = torch.tensor(1.0)
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))

    def set_timesteps(self, num_inference_steps: int, device: Union[str, torch.device, None] = None) -> None:
        if num_inference_steps > self.config.num_train_timesteps:
            raise ValueError("`num_inference_steps` cannot be larger than `num_train_timesteps`")
        self.num_inference_steps = num_inference_steps
        step_ratio = self.config.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64)
        ts += self.config.steps_offset
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    def draws_step_noise(self, eta: float) -> bool:
        return True

    def previous_timestep(self, timestep: int) -> int:
        n = self.num_inference_steps if self.num_inference_steps else self.config.num_train_timesteps
        return timestep - self.config.num_train_timesteps // n

    def _get_variance(self, t: int) -> torch.Tensor:
        prev_t = self.previous_timestep(t)
        alpha_prod_t = self.alphas_cumprod[t]
        alpha_prod_t_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        current_beta_t = 1 - alpha_prod_t / alpha_prod_t_prev
        variance = (1 - alpha_prod_t_prev) / (1 - alpha_prod_t) * current_beta_t
        return torch.clamp(variance, min=1e-20)   # variance_type "fixed_small"

    def _coef_row(self, timestep: int, next_timestep: Optional[int]) -> np.ndarray:
        t = int(timestep)
        return self._cached_row((t, self.previous_timestep(t), next_timestep), lambda: self._make_row(t, next_timestep))

    def _make_row(self, t: int, next_timestep: Optional[int]) -> np.ndarray:
        prev_t = self.previous_timestep(t)
        alpha_prod_t = self.alphas_cumprod[t]
        alpha_prod_t_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        beta_prod_t = 1 - alpha_prod_t
        beta_prod_t_prev = 1 - alpha_prod_t_prev
        current_alpha_t = alpha_prod_t / alpha_prod_t_prev
        current_beta_t = 1 - current_alpha_t
        row = np.zeros(NCOEF, dtype=np.float32)
        row[0] = float(alpha_prod_t ** (0.5))
        row[1] = float(beta_prod_t ** (0.5))
        row[2] = float((alpha_prod_t_prev ** (0.5) * current_beta_t) / beta_prod_t)
        row[3] = float(current_alpha_t ** (0.5) * beta_prod_t_prev / beta_prod_t)
        row[4] = float(self._get_variance(t) ** 0.5) if t > 0 else 0.0
        _add_noise_cols(self.alphas_cumprod, row, next_timestep)
        row[COEF_SOLVER] = _engine.SOLVER["ddpm"]
        return row

    def coef_table(self, timesteps: np.ndarray, eta: float = 0.0) -> np.ndarray:
        """Rows for consecutive loop steps (``eta`` is ignored, as DDPMScheduler.step takes none); the mask-blend columns use the next loop
        timestep, identity on the last step."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        n = len(timesteps)
        return np.stack([self._coef_row(int(timesteps[k]), int(timesteps[k + 1]) if k + 1 < n else None)
                         for k in range(n)]) if n else np.zeros((0, NCOEF), np.float32)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None, return_dict: bool = True,
             variance_noise: Optional[torch.Tensor] = None):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        t = int(timestep)
        row = self._coef_row(t, None)
        noise = None
        if t > 0:
            noise = variance_noise if variance_noise is not None else torch.randn(
                model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
        prev = self._need_engine().solver_step(model_output, sample, row, self.config.prediction_type, step_noise=noise)
        return DDIMSchedulerOutput(prev_sample=prev) if return_dict else (prev,)


class DPMSolverMultistepScheduler(_EngineScheduler):
    """DPM-Solver++(2M) (diffusers 0.19 ``DPMSolverMultistepScheduler``) with that version's defaults: algorithm_type="dpmsolver++",
    solver_order=2, solver_type="midpoint", lower_order_final=True, thresholding=False, no Karras sigmas, timestep_spacing="linspace",
    lambda_min_clipped=-inf.  init_noise_sigma = 1, scale_model_input is the identity, no eta, no clipping of x0; the last step goes to
    timestep 0.  alpha_t = sqrt(alphas_cumprod), sigma_t = sqrt(1 - alphas_cumprod), lambda_t = log(alpha_t) - log(sigma_t) over the
    whole table, as in that version's constructor.

    Orders: the first step of every set_timesteps (so of every loop, strength < 1 included) is first order; the last is first order
    when the schedule has fewer than 15 timesteps (lower_order_final); every other step is second order.
    Rows (SAID_COEF_SOLVER = 2 / 3): alpha_s0, sigma_s0 (convert_model_output's x0), sigma_t / sigma_s0, alpha_t * (exp(-h) - 1), and for
    order 2 1 / r0 (multistep_dpm_solver_second_order_update)."""

    solver = "dpmsolver++"

    def __init__(self, num_train_timesteps: int = 1000, beta_schedule: str = "squaredcos_cap_v2",
                 prediction_type: str = "epsilon", **kwargs):
        self._init_common(num_train_timesteps, beta_schedule, prediction_type)
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_schedule=beta_schedule, prediction_type=prediction_type,
                                      solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                                      thresholding=False, use_karras_sigmas=False, lambda_min_clipped=-float("inf"),
                                      timestep_spacing="linspace", steps_offset=0, **kwargs)
        self.alpha_t = torch.sqrt(self.alphas_cumprod)
        self.sigma_t = torch.sqrt(1 - self.alphas_cumprod)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self.timesteps = torch.from_numpy(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy())
        self.lower_order_nums = 0
        self._x0_hist: Optional[torch.Tensor] = None   # step(): the previous step's x0 on the device

    def set_timesteps(self, num_inference_steps: int, device: Union[str, torch.device, None] = None) -> None:
        # lambda_min_clipped = -inf: the clipped index is 0 and the last timestep num_train_timesteps
        last_timestep = self.config.num_train_timesteps
        ts = np.linspace(0, last_timestep - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        _, unique_indices = np.unique(ts, return_index=True)   # duplicates when num_inference_steps >= num_train_timesteps
        ts = ts[np.sort(unique_indices)]
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)
        self.num_inference_steps = len(ts)
        self.lower_order_nums = 0
        self._x0_hist = None

    def draws_step_noise(self, eta: float) -> bool:
        return False

    def step_orders(self, start: int = 0) -> list:
        """Solver order of each step of a loop over timesteps[start:] that begins with an empty history."""
        L = len(self.timesteps)
        final_low = self.config.lower_order_final and L < 15
        return [1 if (k == start or (k == L - 1 and final_low)) else 2 for k in range(start, L)]

    def _coef_row(self, step_index: int, order: int, next_timestep: Optional[int]) -> np.ndarray:
        ts = self.timesteps
        s0 = int(ts[step_index])
        t = 0 if step_index == len(ts) - 1 else int(ts[step_index + 1])
        s1 = int(ts[step_index - 1]) if order == 2 else None
        return self._cached_row((s0, t, s1, next_timestep), lambda: self._make_row(s0, t, s1, next_timestep))

    def _make_row(self, s0: int, t: int, s1: Optional[int], next_timestep: Optional[int]) -> np.ndarray:
        order = 1 if s1 is None else 2
        lambda_t, lambda_s0 = self.lambda_t[t], self.lambda_t[s0]
        alpha_t, sigma_t, sigma_s0 = self.alpha_t[t], self.sigma_t[t], self.sigma_t[s0]
        h = lambda_t - lambda_s0
        row = np.zeros(NCOEF, dtype=np.float32)
        row[0] = float(self.alpha_t[s0])
        row[1] = float(self.sigma_t[s0])
        row[2] = float(sigma_t / sigma_s0)
        row[3] = float(alpha_t * (torch.exp(-h) - 1.0))
        if order == 2:
            lambda_s1 = self.lambda_t[s1]
            h_0 = lambda_s0 - lambda_s1
            r0 = h_0 / h
            row[4] = float(1.0 / r0)
        _add_noise_cols(self.alphas_cumprod, row, next_timestep)
        row[COEF_SOLVER] = _engine.SOLVER["dpm2" if order == 2 else "dpm1"]
        return row

    def coef_table(self, timesteps: np.ndarray, eta: float = 0.0) -> np.ndarray:
        """Rows for a loop over ``timesteps``, which must be a suffix of ``self.timesteps`` (SAID.inference's timesteps[t_start:]); ``eta``
        is ignored (DPMSolverMultistepScheduler.step takes none).  Mask-blend columns: next loop timestep, identity on the last step."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        ts = np.asarray(timesteps, dtype=np.int64)
        n, L = len(ts), len(self.timesteps)
        if n == 0:
            return np.zeros((0, NCOEF), np.float32)
        start = L - n
        if start < 0 or not np.array_equal(self.timesteps[start:].cpu().numpy(), ts):
            raise ValueError("DPMSolverMultistepScheduler.coef_table: timesteps must be a suffix of the scheduler's timesteps")
        orders = self.step_orders(start)
        return np.stack([self._coef_row(start + k, orders[k], int(ts[k + 1]) if k + 1 < n else None) for k in range(n)])

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None, return_dict: bool = True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        L = len(self.timesteps)
        idx = (self.timesteps.cpu() == int(timestep)).nonzero()
        step_index = L - 1 if len(idx) == 0 else int(idx[0])
        final_low = step_index == L - 1 and self.config.lower_order_final and L < 15
        order = 1 if (self.lower_order_nums < 1 or final_low) else 2
        if self._x0_hist is None or self._x0_hist.shape != sample.shape or self._x0_hist.device != sample.device:
            if order == 2:
                raise ValueError("DPMSolverMultistepScheduler.step: no previous model output for a second-order step")
            self._x0_hist = torch.empty(sample.shape, device=sample.device, dtype=torch.float32)
        row = self._coef_row(step_index, order, None)
        prev = self._need_engine().solver_step(model_output, sample, row, self.config.prediction_type, x0_hist=self._x0_hist)
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        return DDIMSchedulerOutput(prev_sample=prev) if return_dict else (prev,)


SCHEDULERS = {"ddim": DDIMScheduler, "ddpm": DDPMScheduler, "dpmsolver++": DPMSolverMultistepScheduler}


def check_engine_scheduler(scheduler) -> None:
    """The engine runs the tables of the schedulers above only: a foreign object (a diffusers instance, say) is refused."""
    if not isinstance(scheduler, tuple(SCHEDULERS.values())):
        raise TypeError(f"noise_scheduler {type(scheduler).__module__}.{type(scheduler).__name__} is not supported by the HIP engine: use "
                        "said_amd.scheduler.DDIMScheduler, DDPMScheduler or DPMSolverMultistepScheduler")
