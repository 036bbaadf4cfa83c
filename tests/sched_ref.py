"""CPU restatement of diffusers 0.19's DDPMScheduler and DPMSolverMultistepScheduler (the slice SAID.inference uses), written from that
version's published source independently of said_amd.scheduler: the tests compare the engine's tables, its elementwise steps and whole
loops against it.  Tensor ops are fp32 torch ops in the library's order; timesteps are numpy as there.  Not the oracle of the pinned
legs: like the DDIM leg (tests/golden/g9_*_scheduler_leg_unpinned.npz), these scheduler legs are unpinned (no diffusers here).
"""
import math
from typing import List, Optional

import numpy as np
import torch


def _betas(n: int = 1000, max_beta: float = 0.999) -> torch.Tensor:
    # betas_for_alpha_bar (squaredcos_cap_v2)
    def alpha_bar(t):
        return math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
    return torch.tensor([min(1 - alpha_bar((i + 1) / n) / alpha_bar(i / n), max_beta) for i in range(n)], dtype=torch.float32)


def dpm_timesteps(n: int, T: int = 1000) -> np.ndarray:
    """linspace(0, T - 1, n + 1).round()[::-1][:-1], duplicates removed in order of first appearance."""
    ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].astype(np.int64)
    out, seen = [], set()
    for t in ts:
        if int(t) not in seen:
            seen.add(int(t))
            out.append(int(t))
    return np.array(out, dtype=np.int64)


def leading_timesteps(n: int, T: int = 1000) -> np.ndarray:
    r = T // n
    return np.array([k * r for k in range(n)][::-1], dtype=np.int64)


class RefDDPM:
    def __init__(self, prediction_type: str = "epsilon", T: int = 1000):
        self.T, self.prediction_type = T, prediction_type
        self.betas = _betas(T)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.one = torch.tensor(1.0)
        self.init_noise_sigma = 1.0

    def set_timesteps(self, n: int):
        self.num_inference_steps = n
        self.timesteps = torch.from_numpy(leading_timesteps(n, self.T))

    def _prev(self, t: int) -> int:
        return t - self.T // self.num_inference_steps

    def row(self, t: int, t_next: Optional[int]) -> np.ndarray:
        prev_t = self._prev(t)
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        b_t, b_p = 1 - a_t, 1 - a_p
        cur_a = a_t / a_p
        cur_b = 1 - cur_a
        var = torch.clamp((1 - a_p) / (1 - a_t) * (1 - a_t / a_p), min=1e-20)
        r = np.zeros(8, np.float32)
        r[:5] = [float(a_t ** 0.5), float(b_t ** 0.5), float((a_p ** 0.5 * cur_b) / b_t), float(cur_a ** 0.5 * b_p / b_t),
                 float(var ** 0.5) if t > 0 else 0.0]
        r[5:] = _next_cols(self.alphas_cumprod, t_next) + [1.0]
        return r

    def step(self, model_output, t: int, sample, noise=None):
        prev_t = self._prev(t)
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        b_t, b_p = 1 - a_t, 1 - a_p
        cur_a = a_t / a_p
        cur_b = 1 - cur_a
        x0 = _x0(self.prediction_type, model_output, sample, a_t ** 0.5, b_t ** 0.5).clamp(-1.0, 1.0)
        c_x0 = (a_p ** (0.5) * cur_b) / b_t
        c_x = cur_a ** (0.5) * b_p / b_t
        prev = c_x0 * x0 + c_x * sample
        if t > 0:
            var = torch.clamp((1 - a_p) / (1 - a_t) * (1 - a_t / a_p), min=1e-20)
            prev = prev + (var ** 0.5) * noise
        return prev

    def add_noise(self, x, noise, t: int):
        a = self.alphas_cumprod[t]
        return a ** 0.5 * x + (1 - a) ** 0.5 * noise


class RefDPM:
    """DPM-Solver++(2M), midpoint, lower_order_final, no thresholding."""

    def __init__(self, prediction_type: str = "epsilon", T: int = 1000):
        self.T, self.prediction_type = T, prediction_type
        self.betas = _betas(T)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.alpha_t = torch.sqrt(self.alphas_cumprod)
        self.sigma_t = torch.sqrt(1 - self.alphas_cumprod)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self.init_noise_sigma = 1.0

    def set_timesteps(self, n: int):
        ts = dpm_timesteps(n, self.T)
        self.timesteps = torch.from_numpy(ts)
        self.num_inference_steps = len(ts)
        self.model_outputs: List[Optional[torch.Tensor]] = [None, None]
        self.lower_order_nums = 0

    def _index(self, t: int) -> int:
        return int((self.timesteps == t).nonzero()[0])

    def order_at(self, i: int, lower_order_nums: int) -> int:
        L = len(self.timesteps)
        final = i == L - 1 and L < 15
        return 1 if (lower_order_nums < 1 or final) else 2

    def row(self, i: int, order: int, t_next: Optional[int]) -> np.ndarray:
        ts = self.timesteps
        s0 = int(ts[i])
        t = 0 if i == len(ts) - 1 else int(ts[i + 1])
        h = self.lambda_t[t] - self.lambda_t[s0]
        r = np.zeros(8, np.float32)
        r[0], r[1] = float(self.alpha_t[s0]), float(self.sigma_t[s0])
        r[2] = float(self.sigma_t[t] / self.sigma_t[s0])
        r[3] = float(self.alpha_t[t] * (torch.exp(-h) - 1.0))
        if order == 2:
            h_0 = self.lambda_t[s0] - self.lambda_t[int(ts[i - 1])]
            r[4] = float(1.0 / (h_0 / h))
        r[5:] = _next_cols(self.alphas_cumprod, t_next) + [3.0 if order == 2 else 2.0]
        return r

    def step(self, model_output, timestep: int, sample):
        i = self._index(timestep)
        L = len(self.timesteps)
        prev_t = 0 if i == L - 1 else int(self.timesteps[i + 1])
        s0 = int(timestep)
        x0 = _x0(self.prediction_type, model_output, sample, self.alpha_t[s0], self.sigma_t[s0])
        self.model_outputs = [self.model_outputs[1], x0]
        order = self.order_at(i, self.lower_order_nums)
        lam_t, lam_s0 = self.lambda_t[prev_t], self.lambda_t[s0]
        alpha_t, sigma_t, sigma_s0 = self.alpha_t[prev_t], self.sigma_t[prev_t], self.sigma_t[s0]
        h = lam_t - lam_s0
        if order == 1:
            x = (sigma_t / sigma_s0) * sample - (alpha_t * (torch.exp(-h) - 1.0)) * x0
        else:
            s1 = int(self.timesteps[i - 1])
            m0, m1 = self.model_outputs[1], self.model_outputs[0]
            h_0 = lam_s0 - self.lambda_t[s1]
            r0 = h_0 / h
            D0, D1 = m0, (1.0 / r0) * (m0 - m1)
            x = (sigma_t / sigma_s0) * sample - (alpha_t * (torch.exp(-h) - 1.0)) * D0 - 0.5 * (alpha_t * (torch.exp(-h) - 1.0)) * D1
        if self.lower_order_nums < 2:
            self.lower_order_nums += 1
        return x

    def add_noise(self, x, noise, t: int):
        a = self.alphas_cumprod[t]
        return a ** 0.5 * x + (1 - a) ** 0.5 * noise


def _next_cols(ac, t_next):
    if t_next is None:
        return [1.0, 0.0]
    a = ac[t_next]
    return [float(a ** 0.5), float((1 - a) ** 0.5)]


def _x0(pred, m, x, a, s):
    if pred == "epsilon":
        return (x - s * m) / a
    if pred == "sample":
        return m
    return a * x - s * m


def make(name: str, prediction_type: str = "epsilon"):
    return {"ddpm": RefDDPM, "dpmsolver++": RefDPM}[name](prediction_type)


def inference(sd, waveform_processed, sched: str, *, init_latents, num_inference_steps, guidance_scale, guidance_rescale=0.0,
              prediction_type="epsilon", init_samples=None, mask=None, edit_noise=None, strength=1.0, step_noise=None,
              audio_embedding=None, fps=60):
    """diffusion.py:354-472 with the scheduler above in the noise_scheduler slot: the oracle's UNet, audio encoder and guidance.
    Returns (result, final latents)."""
    from oracle import pipeline as op
    from oracle import scheduler as osch
    from oracle import unet as ou
    sd_audio, sd_unet, null_cond = op.split_state_dict(sd)
    B, Ta = waveform_processed.shape
    do_cfg = guidance_scale > 1.0
    window = int(Ta / 16000 * fps)
    sch = make(sched, prediction_type)
    sch.set_timesteps(num_inference_steps)
    latents = (init_latents if init_samples is None else init_samples).clone() * sch.init_noise_sigma
    init_lat = latents.clone()
    init_t = min(int(num_inference_steps * strength), num_inference_steps)
    noise = None
    if init_samples is not None:
        noise = edit_noise
        latents = sch.add_noise(latents, noise, int(sch.timesteps[-init_t]))
    emb = audio_embedding if audio_embedding is not None else op.get_audio_embedding(sd_audio, waveform_processed, window)
    if do_cfg:
        emb = torch.cat([null_cond.repeat(B, emb.shape[1], 1), emb])
    t_start = num_inference_steps - init_t
    for idx, t in enumerate(sch.timesteps[t_start:]):
        x = torch.cat([latents] * 2) if do_cfg else latents
        pred = ou.unet1d_forward(sd_unet, x, t.repeat(x.shape[0]), emb)
        if do_cfg:
            e_u, e_c = pred.chunk(2)
            pred = e_c + guidance_scale * (e_c - e_u)
            if guidance_rescale > 0.0:
                pred = osch.rescale_noise_cfg(pred, e_c, guidance_rescale)
        if sched == "ddpm":
            latents = sch.step(pred, int(t), latents, None if step_noise is None else step_noise[idx])
        else:
            latents = sch.step(pred, int(t), latents)
        if init_samples is not None and mask is not None:
            noisy = init_lat
            nxt = t_start + idx + 1
            if nxt < num_inference_steps:
                noisy = sch.add_noise(init_lat, noise, int(sch.timesteps[nxt]))
            latents = noisy * mask + latents * (1 - mask)
    return latents.clamp(0, 1), latents
