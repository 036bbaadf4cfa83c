"""Median time of one denoiser training step on one MI355X (said_amd.training.UNetTrainer) beside torch-eager on the same GPU running the
restatement of the same step (tests/unet_train_ref.py: forward, objective, autograd backward, clip_grad_norm_, torch.optim.AdamW; no EMA).

    python scripts/bench_unet_train.py [--batch 8] [--frames 120 240] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from said_amd.training import UNetTrainer  # noqa: E402
from said_amd.training.unet import trainable_shapes  # noqa: E402
from said_amd.util.synth import said_state_dict  # noqa: E402
import unet_train_ref as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, nargs="+", default=[120, 240])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    dev = torch.device(a.device)
    sd = said_state_dict(num_w2v_layers=1)
    B = a.batch
    tr = UNetTrainer(sd, dev, max_batch=B, max_frames=max(a.frames), learning_rate=1e-5, num_warmup_steps=10)
    for T in a.frames:
        g = torch.Generator().manual_seed(T)
        coeffs, noise, audio = torch.rand(B, T, 32, generator=g), torch.randn(B, T, 32, generator=g), torch.randn(B, T, 768, generator=g)
        ts, cond = torch.randint(0, 1000, (B,), generator=g), [i % 4 != 0 for i in range(B)]
        audio_d = audio.to(dev)
        times = []
        for k in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            tr.step(coeffs, cond, audio_d, noise=noise, timesteps=ts, dropout_seed=k)   # reads the losses back: one sync per step
            times.append(time.perf_counter() - t0)
        hip_ms = 1e3 * statistics.median(times[a.warmup:])
        # torch eager, fp32, same GPU
        p = {k: sd[k].to(dev).requires_grad_(True) for k in trainable_shapes()}
        opt = torch.optim.AdamW(p.values(), lr=1e-5)
        masks = [m.to(dev, torch.float32) for m in ref.dropout_masks(1, B, T, 0.1)]
        c_d, n_d, ts_d, ac = coeffs.to(dev), noise.to(dev), ts.to(dev), tr.alphas_cumprod.to(dev)
        band_cond = torch.tensor(cond, device=dev)
        times = []
        for k in range(a.warmup + a.steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            noisy, answer = ref.add_noise(ac, c_d, n_d, ts_d, "epsilon", torch.float32)
            losses = ref.objective(ref.forward(p, noisy, ts_d, audio_d, band_cond, masks), answer)
            ref.total_loss(losses).backward()
            torch.nn.utils.clip_grad_norm_(p.values(), 1.0)
            opt.step()
            opt.zero_grad()
            float(losses[0])
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
        eager_ms = 1e3 * statistics.median(times[a.warmup:])
        print(json.dumps({"batch": B, "frames": T, "hip_step_ms": round(hip_ms, 3), "torch_eager_step_ms": round(eager_ms, 3),
                          "speedup": round(eager_ms / hip_ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
