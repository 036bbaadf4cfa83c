"""Median time of one denoiser training step on one MI355X (said_amd.training.UNetTrainer) beside torch-eager on the same GPU running the
restatement of the same step (tests/unet_train_ref.py: forward, objective, autograd backward, clip_grad_norm_, torch.optim.AdamW; no EMA).

    python scripts/bench_unet_train.py [--batch 8] [--frames 120 240] [--steps 20] [--warmup 5] [--feature_dim -1] [--audio_encoder_mode eval|train]

--feature_dim F > 0 trains SAID_UNet1D(feature_dim=F): the trainable nn.Linear(768, F) in front of an F-wide context, on both sides (the eager
side through tests/unet_train_proj_ref.py, which applies the same nn.Linear and the same select).

With --audio_encoder_mode the line also carries what the frozen audio encoder (twelve layers, clips of frames / 60 seconds) adds to a step of
script/train.py: `encode_eval_ms` and, in mode `train`, `encode_train_ms` (Wav2Vec2's train mode: SpecAugment spans, dropouts, LayerDrop off so
that all twelve layers run) — device-event medians, the two modes alternating in one loop — and `step_with_encode_ms`, the host time of encode
(in the chosen mode, draws included) plus step.
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
from said_amd.util.synth import fill_tensor, said_state_dict  # noqa: E402
import unet_train_proj_ref as pref  # noqa: E402
import unet_train_ref as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, nargs="+", default=[120, 240])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--feature_dim", type=int, default=-1, help="> 0: train the audio_proj_layer nn.Linear(768, F) and an F-wide context")
    ap.add_argument("--audio_encoder_mode", choices=["eval", "train"], default=None, help="also time the twelve-layer audio encoder, in eval mode and (train) in train mode")
    a = ap.parse_args()
    dev = torch.device(a.device)
    fd = a.feature_dim if a.feature_dim > 0 else -1
    sd = said_state_dict(num_w2v_layers=1, ctx_dim=fd if fd > 0 else 768)
    if fd > 0:
        sd["audio_proj_layer.weight"], sd["audio_proj_layer.bias"] = fill_tensor("audio_proj_layer.weight", (fd, 768)), fill_tensor("audio_proj_layer.bias", (fd,))
    B = a.batch
    tr = UNetTrainer(sd, dev, max_batch=B, max_frames=max(a.frames), learning_rate=1e-5, num_warmup_steps=10, feature_dim=fd)
    enc = None
    if a.audio_encoder_mode:
        from said_amd.model.diffusion import SAID_UNet1D
        from said_amd.model.wav2vec2 import AudioTrainConfig, draw_audio_train
        from said_amd.util.synth import synth_waveform
        enc = SAID_UNet1D()   # the frozen encoder alone: the trainer takes its (B, T, 768) output whatever --feature_dim is
        enc.load_state_dict(said_state_dict(), strict=True)
        enc.to(dev)
        cfg = AudioTrainConfig(layerdrop=0.0)   # every layer runs: the time does not depend on the draw
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
        p = {k: sd[k].to(dev).requires_grad_(True) for k in trainable_shapes(fd)}
        opt = torch.optim.AdamW(p.values(), lr=1e-5)
        masks = [m.to(dev, torch.float32) for m in ref.dropout_masks(1, B, T, 0.1)]
        c_d, n_d, ts_d, ac = coeffs.to(dev), noise.to(dev), ts.to(dev), tr.alphas_cumprod.to(dev)
        band_cond = torch.tensor(cond, device=dev)
        times = []
        for k in range(a.warmup + a.steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            noisy, answer = ref.add_noise(ac, c_d, n_d, ts_d, "epsilon", torch.float32)
            losses = ref.objective(pref.forward(p, noisy, ts_d, audio_d, band_cond, masks), answer)
            ref.total_loss(losses).backward()
            torch.nn.utils.clip_grad_norm_(p.values(), 1.0)
            opt.step()
            opt.zero_grad()
            float(losses[0])
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
        eager_ms = 1e3 * statistics.median(times[a.warmup:])
        line = {"batch": B, "frames": T, "feature_dim": fd, "hip_step_ms": round(hip_ms, 3), "torch_eager_step_ms": round(eager_ms, 3), "speedup": round(eager_ms / hip_ms, 3)}
        if enc is not None:
            wave = enc.process_audio([synth_waveform(i, 16000 * T // 60).numpy() for i in range(B)]).to(dev)
            train = a.audio_encoder_mode == "train"

            def encode(in_train_mode):
                draws = draw_audio_train(cfg, B, T, 12) if in_train_mode else None
                return enc.get_audio_embedding(wave, T, train_draws=draws, train_cfg=cfg)

            ev = {False: [], True: []}
            for k in range(a.warmup + a.steps):
                for m in ((False, True) if train else (False,)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    encode(m)
                    e1.record()
                    torch.cuda.synchronize(dev)
                    ev[m].append(e0.elapsed_time(e1))
            line["encode_eval_ms"] = round(statistics.median(ev[False][a.warmup:]), 3)
            if train:
                line["encode_train_ms"] = round(statistics.median(ev[True][a.warmup:]), 3)
            times = []
            for k in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                tr.step(coeffs, cond, encode(train), noise=noise, timesteps=ts, dropout_seed=k)
                times.append(time.perf_counter() - t0)
            line["audio_encoder_mode"] = a.audio_encoder_mode
            line["step_with_encode_ms"] = round(1e3 * statistics.median(times[a.warmup:]), 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
