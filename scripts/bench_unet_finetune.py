"""Median time of one denoiser training step that fine-tunes the twelve-layer Wav2Vec2 transformer on one MI355X
(UNetTrainer(finetune_audio_layers=12), train mode: SpecAugment spans, the four dropouts, LayerDrop off so that all twelve layers run) beside

- the frozen-encoder step of scripts/bench_unet_train.py at the same shapes (the audio embedding given), and the same step with the frozen
  encoder's train-mode forward in front of it, as script/train.py --audio_encoder_mode train runs it: what fine-tuning adds;
- torch eager on the same GPU running the fp32 restatement of the fine-tuning step (tests/audio_ft_ref.py: encoder forward, UNet forward,
  objective, autograd backward, clip_grad_norm_, torch.optim.AdamW; no EMA).  The eager side runs the encoder without its dropout masks (the
  restatement draws them with numpy on the host, which is no part of a step's GPU time): fewer operations than the HIP side runs.

    python scripts/bench_unet_finetune.py [--batch 8] [--frames 120 240] [--windows 5] [--steps 10] [--warmup 5] [--layers 12]
                                          [--products fp32 split_fp16] [--baseline_lib PATH]

--products: the arithmetic of the encoder's dense products (UNetTrainer(encoder_products=...)) that the fine-tuning step is
timed in: finetune_step_ms is the fp32 one, finetune_step_split_fp16_ms the split-fp16 one, on one context switched between the windows.
--baseline_lib: a libsaid_hip.so built from another commit; its fine-tuning step (fp32) is timed beside as baseline_finetune_step_ms.

Every figure is the median over --windows timed windows of --steps steps each (host clock around work that ends in a device synchronise),
the sides alternating window by window.  One JSON line per frame count.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from said_amd import _engine  # noqa: E402
from said_amd.model.diffusion import SAID_UNet1D  # noqa: E402
from said_amd.model.wav2vec2 import AudioConfig, AudioTrainConfig, draw_audio_train  # noqa: E402
from said_amd.training import UNetTrainer, trainable_shapes  # noqa: E402
from said_amd.util.synth import said_state_dict, synth_waveform  # noqa: E402
import audio_ft_ref as aft  # noqa: E402
import unet_train_ref as ref  # noqa: E402


def trainer_on_library(path, *args, **kw):
    """A UNetTrainer whose context lives in another build of the library; this build's groups must be bound already."""
    lib = ctypes.CDLL(path)
    for group in ("core", "unet_train", "unet_finetune"):
        _engine._bind(lib, group)
    mine, _engine._lib = _engine._lib, lib
    try:
        return UNetTrainer(*args, **kw)
    finally:
        _engine._lib = mine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, nargs="+", default=[120, 240])
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--products", nargs="+", default=["fp32", "split_fp16"], choices=sorted(_engine.ENCODER_PRODUCTS))
    ap.add_argument("--baseline_lib", default=None)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    dev = torch.device(a.device)
    B, L = a.batch, a.layers
    sd = said_state_dict(num_w2v_layers=L)
    ft = UNetTrainer(sd, dev, max_batch=B, max_frames=max(a.frames), learning_rate=1e-5, num_warmup_steps=10, finetune_audio_layers=L)
    frozen = UNetTrainer(sd, dev, max_batch=B, max_frames=max(a.frames), learning_rate=1e-5, num_warmup_steps=10)
    base = None
    if a.baseline_lib:
        base = trainer_on_library(a.baseline_lib, sd, dev, max_batch=B, max_frames=max(a.frames), learning_rate=1e-5, num_warmup_steps=10,
                                  finetune_audio_layers=L)
    model = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=L))
    model.load_state_dict(sd, strict=True)
    model.to(dev)
    cfg = AudioTrainConfig(layerdrop=0.0)   # every layer runs: the time does not depend on the draw
    p = {k: sd[k].to(dev).requires_grad_(True) for k in trainable_shapes(-1, L)}
    opt = torch.optim.AdamW(p.values(), lr=1e-5)
    for T in a.frames:
        g = torch.Generator().manual_seed(T)
        coeffs, noise = torch.rand(B, T, 32, generator=g), torch.randn(B, T, 32, generator=g)
        ts, cond = torch.randint(0, 1000, (B,), generator=g), [i % 4 != 0 for i in range(B)]
        wave = model.process_audio([synth_waveform(i, 16000 * T // 60).numpy() for i in range(B)]).to(dev)
        feats, audio = model.get_audio_features(wave, T), model.get_audio_embedding(wave, T)
        masks = [m.to(dev, torch.float32) for m in ref.dropout_masks(1, B, T, 0.1)]
        c_d, n_d, ts_d, ac, cond_d = coeffs.to(dev), noise.to(dev), ts.to(dev), ft.alphas_cumprod.to(dev), torch.tensor(cond, device=dev)
        count = [0]

        def ft_step(tr=ft, products="fp32"):
            count[0] += 1
            if tr is ft and ft.eng.encoder_products() != products:
                ft.eng.set_encoder_products(products)
            tr.step(coeffs, cond, feats, noise=noise, timesteps=ts, dropout_seed=count[0], audio_draws=draw_audio_train(cfg, B, T, L), audio_cfg=cfg)

        def frozen_step():
            count[0] += 1
            frozen.step(coeffs, cond, audio, noise=noise, timesteps=ts, dropout_seed=count[0])

        def frozen_encode_step():
            count[0] += 1
            emb = model.get_audio_embedding(wave, T, train_draws=draw_audio_train(cfg, B, T, L), train_cfg=cfg)
            frozen.step(coeffs, cond, emb, noise=noise, timesteps=ts, dropout_seed=count[0])

        def eager_step():
            noisy, answer = ref.add_noise(ac, c_d, n_d, ts_d, "epsilon", torch.float32)
            losses = ref.objective(aft.forward(p, noisy, ts_d, feats, cond_d, masks), answer)
            ref.total_loss(losses).backward()
            torch.nn.utils.clip_grad_norm_(p.values(), 1.0)
            opt.step()
            opt.zero_grad()
            float(losses[0])

        sides = {}
        if base is not None:
            sides["baseline_finetune_step_ms"] = lambda: ft_step(base)
        for mode in a.products:
            sides["finetune_step_ms" if mode == "fp32" else f"finetune_step_{mode}_ms"] = lambda mode=mode: ft_step(ft, mode)
        sides.update({"frozen_step_ms": frozen_step, "frozen_step_with_encode_ms": frozen_encode_step, "torch_eager_step_ms": eager_step})
        for f in sides.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize(dev)
        times = {k: [] for k in sides}
        for _ in range(a.windows):
            for k, f in sides.items():   # the steps read a loss back: each ends in a device synchronise
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    f()
                torch.cuda.synchronize(dev)
                times[k].append(1e3 * (time.perf_counter() - t0) / a.steps)
        line = {"batch": B, "frames": T, "layers": L, "windows": a.windows, "steps": a.steps}
        line.update({k: round(statistics.median(v), 3) for k, v in times.items()})
        line.update({k.replace("_ms", "_spread_ms"): [round(min(v), 3), round(max(v), 3)] for k, v in times.items()})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
