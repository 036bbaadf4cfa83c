"""Train the SAID_UNet1D denoiser on an MI355X (the reference's script/train.py, on said_amd.training.UNetTrainer).

Command-line compatible with the reference (same flags, names and defaults; `--ema` keeps argparse's type=bool behaviour).  Differences:
- The frozen Wav2Vec2 encoder comes from --audio_encoder_weights: a state dict holding `audio_encoder.*` (a SAID_UNet1D checkpoint will
  do), or 'synthetic' for the seeded test weights.  The reference downloads facebook/wav2vec2-base-960h; nothing is downloaded here.
- --audio_encoder_mode {eval,train}: how that frozen encoder runs during the training epoch.  'eval' (the default: the behaviour and, for a
  given --seed, the logs of every earlier version) runs it as in inference.  'train' reproduces the reference, which calls
  said_model.train() before its epoch and so feeds the denoiser conditioning that went through Wav2Vec2's SpecAugment time masking,
  dropouts and LayerDrop (wav2vec2-base-960h's published config values).  Validation runs in eval mode either way.
- --unet_feature_dim F > 0 trains the extra audio_proj_layer = nn.Linear(768, F) inside the HIP step, with the rest: the
  model built here serves only as the frozen encoder, its own audio_proj_layer is never read.  F must be a multiple of 16, at most 1024:
  the inference engine, which runs that encoder and later the checkpoint, takes such context widths only.
- --finetune_audio_encoder trains the Wav2Vec2 transformer (feature projection, positional convolution, every transformer layer of the
  loaded encoder) together with the denoiser in the same HIP step, with the convolutional feature extractor frozen: the reference's
  commented `said_model.audio_encoder.freeze_feature_encoder()` variant, the paper's "finetune_wav2vec" ablation.
  --audio_encoder_mode keeps its meaning: 'train' gives the encoder its masks, dropouts and LayerDrop, 'eval' none.  <epoch>.pth then holds
  the trained audio_encoder.* tensors.  Off by default; without it nothing changes.
- New flags: --seed, --device.  Logs go to stdout and to <output_dir>/log.csv (the reference's TensorBoard keys as columns).
- <output_dir>/<epoch>.pth is SAID_UNet1D's state dict, written between EMA copy_to and restore as in the reference.
"""
import argparse
import csv
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from said_amd.model.diffusion import SAID_UNet1D  # noqa: E402
from said_amd.model.wav2vec2 import AudioTrainConfig  # noqa: E402
from said_amd.training import TrainWindowDataset, UNetTrainer, ValWindowDataset, make_unet_dataloaders, unet_init_state_dict  # noqa: E402
from said_amd.util.blendshape import load_blendshape_coeffs  # noqa: E402

COLUMNS = ["epoch", "Train/Total Loss", "Train/Predict Loss", "Train/Velocity Loss", "Train/Vertex Loss", "Train/Learning Rate",
           "Validation/Total Loss", "Validation/Predict Loss", "Validation/Velocity Loss", "Validation/Vertex Loss"]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Train the SAiD model using BlendVOCA dataset (on an MI355X)")
    ap.add_argument("--audio_dir", type=str, default="../BlendVOCA/audio", help="Directory of the audio data")
    ap.add_argument("--coeffs_dir", type=str, default="../BlendVOCA/blendshape_coeffs", help="Directory of the blendshape coefficients data")
    ap.add_argument("--coeffs_std_path", type=str, default="", help="Path of the coeffs std data")
    ap.add_argument("--blendshape_residuals_path", type=str, default="", help="Path of the blendshape residuals")
    ap.add_argument("--landmarks_path", type=str, default="", help="Path of the landmarks data")
    ap.add_argument("--output_dir", type=str, default="../output", help="Directory of the outputs")
    ap.add_argument("--prediction_type", type=str, default="epsilon", help="'epsilon', 'sample', or 'v_prediction'")
    ap.add_argument("--window_size_min", type=int, default=120, help="Minimum window size of the blendshape coefficients sequence at training")
    ap.add_argument("--batch_size", type=int, default=8, help="Batch size at training")
    ap.add_argument("--epochs", type=int, default=100000, help="The number of epochs")
    ap.add_argument("--num_warmup_epochs", type=int, default=5000, help="The number of warmup epochs")
    ap.add_argument("--num_workers", type=int, default=0, help="The number of workers")
    ap.add_argument("--learning_rate", type=float, default=1e-5, help="Learning rate")
    ap.add_argument("--uncond_prob", type=float, default=0.1, help="Unconditional probability of waveform (for classifier-free guidance)")
    ap.add_argument("--unet_feature_dim", type=int, default=-1, help="Dimension of the latent feature of the UNet")
    ap.add_argument("--weight_vel", type=float, default=1.0, help="Weight for the velocity loss")
    ap.add_argument("--weight_vertex", type=float, default=0.02, help="Weight for the vertex loss")
    ap.add_argument("--ema", type=bool, default=True, help="Use Exponential Moving Average of models weights")
    ap.add_argument("--ema_decay", type=float, default=0.9999, help="Ema decay rate")
    ap.add_argument("--val_period", type=int, default=200, help="Period of validating model")
    ap.add_argument("--val_repeat", type=int, default=50, help="Number of repetition of val dataset")
    ap.add_argument("--save_period", type=int, default=200, help="Period of saving model")
    ap.add_argument("--audio_encoder_weights", type=str, default="../BlendVOCA/SAiD.pth",
                    help="state dict holding audio_encoder.* (the frozen Wav2Vec2), or 'synthetic' for the seeded test weights")
    ap.add_argument("--audio_encoder_mode", type=str, default="eval", choices=["eval", "train"],
                    help="the frozen audio encoder during training: 'eval' as in inference, 'train' as the reference leaves it (SpecAugment, dropout, LayerDrop)")
    ap.add_argument("--finetune_audio_encoder", action="store_true",
                    help="train the Wav2Vec2 transformer with the denoiser (the feature extractor stays frozen)")
    ap.add_argument("--encoder_products", type=str, default=None, choices=["fp32", "split_fp16"],
                    help="with --finetune_audio_encoder: the arithmetic of the encoder's dense products: 'fp32' (the default) or 'split_fp16' "
                         "(split-fp16 operands, 22 significand bits, fp32 accumulation: faster)")
    ap.add_argument("--seed", type=int, default=None, help="seed of Python's random, numpy and torch (unseeded by default)")
    ap.add_argument("--device", type=str, default="cuda:0", help="MI355X to train on (there is no CPU path)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.unet_feature_dim > 0 and (args.unet_feature_dim % 16 or args.unet_feature_dim > 1024):
        raise SystemExit(f"--unet_feature_dim {args.unet_feature_dim}: must be a multiple of 16 up to 1024 (the context widths SAID_UNet1D's engine and the trainer take)")
    if args.encoder_products is not None and not args.finetune_audio_encoder:
        raise SystemExit("--encoder_products: needs --finetune_audio_encoder (the frozen encoder's products are not the trainer's)")
    if args.seed is not None:
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    coeffs_std = None if args.coeffs_std_path == "" else load_blendshape_coeffs(args.coeffs_std_path)
    os.makedirs(args.output_dir, exist_ok=True)

    if args.audio_encoder_weights == "synthetic":
        from said_amd.util import synth
        given = synth.said_state_dict()
    else:
        given = torch.load(args.audio_encoder_weights, map_location="cpu")
    state = {k: v for k, v in given.items() if k.startswith("audio_encoder.")}
    if not state:
        raise SystemExit(f"{args.audio_encoder_weights} holds no audio_encoder.* tensors")
    state.update(unet_init_state_dict(args.unet_feature_dim))
    model = SAID_UNet1D(feature_dim=args.unet_feature_dim, prediction_type=args.prediction_type)
    model.load_state_dict(state, strict=True)
    model.to(args.device)

    kw = dict(audio_dir=args.audio_dir, blendshape_coeffs_dir=args.coeffs_dir, blendshape_deltas_path=args.blendshape_residuals_path or None,
              landmarks_path=args.landmarks_path or None, sampling_rate=model.sampling_rate, uncond_prob=args.uncond_prob)
    train_dataset = TrainWindowDataset(window_size_min=args.window_size_min, **kw)
    val_dataset = ValWindowDataset(**kw)
    if len(train_dataset) == 0:
        raise SystemExit(f"no training data under {args.audio_dir} / {args.coeffs_dir}")
    train_dataloader, val_dataloader = make_unet_dataloaders(train_dataset, val_dataset, args.batch_size, args.num_workers)
    max_frames = max([c.shape[0] for _, c, _ in train_dataset.data + val_dataset.data])
    trainer = UNetTrainer(state, args.device, max_batch=args.batch_size, max_frames=max_frames, learning_rate=args.learning_rate,
                          num_warmup_steps=len(train_dataloader) * args.num_warmup_epochs, ema=args.ema, ema_decay=args.ema_decay, std=coeffs_std,
                          prediction_type=args.prediction_type, feature_dim=args.unet_feature_dim,
                          finetune_audio_layers=model.audio_config.num_hidden_layers if args.finetune_audio_encoder else 0,
                          encoder_products=args.encoder_products)

    audio_train = AudioTrainConfig() if args.audio_encoder_mode == "train" else None
    with open(os.path.join(args.output_dir, "log.csv"), "a", newline="") as f:
        log = csv.DictWriter(f, fieldnames=COLUMNS)
        if f.tell() == 0:
            log.writeheader()
        for epoch in range(1, args.epochs + 1):
            tl = trainer.train_epoch(model, train_dataloader, args.weight_vel, args.weight_vertex, audio_train=audio_train)
            logs = {"epoch": epoch, "Train/Total Loss": tl.total, "Train/Predict Loss": tl.predict, "Train/Velocity Loss": tl.velocity,
                    "Train/Vertex Loss": tl.vertex, "Train/Learning Rate": tl.lr}
            if epoch % args.val_period == 0 and len(val_dataset) > 0:
                if args.ema:
                    trainer.ema_store()
                    trainer.ema_copy_to()
                vl = trainer.validate(model, val_dataloader, args.weight_vel, args.weight_vertex, num_repeat=args.val_repeat)
                logs.update({"Validation/Total Loss": vl.total, "Validation/Predict Loss": vl.predict, "Validation/Velocity Loss": vl.velocity,
                             "Validation/Vertex Loss": vl.vertex})
                if args.ema:
                    trainer.ema_restore()
            log.writerow(logs)
            f.flush()
            print(", ".join(f"{k}={v:.6g}" if isinstance(v, float) else f"{k}={v}" for k, v in logs.items()), flush=True)
            if epoch % args.save_period == 0:
                if args.ema:
                    trainer.ema_store()
                    trainer.ema_copy_to()
                torch.save(trainer.state_dict(), os.path.join(args.output_dir, f"{epoch}.pth"))
                if args.ema:
                    trainer.ema_restore()
    trainer.close()


if __name__ == "__main__":
    main()
