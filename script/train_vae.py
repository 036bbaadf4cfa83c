"""Train the BCVAE on an MI355X (the reference's script/train_vae.py, on said_amd.training.BCVAETrainer).

Command-line compatible with the reference (same flags, names and defaults; `--ema` keeps argparse's type=bool behaviour: any non-empty
string turns it on, `--ema ""` turns it off).  Differences:
- --coeffs_std_path defaults to "" (no std file ships with this repository); a path given reweights the losses by 1 / std, out of place.
- New flags: --seed (seeds Python, numpy and torch; unseeded by default) and --device.
- Logs go to <output_dir>/log.jsonl, one line per epoch with the reference's tensorboard keys.  The output directory is created.
- {epoch}.pth is written every --save_period epochs: the reference's state-dict layout (EMA parameters when --ema, live BatchNorm
  buffers), loadable by the reference's BCVAE and by said_amd.model.vae.BCVAE.
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from said_amd.training import BCVAETrainer, VAEWindowDataset, make_dataloaders  # noqa: E402
from said_amd.util.blendshape import load_blendshape_coeffs  # noqa: E402
from said_amd.util.scheduler import frange_cycle_linear  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Train the VAE for the blendshape coefficients using the BlendVOCA dataset (on an MI355X)")
    ap.add_argument("--coeffs_dir", type=str, default="../BlendVOCA/blendshape_coeffs", help="Directory of the data")
    ap.add_argument("--coeffs_std_path", type=str, default="", help="Path of the coeffs std data ('' = no reweighting)")
    ap.add_argument("--output_dir", type=str, default="../output", help="Directory of the outputs")
    ap.add_argument("--batch_size", type=int, default=8, help="Batch size at training")
    ap.add_argument("--epochs", type=int, default=100000, help="The number of epochs")
    ap.add_argument("--learning_rate", type=float, default=1e-4, help="Learning rate")
    ap.add_argument("--beta", type=float, default=1, help="Beta for beta-VAE")
    ap.add_argument("--beta_cycle", type=int, default=10, help="The number of cycles in beta schedule")
    ap.add_argument("--weight_vel", type=float, default=1.0, help="Weight for the velocity loss")
    ap.add_argument("--ema", type=bool, default=True, help="Use Exponential Moving Average of models weights")
    ap.add_argument("--ema_decay", type=float, default=0.99, help="Ema decay rate")
    ap.add_argument("--val_period", type=int, default=500, help="Period of validating model")
    ap.add_argument("--val_repeat", type=int, default=10, help="Number of repetitions of the validation dataset")
    ap.add_argument("--save_period", type=int, default=500, help="Period of saving model")
    ap.add_argument("--seed", type=int, default=None, help="seed of Python's random, numpy and torch (unseeded by default)")
    ap.add_argument("--device", type=str, default="cuda:0", help="MI355X to train on (there is no CPU path)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.seed is not None:
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    coeffs_std = None if args.coeffs_std_path == "" else load_blendshape_coeffs(args.coeffs_std_path)
    os.makedirs(args.output_dir, exist_ok=True)

    train_dataset = VAEWindowDataset(args.coeffs_dir, dataset_type="train")
    val_dataset = VAEWindowDataset(args.coeffs_dir, dataset_type="val")
    if len(train_dataset) == 0:
        raise SystemExit(f"no training sequences under {args.coeffs_dir} (expected <person id>/sentenceNN*.csv)")
    train_dataloader, val_dataloader = make_dataloaders(train_dataset, val_dataset, args.batch_size)

    num_training_steps = len(train_dataloader) * args.epochs
    trainer = BCVAETrainer(args.device, max_batch=args.batch_size, learning_rate=args.learning_rate, num_training_steps=num_training_steps,
                           ema=args.ema, ema_decay=args.ema_decay, std=coeffs_std)
    trainer.set_train_data(train_dataset)
    if len(val_dataset) > 0:
        trainer.set_val_data(val_dataset)
    beta_schedules = frange_cycle_linear(n_iter=args.epochs, stop=args.beta, n_cycle=args.beta_cycle)

    log_path = os.path.join(args.output_dir, "log.jsonl")
    with open(log_path, "a") as log:
        for epoch in range(1, args.epochs + 1):
            beta_epoch = float(beta_schedules[epoch - 1])
            train_losses = trainer.train_epoch(train_dataloader, beta=beta_epoch, weight_vel=args.weight_vel)
            logs = {
                "Train/Total": train_losses.total,
                "Train/Reconst": train_losses.reconst,
                "Train/Regular": train_losses.regularize,
                "Train/Velocity": train_losses.velocity,
                "Train/Beta": beta_epoch,
                "Train/Learning Rate": train_losses.lr,
            }
            if epoch % args.val_period == 0 and len(val_dataset) > 0:
                val_losses = trainer.validate_epoch(val_dataloader, beta=beta_epoch, weight_vel=args.weight_vel, num_repeat=args.val_repeat)
                logs["Val/Total"] = val_losses.total
                logs["Val/Reconst"] = val_losses.reconst
                logs["Val/Regular"] = val_losses.regularize
                logs["Val/Velocity"] = val_losses.velocity
            log.write(json.dumps({"epoch": epoch, **logs}) + "\n")
            log.flush()
            print(f"epoch {epoch}: " + ", ".join(f"{k}={v:.6g}" for k, v in logs.items()), flush=True)
            if epoch % args.save_period == 0:
                torch.save(trainer.state_dict(ema=args.ema), os.path.join(args.output_dir, f"{epoch}.pth"))
    trainer.close()


if __name__ == "__main__":
    main()
