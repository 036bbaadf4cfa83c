"""Reconstruct blendshape coefficients with the BCVAE on an MI355X: CSV -> encode -> (sample) -> decode -> CSV.

Command-line compatible with the reference's script/inference_vae.py (same flags; `type=bool` flags keep argparse's
behaviour there: any non-empty string turns them on, `--use_noise ""` turns the noise off).  Differences: --weights_path
is required (no VAE checkpoint ships with this repository; `synthetic` selects the seeded test weights), the first 120
frames must exist, and there is no CPU path (`--device cpu` fails).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _common  # noqa: E402
from said_amd.model.vae import BCVAE  # noqa: E402
from said_amd.util.blendshape import (  # noqa: E402
    DEFAULT_BLENDSHAPE_CLASSES,
    load_blendshape_coeffs,
    save_blendshape_coeffs,
    save_blendshape_coeffs_image,
)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Reconstruct the blendshape coefficients using VAE (on an MI355X)")
    ap.add_argument("--weights_path", type=str, required=True, help="BCVAE state dict (vae.pth layout), or 'synthetic' for the seeded test weights")
    ap.add_argument("--blendshape_coeffs_path", type=str, default="../BlendVOCA/blendshape_coeffs/FaceTalk_170731_00024_TA/sentence01.csv",
                    help="input blendshape coefficients (CSV), at least 120 frames")
    for name in ("output_path", "output_image_path", "save_image"):
        typ, default, text = _common.FLAG_TABLE[name]
        ap.add_argument("--" + name, type=typ, default=default, help=text)
    ap.add_argument("--use_noise", type=bool, default=True, help="sample the latent (reparametrisation) instead of using its mean")
    typ, default, text = _common.FLAG_TABLE["device"]
    ap.add_argument("--device", type=typ, default=default, help=text)
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    vae = BCVAE()
    if args.weights_path == "synthetic":
        from said_amd.util import synth
        state = synth.vae_state_dict()
    else:
        state = torch.load(args.weights_path, map_location="cpu")
    vae.load_state_dict(state, strict=True)
    vae.to(args.device).eval()

    coeffs = load_blendshape_coeffs(args.blendshape_coeffs_path)
    if coeffs.shape[0] < vae.seq_len:
        sys.exit(f"{args.blendshape_coeffs_path}: {coeffs.shape[0]} frames, the VAE reconstructs windows of {vae.seq_len}")
    coeffs = coeffs[: vae.seq_len].unsqueeze(0).to(args.device)

    with torch.no_grad():
        out = vae(coeffs, args.use_noise)
    result = out.coeffs_reconst[0].cpu().numpy()
    save_blendshape_coeffs(coeffs=result, classes=DEFAULT_BLENDSHAPE_CLASSES, output_path=args.output_path)
    if args.save_image:
        save_blendshape_coeffs_image(result, args.output_image_path)


if __name__ == "__main__":
    main()
