"""Kernel bring-up aid (run on the GPU box): the fp32 denoise step launch by launch, with its default options, each launch against the float64 evaluation of its
own stored inputs — a command line over tests/test_gpu_unet_f32_kernels.py's harness and tests/unet_f32_ref.py.

    python tests/debug_stages.py [B] [T] [plain|trained]

Prints one line per comparison (e, the fp32 CPU evaluation's own e32, the bound 4 max(e32, 1e-6)) and stops at the first launch beyond its bound.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import test_gpu_unet_f32_kernels as K  # noqa: E402
from oracle import pipeline as op  # noqa: E402
from said_amd.util import synth  # noqa: E402

torch.set_grad_enabled(False)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 70
    fill = sys.argv[3] if len(sys.argv) > 3 else "plain"
    dev = torch.device("cuda:0")
    full = synth.trained_like_state_dict(num_w2v_layers=1) if fill == "trained" else synth.said_state_dict(num_w2v_layers=1)
    _, sd_u, _ = op.split_state_dict(full)
    K._forward_case(K._model(dev, full), sd_u, dev, f"{B} x {T} {fill}", B, T, 21, None)


if __name__ == "__main__":
    main()
