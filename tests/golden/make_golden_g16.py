"""Capture golden G16 (tests/golden/g16_unet_train.npz) from the reference's own UNet1DConditionModel in train() mode.

    python tests/golden/make_golden_g16.py /path/to/reference

Only said/model/unet_1d_condition.py (and the ldm modules it imports) is loaded; SAID / SAID_UNet1D are never constructed.  The module is
built with dropout=0.0, filled with said_amd.util.synth's deterministic values (non-zero in the zero_module convolutions) and run in its
own fp32 (its timestep embedding and GroupNorm32 are fp32 by construction) at B = 2, T = 40 on a context selected between the audio embedding and a null_cond_emb leaf by cond = [True, False].  Stored: the
inputs, the output, and for every parameter (and null_cond_emb) the float64 sum and 2-norm of its gradient under
l1(pred, answer) + l1(diff(pred), diff(answer)); full gradients of the tensors of at most 1536 elements.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from said_amd.util.synth import said_state_dict  # noqa: E402


def main(ref_root: str) -> None:
    for name, path in (("said", os.path.join(ref_root, "said")), ("said.model", os.path.join(ref_root, "said", "model"))):
        pkg = types.ModuleType(name)   # empty packages: the reference's __init__ files import SAID and its dependencies
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    from said.model.unet_1d_condition import UNet1DConditionModel

    B, T = 2, 40
    model = UNet1DConditionModel(32, 32, 768, dropout=0.0)
    sd = said_state_dict(num_w2v_layers=1)
    model.load_state_dict({k[len("denoiser."):]: v for k, v in sd.items() if k.startswith("denoiser.")})
    model = model.train()
    null = sd["null_cond_emb"].clone().requires_grad_(True)
    g = torch.Generator().manual_seed(16)
    x = torch.randn(B, T, 32, generator=g)
    answer = torch.randn(B, T, 32, generator=g)
    audio = torch.randn(B, T, 768, generator=g)
    ts = torch.tensor([25, 730])
    cond = torch.tensor([True, False])
    ctx = torch.where(cond.view(-1, 1, 1), audio, null.expand(B, T, -1))
    out = model(x, ts, ctx)
    a = answer
    loss = F.l1_loss(out, a) + F.l1_loss(out[:, 1:] - out[:, :-1], a[:, 1:] - a[:, :-1])
    loss.backward()
    names = ["null_cond_emb"] + ["denoiser." + k for k, _ in model.named_parameters()]
    grads = [null.grad] + [p.grad for _, p in model.named_parameters()]
    store = dict(x=x.numpy(), answer=answer.numpy(), audio=audio.numpy(), timesteps=ts.numpy(), cond=cond.numpy(), out=out.detach().numpy(),
                 loss=np.float64(loss.item()), names=np.array(names), state_names=np.array(["denoiser." + k for k in model.state_dict()]),
                 grad_sum=np.array([float(q.double().sum()) for q in grads]), grad_norm=np.array([float(q.double().norm()) for q in grads]))
    for n, q in zip(names, grads):
        if q.numel() <= 1536:
            store["g:" + n] = q.numpy().reshape(-1)
    np.savez_compressed(os.path.join(HERE, "g16_unet_train.npz"), **store)


if __name__ == "__main__":
    main(sys.argv[1])
