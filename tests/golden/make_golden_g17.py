"""Capture golden G17 (tests/golden/g17_unet_train_proj.npz) from the reference's own UNet1DConditionModel at a context width of 40, behind a
trainable nn.Linear(768, 40): the feature_dim > 0 variant of SAID_UNet1D, without constructing SAID (its Wav2Vec2 is frozen and plays no part).

    python tests/golden/make_golden_g17.py /path/to/reference

Only said/model/unet_1d_condition.py (and the ldm modules it imports) is loaded, through empty parent packages, as make_golden_g16.py does.

Part A, step parity.  UNet1DConditionModel(32, 32, 40, dropout=0.0) in train(), filled from said_amd.util.synth.said_state_dict(num_w2v_layers=1,
ctx_dim=40); the projection a plain nn.Linear(768, 40) filled with synth.fill_tensor("audio_proj_layer.weight" / ".bias", ...).  B = 2, T = 40.
The context is formed as script/train.py:86-94 forms it: cond_embedding = proj(audio), uncond = null_cond_emb.repeat(B, T, 1),
cond_embedding * mask + uncond * logical_not(mask), cond = [True, False].  The objective is G16's, l1(pred, answer) + l1(diff(pred),
diff(answer)).  Stored: the inputs, the output, the loss, for each of the 163 tensors the float64 sum and 2-norm of its gradient, and the full
gradients of the tensors of at most 1536 elements and of audio_proj_layer.bias.

Part B, init parity.  After torch.manual_seed(17): nn.Linear(768, 40), torch.randn(1, 1, 40), UNet1DConditionModel(32, 32, 40), in the order of
SAID.__init__ / SAID_UNet1D.__init__ (said/model/diffusion.py:108-115, 524-526).  For every tensor its float64 sum and first four values.
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

from said_amd.util.synth import fill_tensor, said_state_dict  # noqa: E402

FD = 40


def main(ref_root: str) -> None:
    for name, path in (("said", os.path.join(ref_root, "said")), ("said.model", os.path.join(ref_root, "said", "model"))):
        pkg = types.ModuleType(name)   # empty packages: the reference's __init__ files import SAID and its dependencies
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    from said.model.unet_1d_condition import UNet1DConditionModel

    # ---- part A
    B, T = 2, 40
    model = UNet1DConditionModel(32, 32, FD, dropout=0.0)
    sd = said_state_dict(num_w2v_layers=1, ctx_dim=FD)
    model.load_state_dict({k[len("denoiser."):]: v for k, v in sd.items() if k.startswith("denoiser.")})
    model = model.train()
    proj = torch.nn.Linear(768, FD)
    with torch.no_grad():
        proj.weight.copy_(fill_tensor("audio_proj_layer.weight", (FD, 768)))
        proj.bias.copy_(fill_tensor("audio_proj_layer.bias", (FD,)))
    null = sd["null_cond_emb"].clone().requires_grad_(True)
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, T, 32, generator=g)
    answer = torch.randn(B, T, 32, generator=g)
    audio = torch.randn(B, T, 768, generator=g)
    ts = torch.tensor([25, 730])
    cond = torch.tensor([True, False])
    cond_embedding = proj(audio)
    uncond_embedding = null.repeat(B, cond_embedding.shape[1], 1)
    cond_mask = cond.view(-1, 1, 1)
    ctx = cond_embedding * cond_mask + uncond_embedding * torch.logical_not(cond_mask)
    out = model(x, ts, ctx)
    a = answer
    loss = F.l1_loss(out, a) + F.l1_loss(out[:, 1:] - out[:, :-1], a[:, 1:] - a[:, :-1])
    loss.backward()
    names = ["null_cond_emb", "audio_proj_layer.weight", "audio_proj_layer.bias"] + ["denoiser." + k for k, _ in model.named_parameters()]
    grads = [null.grad, proj.weight.grad, proj.bias.grad] + [p.grad for _, p in model.named_parameters()]
    assert len(names) == 163
    store = dict(x=x.numpy(), answer=answer.numpy(), audio=audio.numpy(), timesteps=ts.numpy(), cond=cond.numpy(), out=out.detach().numpy(),
                 loss=np.float64(loss.item()), names=np.array(names),
                 grad_sum=np.array([float(q.double().sum()) for q in grads]), grad_norm=np.array([float(q.double().norm()) for q in grads]))
    for n, q in zip(names, grads):
        if q.numel() <= 1536 or n == "audio_proj_layer.bias":
            store["g:" + n] = q.numpy().reshape(-1)

    # ---- part B
    torch.manual_seed(17)
    lin = torch.nn.Linear(768, FD)
    null0 = torch.randn(1, 1, FD)
    fresh = UNet1DConditionModel(32, 32, FD)
    init = [("null_cond_emb", null0), ("audio_proj_layer.weight", lin.weight), ("audio_proj_layer.bias", lin.bias)]
    init += [("denoiser." + k, v) for k, v in fresh.state_dict().items()]
    store["init_names"] = np.array([n for n, _ in init])
    store["init_sum"] = np.array([float(v.detach().double().sum()) for _, v in init])
    store["init_first4"] = np.stack([v.detach().reshape(-1)[:4].numpy() for _, v in init])
    np.savez_compressed(os.path.join(HERE, "g17_unet_train_proj.npz"), **store)


if __name__ == "__main__":
    main(sys.argv[1])
