"""Capture golden G18 (tests/golden/g18_audio_finetune.npz) from the reference's own ModifiedWav2Vec2Model.

    python tests/golden/make_golden_g18.py /path/to/reference

Only said/model/wav2vec2.py is loaded (as make_golden.py loads it for G5); SAID is never constructed.  The module is built with 2 layers, filled
with said_amd.util.synth.said_state_dict(num_w2v_layers=2) (weight-norm keys mapped as G5 maps them), put in eval() and run in its own fp32 on
B = 2 seeded waveforms of 0.4 s with num_frames = 19.  The feature extractor is frozen (freeze_feature_encoder(), the variant that fine-tuning
trains).  Stored: the inputs, last_hidden_state, the conv features after the interpolation, and for every trainable tensor the float64 sum and
2-norm of its gradient under l1(out, target) + l1(diff(out), diff(target)); full gradients of the tensors of at most 1536 elements
(weight_v alone has 4.7 M values).
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

from said_amd.util.synth import said_state_dict, synth_waveform  # noqa: E402

G, V = "conv.parametrizations.weight.original0", "conv.parametrizations.weight.original1"


def main(ref_root: str) -> None:
    for name, path in (("said", os.path.join(ref_root, "said")), ("said.model", os.path.join(ref_root, "said", "model"))):
        pkg = types.ModuleType(name)   # empty packages: the reference's __init__ files import SAID and its dependencies
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    from said.model.wav2vec2 import ModifiedWav2Vec2Model
    from transformers import Wav2Vec2Config

    B, frames, L = 2, 19, 2
    model = ModifiedWav2Vec2Model(Wav2Vec2Config(num_hidden_layers=L))
    sd = {k[len("audio_encoder."):]: v for k, v in said_state_dict(num_w2v_layers=L).items() if k.startswith("audio_encoder.")}
    model.load_state_dict({k.replace("conv.weight_g", G).replace("conv.weight_v", V): v for k, v in sd.items()}, strict=True)
    model = model.eval()
    model.freeze_feature_encoder()
    wave = torch.stack([synth_waveform(i, 6400) for i in range(B)])
    g = torch.Generator().manual_seed(18)
    target = torch.randn(B, frames, 768, generator=g)
    feats = {}
    hook = model.feature_projection.register_forward_pre_hook(lambda m, i: feats.update(x=i[0].detach().clone()))
    out = model(wave, num_frames=frames).last_hidden_state
    hook.remove()
    loss = F.l1_loss(out, target) + F.l1_loss(out[:, 1:] - out[:, :-1], target[:, 1:] - target[:, :-1])
    loss.backward()
    back = {G: "conv.weight_g", V: "conv.weight_v"}
    names, grads = [], []
    for k, p in model.named_parameters():
        if k.startswith("feature_extractor."):
            assert p.grad is None, k
            continue
        for a, b in back.items():
            k = k.replace(a, b)
        names.append("audio_encoder." + k)
        grads.append(p.grad if p.grad is not None else torch.zeros_like(p))
    store = dict(waveform=wave.numpy(), target=target.numpy(), num_frames=np.int64(frames), features=feats["x"].numpy(), out=out.detach().numpy(),
                 loss=np.float64(loss.item()), names=np.array(names), grad_sum=np.array([float(q.double().sum()) for q in grads]),
                 grad_norm=np.array([float(q.double().norm()) for q in grads]))
    for n, q in zip(names, grads):
        if q.numel() <= 1536:
            store["g:" + n] = q.numpy().reshape(-1)
    np.savez_compressed(os.path.join(HERE, "g18_audio_finetune.npz"), **store)
    print(len(names), "tensors; loss", loss.item())


if __name__ == "__main__":
    main(sys.argv[1])
