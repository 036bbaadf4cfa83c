"""The restatement of the denoiser's training step (tests/unet_train_ref.py) behind a trainable audio_proj_layer — TEST INFRASTRUCTURE.

SAID_UNet1D(feature_dim=F > 0) projects the frozen encoder's (B, T, 768) output with nn.Linear(768, F) and only then selects between it and
null_cond_emb (said/model/diffusion.py:228-229, script/train.py:86-94 of the reference).  unet_train_ref's forward takes the context at any
width, so the projection is applied here, in the working dtype, on the tensors "audio_proj_layer.weight" / ".bias" of the same parameter dict:
they are autograd leaves of loss_and_grads and parameters of RefTrainer like every other tensor.  unet_train_ref itself is used as it is: its
loss_and_grads and RefTrainer.step look `forward` up in their module when called, and see the projecting one for the duration of a call.
"""
from contextlib import contextmanager
from unittest import mock

import torch.nn.functional as F

import unet_train_ref as ref

W, B_ = "audio_proj_layer.weight", "audio_proj_layer.bias"
_plain_forward = ref.forward


def project(sd, audio):
    """(B, T, 768) encoder output -> (B, T, F) in sd's dtype; unchanged for a parameter dict without a projection."""
    if W not in sd:
        return audio
    return F.linear(audio.to(sd[W].dtype), sd[W], sd[B_])


def forward(sd, sample, timesteps, audio, cond, masks=None):
    """unet_train_ref.forward on the projected audio: `audio` is the encoder's output, before the projection."""
    return _plain_forward(sd, sample, timesteps, project(sd, audio), cond, masks)


@contextmanager
def _projecting():
    with mock.patch.object(ref, "forward", forward):
        yield


def loss_and_grads(sd, *args, **kw):
    """unet_train_ref.loss_and_grads with the projection in the graph: (losses, {name: gradient}) over every tensor of sd."""
    with _projecting():
        return ref.loss_and_grads(sd, *args, **kw)


class RefTrainer(ref.RefTrainer):
    """unet_train_ref.RefTrainer whose parameter dict holds the projection: clipped, decayed, updated and averaged with the rest."""

    def step(self, *args, **kw):
        with _projecting():
            return super().step(*args, **kw)
