"""The restatement of the denoiser's training step behind a fine-tuned Wav2Vec2 transformer — TEST INFRASTRUCTURE.

Composes two existing restatements under torch autograd, in whatever dtype the parameter dict has: tests/audio_train_ref.py's differentiable
train-mode encoder (the engine's Philox factors; with every probability 0, no mask and no skips it is oracle.wav2vec2's eval forward) on the
conv features, and tests/unet_train_ref.py's step (behind tests/unet_train_proj_ref.py's projection when the dict holds one).  The parameter
dict holds "audio_encoder.*" without the feature extractor beside the denoiser's tensors: all are autograd leaves of loss_and_grads and
parameters of RefTrainer.  As in unet_train_proj_ref, unet_train_ref is used as it is: its loss_and_grads and RefTrainer.step look `forward` up
in their module when called, and see the encoding one for the duration of a call.  Their `audio` argument is then the conv features (B, T, 512).
"""
from contextlib import contextmanager
from unittest import mock

import audio_train_ref as atr
import unet_train_proj_ref as pref
import unet_train_ref as ref

ENC = "audio_encoder."
PUBLISHED = dict(p_feat_proj=0.1, p_hidden=0.1, p_attention=0.1, p_activation=0.1)   # wav2vec2-base-960h's config values


def encoder_sd(sd):
    return {k[len(ENC):]: v for k, v in sd.items() if k.startswith(ENC)}


def conditioning(sd, feats, enc=None):
    """(B, T, 768) last hidden state of the encoder in sd on conv features `feats` (B, T, 512).  enc: None (eval mode) or a dict of
    audio_train_ref.forward's train-mode arguments (mask, skip, seed, p_feat_proj, p_hidden, p_attention, p_activation)."""
    dt = sd["null_cond_emb"].dtype
    return atr.forward(encoder_sd(sd), None, None, dtype=dt, feats=feats.to(dt), **(enc or {}))


def forward(sd, sample, timesteps, feats, cond, masks=None, enc=None):
    """The model output (B, T, 32) on conv features."""
    return pref.forward(sd, sample, timesteps, conditioning(sd, feats, enc), cond, masks)


@contextmanager
def _encoding(enc):
    with mock.patch.object(ref, "forward", lambda sd, sample, timesteps, feats, cond, masks=None: forward(sd, sample, timesteps, feats, cond, masks, enc)):
        yield


def loss_and_grads(sd, *args, enc=None, **kw):
    """unet_train_ref.loss_and_grads with the encoder in the graph: (losses, {name: gradient}) over every tensor of sd."""
    with _encoding(enc):
        return ref.loss_and_grads(sd, *args, **kw)


class RefTrainer(ref.RefTrainer):
    """unet_train_ref.RefTrainer whose parameter dict holds the encoder: one clip over everything, one AdamW, one EMA."""

    def step(self, *args, enc=None, **kw):
        with _encoding(enc):
            return super().step(*args, **kw)
