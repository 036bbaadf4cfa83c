"""Denoiser training on the MI355X (script/train.py of the reference).

``UNetTrainer`` holds UNet1DConditionModel's parameters and ``null_cond_emb`` (with ``feature_dim > 0`` also ``audio_proj_layer``, the
trainable nn.Linear(768, feature_dim) behind the frozen encoder), their AdamW moments and the EMA shadow in one device context
(include/said_unet_train.h) and runs a whole optimizer step there: add_noise, training-mode forward with ResBlock dropout, the objective of
``random_noise_loss``, backward, ``clip_grad_norm_(1.0)``, ``torch.optim.AdamW`` and diffusers' ``EMAModel.step``.  The host draws what the
reference draws on the host (noise and timesteps on torch's CPU generator, plus one 64-bit dropout seed per step) and writes the per-step
scalars.  The audio encoder is frozen; its embedding of the batch is an input of the step.  It runs as in inference, or, with
``train_epoch(..., audio_train=AudioTrainConfig())``, in Wav2Vec2's train mode as the reference's does.  With
``finetune_audio_layers > 0`` the Wav2Vec2 transformer is not frozen: it trains in the same step, behind the frozen feature extractor
(DESIGN.md 16.9).
"""
from __future__ import annotations

import os
import pickle
import random
import re
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn
from torch.utils.data import DataLoader, Dataset, RandomSampler

from .. import _engine
from ..model.wav2vec2 import AudioTrainConfig, draw_audio_train
from ..scheduler import DDIMScheduler
from ..util.audio import load_audio
from ..util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, load_blendshape_coeffs
from ..util.parser import parse_list
from .base import TrainerBase, parse_std
from .vae import DEFAULT_MIRROR_PAIRS, PERSON_IDS_TRAIN, PERSON_IDS_VAL, SENTENCE_IDS

PREDICTION_TYPES = {"epsilon": 0, "sample": 1, "v_prediction": 2}


@dataclass
class UNetLossStepOutput:
    """The losses of one step (script/train.py)"""

    predict: torch.FloatTensor  # MAE loss for the predicted output
    velocity: torch.FloatTensor  # MAE loss for the velocity
    vertex: Optional[torch.FloatTensor]  # MAE loss for the reconstructed vertex


@dataclass
class UNetLossEpochOutput:
    """The averaged losses of one epoch (script/train.py)"""

    total: float = 0
    predict: float = 0
    velocity: float = 0
    vertex: float = 0
    lr: Optional[float] = None


def trainable_shapes(feature_dim: int = -1, finetune_layers: int = 0) -> "OrderedDict[str, Tuple[int, ...]]":
    """Names and shapes of the trainable tensors of SAID_UNet1D(feature_dim=feature_dim) in state_dict() order: null_cond_emb, with
    feature_dim > 0 audio_proj_layer.weight / .bias, then denoiser.model.* as the reference registers them (BasicTransformerBlock: attn1,
    ff, attn2, norm1..3).  The context width (null_cond_emb, attn2.to_k / to_v) is feature_dim when > 0, else 768.  finetune_layers = L > 0
    appends the Wav2Vec2 transformer of an L-layer encoder: audio_encoder.* without audio_encoder.feature_extractor.*, in the encoder's
    state-dict order (said_amd.util.synth.w2v_param_shapes)."""
    C, E = 192, 768
    X = feature_dim if feature_dim > 0 else 768
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict([("null_cond_emb", (1, 1, X))])
    if feature_dim > 0:
        s["audio_proj_layer.weight"], s["audio_proj_layer.bias"] = (X, 768), (X,)
    m = "denoiser.model."

    def wb(p, *shape):
        s[p + ".weight"], s[p + ".bias"] = tuple(shape), (shape[0],)

    def res(p, cin):
        s[p + ".in_layers.0.weight"], s[p + ".in_layers.0.bias"] = (cin,), (cin,)
        wb(p + ".in_layers.2", C, cin, 3)
        wb(p + ".emb_layers.1", C, E)
        s[p + ".out_layers.0.weight"], s[p + ".out_layers.0.bias"] = (C,), (C,)
        wb(p + ".out_layers.3", C, C, 3)
        if cin != C:
            wb(p + ".skip_connection", C, cin, 1)

    def st(p):
        s[p + ".norm.weight"], s[p + ".norm.bias"] = (C,), (C,)
        b = p + ".transformer_blocks.0"

        def attn(a, kd):
            s[f"{b}.{a}.to_q.weight"], s[f"{b}.{a}.to_k.weight"], s[f"{b}.{a}.to_v.weight"] = (C, C), (C, kd), (C, kd)
            wb(f"{b}.{a}.to_out.0", C, C)

        attn("attn1", C)
        wb(b + ".ff.net.0.proj", 2 * 768, C)
        wb(b + ".ff.net.2", C, 768)
        attn("attn2", X)
        for n in ("norm1", "norm2", "norm3"):
            s[f"{b}.{n}.weight"], s[f"{b}.{n}.bias"] = (C,), (C,)
        wb(p + ".proj_out", C, C, 1)

    wb(m + "time_embed.0", E, C)
    wb(m + "time_embed.2", E, E)
    wb(m + "input_blocks.0.0", C, 32, 3)
    res(m + "input_blocks.1.0", C); st(m + "input_blocks.1.1")
    res(m + "middle_block.0", C); st(m + "middle_block.1"); res(m + "middle_block.2", C)
    res(m + "output_blocks.0.0", 2 * C); st(m + "output_blocks.0.1")
    res(m + "output_blocks.1.0", 2 * C); st(m + "output_blocks.1.1")
    s[m + "out.0.weight"], s[m + "out.0.bias"] = (C,), (C,)
    wb(m + "out.2", 32, C, 3)
    if finetune_layers > 0:
        from ..util.synth import w2v_param_shapes
        for k, shp in w2v_param_shapes(finetune_layers).items():
            if not k.startswith("feature_extractor."):
                s["audio_encoder." + k] = tuple(shp)
    return s


def unet_init_state_dict(feature_dim: int = -1) -> "OrderedDict[str, torch.Tensor]":
    """The trainable tensors of a freshly constructed reference denoiser: null_cond_emb = randn(1, 1, 768) (SAID.__init__ draws it before
    the denoiser is built; with feature_dim = F > 0 it constructs nn.Linear(768, F) first and then draws randn(1, 1, F), and the denoiser
    has cross_attention_dim = F), then the layers of UNet1DConditionModel(32, 32, 768) built in the reference's construction order with torch's
    default initialisation, so that after torch.manual_seed(s) the draws are the reference's for the same generator state.  The
    zero_module convolutions (ResBlock out conv, SpatialTransformer proj_out, final out conv) are drawn and then zeroed, as there.
    GroupNorm / LayerNorm gains are 1, biases 0.  (The reference's SAID also constructs the Wav2Vec2 encoder before null_cond_emb, which
    consumes generator state; it is frozen and loaded from a checkpoint, so it is not rebuilt here.)"""
    shapes = trainable_shapes(feature_dim)
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    if feature_dim > 0:
        proj = nn.Linear(768, feature_dim)
        out["audio_proj_layer.weight"], out["audio_proj_layer.bias"] = proj.weight.detach().clone(), proj.bias.detach().clone()
    out["null_cond_emb"] = torch.randn(shapes["null_cond_emb"])
    zeroed = (".out_layers.3.", ".proj_out.", "model.out.2.")
    done = set()
    for k, shp in shapes.items():
        if k in out or k in done:
            continue
        base, leaf = k.rsplit(".", 1)
        if len(shp) == 1 and (base + ".weight") in shapes and len(shapes[base + ".weight"]) == 1:   # a norm
            out[k] = torch.ones(shp) if leaf == "weight" else torch.zeros(shp)
            continue
        if leaf != "weight":
            continue   # a bias is drawn with its weight
        has_bias = (base + ".bias") in shapes
        layer = (nn.Linear(shp[1], shp[0], bias=has_bias) if len(shp) == 2 else nn.Conv1d(shp[1], shp[0], shp[2], padding=shp[2] // 2))
        zero = any(z in k for z in zeroed)
        out[k] = torch.zeros(shp) if zero else layer.weight.detach().clone()
        if has_bias:
            out[base + ".bias"] = torch.zeros(shp[0]) if zero else layer.bias.detach().clone()
            done.add(base + ".bias")
    return OrderedDict((k, out[k]) for k in shapes)


def normalize_deltas(blendshape_delta: torch.Tensor) -> torch.Tensor:
    """(B, 32, V, 3) blendshape deltas -> (B, 32, 3 V), each sample divided by its mean absolute value (script/train.py:135-141)."""
    d = torch.as_tensor(blendshape_delta, dtype=torch.float32)
    b, k, v, i = d.shape
    norm = torch.norm(d, p=1, dim=[1, 2, 3]) / (k * v * i)
    return torch.div(d, norm.view(-1, 1, 1, 1)).reshape(b, k, v * i)


class UNetTrainer(TrainerBase):
    """The denoiser of SAID_UNet1D trained on one MI355X with the reference's step (script/train.py).

    `state_dict` holds at least the trainable keys (null_cond_emb, denoiser.model.*); every other key (the frozen audio_encoder.*) is kept and
    passed through by state_dict(), so a saved file loads into SAID_UNet1D.  num_warmup_steps is the reference's
    len(train_dataloader) * num_warmup_epochs.  `std` (32,) reweights the losses.

    feature_dim = F > 0 trains SAID_UNet1D(feature_dim=F): audio_proj_layer.* of `state_dict` is the trainable projection's initial value,
    the context is F wide, and the audio embedding given to step / eval_loss / forward_only stays the encoder's (B, T, 768) output, before
    the projection (batch_audio_embedding asks the model for that).

    finetune_audio_layers = L > 0 trains the Wav2Vec2 transformer of `state_dict`'s L-layer encoder with the denoiser (the reference's
    `said_model.audio_encoder.freeze_feature_encoder()` variant): audio_encoder.* except audio_encoder.feature_extractor.*
    join the trainable tensors, and step / eval_loss / forward_only take the frozen extractor's features (B, T, 512) (batch_audio_features)
    in place of the audio embedding.  step's audio_draws / audio_cfg put the encoder in Wav2Vec2's train mode.  There
    encoder_products = "split_fp16" runs the encoder's dense products on split-fp16 operands (22 significand bits, fp32 accumulation; DESIGN.md
    16.10) in step, eval_loss and forward_only; "fp32", the default, leaves every launch as it is.  Given without fine-tuning it is refused.
    """

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", max_batch: int = 8, max_frames: int = 512, learning_rate: float = 1e-5,
                 num_warmup_steps: float = 0, ema: bool = True, ema_decay: float = 0.9999, std=None, prediction_type: str = "epsilon",
                 dropout: float = 0.1, weight_decay: float = 0.01, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 num_train_timesteps: int = 1000, feature_dim: int = -1, finetune_audio_layers: int = 0, encoder_products: Optional[str] = None):
        if prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"prediction_type must be one of {sorted(PREDICTION_TYPES)}, got {prediction_type!r}")
        if encoder_products is not None and encoder_products not in _engine.ENCODER_PRODUCTS:
            raise ValueError(f"encoder_products must be one of {sorted(_engine.ENCODER_PRODUCTS)}, got {encoder_products!r}")
        if encoder_products is not None and finetune_audio_layers <= 0:
            raise ValueError("encoder_products: the encoder is frozen here; its products are the trainer's only with finetune_audio_layers > 0")
        self.eng = _engine.UNetTrainEngine(torch.device(device), max_batch, max_frames, feature_dim, finetune_audio_layers)
        self.feature_dim = self.eng.feature_dim
        self.finetune_audio_layers = self.eng.finetune_layers
        self.encoder_products = encoder_products or "fp32"
        if encoder_products is not None:
            self.eng.set_encoder_products(encoder_products)
        self.device = self.eng.device
        self.max_batch, self.max_frames = int(max_batch), int(max_frames)
        self._set_optimizer(learning_rate, num_warmup_steps, weight_decay, betas, eps, ema, ema_decay)
        self.prediction_type, self.dropout = prediction_type, float(dropout)
        self.num_train_timesteps = int(num_train_timesteps)
        self.alphas_cumprod = DDIMScheduler(num_train_timesteps=num_train_timesteps, beta_schedule="squaredcos_cap_v2").alphas_cumprod.float()
        self.eng.set_alphas(self.alphas_cumprod.numpy())
        self.std = parse_std(std)
        self._shapes = trainable_shapes(self.feature_dim, self.finetune_audio_layers)
        self._stored = False
        self.load_state_dict(state_dict)

    # ---- state
    def load_state_dict(self, state_dict: Dict[str, torch.Tensor]) -> None:
        """Set the trainable tensors (strict), keep every other key for state_dict(), and restart the optimizer: zero moments, the EMA
        shadow a copy of the parameters, step count 0."""
        missing = [n for n in self.names if n not in state_dict]
        if missing:
            raise KeyError(f"denoiser state dict misses {missing[:4]}{'...' if len(missing) > 4 else ''}")
        for name, numel in self.eng.tensors:
            v = state_dict[name].detach().cpu().float()
            if tuple(v.shape) != self._shapes[name]:
                raise ValueError(f"{name}: shape {tuple(v.shape)}, expected {self._shapes[name]} (feature_dim={self.feature_dim})")
            self.eng.set_tensor(_engine.UT_STATE, name, v.numpy())
        self._frozen = OrderedDict((k, v.detach().cpu().clone()) for k, v in state_dict.items() if k not in self._shapes)
        self._given_order = list(state_dict)
        self.eng.reset_optimizer()
        self.step_count = 0

    def state_dict(self, ema: bool = False) -> "OrderedDict[str, torch.Tensor]":
        """SAID_UNet1D's checkpoint layout: the live trainable tensors (the EMA shadow with ema=True) and the frozen keys given at
        construction.  The CLI saves between ema_copy_to() and ema_restore(), as the reference does."""
        out = OrderedDict()
        tr = self.parameters_of(_engine.UT_EMA if (ema and self.ema) else _engine.UT_STATE)
        out["null_cond_emb"] = tr["null_cond_emb"]   # SAID registers audio_encoder, (audio_proj_layer,) null_cond_emb's parameter first, denoiser
        if self.finetune_audio_layers > 0:
            # the trained transformer over the frozen feature extractor, in the order the encoder's keys were given in
            out.update((k, tr[k] if k in tr else self._frozen[k]) for k in self._given_order if k.startswith("audio_encoder."))
            out.update((k, v) for k, v in self._frozen.items() if k not in out)
        else:
            out.update(self._frozen)
        out.update((k, v) for k, v in tr.items() if k != "null_cond_emb" and k not in out)
        return out

    # ---- EMAModel.store / copy_to / restore
    def ema_store(self) -> None:
        self.eng.copy(_engine.UT_STASH, _engine.UT_STATE)
        self._stored = True

    def ema_copy_to(self) -> None:
        self.eng.copy(_engine.UT_STATE, _engine.UT_EMA)

    def ema_restore(self) -> None:
        if not self._stored:
            raise RuntimeError("ema_restore() without ema_store()")
        self.eng.copy(_engine.UT_STATE, _engine.UT_STASH)
        self._stored = False

    # ---- the step
    def _scalars(self, weight_vel: float, weight_vertex: float, k: int, dropout: float) -> np.ndarray:
        """SAID_UT_S_* for optimizer step k (0-based), in double as torch / diffusers compute them."""
        s = self._optimizer_scalars(k)
        s[_engine.UT_S_WVEL] = weight_vel
        s[_engine.UT_S_WVERTEX] = weight_vertex
        s[_engine.UT_S_PRED_TYPE] = PREDICTION_TYPES[self.prediction_type]
        s[_engine.UT_S_DROPOUT] = dropout
        return s.astype(np.float32)

    def _draws(self, coeffs, noise, timesteps):
        """The reference's host draws where the caller gives none: torch.randn(latents.shape) and torch.randint(0, N, (B,)) on the CPU
        generator (SAID.add_noise / get_random_timesteps)."""
        x = torch.as_tensor(coeffs, dtype=torch.float32).cpu()
        if timesteps is None:
            timesteps = torch.randint(0, self.num_train_timesteps, (x.shape[0],), dtype=torch.long)
        if noise is None:
            noise = torch.randn(x.shape)
        return x.numpy(), torch.as_tensor(noise, dtype=torch.float32).cpu().numpy(), torch.as_tensor(timesteps).cpu().numpy()

    def enqueue_step(self, coeffs, cond, audio_embedding, noise=None, timesteps=None, dropout_seed: Optional[int] = None, weight_vel: float = 1.0,
                     weight_vertex: float = 0.02, deltas=None, audio_draws=None, audio_cfg: Optional[AudioTrainConfig] = None) -> None:
        """One optimizer step; nothing is read back.  With finetune_audio_layers > 0, `audio_embedding` holds the conv features and
        audio_draws (an AudioTrainDraws) / audio_cfg run the encoder in train mode."""
        if audio_draws is not None and self.finetune_audio_layers <= 0:
            raise ValueError("audio_draws: the encoder is frozen here; it runs in train mode where its embedding is computed (batch_audio_embedding)")
        x, nz, ts = self._draws(coeffs, noise, timesteps)
        if dropout_seed is None:
            dropout_seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if self.dropout > 0 else 0
        self.eng.step(x, nz, ts, cond, audio_embedding, dropout_seed, self._scalars(weight_vel, weight_vertex, self.step_count, self.dropout),
                      self.std, None if deltas is None else np.asarray(deltas, dtype=np.float32), audio_draws=audio_draws,
                      audio_cfg=(audio_cfg or AudioTrainConfig()) if audio_draws is not None else None)
        self.step_count += 1

    def step(self, coeffs, cond, audio_embedding, **kw) -> UNetLossStepOutput:
        """One optimizer step on the windows `coeffs` (B, T, 32) with their `cond` flags (B,) and audio embedding (B, T, 768); reads the
        step's losses back (one host sync).  deltas: (B, 32, 3 V) from normalize_deltas."""
        self.enqueue_step(coeffs, cond, audio_embedding, **kw)
        p, v, x, _, _, _ = self.eng.last_losses()
        return UNetLossStepOutput(predict=torch.tensor(p), velocity=torch.tensor(v), vertex=None if kw.get("deltas") is None else torch.tensor(x))

    def eval_loss(self, coeffs, cond, audio_embedding, noise=None, timesteps=None, weight_vel: float = 1.0, weight_vertex: float = 0.02,
                  deltas=None, use_ema: bool = False) -> None:
        """The objective without dropout and without an update, added to the validation accumulators."""
        x, nz, ts = self._draws(coeffs, noise, timesteps)
        self.eng.eval_loss(x, nz, ts, cond, audio_embedding, self._scalars(weight_vel, weight_vertex, self.step_count, 0.0), self.std,
                           None if deltas is None else np.asarray(deltas, dtype=np.float32), ema=use_ema)

    def forward_only(self, sample, timesteps, cond, audio_embedding, use_ema: bool = False) -> torch.Tensor:
        """The model output (B, T, 32) for a noisy sample, dropout off."""
        return torch.from_numpy(self.eng.forward_only(torch.as_tensor(sample, dtype=torch.float32).cpu().numpy(), torch.as_tensor(timesteps).cpu().numpy(),
                                                      cond, audio_embedding, ema=use_ema))

    def epoch_output(self, val: bool, lr: Optional[float] = None) -> UNetLossEpochOutput:
        """The averaged losses since the last call (training steps, or eval_loss calls with val=True)."""
        acc = self._epoch_sums(val)
        n = acc[4]
        return UNetLossEpochOutput(total=acc[3] / n, predict=acc[0] / n, velocity=acc[1] / n, vertex=acc[2] / n, lr=lr)

    def train_epoch(self, model, train_dataloader: Iterable, weight_vel: float, weight_vertex: float,
                    audio_train: Optional[AudioTrainConfig] = None) -> UNetLossEpochOutput:
        """train_epoch of script/train.py: one step per batch, the audio embedded by `model` (a SAID_UNet1D: its frozen HIP encoder), the
        losses read once at the end; lr is the LR after the last step.  audio_train: the encoder in Wav2Vec2's train mode (the reference
        calls said_model.train() before its epoch); None: as in inference."""
        for data in train_dataloader:
            if self.finetune_audio_layers > 0:
                # the draws come where batch_audio_embedding draws them: before the step's own
                feats = batch_audio_features(model, data)
                draws = None if audio_train is None else draw_audio_train(audio_train, feats.shape[0], feats.shape[1], self.finetune_audio_layers)
                self.enqueue_step(data.blendshape_coeffs, data.cond, feats, weight_vel=weight_vel, weight_vertex=weight_vertex,
                                  deltas=None if data.blendshape_delta is None else normalize_deltas(data.blendshape_delta), audio_draws=draws,
                                  audio_cfg=audio_train)
                continue
            self.enqueue_step(data.blendshape_coeffs, data.cond, batch_audio_embedding(model, data, audio_train, self.feature_dim > 0), weight_vel=weight_vel,
                              weight_vertex=weight_vertex, deltas=None if data.blendshape_delta is None else normalize_deltas(data.blendshape_delta))
        return self.epoch_output(False, self.lr_at(self.step_count))

    def validate(self, model, val_dataloader: Iterable, weight_vel: float, weight_vertex: float, num_repeat: int = 1,
                 use_ema: bool = False) -> UNetLossEpochOutput:
        """validate_epoch of script/train.py: no dropout, no update; on the live parameters (the CLI swaps the EMA in around it, as the
        reference does) or, with use_ema, directly on the EMA copy."""
        for _ in range(num_repeat):
            for data in val_dataloader:
                audio = batch_audio_features(model, data) if self.finetune_audio_layers > 0 else batch_audio_embedding(model, data, before_proj=self.feature_dim > 0)
                self.eval_loss(data.blendshape_coeffs, data.cond, audio, weight_vel=weight_vel, weight_vertex=weight_vertex,
                               deltas=None if data.blendshape_delta is None else normalize_deltas(data.blendshape_delta), use_ema=use_ema)
        return self.epoch_output(True)


def batch_audio_embedding(model, data, audio_train: Optional[AudioTrainConfig] = None, before_proj: bool = False) -> torch.Tensor:
    """(B, T, 768) embedding of a batch's waveforms by the model's frozen audio encoder, as random_noise_loss obtains it.  `before_proj`
    (the trainers with feature_dim > 0 set it): a model with an audio_proj_layer returns the features before it, still (B, T, 768); the
    model's own projection is never read.  With
    `audio_train` the encoder runs in Wav2Vec2's train mode, as the reference's does during its training epoch: the span mask, the
    LayerDrop decisions and the dropout seed are drawn here (draw_audio_train), before the step draws its own."""
    wave = model.process_audio(data.waveform).to(next(model.parameters()).device)
    frames = data.blendshape_coeffs.shape[1]
    if audio_train is None:
        return model.get_audio_embedding(wave, frames, before_proj=before_proj).float()
    draws = draw_audio_train(audio_train, wave.shape[0], frames, model.audio_config.num_hidden_layers)
    return model.get_audio_embedding(wave, frames, train_draws=draws, train_cfg=audio_train, before_proj=before_proj).float()


def batch_audio_features(model, data) -> torch.Tensor:
    """(B, T, 512) conv features of a batch's waveforms by the model's frozen feature extractor, interpolated to the batch's frames: what a
    trainer with finetune_audio_layers > 0 takes in place of the audio embedding."""
    wave = model.process_audio(data.waveform).to(next(model.parameters()).device)
    return model.get_audio_features(wave, data.blendshape_coeffs.shape[1]).float()


# ---------------------------------------------------------------------------------------------------------------- data sets
@dataclass
class DataItem:
    waveform: torch.Tensor  # (audio_seq_len,)
    blendshape_coeffs: torch.Tensor  # (blendshape_seq_len, 32)
    cond: bool = True
    blendshape_delta: Optional[torch.Tensor] = None  # (32, |V|, 3)


@dataclass
class DataBatch:
    waveform: List[np.ndarray]
    blendshape_coeffs: torch.Tensor  # (B, T, 32)
    cond: torch.Tensor  # (B,) bool
    blendshape_delta: Optional[torch.Tensor] = None  # (B, 32, |V|, 3)


def cut_window(seq: torch.Tensor, start: int, length: int, pad_before: int, pad_after: int) -> torch.Tensor:
    """F.pad(seq, (pad_before, pad_after) along dim 0, "replicate")[start : start + length] without forming the padded tensor: padded
    position q holds seq[clamp(q - pad_before, 0, n - 1)]; positions past the padded end are dropped, as a slice drops them."""
    n = seq.shape[0]
    q = torch.arange(start, min(start + length, n + pad_before + pad_after))
    return seq[(q - pad_before).clamp(0, n - 1)]


class _WindowDataset(Dataset):
    fps = 60

    def _load(self, audio_dir, coeffs_dir, deltas_path, landmarks_path, person_ids, classes, pairs, items):
        self.classes = list(classes)
        self.mirror_indices, self.mirror_indices_flip = [], []
        for left, right in pairs:
            il, ir = self.classes.index(left), self.classes.index(right)
            self.mirror_indices += [il, ir]
            self.mirror_indices_flip += [ir, il]
        if items is not None:   # (waveform, coeffs[, delta]) given directly
            self.data = [(torch.as_tensor(i[0], dtype=torch.float32), torch.as_tensor(i[1], dtype=torch.float32).clone(),
                          None if len(i) < 3 or i[2] is None else torch.as_tensor(i[2], dtype=torch.float32)) for i in items]
            return
        deltas = None
        if deltas_path:
            with open(deltas_path, "rb") as f:
                deltas = pickle.load(f)
        landmarks = parse_list(landmarks_path, int) if landmarks_path else None
        per_person: Dict[str, Optional[torch.Tensor]] = {}
        self.data = []
        for pid in person_ids:
            cdir = os.path.join(coeffs_dir, pid)
            names = os.listdir(cdir) if os.path.exists(cdir) else []
            for sid in SENTENCE_IDS:
                audio = os.path.join(audio_dir, pid, f"sentence{sid:02}.wav")
                if not os.path.exists(audio):
                    continue
                pat = re.compile(rf"^sentence{sid:02}(-.+)?\.csv$")
                for name in names:
                    if not pat.match(name):
                        continue
                    if pid not in per_person:
                        d = None
                        if deltas is not None:
                            d = torch.FloatTensor(np.stack(list(deltas[pid].values()), axis=0))
                            if landmarks:
                                d = d[:, landmarks, :]
                        per_person[pid] = d
                    self.data.append((load_audio(audio, self.sampling_rate), load_blendshape_coeffs(os.path.join(cdir, name)), per_person[pid]))

    def __len__(self) -> int:
        return len(self.data)


class TrainWindowDataset(_WindowDataset):
    """BlendVOCATrainDataset (dataset_voca.py:364-624).  ``dataset[i]`` draws cond, hflip and zero-out with Python ``random`` in the
    reference's order; ``collate_fn`` draws the window size, then per item bdx and the delay, and cuts the coefficient and waveform windows
    with replicate padding.  As in the reference with preload, the flip swaps columns of the stored sequence in place."""

    def __init__(self, audio_dir: Optional[str] = None, blendshape_coeffs_dir: Optional[str] = None, blendshape_deltas_path: Optional[str] = None,
                 landmarks_path: Optional[str] = None, sampling_rate: int = 16000, window_size_min: int = 120, uncond_prob: float = 0.1,
                 zero_prob: float = 0, hflip: bool = True, delay: bool = True, delay_thres: int = 1,
                 classes: Sequence[str] = DEFAULT_BLENDSHAPE_CLASSES, classes_mirror_pair=DEFAULT_MIRROR_PAIRS, items=None,
                 person_ids: Sequence[str] = PERSON_IDS_TRAIN):
        self.sampling_rate, self.window_size_min, self.uncond_prob, self.zero_prob = sampling_rate, window_size_min, uncond_prob, zero_prob
        self.hflip, self.delay, self.delay_thres = hflip, delay, delay_thres
        self._load(audio_dir, blendshape_coeffs_dir, blendshape_deltas_path, landmarks_path, person_ids, classes, classes_mirror_pair, items)

    def __getitem__(self, index: int) -> DataItem:
        waveform, coeffs, delta = self.data[index]
        cond = random.uniform(0, 1) > self.uncond_prob
        if self.hflip and random.uniform(0, 1) < 0.5:
            coeffs[:, self.mirror_indices] = coeffs[:, self.mirror_indices_flip]
        if random.uniform(0, 1) < self.zero_prob:
            waveform, coeffs = torch.zeros_like(waveform), torch.zeros_like(coeffs)
        return DataItem(waveform=waveform, blendshape_coeffs=coeffs, cond=cond, blendshape_delta=delta)

    def collate_fn(self, examples: List[DataItem]) -> DataBatch:
        shortest = min(e.blendshape_coeffs.shape[0] for e in examples)
        window = random.randrange(self.window_size_min, shortest + 1)
        wave_len = (self.sampling_rate * window) // self.fps
        half, half_wave, th = window // 2, wave_len // 2, self.delay_thres
        waves, wins = [], []
        for e in examples:
            n = e.blendshape_coeffs.shape[0]
            bdx = random.randint(-half, max(0, n - half - 1))
            wdx = (self.sampling_rate * bdx) // self.fps
            if self.delay and random.uniform(0, 1) < 0.5:
                wdx = random.randint(wdx - th, wdx + th)
            wins.append(cut_window(e.blendshape_coeffs, bdx + half, window, half, window))
            waves.append(cut_window(e.waveform, max(0, wdx + half_wave + th), wave_len, half_wave + th, wave_len + th).numpy())
        delta = None if examples[0].blendshape_delta is None else torch.stack([e.blendshape_delta for e in examples])
        return DataBatch(waveform=waves, blendshape_coeffs=torch.stack(wins), cond=torch.BoolTensor([e.cond for e in examples]), blendshape_delta=delta)


class ValWindowDataset(_WindowDataset):
    """BlendVOCAValDataset (dataset_voca.py:627-774): whole sequences, the waveform cut or zero-padded to the coefficient length; draws
    cond and zero-out (no flip)."""

    def __init__(self, audio_dir: Optional[str] = None, blendshape_coeffs_dir: Optional[str] = None, blendshape_deltas_path: Optional[str] = None,
                 landmarks_path: Optional[str] = None, sampling_rate: int = 16000, uncond_prob: float = 0.1, zero_prob: float = 0,
                 hflip: bool = True, classes: Sequence[str] = DEFAULT_BLENDSHAPE_CLASSES, classes_mirror_pair=DEFAULT_MIRROR_PAIRS, items=None,
                 person_ids: Sequence[str] = PERSON_IDS_VAL):
        self.sampling_rate, self.uncond_prob, self.zero_prob, self.hflip = sampling_rate, uncond_prob, zero_prob, hflip
        self._load(audio_dir, blendshape_coeffs_dir, blendshape_deltas_path, landmarks_path, person_ids, classes, classes_mirror_pair, items)

    def __getitem__(self, index: int) -> DataItem:
        waveform, coeffs, delta = self.data[index]
        wave_len = (self.sampling_rate * coeffs.shape[0]) // self.fps
        cut = waveform[:wave_len]
        window = torch.zeros(wave_len)
        window[: cut.shape[0]] = cut
        cond = random.uniform(0, 1) > self.uncond_prob
        if random.uniform(0, 1) < self.zero_prob:
            window, coeffs = torch.zeros_like(window), torch.zeros_like(coeffs)
        return DataItem(waveform=window, blendshape_coeffs=coeffs, cond=cond, blendshape_delta=delta)

    @staticmethod
    def collate_fn(examples: List[DataItem]) -> DataBatch:
        delta = None if examples[0].blendshape_delta is None else torch.stack([e.blendshape_delta for e in examples])
        return DataBatch(waveform=[e.waveform.numpy() for e in examples], blendshape_coeffs=torch.stack([e.blendshape_coeffs for e in examples]),
                         cond=torch.BoolTensor([e.cond for e in examples]), blendshape_delta=delta)


def make_unet_dataloaders(train_dataset: TrainWindowDataset, val_dataset: Optional[ValWindowDataset], batch_size: int, num_workers: int = 0):
    """The reference's loaders: RandomSampler(replacement=True, num_samples=len) in batches of `batch_size`; validation in order, batch 1."""
    sampler = RandomSampler(train_dataset, replacement=True, num_samples=len(train_dataset))
    train = DataLoader(train_dataset, batch_size=batch_size, sampler=sampler, collate_fn=train_dataset.collate_fn, num_workers=num_workers)
    val = None if val_dataset is None else DataLoader(val_dataset, batch_size=1, shuffle=False, collate_fn=ValWindowDataset.collate_fn,
                                                      num_workers=num_workers)
    return train, val
