"""BCVAE training on the MI355X (script/train_vae.py, script/dataset/dataset_voca.py:1090-1264 of the reference).

``BCVAETrainer`` holds the model state, the AdamW moments and the EMA shadow in one device context (include/said_train.h) and runs a
whole optimizer step there: training-mode forward, ``elbo_loss`` (reweighted out of place), backward, ``clip_grad_norm_(1.0)``,
``torch.optim.AdamW`` and diffusers' ``EMAModel.step``, replayed from a captured graph.  The host only draws what the reference draws on
the host (the window choice with Python ``random``, the reparametrisation noise with ``torch.randn`` on the CPU generator) and writes
the per-step scalars.  Losses stay on the device until the end of an epoch.

``VAEWindowDataset`` is BlendVOCAVAEDataset with the windows cut on the device: ``__getitem__`` makes the reference's draws and returns
(sequence, bdx, flip, zero); the sequences are uploaded once.  Batching goes through torch's own DataLoader and RandomSampler, so the
draw order is the reference's.
"""
from __future__ import annotations

import math
import os
import random
import re
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn
from torch.utils.data import DataLoader, Dataset, RandomSampler

from .. import _engine
from ..util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, load_blendshape_coeffs
from .base import TrainerBase, parse_std

PERSON_IDS_TRAIN = [
    "FaceTalk_170725_00137_TA", "FaceTalk_170728_03272_TA", "FaceTalk_170811_03274_TA", "FaceTalk_170904_00128_TA",
    "FaceTalk_170904_03276_TA", "FaceTalk_170912_03278_TA", "FaceTalk_170913_03279_TA", "FaceTalk_170915_00223_TA",
]
PERSON_IDS_VAL = ["FaceTalk_170811_03275_TA", "FaceTalk_170908_03277_TA"]
PERSON_IDS_TEST = ["FaceTalk_170731_00024_TA", "FaceTalk_170809_00138_TA"]
SENTENCE_IDS = list(range(1, 41))
DEFAULT_MIRROR_PAIRS: List[Tuple[str, str]] = [
    ("jawLeft", "jawRight"), ("mouthLeft", "mouthRight"), ("mouthSmileLeft", "mouthSmileRight"), ("mouthFrownLeft", "mouthFrownRight"),
    ("mouthDimpleLeft", "mouthDimpleRight"), ("mouthStretchLeft", "mouthStretchRight"), ("mouthPressLeft", "mouthPressRight"),
    ("mouthLowerDownLeft", "mouthLowerDownRight"), ("mouthUpperUpLeft", "mouthUpperUpRight"), ("cheekSquintLeft", "cheekSquintRight"),
    ("noseSneerLeft", "noseSneerRight"),
]
# the BatchNorm1d layers whose preceding layer's bias they cancel: the exact gradient of these biases is 0
BN_CANCELLED_BIASES = [
    "encoder.conv_layers.0.bias", "encoder.conv_layers.3.bias", "encoder.conv_layers.6.bias", "encoder.conv_layers.9.bias",
    "encoder.fc_layers.0.bias", "encoder.fc_layers.3.bias", "decoder.fc_layers.0.bias", "decoder.conv_layers.0.bias", "decoder.conv_layers.3.bias",
]


@dataclass
class LossStepOutput:
    """The losses of one step (script/train_vae.py)"""

    reconst: torch.FloatTensor  # (1,), Reconstruction loss
    regularize: torch.FloatTensor  # (1,), Regularization loss
    velocity: torch.FloatTensor  # (1,), Velocity loss


@dataclass
class LossEpochOutput:
    """The averaged losses of one epoch (script/train_vae.py)"""

    total: float  # Averaged total loss
    reconst: float  # Averaged reconstruction loss
    regularize: float  # Averaged regularization loss
    velocity: float  # Averaged velocity loss
    lr: Optional[float] = None  # Last learning rate


# ---------------------------------------------------------------------------------------------------------------- initial weights
def _reference_modules(channels: int = 32, seq_len: int = 120, z_dim: int = 64) -> nn.Module:
    """The reference BCVAE's layers (said/model/vae.py), built in its module order so that torch's default initialisation draws the same
    numbers from the global generator."""
    enc = nn.Module()
    enc.conv_layers = nn.Sequential(
        nn.Conv1d(channels, 32, kernel_size=3, stride=1), nn.BatchNorm1d(32), nn.LeakyReLU(0.2, True),
        nn.Conv1d(32, 64, kernel_size=3, stride=1), nn.BatchNorm1d(64), nn.LeakyReLU(0.2, True),
        nn.Conv1d(64, 64, kernel_size=4, stride=2), nn.BatchNorm1d(64), nn.LeakyReLU(0.2, True),
        nn.Conv1d(64, 32, kernel_size=3, stride=1), nn.Flatten())
    enc.fc_layers = nn.Sequential(
        nn.Linear(1760, 256), nn.BatchNorm1d(256), nn.LeakyReLU(inplace=True),
        nn.Linear(256, 128), nn.BatchNorm1d(128), nn.LeakyReLU(inplace=True), nn.Linear(128, z_dim))
    enc.fc_mu = nn.Linear(z_dim, z_dim)
    enc.fc_logvar = nn.Linear(z_dim, z_dim)
    dec = nn.Module()
    dec.fc_layers = nn.Sequential(
        nn.Linear(z_dim, 2 * seq_len), nn.BatchNorm1d(2 * seq_len), nn.LeakyReLU(inplace=True),
        nn.Linear(2 * seq_len, 4 * seq_len), nn.Unflatten(1, (4, seq_len)))
    dec.conv_layers = nn.Sequential(
        nn.ConvTranspose1d(4, 32, 3), nn.BatchNorm1d(32), nn.LeakyReLU(0.2, True),
        nn.ConvTranspose1d(32, 32, 3), nn.BatchNorm1d(32), nn.LeakyReLU(0.2, True),
        nn.Conv1d(32, 32, 3), nn.Conv1d(32, channels, 3), nn.ReLU(), nn.Tanh())
    m = nn.Module()
    m.encoder = enc
    m.decoder = dec
    return m


def bcvae_init_state_dict() -> "OrderedDict[str, torch.Tensor]":
    """The state dict of a freshly constructed reference BCVAE(): after torch.manual_seed(s) it is bit-identical to the reference's."""
    return OrderedDict((k, v.detach().clone()) for k, v in _reference_modules().state_dict().items())


# ---------------------------------------------------------------------------------------------------------------- windows
def mirror_permutation(classes: Sequence[str] = DEFAULT_BLENDSHAPE_CLASSES,
                       pairs: Sequence[Tuple[str, str]] = DEFAULT_MIRROR_PAIRS) -> np.ndarray:
    """perm (C,) with flipped[:, c] = window[:, perm[c]]: coeffs_window[:, mirror_indices] = coeffs_window[:, mirror_indices_flip]."""
    perm = np.arange(len(classes), dtype=np.int32)
    for left, right in pairs:
        il, ir = classes.index(left), classes.index(right)
        perm[il], perm[ir] = ir, il
    return perm


def get_data_paths(coeffs_dir: str, person_ids: Sequence[str], sentence_ids: Iterable[int] = SENTENCE_IDS) -> List[Tuple[str, int, str]]:
    """(person id, sentence id, path) of every `sentenceNN(-.+)?.csv` under `<coeffs_dir>/<pid>/`, persons and sentences in the given order,
    files of one sentence in os.listdir order (BlendVOCAVAEDataset.get_data_paths)."""
    out = []
    for pid in person_ids:
        d = os.path.join(coeffs_dir, pid)
        if not os.path.exists(d):
            continue
        names = os.listdir(d)
        for sid in sentence_ids:
            pat = re.compile(rf"^sentence{sid:02}(-.+)?\.csv$")
            for name in names:
                if pat.match(name) and os.path.exists(os.path.join(d, name)):
                    out.append((pid, sid, os.path.join(d, name)))
    return out


class VAEWindowDataset(Dataset):
    """BlendVOCAVAEDataset (dataset_voca.py:1090-1264) with the windows cut on the device.  ``dataset[i]`` makes the reference's draws for
    sequence i and returns int32 (i, bdx, flip, zero); ``window(item)`` cuts that window on the host."""

    def __init__(self, coeffs_dir: Optional[str] = None, window_size: int = 120, zero_prob: float = 0.0, hflip: bool = True,
                 dataset_type: str = "train", classes: Sequence[str] = DEFAULT_BLENDSHAPE_CLASSES,
                 classes_mirror_pair: Sequence[Tuple[str, str]] = DEFAULT_MIRROR_PAIRS, sequences: Optional[List[np.ndarray]] = None):
        if window_size != 120:
            raise ValueError("the BCVAE trains on windows of 120 frames")
        self.window_size, self.zero_prob, self.hflip = window_size, float(zero_prob), bool(hflip)
        self.mirror = mirror_permutation(list(classes), list(classes_mirror_pair))
        if sequences is None:
            ids = {"train": PERSON_IDS_TRAIN, "val": PERSON_IDS_VAL}.get(dataset_type, PERSON_IDS_TEST)
            self.data_paths = get_data_paths(coeffs_dir, ids)
            sequences = [load_blendshape_coeffs(p).numpy() for _, _, p in self.data_paths]
        else:
            self.data_paths = []
        self.sequences = [np.ascontiguousarray(s, dtype=np.float32) for s in sequences]
        for i, s in enumerate(self.sequences):
            if s.ndim != 2 or s.shape[1] != len(classes) or s.shape[0] < 1:
                raise ValueError(f"sequence {i} has shape {s.shape}, expected (T >= 1, {len(classes)})")

    def __len__(self) -> int:
        return len(self.sequences)

    def __getitem__(self, index: int) -> np.ndarray:
        n = self.sequences[index].shape[0]
        half = self.window_size // 2
        bdx = random.randint(-half, max(0, n - half - 1))
        flip = bool(self.hflip and random.uniform(0, 1) < 0.5)
        zero = random.uniform(0, 1) < self.zero_prob
        return np.array([index, bdx, int(flip), int(zero)], dtype=np.int32)

    def window(self, item: Sequence[int]) -> np.ndarray:
        """(120, C) window of item (i, bdx, flip, zero): replication padding of 60 frames before and 120 after, then the flip and the zero-out."""
        s = self.sequences[int(item[0])]
        half = self.window_size // 2
        padded = np.concatenate([np.repeat(s[:1], half, 0), s, np.repeat(s[-1:], self.window_size, 0)], 0)
        w = padded[int(item[1]) + half: int(item[1]) + half + self.window_size].copy()
        if item[2]:
            w = w[:, self.mirror]
        if item[3]:
            w = np.zeros_like(w)
        return w

    def packed(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(frames (sum T, C), offsets, lengths) for the device."""
        lengths = np.array([s.shape[0] for s in self.sequences], dtype=np.int32)
        offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        return np.concatenate(self.sequences, 0), offsets, lengths

    @staticmethod
    def collate_fn(items: List[np.ndarray]) -> np.ndarray:
        return np.stack(items)


def make_dataloaders(train_dataset: VAEWindowDataset, val_dataset: Optional[VAEWindowDataset], batch_size: int):
    """The reference's loaders: RandomSampler(replacement=True, num_samples=len) in batches of `batch_size` (the last may be short);
    validation in order, batch 1."""
    sampler = RandomSampler(train_dataset, replacement=True, num_samples=len(train_dataset))
    train = DataLoader(train_dataset, batch_size=batch_size, sampler=sampler, collate_fn=VAEWindowDataset.collate_fn)
    val = None if val_dataset is None else DataLoader(val_dataset, batch_size=1, shuffle=False, collate_fn=VAEWindowDataset.collate_fn)
    return train, val


# ---------------------------------------------------------------------------------------------------------------- trainer
class BCVAETrainer(TrainerBase):
    """BCVAE(channels=32, seq_len=120, z_dim=64) trained on one MI355X with the reference's step (script/train_vae.py).

    learning_rate, weight decay 0.01 and betas / eps are torch.optim.AdamW's; the LR follows constant_with_warmup with
    num_warmup_steps = 0.1 * num_training_steps; ema / ema_decay are EMAModel(params, decay=ema_decay).  `std` (32,) reweights the losses.
    """

    def __init__(self, device="cuda", max_batch: int = 8, learning_rate: float = 1e-4, num_training_steps: int = 1,
                 ema: bool = True, ema_decay: float = 0.99, std=None, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 weight_decay: float = 0.01, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, use_graph: bool = True):
        self.eng = _engine.TrainEngine(torch.device(device), max_batch)
        self.device = self.eng.device
        self.max_batch = int(max_batch)
        self.num_warmup_steps = 0.1 * num_training_steps
        self._set_optimizer(learning_rate, self.num_warmup_steps, weight_decay, betas, eps, ema, ema_decay)
        self.use_graph = bool(use_graph)
        self.std = parse_std(std)
        self._template = bcvae_init_state_dict() if state_dict is None else None
        self.load_state_dict(self._template if state_dict is None else state_dict)
        self._has_train, self._has_val = False, False

    # ---- state
    @property
    def param_names(self) -> List[str]:
        return [n for n, _, c in self.eng.tensors if not (c or n.endswith("running_mean") or n.endswith("running_var"))]

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor]) -> None:
        """Set the model state (all 70 reference keys, strict) and restart the optimizer: zero moments, the EMA shadow a copy of the
        parameters, step count 0."""
        names = self.names
        missing, unexpected = [n for n in names if n not in state_dict], [k for k in state_dict if k not in names]
        if missing or unexpected:
            raise KeyError(f"BCVAE state dict mismatch: missing {missing[:4]}, unexpected {unexpected[:4]}")
        self._shapes = OrderedDict()
        for name, numel, _ in self.eng.tensors:
            v = state_dict[name].detach().cpu()
            if v.numel() != numel:
                raise ValueError(f"{name}: {v.numel()} elements, expected {numel}")
            self._shapes[name] = tuple(v.shape)
            self.eng.set_tensor(_engine.TRAIN_STATE, name, v.numpy())
        self.eng.reset_optimizer()
        self.step_count = 0

    def state_dict(self, ema: bool = True) -> "OrderedDict[str, torch.Tensor]":
        """The checkpoint layout: the 70 reference keys; parameters from the EMA shadow when ema (and the trainer keeps one), running
        statistics and num_batches_tracked (int64) live."""
        use_ema = ema and self.ema
        out = OrderedDict()
        for name, _, counter in self.eng.tensors:
            is_param = not (counter or name.endswith("running_mean") or name.endswith("running_var"))
            out[name] = self._get(_engine.TRAIN_EMA if (use_ema and is_param) else _engine.TRAIN_STATE, name)
        return out

    # ---- data
    def set_train_data(self, dataset: VAEWindowDataset) -> None:
        self.eng.set_data(_engine.TRAIN_SET_TRAIN, *dataset.packed(), dataset.mirror)
        self._has_train = True

    def set_val_data(self, dataset: VAEWindowDataset) -> None:
        self.eng.set_data(_engine.TRAIN_SET_VAL, *dataset.packed(), dataset.mirror)
        self._has_val = True

    # ---- the step
    def _scalars(self, beta: float, weight_vel: float, k: int) -> np.ndarray:
        """SAID_TRAIN_S_* for optimizer step k (0-based), in double as torch / diffusers compute them."""
        s = self._optimizer_scalars(k)
        s[_engine.TRAIN_S_BETA] = beta
        s[_engine.TRAIN_S_WVEL] = weight_vel
        return s.astype(np.float32)

    def _items(self, items) -> np.ndarray:
        it = np.asarray(items, dtype=np.int32)
        if it.ndim != 2 or it.shape[1] != _engine.TRAIN_ITEM:
            raise ValueError(f"items must be (B, 4) (sequence, bdx, flip, zero), got {it.shape}")
        return it

    def _eps(self, eps, B: int) -> np.ndarray:
        if eps is None:   # the reference's draw: torch.randn(B, z_dim) on the CPU generator (vae.py:110)
            eps = torch.randn(B, 64)
        e = np.asarray(torch.as_tensor(eps, dtype=torch.float32).cpu(), dtype=np.float32)
        if e.shape != (B, 64):
            raise ValueError(f"eps must be ({B}, 64), got {e.shape}")
        return e

    def _step(self, items, eps, beta: float, weight_vel: float) -> None:
        it = self._items(items)
        B = it.shape[0]
        if B == 1:
            raise ValueError("Expected more than 1 value per channel when training: a batch of 1 cannot train the BCVAE "
                             "(its linear layers' BatchNorm1d normalises over the batch)")
        if not self._has_train:
            raise RuntimeError("no training set on the device: call set_train_data first")
        e = self._eps(eps, B)
        self.eng.step(it, e, self._scalars(beta, weight_vel, self.step_count), self.std, use_graph=self.use_graph)
        self.step_count += 1

    def step(self, items, eps=None, beta: float = 1.0, weight_vel: float = 1.0) -> LossStepOutput:
        """One optimizer step on the windows `items` (B, 4) of the training set; reads the step's losses back (one host sync)."""
        self._step(items, eps, beta, weight_vel)
        rec, reg, vel, _ = self.eng.last_losses()
        return LossStepOutput(reconst=torch.tensor(rec), regularize=torch.tensor(reg), velocity=torch.tensor(vel))

    def _epoch_output(self, val: bool, lr: Optional[float]) -> LossEpochOutput:
        acc = self._epoch_sums(val)
        n = acc[4]
        return LossEpochOutput(total=acc[3] / n, reconst=acc[0] / n, regularize=acc[1] / n, velocity=acc[2] / n, lr=lr)

    def train_epoch(self, train_dataloader: Iterable, beta: float, weight_vel: float) -> LossEpochOutput:
        """train_epoch of script/train_vae.py: one step per batch, losses read once at the end; lr is the LR after the last step."""
        for items in train_dataloader:
            self._step(items, None, beta, weight_vel)
        return self._epoch_output(False, self.lr_at(self.step_count))

    def validate_epoch(self, val_dataloader: Iterable, beta: float, weight_vel: float, num_repeat: int = 1,
                       use_ema: Optional[bool] = None) -> LossEpochOutput:
        """validate_epoch of script/train_vae.py: eval-mode BatchNorm, use_noise=True; with the EMA parameters (and live running
        statistics) when the trainer keeps an EMA, as the reference swaps them in."""
        if not self._has_val:
            raise RuntimeError("no validation set on the device: call set_val_data first")
        ema = self.ema if use_ema is None else bool(use_ema)
        sc = self._scalars(beta, weight_vel, self.step_count)
        for _ in range(num_repeat):
            for items in val_dataloader:
                it = self._items(items)
                self.eng.eval_loss(_engine.TRAIN_SET_VAL, it, self._eps(None, it.shape[0]), sc, self.std, ema)
        return self._epoch_output(True, None)
