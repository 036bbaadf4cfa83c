"""A functional restatement of the reference's BCVAE training step, for tests and measurements (float64 by default).

The forward is said/model/vae.py written with torch.nn.functional on a dict of tensors; the loss is elbo_loss of script/train_vae.py with the
reweighting done out of place; the step is torch's own clip_grad_norm_ and AdamW, the LR lambda of constant_with_warmup and the EMA of
diffusers' EMAModel restated (said_amd/util/scheduler.py).  It runs on the CPU (or any torch device) and needs neither the reference nor
the HIP library.  Pinned to the reference by tests/golden/g14_vae_train.npz (tests/golden/make_golden_g14.py).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from said_amd.util.scheduler import constant_with_warmup_lambda, ema_decay

BN_LAYERS = ["encoder.conv_layers.1", "encoder.conv_layers.4", "encoder.conv_layers.7", "encoder.fc_layers.1", "encoder.fc_layers.4",
             "decoder.fc_layers.1", "decoder.conv_layers.1", "decoder.conv_layers.4"]


def is_param(name: str) -> bool:
    return not (name.endswith("running_mean") or name.endswith("running_var") or name.endswith("num_batches_tracked"))


def split_state(sd: Dict[str, torch.Tensor], dtype=torch.float64, device="cpu"):
    """(params, buffers): leaf tensors that require grad, and the running statistics (num_batches_tracked int64)."""
    params, bufs = OrderedDict(), OrderedDict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            bufs[k] = v.detach().clone().to(device)
        elif is_param(k):
            params[k] = v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
        else:
            bufs[k] = v.detach().to(device=device, dtype=dtype).clone()
    return params, bufs


def forward(p, bufs, x, eps, train: bool = True):
    """(mean, log_var, coeffs_reconst) of BCVAE.forward(x, use_noise=True) with the given noise; train: batch statistics, running stats
    and num_batches_tracked updated (BatchNorm1d in training mode)."""

    def bn(h, name, slope):
        if train:
            bufs[name + ".num_batches_tracked"] += 1
        h = F.batch_norm(h, bufs[name + ".running_mean"], bufs[name + ".running_var"], p[name + ".weight"], p[name + ".bias"], training=train,
                         momentum=0.1, eps=1e-5)
        return F.leaky_relu(h, slope)

    def conv(h, name, stride=1):
        return F.conv1d(h, p[name + ".weight"], p[name + ".bias"], stride=stride)

    def lin(h, name):
        return F.linear(h, p[name + ".weight"], p[name + ".bias"])

    h = x.transpose(1, 2)
    h = bn(conv(h, "encoder.conv_layers.0"), "encoder.conv_layers.1", 0.2)
    h = bn(conv(h, "encoder.conv_layers.3"), "encoder.conv_layers.4", 0.2)
    h = bn(conv(h, "encoder.conv_layers.6", 2), "encoder.conv_layers.7", 0.2)
    h = conv(h, "encoder.conv_layers.9").flatten(1)
    h = bn(lin(h, "encoder.fc_layers.0"), "encoder.fc_layers.1", 0.01)
    h = bn(lin(h, "encoder.fc_layers.3"), "encoder.fc_layers.4", 0.01)
    h = lin(h, "encoder.fc_layers.6")
    mean, log_var = lin(h, "encoder.fc_mu"), lin(h, "encoder.fc_logvar")
    z = mean + torch.exp(0.5 * log_var) * eps
    h = bn(lin(z, "decoder.fc_layers.0"), "decoder.fc_layers.1", 0.01)
    h = lin(h, "decoder.fc_layers.3").unflatten(1, (4, -1))
    h = bn(F.conv_transpose1d(h, p["decoder.conv_layers.0.weight"], p["decoder.conv_layers.0.bias"]), "decoder.conv_layers.1", 0.2)
    h = bn(F.conv_transpose1d(h, p["decoder.conv_layers.3.weight"], p["decoder.conv_layers.3.bias"]), "decoder.conv_layers.4", 0.2)
    h = conv(conv(h, "decoder.conv_layers.6"), "decoder.conv_layers.7")
    y = torch.tanh(torch.relu(h)).transpose(1, 2)
    return mean, log_var, y


def encode_eval(p, bufs, x):
    """Eval-mode (mean, log_var) of BCVAE.encode."""
    with torch.no_grad():
        mean, log_var, _ = forward(p, bufs, x, torch.zeros(x.shape[0], 64, dtype=x.dtype), train=False)
    return mean, log_var


def elbo(x, mean, log_var, y, std: Optional[torch.Tensor] = None):
    """(reconst, kld, vel) of elbo_loss; with std, x / std and y / std out of place."""
    B = x.shape[0]
    a, pr = (x, y) if std is None else (x / std.view(1, 1, -1), y / std.view(1, 1, -1))
    reconst = 0.5 * ((a - pr) ** 2).sum() / B
    kld = 0.5 * torch.mean(torch.sum(mean ** 2 + torch.exp(log_var) - log_var - 1, dim=1))
    da, dp = a[:, 1:] - a[:, :-1], pr[:, 1:] - pr[:, :-1]
    vel = 0.5 * ((dp - da) ** 2).sum() / B
    return reconst, kld, vel


class RefTrainer:
    """The reference step on the restated forward: backward, clip_grad_norm_(1.0), AdamW (torch defaults but lr), EMA, LR lambda."""

    def __init__(self, sd, lr=1e-4, num_training_steps=1, ema_decay_=0.99, dtype=torch.float64, device="cpu", std=None):
        self.params, self.bufs = split_state(sd, dtype, device)
        self.plist = list(self.params.values())
        self.opt = torch.optim.AdamW(self.plist, lr=lr)
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.opt, constant_with_warmup_lambda(0.1 * num_training_steps))
        self.shadow = [q.detach().clone() for q in self.plist]
        self.ema_decay, self.n_ema = ema_decay_, 0
        self.dtype, self.device = dtype, device
        self.std = None if std is None else torch.as_tensor(std, dtype=dtype, device=device).reshape(-1)
        self.last_grads = None

    def step(self, x, eps, beta=1.0, weight_vel=1.0):
        x = torch.as_tensor(x).to(self.device, self.dtype)
        eps = torch.as_tensor(eps).to(self.device, self.dtype)
        with torch.enable_grad():
            mean, log_var, y = forward(self.params, self.bufs, x, eps, train=True)
            reconst, kld, vel = elbo(x, mean, log_var, y, self.std)
            loss = reconst + beta * kld + weight_vel * vel
            loss.backward()
        self.last_grads = OrderedDict((k, v.grad.detach().clone()) for k, v in self.params.items())
        torch.nn.utils.clip_grad_norm_(self.plist, 1.0)
        self.opt.step()
        self.n_ema += 1
        d = ema_decay(self.n_ema, self.ema_decay)
        with torch.no_grad():
            for s, q in zip(self.shadow, self.plist):
                s.sub_((1 - d) * (s - q))
        self.sched.step()
        self.opt.zero_grad()
        return np.array([float(v.detach()) for v in (reconst, kld, vel, loss)])

    def state(self, ema=False):
        out = OrderedDict()
        for k, v in self.params.items():
            out[k] = v.detach().clone()
        if ema:
            for (k, _), s in zip(self.params.items(), self.shadow):
                out[k] = s.clone()
        out.update((k, v.clone()) for k, v in self.bufs.items())
        return out


def windows_of(seqs, items, mirror):
    """(B, 120, 32) windows of items (seq, bdx, flip, zero) cut from seqs as BlendVOCAVAEDataset.__getitem__ does."""
    out = []
    for s_, bdx, flip, zero in np.asarray(items):
        s = np.asarray(seqs[s_])
        padded = np.concatenate([np.repeat(s[:1], 60, 0), s, np.repeat(s[-1:], 120, 0)], 0)
        w = padded[bdx + 60: bdx + 180].copy()
        if flip:
            w = w[:, mirror]
        if zero:
            w = np.zeros_like(w)
        out.append(w)
    return np.stack(out).astype(np.float32)
