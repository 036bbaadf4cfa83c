"""Restatement of the denoiser's training step in functional torch — TEST INFRASTRUCTURE.

The forward of oracle/unet.py in whatever dtype the state dict has (float64 for references, float32 to measure fp32's own error), with explicit
ResBlock dropout masks, the objective of random_noise_loss (script/train.py:45-155 of the reference, in-place reweighting included),
clip_grad_norm_(1.0), AdamW and EMAModel.step.  Gradients come from torch.autograd.  The sinusoidal timestep features are computed in fp32 in
every dtype, as the reference computes them: they are an input of the model, not part of its arithmetic.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from philox_ref import philox4x32_10

HEADS = 6
RES = ["denoiser.model.input_blocks.1.0", "denoiser.model.middle_block.0", "denoiser.model.middle_block.2",
       "denoiser.model.output_blocks.0.0", "denoiser.model.output_blocks.1.0"]


def timestep_embedding(timesteps, dim=192, max_period=10000):
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float32) / half).to(timesteps.device)
    args = timesteps[:, None].float() * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def alignment_band(x_len, c_len, pad=1):
    ratio = c_len / x_len
    kh = ratio / 2 + pad
    m = torch.ones(x_len, c_len, dtype=torch.bool)
    for i in range(x_len):
        mid = (i + 0.5) * ratio
        m[i, max(round(mid - kh), 0):min(round(mid + kh), c_len)] = False
    return m


def dropout_masks(seed, B, T, p):
    """The five ResBlock keep factors (B, T, 192) of the step's Philox stream: key = seed, counter = (ResBlock, (b T + t) 192 + c, 0, 0);
    kept iff (word 0 >> 8) 2^-24 >= p, scaled by the fp32 value of 1 / (1 - p)."""
    if p <= 0:
        return None
    elem = np.arange(B * T * 192, dtype=np.uint32)
    z = np.zeros_like(elem)
    p32 = np.float32(p)
    keep = np.float32(1) / (np.float32(1) - p32)
    out = []
    for layer in range(5):
        r0 = philox4x32_10(z + np.uint32(layer), elem, z, z, np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))[0]
        u = (r0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        out.append(torch.from_numpy(np.where(u >= p32, keep, np.float32(0)).astype(np.float64)).reshape(B, T, 192))
    return out


def _attention(sd, p, x, context, mask):
    q = F.linear(x, sd[p + ".to_q.weight"])
    c = x if context is None else context
    k, v = F.linear(c, sd[p + ".to_k.weight"]), F.linear(c, sd[p + ".to_v.weight"])
    b, n, _ = q.shape
    split = lambda t: t.reshape(b, t.shape[1], HEADS, -1).permute(0, 2, 1, 3)
    sim = torch.einsum("bhid,bhjd->bhij", split(q), split(k)) * (32 ** -0.5)
    if mask is not None:
        sim = sim.masked_fill(mask[None, None], -torch.finfo(sim.dtype).max)
    out = torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), split(v)).permute(0, 2, 1, 3).reshape(b, n, -1)
    return F.linear(out, sd[p + ".to_out.0.weight"], sd[p + ".to_out.0.bias"])


def _res(sd, p, x, emb, mask):
    h = F.silu(F.group_norm(x, 32, sd[p + ".in_layers.0.weight"], sd[p + ".in_layers.0.bias"], eps=1e-5))
    h = F.conv1d(h, sd[p + ".in_layers.2.weight"], sd[p + ".in_layers.2.bias"], padding=1)
    h = h + F.linear(F.silu(emb), sd[p + ".emb_layers.1.weight"], sd[p + ".emb_layers.1.bias"])[..., None]
    h = F.silu(F.group_norm(h, 32, sd[p + ".out_layers.0.weight"], sd[p + ".out_layers.0.bias"], eps=1e-5))
    if mask is not None:
        h = h * mask.transpose(1, 2).to(h.dtype)
    h = F.conv1d(h, sd[p + ".out_layers.3.weight"], sd[p + ".out_layers.3.bias"], padding=1)
    if (p + ".skip_connection.weight") in sd:
        x = F.conv1d(x, sd[p + ".skip_connection.weight"], sd[p + ".skip_connection.bias"])
    return x + h


def _st(sd, p, x, context, band):
    b = p + ".transformer_blocks.0"
    h = F.group_norm(x, 32, sd[p + ".norm.weight"], sd[p + ".norm.bias"], eps=1e-6).transpose(1, 2)
    ln = lambda t, n: F.layer_norm(t, (192,), sd[f"{b}.{n}.weight"], sd[f"{b}.{n}.bias"])
    h = _attention(sd, b + ".attn1", ln(h, "norm1"), None, None) + h
    h = _attention(sd, b + ".attn2", ln(h, "norm2"), context, band) + h
    y = F.linear(ln(h, "norm3"), sd[b + ".ff.net.0.proj.weight"], sd[b + ".ff.net.0.proj.bias"])
    a, gate = y.chunk(2, dim=-1)
    h = F.linear(a * F.gelu(gate), sd[b + ".ff.net.2.weight"], sd[b + ".ff.net.2.bias"]) + h
    return F.conv1d(h.transpose(1, 2), sd[p + ".proj_out.weight"], sd[p + ".proj_out.bias"]) + x


def forward(sd, sample, timesteps, audio, cond, masks=None):
    """Model output (B, T, 32).  sd: trainable tensors (null_cond_emb, denoiser.model.*) in the working dtype; cond (B,) bool selects the audio
    embedding or null_cond_emb; masks: dropout_masks(...) or None."""
    dt = sd["null_cond_emb"].dtype
    m = "denoiser.model."
    cm = torch.as_tensor(cond, dtype=torch.bool, device=audio.device).view(-1, 1, 1)
    ctx = torch.where(cm, audio.to(dt), sd["null_cond_emb"].expand(audio.shape[0], audio.shape[1], -1))
    band = alignment_band(sample.shape[1], ctx.shape[1]).to(ctx.device)
    e = timestep_embedding(timesteps).to(dt)
    emb = F.linear(F.silu(F.linear(e, sd[m + "time_embed.0.weight"], sd[m + "time_embed.0.bias"])), sd[m + "time_embed.2.weight"], sd[m + "time_embed.2.bias"])
    mk = (lambda i: None) if masks is None else (lambda i: masks[i])
    h0 = F.conv1d(sample.to(dt).transpose(1, 2), sd[m + "input_blocks.0.0.weight"], sd[m + "input_blocks.0.0.bias"], padding=1)
    s1 = _st(sd, m + "input_blocks.1.1", _res(sd, RES[0], h0, emb, mk(0)), ctx, band)
    h = _st(sd, m + "middle_block.1", _res(sd, RES[1], s1, emb, mk(1)), ctx, band)
    h = _res(sd, RES[2], h, emb, mk(2))
    h = _st(sd, m + "output_blocks.0.1", _res(sd, RES[3], torch.cat([h, s1], 1), emb, mk(3)), ctx, band)
    h = _st(sd, m + "output_blocks.1.1", _res(sd, RES[4], torch.cat([h, h0], 1), emb, mk(4)), ctx, band)
    h = F.silu(F.group_norm(h, 32, sd[m + "out.0.weight"], sd[m + "out.0.bias"], eps=1e-5))
    return F.conv1d(h, sd[m + "out.2.weight"], sd[m + "out.2.bias"], padding=1).transpose(1, 2)


def add_noise(alphas_cumprod, x0, noise, timesteps, prediction_type, dt):
    """(noisy, answer): diffusers' add_noise / get_velocity with the fp32 square roots of the fp32 alphas_cumprod."""
    ac = alphas_cumprod.float()[timesteps]
    sa, sb = (ac ** 0.5).to(dt).view(-1, 1, 1), ((1 - ac) ** 0.5).to(dt).view(-1, 1, 1)
    x0, noise = x0.to(dt), noise.to(dt)
    noisy = sa * x0 + sb * noise
    answer = {"epsilon": noise, "sample": x0, "v_prediction": sa * noise - sb * x0}[prediction_type]
    return noisy, answer


def objective(pred, answer, std=None, deltas=None):
    """(predict, velocity, vertex | None) of random_noise_loss: with std, answer and pred are divided in place, so the vertex term sees the
    reweighted tensors.  deltas: (B, 32, 3 V), already normalised."""
    if std is not None:
        answer = answer / std.to(pred.dtype).view(1, 1, -1)
        pred = pred / std.to(pred.dtype).view(1, 1, -1)
    lp = F.l1_loss(pred, answer)
    lv = F.l1_loss(pred[:, 1:] - pred[:, :-1], answer[:, 1:] - answer[:, :-1])
    lx = None
    if deltas is not None:
        d = deltas.to(pred.dtype)
        lx = F.l1_loss(torch.bmm(pred, d), torch.bmm(answer, d))
    return lp, lv, lx


def total_loss(losses, weight_vel=1.0, weight_vertex=0.02):
    lp, lv, lx = losses
    return lp + weight_vel * lv + (weight_vertex * lx if lx is not None else 0.0)


def loss_and_grads(sd, alphas_cumprod, coeffs, noise, timesteps, audio, cond, prediction_type="epsilon", std=None, deltas=None, masks=None,
                   weight_vel=1.0, weight_vertex=0.02):
    """(losses, {name: gradient}) by autograd in sd's dtype."""
    dt = sd["null_cond_emb"].dtype
    with torch.enable_grad():   # other test modules of the suite switch autograd off process-wide
        p = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
        noisy, answer = add_noise(alphas_cumprod, coeffs, noise, timesteps, prediction_type, dt)
        losses = objective(forward(p, noisy, timesteps, audio, cond, masks), answer, std, deltas)
        total_loss(losses, weight_vel, weight_vertex).backward()
    return [None if l is None else l.detach() for l in losses], {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}


class RefTrainer:
    """clip_grad_norm_(1.0), torch.optim.AdamW (single-tensor form) and EMAModel.step on autograd's gradients, in sd's dtype."""

    def __init__(self, sd, lr, lr_lambda, ema_decay_fn, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8):
        self.p = {k: v.clone() for k, v in sd.items()}
        self.m = {k: torch.zeros_like(v) for k, v in sd.items()}
        self.v = {k: torch.zeros_like(v) for k, v in sd.items()}
        self.ema = {k: v.clone() for k, v in sd.items()}
        self.lr, self.lr_lambda, self.ema_decay_fn, self.wd, self.betas, self.eps, self.k = lr, lr_lambda, ema_decay_fn, weight_decay, betas, eps, 0
        self.clip_factors = []

    def step(self, *args, **kw):
        losses, g = loss_and_grads(self.p, *args, **kw)
        total = torch.sqrt(sum((x.norm() ** 2 for x in g.values())))
        cf = min(1.0, 1.0 / (float(total) + 1e-6))
        self.clip_factors.append(cf)
        b1, b2 = self.betas
        lr, n = self.lr * self.lr_lambda(self.k), self.k + 1
        omd = 1 - self.ema_decay_fn(n)
        for k in self.p:
            gk = g[k] * cf
            self.p[k] = self.p[k] * (1 - lr * self.wd)
            self.m[k] = self.m[k] + (1 - b1) * (gk - self.m[k])
            self.v[k] = self.v[k] * b2 + (1 - b2) * gk * gk
            den = self.v[k].sqrt() / math.sqrt(1 - b2 ** n) + self.eps
            self.p[k] = self.p[k] - (lr / (1 - b1 ** n)) * (self.m[k] / den)
            self.ema[k] = self.ema[k] - omd * (self.ema[k] - self.p[k])
        self.k += 1
        self.last_grads = g
        return losses
