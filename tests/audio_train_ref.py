"""Restatement of the audio encoder's train-mode forward (include/said_audio_train.h) with explicit inputs — TEST INFRASTRUCTURE.

transformers 4.30.2's ``Wav2Vec2Model`` in ``train()`` (post-LN encoder) over the reference's interpolating forward, from the pieces of
oracle/wav2vec2.py: the span mask, the skipped layers, the dropout seed and the four probabilities are arguments, and the dropout masks
are the engine's Philox masks (tests/philox_ref.py), so the whole forward is a function that float64 can evaluate.  ``dtype`` float32
gives the CPU fp32 evaluation of the same function, whose error against float64 is the yardstick of tests/test_gpu_audio_train.py.
With every probability 0, no mask and no skips this is oracle.wav2vec2.wav2vec2_forward operation for operation.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import wav2vec2 as ow
from philox_ref import philox4x32_10

SITE_FEAT_PROJ, SITE_FRONT = 0, 1
KINDS = {"feat_proj": 1, "front": 2, "attention": 4, "attn_out": 8, "activation": 16, "ffn_out": 32}   # the bits of said_debug_option "audio_train_sites"


def layer_site(layer: int, which: int) -> int:
    """which: 0 probabilities, 1 attention output, 2 activation, 3 FFN output"""
    return 16 + 4 * layer + which


def _keep(words: np.ndarray, p: float) -> np.ndarray:
    """float32 keep factors of Philox words: u = (word >> 8) 2^-24, kept iff u >= p, a kept element times fp32(1 / (1 - p))."""
    p32 = np.float32(p)
    u = (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.where(u >= p32, np.float32(1) / (np.float32(1) - p32), np.float32(0))


def elementwise_factors(seed: int, site: int, shape, p: float) -> np.ndarray:
    """Keep factors of a (B, T, C) site: element e of the flattened tensor is word e & 3 of counter (site, e >> 2, 0, 0)."""
    n = int(np.prod(shape))
    assert n % 4 == 0 and n < 2 ** 32
    c1 = np.arange(n // 4, dtype=np.uint32)
    z = np.zeros_like(c1)
    w = philox4x32_10(z + np.uint32(site), c1, z, z, np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))
    return _keep(np.stack(w, axis=1).reshape(n), p).reshape(shape)


def attention_factors(seed: int, site: int, B: int, heads: int, T: int, p: float) -> np.ndarray:
    """Keep factors (B, heads, T, T) of the attention probabilities: query i, key j of (b, head) is word j & 3 of counter
    (site, (b heads + head) T + i, j >> 2, 0)."""
    rows = B * heads * T
    assert rows < 2 ** 32
    nj = (T + 3) // 4
    c1 = np.repeat(np.arange(rows, dtype=np.uint32), nj)
    c2 = np.tile(np.arange(nj, dtype=np.uint32), rows)
    z = np.zeros_like(c1)
    w = philox4x32_10(z + np.uint32(site), c1, c2, z, np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))
    return _keep(np.stack(w, axis=1).reshape(rows, 4 * nj)[:, :T], p).reshape(B, heads, T, T)


def _drop(x: torch.Tensor, seed: int, site: int, p: float) -> torch.Tensor:
    if p <= 0:
        return x
    return x * torch.from_numpy(elementwise_factors(seed, site, tuple(x.shape), p)).to(x.dtype)


def attention(sd, pfx, x, seed, site, p):
    """oracle.wav2vec2.attention with dropout on the normalised probabilities."""
    b, t, c = x.shape
    d = c // ow.HEADS
    q = F.linear(x, sd[pfx + ".q_proj.weight"], sd[pfx + ".q_proj.bias"]) * (d ** -0.5)
    k = F.linear(x, sd[pfx + ".k_proj.weight"], sd[pfx + ".k_proj.bias"])
    v = F.linear(x, sd[pfx + ".v_proj.weight"], sd[pfx + ".v_proj.bias"])

    def split(z):
        return z.view(b, t, ow.HEADS, d).transpose(1, 2)

    w = torch.matmul(split(q), split(k).transpose(2, 3)).softmax(dim=-1)
    if p > 0:
        w = w * torch.from_numpy(attention_factors(seed, site, b, ow.HEADS, t, p)).to(w.dtype)
    o = torch.matmul(w, split(v)).transpose(1, 2).reshape(b, t, c)
    return F.linear(o, sd[pfx + ".out_proj.weight"], sd[pfx + ".out_proj.bias"])


def encoder_layer(sd, pfx, x, layer, seed, p_attention, p_attn_out, p_activation, p_ffn_out):
    c = x.shape[-1]
    a = attention(sd, pfx + ".attention", x, seed, layer_site(layer, 0), p_attention)
    x = x + _drop(a, seed, layer_site(layer, 1), p_attn_out)
    x = F.layer_norm(x, (c,), sd[pfx + ".layer_norm.weight"], sd[pfx + ".layer_norm.bias"], ow.LN_EPS)
    f = F.linear(x, sd[pfx + ".feed_forward.intermediate_dense.weight"], sd[pfx + ".feed_forward.intermediate_dense.bias"])
    f = _drop(F.gelu(f), seed, layer_site(layer, 2), p_activation)
    f = F.linear(f, sd[pfx + ".feed_forward.output_dense.weight"], sd[pfx + ".feed_forward.output_dense.bias"])
    x = x + _drop(f, seed, layer_site(layer, 3), p_ffn_out)
    return F.layer_norm(x, (c,), sd[pfx + ".final_layer_norm.weight"], sd[pfx + ".final_layer_norm.bias"], ow.LN_EPS)


def features(sd, input_values, num_frames, dtype=torch.float64):
    """(B, frames, 512) conv features after the interpolation: the part of the forward that train mode leaves alone."""
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith("feature_extractor.")}
    h = ow.feature_extractor(sd, input_values.to(dtype))
    if num_frames is not None:
        h = F.interpolate(h, size=num_frames, align_corners=True, mode="linear")
    return h.transpose(1, 2)


def forward(sd, input_values, num_frames, mask=None, skip=(), seed=0, p_feat_proj=0.0, p_hidden=0.0, p_attention=0.0, p_activation=0.0,
            dtype=torch.float64, feats=None, kinds=None):
    """(B, frames, 768) last hidden state.  sd: the encoder's state dict without the ``audio_encoder.`` prefix; mask: (B, frames) bool or
    None; skip: layer indices (or one bool per layer) that LayerDrop skips.  feats: features(...) of the same inputs and dtype, if the
    caller has them already.  kinds: the kinds of dropout site that draw a mask, a subset of KINDS (None: all) — p_hidden serves three of
    them, which said_debug_option "audio_train_sites" tells apart in the same way."""
    on = lambda kind, p: p if (kinds is None or kind in kinds) else 0.0
    h = features(sd, input_values, num_frames, dtype) if feats is None else feats
    sd = {k: v.to(dtype) for k, v in sd.items() if not k.startswith("feature_extractor.")}
    c = h.shape[-1]
    h = F.layer_norm(h, (c,), sd["feature_projection.layer_norm.weight"], sd["feature_projection.layer_norm.bias"], ow.LN_EPS)
    h = F.linear(h, sd["feature_projection.projection.weight"], sd["feature_projection.projection.bias"])
    h = _drop(h, seed, SITE_FEAT_PROJ, on("feat_proj", p_feat_proj))
    if mask is not None:
        h = h.clone()
        h[torch.as_tensor(np.asarray(mask), dtype=torch.bool)] = sd["masked_spec_embed"]
    w = ow.pos_conv_weight(sd)
    k = w.shape[-1]
    groups = h.shape[-1] // w.shape[1]
    pos = F.conv1d(h.transpose(1, 2), w, sd["encoder.pos_conv_embed.conv.bias"], padding=k // 2, groups=groups)
    if k % 2 == 0:
        pos = pos[:, :, :-1]
    pos = F.gelu(pos).transpose(1, 2)
    h = h + pos
    H = h.shape[-1]
    h = F.layer_norm(h, (H,), sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"], ow.LN_EPS)
    h = _drop(h, seed, SITE_FRONT, on("front", p_hidden))
    n = ow.num_layers(sd)
    skip = list(skip)
    skipped = {l for l in range(n) if skip[l]} if len(skip) == n and all(isinstance(v, (bool, np.bool_)) for v in skip) else set(skip)
    for l in range(n):
        if l not in skipped:
            h = encoder_layer(sd, f"encoder.layers.{l}", h, l, seed, on("attention", p_attention), on("attn_out", p_hidden),
                              on("activation", p_activation), on("ffn_out", p_hidden))
    return h
