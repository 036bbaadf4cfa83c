"""Launch-by-launch restatement of the fp32 audio encoder (said_amd/csrc/audio_enc.cpp, fp32 branch) — TEST INFRASTRUCTURE.

One function per launch of said_audio_encode / said_audio_extract_features in fp32 mode (the stage order of said_debug_option "audio_stop_after",
said_hip_debug.h).  Each takes the launch's inputs AS THE ENGINE STORES THEM, in the kernel's layouts, plus the audio state dict (keys without the
"audio_encoder." prefix), and returns what the kernel should store in the rows it owns:

  channel-major   (B, C, pitch) fp32, pitch = the valid length rounded up to 32; the functions read [..., :T] only — what lies in T .. pitch is
                  whatever an earlier call left and must not matter — and return (B, C, T);
  aQK             (B, 24, rows, 64): heads of q then of k, token-major per head, rows = pitch; q is NOT scaled (attention applies 64 ** -0.5);
  V               (B, 768, pitch): channel-major, head h in channels 64 h .. 64 h + 63.

dtype = torch.float64 is the reference (operands unrounded: both fp32 modes multiply at fp32 grade, split-fp16 or fp32 MFMAs), dtype = torch.float32
the torch CPU twin that says how far a correct fp32 evaluation of the identical inputs may sit from it.  Chained without the layouts' padding the
functions are oracle/wav2vec2.py::wav2vec2_forward (tests/test_audio_f32_ref_cpu.py).  `defect`: a named wrong variant of the launch, for that
module's mutant test only.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from audio_bf16_ref import (CONV, CONV_K, CONV_S, FFN, H, HD, HEADS, LN_EPS, POS_CG, POS_G, audio_sd, check_exact, check_f32, conv_lengths,  # noqa: F401
                            f32_bound, qkv_weight, rel_max)

# stage numbers of the fp32 branch (said_hip_debug.h)
ST_CONV0, ST_NORM, ST_CONV1, ST_INTERP, ST_FPROJ, ST_POS, ST_ENC_LN, ST_LAYER0 = 0, 1, 2, 8, 9, 10, 11, 12
LY_QKV, LY_ATTN, LY_OUT, LY_LN1, LY_FF1, LY_FF2, LY_LN2 = range(7)
LY_STAGES = 7


def pitch_of(T: int) -> int:
    return (T + 31) // 32 * 32


# The shapes tests/test_gpu_audio_f32_kernels.py runs, each with the plan it is there for (asserted against said_amd/csrc/audio_plan.h by
# tests/test_audio_plan_cpu.py): B clips of Ta samples, `frames` (None: no interpolation), clips per pass, the passes, token tiles of the first
# pass, and per launch site the (NB, KS) cgemm_kernel runs on / the key slices of attention.
def _plan(convs, hidden, ff1, qkv, pos_nb, attn):
    """convs: the shapes of conv1, conv2, ... as far as they differ from (1, 8)."""
    p = {f"conv{i}": (convs[i - 1] if i <= len(convs) else (1, 8)) for i in range(1, 7)}
    p.update(fproj=hidden, out=hidden, ff2=hidden, ff1=ff1, qkv=qkv, pos=(pos_nb, 8), proj=(1, 8), attn=attn)
    return p


SHAPES = {
    "S": dict(B=3, Ta=16000, frames=59, chunk=32, passes=[3], tiles=6, plan=_plan([(2, 8)], (1, 8), (1, 8), (2, 8), 1, 8)),
    "N": dict(B=2, Ta=8000, frames=None, chunk=32, passes=[2], tiles=2, plan=_plan([], (1, 8), (1, 8), (2, 8), 1, 8)),
    "M": dict(B=1, Ta=4000, frames=599, chunk=32, passes=[1], tiles=19, plan=_plan([], (1, 8), (2, 8), (2, 8), 1, 8)),
    "D": dict(B=9, Ta=4000, frames=599, chunk=32, passes=[9], tiles=171, plan=_plan([(2, 8)], (6, 4), (6, 4), (6, 4), 2, 4)),
    "C": dict(B=9, Ta=16000, frames=59, chunk=32, passes=[9], tiles=18, plan=_plan([(4, 4), (2, 8), (2, 8)], (1, 8), (2, 8), (2, 8), 1, 8)),
    "K": dict(B=86, Ta=1000, frames=250, chunk=86, passes=[86], tiles=688, plan=_plan([(4, 4), (2, 8)], (6, 4), (6, 4), (6, 4), 2, 1)),
    "S2": dict(B=3, Ta=16000, frames=59, chunk=2, passes=[2, 1], tiles=4, plan=_plan([(2, 8)], (1, 8), (1, 8), (2, 8), 1, 8)),
}


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def _w(sd, key, dtype):
    return sd[key].to(dtype)


def _gemm_cm(x, w, b=None):
    """y[b, n, t] = sum_c w[n, c] x[b, c, t] (+ bias[n]) on channel-major data."""
    y = torch.matmul(w, x)
    return y if b is None else y + b[None, :, None]


# ---------------------------------------------------------------- feature extractor
def conv0(sd, wav, dtype=torch.float64):
    """conv0_kernel: Conv1d(1, 512, 10, stride 5, no bias); wav (B, Ta) -> (B, 512, L0)."""
    return F.conv1d(wav.to(dtype)[:, None], _w(sd, "feature_extractor.conv_layers.0.conv.weight", dtype), None, stride=CONV_S[0])


def rownorm_gelu(sd, y, T, dtype=torch.float64, defect=None):
    """rownorm_gelu_kernel: GroupNorm(512, 512) — every channel over its own T frames — + GELU, in place; y (B, 512, pitch) -> (B, 512, T)."""
    x = y.to(dtype)
    st = x if defect == "stats_over_pitch" else x[..., :T]
    mean = st.mean(dim=2, keepdim=True)
    var = (st - mean).pow(2).mean(dim=2, keepdim=True)
    g = _w(sd, "feature_extractor.conv_layers.0.layer_norm.weight", dtype)[None, :, None]
    b = _w(sd, "feature_extractor.conv_layers.0.layer_norm.bias", dtype)[None, :, None]
    return _gelu((x[..., :T] - mean) / torch.sqrt(var + 1e-5) * g + b)


def conv(sd, i, x, Tin, dtype=torch.float64, defect=None):
    """cgemm_kernel's strided-convolution segment: Conv1d(512, 512, k, stride 2, no bias) + GELU; x (B, 512, pitch_in) -> (B, 512, Lout).
    Output t is rows 2 t .. 2 t + k - 1 of the input times the weight's taps."""
    k, s = CONV_K[i], CONV_S[i]
    w = _w(sd, f"feature_extractor.conv_layers.{i}.conv.weight", dtype)             # (N, C, k)
    Lout = (Tin - k) // s + 1
    xin = x.to(dtype)
    if defect == "row_start":          # every output row begins one input row late (reads pad / stale rows at the end)
        xin = torch.cat([xin[..., 1:], xin[..., :1]], dim=2)
    rows = xin[..., :Tin].unfold(2, k, s)[:, :, :Lout]                              # (B, C, Lout, k)
    if defect == "tap_shift":          # the last tap reads one row further
        nxt = torch.cat([xin[..., 1:], xin[..., :1]], dim=2).unfold(2, k, s)[:, :, :Lout]
        rows = torch.cat([rows[..., :k - 1], nxt[..., k - 1:]], dim=3)
    B = rows.shape[0]
    a = rows.permute(0, 2, 1, 3).reshape(B, Lout, CONV * k)
    y = a @ w.reshape(w.shape[0], CONV * k).t()                                      # (B, Lout, N)
    return _gelu(y).transpose(1, 2).contiguous()


def interp_linear(x, Tin, Tout, dtype=torch.float64, kernel_weights=True, defect=None):
    """interp_linear_kernel: F.interpolate(linear, align_corners=True) along t; x (B, 512, pitch_in) -> (B, 512, Tout).
    kernel_weights: the interpolation weights are fp32 by construction (pos = scale * i, l1 = pos - i0, l0 = 1 - l1, each correctly rounded; at
    position 48 an fp32 `pos` is 4e-6 from the exact one), so they are taken as the kernel forms them and the arithmetic on them runs in `dtype`;
    False: F.interpolate itself (the oracle's call)."""
    h = x.to(dtype)[..., :Tin]
    if defect == "align_corners":
        return F.interpolate(h, size=Tout, align_corners=False, mode="linear")
    if not kernel_weights:
        return F.interpolate(h, size=Tout, align_corners=True, mode="linear")
    f32 = torch.float32
    scale = torch.tensor(float(Tin - 1), dtype=f32) / torch.tensor(float(Tout - 1), dtype=f32) if Tout > 1 else torch.zeros((), dtype=f32)
    pos = scale * torch.arange(Tout, dtype=f32)
    i0 = pos.to(torch.int64).clamp(max=Tin - 1)
    i1 = i0 + (i0 < Tin - 1).to(torch.int64)
    l1 = pos - i0.to(f32)
    l0 = 1.0 - l1
    return l0.to(dtype) * h[..., i0] + l1.to(dtype) * h[..., i1]


def cm_to_tm(x, T):
    """cm_to_tm_kernel: (B, C, pitch) -> (B, T, C), a pure layout kernel."""
    return x[..., :T].transpose(1, 2).contiguous()


# ---------------------------------------------------------------- projection, positional convolution, LayerNorm
def fproj(sd, x, T, dtype=torch.float64):
    """cgemm_kernel with the XF_LN operand transform: feature_projection.layer_norm (over the 512 channels of a token) then
    feature_projection.projection; x (B, 512, pitch) -> (B, 768, T)."""
    h = F.layer_norm(x.to(dtype)[..., :T].transpose(1, 2), (CONV,), _w(sd, "feature_projection.layer_norm.weight", dtype),
                     _w(sd, "feature_projection.layer_norm.bias", dtype), LN_EPS)
    return _gemm_cm(h.transpose(1, 2), _w(sd, "feature_projection.projection.weight", dtype), _w(sd, "feature_projection.projection.bias", dtype))


def pos_weight(sd, dtype=torch.float64, host_fold=True):
    """weight_norm(dim=2) of the positional convolution, (768, 48, K).  host_fold: folded in fp32 as weights.cpp folds it (squares summed in double,
    the norm and g / norm in fp32) — the weight the kernel multiplies by; False: folded in `dtype` (the oracle's)."""
    g, v = sd["encoder.pos_conv_embed.conv.weight_g"], sd["encoder.pos_conv_embed.conv.weight_v"]
    if host_fold:
        g, v = g.float(), v.float()
        nk = v.double().pow(2).sum(dim=(0, 1), keepdim=True).sqrt().float()
        return (v * (g / nk)).to(dtype)
    g, v = g.to(dtype), v.to(dtype)
    return v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())


def posconv(sd, h, T, dtype=torch.float64, host_fold=True, defect=None):
    """cgemm_kernel's grouped segment: Conv1d(768, 768, 128, padding 64, groups 16), last output dropped, + bias, GELU (the residual is added by the
    LayerNorm launch); h (B, 768, pitch) -> (B, 768, T).  Output t of group g is input rows t - 64 .. t + 63 (zero outside 0 .. T - 1) of the group's
    48 channels."""
    w = pos_weight(sd, dtype, host_fold)                                             # (768, 48, K)
    K = w.shape[2]
    wg = w.view(POS_G, POS_CG, POS_CG, K).permute(0, 3, 2, 1).reshape(POS_G, K * POS_CG, POS_CG)   # [g][(k, c)][n]
    x = h.to(dtype)[..., :T]
    B = x.shape[0]
    xg = x.view(B, POS_G, POS_CG, T)
    if defect == "group_neighbour":
        xg = torch.roll(xg, -1, dims=1)
    lead = K // 2 - (1 if defect == "keep_last" else 0)   # keeping the last output and dropping the first shifts every output by one
    out = torch.empty(B, H, T, dtype=dtype)
    for b in range(B):   # clip by clip: the unfolded operand of a long batch is gigabytes
        xp = F.pad(xg[b], (lead, K - lead))                                          # (16, 48, T + K)
        a = xp.unfold(2, K, 1)[:, :, :T].permute(0, 2, 3, 1).reshape(POS_G, T, K * POS_CG)   # [g][t][(k, c)]
        out[b] = (a @ wg).permute(0, 2, 1).reshape(H, T)
    return _gelu(out + _w(sd, "encoder.pos_conv_embed.conv.bias", dtype)[None, :, None])


def layernorm(sd, prefix, x, add, T, dtype=torch.float64):
    """layernorm_cm_kernel: LayerNorm over the 768 channels of (x + add) per token; x, add (B, 768, pitch) (add may be None) -> (B, 768, T).
    prefix: "encoder.layer_norm", "encoder.layers.0.layer_norm", "encoder.layers.0.final_layer_norm"."""
    v = x.to(dtype)[..., :T]
    if add is not None:
        v = v + add.to(dtype)[..., :T]
    y = F.layer_norm(v.transpose(1, 2), (v.shape[1],), _w(sd, prefix + ".weight", dtype), _w(sd, prefix + ".bias", dtype), LN_EPS)
    return y.transpose(1, 2).contiguous()


# ---------------------------------------------------------------- encoder layer
def qkv(sd, l, h, T, dtype=torch.float64):
    """cgemm_kernel with EPI_QKV: q | k | v projections; h (B, 768, pitch) -> (qk (B, 24, T, 64) token-major per head, v (B, 768, T))."""
    w, b = qkv_weight(sd, l)
    y = _gemm_cm(h.to(dtype)[..., :T], w.to(dtype), b.to(dtype))                     # (B, 2304, T)
    B = y.shape[0]
    qk = y[:, :2 * H].reshape(B, 2 * HEADS, HD, T).transpose(2, 3).contiguous()
    return qk, y[:, 2 * H:].contiguous()


def attention(qk, vt, T, ks=1, dtype=torch.float64, defect=None):
    """attn_kernel<2, ks, PM 2 / PM 0>: softmax(q k^T / 8) v per head with the kernel's key slicing; qk (B, 24, rows, 64), vt (B, 768, pitch) ->
    (B, 768, T) channel-major.  Key tiles of 32, slice w of `ks` taking tiles w, w + ks, ...; per tile the running maximum m, p = exp(s - m), the row sum
    and the P V product rescaled by exp(m_old - m); keys >= T of the last tile masked; the slices merged with exp(m_w - M); one division at the end.
    In exact arithmetic that is the plain softmax (the CPU module shows it); restated so that a wrong slice or mask has a name."""
    B = qk.shape[0]
    q, k = qk[:, :HEADS, :T].to(dtype), qk[:, HEADS:].to(dtype)
    v = vt.to(dtype).view(B, HEADS, HD, -1)
    if defect == "v_row":              # V fetched one pitch further: the next channel's row
        v = torch.roll(vt.to(dtype), -1, dims=1).view(B, HEADS, HD, -1)
    nkt = (T + 31) // 32
    Tk = nkt * 32 if defect == "unmasked" else T   # the last tile's keys T .. 32 nkt - 1 take part
    s_all = q @ k[:, :, :Tk].transpose(2, 3) * 0.125                                 # (B, 12, T, Tk)
    ms, ls, os_ = [], [], []
    for w in range(ks):
        m = torch.full((B, HEADS, T), -1.0e30, dtype=dtype)
        lsum = torch.zeros(B, HEADS, T, dtype=dtype)
        o = torch.zeros(B, HEADS, T, HD, dtype=dtype)
        for kt in range(w, nkt, ks):
            j0, j1 = kt * 32, min(kt * 32 + 32, Tk)
            s = s_all[..., j0:j1]
            mn = torch.maximum(m, s.amax(dim=-1))
            alpha = torch.exp(m - mn)
            p = torch.exp(s - mn[..., None])
            lsum = lsum * alpha + p.sum(dim=-1)
            o = o * alpha[..., None] + p @ v[..., j0:j1].transpose(2, 3)
            m = mn
        ms.append(m), ls.append(lsum), os_.append(o)
    if defect == "slice_dropped":      # the last slice that has a key tile never reaches the merge
        last = min(ks, nkt) - 1
        ms, ls, os_ = ms[:last] + ms[last + 1:], ls[:last] + ls[last + 1:], os_[:last] + os_[last + 1:]
    M = torch.stack(ms).amax(dim=0)
    Lsum = torch.zeros_like(M)
    acc = torch.zeros_like(os_[0])
    for m, lsum, o in zip(ms, ls, os_):
        f = torch.exp(m - M)
        Lsum = Lsum + lsum * f
        acc = acc + o * f[..., None]
    return (acc / Lsum[..., None]).permute(0, 1, 3, 2).reshape(B, H, T)


def attention_plain(qk, vt, T, dtype=torch.float64):
    """softmax(q k^T / 8) v without any slicing -> (B, 768, T)."""
    B = qk.shape[0]
    q, k = qk[:, :HEADS, :T].to(dtype), qk[:, HEADS:, :T].to(dtype)
    v = vt.to(dtype).view(B, HEADS, HD, -1)[..., :T]
    p = torch.softmax(q @ k.transpose(2, 3) * 0.125, dim=-1)
    return (p @ v.transpose(2, 3)).permute(0, 1, 3, 2).reshape(B, H, T)


def _linear_res(sd, p, x, res, T, dtype, defect=None, act=False):
    y = x.to(dtype)[..., :T]
    w = _w(sd, p + "weight", dtype)
    out = _gemm_cm(y, w, _w(sd, p + "bias", dtype))
    if defect == "k_block":            # the workgroup of token tile 0, column tile 0 leaves out its last 32-channel K block
        out[:, :32, :32] = _gemm_cm(y[:, :-32, :32], w[:32, :-32], _w(sd, p + "bias", dtype)[:32])
    if act:
        out = _gelu(out)
    if res is not None:
        r = res.to(dtype)
        out = out + (r[..., 1:T + 1] if defect == "res_neighbour" else r[..., :T])
    return out


def out_proj(sd, l, o, res, T, dtype=torch.float64, defect=None):
    """cgemm_kernel with RES_PLAIN: attention.out_proj + residual; o, res (B, 768, pitch) -> (B, 768, T)."""
    return _linear_res(sd, f"encoder.layers.{l}.attention.out_proj.", o, res, T, dtype, defect)


def ff1(sd, l, h, T, dtype=torch.float64):
    """feed_forward.intermediate_dense + GELU; h (B, 768, pitch) -> (B, 3072, T)."""
    return _linear_res(sd, f"encoder.layers.{l}.feed_forward.intermediate_dense.", h, None, T, dtype, act=True)


def ff2(sd, l, f, res, T, dtype=torch.float64, defect=None):
    """feed_forward.output_dense + residual (RES_PLAIN); f (B, 3072, pitch), res (B, 768, pitch) -> (B, 768, T)."""
    return _linear_res(sd, f"encoder.layers.{l}.feed_forward.output_dense.", f, res, T, dtype, defect)


def proj(w, b, h, T, dtype=torch.float64):
    """audio_proj_layer (weight (D, 768) and bias of the full state dict); h (B, 768, pitch) -> (B, D, T)."""
    return _gemm_cm(h.to(dtype)[..., :T], w.to(dtype), b.to(dtype))


def num_layers(sd) -> int:
    n = 0
    while f"encoder.layers.{n}.layer_norm.weight" in sd:
        n += 1
    return n


def padded(x, fill=None):
    """(B, C, T) -> (B, C, pitch) as the engine stores it: the rows T .. pitch hold `fill` (a tensor generator's values, or zeros)."""
    T = x.shape[-1]
    out = torch.zeros(*x.shape[:-1], pitch_of(T), dtype=x.dtype) if fill is None else fill(*x.shape[:-1], pitch_of(T)).to(x.dtype)
    out[..., :T] = x
    return out


def encode(sd, wav, num_frames, dtype=torch.float64, ks=8, proj_wb=None, features_only=False, fill=None, kernel_weights=False, host_fold=False):
    """The launches chained as audio_encode chains them, every intermediate padded to its pitch with `fill` -> (B, frames, 768 | D | 512)."""
    L = conv_lengths(wav.shape[1])
    x = padded(conv0(sd, wav, dtype), fill)
    x = padded(rownorm_gelu(sd, x, L[0], dtype), fill)
    for i in range(1, 7):
        x = padded(conv(sd, i, x, L[i - 1], dtype), fill)
    T = L[6]
    if num_frames is not None:
        x = padded(interp_linear(x, L[6], num_frames, dtype, kernel_weights), fill)
        T = num_frames
    if features_only:
        return cm_to_tm(x, T)
    h = padded(fproj(sd, x, T, dtype), fill)
    pos = padded(posconv(sd, h, T, dtype, host_fold), fill)
    h = padded(layernorm(sd, "encoder.layer_norm", h, pos, T, dtype), fill)
    for l in range(num_layers(sd)):
        qk, v = qkv(sd, l, h, T, dtype)
        qk = padded(qk.transpose(2, 3), fill).transpose(2, 3).contiguous()
        o = padded(attention(qk, padded(v, fill), T, ks, dtype), fill)
        t = padded(out_proj(sd, l, o, h, T, dtype), fill)
        h = padded(layernorm(sd, f"encoder.layers.{l}.layer_norm", t, None, T, dtype), fill)
        f = padded(ff1(sd, l, h, T, dtype), fill)
        t = padded(ff2(sd, l, f, h, T, dtype), fill)
        h = padded(layernorm(sd, f"encoder.layers.{l}.final_layer_norm", t, None, T, dtype), fill)
    if proj_wb is not None:
        h = padded(proj(proj_wb[0], proj_wb[1], h, T, dtype), fill)
    return cm_to_tm(h, T)
