"""Stage-by-stage restatement of the bf16 audio encoder (said_amd/csrc/audio_enc.cpp, bf16 branch) — TEST INFRASTRUCTURE.

One function per stage of said_audio_encode (the stage order of said_debug_option "audio_stop_after", said_hip_debug.h).  Each takes the stage's
inputs AS THE ENGINE STORES THEM (token-major, already in the stored type's value set) plus the audio state dict (keys without the "audio_encoder."
prefix) and returns what the kernel should store:

  * rounded=True (the kernel's arithmetic): the operands of every product that bf16 mode runs on v_mfma_f32_32x32x16_bf16 are rounded to bf16
    (nearest even), the sums are exact in `dtype`; everything else is evaluated in `dtype`; the result is rounded to the stored type
    (store=False: returned before that last rounding);
  * rounded=False: the same function without any rounding — chained, that is oracle/wav2vec2.py::wav2vec2_forward (tests/test_audio_bf16_ref_cpu.py);
  * dtype: torch.float64 for the reference, torch.float32 for the "same operands, fp32 arithmetic" evaluation that measures how far a correct fp32
    accumulation may sit from the float64 one.

Weight layouts follow said_amd/csrc/weights.cpp and weight_pack.h: conv weights tap-major [N][taps * 512], q | k | v concatenated, the positional convolution's
weight_norm folded in fp32 as the host folds it and split into 16 groups of 48 output rows over [tap][48 channels].
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

HEADS, HD, H, CONV, FFN = 12, 64, 768, 512, 3072
CONV_K = (10, 3, 3, 3, 3, 2, 2)
CONV_S = (5, 2, 2, 2, 2, 2, 2)
POS_G, POS_CG = 16, 48
LN_EPS = 1e-5
# stage numbers (said_hip_debug.h)
ST_CONV0, ST_INTERP, ST_FPROJ, ST_GROUP, ST_POS, ST_ENC_LN, ST_LAYER0 = 0, 7, 8, 9, 10, 11, 12
LY_QKV, LY_ATTN, LY_CM2TM, LY_OUT, LY_LN1, LY_FF1, LY_FF2, LY_LN2 = range(8)


def conv_lengths(Ta: int):
    L = []
    for k, s in zip(CONV_K, CONV_S):
        Ta = (Ta - k) // s + 1
        L.append(Ta)
    return L


def audio_sd(sd):
    """The audio encoder's tensors of a full state dict, prefix removed."""
    p = "audio_encoder."
    return {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}


# ---------------------------------------------------------------- roundings
def round_bf16(x: torch.Tensor) -> torch.Tensor:
    """x rounded to the nearest bf16 (ties to even), returned in x's dtype.  float64 goes through fp32; where that first rounding lands exactly on a
    bf16 tie although x was not one, the fp32 value is moved one ulp towards x first, so the result is the correctly rounded one."""
    if x.dtype == torch.float32:
        return x.bfloat16().float()
    x32 = x.float()
    bits = x32.view(torch.int32)
    err = x - x32.double()
    tie = ((bits & 0xFFFF) == 0x8000) & (err != 0)
    up = (err > 0) == (x32 > 0)   # the true value is larger in magnitude
    bits = bits + torch.where(tie, torch.where(up, 1, -1), 0).to(torch.int32)
    return bits.view(torch.float32).bfloat16().to(x.dtype)


def _op(x, rounded, dtype):     # a product operand
    x = x.to(dtype)
    return round_bf16(x) if rounded else x


def _store_bf16(y, rounded, store):
    return round_bf16(y) if (rounded and store) else y


def _store_f32(y, rounded, store):
    return y.float().to(y.dtype) if (rounded and store) else y


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def _linear(x, w, b, rounded, dtype):
    y = _op(x, rounded, dtype) @ _op(w, rounded, dtype).t()
    return y if b is None else y + b.to(dtype)


# ---------------------------------------------------------------- feature extractor
def conv0(sd, wav, rounded=True, dtype=torch.float64, store=True):
    """Conv1d(1, 512, 10, stride 5, no bias) + GroupNorm(512, 512) + GELU (all fp32 in the kernel: no bf16 operand) -> (B, L0, 512) bf16."""
    h = F.conv1d(wav.to(dtype)[:, None], sd["feature_extractor.conv_layers.0.conv.weight"].to(dtype), None, stride=CONV_S[0])
    h = F.group_norm(h, CONV, sd["feature_extractor.conv_layers.0.layer_norm.weight"].to(dtype),
                     sd["feature_extractor.conv_layers.0.layer_norm.bias"].to(dtype), eps=1e-5)
    return _store_bf16(_gelu(h).transpose(1, 2).contiguous(), rounded, store)


def conv_rows(x, k, s):
    """The overlapping rows of a strided Conv1d over token-major data: (B, Lin, C) -> (B, Lout, k * C), tap-major."""
    B, _, C = x.shape
    return x.unfold(1, k, s).permute(0, 1, 3, 2).reshape(B, -1, k * C)


def conv_weight_tap_major(w):
    """(N, C, k) -> (N, k * C) (weight_pack.h tap_major)."""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1)


def conv(sd, i, x, rounded=True, dtype=torch.float64, store=True):
    """Conv1d(512, 512, k, stride 2, no bias) + GELU as a GEMM with overlapping rows; x (B, Lin, 512) bf16 -> (B, Lout, 512) bf16."""
    w = conv_weight_tap_major(sd[f"feature_extractor.conv_layers.{i}.conv.weight"])
    y = _linear(conv_rows(x.to(dtype), CONV_K[i], CONV_S[i]), w, None, rounded, dtype)
    return _store_bf16(_gelu(y), rounded, store)


def interp_ln(sd, x, num_frames, rounded=True, dtype=torch.float64, store=True):
    """F.interpolate(linear, align_corners=True) to num_frames + feature_projection.layer_norm; x (B, L6, 512) bf16 -> (B, num_frames, 512) bf16."""
    h = x.to(dtype)
    if num_frames is not None and rounded:
        # the kernel's interpolation weights are fp32 by construction (interp_ln_tm_kernel: pos = scale * i, l1 = pos - i0, l0 = 1 - l1, each correctly rounded):
        # at position 48 an fp32 `pos` is 4e-6 from the exact one, so the weights are taken as the kernel forms them and the arithmetic on them runs in `dtype`
        Tin = h.shape[1]
        scale = torch.tensor(float(Tin - 1), dtype=torch.float32) / torch.tensor(float(num_frames - 1), dtype=torch.float32) if num_frames > 1 else torch.zeros((), dtype=torch.float32)
        pos = scale * torch.arange(num_frames, dtype=torch.float32)
        i0 = pos.to(torch.int64).clamp(max=Tin - 1)
        i1 = i0 + (i0 < Tin - 1).to(torch.int64)
        l1 = pos - i0.to(torch.float32)
        l0 = 1.0 - l1
        h = l0.to(dtype)[None, :, None] * h[:, i0] + l1.to(dtype)[None, :, None] * h[:, i1]
    elif num_frames is not None:
        h = F.interpolate(h.transpose(1, 2), size=num_frames, align_corners=True, mode="linear").transpose(1, 2)
    h = F.layer_norm(h, (CONV,), sd["feature_projection.layer_norm.weight"].to(dtype), sd["feature_projection.layer_norm.bias"].to(dtype), LN_EPS)
    return _store_bf16(h, rounded, store)


def fproj(sd, x, rounded=True, dtype=torch.float64, store=True):
    """feature_projection.projection; x (B, F, 512) bf16 -> (B, F, 768) fp32."""
    return _store_f32(_linear(x, sd["feature_projection.projection.weight"], sd["feature_projection.projection.bias"], rounded, dtype), rounded, store)


# ---------------------------------------------------------------- positional convolution
def group_rows(T: int, taps: int = 128) -> int:
    return (T + taps + 7) // 8 * 8


def tm_to_group(h, rounded=True, dtype=torch.float64, store=True, taps=128):
    """tm_to_group_bf16: (B, T, 768) fp32 -> (B, 16, R, 48) bf16, taps / 2 zero rows in front, zeros behind (R = roundup(T + taps, 8))."""
    B, T, _ = h.shape
    R = group_rows(T, taps)
    out = torch.zeros(B, POS_G, R, POS_CG, dtype=dtype)
    out[:, :, taps // 2:taps // 2 + T] = h.to(dtype).view(B, T, POS_G, POS_CG).permute(0, 2, 1, 3)
    return _store_bf16(out, rounded, store)


def pos_weight_groups(sd):
    """weight_norm(dim=2) folded in fp32 as weights.cpp folds it (squares summed in double, the norm and g / norm in fp32), then per group
    [16][48 outputs][tap][48 channels] (the host pads each group's rows to 64 with zeros: columns the launch never stores)."""
    g = sd["encoder.pos_conv_embed.conv.weight_g"].float()
    v = sd["encoder.pos_conv_embed.conv.weight_v"].float()              # (768, 48, K)
    nk = v.double().pow(2).sum(dim=(0, 1), keepdim=True).sqrt().float()
    w = v * (g / nk)                                                     # fp32, (768, 48, K)
    K = w.shape[2]
    return w.view(POS_G, POS_CG, POS_CG, K).permute(0, 1, 3, 2).contiguous()   # [g][n][k][c]


def posconv(sd, xg, h, rounded=True, dtype=torch.float64, store=True):
    """Grouped Conv1d(768, 768, 128, padding 64, groups 16) (last output dropped) + bias + GELU + hidden state; xg (B, 16, R, 48) bf16,
    h (B, T, 768) fp32 -> (B, T, 768) fp32.  Output token t of group g is rows t .. t + 127 of xg[b, g] times the group's tap-major weights."""
    B, T, _ = h.shape
    w = _op(pos_weight_groups(sd), rounded, dtype)                       # (16, 48, K, 48)
    K = w.shape[2]
    x = _op(xg, rounded, dtype)
    y = torch.zeros(B, POS_G, T, POS_CG, dtype=dtype)
    step = 16
    for k0 in range(0, K, step):   # sixteen taps at a time: the full (T, K * 48) operand of a long clip batch is gigabytes
        a = x[:, :, k0:k0 + T + step - 1].unfold(2, step, 1).permute(0, 1, 2, 4, 3).reshape(B, POS_G, T, step * POS_CG)
        y += a @ w[:, :, k0:k0 + step].reshape(POS_G, POS_CG, step * POS_CG).transpose(1, 2)
    y = y.permute(0, 2, 1, 3).reshape(B, T, H) + sd["encoder.pos_conv_embed.conv.bias"].to(dtype)
    return _store_f32(_gelu(y) + h.to(dtype), rounded, store)


# ---------------------------------------------------------------- LayerNorm with fp32 and bf16 copies
def ln(sd, prefix, x, rounded=True, dtype=torch.float64, store=True):
    """ln_tm: LayerNorm(768) of x (B, T, 768) fp32 -> (fp32 copy, bf16 copy).  prefix: "encoder.layer_norm", "encoder.layers.0.layer_norm", ..."""
    y = F.layer_norm(x.to(dtype), (x.shape[-1],), sd[prefix + ".weight"].to(dtype), sd[prefix + ".bias"].to(dtype), LN_EPS)
    return _store_f32(y, rounded, store), _store_bf16(y, rounded, store)


# ---------------------------------------------------------------- encoder layer
def qkv_weight(sd, l):
    p = f"encoder.layers.{l}.attention."
    w = torch.cat([sd[p + n + "_proj.weight"] for n in "qkv"], 0)
    b = torch.cat([sd[p + n + "_proj.bias"] for n in "qkv"], 0)
    return w, b


def qkv(sd, l, hb, rounded=True, dtype=torch.float64, store=True):
    """q | k | v projections into attn.hip's layouts; hb (B, T, 768) bf16 -> (qk (B, 24, T, 64) fp32: heads of q then of k, token-major per head;
    vt (B, 768, T) fp32 channel-major).  q is NOT scaled here: attention applies head_dim ** -0.5 to the scores."""
    w, b = qkv_weight(sd, l)
    y = _store_f32(_linear(hb, w, b, rounded, dtype), rounded, store)
    B, T, _ = y.shape
    qk = y[..., :2 * H].reshape(B, T, 2 * HEADS, HD).permute(0, 2, 1, 3).contiguous()
    vt = y[..., 2 * H:].transpose(1, 2).contiguous()
    return qk, vt


def attention(qk, vt, ks=1, rounded=True, dtype=torch.float64, store=True, out_bf16=False):
    """attn_kernel in product mode 1 (bf16 operands); qk (B, 24, T, 64), vt (B, 768, T) fp32 -> (B, T, 768) token-major values.
    rounded=True restates the kernel's online softmax: q, k, v rounded to bf16; key tiles of 32, slice w of `ks` taking tiles w, w + ks, ...; per tile the
    running maximum m in raw score units, p = exp2((s - m) * c2) with c2 = fp32(scale * log2 e), the row sum from the UNROUNDED p, the P V product from p
    ROUNDED to bf16, the accumulator rescaled by exp2((m_old - m) * c2); the slices merged with exp2((m_w - M) * c2); one division at the end.
    rounded=False: softmax(q k^T / 8) v on the stored fp32 values.  out_bf16: the token-major bf16 store of the key-split-free form (o_mode 2)."""
    B, _, T, _ = qk.shape
    q, k = qk[:, :HEADS].to(dtype), qk[:, HEADS:].to(dtype)
    v = vt.to(dtype).view(B, HEADS, HD, T)
    if not rounded:
        p = torch.softmax(q @ k.transpose(2, 3) * 0.125, dim=-1)
        return (p @ v.transpose(2, 3)).permute(0, 2, 1, 3).reshape(B, T, H)
    q, k, v = round_bf16(q), round_bf16(k), round_bf16(v)
    c2 = float(torch.tensor(0.125 * 1.4426950408889634, dtype=torch.float32))
    s_all = q @ k.transpose(2, 3)                                     # (B, 12, T, T) raw scores
    nkt = (T + 31) // 32
    ms, ls, os_ = [], [], []
    for w in range(ks):
        m = torch.full((B, HEADS, T), -1.0e30, dtype=dtype)
        lsum = torch.zeros(B, HEADS, T, dtype=dtype)
        o = torch.zeros(B, HEADS, T, HD, dtype=dtype)
        for kt in range(w, nkt, ks):
            j0, j1 = kt * 32, min(kt * 32 + 32, T)
            s = s_all[..., j0:j1]
            mn = torch.maximum(m, s.amax(dim=-1))
            alpha = torch.exp2((m - mn) * c2)
            p = torch.exp2(s * c2 - (mn * c2)[..., None])
            lsum = lsum * alpha + p.sum(dim=-1)
            o = o * alpha[..., None] + round_bf16(p) @ v[..., j0:j1].transpose(2, 3)
            m = mn
        ms.append(m), ls.append(lsum), os_.append(o)
    M = torch.stack(ms).amax(dim=0)
    Lsum = torch.zeros_like(M)
    acc = torch.zeros_like(os_[0])
    for m, lsum, o in zip(ms, ls, os_):
        f = torch.exp2((m - M) * c2)
        Lsum = Lsum + lsum * f
        acc = acc + o * f[..., None]
    y = (acc / Lsum[..., None]).permute(0, 2, 1, 3).reshape(B, T, H)
    return _store_bf16(y, rounded, store) if out_bf16 else _store_f32(y, rounded, store)


def cm_to_tm(o_cm, rounded=True, dtype=torch.float64, store=True):
    """cm_to_tm_bf16: (B, 768, T) fp32 channel-major -> (B, T, 768) bf16 (a pure layout + rounding kernel)."""
    return _store_bf16(o_cm.to(dtype).transpose(1, 2).contiguous(), rounded, store)


def out_proj(sd, l, o, res, rounded=True, dtype=torch.float64, store=True):
    """attention.out_proj + residual; o (B, T, 768) bf16, res (B, T, 768) fp32 -> (B, T, 768) fp32."""
    p = f"encoder.layers.{l}.attention.out_proj."
    return _store_f32(_linear(o, sd[p + "weight"], sd[p + "bias"], rounded, dtype) + res.to(dtype), rounded, store)


def ff1(sd, l, hb, rounded=True, dtype=torch.float64, store=True):
    """feed_forward.intermediate_dense + GELU; hb (B, T, 768) bf16 -> (B, T, 3072) bf16."""
    p = f"encoder.layers.{l}.feed_forward.intermediate_dense."
    return _store_bf16(_gelu(_linear(hb, sd[p + "weight"], sd[p + "bias"], rounded, dtype)), rounded, store)


def ff2(sd, l, f, res, rounded=True, dtype=torch.float64, store=True):
    """feed_forward.output_dense + residual; f (B, T, 3072) bf16, res (B, T, 768) fp32 -> (B, T, 768) fp32."""
    p = f"encoder.layers.{l}.feed_forward.output_dense."
    return _store_f32(_linear(f, sd[p + "weight"], sd[p + "bias"], rounded, dtype) + res.to(dtype), rounded, store)


def num_layers(sd) -> int:
    n = 0
    while f"encoder.layers.{n}.layer_norm.weight" in sd:
        n += 1
    return n


def encode(sd, wav, num_frames, rounded=True, dtype=torch.float64, ks=1):
    """The stages chained as said_audio_encode chains them -> (B, num_frames, 768)."""
    x = conv0(sd, wav, rounded, dtype)
    for i in range(1, 7):
        x = conv(sd, i, x, rounded, dtype)
    x = interp_ln(sd, x, num_frames, rounded, dtype)
    h = fproj(sd, x, rounded, dtype)
    t = posconv(sd, tm_to_group(h, rounded, dtype), h, rounded, dtype)
    h, hb = ln(sd, "encoder.layer_norm", t, rounded, dtype)
    for l in range(num_layers(sd)):
        qk, vt = qkv(sd, l, hb, rounded, dtype)
        o = attention(qk, vt, ks, rounded, dtype, out_bf16=True)   # (through cm_to_tm_bf16 or its own store: bf16 either way)
        t = out_proj(sd, l, o, h, rounded, dtype)
        h, hb = ln(sd, f"encoder.layers.{l}.layer_norm", t, rounded, dtype)
        t = ff2(sd, l, ff1(sd, l, hb, rounded, dtype), h, rounded, dtype)
        h, hb = ln(sd, f"encoder.layers.{l}.final_layer_norm", t, rounded, dtype)
    return h


# ---------------------------------------------------------------- the comparisons (shared by the CPU and the GPU tests)
F32_FACTOR, F32_FLOOR = 4.0, 1e-6   # tests/test_gpu_unet_train.py's rule: the factor covers another summation order


def rel_max(a, ref64):
    return float((a.double() - ref64).abs().max()) / float(ref64.abs().max())


def f32_bound(ref32, ref64):
    """(e32, bound): the fp32 evaluation's own distance from the float64 one, of the largest magnitude, and what a kernel may have."""
    e32 = rel_max(ref32, ref64)
    return e32, F32_FACTOR * max(e32, F32_FLOOR)


def check_f32(name, got, ref64, ref32):
    """An fp32 store: e = max |got - ref64| / max |ref64| <= 4 max(e32, 1e-6)."""
    e = rel_max(got, ref64)
    e32, bound = f32_bound(ref32, ref64)
    print(f"{name}: e {e:.2e} (fp32 CPU evaluation {e32:.2e}, bound {bound:.2e}) of max |ref| {float(ref64.abs().max()):.3g}, {got.numel()} elements")
    assert math.isfinite(e) and e <= bound, f"{name}: {e:.3e} of range, bound {bound:.3e}"
    return e, bound


def bf16_step(x):
    """The spacing of bf16 values at |x| (8 significand bits)."""
    _, ex = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), ex - 8)


def bf16_stats(got, ref_r, abs_bound):
    """(share of bit-equal elements, number of elements neither bit-equal nor within one bf16 step nor within abs_bound, largest |difference|)."""
    got, ref_r = got.double(), ref_r.double()
    d = (got - ref_r).abs()
    eq = d == 0
    ok = eq | (d <= torch.maximum(bf16_step(ref_r), bf16_step(got))) | (d <= abs_bound)
    return float(eq.double().mean()), int((~ok).sum()), float(d.max())


def check_bf16(name, got, ref_r, ref_pre64, ref_pre32, ref_r32):
    """A bf16 store.  got, ref_r: stored values and the rounded float64 reference; ref_pre64 / ref_pre32: the float64 and fp32 evaluations before the store's
    rounding (they give the fp32 bound in absolute terms); ref_r32: the fp32 evaluation rounded (the reference's own bit-equal share)."""
    e32, bound = f32_bound(ref_pre32, ref_pre64)
    abs_bound = bound * float(ref_pre64.abs().max())
    own, _, _ = bf16_stats(ref_r32, ref_r, abs_bound)
    assert own >= 0.999, f"{name}: the fp32 CPU evaluation of these inputs is only {100 * own:.3f} % bit-equal to the float64 one: the inputs are at fault, not the kernel"
    share, bad, dmax = bf16_stats(got, ref_r, abs_bound)
    print(f"{name}: {100 * share:.3f} % bit-equal (fp32 CPU evaluation {100 * own:.3f} %), {bad} elements beyond one bf16 step and {abs_bound:.2e}, "
          f"max |diff| {dmax:.2e} of max |ref| {float(ref_r.abs().max()):.3g}, {got.numel()} elements")
    assert share >= 0.99, f"{name}: {100 * share:.3f} % bit-equal, at least 99 % wanted"
    assert bad == 0, f"{name}: {bad} elements differ by more than one bf16 step and more than {abs_bound:.3e}"
    return share, dmax


def check_exact(name, got, ref):
    n = int((got.double() != ref.double()).sum())
    print(f"{name}: {n} of {got.numel()} elements differ (exact layout kernel)")
    assert n == 0, f"{name}: {n} elements differ"


def check_attention(name, got, ref_r, ref_u):
    """rms(got - rounded reference) <= 0.1 rms(unrounded - rounded): DESIGN 7.2's criterion for the UNet's bf16 attention."""
    got, ref_r, ref_u = got.double(), ref_r.double(), ref_u.double()
    r = float((got - ref_r).pow(2).mean().sqrt())
    noise = float((ref_u - ref_r).pow(2).mean().sqrt())
    print(f"{name}: rms(got - rounded ref) {r:.2e}, max {float((got - ref_r).abs().max()):.2e}; rms(unrounded - rounded ref) {noise:.2e} (bound {0.1 * noise:.2e}); "
          f"max |ref| {float(ref_r.abs().max()):.3g}")
    assert math.isfinite(r) and r <= 0.1 * noise, f"{name}: rms {r:.3e}, bound {0.1 * noise:.3e}"
    return r, noise
