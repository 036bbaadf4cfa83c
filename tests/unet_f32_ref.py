"""Launch-by-launch restatement of the channel-major fp32 denoise step (said_amd/csrc/unet_sched.cpp: run_unet / run_resblock / run_transformer) — TEST INFRASTRUCTURE.

One function per launch of the default (fp32, split-fp16) schedule, and one per launch of the five-launch tail behind a block's self-attention (to_out1, q_band,
to_out2, geglu, ffproj: strict fp32, and the default mode where the fused tail's window tile cannot hold the band); chain() is their composition.  Each takes the launch's inputs AS THE ENGINE STORES THEM (channel-major (B, C, T) without the pad
tokens [T, Tp); q / k token-major per head; k / v decoded from their packed split pairs) plus the UNet state dict (`model.*` keys) and `dtype`, and returns what the
launch stores.  Operands are NOT rounded: split-fp16 represents an operand to 2^-22, so the float64 evaluation is the yardstick and the float32 one (torch CPU)
measures how far a correct fp32 evaluation of the same inputs may sit from it (audio_bf16_ref.check_f32).  GroupNorm is evaluated from the stored values, not from
the producer's partial statistics: those are held to the values on their own (norm_from_partials).

MUTANT: tests/test_unet_f32_ref_cpu.py sets it to one of MUTANTS to prove that the comparison has teeth — each names one way a kernel of the step can be wrong.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

MC, HEADS, HD, FFI, NST, CIN = 192, 6, 32, 768, 4, 32
RES = ("model.input_blocks.1.0", "model.middle_block.0", "model.middle_block.2", "model.output_blocks.0.0", "model.output_blocks.1.0")
ST = ("model.input_blocks.1.1", "model.middle_block.1", "model.output_blocks.0.1", "model.output_blocks.1.1")
SCALE = HD ** -0.5

MUTANTS = ("fp16_operands", "k_block_dropped", "tap_shifted", "pad_tap_nonzero", "residual_of_neighbour_sample", "gn_neighbour_group", "gn_over_tp",
           "emb_row_of_other_sample", "last_key_tile_missing", "band_shifted", "geglu_swapped", "uncond_runs_cross_attention", "y2_not_written",
           "mask_blend_order",
           # the seams between the five launches of the unfused tail
           "x1_of_wrong_sample_under_x_off", "y2_without_c2", "to_out2_writes_uncond_slot", "band_truncated_to_8_keys", "wide_band_off_by_one",
           "ffproj_second_segment_dropped")
MUTANT = None


def _m(name: str) -> bool:
    assert name in MUTANTS
    return MUTANT == name


def _op(x: torch.Tensor) -> torch.Tensor:
    """An operand of a matrix product (mutant: the high plane alone)."""
    return x.half().to(x.dtype) if _m("fp16_operands") else x


def rup(a: int, b: int) -> int:
    return (a + b - 1) // b * b


# ---------------------------------------------------------------- stored formats
def decode_split(packed: torch.Tensor):
    """fp32-typed dwords holding (h | l << 16) (split_f16.h pack_split_f16) -> (h + 2^-11 l in float64, h, l as fp16 tensors)."""
    u = packed.contiguous().view(torch.int32)
    h = (u & 0xFFFF).to(torch.int16).view(torch.float16)
    lo = ((u >> 16) & 0xFFFF).to(torch.int16).view(torch.float16)
    return h.double() + lo.double() * 2.0 ** -11, h, lo


def split_is_consistent(h: torch.Tensor, lo: torch.Tensor):
    """(elements whose low plane is NOT a rounded remainder of the stored high plane, elements whose remainder is exactly half a step of h).
    x = h + 2^-11 l is exact in fp32 (22 significand bits + sign), and the producer's fp32 value was x up to l's own rounding; l = RN16((x' - h) 2^11) of that
    value x' with h = RN16(x') means |x - h| <= half an fp16 step of h, i.e. RN16(x) = h — except where the remainder rounded up to exactly half a step, which makes
    x a tie (about one element in 2^13).  A tie is what planes from two different conversions produce too, with the value off by a whole step: those
    elements are decided by the value comparison, everything else here."""
    x64 = h.double() + lo.double() * 2.0 ** -11
    x = x64.float()
    assert torch.equal(x.double(), x64), "h + 2^-11 l is not an fp32 number"
    _, ex = torch.frexp(h.double().abs().clamp_min(2.0 ** -14))
    half_step = torch.ldexp(torch.ones_like(x64), ex - 12)
    tie = (x64 - h.double()).abs() == half_step
    bad = (x.half() != h) & ~tie
    return int(bad.sum()), int(tie.sum())


# ---------------------------------------------------------------- GroupNorm
def group_norm(x, groups, gamma, beta, eps, dt, Tp=None):
    """GroupNorm of channel-major x (B, C, T) in dt; gamma / beta None: the normalised tensor alone."""
    B, C, T = x.shape
    xg = x.to(dt).reshape(B, groups, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    if _m("gn_over_tp"):   # the pad tokens [T, Tp) counted as zeros
        f = T / (Tp if Tp is not None else rup(T, 32))
        ex2 = (var + mean * mean) * f
        mean = mean * f
        var = ex2 - mean * mean
    if _m("gn_neighbour_group"):
        mean, var = mean.roll(1, 1), var.roll(1, 1)
    y = ((xg - mean[..., None]) / torch.sqrt(var[..., None] + eps)).reshape(B, C, T)
    if gamma is None:
        return y
    return y * gamma.to(dt)[None, :, None] + beta.to(dt)[None, :, None]


def merge_partials(st: torch.Tensor, T: int, cpg: int):
    """A producer's partial statistics [B][32-token tile][C][(mean, M2)] merged as the consumers merge them (gemm_common.h gn_finish: Chan's update over the
    tiles and the group's channels) -> (mean, variance) per (B, C / cpg), float64."""
    B, npart, C, _ = st.shape
    cnt = torch.tensor([min(32, T - 32 * p) for p in range(npart)], dtype=torch.float64).view(1, npart, 1)
    mean_pc, m2_pc = st[..., 0].double(), st[..., 1].double()
    G = C // cpg
    gm = (cnt * mean_pc).view(B, npart, G, cpg).sum(dim=(1, 3)) / (cpg * T)
    gm_c = gm.repeat_interleave(cpg, dim=1).view(B, 1, C)
    m2 = (m2_pc + cnt * (mean_pc - gm_c) ** 2).view(B, npart, G, cpg).sum(dim=(1, 3))
    return gm, m2 / (cpg * T)


def partials_of(y: torch.Tensor) -> torch.Tensor:
    """What a producer stores beside y (B, C, T): per 32-token tile and channel (mean, M2) -> (B, np, C, 2) fp32 (CPU-made stand-in for the self-check)."""
    T = y.shape[-1]
    parts = [y[..., t0:min(T, t0 + 32)].double() for t0 in range(0, T, 32)]
    return torch.stack([torch.stack([p.mean(-1), ((p - p.mean(-1, keepdim=True)) ** 2).sum(-1)], dim=-1) for p in parts], dim=1).float()


def norm_from_partials(y: torch.Tensor, st: torch.Tensor, cpg: int = 6, eps: float = 1e-5) -> torch.Tensor:
    """The normalised tensor that the stored output y (B, C, T) and its stored partials imply (float64)."""
    T = y.shape[-1]
    mean, var = merge_partials(st, T, cpg)
    mean_c, var_c = mean.repeat_interleave(cpg, dim=1)[..., None], var.repeat_interleave(cpg, dim=1)[..., None]
    return (y.double() - mean_c) / torch.sqrt(var_c + eps)


def gn_coef(sd, j, x, dt):
    """The rows the q/k/v GEMM leaves for the chain: GroupNorm(32 groups, eps 1e-6) of block j's input as (a, b) per channel, y = a x + b -> (B, 192, 2)."""
    p = ST[j]
    B, C, T = x.shape
    xg = x.to(dt).reshape(B, 32, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    rstd = (1.0 / torch.sqrt(var + 1e-6)).repeat_interleave(C // 32, dim=1)
    a = sd[p + ".norm.weight"].to(dt)[None] * rstd
    b = sd[p + ".norm.bias"].to(dt)[None] - mean.repeat_interleave(C // 32, dim=1) * a
    return torch.stack([a, b], dim=-1)


# ---------------------------------------------------------------- products
def _conv3(h, w, dt):
    """Conv1d(k = 3, padding 1) of h (B, C, T) with w (N, C, 3): tap k reads token t + k - 1, zeros outside [0, T)."""
    T = h.shape[-1]
    hp = F.pad(h, (1, 2))
    if _m("pad_tap_nonzero"):
        hp[..., T + 1] = h[..., T - 1]
    taps = [hp[..., k:k + T] for k in range(3)]
    if _m("tap_shifted"):
        taps[2] = hp[..., 3:3 + T]
    w = _op(w.to(dt))
    y = sum(torch.einsum("nc,bct->bnt", w[:, :, k], _op(taps[k])) for k in range(3))
    if _m("k_block_dropped") and T > 32:   # wave 7's 24 channels of one workgroup: sample 0, column tile 0, token tile 1
        hd = h.clone()
        hd[:, h.shape[1] - 24:] = 0
        hp = F.pad(hd, (1, 1))
        yd = sum(torch.einsum("nc,bct->bnt", w[:, :, k], hp[..., k:k + T]) for k in range(3))
        y[0, :32, 32:64] = yd[0, :32, 32:64]
    return y


def _lin(x, w, b, dt):
    """x (..., K) token-major times w (N, K)."""
    y = _op(x) @ _op(w.to(dt)).t()
    return y if b is None else y + b.to(dt)


def _silu(x):
    return x * torch.sigmoid(x)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def _ln(x, g, b, dt):
    return F.layer_norm(x, (x.shape[-1],), g.to(dt), b.to(dt), 1e-5)


# ---------------------------------------------------------------- time embedding (run_time_embed; not a launch of the step: its rows are an input, read back from EO)
def time_rows(sd, ts, dt):
    """EO: the five ResBlocks' emb_layers rows of every timestep -> (5, N, 192).  The frequencies are fp32 by construction (oracle/unet.py timestep_embedding)."""
    half = MC // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
    args = ts[:, None].to(dt) * freqs[None].to(dt)
    e = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    e = _silu(_lin(e, sd["model.time_embed.0.weight"], sd["model.time_embed.0.bias"], dt))
    e = _lin(e, sd["model.time_embed.2.weight"], sd["model.time_embed.2.bias"], dt)
    return torch.stack([_lin(_silu(e), sd[p + ".emb_layers.1.weight"], sd[p + ".emb_layers.1.bias"], dt) for p in RES])


# ---------------------------------------------------------------- the launches
def conv_in(sd, x, dt):
    """input_blocks.0: Conv1d(32 -> 192, k 3); x (B, 32, T) -> H0 (B, 192, T)."""
    return _conv3(x.to(dt), sd["model.input_blocks.0.0.weight"], dt) + sd["model.input_blocks.0.0.bias"].to(dt)[None, :, None]


def res_operand1(sd, i, xs, dt):
    """The operand of ResBlock i's first convolution, SiLU(GroupNorm(cat(xs))) (B, cin, T): what prep_kernel stores for fgemm_kernel on the large-batch route."""
    p = RES[i]
    x = torch.cat([t.to(dt) for t in xs], dim=1)
    return _silu(group_norm(x, 32, sd[p + ".in_layers.0.weight"], sd[p + ".in_layers.0.bias"], 1e-5, dt))


def res_operand2(sd, i, m, dt):
    """... of its second convolution, SiLU(GroupNorm(m))."""
    p = RES[i]
    return _silu(group_norm(m, 32, sd[p + ".out_layers.0.weight"], sd[p + ".out_layers.0.bias"], 1e-5, dt))


def qkv_operand(sd, j, x, dt):
    """... of SpatialTransformer j's q/k/v projection, LayerNorm(GroupNorm(x)) token-major (B, T, 192)."""
    p, tb = ST[j], ST[j] + ".transformer_blocks.0"
    g = group_norm(x, 32, sd[p + ".norm.weight"], sd[p + ".norm.bias"], 1e-6, dt).transpose(1, 2)
    return _ln(g, sd[tb + ".norm1.weight"], sd[tb + ".norm1.bias"], dt)


def res_conv1(sd, i, xs, e_row, dt, operand=None):
    """ResBlock i, in_layers + emb: GroupNorm(32 groups over the concatenated channels, eps 1e-5) + SiLU, conv3, bias, the timestep row; xs: one or two (B, 192, T)
    sources (two: the K segments of the concatenated input), e_row (B, 192) as read from EO -> M.  operand: the stored operand (res_operand1) instead of xs."""
    p = RES[i]
    h = res_operand1(sd, i, xs, dt) if operand is None else operand.to(dt)
    e = e_row.to(dt)
    if _m("emb_row_of_other_sample"):
        e = e.roll(1, 0)
    return _conv3(h, sd[p + ".in_layers.2.weight"], dt) + (sd[p + ".in_layers.2.bias"].to(dt)[None] + e)[..., None]


def res_conv2(sd, i, m, xs, dt, operand=None):
    """ResBlock i, out_layers + skip: GroupNorm + SiLU + conv3 of m, then + xs[0] (one source) or + the 1x1 skip convolution over the concatenated raw sources
    (two more K segments) -> (y, y2): y2 is the duplicate store of the guidance-shared block (a copy of y in the conditional half's slots).
    operand: the stored operand (res_operand2) instead of m."""
    p = RES[i]
    h = res_operand2(sd, i, m, dt) if operand is None else operand.to(dt)
    y = _conv3(h, sd[p + ".out_layers.3.weight"], dt) + sd[p + ".out_layers.3.bias"].to(dt)[None, :, None]
    if len(xs) == 2:
        x = torch.cat([t.to(dt) for t in xs], dim=1)
        w = sd[p + ".skip_connection.weight"].to(dt)[:, :, 0]
        y = y + torch.einsum("nc,bct->bnt", _op(w), _op(x)) + sd[p + ".skip_connection.bias"].to(dt)[None, :, None]
    else:
        r = xs[0].to(dt)
        y = y + (r.roll(1, 0) if _m("residual_of_neighbour_sample") else r)
    return y, (torch.zeros_like(y) if _m("y2_not_written") else y.clone())


def qkv(sd, j, x, dt, operand=None):
    """SpatialTransformer j: GroupNorm(eps 1e-6) -> LayerNorm(norm1) -> to_q | to_k | to_v of the block input x (B, 192, T)
    -> q, k (B, 6, T, 32) token-major per head (QK's layout), v (B, 192, T) channel-major (VT's).  operand: the stored operand (qkv_operand) instead of x."""
    tb = ST[j] + ".transformer_blocks.0"
    y = qkv_operand(sd, j, x, dt) if operand is None else operand.to(dt)
    B, T, _ = y.shape
    q, k, v = (_lin(y, sd[tb + f".attn1.to_{n}.weight"], None, dt) for n in "qkv")
    heads = lambda t: t.reshape(B, T, HEADS, HD).permute(0, 2, 1, 3)
    return heads(q), heads(k), v.transpose(1, 2)


def self_attention(q, k, v, dt):
    """softmax(q k^T / sqrt(32)) v; q, k (B, 6, T, 32), v (B, 192, T) -> O (B, 192, T) channel-major."""
    B, _, T, _ = q.shape
    q, k = _op(q.to(dt)), _op(k.to(dt))
    vh = _op(v.to(dt)).reshape(B, HEADS, HD, T)
    s = q @ k.transpose(2, 3) * SCALE
    if _m("last_key_tile_missing"):
        s[..., (T - 1) // 32 * 32:] = -torch.finfo(dt).max
    return (_op(torch.softmax(s, dim=-1)) @ vh.transpose(2, 3)).permute(0, 1, 3, 2).reshape(B, MC, T)


def alignment_mask(T: int, S: int) -> torch.Tensor:
    from oracle import unet as ou
    return ou.alignment_mask(1, T, S)[0]


def c2_const(sd, j, null, dt):
    """The unconditional half's cross-attention output: every key is the null embedding, so the softmax averages identical values -> to_out(to_v(null)) + bias, (192,)."""
    tb = ST[j] + ".transformer_blocks.0"
    v = sd[tb + ".attn2.to_v.weight"].to(dt) @ null.to(dt).reshape(-1)
    return sd[tb + ".attn2.to_out.0.weight"].to(dt) @ v + sd[tb + ".attn2.to_out.0.bias"].to(dt)


def folded_proj_out(sd, j):
    """proj_out o ff.net.2 in float64: (P F2, P, P b2 + bp) (weights.cpp fold_ffproj)."""
    p, tb = ST[j], ST[j] + ".transformer_blocks.0"
    P = sd[p + ".proj_out.weight"].reshape(MC, MC).double()
    return P @ sd[tb + ".ff.net.2.weight"].double(), P, P @ sd[tb + ".ff.net.2.bias"].double() + sd[p + ".proj_out.bias"].double()


def _tb(sd, j):
    return lambda n: sd[ST[j] + ".transformer_blocks.0" + n]


def coef_from_partials(sd, j, st, T, dt):
    """The block input's GroupNorm (32 groups, eps 1e-6) as (a, b) rows from its producer's stored partials (n, np, 192, 2), merged as the RES_GN epilogue merges
    them -> (n, 192, 2)."""
    mean, var = merge_partials(st, T, MC // 32)
    rstd = (1.0 / torch.sqrt(var + 1e-6)).repeat_interleave(MC // 32, dim=1)
    a = sd[ST[j] + ".norm.weight"].double()[None] * rstd
    b = sd[ST[j] + ".norm.bias"].double()[None] - mean.repeat_interleave(MC // 32, dim=1) * a
    return torch.stack([a, b], dim=-1).to(dt)


def to_out1(sd, j, o, xin, gn, dt, null=None):
    """Launch 1 of the five-launch tail: x1 = attn1.to_out(o) + GroupNorm(xin).  o, xin (n, 192, T) channel-major as stored; gn: the (a, b) rows (n, 192, 2) that
    fgemm_kernel reads (and stchain_kernel), or the producer's partials (n, np, 192, 2) that ugemm_kernel's RES_GN epilogue merges itself.
    -> (x1, y2): y2 = x1 + c2, the duplicate the guided step stores into X2 for every sample of the launch (null given), else None."""
    W = _tb(sd, j)
    T = o.shape[-1]
    coef = coef_from_partials(sd, j, gn, T, dt) if gn.dim() == 4 else gn.to(dt)
    g = xin.to(dt) * coef[..., 0, None] + coef[..., 1, None]
    x1 = _lin(o.to(dt).transpose(1, 2), W(".attn1.to_out.0.weight"), W(".attn1.to_out.0.bias"), dt).transpose(1, 2) + g
    if null is None:
        return x1, None
    return x1, (x1.clone() if _m("y2_without_c2") else x1 + c2_const(sd, j, null, dt)[None, :, None])


def q2(sd, j, x1, dt):
    """attn2.to_q(norm2(x1)); x1 (n, 192, T) -> (n, 192, T) channel-major: what the plain projection in front of band_wide_kernel stores."""
    W = _tb(sd, j)
    return _lin(_ln(x1.to(dt).transpose(1, 2), W(".norm2.weight"), W(".norm2.bias"), dt), W(".attn2.to_q.weight"), None, dt).transpose(1, 2)


def band_mask(T: int, S: int) -> torch.Tensor:
    """alignment_mask(T, S) (True: masked) with the mutants of the band's seams."""
    mask = alignment_mask(T, S)
    if _m("band_shifted"):
        mask = mask.roll(1, 1)
    width = (~mask).sum(1)
    if int(width.max()) > 8:
        lo = (~mask).int().argmax(1)
        if _m("band_truncated_to_8_keys"):   # the fused epilogue's eight keys where the window is wider
            mask = mask | (torch.arange(S)[None] >= (lo + 8)[:, None])
        if _m("wide_band_off_by_one"):       # band_wide_kernel's window one key further: [lo + 1, hi + 1)
            mask = mask.roll(1, 1)
            mask[:, 0] = True
    return mask


def band(q, k2, v2, T, S, dt):
    """The banded softmax over the stored K / V of the context: q (n, 192, T) channel-major, k2, v2 (n, 192, S) -> (n, 192, T).  band_wide_kernel in place, or
    the second half of the EPI_BAND epilogue."""
    n = q.shape[0]
    qh = q.to(dt).reshape(n, HEADS, HD, T).transpose(2, 3)
    kh = k2.to(dt).reshape(n, HEADS, HD, S)
    vh = v2.to(dt).reshape(n, HEADS, HD, S)
    s = (qh @ kh * SCALE).masked_fill(band_mask(T, S)[None, None], -torch.finfo(dt).max)
    return (torch.softmax(s, dim=-1) @ vh.transpose(2, 3)).permute(0, 1, 3, 2).reshape(n, MC, T)


def q_band(sd, j, x1, k2, v2, T, S, dt):
    """Launch 2: to_q(norm2(x1)) and the banded softmax at any window width — the fused EPI_BAND epilogue, or the plain projection followed by band_wide_kernel."""
    return band(q2(sd, j, x1, dt), k2, v2, T, S, dt)


def to_out2(sd, j, o2, x1, dt, x_off=0, kv_off=0, x2=None):
    """Launch 3: x2 = attn2.to_out(o2) + x1 for the n samples of o2 (the cross-attention range).  x1: the whole stored X1, read from sample x_off on; x2: the stored
    X2 before the launch (the guided step: y2 of launch 1 in every slot) — then the result is that buffer with slots [kv_off, kv_off + n) alone replaced."""
    W = _tb(sd, j)
    n = o2.shape[0]
    r = x1[0:n] if (_m("x1_of_wrong_sample_under_x_off") and x_off) else x1[x_off:x_off + n]
    y = _lin(o2.to(dt).transpose(1, 2), W(".attn2.to_out.0.weight"), W(".attn2.to_out.0.bias"), dt).transpose(1, 2) + r.to(dt)
    if x2 is None:
        return y
    out = x2.to(dt).clone()
    out[kv_off:kv_off + n] = y
    if _m("to_out2_writes_uncond_slot") and kv_off:
        out[0:n] = y
    return out


def geglu_operand(sd, j, x2, dt):
    """norm3(x2) token-major (n, T, 192): what the third preparation launch of the large-batch route stores for fgemm_kernel."""
    W = _tb(sd, j)
    return _ln(x2.to(dt).transpose(1, 2), W(".norm3.weight"), W(".norm3.bias"), dt)


def geglu(sd, j, x2, dt, operand=None):
    """Launch 4: ff.net.0 over norm3(x2), value x gelu(gate); x2 (n, 192, T) -> F (n, 768, T).  operand: the stored operand (geglu_operand) instead of x2."""
    W = _tb(sd, j)
    y = geglu_operand(sd, j, x2, dt) if operand is None else operand.to(dt)
    hv = _lin(y, W(".ff.net.0.proj.weight"), W(".ff.net.0.proj.bias"), dt)
    a, gate = hv.chunk(2, dim=-1)
    if _m("geglu_swapped"):
        a, gate = gate, a
    return (a * _gelu(gate)).transpose(1, 2)


def ffproj(sd, j, h, x2, xin, dt):
    """Launch 5: the folded proj_out over the K segments [h ; x2] (weights folded in float64, weights.cpp fold_ffproj) + bias + x_in; h (n, 768, T), x2, xin
    (n, 192, T) -> the block's output (n, 192, T).  (Its GroupNorm partials are held to the stored output on their own: norm_from_partials.)"""
    PF, P, PB = folded_proj_out(sd, j)
    y = _lin(h.to(dt).transpose(1, 2), PF, None, dt)
    if not _m("ffproj_second_segment_dropped"):
        y = y + _lin(x2.to(dt).transpose(1, 2), P, None, dt)
    return (y + PB.to(dt)).transpose(1, 2) + xin.to(dt)


def chain(sd, j, o, xin, coef, k2, v2, dt, nsamp=None, in_mod=0, n_uncond=0, null=None):
    """stchain_kernel's whole tail of SpatialTransformer j: the five launches composed.  o, xin (n_in, 192, T): the self-attention output and the block input; coef
    (n_in, 192, 2): the GroupNorm (a, b) rows as stored; k2, v2 (nsamp, 192, S): block j's rows of the stored KV (those of unconditional samples are never read).
    Output sample s reads input sample s % in_mod (in_mod > 0: the guidance-shared block), samples [0, n_uncond) are unconditional: x2 = x1 + c2 instead of the
    cross-attention.  -> the block's output (nsamp, 192, T)."""
    n_in, _, T = o.shape
    nsamp = n_in if nsamp is None else nsamp
    idx = torch.arange(nsamp) % in_mod if in_mod else torch.arange(nsamp)
    x1, y2 = to_out1(sd, j, o, xin, coef, dt, null=null if n_uncond else None)
    x1 = x1[idx]
    x2 = to_out2(sd, j, q_band(sd, j, x1, k2, v2, T, k2.shape[-1], dt), x1, dt)
    if n_uncond and not _m("uncond_runs_cross_attention"):
        x2 = torch.cat([y2[idx][:n_uncond], x2[n_uncond:]])
    return ffproj(sd, j, geglu(sd, j, x2, dt), x2, xin[idx], dt)


def out_conv(sd, h, dt):
    """out: GroupNorm(eps 1e-5) + SiLU + Conv1d(192 -> 32, k 3); h (B, 192, T) -> eps (B, 32, T)."""
    y = _silu(group_norm(h, 32, sd["model.out.0.weight"], sd["model.out.0.bias"], 1e-5, dt))
    return _conv3(y, sd["model.out.2.weight"], dt) + sd["model.out.2.bias"].to(dt)[None, :, None]


def step_update(e_c, e_u, x, cf, gs, dt, noise=None, init=None, enoise=None, mask=None):
    """sched_math.h step_update for a DDIM row with epsilon prediction: guidance, x0 (clipped), the update, eta noise, the editing-mask blend.  cf: the fp32
    coefficient row (sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), direction factor, eta std, the blend's pair for the next timestep); tensors of any common shape."""
    c = [torch.tensor(float(v), dtype=torch.float32).to(dt) for v in cf[:7]]
    e_c = e_c.to(dt)
    e = e_c if e_u is None else e_c + gs * (e_c - e_u.to(dt))
    x = x.to(dt)
    x0 = ((x - c[1] * e) / c[0]).clamp(-1.0, 1.0)
    prev = c[2] * x0 + c[3] * e
    if noise is not None:
        prev = prev + c[4] * noise.to(dt)
    if mask is not None:
        noisy = c[5] * init.to(dt) + c[6] * enoise.to(dt)
        m = mask.to(dt)
        prev = noisy * (1.0 - m) + prev * m if _m("mask_blend_order") else noisy * m + prev * (1.0 - m)
    return prev


def out_sched(sd, h, x, cf, gs, dt, **kw):
    """out_sched_kernel<CFG>: the out convolution of both halves (unconditional first), guidance, the update; h (2 B, 192, T), x (B, 32, T) -> (B, 32, T)."""
    B = x.shape[0]
    eps = out_conv(sd, h, dt)
    return step_update(eps[B:], eps[:B], x, cf, gs, dt, **kw)


# ---------------------------------------------------------------- the context's K / V (run_kv; once per call, not a launch of the step)
def kv_all(sd, ctx, dt):
    """KV: to_k | to_v of the four blocks' cross-attention over the context (B, S, 768) -> (B, 4 * 384, S): block j's K rows, then its V rows."""
    w = torch.cat([sd[ST[j] + f".transformer_blocks.0.attn2.to_{n}.weight"] for j in range(NST) for n in "kv"], 0)
    return _lin(ctx.to(dt), w, None, dt).transpose(1, 2)


# ---------------------------------------------------------------- the launches chained (tests/test_unet_f32_ref_cpu.py: against the oracle)
def forward(sd, x, ts, ctx, dt, n_clips=0, null=None, trace=None):
    """run_unet on x (B, 32, T) channel-major -> eps (B, 32, T), or the last hidden state when n_clips > 0 asks for the guided step's schedule: x holds the n_clips
    clips' latents once, every tensor behind the shared first block has 2 n_clips samples (unconditional first), ctx the clips' context.
    trace: a list that receives (launch name, output) in launch order."""
    t = (lambda n, v: trace.append((n, v))) if trace is not None else (lambda n, v: None)
    Bc = n_clips
    rows = time_rows(sd, ts, dt)                                   # (5, N, 192)
    kv = kv_all(sd, ctx, dt)
    if Bc:   # the unconditional half's rows are never read
        kv = torch.cat([torch.zeros_like(kv), kv])
    e = lambda i, n: rows[i][:n] if not Bc else rows[i][:1].expand(n, -1)
    H0 = conv_in(sd, x, dt)
    t("conv_in", H0)

    def res(i, xs, shared=False):
        n = xs[0].shape[0]
        m = res_conv1(sd, i, xs, e(i, n), dt)
        t(f"res{i}.conv1", m)
        y, y2 = res_conv2(sd, i, m, xs, dt)
        t(f"res{i}.conv2", y)
        return (y, y2) if shared else y

    def st(j, x_in, shared=False):
        q, k, v = qkv(sd, j, x_in, dt)
        t(f"st{j}.qkv", (q, k, v))
        o = self_attention(q, k, v, dt)
        t(f"st{j}.attn", o)
        ks, vs = kv[:, j * 2 * MC:j * 2 * MC + MC], kv[:, j * 2 * MC + MC:(j + 1) * 2 * MC]
        y = chain(sd, j, o, x_in, gn_coef(sd, j, x_in, dt), ks, vs, dt, nsamp=2 * Bc if Bc else None, in_mod=Bc if shared else 0, n_uncond=Bc, null=null)
        t(f"st{j}.chain", y)
        return y

    if Bc:
        P, _ = res(0, [H0], shared=True)
        H1 = st(0, P, shared=True)
        H0 = torch.cat([H0, H0])
    else:
        H1 = st(0, res(0, [H0]))
    Q = st(1, res(1, [H1]))
    P = res(2, [Q])
    P = st(2, res(3, [P, H1]))
    P = st(3, res(4, [P, H0]))
    if Bc:
        return P
    eps = out_conv(sd, P, dt)
    t("out", eps)
    return eps
