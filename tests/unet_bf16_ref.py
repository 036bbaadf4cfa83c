"""Launch-by-launch restatement of the token-major bf16 denoise step (said_amd/csrc/unet_sched.cpp: run_resblock_tm / run_transformer_tm / run_tm_tail) — TEST INFRASTRUCTURE.

One function per launch of bf16 mode's large-batch schedule: conv_in_kernel<TM>, rgemm_kernel's variants (RG_VARIANTS, rgemm_plan.h), battn_kernel, stchain_kernel<bf16>, the
channel-major xgemm_kernel proj_out and the out convolution.  Each takes the launch's inputs AS THE ENGINE STORES THEM — token-major activations (B, T, 192) holding bf16
values, without the pad tokens; GroupNorm partials [B][32-token tile][192][(mean, M2)] of the producer; q / k per head, v per channel — plus the UNet state dict and
    rounded  True: both operands of every product that runs on v_mfma_f32_32x32x16_bf16 are rounded to bf16 (nearest even) WHERE THE KERNEL ROUNDS THEM, sums in `dtype`;
             False: the same function without any rounding — chained in schedule order that is the oracle (tests/test_unet_bf16_ref_cpu.py);
    dtype    torch.float64 for the reference, torch.float32 for the evaluation that measures how far a correct fp32 accumulation may sit from it;
    store    False: the value before the store's rounding.
What is restated is the kernels, not the oracle: GroupNorm coefficients (a, b) come from the producer's partials and are fp32 tables (gemm_common.h gn20_finish); the
fused tail's LayerNorm affines are folded into the next product's weights before rounding and proj_out o ff.net.2 is formed in double (weights.cpp fold_ffproj,
weight_pack.h fold_gamma) while rgemm_kernel's LayerNorm applies its affine itself; the bf16 partial sum between the column-range launches is kept; q is multiplied by
fp32(ATTN_SCALE * LOG2E) before its rounding; v is stored token-permuted per 16; the fused tail's K / V window tiles are the bf16 key-major copy; battn_kernel's online
softmax keeps a per-query reference taken from the first key tile's maximum, moves it only when a later tile exceeds it by more than 16 in the exponent, rounds the
probabilities to bf16 and sums the ROUNDED probabilities (its ones-MFMA).

The rules (check_* below and in audio_bf16_ref.py) are the project's: layout-only stores exact; a single product with an fp32 store within 4 max(e32, 1e-6) of range
(check_f32); with a bf16 store >= 99 % bit-equal and every element within one bf16 step or that bound (check_bf16).  Where the kernel transforms its operand itself
(silu(GroupNorm), LayerNorm, LayerNorm(GroupNorm)) an operand within delta = 4 max(max |t32 - t64|, 1e-6 max |t64|) of a bf16 rounding boundary may round either way:
an output element's bound grows by sum |w| step(t) over its ambiguous operands (flip_allowance) — the 99 % floor stays.  single_stats states the element rule, with its
one deviation from the letter (beside a non-zero allowance the stored value is also measured against the UNROUNDED reference, + half a step) and the reason; GEGLU's floor
is asked of the elements whose gate leaves gelu relative accuracy in fp32 (geglu_parts' floor_mask), its element bound of all.  Launches with several dependent products
(the fused tail, the q projection + band, attention) are held by check_multi: >= 97 % bit-equal, every element within max(one bf16 step, cap), attention also by
audio_bf16_ref.check_attention.

CAPS: the cap of a multi-product launch is 4 x the largest pre-store |fp32 - float64| of this reference's own pair (the 4: the GPU's summation order and exp / erf
differ from torch's), of max |ref|, over 64 seeded evaluations of the network at T = 70 per fill — each gives the four blocks' launches, 256 pairs per kind — and, for
battn_kernel, 8 more at T = 290 and 8 with to_q / to_k x 8 (its rebase branch); tests/test_unet_bf16_ref_cpu.py::test_caps_are_the_measured_ones measures them again.
A cap above 1e-2 means that the fill, not the kernel, is at fault, and the rule keeps 1e-2.  Measured (largest difference -> cap):
    fused tail (stchain_kernel<bf16>)   plain 1.23e-3 -> 4.9e-3     trained-like 6.9e-3 -> 2.8e-2, kept at 1.0e-2 (one outlier pair in 256; the next is 2.0e-3)
    q projection + band                 plain 6.7e-4 -> 2.7e-3      trained-like 6.0e-4 -> 2.4e-3
    battn_kernel                        plain 6.4e-4 -> 2.5e-3      trained-like 7.8e-4 -> 3.1e-3
MUTANTS: twelve ways a kernel of the step can be wrong; each fails the rule of its launch at least ten times over on the CPU (tests/test_unet_bf16_ref_cpu.py: 79 x,
the band off by one row inside the fused tail, ... 1.3e3 x).  rebase_skipped shows in the result only where a score exceeds the reference by 128 in the exponent
(the probability overflows fp32; below that a skipped rebase changes nothing but fp32 rounding): its case scales to_q / to_k by 2^6, and its factor is infinite.
MUTANT: tests/test_unet_bf16_ref_cpu.py sets it to one of MUTANTS to prove that each rule has teeth.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from audio_bf16_ref import F32_FACTOR, F32_FLOOR, bf16_stats, bf16_step, f32_bound, round_bf16
from unet_f32_ref import (FFI, HD, HEADS, MC, NST, RES, ST, alignment_mask, c2_const, folded_proj_out, kv_all, rup, step_update, time_rows)  # noqa: F401

ATTN_SCALE = float(torch.tensor(0.17677669529663687, dtype=torch.float32))
LOG2E = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
Q_SCALE = float(torch.tensor(ATTN_SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))   # unet_sched.cpp: t.q_scale = ATTN_SCALE * LOG2E in fp32
REBASE = 16.0


def _scales(rounded):
    """(attention scale, q's factor): the kernels' fp32 constants, or — without roundings — the numbers they stand for."""
    return (ATTN_SCALE, Q_SCALE) if rounded else (HD ** -0.5, HD ** -0.5 * math.log2(math.e))

MUTANTS = ("tap_shifted", "k_dropped", "gn_neighbour_sample", "gn_ring_wrapped", "v_permutation_undone", "last_key_tile_unmasked", "rebase_skipped", "band_off_by_one",
           "geglu_swapped", "partial_sum_dropped", "c2_on_conditional_half", "gn_over_pitch")
MUTANT = None

# multi-product launches: cap / max |ref| per (launch kind, fill); measured by tests/test_unet_bf16_ref_cpu.py (64 draws, T = 70; the figure behind each is the largest
# pre-store |fp32 - float64| of the reference pair, x 4)
CAPS = {("chain", "plain"): 4.907e-3, ("chain", "trained"): 1.0e-2, ("band", "plain"): 2.669e-3, ("band", "trained"): 2.391e-3,
        ("battn", "plain"): 2.546e-3, ("battn", "trained"): 3.123e-3}


def _m(name: str) -> bool:
    assert name in MUTANTS
    return MUTANT == name


# ---------------------------------------------------------------- roundings and statistics
def _rb(x, rounded):
    return round_bf16(x) if rounded else x


def _store(y, rounded, store):
    return round_bf16(y) if (rounded and store) else y


def _f32(y, rounded, store):
    return y.float().to(y.dtype) if (rounded and store) else y


def partials(y, T=None):
    """GroupNorm partials of y (B, T, C) as the producers store them: (mean, M2) per 32-token tile and channel -> (B, np, C, 2) in y's dtype."""
    B, T_, C = y.shape
    out = []
    for t0 in range(0, T_, 32):
        t = y[:, t0:t0 + 32]
        m = t.mean(1)
        out.append(torch.stack([m, ((t - m[:, None]) ** 2).sum(1)], -1))
    return torch.stack(out, 1)


def gn_coef(st, T, gamma, beta, eps, cpg, rounded, dtype):
    """(a, b) per (sample, channel), y = a x + b, from a producer's partials [B][tile][C][2] (gemm_common.h gn20_finish: Chan's merge over tiles and the group's
    channels; the tables are fp32).  cpg: channels per group (6; 12 for one source of a concatenated input)."""
    B, npart, C, _ = st.shape
    dt = dtype
    Tn = T
    cnt = torch.tensor([min(32, T - 32 * p) for p in range(npart)], dtype=dt).view(1, npart, 1)
    mean_pc, m2_pc = st[..., 0].to(dt), st[..., 1].to(dt)
    G = C // cpg
    if _m("gn_over_pitch"):   # the statistics divided by the padded token count
        Tn = rup(T, 32)
    gm = (cnt * mean_pc).view(B, npart, G, cpg).sum(dim=(1, 3)) / (cpg * Tn)
    gm_c = gm.repeat_interleave(cpg, dim=1).view(B, 1, C)
    m2 = (m2_pc + cnt * (mean_pc - gm_c) ** 2).view(B, npart, G, cpg).sum(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(m2 / (cpg * Tn) + eps)
    a = gamma.to(dt).view(1, C) * rstd.repeat_interleave(cpg, dim=1)
    b = beta.to(dt).view(1, C) - gm.repeat_interleave(cpg, dim=1) * a
    if rounded:
        a, b = a.float().to(dt), b.float().to(dt)
    if _m("gn_neighbour_sample"):   # slot (b + 1) & 3 of the table ring
        a, b = a.roll(-1, 0), b.roll(-1, 0)
    if _m("gn_ring_wrapped"):       # the slot still holds the table of four samples earlier
        a, b = a.roll(4, 0), b.roll(4, 0)
    return a, b


def _silu(x):
    return x * torch.sigmoid(x)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def _ln(x, g=None, b=None):
    """rgemm_kernel's helper waves / the fused tail: two-pass LayerNorm over 192 channels, eps 1e-5."""
    mu = x.mean(-1, keepdim=True)
    y = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    return y if g is None else y * g.to(x.dtype) + b.to(x.dtype)


# ---------------------------------------------------------------- a launch in three parts
class Parts:
    """t: the product's operand before its rounding (dtype); prod(op, absw): the product with the (rounded) weights, absw: with their magnitudes; epi(acc): the
    epilogue up to the value that is stored; transforms: the kernel makes t itself (flip_allowance applies); floor_mask(): the elements the bit-equal floor is asked of
    (None: all)."""

    def __init__(self, t, prod, epi, transforms, round_op=True, floor_mask=None):
        self.t, self.prod, self.epi, self.transforms, self.round_op, self.floor_mask = t, prod, epi, transforms, round_op, floor_mask


def finish(p: Parts, rounded, store, bf16=True):
    y = p.epi(p.prod(_rb(p.t, rounded and p.round_op), False))
    return _store(y, rounded, store) if bf16 else _f32(y, rounded, store)


def flip_allowance(p64: Parts, p32: Parts):
    """sum |w| step(t) over the operands whose rounding the kernel's own fp32 transform may decide the other way (module docstring) -> (allowance per output element,
    share of ambiguous operands)."""
    if not p64.transforms:
        return 0.0, 0.0
    t64 = p64.t
    delta = F32_FACTOR * max(float((p32.t.double() - t64).abs().max()), F32_FLOOR * float(t64.abs().max()))
    amb = round_bf16(t64 - delta) != round_bf16(t64 + delta)
    return p64.prod(amb.to(t64.dtype) * torch.maximum(bf16_step(t64 - delta), bf16_step(t64 + delta)), True), float(amb.double().mean())


def _conv3(h, w, absw=False):
    """Conv1d(k 3, padding 1) over token-major h (B, T, C) with w (N, C, 3): tap k reads token t + k - 1, zeros outside [0, T)."""
    B, T, C = h.shape
    w = w.abs() if absw else w
    hp = F.pad(h, (0, 0, 1, 2))
    taps = [hp[:, k:k + T] for k in range(3)]
    y = sum(taps[k] @ w[:, :, k].t() for k in range(3))
    if not absw and T > 32 and (_m("tap_shifted") or _m("k_dropped")):   # one token tile of sample 0: tokens [32, 64)
        tp = list(taps)
        wk = w.clone()
        if _m("tap_shifted"):
            tp[2] = hp[:, 3:3 + T]
        else:
            wk[:, 64:72, 0] = 0   # one k8 half of a k16 step of tap 0
        yd = sum(tp[k] @ wk[:, :, k].t() for k in range(3))
        y = y.clone()
        y[0, 32:64] = yd[0, 32:64]
    return y


def _lin(x, w, absw=False):
    return x @ (w.abs() if absw else w).t()


def _w(w, rounded, dtype):
    return _rb(w.to(dtype), rounded)


# ---------------------------------------------------------------- conv_in_kernel<TM>
def conv_in_parts(sd, x, rounded=True, dtype=torch.float64):
    """input_blocks.0 on fp32 matrix instructions (no bf16 operand); x (B, 32, T) channel-major latents."""
    w = sd["model.input_blocks.0.0.weight"].to(dtype)
    return Parts(x.to(dtype).transpose(1, 2), lambda op, absw: _conv3(op, w, absw), lambda acc: acc + sd["model.input_blocks.0.0.bias"].to(dtype), False, round_op=False)


def conv_in(sd, x, rounded=True, dtype=torch.float64, store=True):
    """-> (H0 (B, T, 192) bf16, the partials — of the fp32 values, not of their bf16 store)."""
    y = finish(conv_in_parts(sd, x, rounded, dtype), rounded, False)
    return _store(y, rounded, store), partials(_f32(y, rounded, True))


# ---------------------------------------------------------------- rgemm_kernel: the ResBlock convolutions
def conv_parts(x, st_x, gamma, beta, cpg, w, add, res, rounded, dtype):
    """<3, 0, 1, RES, DUP, STATS>: silu(GroupNorm(x)) from the producer's partials -> conv3 with w (192, 192, 3) -> + add (B, 192) or (192,) + res (B, T, 192)."""
    T = x.shape[1]
    a, b = gn_coef(st_x, T, gamma, beta, 1e-5, cpg, rounded, dtype)
    t = _silu(x.to(dtype) * a[:, None] + b[:, None])
    wr = _w(w, rounded, dtype)
    addv = add.to(dtype)
    addv = addv[:, None] if addv.dim() == 2 else addv

    def epi(acc):
        y = acc + addv
        return y if res is None else y + res.to(dtype)
    return Parts(t, lambda op, absw: _conv3(op, wr, absw), epi, True)


def res_conv1_parts(sd, i, x, st_x, e_row, rounded=True, dtype=torch.float64):
    """ResBlock i (one source), in_layers + the timestep row e_row (B, 192) as read from EO."""
    p = RES[i]
    return conv_parts(x, st_x, sd[p + ".in_layers.0.weight"], sd[p + ".in_layers.0.bias"], 6, sd[p + ".in_layers.2.weight"],
                      sd[p + ".in_layers.2.bias"].to(dtype)[None] + e_row.to(dtype), None, rounded, dtype)


def res_conv2_parts(sd, i, m, st_m, x, rounded=True, dtype=torch.float64):
    """ResBlock i (one source), out_layers + the identity skip x."""
    p = RES[i]
    return conv_parts(m, st_m, sd[p + ".out_layers.0.weight"], sd[p + ".out_layers.0.bias"], 6, sd[p + ".out_layers.3.weight"], sd[p + ".out_layers.3.bias"], x, rounded, dtype)


def cat_conv1a_parts(sd, i, x0, st0, rounded=True, dtype=torch.float64):
    """Concatenated-input ResBlock i, in_layers over source 0's 192 input channels (GroupNorm groups of 12) -> the bf16 partial sum (<3, 0, 1, 0, false, false>)."""
    p = RES[i]
    return conv_parts(x0, st0, sd[p + ".in_layers.0.weight"][:MC], sd[p + ".in_layers.0.bias"][:MC], 12, sd[p + ".in_layers.2.weight"][:, :MC], torch.zeros(MC), None, rounded, dtype)


def cat_conv1b_parts(sd, i, x1, st1, part, e_row, rounded=True, dtype=torch.float64):
    """... over source 1's channels + bias + timestep row + the stored partial sum -> M."""
    p = RES[i]
    part = torch.zeros_like(part) if _m("partial_sum_dropped") else part
    return conv_parts(x1, st1, sd[p + ".in_layers.0.weight"][MC:], sd[p + ".in_layers.0.bias"][MC:], 12, sd[p + ".in_layers.2.weight"][:, MC:],
                      sd[p + ".in_layers.2.bias"].to(dtype)[None] + e_row.to(dtype), part, rounded, dtype)


def cat_skip_parts(sd, i, x0, x1, rounded=True, dtype=torch.float64):
    """... the 1x1 skip convolution over the raw concatenated input, two 192-channel chunks (<1, 0, 0, 0, false, false, 2>; its bias rides with conv 2's)."""
    w = _w(sd[RES[i] + ".skip_connection.weight"][:, :, 0], rounded, dtype)
    return Parts(torch.cat([x0, x1], -1).to(dtype), lambda op, absw: _lin(op, w, absw), lambda acc: acc, False)


def cat_conv2_parts(sd, i, m, st_m, skip, rounded=True, dtype=torch.float64):
    """... out_layers + both biases + the stored skip product."""
    p = RES[i]
    return conv_parts(m, st_m, sd[p + ".out_layers.0.weight"], sd[p + ".out_layers.0.bias"], 6, sd[p + ".out_layers.3.weight"],
                      sd[p + ".out_layers.3.bias"].to(dtype) + sd[p + ".skip_connection.bias"].to(dtype), skip, rounded, dtype)


def with_stats(p: Parts, rounded, store=True):
    """(stored bf16 result, GroupNorm partials of the STORED values) of a launch with STATS."""
    y = finish(p, rounded, store)
    return y, partials(y)


# ---------------------------------------------------------------- rgemm_kernel: q / k / v
V_ORDER = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)   # stored position -> token inside a block of 16 (TGemmArgs::qkv_bf16)


def v_stored(v):
    """v (B, 192, Tp) in token order -> as stored for battn_kernel (Tp a multiple of 16)."""
    if _m("v_permutation_undone"):
        return v
    B, C, Tp = v.shape
    return v.view(B, C, Tp // 16, 16)[..., list(V_ORDER)].reshape(B, C, Tp)


def v_tokens(v_st):
    """The inverse: stored v -> token order (the permutation is an involution)."""
    B, C, Tp = v_st.shape
    return v_st.view(B, C, Tp // 16, 16)[..., list(V_ORDER)].reshape(B, C, Tp)


def qkv_parts(sd, j, x, st_x, rounded=True, dtype=torch.float64, scaled=False):
    """<1, 1, 3, 0>: LayerNorm(norm1)(GroupNorm(eps 1e-6)(x)) -> [to_q | to_k | to_v] -> (B, T, 576).  scaled: q's columns times Q_SCALE, as the bf16 store has them
    (the kernel multiplies the fp32 sum; here the factor rides on the rounded weights, which is the same number in float64)."""
    p, tb = ST[j], ST[j] + ".transformer_blocks.0"
    a, b = gn_coef(st_x, x.shape[1], sd[p + ".norm.weight"], sd[p + ".norm.bias"], 1e-6, 6, rounded, dtype)
    t = _ln(x.to(dtype) * a[:, None] + b[:, None], sd[tb + ".norm1.weight"], sd[tb + ".norm1.bias"])
    w = _w(torch.cat([sd[tb + f".attn1.to_{n}.weight"] for n in "qkv"], 0), rounded, dtype)
    if scaled:
        w = torch.cat([w[:MC] * _scales(rounded)[1], w[MC:]], 0)
    return Parts(t, lambda op, absw: _lin(op, w, absw), lambda acc: acc, True)


def qkv_split(y, rounded, store, bf16=True):
    """(B, T, 576) of qkv_parts (scaled = bf16) -> q, k (B, 6, T, 32) and v (B, 192, T) in token order as stored: bf16 (battn_kernel) or fp32 (T > 640)."""
    B, T, _ = y.shape
    heads = lambda t: t.reshape(B, T, HEADS, HD).permute(0, 2, 1, 3)
    q, k, v = y[..., :MC], y[..., MC:2 * MC], y[..., 2 * MC:].transpose(1, 2)
    st = _store if bf16 else _f32
    return st(heads(q), rounded, store), st(heads(k), rounded, store), st(v, rounded, store)


def qkv_join(q, k, v):
    """The inverse layout: q, k (B, 6, T, 32), v (B, 192, T) -> (B, T, 576)."""
    B, H, T, _ = q.shape
    tm = lambda t: t.permute(0, 2, 1, 3).reshape(B, T, MC)
    return torch.cat([tm(q), tm(k), v.transpose(1, 2)], -1)


# ---------------------------------------------------------------- battn_kernel
def battn(q, k, v, rounded=True, dtype=torch.float64, store=True, stats=None):
    """q (pre-multiplied by Q_SCALE), k (B, 6, T, 32), v (B, 192, T) token order -> O (B, T, 192).  The kernel's online softmax, per query: scores are exponents of
    two; the reference is the first key tile's maximum and moves by mx only when a later tile's maximum exceeds it by more than 16; p = exp2(s - ref) rounded to
    bf16; the row sum is that of the ROUNDED p; the accumulators are rescaled when the reference moves.  stats: a dict that receives the share of (sample, head,
    query) rows that moved their reference after the first tile."""
    B, H, T, _ = q.shape
    q, k = q.to(dtype), k.to(dtype)
    vh = v.to(dtype).reshape(B, H, HD, T).transpose(2, 3)        # (B, 6, T, 32)
    s_all = q @ k.transpose(2, 3)
    ref = torch.zeros(B, H, T, dtype=dtype)
    o = torch.zeros(B, H, T, HD, dtype=dtype)
    ls = torch.zeros(B, H, T, dtype=dtype)
    moved = torch.zeros(B, H, T, dtype=torch.bool)
    nkt = (T + 31) // 32
    for kt in range(nkt):
        j0, j1 = kt * 32, min(kt * 32 + 32, T)
        s = s_all[..., j0:j1] - ref[..., None]
        vt = vh[:, :, j0:j1]
        if _m("last_key_tile_unmasked") and j1 - j0 < 32:   # the pad keys take part: K's pad rows hold the last key again, V's pad columns are zero
            npad = 32 - (j1 - j0)
            s = torch.cat([s, (s_all[..., T - 1:T] - ref[..., None]).expand(-1, -1, -1, npad)], -1)
            vt = torch.cat([vt, torch.zeros(B, H, npad, HD, dtype=dtype)], 2)
        mx = s.amax(-1)
        rebase = torch.ones_like(moved) if kt == 0 else (mx > REBASE)
        if kt and _m("rebase_skipped"):
            rebase = torch.zeros_like(moved)
        d = torch.where(rebase, mx, torch.zeros_like(mx))
        f = torch.zeros_like(mx) if kt == 0 else torch.exp2(-d)
        s, ref, o, ls = s - d[..., None], ref + d, o * f[..., None], ls * f
        if kt:
            moved |= rebase
        p = torch.exp2(s)
        if rounded:
            p = round_bf16(p.float().to(dtype))   # (fp32 first: a score 128 above the reference is inf in the kernel)
        o = o + p @ vt
        ls = ls + p.sum(-1)
    if stats is not None:
        stats["rebased"] = float(moved.double().mean())
    y = (o / ls[..., None]).permute(0, 2, 1, 3).reshape(B, T, MC)
    return _store(y, rounded, store)


# ---------------------------------------------------------------- the band, shared by the fused tail and rgemm_kernel<1, 4, 2, 0>
def _band(q, k2, v2, T, S, rounded=True):
    """q (n, T, 192) fp32-type values; k2, v2 (n, S, 192) key-major -> softmax over each query's window (fp32 in the kernels: no rounding inside) -> (n, T, 192)."""
    n = q.shape[0]
    dt = q.dtype
    sp = lambda t, L: t.reshape(n, L, HEADS, HD).permute(0, 2, 1, 3)
    mask = alignment_mask(T, S)
    if _m("band_off_by_one"):
        mask = mask.roll(1, 1)
    s = (sp(q, T) @ sp(k2.to(dt), S).transpose(2, 3) * _scales(rounded)[0]).masked_fill(mask[None, None], -torch.finfo(dt).max)
    return (torch.softmax(s, dim=-1) @ sp(v2.to(dt), S)).permute(0, 2, 1, 3).reshape(n, T, MC)


# ---------------------------------------------------------------- stchain_kernel<bf16>: everything behind the self-attention as one launch
def chain(sd, j, o, xin, st_x, k2, v2, rounded=True, dtype=torch.float64, store=True, nsamp=None, in_mod=0, n_uncond=0, null=None):
    """o, xin (n_in, T, 192) bf16 as stored; st_x: xin's partials; k2, v2 (nsamp, S, 192): block j's K / V rows of the bf16 key-major copy KVT.  Output sample s reads
    input sample s % in_mod (in_mod > 0: the guidance-shared block); samples [0, n_uncond) are unconditional: x2 = x1 + c2.  x1, x2 and q stay fp32 in registers
    and are rounded only as operands; LayerNorm 2 / 3's affines are folded into to_q / GEGLU before the weights are rounded.  -> (y (nsamp, T, 192), partials of the stored y)."""
    p, tb = ST[j], ST[j] + ".transformer_blocks.0"
    W = lambda n: sd[tb + n]
    dt = dtype
    r = lambda t: _rb(t, rounded)
    n_in, T, _ = o.shape
    nsamp = n_in if nsamp is None else nsamp
    idx = torch.arange(nsamp) % in_mod if in_mod else torch.arange(nsamp)
    fold = lambda w, g: (w.double() * g.double()[None]).float() if rounded else w.double() * g.double()[None]
    f32v = lambda v: v.float().to(dt) if rounded else v.to(dt)
    Wq = _w(fold(W(".attn2.to_q.weight"), W(".norm2.weight")), rounded, dt)
    bq = f32v(W(".attn2.to_q.weight").double() @ W(".norm2.bias").double())
    Wf = _w(fold(W(".ff.net.0.proj.weight"), W(".norm3.weight")), rounded, dt)
    bf = f32v(W(".ff.net.0.proj.bias").double() + W(".ff.net.0.proj.weight").double() @ W(".norm3.bias").double())
    PF, P, PB = folded_proj_out(sd, j)
    PF, PB = (PF.float() if rounded else PF), f32v(PB)
    a, b = gn_coef(st_x, T, sd[p + ".norm.weight"], sd[p + ".norm.bias"], 1e-6, 6, rounded, dt)
    xin_d = xin.to(dt)
    g = xin_d * a[:, None] + b[:, None]
    x1 = (_lin(o.to(dt), _w(W(".attn1.to_out.0.weight"), rounded, dt)) + W(".attn1.to_out.0.bias").to(dt) + g)[idx]
    q = _lin(r(_ln(x1)), Wq) + bq
    S = k2.shape[1]
    o2 = _band(q, k2, v2, T, S, rounded)
    x2 = _lin(r(o2), _w(W(".attn2.to_out.0.weight"), rounded, dt)) + W(".attn2.to_out.0.bias").to(dt) + x1
    if n_uncond:
        c2 = f32v(c2_const(sd, j, null, torch.float64))
        xu = x1 + c2
        if _m("c2_on_conditional_half"):
            x2 = x2 + c2
        x2 = torch.cat([xu[:n_uncond], x2[n_uncond:]])
    hv = _lin(r(_ln(x2)), Wf) + bf
    val, gate = hv.chunk(2, dim=-1)
    if _m("geglu_swapped"):
        val, gate = gate, val
    y = _lin(r(val * _gelu(gate)), _w(PF, rounded, dt)) + _lin(r(x2), _w(P, rounded, dt)) + PB + xin_d[idx]
    y = _store(y, rounded, store)
    return y, partials(y)


# ---------------------------------------------------------------- the six-launch tail (st_chain_bf16 = 0; the last block of forward(): five, ending channel-major)
def out1_parts(sd, j, o, xin, st_x, rounded=True, dtype=torch.float64):
    """<1, 0, 0, 2, DUP, false>: attn1.to_out of the stored attention output + bias + GroupNorm(eps 1e-6)(x_in) from its producer's partials -> x1 (bf16)."""
    p, tb = ST[j], ST[j] + ".transformer_blocks.0"
    a, b = gn_coef(st_x, xin.shape[1], sd[p + ".norm.weight"], sd[p + ".norm.bias"], 1e-6, 6, rounded, dtype)
    w = _w(sd[tb + ".attn1.to_out.0.weight"], rounded, dtype)
    g = xin.to(dtype) * a[:, None] + b[:, None]
    return Parts(o.to(dtype), lambda op, absw: _lin(op, w, absw), lambda acc: acc + sd[tb + ".attn1.to_out.0.bias"].to(dtype) + g, False)


def out1_dup(sd, j, x1_stored, null, rounded=True, dtype=torch.float64, store=True):
    """DUP: the unconditional half's x2 = (stored x1) + c2, rounded again."""
    c2 = c2_const(sd, j, null, torch.float64)
    c2 = c2.float().to(dtype) if rounded else c2.to(dtype)
    return _store(x1_stored.to(dtype) + c2, rounded, store)


def q2_band(sd, j, x1, k2, v2, rounded=True, dtype=torch.float64, store=True):
    """<1, 4, 2, 0>: q = to_q(LayerNorm(norm2)(x1)), the banded softmax over the fp32 K / V rows of KV (k2, v2 (n, S, 192) key-major views of it) -> O2 (bf16).
    Two dependent products as far as roundings go (the operand, then the store): a multi-product launch."""
    tb = ST[j] + ".transformer_blocks.0"
    t = _ln(x1.to(dtype), sd[tb + ".norm2.weight"], sd[tb + ".norm2.bias"])
    q = _lin(_rb(t, rounded), _w(sd[tb + ".attn2.to_q.weight"], rounded, dtype))
    return _store(_band(q, k2, v2, x1.shape[1], k2.shape[1], rounded), rounded, store)


def out2_parts(sd, j, o2, x1, rounded=True, dtype=torch.float64):
    """<1, 0, 0, 1, false, false>: attn2.to_out + bias + x1 -> x2 (bf16)."""
    tb = ST[j] + ".transformer_blocks.0"
    w = _w(sd[tb + ".attn2.to_out.0.weight"], rounded, dtype)
    return Parts(o2.to(dtype), lambda op, absw: _lin(op, w, absw), lambda acc: acc + sd[tb + ".attn2.to_out.0.bias"].to(dtype) + x1.to(dtype), False)


def geglu_parts(sd, j, x2, rounded=True, dtype=torch.float64):
    """<1, 2, 2, 0>: ff.net.0.proj of LayerNorm(norm3)(x2), value * gelu(gate) -> F (B, T, 768) bf16."""
    tb = ST[j] + ".transformer_blocks.0"
    t = _ln(x2.to(dtype), sd[tb + ".norm3.weight"], sd[tb + ".norm3.bias"])
    w = _w(sd[tb + ".ff.net.0.proj.weight"], rounded, dtype)
    bias = sd[tb + ".ff.net.0.proj.bias"].to(dtype)

    def epi(acc):
        val, gate = (acc + bias).chunk(2, dim=-1)
        if _m("geglu_swapped"):
            val, gate = gate, val
        return val * _gelu(gate)

    def prod(op, absw):
        y = _lin(op, w, absw)
        if absw:   # first order: |d (value gelu(gate))| <= |gelu(gate)| |d value| + |value| max |gelu'| |d gate|, max |gelu'| = 1.13
            val, gate = (_lin(_rb(t, rounded), w) + bias).chunk(2, dim=-1)
            dv, dg = y.chunk(2, dim=-1)
            return _gelu(gate).abs() * dv + 1.13 * val.abs() * dg
        return y
    def floor_mask():
        # value * gelu(gate) with gelu(g) = g Phi(g), Phi(g) = (1 + erf(g / sqrt 2)) / 2: in fp32 the sum 1 + erf loses relative accuracy as Phi -> 0 — an error of
        # half an ulp of 1, 6e-8, becomes 6e-8 / (2 Phi) of the product, and a relative error r flips a bf16 rounding with probability ~ 2^8 r.  The floor (1 % unequal)
        # is asked of the elements where that is below a tenth of it: 2^8 * 6e-8 / (2 Phi) <= 1e-3, i.e. Phi(gate) >= 1 / 128 (gate >= -2.42); the element bound of all
        _, gate = (_lin(_rb(t, rounded), w) + bias).chunk(2, dim=-1)
        return 0.5 * (1.0 + torch.erf(gate.double() * 0.70710678118654752440)) >= 1.0 / 128
    return Parts(t, prod, epi, True, floor_mask=floor_mask)


def _ffproj(sd, j, rounded, dtype):
    PF, P, PB = folded_proj_out(sd, j)
    if rounded:
        PF, PB = PF.float(), PB.float()
    return _w(PF, rounded, dtype), _w(P, rounded, dtype), PB.to(dtype)


def proj_h_parts(sd, j, f, xin, rounded=True, dtype=torch.float64):
    """<1, 0, 0, 1, false, false, 4>: (P F2) h over the GEGLU product's 768 columns + x_in -> the bf16 partial sum."""
    PF, _, _ = _ffproj(sd, j, rounded, dtype)
    return Parts(f.to(dtype), lambda op, absw: _lin(op, PF, absw), lambda acc: acc + xin.to(dtype), False)


def proj_x_parts(sd, j, x2, part, rounded=True, dtype=torch.float64):
    """<1, 0, 0, 1, false, true>: P x2 + (P b2 + bp) + the stored partial sum -> the block's output."""
    _, P, PB = _ffproj(sd, j, rounded, dtype)
    part = torch.zeros_like(part) if _m("partial_sum_dropped") else part
    return Parts(x2.to(dtype), lambda op, absw: _lin(op, P, absw), lambda acc: acc + PB + part.to(dtype), False)


def proj_out_cm_parts(sd, j, f, x2, xin, rounded=True, dtype=torch.float64):
    """xgemm_kernel, the launch forward() ends the last block with: [P F2 | P] over [h ; x2] + bias + x_in -> fp32 (stored channel-major, with partials)."""
    PF, P, PB = _ffproj(sd, j, rounded, dtype)
    w = torch.cat([PF, P], 1)
    return Parts(torch.cat([f, x2], -1).to(dtype), lambda op, absw: _lin(op, w, absw), lambda acc: acc + PB + xin.to(dtype), False)


# ---------------------------------------------------------------- the out convolution (forward(): channel-major fp32 input, bf16 operands)
def out_conv_parts(sd, h, st_h, rounded=True, dtype=torch.float64):
    """out: silu(GroupNorm(eps 1e-5)) of the fp32 hidden state h (B, T, 192) from its partials -> Conv1d(192 -> 32, k 3) -> eps (B, T, 32) fp32."""
    a, b = gn_coef(st_h, h.shape[1], sd["model.out.0.weight"], sd["model.out.0.bias"], 1e-5, 6, rounded, dtype)
    t = _silu(h.to(dtype) * a[:, None] + b[:, None])
    w = _w(sd["model.out.2.weight"], rounded, dtype)
    return Parts(t, lambda op, absw: _conv3(op, w, absw), lambda acc: acc + sd["model.out.2.bias"].to(dtype), True)


# ---------------------------------------------------------------- K / V of the context
def kvt(kv, rounded=True):
    """KVT in bf16 mode: the key-major bf16 copy of KV (B, 1536, S) -> (B, S, 1536)."""
    return _rb(kv.transpose(1, 2), rounded)


# ---------------------------------------------------------------- the launches chained (tests/test_unet_bf16_ref_cpu.py)
def forward(sd, x, ts, ctx, rounded=False, dtype=torch.float64, n_clips=0, null=None, six=False, trace=None):
    """run_unet's token-major schedule on x (B, 32, T) channel-major -> eps (B, T, 32), or under n_clips > 0 (the guided step: x holds the clips' latents once, every
    tensor behind the shared first block has 2 n_clips samples, unconditional first) the last hidden state and its partials.  six: rgemm's six launches instead of
    the fused tail.  trace: receives (launch name, output) in launch order."""
    t = (lambda n, v: trace.append((n, v))) if trace is not None else (lambda n, v: None)
    kw = dict(rounded=rounded, dtype=dtype)
    Bc = n_clips
    T = x.shape[-1]
    rows = time_rows(sd, ts, dtype)
    kv = kv_all(sd, ctx, dtype)
    kv = _f32(kv, rounded, True)
    if Bc:
        kv = torch.cat([torch.zeros_like(kv), kv])
    kv_t = kvt(kv, rounded)
    e = lambda i, n: rows[i][:n] if not Bc else rows[i][:1].expand(n, -1)
    H0, sH0 = conv_in(sd, x, **kw)
    t("conv_in", H0)

    def res(i, x0, s0, dup=False):
        m, sm = with_stats(res_conv1_parts(sd, i, x0, s0, e(i, x0.shape[0]), **kw), rounded)
        t(f"res{i}.conv1", m)
        y, sy = with_stats(res_conv2_parts(sd, i, m, sm, x0, **kw), rounded)
        t(f"res{i}.conv2", y)
        return y, sy

    def res_cat(i, x0, s0, x1, s1):
        part = finish(cat_conv1a_parts(sd, i, x0, s0, **kw), rounded, True)
        t(f"res{i}.conv1a", part)
        m, sm = with_stats(cat_conv1b_parts(sd, i, x1, s1, part, e(i, x0.shape[0]), **kw), rounded)
        t(f"res{i}.conv1b", m)
        skip = finish(cat_skip_parts(sd, i, x0, x1, **kw), rounded, True)
        t(f"res{i}.skip", skip)
        y, sy = with_stats(cat_conv2_parts(sd, i, m, sm, skip, **kw), rounded)
        t(f"res{i}.conv2", y)
        return y, sy

    def st(j, xin, sx, shared=False, last=False):
        q, k, v = qkv_split(finish(qkv_parts(sd, j, xin, sx, scaled=True, **kw), rounded, False), rounded, True)
        t(f"st{j}.qkv", (q, k, v))
        o = battn(q, k, v, **kw)
        t(f"st{j}.attn", o)
        nsamp = 2 * Bc if Bc else xin.shape[0]
        lo = j * 2 * MC
        if not six and not (last and not Bc):   # (the loop's last kernel reads the token-major hidden state: its last block is fused too)
            y, sy = chain(sd, j, o, xin, sx, kv_t[:, :, lo:lo + MC], kv_t[:, :, lo + MC:lo + 2 * MC], nsamp=nsamp, in_mod=Bc if shared else 0, n_uncond=Bc, null=null, **kw)
            t(f"st{j}.chain", y)
            return y, sy
        idx = torch.arange(nsamp) % Bc if shared else torch.arange(nsamp)
        x1 = finish(out1_parts(sd, j, o, xin, sx, **kw), rounded, True)
        t(f"st{j}.out1", x1)
        x2u = out1_dup(sd, j, x1, null, **kw) if Bc else None
        x1c = x1[idx][Bc:]                       # the cross-attention's samples: the conditional half (all samples without guidance)
        kvk = kv.transpose(1, 2)[Bc:]
        o2 = q2_band(sd, j, x1c, kvk[:, :, lo:lo + MC], kvk[:, :, lo + MC:lo + 2 * MC], **kw)
        t(f"st{j}.band", o2)
        x2 = finish(out2_parts(sd, j, o2, x1c, **kw), rounded, True)
        if Bc:
            x2 = torch.cat([x2u[idx][:Bc], x2])
        t(f"st{j}.out2", x2)
        f = finish(geglu_parts(sd, j, x2, **kw), rounded, True)
        t(f"st{j}.geglu", f)
        if last and not Bc:
            y = finish(proj_out_cm_parts(sd, j, f, x2, xin[idx], **kw), rounded, True, bf16=False)
            t(f"st{j}.proj_out_cm", y)
            return y, partials(y)
        part = finish(proj_h_parts(sd, j, f, xin[idx], **kw), rounded, True)
        t(f"st{j}.proj_h", part)
        y, sy = with_stats(proj_x_parts(sd, j, x2, part, **kw), rounded)
        t(f"st{j}.proj_x", y)
        return y, sy

    if Bc:
        P, sP = res(0, H0, sH0)
        H1, sH1 = st(0, P, sP, shared=True)
        H0, sH0 = torch.cat([H0, H0]), torch.cat([sH0, sH0])
    else:
        H1, sH1 = st(0, *res(0, H0, sH0))
    Q, sQ = st(1, *res(1, H1, sH1))
    P, sP = res(2, Q, sQ)
    P, sP = st(2, *res_cat(3, P, sP, H1, sH1))
    P, sP = st(3, *res_cat(4, P, sP, H0, sH0), last=True)
    if Bc:
        return P, sP
    eps = finish(out_conv_parts(sd, P, sP, **kw), rounded, True, bf16=False)
    t("out", eps)
    return eps


def out_sched(sd, h, st_h, x, cf, gs, rounded=True, dtype=torch.float64, **kw):
    """out_sched_tm_kernel<CFG>: the out convolution of both halves (unconditional first) of the token-major bf16 hidden state, guidance, the update; h (2 B, T, 192),
    x (B, T, 32) -> (B, T, 32)."""
    B = x.shape[0]
    eps = finish(out_conv_parts(sd, h, st_h, rounded, dtype), rounded, False, bf16=False)
    return step_update(eps[B:], eps[:B], x, cf, gs, dtype, **kw)


# ---------------------------------------------------------------- the comparisons
def check_f32_allow(name, got, ref64, ref32, allow=0.0):
    """check_f32 with the flip allowance added to the absolute bound -> (e, bound) of max |ref|."""
    rng = float(ref64.abs().max())
    e32, bound = f32_bound(ref32, ref64)
    d = (got.double() - ref64).abs()
    lim = bound * rng + allow
    bad = int((d > lim).sum())
    e = float(d.max()) / rng
    amax = float(allow.max()) / rng if torch.is_tensor(allow) else 0.0
    print(f"{name}: e {e:.2e} (fp32 CPU evaluation {e32:.2e}, bound {bound:.2e}, largest allowance {amax:.2e}) of max |ref| {rng:.3g}; {bad} of {got.numel()} elements out")
    assert math.isfinite(e) and bad == 0, f"{name}: {bad} elements beyond {bound:.3e} of range + their allowance (largest difference {e:.3e})"
    return e, bound


def stored_limit(abs_bound, allow, ref_r):
    """An upper bound of every alternative of single_stats' element rule, as a distance between STORED values: what tests/test_unet_bf16_ref_cpu.py divides a mutant's
    distance by (so its factors are lower bounds)."""
    if not torch.is_tensor(allow):
        return abs_bound
    return abs_bound + allow + (allow > 0).to(allow.dtype) * bf16_step(ref_r)


def single_stats(got, p64: Parts, p32: Parts, pair=None):
    """A single-product launch with a bf16 store against its reference pair -> dict.  Element rule: a stored value is in when it is bit-equal to the rounded float64
    reference, or within one bf16 step of it, or within the fp32 bound 4 max(e32, 1e-6) of range + its flip allowance of it (audio_bf16_ref.check_bf16 with the
    allowance added to the absolute bound) — or, where the allowance is not zero, within fp32 bound + allowance + HALF a step of the float64 reference BEFORE its
    rounding.  The last alternative is a deviation from the letter of the rule, derived as follows: bound + allowance limits the PRE-store difference |y - pre64|,
    and the kernel's store moves y by at most half a step; measuring against the rounded reference instead charges the kernel for the reference's own rounding too,
    which matters only here, where the allowance (up to 1.3e-3 of range) is of the size of a step — the fp32 bound (4e-6) never is.
    Floor: the bit-equal share, over the elements p64.floor_mask selects (all, unless the launch names elements no fp32 evaluation can reproduce bit for bit)."""
    got = got.double()
    if pair is None:
        pre64, pre32 = finish(p64, True, False), finish(p32, True, False)
        allow, amb = flip_allowance(p64, p32)
        pair = dict(pre64=pre64, pre32=pre32, ref_r=round_bf16(pre64), allow=allow, amb=amb, rng=float(pre64.abs().max()), bound=f32_bound(pre32, pre64)[1],
                    mask=p64.floor_mask() if p64.floor_mask is not None else None)
    pre64, pre32, ref_r, allow, amb, rng, bound = (pair[k] for k in ("pre64", "pre32", "ref_r", "allow", "amb", "rng", "bound"))
    lim = bound * rng + allow
    d = (got - ref_r).abs()
    eq = d == 0
    ok = eq | (d <= torch.maximum(bf16_step(ref_r), bf16_step(got))) | (d <= lim)
    if torch.is_tensor(allow):
        ok = ok | ((allow > 0) & ((got - pre64).abs() <= lim + 0.5 * bf16_step(got)))
    mask = pair["mask"]
    share_all = float(eq.double().mean())
    return dict(share=share_all if mask is None else float(eq[mask].double().mean()), share_all=share_all, masked=1.0 if mask is None else float(mask.double().mean()),
                bad=int((~ok).sum()), out=~ok, dmax=float(d.max()), pair=pair, **{k: pair[k] for k in ("rng", "bound", "allow", "amb", "pre64", "pre32", "ref_r")})


def check_bf16_allow(name, got, p64: Parts, p32: Parts):
    """A single-product launch with a bf16 store on its own inputs: >= 99 % bit-equal, every element inside single_stats' rule.
    -> (bit-equal share, largest difference / range, largest allowance / range)"""
    st = single_stats(got, p64, p32)
    own = single_stats(round_bf16(st["pre32"].double()), p64, p32, st["pair"])
    # the reference pair itself: 99.9 % as in audio_bf16_ref.check_bf16 where the operand is stored data; where the kernel transforms it, flips of ambiguous operands
    # cost a correct evaluation bit-equal elements too (on the CPU: 99.45 % for the concatenated convolutions' partial sums ... 99.99 %): the kernel's own floor
    own_floor = 0.99 if p64.transforms else 0.999
    assert own["share"] >= own_floor and own["bad"] == 0, (f"{name}: the fp32 CPU evaluation of these inputs is {100 * own['share']:.3f} % bit-equal with {own['bad']} elements out: "
                                                          "the inputs are at fault, not the kernel")
    rng, allow = st["rng"], st["allow"]
    amax = float(allow.max()) / rng if torch.is_tensor(allow) else 0.0
    part = "" if st["masked"] == 1.0 else f" over the {100 * st['masked']:.2f} % of the elements the floor is asked of (all elements: {100 * st['share_all']:.3f} %, fp32 CPU evaluation {100 * own['share_all']:.3f} %)"
    print(f"{name}: {100 * st['share']:.3f} % bit-equal (fp32 CPU evaluation {100 * own['share']:.3f} %){part}, {st['bad']} elements out, max |diff| {st['dmax'] / rng:.2e} of max |ref| {rng:.3g}; "
          f"{100 * st['amb']:.3f} % of the operands ambiguous, largest allowance {amax:.2e} of range; {got.numel()} elements")
    for ix in st["out"].nonzero()[:12].tolist():   # where and by how much
        ix = tuple(ix)
        al = float(allow[ix]) if torch.is_tensor(allow) else 0.0
        print(f"{name}: out at {ix}: stored {float(got[ix]):.8g}, reference {float(st['pre64'][ix]):.8g} -> {float(st['ref_r'][ix]):.8g}, fp32 CPU evaluation {float(st['pre32'][ix]):.8g}, "
              f"fp32 bound {st['bound'] * rng:.3g}, allowance {al:.3g}")
    assert st["share"] >= 0.99, f"{name}: {100 * st['share']:.3f} % bit-equal, at least 99 % wanted"
    assert st["bad"] == 0, f"{name}: {st['bad']} elements outside one bf16 step and outside the fp32 bound + their flip allowance"
    return st["share"], st["dmax"] / rng, amax


def check_multi(name, got, ref_r, cap):
    """A multi-product launch: >= 97 % bit-equal over the whole launch, every element within max(one bf16 step, cap x max |ref|)."""
    assert 0 < cap <= 1e-2, f"{name}: a cap of {cap:.2e} of range — the inputs are at fault"
    rng = float(ref_r.abs().max())
    share, bad, dmax = bf16_stats(got, ref_r, cap * rng)
    print(f"{name}: {100 * share:.3f} % bit-equal, {bad} elements beyond one bf16 step and the cap {cap:.2e}, max |diff| {dmax / rng:.2e} of max |ref| {rng:.3g}, {got.numel()} elements")
    assert share >= 0.97, f"{name}: {100 * share:.3f} % bit-equal, at least 97 % wanted"
    assert bad == 0, f"{name}: {bad} elements beyond max(one bf16 step, {cap:.2e} of range)"
    return share, dmax / rng
