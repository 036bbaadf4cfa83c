"""tests/unet_f32_ref.py on the CPU: tied to the oracle, and shown to have teeth.

* Tie: the launches chained in float64 against the oracle's op sequence in float64 (oracle/unet.py with its `.float()` casts redirected), for the forward pass and
  for one guided DDIM step, at shape S (2 samples x 70 frames).  Both sides are float64; they differ by the folded proj_out and by summation order (~1e-13), and the
  bound of 1e-9 of range is three orders below any fp32 bound the GPU test applies.
* Teeth: every mutant of unet_f32_ref.MUTANTS, applied to the reference of the launch it belongs to and compared with the unmutated float64 reference of the same
  stored inputs, must exceed that launch's bound 4 max(e32, 1e-6) (tests/test_gpu_unet_f32_kernels.py's rule) at least ten times.  The ratios are printed.
  The six mutants of the seams between the five launches of the unfused tail (and band_shifted / geglu_swapped again) are applied at the launch's own output, on
  CPU-made stored inputs at the shapes tests/test_gpu_unet_f32_strict_kernels.py runs: the guided step's second block at 1 clip x 70 (x_off = kv_off = 1) and the
  wide-band shapes W; to_out1's two forms (merged partials, coefficient rows) are shown to agree.
"""
from unittest import mock

import numpy as np
import pytest
import torch

import unet_f32_ref as R
from audio_bf16_ref import f32_bound, rel_max
from oracle import pipeline as op
from oracle import scheduler as osch
from oracle import unet as ou
from said_amd.util import synth

torch.set_grad_enabled(False)
F64, F32 = torch.float64, torch.float32
B, T = 2, 70           # shape S
GS = 2.0


@pytest.fixture(scope="module")
def sd_null():
    _, sd_u, null = op.split_state_dict(synth.said_state_dict(num_w2v_layers=1))
    return sd_u, null


@pytest.fixture(scope="module")
def inputs():
    x = synth.synth_latents(301, (B, T, 32))
    c = synth.synth_latents(302, (B, T, 768))
    ts = (torch.arange(B) * 137 + 500) % 1000
    return x, ts, c


def _oracle64(sd_u, x, ts, c):
    with mock.patch.object(torch.Tensor, "float", torch.Tensor.double):
        return ou.unet1d_forward({k: v.double() for k, v in sd_u.items()}, x.double(), ts, c.double())


def _coef(k=24, eta=0.0, n=1):
    from said_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler()
    sch.set_timesteps(50)
    ts = sch.timesteps.numpy()
    return ts, sch.coef_table(ts[k:k + n], eta)


@pytest.fixture(scope="module")
def trace(sd_null, inputs):
    """The forward pass's launches in float64, in launch order."""
    sd_u, _ = sd_null
    x, ts, c = inputs
    tr = []
    out = R.forward(sd_u, x.transpose(1, 2), ts, c, F64, trace=tr)
    return out, dict(tr), [n for n, _ in tr]


def test_forward_chained_in_float64_is_the_oracle(sd_null, inputs, trace):
    sd_u, _ = sd_null
    x, ts, c = inputs
    out, _, names = trace
    assert len(names) == 24, "conv_in, 5 x 2 ResBlock convolutions, 4 x (q/k/v, attention, chain), out"
    ref = _oracle64(sd_u, x, ts, c).transpose(1, 2)
    e = rel_max(out, ref)
    print(f"forward, launches chained in float64 vs the oracle in float64: {e:.2e} of max |ref|")
    assert e <= 1e-9


def test_guided_step_chained_in_float64_is_the_oracle(sd_null, inputs):
    sd_u, null = sd_null
    lat, c = inputs[0][:1], inputs[2][:1]
    ts, coef = _coef()
    tt = int(ts[24])
    with mock.patch.object(torch.Tensor, "float", torch.Tensor.double):
        pred = ou.unet1d_forward({k: v.double() for k, v in sd_u.items()}, torch.cat([lat] * 2).double(), torch.tensor([tt, tt]),
                                 torch.cat([null.repeat(1, T, 1), c]).double())
    e_u, e_c = pred.chunk(2)
    o = osch.OracleDDIM()
    o.set_timesteps(50)
    want = o.step(e_c + GS * (e_c - e_u), tt, lat.double())
    P = R.forward(sd_u, lat.transpose(1, 2), torch.tensor([tt]), c, F64, n_clips=1, null=null)
    got = R.out_sched(sd_u, P, lat.transpose(1, 2), coef[0], GS, F64).transpose(1, 2)
    e = rel_max(got, want)
    print(f"guided step, launches chained in float64 vs the oracle in float64: {e:.2e} of max |ref|")
    assert e <= 1e-9


def _stored(t):
    return tuple(_stored(u) for u in t) if isinstance(t, tuple) else t.float()


def _mutant_cases(sd_u, null, inputs, tr):
    """{mutant: (launch name, fn(dtype) -> the launch's stored output)} on the stored (fp32) inputs of shape S."""
    x, ts, c = inputs
    H0, M, P = _stored(tr["conv_in"]), _stored(tr["res0.conv1"]), _stored(tr["res0.conv2"])
    q, k, v = _stored(tr["st0.qkv"])
    O = _stored(tr["st0.attn"])
    rows = R.time_rows(sd_u, ts, F64).float()
    kv = R.kv_all(sd_u, c, F64).float()
    k2, v2 = kv[:, :R.MC], kv[:, R.MC:2 * R.MC]
    coef0 = R.gn_coef(sd_u, 0, P, F64).float()
    conv1 = ("res0.conv1", lambda dt: R.res_conv1(sd_u, 0, [H0], rows[0], dt))
    conv2 = ("res0.conv2", lambda dt: R.res_conv2(sd_u, 0, M, [H0], dt)[0])
    chain = ("st0.chain", lambda dt: R.chain(sd_u, 0, O, P, coef0, k2, v2, dt))
    # the guided step's second block: sample 0 unconditional, sample 1 conditional; the unconditional slot of KV holds what a kernel that wrongly ran the
    # cross-attention would find there — here the conditional sample's rows
    Pm = _stored(tr["res1.conv2"])
    O1 = _stored(tr["st1.attn"])
    coef1 = R.gn_coef(sd_u, 1, Pm, F64).float()
    kb, vb = kv[:, 2 * R.MC:3 * R.MC], kv[:, 3 * R.MC:4 * R.MC]
    guided = ("st1.chain, guided", lambda dt: R.chain(sd_u, 1, O1, Pm, coef1, kb[1:].expand(2, -1, -1), vb[1:].expand(2, -1, -1), dt, n_uncond=1, null=null))
    # the step update with eta noise and a mask that crosses the token-tile boundary at 64
    _, cf = _coef(eta=1.0, n=2)
    eps = _stored(tr["out"])
    xl = x.transpose(1, 2)[:1]
    nz, init, en = (synth.synth_latents(s, (1, T, 32)).transpose(1, 2) for s in (311, 312, 313))
    mask = torch.zeros(1, 32, T)
    mask[:, :, 60:68] = 1
    mask[:, :5] = 1
    upd = ("out_sched update", lambda dt: R.step_update(eps[1:], eps[:1], xl, cf[0], GS, dt, noise=nz, init=init.abs().clamp(0, 1), enoise=en, mask=mask))
    return {
        "fp16_operands": conv1, "k_block_dropped": conv1, "tap_shifted": conv1, "pad_tap_nonzero": conv1, "gn_neighbour_group": conv1, "gn_over_tp": conv1,
        "emb_row_of_other_sample": conv1, "residual_of_neighbour_sample": conv2,
        "y2_not_written": ("res0.conv2, duplicate store", lambda dt: R.res_conv2(sd_u, 0, M, [H0], dt)[1]),
        "last_key_tile_missing": ("st0.attn", lambda dt: R.self_attention(q, k, v, dt)),
        "band_shifted": chain, "geglu_swapped": chain, "uncond_runs_cross_attention": guided, "mask_blend_order": upd,
    }   # (the mutants of the five-launch tail's seams: _tail_mutant_cases)


def _tail_inputs(sd_u, T, S, seed):
    """CPU-made stored inputs of block 0's five-launch tail at 2 x (T, S): (o, xin, k2, v2) in fp32, from the launches chained in float64."""
    x = synth.synth_latents(seed, (2, T, 32))
    c = synth.synth_latents(seed + 1, (2, S, 768))
    tr = []
    R.forward(sd_u, x.transpose(1, 2), (torch.arange(2) * 137 + 500) % 1000, c, F64, trace=tr)
    tr = dict(tr)
    kv = R.kv_all(sd_u, c, F64).float()
    return _stored(tr["st0.attn"]), _stored(tr["res0.conv2"]), kv[:, :R.MC], kv[:, R.MC:2 * R.MC]


# the band shapes of tests/test_gpu_unet_f32_strict_kernels.py: W (windows wider than 8 keys), N (narrow windows the fused tail's window tile cannot hold)
W_SHAPES = ((10, 100), (37, 400))


def _tail_mutant_cases(sd_u, null, inputs, tr):
    """[(mutant, launch name, fn(dtype))] for the seams between the five launches of the unfused tail, each at the launch's own output: shape S, the guided step's
    second block at 1 clip x 70 (sample 0 unconditional, sample 1 conditional: x_off = kv_off = 1), and the wide-band shapes W."""
    _, ts, c = inputs
    Pm, O1 = _stored(tr["res1.conv2"]), _stored(tr["st1.attn"])
    st = R.partials_of(Pm)
    kv = R.kv_all(sd_u, c, F64).float()
    kb, vb = kv[:, 2 * R.MC:3 * R.MC], kv[:, 3 * R.MC:4 * R.MC]
    x1, y2 = (t.float() for t in R.to_out1(sd_u, 1, O1, Pm, st, F64, null=null))
    o2 = R.q_band(sd_u, 1, x1[1:], kb[1:], vb[1:], T, T, F64).float()
    O = torch.cat([O1[:1], o2])   # (the band overwrites the attention output's slots in place)
    x2 = R.to_out2(sd_u, 1, O[1:], x1, F64, x_off=1, kv_off=1, x2=y2).float()
    h = R.geglu(sd_u, 1, x2, F64).float()
    out = [
        ("y2_without_c2", "st1 to_out1, y2 (guided)", lambda dt: R.to_out1(sd_u, 1, O1, Pm, st, dt, null=null)[1]),
        ("x1_of_wrong_sample_under_x_off", "st1 to_out2 (guided)", lambda dt: R.to_out2(sd_u, 1, O[1:], x1, dt, x_off=1, kv_off=1, x2=y2)),
        ("to_out2_writes_uncond_slot", "st1 to_out2 (guided)", lambda dt: R.to_out2(sd_u, 1, O[1:], x1, dt, x_off=1, kv_off=1, x2=y2)),
        ("geglu_swapped", "st1 geglu", lambda dt: R.geglu(sd_u, 1, x2, dt)),
        ("ffproj_second_segment_dropped", "st1 ffproj", lambda dt: R.ffproj(sd_u, 1, h, x2, Pm, dt)),
        ("band_shifted", "st1 q_band", lambda dt: R.q_band(sd_u, 1, x1, kb, vb, T, T, dt)),
    ]
    for Tw, Sw in W_SHAPES:
        o, xin, k2, v2 = _tail_inputs(sd_u, Tw, Sw, 330 + Tw)
        xw = R.to_out1(sd_u, 0, o, xin, R.partials_of(xin), F64)[0].float()
        qw = R.q2(sd_u, 0, xw, F64).float()
        out.append(("band_truncated_to_8_keys", f"st0 q_band, W {Tw} x {Sw}", lambda dt, a=(xw, k2, v2, Tw, Sw): R.q_band(sd_u, 0, *a, dt)))
        out.append(("wide_band_off_by_one", f"st0 band_wide, W {Tw} x {Sw}", lambda dt, a=(qw, k2, v2, Tw, Sw): R.band(*a, dt)))
    return out


def test_partials_made_on_the_cpu_give_the_coefficient_rows(sd_null, trace):
    """to_out1's two forms agree: the (a, b) rows from merged partials (the RES_GN epilogue) are gn_coef's rows from the values (what fgemm_kernel reads)."""
    sd_u, _ = sd_null
    P = _stored(trace[1]["res0.conv2"])
    e = rel_max(R.coef_from_partials(sd_u, 0, R.partials_of(P), T, F64), R.gn_coef(sd_u, 0, P, F64))
    print(f"GroupNorm rows from CPU-made partials vs from the values: {e:.2e}")
    assert e <= 1e-6   # (the partials are stored in fp32)


def test_every_mutant_exceeds_its_launch_bound_tenfold(sd_null, inputs, trace):
    sd_u, null = sd_null
    cases = [(n, *v) for n, v in _mutant_cases(sd_u, null, inputs, trace[1]).items()] + _tail_mutant_cases(sd_u, null, inputs, trace[1])
    assert {n for n, _, _ in cases} == set(R.MUTANTS)
    worst = np.inf
    for name, launch, fn in cases:
        assert R.MUTANT is None
        ref64, ref32 = fn(F64), fn(F32)
        e32, bound = f32_bound(ref32, ref64)
        try:
            R.MUTANT = name
            mut = fn(F64)
        finally:
            R.MUTANT = None
        e = rel_max(mut, ref64)
        print(f"mutant {name:32s} on {launch:30s}: {e:.2e} of max |ref|, bound {bound:.2e} (fp32 CPU evaluation {e32:.2e}): ratio {e / bound:.3g}")
        worst = min(worst, e / bound)
        assert e >= 10 * bound, f"{name}: only {e / bound:.2f} x the bound of {launch}"
    print(f"smallest ratio {worst:.3g}")


def test_split_pair_check_sees_a_low_plane_that_is_not_the_remainder_of_the_stored_high_plane():
    """decode_split / split_is_consistent on pairs made here: consistent ones pass; a low plane that is the remainder of the OTHER fp16 neighbour does not."""
    x = synth.synth_latents(321, (4096,)) * 3
    h = x.half()
    lo = ((x - h.float()) * 2048.0).half()
    packed = (h.view(torch.int16).to(torch.int32) & 0xFFFF | (lo.view(torch.int16).to(torch.int32) << 16)).view(torch.float32)
    val, h2, l2 = R.decode_split(packed)
    assert torch.equal(h2.view(torch.int16), h.view(torch.int16)) and torch.equal(l2.view(torch.int16), lo.view(torch.int16))
    assert float((val - x.double()).abs().max()) <= 2.0 ** -21 * float(x.abs().max())
    assert R.split_is_consistent(h2, l2)[0] == 0
    other = (h.view(torch.int16) + 1).view(torch.float16)   # the fp16 neighbour one step up in magnitude: the low plane is ITS remainder, the stored high plane is h
    assert R.split_is_consistent(h, ((x - other.float()) * 2048.0).half())[0] > 4000
