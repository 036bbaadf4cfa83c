"""The fp32 (split-fp16) denoise step kernel by kernel (run on the MI355X with `-m gpu`).

fp32 mode with its default options — nothing switched off — is stopped behind every launch of the channel-major schedule (said_debug_stop_after), the launch's
inputs and outputs are read back AS STORED (the workspace list: Engine.ws_buffers / ws_snapshot), and the output is compared with tests/unet_f32_ref.py's evaluation
of those inputs in float64 (tests/test_unet_f32_ref_cpu.py ties that restatement to the oracle and shows that twenty ways of being wrong exceed the bound 70 x
at least).  The rule is the project's (audio_bf16_ref.check_f32):
    max |got - ref64| / max |ref64| <= 4 max(e32, 1e-6),   e32 the same figure of the torch fp32 CPU evaluation of the identical inputs,
over all samples, channels and tokens [0, T).  Per launch: conv_in_kernel / the generic convolution (H0); ugemm_kernel with ugemm_body or kconv_body (the ResBlock
convolutions, one and two K segments, residual or 1x1 skip segments, the duplicate store); the q/k/v GEMM (q; k and v decoded from their packed split pairs, whose
low plane must be a rounded remainder of the stored high plane; the gn_coef rows); attn_kernel<PM = 3> / attn2q_kernel; stchain_kernel's whole tail; the out
convolution; out_sched_kernel<CFG> (guidance, DDIM update, eta noise, mask blend: masked elements bit-exact).  Every launch that stores GroupNorm partials: the
normalised tensor the merged partials imply against the float64 GroupNorm of the stored output.  Apart from the step: KV against the float64 projection of the
context, KVT as its exact transpose.  A buffer read again at a later stop must be bit-equal to what the earlier stop saw.  Pad tokens [T, Tp) are never compared:
instead every shape's forward pass and one guided step (with eta noise and the mask blend) run with the workspace filled with 0x00, 0xFF and 0x7F first and must be
finite and bit-identical — F, whose operand buffers have rows nobody writes, included.

Shapes (each the smallest that reaches what is named; asserted here from the stage log — kind, epi, NB, KS per launch — and the counters; what the log does not
carry — split-fp16 or fp32 matrix instructions, kconv_body or the block loop, token tiles per workgroup, the chain's slices — is held on the CPU by
tests/test_ugemm_plan_cpu.py::test_shapes_of_the_fp32_kernel_test_reach_what_they_are_named_for, from ugemm_plan.h and stchain.h):
  S      forward, 2 x 70 (6 token tiles, the last of a sample 6 tokens): every 192-wide GEMM and q/k/v at NB = 1, the concatenated convolutions on kconv_body,
         attention with 8 key slices, the three-slice chain; 24 launches.  Also on synth.trained_like_state_dict.
  G      one guided loop step, 1 clip x 70: conv_in_kernel with two copies, the duplicate stores, the shared first block, c2, out_sched_kernel<CFG>; 24 graph nodes.
  G-eta  as G with eta = 1 noise and a mask that crosses the token-tile boundary at 64.
  M1     forward, 3 x 290 (30 tiles): q/k/v NB = 3, attention with 4 key slices.
  M2     forward, 5 x 290 (50 tiles): 192-wide NB = 2, q/k/v NB = 2, the concatenated convolutions on the fp32-MFMA NB = 2 shapes.
  L      forward, 7 x 417 (98 tiles, a sample's last tile 1 token): 192-wide NB = 3, the kconv NB = 1 switch, q/k/v on the multi-tile fp32 kernel storing packed
         k / v, attn2q_kernel with a phantom query tile, the two-slice chain (98 > CHAIN3_MAX_TILES = 85).
  F      forward, 3 x 70 with said_debug_option "unet_tgemm_min_tokens" = 0: the large-batch fp32 route at toy size — prep_kernel in pack mode on its own (the
         operand buffers uPA / uPL, the raw copy uPB for the 1x1 skip, the padding rows, the gn_coef rows) and fgemm_kernel<SP, PK> for the ResBlock convolutions
         and q/k/v from those stored operands, then attention and the chain; 40 launches.
Measured (MI355X; e of max |ref| beside the fp32 CPU evaluation's own e32, over all shapes; the bound is its floor 4e-6 everywhere, e32 <= 9.4e-7): conv_in
1.6e-7 (e32 2.0e-7); ResBlock conv 1 / conv 2 on ugemm_kernel 2.9e-7 / 2.5e-7 (6.1e-7 / 6.0e-7), on fgemm_kernel 3.3e-7 / 2.1e-7; q / k / v 2.5e-7 / 3.1e-7 / 2.7e-7
(7.5e-7 / 9.1e-7 / 6.4e-7), on fgemm_kernel 1.5e-7 / 1.8e-7 / 1.7e-7; gn_coef a / b 1.9e-7 / 2.9e-7; self-attention 3.2e-7 on the plain fill, 9.7e-7 on the
trained-like one (e32 9.4e-7); the chain 3.8e-7 (6.9e-7); the out convolution 2.0e-7; out_sched_kernel<CFG> 2.9e-7, with eta noise and the mask 3.0e-7 (5.8e-7);
prep_kernel's operands 2.4e-7 ... 2.9e-7; GroupNorm from the stored partials 9e-9 ... 3.8e-8 (the fp32 CPU GroupNorm: 7e-8 ... 1.5e-7); KV 4.3e-7; no packed pair
inconsistent (one element in ~2000 has a remainder of exactly half a step); KVT, y2, conv_in's second copy, masked elements exact; the fills (S, M1, M2, L, F; forward pass and guided step with eta noise and mask) finite
and bit-identical.
Largest e per shape: S 3.1e-7, M1 2.7e-7, M2 3.2e-7, L 4.3e-7, S trained-like 9.7e-7, G 2.9e-7, G-eta 3.0e-7, F 3.3e-7.  pytest --durations: L 1.1 s,
S trained-like 0.8 s, S 0.5 s, M2 0.3 s, M1 0.2 s, F 0.14 s, G / G-eta 0.1 s, each of the five fill tests <= 0.03 s (the module's model 2 s once).
The schedules, the stop-and-read loop (Stops) and the per-launch checks live in tests/unet_f32_stops.py, shared with tests/test_gpu_unet_f32_strict_kernels.py (strict
fp32, the five-launch tail, attn_kernel<QW 4>, the one-slice chain).
"""
import numpy as np
import pytest
import torch

import unet_f32_ref as R
from audio_bf16_ref import check_exact, check_f32
from oracle import pipeline as op
from said_amd.util import synth
# the schedules, the stop-and-read loop and the per-launch checks: shared with tests/test_gpu_unet_f32_strict_kernels.py
from unet_f32_stops import (F32, F64, GS, MC, Stops, _check_launch, _check_launch_f, _kv_checks, _model, _partials, _poison, _schedule, _schedule_f,  # noqa: F401
                            _summary)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def plain(dev):
    sd = synth.said_state_dict(num_w2v_layers=1)
    _, sd_u, null = op.split_state_dict(sd)
    return _model(dev, sd), sd_u, null


# ---------------------------------------------------------------- the schedule's stage log
def _expected_stages(guided, nb_in, nb, nb_cat, nb_qkv, ks):
    """(kind, epi, NB, KS) per launch as unet_sched.cpp logs them: 0 the generic GEMM, 2 ugemm_kernel, 1 attention (NB = head_dim / 32; KS 34 = attn2q_kernel),
    10 stchain_kernel, 11 conv_in_kernel, 12 the out convolution.  profile_unet never logs out_sched_kernel: its stage list ends with the out convolution."""
    out = []
    for la in _schedule(False):
        k = la[0]
        if k == "conv_in":
            out.append((11, 0, 1, 4) if guided else (0, 0, nb_in, 8))
        elif k in ("conv1", "conv2"):
            out.append((2, 0, nb_cat if la[3] else nb, 8))
        elif k == "qkv":
            out.append((2, 1, nb_qkv, 8))
        elif k == "attn":
            out.append((1, -1, 1, ks))
        elif k == "chain":
            out.append((10, 0, 6, 8))
        else:
            out.append((12, 0, 1, 8))
    return out


# ---------------------------------------------------------------- forward shapes
def _forward_case(model, sd, dev, tag, B, T, seed, stages):
    x = synth.synth_latents(seed, (B, T, 32))
    ctx = synth.synth_latents(seed + 1, (B, T, 768))
    ts = (torch.arange(B) * 137 + 500) % 1000
    eng = model._get_engine(max(B, 2), max(T, 64))
    xd, cd = x.to(dev), ctx.to(dev)
    out = {}

    def run():
        out["y"] = eng.unet_forward(xd, ts, cd)
        torch.cuda.synchronize()

    s = Stops(eng, B, T, T, run)
    sched = _schedule(False)
    rec = []
    try:
        n0 = eng.debug_get("n_stchain")
        for k, la in enumerate(sched, 1):
            c = s.stop(k, la)
            if k == 1:
                check_exact(f"{tag} x (channel-major latents)", c["x"], x.transpose(1, 2))
                _kv_checks(tag, sd, s, ctx, 0, rec)
            _check_launch(tag, sd, None, la, c, B, 0, rec)
        # stop k issues the first k launches again: 3 + 2 x 5 + ... fused tails in all
        assert eng.debug_get("n_stchain") - n0 == sum(1 for k in range(1, len(sched) + 1) for la in sched[:k] if la[0] == "chain")
        eng.debug_stop_after(-1)
        run()
        check_exact(f"{tag} the unstopped call's result against the last stop's eps", out["y"].cpu().transpose(1, 2), s.cur["eps"])
        for name in ("P", "stP", "KV"):
            assert torch.equal(s.read(name).view(torch.int32), s.cur[name].view(torch.int32)), name
        log = [(d["kind"], d["epi"], d["NB"], d["KS"]) for d in eng.profile_unet(B, T, reps=1)]
    finally:
        eng.debug_stop_after(-1)
    print(f"{tag}: stage log {log}")
    assert stages is None or log == stages, f"{tag}: the launches are not the ones this shape is here for"
    _summary(tag, rec)


#        tag   B  T    conv_in NB, 192-wide NB, concatenated NB, q/k/v NB, attention KS
SHAPES = {"S": (2, 70, 1, 1, 1, 1, 8), "M1": (3, 290, 1, 1, 1, 3, 4), "M2": (5, 290, 2, 2, 2, 2, 4), "L": (7, 417, 2, 3, 1, 3, 34)}


@pytest.mark.parametrize("tag", list(SHAPES))
def test_forward_launches_on_their_own_inputs(plain, dev, tag):
    """Every launch of the forward pass at shapes S, M1, M2 and L (all launches, all samples)."""
    model, sd, _ = plain
    B, T, *nbs = SHAPES[tag]
    _forward_case(model, sd, dev, tag, B, T, 400 + 10 * len(tag) + B, _expected_stages(False, *nbs))


def test_forward_launches_on_trained_like_weights(dev):
    """Shape S on synth.trained_like_state_dict (heavy tails, outlier channels, norm gains up to 10: the fill that found DESIGN 9.2's bug)."""
    full = synth.trained_like_state_dict(num_w2v_layers=1)
    _, sd_u, _ = op.split_state_dict(full)
    model = _model(dev, full)
    B, T, *nbs = SHAPES["S"]
    _forward_case(model, sd_u, dev, "S trained-like", B, T, 431, _expected_stages(False, *nbs))


@pytest.mark.parametrize("tag", list(SHAPES) + ["F"])
def test_workspace_fill_does_not_reach_a_result(plain, dev, tag):
    """The stand-in for comparing pad tokens: every shape's forward pass and one guided step from a workspace of zeros, NaNs and 3.4e38.  F: the large-batch route,
    whose token-major operands have rup(T + 2, 32) rows per sample of which prep_kernel writes T + 2 and fgemm_kernel's 64-row tiles read more."""
    model, _, _ = plain
    B, T = (3, 70) if tag == "F" else SHAPES[tag][:2]
    opts = {"unet_tgemm_min_tokens": 0} if tag == "F" else None
    eng = _poison(model, dev, B, T, 450 + B + (10 if tag == "F" else 0), opts)
    if tag == "F":   # the option reached the schedule: with it the forward pass has prep_kernel / fgemm_kernel launches (kinds 5 / 4), without it none
        try:
            eng.debug_option("unet_tgemm_min_tokens", 0)
            kinds = [d["kind"] for d in eng.profile_unet(B, T, reps=1)]
        finally:
            eng.debug_option("unet_tgemm_min_tokens", -1)
        assert kinds.count(5) == 16 and kinds.count(4) == 14, kinds


# ---------------------------------------------------------------- the guided loop step
@pytest.mark.parametrize("case", ["G", "G-eta"])
def test_guided_step_launches_on_their_own_inputs(plain, dev, case):
    """One guided loop step of one clip x 70 frames (Engine.denoise_loop, one timestep, guidance 2): every launch of the headline's own structure, then
    out_sched_kernel<CFG> against the float64 out convolution + guidance + update of its stored inputs (G-eta: with eta = 1 noise and the mask blend; the blend's
    coefficient pair is the next timestep's, from a two-step table)."""
    model, sd, null = plain
    Bc, T, k = 1, 70, 24
    Be = 2 * Bc
    eta = 1.0 if case == "G-eta" else 0.0
    lat = synth.synth_latents(461, (Bc, T, 32))
    ctx = synth.synth_latents(462, (Bc, T, 768))
    sch = model.noise_scheduler
    sch.set_timesteps(50)
    ts = sch.timesteps.numpy()
    coef = sch.coef_table(ts[k:k + 2], eta)[:1]
    kw, kwd = {}, {}
    if eta > 0:
        mask = torch.zeros(Bc, T, 32)
        mask[:, 60:68] = 1
        mask[:, :, :5] = 1
        kw = dict(noise=synth.synth_latents(463, (Bc, T, 32)), init=synth.synth_latents(464, (Bc, T, 32)).abs().clamp(0, 1), enoise=synth.synth_latents(465, (Bc, T, 32)),
                  mask=mask)
        kwd = dict(step_noise=kw["noise"][None].to(dev), init_latents=kw["init"].to(dev), edit_noise=kw["enoise"].to(dev), mask=mask.to(dev))
    eng = model._get_engine(Be, max(T, 64))
    latd, ctxd = lat.to(dev), ctx.to(dev)
    out = {}

    def run():
        out["y"] = eng.denoise_loop(latents=latd, context=ctxd, timesteps=ts[k:k + 1], coef=coef, prediction_type="epsilon", guidance_scale=GS, guidance_rescale=0.0,
                                    latent_scale=1.0, **kwd)[1]
        torch.cuda.synchronize()

    s = Stops(eng, Be, T, T, run)
    sched = _schedule(True)
    rec = []
    try:
        n0 = eng.debug_get("n_out_sched")
        for n, la in enumerate(sched[:-1], 1):
            c = s.stop(n, la)
            if n == 1:
                check_exact(f"{case} x (channel-major latents)", c["x"][:Bc], lat.transpose(1, 2))
                _kv_checks(case, sd, s, ctx, Bc, rec)
            _check_launch(case, sd, null, la, c, Be, Bc, rec)
        assert eng.debug_get("n_out_sched") == n0, "no stop so far reached the step's last launch"
        eng.debug_stop_after(-1)
        run()
        assert eng.debug_get("n_out_sched") > n0 and eng.graph_num_nodes() == 24
        for name in ("P", "stP"):
            assert torch.equal(s.read(name).view(torch.int32), s.cur[name].view(torch.int32)), name
        log = [(d["kind"], d["epi"], d["NB"], d["KS"]) for d in eng.profile_unet(Be, T, reps=1, cfg_clips=Bc)]
    finally:
        eng.debug_stop_after(-1)
    assert log == _expected_stages(True, 1, 1, 1, 1, 8), log
    got = out["y"].cpu()
    P = s.cur["P"]
    cm = {n: v.transpose(1, 2) for n, v in kw.items()}
    fn = lambda dt: R.out_sched(sd, P, lat.transpose(1, 2), coef[0], GS, dt, **cm).transpose(1, 2)
    rec.append(("out_sched",) + check_f32(f"{case} out_sched_kernel<CFG>", got, fn(F64), fn(F32)))
    rec.append(("stP",) + _partials(f"{case} st3 chain (out_sched's input)", P, s.cur["stP"]))
    if eta > 0:   # masked elements do not depend on the model output: add_noise(init, edit_noise, t_next) in fp32, bit for bit
        m = kw["mask"].bool()
        cf = torch.from_numpy(np.asarray(coef[0], dtype=np.float32))
        assert float(cf[5]) != 1.0 and float(cf[6]) != 0.0, "the blend's pair is the next timestep's"
        noisy = cf[5] * kw["init"] + cf[6] * kw["enoise"]
        assert torch.equal(got[m], noisy[m]), "a masked element is not the noised initial latent"
        assert bool(m[:, 60:68].all()) and not bool(m[:, 68:, 5:].any()), "the mask crosses the token-tile boundary at 64"
    _summary(case, rec)


# ---------------------------------------------------------------- shape F: the large-batch route (prep_kernel + fgemm_kernel) at toy size
def test_large_batch_route_at_toy_size(plain, dev):
    """Shape F: prep_kernel in pack mode and fgemm_kernel<SP, PK> on their own stored inputs, then attention and the chain behind them."""
    model, sd, _ = plain
    B, T, tag = 3, 70, "F"
    x = synth.synth_latents(471, (B, T, 32))
    ctx = synth.synth_latents(472, (B, T, 768))
    ts = (torch.arange(B) * 137 + 500) % 1000
    eng = model._get_engine(max(B, 2), max(T, 64))
    xd, cd = x.to(dev), ctx.to(dev)
    out = {}

    def run():
        out["y"] = eng.unet_forward(xd, ts, cd)
        torch.cuda.synchronize()

    sched = _schedule_f()
    assert len(sched) == 40
    rec = []
    try:
        eng.debug_option("unet_tgemm_min_tokens", 0)
        s = Stops(eng, B, T, T, run)
        for k, la in enumerate(sched, 1):
            c = s.stop(k, la)
            _check_launch_f(tag, sd, la, c, B, T, rec)
        eng.debug_stop_after(-1)
        run()
        check_exact(f"{tag} the unstopped call's result against the last stop's eps", out["y"].cpu().transpose(1, 2), s.cur["eps"])
        log = [(d["kind"], d["epi"], d["NB"], d["KS"]) for d in eng.profile_unet(B, T, reps=1)]
    finally:
        eng.debug_stop_after(-1)
        eng.debug_option("unet_tgemm_min_tokens", -1)
    # 5 the preparation kernel, 4 the token-major fp32 GEMM (96-column tiles, KS 32 marks fgemm_kernel); the rest as in _expected_stages
    want = {"conv_in": (0, 0, 1, 8), "prep0": (5, -2, 0, 0), "prep1": (5, -2, 0, 0), "fconv1": (4, 0, 96, 32), "fconv2": (4, 0, 96, 32), "fqkv": (4, 1, 96, 32),
            "attn": (1, -1, 1, 8), "chain": (10, 0, 6, 8), "out": (12, 0, 1, 8)}
    print(f"{tag}: stage log {log}")
    assert log == [want[la[0]] for la in sched], f"{tag}: the launches are not the ones this shape is here for"
    _summary(tag, rec)
