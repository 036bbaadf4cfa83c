"""The strict-fp32 denoise step, and the default mode's routes beside the fused tail, kernel by kernel (run on the MI355X with `-m gpu`).

tests/test_gpu_unet_f32_kernels.py's method (shared code: tests/unet_f32_stops.py) on the schedules that file does not reach.  The step is stopped behind every launch
(said_debug_stop_after), the launch's inputs and outputs are read back AS STORED (the workspace list), and the output is compared with tests/unet_f32_ref.py's float64
evaluation of those inputs — its functions take unrounded operands, which is strict mode's arithmetic exactly — under the project's rule (audio_bf16_ref.check_f32):
    max |got - ref64| / max |ref64| <= 4 max(e32, 1e-6),   e32 the same figure of the torch fp32 CPU evaluation of the identical inputs,
over all samples, channels and tokens [0, T); no launch is skipped or sampled.  Every launch that stores GroupNorm partials: the normalised tensor the merged partials
imply against the float64 GroupNorm of the stored output.  Layout-only stores (the raw x2 copy, the raw skip-convolution copy in strict mode, x) and masked elements
are exact; slots a launch must leave alone (the unconditional slots of X2 behind to_out2, of O behind the band) are bit-equal to what they were; a buffer read again at a
later stop is bit-equal.  Strict mode is selected with set_mfma_dtype("fp32_strict"); effective_precision() and the split switches (all off) are asserted.

The five launches behind a block's self-attention (strict fp32 has no fused tail; the default mode leaves it where set_band's rule says the 56-key window tile cannot hold
the band), each against its own function of unet_f32_ref.py: to_out1 (attn1.to_out + the GroupNorm'ed residual from the block input's stored partials, under guidance the
duplicate y2 = x1 + c2 of every sample of the launch), q_band (to_q + the band: the fused EPI_BAND epilogue, or the plain projection on the generic GEMM followed by
band_wide_kernel in place, each held on its own), to_out2 (the conditional slots [Bc, 2 Bc) alone), geglu, ffproj (two K segments [h ; x2], float64-folded weights, + x_in).
tests/test_unet_f32_ref_cpu.py shows that chain() is their composition and that a mutant of each seam fails this rule 1.2e5 x at least.

Shapes (each the smallest that reaches what is named; asserted from the stage log — kind, epi, NB, KS per launch — and the counters: n_stchain does not move wherever the
five-launch tail is meant; what the log does not carry — fp32 or split-fp16 MFMAs, tiles per workgroup, the band rule — is held on the CPU by
tests/test_ugemm_plan_cpu.py::test_shapes_of_the_strict_fp32_kernel_test_reach_what_they_are_named_for from ugemm_plan.h, stchain.h and set_band's rule restated):
  S*          forward 2 x 70, strict, 40 launches: every fp32-MFMA NB = 1 row, the five tail launches, attn_kernel<PM 0> with 8 key slices.  Also on trained_like_state_dict.
  G*, G-eta*  one guided loop step of 1 clip x 70, strict, 40 graph nodes: shared first block, y2 duplicates, x_off / kv_off of the conditional half, out_sched_kernel<CFG>
              with its convolution on fp32 MFMAs; G-eta*: eta noise and a mask across the token-tile boundary at 64, masked elements exact.
  M1*, M2*, L*  forward 3 x 290, 5 x 290, 7 x 417, strict: NB 3 / 2 / 3 (q/k/v, to_out2, GEGLU NB 2 / 4 / 4, proj_out), multi-tile q/k/v storing plain k and v, PM 0 with
              4 key slices; at L* the log's KS is 4: attn2q_kernel (34) is not taken.
  F*          forward 3 x 70, strict, "unet_tgemm_min_tokens" = 0, 60 launches: prep_kernel without packing, fgemm_kernel on fp32 MFMAs for the convolutions and q/k/v, the
              third preparation launch, token-major GEGLU and the two-operand folded proj_out.
  F5          as F*, default precision with "st_chain" = 0: those two launches on fgemm_kernel<SP> with unpacked operands.
  Q           172 x 33 (344 token tiles, 2064 >= 2048 (sample, head, tile) triples, a sample's last tile one token), stopped behind the first SpatialTransformer:
              (a) default: plain k / v, attn_kernel<QW 4, PM 2>, the one-slice stchain_kernel<false, 1>; (b) default with "unet_tgemm_min_tokens" = 0: kv_pack pairs from
              fgemm_kernel (none inconsistent), attn_kernel<QW 4, PM 3>; (c) strict with it: PM 0 storing token-major into the operand buffer, to_out1 on fgemm_kernel
              with the coefficient residual.
  W           forward 2 x (T, S) = (10, 100) and (37, 400) (windows of 12 and 13 keys), default and strict: plain to_q + band_wide_kernel and the rest of the tail on
              split-fp16 operands and on fp32 MFMAs.
  N           forward 2 x (10, 57), default precision: the smallest (by S, then T) band of at most 8 keys that fails the tile rule (one tile spans 57 > CHAIN_KW keys):
              the five-launch tail with the fused EPI_BAND epilogue on split-fp16 operands.
  W and N have no stage log (said_profile_unet has no context length of its own): their launches are identified by the stop-by-stop comparisons and n_stchain alone.
Pad tokens are never compared: S*, L*, F*, G-eta* (forward pass and a guided step with eta noise and the mask) and W default / strict (forward pass at (37, 400)) run from a
workspace filled with 0x00, 0xFF and 0x7F and are finite and bit-identical.

Measured (MI355X, one run; e of max |ref| beside the fp32 CPU evaluation's own e32 in brackets, largest over the shapes named; the bound was its floor 4e-6 everywhere
but the trained-like self-attention, 9.5e-6 = 4 x 2.4e-6, and L*'s GEGLU, 4.04e-6).  No launch needed anything but the rule.
  strict (S*, M1*, M2*, L*, G*, G-eta*, F*, W strict, Q(c)): conv_in 1.7e-7 (2.4e-7); ResBlock conv 1 / conv 2 on ugemm_kernel's fp32 rows 3.2e-7 / 1.6e-7 (4.9e-7 / 3.2e-7),
    concatenated 3.8e-7 / 2.8e-7 (4.4e-7 / 6.0e-7), on fgemm_kernel 5.7e-7 / 2.9e-7 and 6.9e-7 / 4.8e-7 (4.6e-7 / 2.7e-7, 3.3e-7 / 4.2e-7); q / k / v 2.5e-7 / 2.4e-7 /
    2.3e-7 (6.8e-7 / 7.9e-7 / 6.9e-7), on fgemm_kernel 3.8e-7 / 3.9e-7 / 4.2e-7; self-attention PM 0 7.1e-7 (5.9e-7), token-major store 4.1e-7; to_out1 1.9e-7 (2.6e-7),
    its y2 1.9e-7, on fgemm_kernel 1.3e-7; to_q + band 2.4e-7 (5.1e-7); plain to_q 5.5e-7 (4.9e-7), band_wide_kernel 3.3e-7 (3.6e-7); to_out2 1.3e-7 (5.2e-7); GEGLU
    1.0e-6 (1.0e-6; L*), on fgemm_kernel 4.2e-7; folded proj_out 1.5e-7 (5.7e-7), on fgemm_kernel 3.1e-7; out convolution 3.3e-7; out_sched_kernel<CFG> 3.9e-7 (5.9e-7);
    prep_kernel's operands 1.4e-7 ... 2.8e-7, gn_coef 1.9e-7; GroupNorm from the stored partials 1.6e-8 ... 4.0e-8 (fp32 CPU: 1.0e-7 ... 1.6e-7); KV 4.3e-7.
  strict, trained-like (S*): self-attention 1.0e-6 (2.4e-6), to_q + band 5.2e-7, GEGLU 3.9e-7, everything else <= 3.9e-7.
  default (F5, W default, N, Q(a), Q(b)): to_out1 1.5e-7 (2.4e-7); to_q + band 2.3e-7 (6.8e-7); plain to_q 5.5e-7, band_wide_kernel 5.0e-7 (4.3e-7); to_out2 9.6e-8;
    GEGLU (fp32 rows: no one-tile split shape) 4.5e-7 (9.7e-7), on fgemm_kernel<SP> 2.4e-7; folded proj_out 1.4e-7, on fgemm_kernel<SP> 1.6e-7; attn_kernel<QW 4> PM 2 / PM 3
    2.7e-7 (4.6e-7); the one-slice chain 2.5e-7 (4.1e-7); q / k / v 2.0e-7 / 2.9e-7 / 2.8e-7; no packed pair inconsistent.
Largest e per shape: S* 5.8e-7, M1* 3.8e-7, M2* 7.7e-7, L* 1.0e-6, S* trained-like 1.05e-6, G* / G-eta* 4.1e-7, F* 6.9e-7, F5 2.6e-7, W 5.0e-7 ... 5.5e-7, N 2.8e-7,
Q(a) / Q(b) 4.0e-7, Q(c) 5.7e-7; the largest e / bound is 0.25 (L*, GEGLU).  pytest --durations (the module on its own): L* 1.1 s, S* trained-like 1.0 s,
S* 0.8 s, Q(b) 0.7 s, Q(a) 0.6 s (1.2 s in another run), Q(c) 0.4 s, M2* 0.3 s, M1* 0.2 s, F5 / F* 0.17 / 0.15 s, G* / G-eta* 0.12 / 0.13 s, W <= 0.10 s, N 0.06 s, each fill
test <= 0.05 s (the module's model 2 s once); the module 7.4 s.
"""
import contextlib
import os
import re

import numpy as np
import pytest
import torch

import unet_f32_ref as R
from audio_bf16_ref import check_exact, check_f32
from oracle import pipeline as op
from said_amd.util import synth
from unet_f32_stops import (F32, F64, GS, Stops, _check_launch, _check_launch_f, _kv_checks, _model, _partials, _poison, _schedule, _schedule_f, _summary,
                            smallest_narrow_band_the_window_tile_cannot_hold)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "said_amd", "csrc", "stchain.h")) as _f:
    CHAIN_KW = int(re.search(r"constexpr int CHAIN_KW = (\d+);", _f.read()).group(1))

#         tag    B  T    conv_in NB, 192-wide NB, concatenated NB, q/k/v NB, attention KS, to_out2 NB, GEGLU NB   (strict fp32: every row on the fp32 MFMAs;
#         tests/test_ugemm_plan_cpu.py::test_shapes_of_the_strict_fp32_kernel_test_reach_what_they_are_named_for holds that and these NB from ugemm_plan.h)
SHAPES = {"S*": (2, 70, 1, 1, 1, 1, 8, 1, 1), "M1*": (3, 290, 1, 1, 1, 3, 4, 1, 2), "M2*": (5, 290, 2, 2, 2, 2, 4, 2, 4), "L*": (7, 417, 2, 3, 2, 3, 4, 3, 4)}
F_SHAPE = (3, 70)             # F*, F5
Q_SHAPE = (172, 33)           # 344 token tiles: 2064 >= 2048 (sample, head, tile) triples; a sample's last tile is one token
W_SHAPES = ((10, 100), (37, 400))                                   # windows wider than 8 keys: 12 and 13
N_SHAPE = smallest_narrow_band_the_window_tile_cannot_hold(CHAIN_KW)   # (10, 57): windows of 8 keys, one 32-token tile spanning all 57 > CHAIN_KW = 56 keys


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def plain(dev):
    sd = synth.said_state_dict(num_w2v_layers=1)
    _, sd_u, null = op.split_state_dict(sd)
    return _model(dev, sd), sd_u, null


@contextlib.contextmanager
def _precision(model, strict):
    """The module's model in strict fp32 (set_mfma_dtype: every engine it hands out is switched) or the default mode; the default again afterwards."""
    model.set_mfma_dtype("fp32_strict" if strict else "fp32")
    try:
        yield
    finally:
        model.set_mfma_dtype("fp32")


def _engine(model, strict, batch, frames):
    eng = model._get_engine(batch, frames)
    assert eng.effective_precision() == ("fp32_strict" if strict else "fp32"), eng.effective_precision()
    # strict fp32 switches every split-fp16 product off, the fused tail (which has no other arithmetic) with them
    assert (eng.debug_get("ugemm_split"), eng.debug_get("gemm_split"), eng.debug_get("attn_split"), eng.debug_get("st_chain")) == ((0,) * 4 if strict else (1,) * 4)
    return eng


def _stages5(guided, nb_in, nb, nb_cat, nb_qkv, ks, nb_out2, nb_geglu):
    """(kind, epi, NB, KS) per launch of the channel-major schedule with the five-launch tail, as unet_sched.cpp logs them: 0 the generic GEMM, 2 ugemm_kernel
    (epi 0 store, 1 q/k/v, 2 GEGLU, 3 band), 1 attention, 11 conv_in_kernel, 12 the out convolution."""
    out = []
    for la in _schedule(False, five=True):
        k = la[0]
        if k == "conv_in":
            out.append((11, 0, 1, 4) if guided else (0, 0, nb_in, 8))
        elif k in ("conv1", "conv2"):
            out.append((2, 0, nb_cat if la[3] else nb, 8))
        elif k == "qkv5":
            out.append((2, 1, nb_qkv, 8))
        elif k == "attn":
            out.append((1, -1, 1, ks))
        elif k == "out1":
            out.append((2, 0, 1, 8))
        elif k == "qband":
            out.append((2, 3, 1, 8))
        elif k == "out2":
            out.append((2, 0, nb_out2, 8))
        elif k == "geglu":
            out.append((2, 2, nb_geglu, 8))
        elif k == "ffproj":
            out.append((2, 0, nb, 8))
        else:
            out.append((12, 0, 1, 8))
    return out


# kinds of the large-batch route: 5 the preparation kernel, 4 the token-major fp32 GEMM (KS 32 marks fgemm_kernel; NB its column tile: 96, GEGLU's 1536 columns 128)
F_STAGES = {"conv_in": (0, 0, 1, 8), "prep0": (5, -2, 0, 0), "prep1": (5, -2, 0, 0), "prep1n": (5, -2, 0, 0), "prep2": (5, -2, 0, 0), "fconv1": (4, 0, 96, 32),
            "fconv2": (4, 0, 96, 32), "fqkv": (4, 1, 96, 32), "fgeglu": (4, 2, 128, 32), "fffproj": (4, 0, 96, 32), "fout1": (4, 0, 96, 32), "attn": (1, -1, 1, 8),
            "attn_tm": (1, -1, 1, -4), "chain": (10, 0, 6, 8), "out1": (2, 0, 1, 8), "qband": (2, 3, 1, 8), "out2": (2, 0, 1, 8), "out": (12, 0, 1, 8)}


def _forward_case(model, sd, dev, tag, B, T, seed, sched, *, strict, stages=None, S=None, opts=None, upto=None, packed=None):
    """The forward pass stopped behind each of the first `upto` launches of `sched` (all of them by default); every launch on its own stored inputs.
    stages: the expected stage log (only where S = T: said_profile_unet has no context length of its own).  packed: as _check_launch_f (default: not strict)."""
    S = T if S is None else S
    packed = (not strict) if packed is None else packed
    x = synth.synth_latents(seed, (B, T, 32))
    ctx = synth.synth_latents(seed + 1, (B, S, 768))
    ts = (torch.arange(B) * 137 + 500) % 1000
    sched = sched[:upto] if upto else sched
    n_chain = sum(1 for k in range(1, len(sched) + 1) for la in sched[:k] if la[0] == "chain")
    rec = []
    out = {}
    with _precision(model, strict):
        eng = _engine(model, strict, max(B, 2), max(T, S, 64))
        xd, cd = x.to(dev), ctx.to(dev)

        def run():
            out["y"] = eng.unet_forward(xd, ts, cd)
            torch.cuda.synchronize()

        log = None
        try:
            for k, v in (opts or {}).items():
                eng.debug_option(k, v)
            s = Stops(eng, B, T, S, run)
            n0 = eng.debug_get("n_stchain")
            for k, la in enumerate(sched, 1):
                c = s.stop(k, la)
                if k == 1:
                    check_exact(f"{tag} x (channel-major latents)", c["x"], x.transpose(1, 2))
                    _kv_checks(tag, sd, s, ctx, 0, rec, kvt=n_chain > 0)
                _check_launch_f(tag, sd, la, c, B, T, rec, packed=packed, prev=s.prev, S=S)
            # stop k issues the first k launches again; a schedule without the fused tail never launches it
            assert eng.debug_get("n_stchain") - n0 == n_chain, (eng.debug_get("n_stchain") - n0, n_chain)
            eng.debug_stop_after(-1)
            run()
            assert eng.debug_get("n_stchain") - n0 == n_chain + (4 if n_chain else 0)   # (the whole pass: four fused tails, or none)
            if not upto:
                check_exact(f"{tag} the unstopped call's result against the last stop's eps", out["y"].cpu().transpose(1, 2), s.cur["eps"])
                for name in ("P", "stP", "KV"):
                    assert torch.equal(s.read(name).view(torch.int32), s.cur[name].view(torch.int32)), name
            assert torch.isfinite(out["y"]).all()
            if S == T:
                log = [(d["kind"], d["epi"], d["NB"], d["KS"]) for d in eng.profile_unet(B, T, reps=1)]
        finally:
            eng.debug_stop_after(-1)
            for k in (opts or {}):
                eng.debug_option(k, -1)
    if log is not None:
        print(f"{tag}: stage log {log}")
        assert stages is None or log[:len(sched)] == stages[:len(sched)], f"{tag}: the launches are not the ones this shape is here for"
        assert upto or len(log) == len(sched), (len(log), len(sched))
    _summary(tag, rec)


# ---------------------------------------------------------------- S*, M1*, M2*, L*: strict fp32, forward
@pytest.mark.parametrize("tag", list(SHAPES))
def test_strict_forward_launches_on_their_own_inputs(plain, dev, tag):
    """Every one of the 40 launches of the strict-fp32 forward pass (all samples): the fp32-MFMA rows of ugemm_kernel at NB 1 / 2 / 3, q/k/v storing plain k and v,
    attn_kernel<PM = 0> with 8 and 4 key slices (L*: KS 4 in the log — attn2q_kernel, KS 34, is not taken), and the five launches behind the self-attention."""
    model, sd, _ = plain
    B, T, *nbs = SHAPES[tag]
    sched = _schedule(False, five=True)
    assert len(sched) == 40
    _forward_case(model, sd, dev, tag, B, T, 500 + 10 * len(tag) + B, sched, strict=True, stages=_stages5(False, *nbs))


def test_strict_forward_launches_on_trained_like_weights(dev):
    """Shape S* on synth.trained_like_state_dict (heavy tails, outlier channels, norm gains up to 10)."""
    full = synth.trained_like_state_dict(num_w2v_layers=1)
    _, sd_u, _ = op.split_state_dict(full)
    model = _model(dev, full)
    B, T, *nbs = SHAPES["S*"]
    _forward_case(model, sd_u, dev, "S* trained-like", B, T, 531, _schedule(False, five=True), strict=True, stages=_stages5(False, *nbs))


# ---------------------------------------------------------------- G*, G-eta*: strict fp32, one guided loop step
@pytest.mark.parametrize("case", ["G*", "G-eta*"])
def test_strict_guided_step_launches_on_their_own_inputs(plain, dev, case):
    """One guided loop step of one clip x 70 frames in strict fp32: the shared first block, the y2 = x1 + c2 duplicates of to_out1, the x_off / kv_off offsets of the
    conditional half through the band and to_out2 (whose unconditional slots stay as to_out1 left them, bit for bit), then out_sched_kernel<CFG> — its convolution on
    fp32 MFMAs — against the float64 out convolution + guidance + update of its stored inputs (G-eta*: with eta = 1 noise and a mask across the tile boundary at 64)."""
    model, sd, null = plain
    Bc, T, k = 1, 70, 24
    Be = 2 * Bc
    eta = 1.0 if case == "G-eta*" else 0.0
    lat = synth.synth_latents(561, (Bc, T, 32))
    ctx = synth.synth_latents(562, (Bc, T, 768))
    sch = model.noise_scheduler
    sch.set_timesteps(50)
    ts = sch.timesteps.numpy()
    coef = sch.coef_table(ts[k:k + 2], eta)[:1]
    kw, kwd = {}, {}
    if eta > 0:
        mask = torch.zeros(Bc, T, 32)
        mask[:, 60:68] = 1
        mask[:, :, :5] = 1
        kw = dict(noise=synth.synth_latents(563, (Bc, T, 32)), init=synth.synth_latents(564, (Bc, T, 32)).abs().clamp(0, 1), enoise=synth.synth_latents(565, (Bc, T, 32)),
                  mask=mask)
        kwd = dict(step_noise=kw["noise"][None].to(dev), init_latents=kw["init"].to(dev), edit_noise=kw["enoise"].to(dev), mask=mask.to(dev))
    sched = _schedule(True, five=True)
    rec, out = [], {}
    with _precision(model, True):
        eng = _engine(model, True, Be, max(T, 64))
        latd, ctxd = lat.to(dev), ctx.to(dev)

        def run():
            out["y"] = eng.denoise_loop(latents=latd, context=ctxd, timesteps=ts[k:k + 1], coef=coef, prediction_type="epsilon", guidance_scale=GS, guidance_rescale=0.0,
                                        latent_scale=1.0, **kwd)[1]
            torch.cuda.synchronize()

        s = Stops(eng, Be, T, T, run)
        try:
            n0, c0 = eng.debug_get("n_out_sched"), eng.debug_get("n_stchain")
            for n, la in enumerate(sched[:-1], 1):
                c = s.stop(n, la)
                if n == 1:
                    check_exact(f"{case} x (channel-major latents)", c["x"][:Bc], lat.transpose(1, 2))
                    _kv_checks(case, sd, s, ctx, Bc, rec, kvt=False)
                _check_launch(case, sd, null, la, c, Be, Bc, rec, packed=False, prev=s.prev)
            assert eng.debug_get("n_out_sched") == n0, "no stop so far reached the step's last launch"
            eng.debug_stop_after(-1)
            run()
            assert eng.debug_get("n_out_sched") > n0 and eng.debug_get("n_stchain") == c0
            nodes = eng.graph_num_nodes()
            print(f"{case}: {nodes} graph nodes")
            assert nodes == len(sched) == 40
            for name in ("P", "stP"):
                assert torch.equal(s.read(name).view(torch.int32), s.cur[name].view(torch.int32)), name
            log = [(d["kind"], d["epi"], d["NB"], d["KS"]) for d in eng.profile_unet(Be, T, reps=1, cfg_clips=Bc)]
        finally:
            eng.debug_stop_after(-1)
    assert log == _stages5(True, 1, 1, 1, 1, 8, 1, 1), log
    got = out["y"].cpu()
    P = s.cur["P"]
    cm = {n: v.transpose(1, 2) for n, v in kw.items()}
    fn = lambda dt: R.out_sched(sd, P, lat.transpose(1, 2), coef[0], GS, dt, **cm).transpose(1, 2)
    rec.append(("out_sched",) + check_f32(f"{case} out_sched_kernel<CFG>", got, fn(F64), fn(F32)))
    rec.append(("stP",) + _partials(f"{case} st3 folded proj_out (out_sched's input)", P, s.cur["stP"]))
    if eta > 0:   # masked elements do not depend on the model output: add_noise(init, edit_noise, t_next) in fp32, bit for bit
        m = kw["mask"].bool()
        cf = torch.from_numpy(np.asarray(coef[0], dtype=np.float32))
        assert float(cf[5]) != 1.0 and float(cf[6]) != 0.0, "the blend's pair is the next timestep's"
        noisy = cf[5] * kw["init"] + cf[6] * kw["enoise"]
        assert torch.equal(got[m], noisy[m]), "a masked element is not the noised initial latent"
        assert bool(m[:, 60:68].all()) and not bool(m[:, 68:, 5:].any()), "the mask crosses the token-tile boundary at 64"
    _summary(case, rec)


# ---------------------------------------------------------------- F*, F5: the large-batch route at toy size without the fused tail
@pytest.mark.parametrize("tag", ["F*", "F5"])
def test_large_batch_route_without_the_fused_tail(plain, dev, tag):
    """3 x 70 with "unet_tgemm_min_tokens" = 0.  F* (strict fp32): prep_kernel without packing, fgemm_kernel on fp32 MFMAs for the convolutions and q/k/v (plain k and
    v), and behind the channel-major to_out1 / band / to_out2 the token-major GEGLU and two-operand folded proj_out launches.  F5 (default precision, "st_chain" = 0):
    the same two launches on fgemm_kernel<SP> with unpacked operands, behind packed convolution and q/k/v operands."""
    model, sd, _ = plain
    strict = tag == "F*"
    B, T = F_SHAPE
    sched = _schedule_f(five=True)
    assert len(sched) == 60
    opts = {"unet_tgemm_min_tokens": 0} if strict else {"unet_tgemm_min_tokens": 0, "st_chain": 0}
    _forward_case(model, sd, dev, tag, B, T, 571 if strict else 575, sched, strict=strict, stages=[F_STAGES[la[0]] for la in sched], opts=opts)


# ---------------------------------------------------------------- W, N: bands the fused tail's window tile cannot hold
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("TS", W_SHAPES, ids=lambda ts: "%dx%d" % ts)
def test_wide_band_launches_on_their_own_inputs(plain, dev, TS, strict):
    """W: 2 x (T, S) with windows wider than 8 keys: the plain to_q projection (the generic GEMM) + band_wide_kernel in place, and the rest of the five-launch tail,
    on split-fp16 operands (default) and on fp32 MFMAs (strict); stchain_kernel never runs."""
    model, sd, _ = plain
    T, S = TS
    tag = f"W {T} x {S} {'strict' if strict else 'default'}"
    _forward_case(model, sd, dev, tag, 2, T, 580 + T, _schedule(False, five=True, wide=True), strict=strict, S=S)


def test_narrow_band_the_window_tile_cannot_hold(plain, dev):
    """N: 2 x (10, 57), default precision — windows of at most 8 keys, so the fused EPI_BAND epilogue, but one token tile spans more than CHAIN_KW keys, so the
    five-launch tail on split-fp16 operands (k and v packed for attn_kernel<PM = 3>); stchain_kernel never runs."""
    model, sd, _ = plain
    T, S = N_SHAPE
    assert (T, S) == (10, 57)
    _forward_case(model, sd, dev, f"N {T} x {S}", 2, T, 591, _schedule(False, five=True), strict=False, S=S)


# ---------------------------------------------------------------- Q: 2064 (sample, head, tile) triples, stopped behind the first SpatialTransformer
def _q_sched(route):
    if route == "a":     # channel-major: conv_in, the first ResBlock, q/k/v (plain k and v: no key split), attn_kernel<QW 4, PM 2>, the one-slice stchain_kernel
        return _schedule(False)[:6]
    f = _schedule_f()
    if route == "b":     # large-batch route: ..., prep_kernel, fgemm_kernel with the kv_pack epilogue, attn_kernel<QW 4, PM 3>, the one-slice stchain_kernel
        return f[:9]
    # strict: ..., attn_kernel<QW 4, PM 0> storing token-major into the q/k/v operand buffer, to_out1 on fgemm_kernel with the coefficient residual
    return f[:7] + [("attn_tm", 0), ("fout1", 0, "P")]


@pytest.mark.parametrize("route", ["a", "b", "c"])
def test_four_query_tile_attention_and_what_follows_it(plain, dev, route):
    """Q: 172 x 33.  (a) default mode; (b) default mode with "unet_tgemm_min_tokens" = 0; (c) strict fp32 with "unet_tgemm_min_tokens" = 0.  The fused tail of (a) and
    (b) runs as one slice per token tile: 344 tiles > CHAIN2_MAX_TILES."""
    model, sd, _ = plain
    B, T = Q_SHAPE
    assert B * ((T + 31) // 32) * R.HEADS == 2064 >= 2048
    sched = _q_sched(route)
    qa = {"conv_in": (0, 0, 2, 8), "conv1": (2, 0, 2, 8), "conv2": (2, 0, 2, 8), "qkv": (2, 1, 3, 8), "attn": (1, -1, 1, -4), "chain": (10, 0, 6, 8)}
    qf = dict(F_STAGES, conv_in=(0, 0, 2, 8), attn=(1, -1, 1, -4))
    stages = [(qa if route == "a" else qf)[la[0]] for la in sched]
    _forward_case(model, sd, dev, f"Q({route})", B, T, 600, sched, strict=route == "c", stages=stages, opts=None if route == "a" else {"unet_tgemm_min_tokens": 0},
                  upto=len(sched), packed=route == "b")


# ---------------------------------------------------------------- the stand-in for comparing pad tokens
@pytest.mark.parametrize("tag", ["S*", "L*", "F*", "G-eta*", "W default", "W strict"])
def test_workspace_fill_does_not_reach_a_result(plain, dev, tag):
    """Forward pass and one guided step (eta noise, mask across the tile boundary at 64) from a workspace of zeros, NaNs and 3.4e38: finite and bit-identical.
    W: the forward pass at 2 x (37, 400) (the loop has no context length of its own)."""
    model, _, _ = plain
    strict = tag != "W default"
    with _precision(model, strict):
        if tag.startswith("W"):
            T, S = W_SHAPES[1]
            eng = _poison(model, dev, 2, T, 650, S=S, guided=False)
        elif tag == "F*":
            eng = _poison(model, dev, *F_SHAPE, 660, {"unet_tgemm_min_tokens": 0})
        elif tag == "G-eta*":
            eng = _poison(model, dev, 1, 70, 670)
        else:
            eng = _poison(model, dev, *SHAPES[tag][:2], 640 + SHAPES[tag][0])
        assert eng.effective_precision() == ("fp32_strict" if strict else "fp32")
