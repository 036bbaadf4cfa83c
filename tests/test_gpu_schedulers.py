"""DDPM and DPM-Solver++(2M) on the HIP engine (`-m gpu`): the stand-alone step against the CPU restatement of diffusers 0.19
(tests/sched_ref.py) bit for bit, whole loops against the oracle UNet driven by that restatement, every update site of the step's last
kernel, clip groups, device noise, graph sizes and the engine's refusals.

Synthetic weights and epsilon prediction make DPM-Solver++ ill-conditioned: its x0 = (x - sigma eps) / alpha divides by
alpha(999) = 4.9e-5 and, unlike DDIM and DDPM, is not clipped, so the model's last-bit differences grow by ~1e3 in the first step.
Comparisons of two model evaluations therefore use v_prediction (x0 = alpha x - sigma v) unless they are bit-exact; epsilon is covered
bit for bit by the stand-alone step and, in a whole loop, relative to the latents' own scale."""
import numpy as np
import pytest
import torch

from oracle import pipeline as op
from said_amd import _engine
from said_amd.scheduler import SCHEDULERS, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler
from said_amd.util import synth

import sched_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd_full():
    return synth.said_state_dict()


@pytest.fixture(scope="module")
def model(dev, sd_full):
    from said_amd.model.diffusion import SAID_UNet1D
    m = SAID_UNet1D()
    m.load_state_dict(sd_full, strict=True)
    m.to(dev).eval()
    return m


class _Sched:
    """model.noise_scheduler = <name> for the block (SAID_UNet1D does not forward noise_scheduler, as in the reference); DDIM after."""

    def __init__(self, model, name, pred="epsilon"):
        self.model, self.name, self.pred = model, name, pred

    def __enter__(self):
        self.model.noise_scheduler = SCHEDULERS[self.name](num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", prediction_type=self.pred)
        return self.model.noise_scheduler

    def __exit__(self, *exc):
        self.model.noise_scheduler = DDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", prediction_type="epsilon")


def _counts(eng, fresh=False):
    """Launches issued so far through the step's last kernel, per kernel (the host-side stage counters).  fresh: drop the cached step graph
    first (any said_debug_option does; "out_tm" -1 is its default), so that the next loop captures and counts its own."""
    if fresh:
        eng.debug_option("out_tm", -1)
    return {k: eng.debug_get(k) for k in ("n_out_sched", "n_out_sched_tm", "n_sched_step")}


def _grew(before, after):
    return {k for k in before if after[k] > before[k]}


# ---------------------------------------------------------------- said_solver_step: bit-exact against the CPU restatement
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", ["ddpm", "dpm1", "dpm2"])
@pytest.mark.parametrize("pred", ["epsilon", "sample", "v_prediction"])
def test_solver_step_bit_exact(model, dev, pred, kind, masked):
    B, T, C = 2, 60, 32
    e_c, e_u, x = (synth.synth_latents(700 + i, (B, T, C)) for i in range(3))
    hist, z, init, en = (synth.synth_latents(710 + i, (B, T, C)) for i in range(4))
    mask = (synth.synth_latents(720, (B, T, C)) > 0).float() if masked else None
    gs = 2.5
    e = e_c + gs * (e_c - e_u)   # diffusion.py:430-434
    if kind == "ddpm":
        s, r = DDPMScheduler(prediction_type=pred), sched_ref.RefDDPM(pred)
        s.set_timesteps(50)
        r.set_timesteps(50)
        t, t_next = 500, 480
        row = s._coef_row(t, t_next)
        want = r.step(e, t, x, z)
    else:
        s, r = DPMSolverMultistepScheduler(prediction_type=pred), sched_ref.RefDPM(pred)
        s.set_timesteps(25)
        r.set_timesteps(25)
        i = 6
        t, t_next = int(r.timesteps[i]), int(r.timesteps[i + 1])
        order = 2 if kind == "dpm2" else 1
        row = s._coef_row(i, order, t_next)
        r.model_outputs, r.lower_order_nums = [None, hist], order - 1
        want = r.step(e, t, x)
    assert np.array_equal(row, r.row(i, order, t_next) if kind != "ddpm" else r.row(t, t_next))
    if masked:
        want = r.add_noise(init, en, t_next) * mask + want * (1 - mask)
    eng = model._get_engine(2, 64)
    h = hist.clone().to(dev)
    got = eng.solver_step(e_c.to(dev), x.to(dev), row, pred, x0_hist=h, model_output_uncond=e_u.to(dev), guidance_scale=gs,
                          step_noise=z.to(dev) if kind == "ddpm" else None, init_latents=init.to(dev) if masked else None,
                          edit_noise=en.to(dev) if masked else None, mask=mask.to(dev) if masked else None).cpu()
    print(f"said_solver_step {kind} {pred} mask={masked}: max |gpu - cpu| {float((got - want).abs().max()):.3e}")
    assert torch.equal(got, want)
    if kind == "ddpm":
        assert torch.equal(h.cpu(), hist)                     # DDPM keeps no history
    else:
        assert torch.equal(h.cpu(), r.model_outputs[1])       # this step's x0, for the next step


def test_scheduler_step_api_runs_the_engine(model, dev):
    """DPMSolverMultistepScheduler.step / DDPMScheduler.step (the diffusers-style surface) go through said_solver_step, history included."""
    x0 = synth.synth_latents(730, (1, 30, 32))
    outs = [synth.synth_latents(731 + k, (1, 30, 32)) for k in range(4)]
    with _Sched(model, "dpmsolver++", "v_prediction") as s:
        model._get_engine(2, 64)   # (attaches the engine to the scheduler in the slot)
        s.set_timesteps(4)
        r = sched_ref.RefDPM("v_prediction")
        r.set_timesteps(4)
        x, xr = x0.to(dev), x0.clone()
        for k, t in enumerate(s.timesteps):
            x = s.step(outs[k].to(dev), t, x).prev_sample
            xr = r.step(outs[k], int(t), xr)
        assert torch.equal(x.cpu(), xr)
    with _Sched(model, "ddpm") as s:
        model._get_engine(2, 64)
        s.set_timesteps(4)
        r = sched_ref.RefDDPM()
        r.set_timesteps(4)
        z = synth.synth_latents(740, (1, 30, 32))
        got = s.step(outs[0].to(dev), s.timesteps[0], x0.to(dev), variance_noise=z.to(dev)).prev_sample
        assert torch.equal(got.cpu(), r.step(outs[0], int(s.timesteps[0]), x0, z))


# ---------------------------------------------------------------- whole loops against the oracle UNet + the restatement
def _loop(model, sd_full, dev, sched, *, N, B=1, Ta=16000, gs=2.0, rescale=0.0, pred="v_prediction", edit=False, strength=1.0, tol=1e-3,
          step_noise_seed=None):
    T = int(Ta / 16000 * 60)
    proc = op.process_audio([synth.synth_waveform(10 + i, Ta).numpy() for i in range(B)])
    lat = synth.synth_latents(100, (B, T, 32))
    kw, okw = {}, {}
    if edit:
        init = torch.sigmoid(synth.synth_latents(101, (B, T, 32))) * 0.5
        mask = torch.zeros(B, T, 32)
        mask[:, : T // 3] = 1.0
        mask[:, :, :4] = 1.0
        en = synth.synth_latents(102, (B, T, 32))
        kw = dict(init_samples=init.to(dev), mask=mask.to(dev), edit_noise=en.to(dev))
        okw = dict(init_samples=init, mask=mask, edit_noise=en)
    init_t = min(int(N * strength), N)
    sn = synth.synth_latents(103, (init_t, B, T, 32)) if sched == "ddpm" else None
    with _Sched(model, sched, pred):
        eng = model._get_engine(2 * B if gs > 1 else B, T)
        c0 = _counts(eng, fresh=True)
        out = model.inference(proc.to(dev), num_inference_steps=N, strength=strength, guidance_scale=gs, guidance_rescale=rescale,
                              init_latents=lat.to(dev), step_noise=None if sn is None else sn.to(dev), **kw)
        grew = _grew(c0, _counts(eng))
        nodes = eng.graph_num_nodes()
    ref, _ = sched_ref.inference(sd_full, proc, sched, init_latents=lat, num_inference_steps=N, strength=strength, guidance_scale=gs,
                                 guidance_rescale=rescale, prediction_type=pred, step_noise=sn, **okw)
    got = out.result.cpu()
    err = float((got - ref).abs().max())
    print(f"{sched} {pred} N={N} B={B} gs={gs} rescale={rescale} edit={edit} strength={strength}: max abs err vs oracle {err:.3e}; "
          f"last kernel {sorted(grew)}, {nodes} graph nodes per step")
    assert got.shape == (B, T, 32) and 0.0 <= float(got.min()) and float(got.max()) <= 1.0
    assert err <= tol, err
    return grew


@pytest.mark.parametrize("N", [1, 2, 14, 15, 25])
def test_dpm_loop_vs_oracle_fused_out_sched_kernel(model, sd_full, dev, N):
    """fp32, one clip under guidance: the update runs in out_sched_kernel<CFG, SP, 1> (the stage counters say which kernel ran)."""
    grew = _loop(model, sd_full, dev, "dpmsolver++", N=N)
    assert grew == {"n_out_sched"}


def test_dpm_loop_vs_oracle_rescale_sched_step_kernel(model, sd_full, dev):
    """guidance_rescale > 0 keeps the unfused route: the update runs in sched_step_kernel<1>."""
    grew = _loop(model, sd_full, dev, "dpmsolver++", N=14, B=2, Ta=8000, gs=2.5, rescale=0.7)
    assert grew == {"n_sched_step"}


def test_dpm_loop_vs_oracle_editing_mask_strength(model, sd_full, dev):
    """init_samples + mask at strength 0.5: the loop starts mid-schedule, first order, with the history empty."""
    _loop(model, sd_full, dev, "dpmsolver++", N=25, B=2, edit=True, strength=0.5)


def test_dpm_loop_sample_prediction(model, sd_full, dev):
    _loop(model, sd_full, dev, "dpmsolver++", N=15, pred="sample")


def test_dpm_loop_epsilon_strict_retry_and_oracle(model, sd_full, dev):
    """epsilon (see the module docstring): with these weights the latents grow to ~1e5, past the split-fp16 products' operand domain
    (|x| < 65504), so fp32 mode sees a non-finite model output and SAID.inference re-runs the call on fp32 matrix instructions — from the
    same start, the first step first order, so the retry overwrites the x0 history before it reads it: bit-identical to a strict run.
    The strict run's final latents match the oracle relative to their own scale."""
    B, T, N = 1, 60, 15
    proc = op.process_audio([synth.synth_waveform(10, 16000).numpy()])
    lat = synth.synth_latents(100, (B, T, 32))
    emb = model.get_audio_embedding(proc.to(dev), T)
    with _Sched(model, "dpmsolver++", "epsilon") as s:
        with pytest.warns(RuntimeWarning, match="split-fp16"):
            retried = model.inference(proc.to(dev), num_inference_steps=N, guidance_scale=2.0, init_latents=lat.to(dev), audio_embedding=emb).result
        try:
            model.set_mfma_dtype("fp32_strict")
            strict = model.inference(proc.to(dev), num_inference_steps=N, guidance_scale=2.0, init_latents=lat.to(dev), audio_embedding=emb).result
            s.set_timesteps(N)
            ts = s.timesteps.numpy()
            _, latf, _ = model._get_engine(2, T).denoise_loop(latents=lat.to(dev), context=emb, timesteps=ts, coef=s.coef_table(ts),
                                                              prediction_type="epsilon", guidance_scale=2.0, guidance_rescale=0.0, latent_scale=1.0)
        finally:
            model.set_mfma_dtype("fp32")
    assert torch.equal(retried, strict)
    _, ref = sched_ref.inference(sd_full, proc, "dpmsolver++", init_latents=lat, num_inference_steps=N, guidance_scale=2.0,
                                 prediction_type="epsilon", audio_embedding=emb.cpu())
    rel = float((latf.cpu() - ref).abs().max()) / float(ref.abs().max())
    print(f"dpmsolver++ epsilon N={N}, strict fp32: final latents max |gpu - oracle| / max |oracle| {rel:.3e} (latent scale {float(ref.abs().max()):.3e})")
    assert torch.isfinite(latf).all() and rel <= 1e-3


def test_ddpm_loop_vs_oracle_injected_noise(model, sd_full, dev):
    grew = _loop(model, sd_full, dev, "ddpm", N=10, B=2, pred="epsilon")
    assert grew == {"n_out_sched"}


def test_ddpm_editing_vs_oracle(model, sd_full, dev):
    _loop(model, sd_full, dev, "ddpm", N=20, B=1, edit=True, strength=0.5, pred="epsilon")


def test_ddpm_device_noise_equals_the_same_loop_fed_philox_draws(model, dev):
    """use_step_noise = 2 (Philox inside the step's last kernel): the same loop with said_philox_normal's draws injected gives the same bits."""
    B, T, N = 2, 60, 8
    wav = torch.zeros(B, T * 16000 // 60, device=dev)
    emb = synth.synth_latents(750, (B, T, 768)).to(dev)
    lat = synth.synth_latents(751, (B, T, 32)).to(dev)
    with _Sched(model, "ddpm"):
        torch.manual_seed(21)
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))   # the one draw SAID.inference makes
        torch.manual_seed(21)
        a = model.inference(wav, num_inference_steps=N, guidance_scale=2.0, init_latents=lat, audio_embedding=emb).result
        sn = model._eng.philox_normal(seed, 0, N, (B, T, 32))
        b = model.inference(wav, num_inference_steps=N, guidance_scale=2.0, init_latents=lat, audio_embedding=emb, step_noise=sn).result
        c = model.inference(wav, num_inference_steps=N, guidance_scale=2.0, init_latents=lat, audio_embedding=emb, step_noise=torch.zeros_like(sn)).result
    assert torch.equal(a, b)
    assert not torch.equal(a, c)   # the noise is there at all


# ---------------------------------------------------------------- bf16 large batch: out_sched_tm_kernel, clip groups, graph sizes
def test_dpm_bf16_batch32_out_sched_tm_kernel(model, dev):
    """bf16, 32 clips x 600 frames under guidance: the update runs in out_sched_tm_kernel<CFG, 1>; against the same loop on round 3's
    channel-major route (said_debug_option "out_tm" = 0: out_sched_kernel<CFG, SP, 1>) within the bf16 per-step bound, masked frames identical."""
    B, T, N = 32, 600, 3
    ctx = synth.synth_latents(960, (B, T, 768)).to(dev)
    init = synth.synth_latents(961, (B, T, 32)).abs().clamp(0, 1).to(dev)
    en = synth.synth_latents(962, (B, T, 32)).to(dev)
    mask = torch.zeros(B, T, 32, device=dev)
    mask[:, 100:300] = 1
    wav = torch.zeros(B, T * 16000 // 60, device=dev)
    res, grew = {}, {}
    try:
        model.set_mfma_dtype("bf16")
        model.clip_groups = 1
        with _Sched(model, "dpmsolver++", "v_prediction"):
            for ot in (0, 1):
                eng = model._get_engine(2 * B, T)
                eng.debug_option("out_tm", ot)
                c0 = _counts(eng)
                res[ot] = model.inference(wav, audio_embedding=ctx, num_inference_steps=N, guidance_scale=2.0, init_samples=init, mask=mask,
                                          edit_noise=en).result
                grew[ot] = _grew(c0, _counts(eng))
    finally:
        model._eng.debug_option("out_tm", -1)
        model.clip_groups = None
        model.set_mfma_dtype("fp32")
    d = float((res[0] - res[1]).abs().max())
    print(f"dpm bf16 B=32: out_sched_tm vs channel-major route, max |diff| after {N} steps {d:.3e}; kernels {grew}")
    assert grew[1] == {"n_out_sched_tm"} and grew[0] == {"n_out_sched"}
    assert torch.isfinite(res[1]).all() and d <= 0.087
    assert torch.equal(res[1][:, 100:300], res[0][:, 100:300])


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_dpm_clip_groups_equal_whole_batch(model, dev, mode):
    """Concurrent clip groups (each context its own x0 history) against the unsplit batch: bf16 bit-identical, fp32 within the existing group
    tolerance (the GEMM tile follows the launch size)."""
    B, T, N = 32, 600, 6
    wav = torch.zeros(B, T * 16000 // 60, device=dev)
    emb = synth.synth_latents(780, (B, T, 768)).to(dev)
    lat = synth.synth_latents(781, (B, T, 32)).to(dev)
    out = {}
    model.set_mfma_dtype(mode)
    try:
        with _Sched(model, "dpmsolver++", "v_prediction"):
            for g in (1, 2, 3):
                model.clip_groups = g
                out[g] = model.inference(wav, num_inference_steps=N, guidance_scale=2.0, init_latents=lat, audio_embedding=emb,
                                         save_intermediate=True)
    finally:
        model.clip_groups = None
        model.set_mfma_dtype("fp32")
    for g in (2, 3):
        d = float((out[1].result - out[g].result).abs().max())
        di = max(float((x - y).abs().max()) for x, y in zip(out[1].intermediates, out[g].intermediates))
        print(f"dpm clip groups {mode}, {g} groups: max |whole - split| result {d:.3e}, intermediates {di:.3e}")
        if mode == "bf16":
            assert d == 0.0 and di == 0.0
        else:
            assert d <= 1e-4 and di <= 5e-4


@pytest.mark.parametrize("mode,B,T,nodes", [("fp32", 1, 600, 24), ("bf16", 32, 600, 28), ("fp32", 32, 600, 40)])
def test_dpm_graph_nodes_per_step_equal_ddim(model, dev, mode, B, T, nodes):
    """bench.py's default line, configs[2] and the fp32 batch-32 line (one group): the DPM step graph holds as many launches as DDIM's,
    and a cached DDIM graph is not replayed for DPM (the solver family is part of the graph key)."""
    wav = torch.zeros(B, T * 16000 // 60, device=dev)
    emb = synth.synth_latents(790, (B, T, 768)).to(dev)
    lat = synth.synth_latents(791, (B, T, 32)).to(dev)
    got = {}
    model.set_mfma_dtype(mode)
    model.clip_groups = 1
    try:
        for name in ("ddim", "dpmsolver++"):
            with _Sched(model, name, "v_prediction"):
                r = model.inference(wav, num_inference_steps=2, guidance_scale=2.0, init_latents=lat, audio_embedding=emb).result
                got[name] = (model._eng.graph_num_nodes(), r)
    finally:
        model.clip_groups = None
        model.set_mfma_dtype("fp32")
    print(f"graph nodes per step {mode} B={B}: ddim {got['ddim'][0]}, dpm {got['dpmsolver++'][0]}")
    assert got["ddim"][0] == got["dpmsolver++"][0] == nodes
    assert not torch.equal(got["ddim"][1], got["dpmsolver++"][1])


# ---------------------------------------------------------------- refusals
def test_engine_refuses_foreign_scheduler_and_malformed_tables(model, dev):
    class Foreign:
        timesteps = torch.arange(3)
        init_noise_sigma = 1.0

        def set_timesteps(self, n, device=None):
            pass
    old = model.noise_scheduler
    model.noise_scheduler = Foreign()
    try:
        with pytest.raises(TypeError, match="DDIMScheduler, DDPMScheduler or DPMSolverMultistepScheduler"):
            model.inference(torch.zeros(1, 1600, device=dev), num_inference_steps=3)
    finally:
        model.noise_scheduler = old
    B, T = 1, 30
    eng = model._get_engine(2, 64)
    ctx = synth.synth_latents(800, (B, T, 768)).to(dev)
    lat = synth.synth_latents(801, (B, T, 32)).to(dev)
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(5)
    ts = s.timesteps.numpy()
    good = s.coef_table(ts)
    d = DDIMScheduler()
    d.set_timesteps(5)
    kw = dict(latents=lat, context=ctx, timesteps=ts, prediction_type="epsilon", guidance_scale=1.0, guidance_rescale=0.0, latent_scale=1.0)
    bad_code = good.copy(); bad_code[2, 7] = 5.0
    bad_frac = good.copy(); bad_frac[1, 7] = 2.5
    first2 = good.copy(); first2[0, 7] = 3.0
    mixed = np.concatenate([good[:2], d.coef_table(d.timesteps.numpy()[2:], 0.0)])
    for tab, msg in ((bad_code, "unknown solver code"), (bad_frac, "unknown solver code"), (first2, "first step"), (mixed, "mixed")):
        with pytest.raises(_engine.EngineError, match=msg):
            eng.denoise_loop(coef=tab, **kw)
    with pytest.raises(_engine.EngineError, match="step noise"):
        eng.denoise_loop(coef=good, noise_seed=7, **kw)
    with pytest.raises(_engine.EngineError, match="solver code"):
        eng.solver_step(lat, lat, d.coef_table(d.timesteps.numpy(), 0.0)[0], "epsilon")
    with pytest.raises(_engine.EngineError, match="x0_hist"):
        eng.solver_step(lat, lat, good[1], "epsilon")
    eng.denoise_loop(coef=good, **kw)   # the well-formed table still runs after the refusals
