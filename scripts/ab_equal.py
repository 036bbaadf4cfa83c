"""Bit-identity of two builds of the engine: runs the UNet (fp32 and bf16 mode, a few shapes), a short guided loop and the audio encoder (fp32 mode; bf16 mode on the
direct-to-LDS and on the staged tile kernels) on the library given as argv[1] and saves / compares the results with those of a previous invocation:   python scripts/ab_equal.py <lib> save|cmp <file>
Also short loops through every route of the step's last kernel (editing mask, device noise, DDPM, DPM-Solver++, guidance_rescale, bf16 at 32 clips) and one said_ddim_step / said_solver_step call."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from said_amd import _engine  # noqa: E402

_engine._LIB_PATH = os.path.abspath(sys.argv[1])
from said_amd.model.diffusion import SAID_UNet1D  # noqa: E402
from said_amd.util import synth  # noqa: E402

torch.set_grad_enabled(False)
dev = torch.device("cuda:0")
out = {}
for mode in ("fp32", "bf16"):
    m = SAID_UNet1D()
    m.load_state_dict(synth.said_state_dict(), strict=True)
    m.to(dev).eval()
    m.set_mfma_dtype(mode)
    for B, T in ((2, 600), (3, 333), (1, 37), (16, 600), (2, 1800)):
        x = synth.synth_latents(11, (B, T, 32)).to(dev)
        c = synth.synth_latents(12, (B, T, 768)).to(dev)
        ts = torch.full((B,), 500, dtype=torch.long)
        out[f"{mode}_fwd_{B}x{T}"] = m.forward(x, ts.to(dev), c).cpu()
    lat = synth.synth_latents(7, (1, 600, 32)).to(dev)
    emb = synth.synth_latents(8, (1, 600, 768)).to(dev)
    out[f"{mode}_loop"] = m.inference(torch.zeros(1, 160000, device=dev), num_inference_steps=12, guidance_scale=2.0, eta=0.0, init_latents=lat, audio_embedding=emb).result.cpu()
# the update that ends a step, through each of its kernels: short loops on the engine (result, final latents and intermediates), one stand-alone step each
from said_amd.scheduler import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler  # noqa: E402


def short_loop(m, B, T, kind, N=4, eta=0.0, pred="epsilon", masked=False, seed=None, rescale=0.0):
    s = {"ddim": DDIMScheduler, "ddpm": DDPMScheduler, "dpm": DPMSolverMultistepScheduler}[kind](prediction_type=pred)
    s.set_timesteps(N)
    ts = s.timesteps.numpy()
    coef = s.coef_table(ts, eta) if kind == "ddim" else s.coef_table(ts)
    kw = {}
    if masked:
        mask = torch.zeros(B, T, 32, device=dev)
        mask[:, T // 4:T // 2, :8] = 1
        kw = dict(init_latents=torch.sigmoid(synth.synth_latents(23, (B, T, 32))).to(dev), edit_noise=synth.synth_latents(24, (B, T, 32)).to(dev), mask=mask)
    r = m._get_engine(2 * B, T).denoise_loop(latents=synth.synth_latents(21, (B, T, 32)).to(dev), context=synth.synth_latents(22, (B, T, 768)).to(dev), timesteps=ts, coef=coef,
                                             prediction_type=pred, guidance_scale=2.0, guidance_rescale=rescale, latent_scale=1.0, save_intermediate=True, noise_seed=seed, **kw)
    return torch.cat([t.flatten() for t in r]).cpu()


m.set_mfma_dtype("fp32")
out["loop_mask"] = short_loop(m, 2, 333, "ddim", masked=True)
out["loop_eta1_device_noise"] = short_loop(m, 2, 333, "ddim", eta=1.0, seed=1234567)
out["loop_ddpm"] = short_loop(m, 1, 600, "ddpm", N=5, seed=7654321, masked=True)
out["loop_dpm"] = short_loop(m, 2, 333, "dpm", N=6, pred="v_prediction")
out["loop_rescale"] = short_loop(m, 2, 333, "ddim", eta=1.0, seed=99, rescale=0.7, masked=True)
out["loop_rescale_dpm"] = short_loop(m, 1, 37, "dpm", N=3, pred="v_prediction", rescale=0.7)
m.set_mfma_dtype("bf16")
out["bf16_loop_32x600_mask"] = short_loop(m, 32, 600, "ddim", N=3, eta=1.0, seed=5, masked=True)
out["bf16_loop_32x600_dpm"] = short_loop(m, 32, 600, "dpm", N=3, pred="v_prediction", masked=True)
m.set_mfma_dtype("fp32")
eng = m._get_engine(2, 64)
e_c, e_u, x, z, init, en, hist = (synth.synth_latents(30 + i, (2, 61, 32)).to(dev) for i in range(7))
mk = (synth.synth_latents(37, (2, 61, 32)) > 0).float().to(dev)
s = DDIMScheduler()
s.set_timesteps(50)
out["ddim_step"] = eng.ddim_step(e_c, x, s._coef_row(500, 1.0, 480), "epsilon", eps_uncond=e_u, guidance_scale=2.5, step_noise=z, init_latents=init, edit_noise=en, mask=mk).cpu()
s = DPMSolverMultistepScheduler(prediction_type="v_prediction")
s.set_timesteps(25)
out["solver_step"] = eng.solver_step(e_c, x, s._coef_row(6, 2, int(s.timesteps[7])), "v_prediction", x0_hist=hist, model_output_uncond=e_u, guidance_scale=2.5, init_latents=init,
                                     edit_noise=en, mask=mk).cpu()
out["solver_step_x0_hist"] = hist.cpu()
# the audio encoder: bf16 mode runs the per-sample tile kernels of tgemm.hip (feature extractor, grouped positional convolution, projections), which no UNet case reaches
from oracle import pipeline as op  # noqa: E402
from said_amd.model.wav2vec2 import AudioConfig  # noqa: E402

m = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=2))
m.load_state_dict(synth.said_state_dict(num_w2v_layers=2), strict=True)
m.to(dev).eval()
eng = m._get_engine(2, 64)
for B, secs in ((1, 3), (2, 10), (32, 10)):
    proc = op.process_audio([synth.synth_waveform(700 + i, 16000 * secs).numpy() for i in range(B)]).to(dev)
    for mode, direct in (("fp32", -1), ("bf16", 1), ("bf16", 0)):
        m.set_mfma_dtype(mode)
        eng.debug_option("tgemm_direct", direct)
        out[f"{mode}_audio_{B}x{secs}s_direct{direct}"] = m.get_audio_embedding(proc, 60 * secs).cpu()
eng.debug_option("tgemm_direct", -1)
m.set_mfma_dtype("fp32")
if sys.argv[2] == "save":
    torch.save(out, sys.argv[3])
    print("saved", len(out), "tensors")
else:
    ref = torch.load(sys.argv[3])
    bad = [k for k in out if not torch.equal(out[k], ref[k])]
    for k in out:
        print(f"{k:32s} max |diff| {float((out[k] - ref[k]).abs().max()):.3e}")
    print("BIT-IDENTICAL" if not bad else f"DIFFERENT: {bad}")
