"""The one per-element update that ends a denoise step (sched_math.h step_update), through every kernel route of the loop (`-m gpu`):
out_sched_kernel (fp32, fused), sched_step_kernel (guidance_rescale > 0, unfused) and out_sched_tm_kernel (bf16, token-major).

Shape: B = 2 clips, T = 33 frames (one full and one partial 32-token tile), 32 channels, N = 3 steps, guidance 2.0, intermediates saved.
The stage counters say which kernel ran.  What the update adds is checked bit for bit: device noise against the same loop fed the
Philox draws, masked elements against the last row's add_noise, the first intermediate against the input.  DPM-Solver++ (step 1 is a
second-order row, so it reads the x0 history) against tests/sched_ref.py's loop on the fp32 route and against the channel-major route
in bf16, at test_gpu_schedulers.py's tolerances."""
import pytest
import torch

from said_amd.scheduler import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler
from said_amd.util import synth

import sched_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

B, T, C, N, GS, LS = 2, 33, 32, 3, 2.0, 0.7
SEED = 0x5A1D0123456789
COUNTERS = ("n_out_sched", "n_sched_step", "n_out_sched_tm")
# route -> (mfma dtype, guidance_rescale, debug options while it runs, the counter that must grow)
ROUTES = {
    "fused_fp32": ("fp32", 0.0, {}, "n_out_sched"),
    "unfused_rescale": ("fp32", 0.7, {}, "n_sched_step"),
    "token_major_bf16": ("bf16", 0.0, {"unet_tgemm_min_tokens": 0}, "n_out_sched_tm"),   # (the token-major schedule forced at 66 tokens)
}


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


@pytest.fixture(scope="module")
def data():
    """The loop's inputs (CPU, never modified).  The mask is 1 on tokens 28..35 — across the tile boundary at token 32 — of channels 3..6."""
    mask = torch.zeros(B, T, C)
    mask[:, 28:, 3:7] = 1.0
    return dict(lat=synth.synth_latents(810, (B, T, C)), emb=synth.synth_latents(811, (B, T, 768)),
                init=torch.sigmoid(synth.synth_latents(812, (B, T, C))) * 0.5, en=synth.synth_latents(813, (B, T, C)), mask=mask)


def _table(kind, pred="epsilon"):
    s = {"ddim": DDIMScheduler, "ddpm": DDPMScheduler, "dpm": DPMSolverMultistepScheduler}[kind](prediction_type=pred)
    s.set_timesteps(N)
    ts = s.timesteps.numpy()
    return ts, (s.coef_table(ts, 1.0) if kind == "ddim" else s.coef_table(ts))   # DDIM: eta = 1


class _Route:
    """The model's engine set up for one route; precision and debug options restored on exit."""

    def __init__(self, model, route):
        self.model, (self.dtype, self.rescale, self.opts, self.counter) = model, ROUTES[route]

    def __enter__(self):
        self.model.set_mfma_dtype(self.dtype)
        self.eng = self.model._get_engine(2 * B, T)
        for k, v in self.opts.items():
            self.eng.debug_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.opts:
            self.eng.debug_option(k, -1)
        self.eng.debug_option("out_tm", -1)
        self.model.set_mfma_dtype("fp32")

    def loop(self, data, dev, ts, coef, pred="epsilon", masked=False, latent_scale=LS, **noise):
        """One loop; returns (result, final latents, intermediates) on the CPU after asserting that this route's kernel, and no other, ran."""
        kw = dict(init_latents=data["init"].to(dev), edit_noise=data["en"].to(dev), mask=data["mask"].to(dev)) if masked else {}
        self.eng.debug_option("out_tm", self.opts.get("out_tm", -1))   # (drops the cached step graph: this loop captures and counts its own)
        c0 = {k: self.eng.debug_get(k) for k in COUNTERS}
        out = self.eng.denoise_loop(latents=data["lat"].to(dev), context=data["emb"].to(dev), timesteps=ts, coef=coef, prediction_type=pred,
                                    guidance_scale=GS, guidance_rescale=self.rescale, latent_scale=latent_scale, save_intermediate=True, **kw, **noise)
        grew = {k for k in COUNTERS if self.eng.debug_get(k) > c0[k]}
        assert grew == {self.counter}, grew
        return tuple(t.cpu() for t in out)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_update_noise_mask_and_intermediates_bit_exact(model, dev, data, route, kind, masked):
    ts, coef = _table(kind)
    with _Route(model, route) as r:
        seeded = r.loop(data, dev, ts, coef, masked=masked, noise_seed=SEED)
        sn = r.eng.philox_normal(SEED, 0, N, (B, T, C))
        fed = r.loop(data, dev, ts, coef, masked=masked, step_noise=sn)
        zeros = r.loop(data, dev, ts, coef, masked=masked, step_noise=torch.zeros_like(sn))
    for a, b in zip(seeded, fed):   # result, final latents, intermediates
        assert torch.equal(a, b)
    assert not torch.equal(seeded[1], zeros[1])   # the noise is there at all
    assert torch.equal(seeded[2][0], data["lat"] / torch.full_like(data["lat"], LS))   # the pre-step latents of step 0 are the input
    if masked:   # add_noise(init, edit_noise) of the last row: separately rounded multiply, multiply, add
        cf = torch.from_numpy(coef[-1])
        want = cf[5] * data["init"] + cf[6] * data["en"]
        m = data["mask"] == 1
        assert torch.equal(seeded[1][m], want[m])


def test_dpm_second_order_row_fused_fp32_vs_oracle(model, sd_full, dev, data):
    """out_sched_kernel<CFG, SP, 1> against the oracle UNet driven by the CPU restatement of DPM-Solver++ (v_prediction: see test_gpu_schedulers.py)."""
    ts, coef = _table("dpm", "v_prediction")
    assert [int(v) for v in coef[:, 7]] == [2, 3, 2]
    with _Route(model, "fused_fp32") as r:
        got = r.loop(data, dev, ts, coef, pred="v_prediction", latent_scale=1.0)[0]
    ref, _ = sched_ref.inference(sd_full, torch.zeros(B, T * 16000 // 60), "dpmsolver++", init_latents=data["lat"], num_inference_steps=N, guidance_scale=GS,
                                 prediction_type="v_prediction", audio_embedding=data["emb"])
    err = float((got - ref).abs().max())
    print(f"dpmsolver++ N={N} B={B} T={T}, fused fp32 route: max abs err vs oracle {err:.3e}")
    assert err <= 1e-3, err


def test_dpm_second_order_row_token_major_bf16_vs_channel_major(model, dev, data):
    """out_sched_tm_kernel<CFG, 1> against the same bf16 loop on the channel-major route (out_sched_kernel), test_gpu_schedulers.py's bf16 bound;
    masked elements identical."""
    ts, coef = _table("dpm", "v_prediction")
    res = {}
    for ot, counter in ((1, "n_out_sched_tm"), (0, "n_out_sched")):
        with _Route(model, "token_major_bf16") as r:
            r.opts, r.counter = dict(r.opts, out_tm=ot), counter
            r.eng.debug_option("out_tm", ot)
            res[ot] = r.loop(data, dev, ts, coef, pred="v_prediction", masked=True, latent_scale=1.0)[0]
    d = float((res[0] - res[1]).abs().max())
    print(f"dpmsolver++ N={N} B={B} T={T}, bf16: token-major vs channel-major last kernel, max |diff| {d:.3e}")
    assert torch.isfinite(res[1]).all() and d <= 0.087
    m = data["mask"] == 1
    assert torch.equal(res[1][m], res[0][m])
