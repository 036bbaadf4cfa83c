"""said_clone from a parent that has already been used: the clone shares the parent's weights and switches and nothing else.

A used parent holds grown audio buffers, a grown step-noise buffer, a cached step graph and debug state.  A clone made then must start
without any of it (its own buffers grow on its own stream), compute exactly what the parent computes, and leave the parent as it was."""
import pytest
import torch

from said_amd import _engine
from said_amd.scheduler import DDIMScheduler
from said_amd.util import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

B, T, N = 1, 40, 2          # one clip under guidance: a launch of two samples, the small-batch schedule of either mode
CLIPS, TA = 2, 16000        # two one-second clips


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def parent(dev, unet_sd, w2v_sd):
    sd = {"null_cond_emb": synth.fill_tensor("null_cond_emb", (1, 1, 768))}
    sd.update({"audio_encoder." + k: v for k, v in w2v_sd.items()})
    sd.update({"denoiser." + k: v for k, v in unet_sd.items()})
    eng = _engine.Engine(dev, 2 * B, 64)
    eng.load_weights(sd)
    yield eng
    eng.close()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_clone_of_used_parent_starts_clean_and_computes_the_same(parent, dev, mode):
    """Same schedule at the same launch size on another context: bit-identical in both modes, as a rerun on one context is."""
    wav = torch.stack([synth.synth_waveform(900 + i, TA) for i in range(CLIPS)]).to(dev)
    sch = DDIMScheduler()
    sch.set_timesteps(N)
    ts = sch.timesteps.numpy()
    parent.set_precision(mode)
    try:
        # ---- use the parent: audio buffers grow, the step-noise buffer grows, a step graph is cached, the debug state is touched
        audio_p = parent.audio_encode(wav, T)
        kw = dict(latents=synth.synth_latents(901, (B, T, 32)).to(dev), context=audio_p[:B].contiguous(), timesteps=ts, coef=sch.coef_table(ts, 1.0),
                  prediction_type="epsilon", guidance_scale=2.0, guidance_rescale=0.0, latent_scale=1.0,
                  step_noise=synth.synth_latents(902, (N, B, T, 32)).to(dev), save_intermediate=True)
        res_p, lat_p, inter_p = parent.denoise_loop(**kw)
        assert parent.graph_num_nodes() > 0
        parent.debug_stop_after(3)
        parent.debug_stop_after(-1)
        torch.cuda.synchronize()

        clone = parent.clone(2 * B, 64)
        try:
            assert clone.graph_num_nodes() == 0
            with torch.cuda.stream(clone.stream):
                res_c, lat_c, inter_c = clone.denoise_loop(**kw)
                audio_c = clone.audio_encode(wav, T)
            clone.stream.synchronize()
            assert clone.graph_num_nodes() == parent.graph_num_nodes()
            assert bool(torch.isfinite(res_p).all()) and float(res_p.abs().max()) > 0
            assert torch.equal(res_c, res_p) and torch.equal(lat_c, lat_p) and torch.equal(inter_c, inter_p)
            assert torch.equal(audio_c, audio_p)
            # the clone touched nothing of the parent
            res_2, lat_2, inter_2 = parent.denoise_loop(**kw)
            assert torch.equal(res_2, res_p) and torch.equal(lat_2, lat_p) and torch.equal(inter_2, inter_p)
            assert torch.equal(parent.audio_encode(wav, T), audio_p)
            torch.cuda.synchronize()
        finally:
            clone.close()
            parent._clones.remove(clone)
    finally:
        parent.set_precision("fp32")
