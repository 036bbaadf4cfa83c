"""BCVAE decoder on the MI355X (said_vae_decode: one fused launch, vae_dec.hip) against golden G11 — the reference's own
BCVAE in eval mode — and the float64 restatement of test_vae_decoder_cpu.py.  Tolerance: 2e-6 x max(1, rms(latent)) absolute
against the restatement (test_vae_decoder_cpu.row_scale), 4e-6 x that against G11 (two fp32 summation orders)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from said_amd import _engine
from said_amd.util import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_vae_decoder_cpu import decoder_f64, row_scale  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
TOL = 2e-6


def _model(sd=None):
    from said_amd.model.vae import BCVAE
    m = BCVAE()
    m.load_state_dict(synth.vae_state_dict() if sd is None else sd, strict=True)
    return m.to(DEV).eval()


def _coeffs(n):
    return torch.sigmoid(synth.synth_latents(1102, (32, 120, 32)))[:n]   # make_golden_g11.g11_coeffs


def _err(got, ref, lat):
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / row_scale(lat)).max())


def test_decode_vs_golden_and_f64(golden):
    g = golden("g11_vae_decoder")
    m = _model()
    assert m._get_engine().has_decoder
    lat = g["dec_latent"]
    got = m.decode(torch.from_numpy(lat).to(DEV)).cpu().numpy()
    assert got.shape == (64, 120, 32)
    e64 = _err(got, decoder_f64(synth.vae_state_dict())(lat).numpy(), lat)
    eg = _err(got, g["dec_coeffs"], lat)
    print(f"vae decode: scaled max err {e64:.2e} vs float64, {eg:.2e} vs G11; raw max {np.abs(got - g['dec_coeffs']).max():.2e}")
    assert e64 <= TOL and eg <= 2 * TOL
    assert (got == 0).any() and (got > 0.999).any() and got.max() <= 1.0
    assert any("libsaid_hip.so" in ln for ln in open("/proc/self/maps"))


def test_forward_without_noise_vs_golden(golden):
    g = golden("g11_vae_decoder")
    out = _model()(_coeffs(32).to(DEV), False)
    for f in ("mean", "log_var", "latent"):
        ref = g["fwd_" + f]
        assert np.abs(getattr(out, f).cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max(), f   # the encoder's G10 tolerance
    assert torch.equal(out.latent, out.mean)
    lat = out.latent.cpu().numpy()
    got = out.coeffs_reconst.cpu().numpy()
    e64, eg = _err(got, decoder_f64(synth.vae_state_dict())(lat).numpy(), lat), _err(got, g["fwd_coeffs_reconst"], lat)
    print(f"vae forward(use_noise=False): {e64:.2e} vs float64 of its own latent, {eg:.2e} vs G11")
    assert e64 <= TOL
    assert eg <= 1e-4   # G11's latent is the reference encoder's; ours differs within the encoder tolerance


def test_forward_with_noise_is_the_reference_draw(golden):
    g = golden("g11_vae_decoder")
    m = _model()
    coeffs = _coeffs(8).to(DEV)
    torch.manual_seed(int(g["noise_seed"]))
    out = m(coeffs, True)
    eps = torch.from_numpy(g["noise_eps"]).to(DEV)
    assert torch.equal(out.latent, out.mean + torch.exp(0.5 * out.log_var) * eps), "the noise is G11(c)'s, drawn as the reference draws it"
    assert np.abs(out.latent.cpu().numpy() - g["noise_latent"]).max() <= 1e-4 * np.abs(g["noise_latent"]).max()
    lat = out.latent.cpu().numpy()
    e64 = _err(out.coeffs_reconst.cpu().numpy(), decoder_f64(synth.vae_state_dict())(lat).numpy(), lat)
    print(f"vae forward(use_noise=True): {e64:.2e} vs float64 (fused reparametrisation)")
    assert e64 <= TOL
    again = m(coeffs, True, eps=eps)
    assert torch.equal(again.coeffs_reconst, out.coeffs_reconst) and torch.equal(again.latent, out.latent)
    # the standalone path: reparametrize + decode
    torch.manual_seed(int(g["noise_seed"]))
    z = m.reparametrize(out.mean, out.log_var)
    assert torch.equal(z, out.latent)
    assert float((m.decode(z) - out.coeffs_reconst).abs().max()) <= 1e-6


def test_decode_chunking_and_edge_cases():
    m = _model()
    eng = m._get_engine()
    g = torch.Generator()
    g.manual_seed(77)
    n_big = 16384 + 3   # one more launch than vae.cpp's 16384-window chunk
    z = torch.randn(n_big, 64, generator=g).to(DEV)
    big = m.decode(z)
    assert big.shape == (n_big, 120, 32)
    for n in (1, 4097):
        part = m.decode(z[:n])
        assert torch.equal(part, big[:n]), n
    for r in (0, 1, 4096, 16383, 16384, n_big - 1):
        assert torch.equal(m.decode(z[r:r + 1]), big[r:r + 1]), r
    # fused reparametrisation across the chunk boundary
    lv = 0.1 * torch.randn(n_big, 64, generator=g).to(DEV)
    e = torch.randn(n_big, 64, generator=g).to(DEV)
    fused = eng.decode(z, lv, e)
    for r in (0, 16384, n_big - 1):
        assert float((fused[r] - eng.decode(z[r:r + 1], lv[r:r + 1], e[r:r + 1])[0]).abs().max()) == 0.0
    empty = m.decode(torch.empty(0, 64, device=DEV))
    assert empty.shape == (0, 120, 32)
    zt = z[:64].t().contiguous().t()   # non-contiguous view of the same values
    assert not zt.is_contiguous()
    assert torch.equal(m.decode(zt), big[:64])
    assert torch.equal(m.decode(z[:128:2]), m.decode(z[:128:2].contiguous()))


def test_encode_unchanged_by_decoder_weights():
    """An engine loaded with the full 70-tensor dict encodes bit-identically to one loaded with the encoder half only."""
    coeffs = torch.sigmoid(synth.synth_latents(41, (5, 120, 32))).to(DEV)
    seq = torch.sigmoid(synth.synth_latents(42, (300, 32))).to(DEV)
    outs = []
    for sd in (synth.vae_encoder_state_dict(), synth.vae_state_dict()):
        e = _engine.VaeEngine(DEV)
        e.load_weights(sd)
        outs.append(e.encode(coeffs, 5, 120 * 32) + e.encode(seq, 181, 32, want_logvar=False)[:1])
        e.close()
    assert not any(t.isnan().any() for t in outs[0])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_decoder_error_paths():
    enc = synth.vae_encoder_state_dict()
    e = _engine.VaeEngine(DEV)
    e.load_weights(enc)
    assert not e.has_decoder
    with pytest.raises(_engine.EngineError, match="decoder"):
        e.decode(torch.zeros(2, 64, device=DEV))
    e.close()
    sd = synth.vae_state_dict()
    partial = {k: v for k, v in sd.items() if k != "decoder.conv_layers.7.bias"}
    e = _engine.VaeEngine(DEV)
    with pytest.raises(_engine.EngineError, match="partial decoder"):
        e.load_weights(partial)
    e.close()
    bad = dict(sd)
    bad["decoder.fc_layers.3.weight"] = torch.zeros(480, 239)
    e = _engine.VaeEngine(DEV)
    with pytest.raises(_engine.EngineError, match="size mismatch"):
        e.load_weights(bad)
    e.close()
    m = _model()
    for shape in ((2, 63), (64,), (2, 64, 1)):
        with pytest.raises(ValueError):
            m.decode(torch.zeros(*shape, device=DEV))
    with pytest.raises(_engine.EngineError):
        m.decode(torch.zeros(2, 64, device=DEV, dtype=torch.float64))
    m.train()
    with pytest.raises(_engine.EngineError):
        m.decode(torch.zeros(1, 64, device=DEV))


def test_inference_vae_cli_end_to_end(tmp_path):
    from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, save_blendshape_coeffs
    sd = synth.vae_state_dict()
    wpath = tmp_path / "vae.pt"
    torch.save(sd, wpath)
    seq = torch.sigmoid(synth.synth_latents(1103, (150, 32))).numpy()
    src, dst, img = tmp_path / "in.csv", tmp_path / "out.csv", tmp_path / "out.png"
    save_blendshape_coeffs(coeffs=seq, classes=DEFAULT_BLENDSHAPE_CLASSES, output_path=str(src))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "script", "inference_vae.py"), "--weights_path", str(wpath),
                        "--blendshape_coeffs_path", str(src), "--output_path", str(dst), "--output_image_path", str(img),
                        "--save_image", "1", "--use_noise", "", "--device", "cuda:0"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    import pandas as pd
    table = pd.read_csv(dst)
    assert list(table.columns) == list(DEFAULT_BLENDSHAPE_CLASSES) and table.shape == (120, 32)
    assert img.exists()
    lat = _model().encode(torch.from_numpy(seq[None, :120]).to(DEV)).mean.cpu().numpy()
    ref = decoder_f64(sd)(lat).numpy()[0]
    assert np.abs(table.values - ref).max() <= 2 * TOL   # the CSV's text round trip adds ~1e-8
