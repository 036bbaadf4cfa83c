"""BCVAE decoder (said/model/vae.py:115-170), CPU side: the synthetic full state dict, a float64 restatement of the decoder
pinned to golden G11 (the reference's own BCVAE), the ConvTranspose1d -> flipped Conv1d rewrite the host packing uses
(vae.cpp load_vae_decoder), and the reconstruction CLI's flags.  The GPU tests (test_gpu_vae_decoder.py) compare the
engine against the same restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn

from said_amd.util import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# model/vae.pth's key set (said/model/vae.py:26-64, 135-156): what a strict load into the reference's BCVAE expects
REFERENCE_VAE_KEYS = set(synth.vae_encoder_param_shapes()) | set(synth.vae_decoder_param_shapes()) | {
    p + ".num_batches_tracked" for p in ("encoder.conv_layers.1", "encoder.conv_layers.4", "encoder.conv_layers.7", "encoder.fc_layers.1",
                                         "encoder.fc_layers.4", "decoder.fc_layers.1", "decoder.conv_layers.1", "decoder.conv_layers.4")}


def _bn(sd, pre, n):
    m = nn.BatchNorm1d(n).double().eval()
    for leaf in ("weight", "bias", "running_mean", "running_var"):
        getattr(m, leaf).data.copy_(sd[f"{pre}.{leaf}"].double())
    return m


def _affine(m, sd, pre):
    m = m.double().eval()
    m.weight.data.copy_(sd[pre + ".weight"].double())
    m.bias.data.copy_(sd[pre + ".bias"].double())
    return m


def decoder_f64(sd):
    """BCDecoder.forward (vae.py:135-170) in float64, eval mode, from plain torch modules: (B, 64) -> (B, 120, 32)."""
    D = "decoder."
    fc = nn.Sequential(_affine(nn.Linear(64, 240), sd, D + "fc_layers.0"), _bn(sd, D + "fc_layers.1", 240), nn.LeakyReLU(),
                       _affine(nn.Linear(240, 480), sd, D + "fc_layers.3"), nn.Unflatten(1, (4, 120)))
    conv = nn.Sequential(_affine(nn.ConvTranspose1d(4, 32, 3), sd, D + "conv_layers.0"), _bn(sd, D + "conv_layers.1", 32), nn.LeakyReLU(0.2),
                         _affine(nn.ConvTranspose1d(32, 32, 3), sd, D + "conv_layers.3"), _bn(sd, D + "conv_layers.4", 32), nn.LeakyReLU(0.2),
                         _affine(nn.Conv1d(32, 32, 3), sd, D + "conv_layers.6"), _affine(nn.Conv1d(32, 32, 3), sd, D + "conv_layers.7"),
                         nn.ReLU(), nn.Tanh())

    def run(latent):
        with torch.no_grad():
            return conv(fc(torch.as_tensor(latent).double())).transpose(1, 2)
    return run


def row_scale(latent):
    """(B, 1, 1) max(1, rms(z)) per row.  Every layer ahead of the final ReLU/tanh is piecewise linear in z, so activations -- and
    the fp32 rounding error of any summation order -- grow linearly with the latent's magnitude: tolerances are 2e-6 x this
    (the reference's own fp32 result sits within 1.1e-6 x this of the float64 restatement on G11)."""
    z = np.asarray(latent, dtype=np.float64)
    return np.maximum(1.0, np.sqrt((z * z).mean(1)))[:, None, None]


def test_vae_state_dict_is_the_reference_layout():
    sd = synth.vae_state_dict()
    assert len(sd) == 70 and set(sd) == REFERENCE_VAE_KEYS
    enc = synth.vae_encoder_state_dict()
    for k, v in enc.items():
        assert torch.equal(sd[k], v), k
    assert set(synth.vae_decoder_param_shapes()) == {k for k in REFERENCE_VAE_KEYS if k.startswith("decoder.") and "num_batches" not in k}
    assert torch.equal(synth.vae_state_dict()["decoder.fc_layers.3.weight"], sd["decoder.fc_layers.3.weight"])   # deterministic
    from said_amd.model.vae import BCVAE
    m = BCVAE()
    m.load_state_dict(sd, strict=True)
    assert set(m.state_dict()) == REFERENCE_VAE_KEYS
    for k, v in sd.items():
        assert tuple(m.state_dict()[k].shape) == tuple(v.shape), k
    rv = sd["decoder.conv_layers.1.running_var"]
    assert float(rv.min()) < 0.5 and float(rv.max()) > 1.5   # BatchNorm statistics far from identity: the host folding matters


def test_f64_restatement_reproduces_g11(golden):
    """Pins the restatement the GPU tests use to the reference's own BCVAE (G11, fp32 on the CPU)."""
    g = golden("g11_vae_decoder")
    dec = decoder_f64(synth.vae_state_dict())
    for lat, ref in ((g["dec_latent"], g["dec_coeffs"]), (g["fwd_latent"], g["fwd_coeffs_reconst"]), (g["noise_latent"], g["noise_coeffs_reconst"])):
        got = dec(lat).numpy()
        assert got.shape == ref.shape
        assert (np.abs(got - ref) / row_scale(lat)).max() <= 2e-6
    d = g["dec_coeffs"]
    assert (d == 0).any() and (d > 0.999).any(), "G11(a) covers both the ReLU-clipped and the tanh-saturated regions"
    torch.manual_seed(int(g["noise_seed"]))
    assert np.array_equal(torch.randn(8, 64).numpy(), g["noise_eps"]), "G11(c)'s noise is torch.randn(B, 64) on the CPU generator"


def _conv_transpose_as_flipped_conv(x, w):
    """numpy restatement of the host rewrite: stride-1 ConvTranspose1d, weight (cin, cout, k), as a valid Conv1d with weight
    w'[co][ci][j] = w[ci][co][k-1-j] over x zero-padded by k-1 on each side."""
    B, cin, L = x.shape
    k = w.shape[2]
    wc = np.ascontiguousarray(np.transpose(w, (1, 0, 2))[:, :, ::-1])
    xp = np.pad(x, ((0, 0), (0, 0), (k - 1, k - 1)))
    Lo = L + k - 1
    y = np.zeros((B, w.shape[1], Lo))
    for j in range(k):
        y += np.einsum("oc,bct->bot", wc[:, :, j], xp[:, :, j:j + Lo])
    return y


@pytest.mark.parametrize("cin,cout,k,L", [(4, 32, 3, 120), (32, 32, 3, 122), (3, 5, 4, 7)])
def test_conv_transpose_rewrite_matches_torch(cin, cout, k, L):
    g = torch.Generator()
    g.manual_seed(cin * 1000 + cout * 10 + k)
    x = torch.randn(2, cin, L, generator=g, dtype=torch.float64)
    w = torch.randn(cin, cout, k, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.conv_transpose1d(x, w).numpy()
    got = _conv_transpose_as_flipped_conv(x.numpy(), w.numpy())
    assert got.shape == ref.shape == (2, cout, L + k - 1)
    assert np.abs(got - ref).max() <= 1e-12


def test_inference_vae_help_lists_the_reference_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "script", "inference_vae.py"), "--help"], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    for flag in ("--weights_path", "--blendshape_coeffs_path", "--output_path", "--output_image_path", "--save_image", "--use_noise", "--device"):
        assert flag in r.stdout, flag
