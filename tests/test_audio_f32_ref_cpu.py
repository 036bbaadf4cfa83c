"""tests/audio_f32_ref.py without a GPU: the per-launch restatement of the fp32 audio encoder is the oracle, and it sees the defects it is there for.

1. The launches chained in float64 — every intermediate stored in the kernel's padded layouts, the pad rows filled with large finite values that must
   not matter — equal oracle/wav2vec2.py run in float64 to rounding (1e-12 of range asked, about 1e-14 seen): with and without interpolation, with
   audio_proj_layer, and for the features-only result; with one and with eight key slices.
2. Eleven wrong variants of single launches (the dropped K block on two of them), each on CPU-made data of the GPU module's shape S, each measured with that module's rule
   max |got - ref64| / max |ref64| <= 4 max(e32, 1e-6): every one is at least 50 x beyond the bound (the factors are printed).
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import audio_f32_ref as R  # noqa: E402
from oracle import wav2vec2 as O  # noqa: E402
from said_amd.util import synth  # noqa: E402

torch.set_grad_enabled(False)
F64, F32 = torch.float64, torch.float32
FD = 64


@pytest.fixture(scope="module")
def full_sd():
    sd = synth.said_state_dict(num_w2v_layers=1)
    sd["audio_proj_layer.weight"] = synth.fill_tensor("audio_proj_layer.weight", (FD, 768))
    sd["audio_proj_layer.bias"] = synth.fill_tensor("audio_proj_layer.bias", (FD,))
    return sd


@pytest.fixture(scope="module")
def sd(full_sd):
    return R.audio_sd(full_sd)


def _wav(B, Ta, seed):
    w = torch.stack([synth.synth_waveform(seed + i, Ta) for i in range(B)])
    return (w - w.mean(1, keepdim=True)) / torch.sqrt(w.var(1, unbiased=False, keepdim=True) + 1e-7)


class _Float64Input(torch.Tensor):
    """wav2vec2_forward begins with input_values.float(); this input stays what it is, so that the oracle's own code runs in float64."""
    def float(self):
        return self.as_subclass(torch.Tensor)


def _junk(*shape):
    """What a pad row may hold: large, finite, different everywhere."""
    g = torch.Generator().manual_seed(sum(shape))
    return torch.randn(*shape, generator=g, dtype=F64) * 1.0e3


# ---------------------------------------------------------------------------------------------------------------- the tie to the oracle
@pytest.mark.parametrize("frames", [59, None])
def test_chained_launches_are_the_oracle_in_float64(sd, full_sd, frames):
    wav = _wav(2, 4000, 900)
    sd64 = {k: v.double() for k, v in sd.items()}
    want, feats = O.wav2vec2_forward(sd64, wav.double().as_subclass(_Float64Input), frames)
    assert want.dtype == F64 and feats.dtype == F64
    scale = float(want.abs().max())
    for ks in (1, 8):
        got = R.encode(sd64, wav, frames, F64, ks=ks, fill=_junk)
        e = float((got - want).abs().max()) / scale
        print(f"frames {frames}, {ks} key slices: chained launches vs oracle in float64: {e:.2e} of range")
        assert got.shape == want.shape and e <= 1e-12
    W, b = full_sd["audio_proj_layer.weight"].double(), full_sd["audio_proj_layer.bias"].double()
    got = R.encode(sd64, wav, frames, F64, proj_wb=(W, b), fill=_junk)
    wantp = F.linear(want, W, b)
    e = float((got - wantp).abs().max()) / float(wantp.abs().max())
    print(f"frames {frames}: with audio_proj_layer: {e:.2e} of range")
    assert got.shape == wantp.shape and e <= 1e-12
    got = R.encode(sd64, wav, frames, F64, features_only=True, fill=_junk)
    wantf = (feats if frames is None else F.interpolate(feats, size=frames, align_corners=True, mode="linear")).transpose(1, 2)
    e = float((got - wantf).abs().max()) / float(wantf.abs().max())
    print(f"frames {frames}: features only: {e:.2e} of range")
    assert got.shape == wantf.shape and e <= 1e-12


def test_kernel_formed_interpolation_weights_and_host_folded_weight_norm_stay_at_fp32_distance(sd):
    """The two places where the GPU module's reference follows the engine instead of the oracle: interpolation weights formed in fp32
    (interp_linear_kernel) and weight_norm folded in fp32 on the host.  Both sit at fp32 rounding distance from the exact ones."""
    x = R.padded(torch.randn(2, 512, 12, generator=torch.Generator().manual_seed(5), dtype=F64))
    a, b = R.interp_linear(x, 12, 599, F64, True), R.interp_linear(x, 12, 599, F64, False)
    e = R.rel_max(a, b)
    print(f"interpolation 12 -> 599, fp32-formed weights vs exact: {e:.2e} of range")
    assert 0 < e <= 1e-6
    w32, w64 = R.pos_weight(sd, F64, True), R.pos_weight(sd, F64, False)
    e = R.rel_max(w32, w64)
    print(f"positional weight, folded in fp32 vs float64: {e:.2e} of range")
    assert 0 < e <= 2e-7


def test_sliced_attention_is_the_plain_softmax():
    g = torch.Generator().manual_seed(11)
    qk, vt = torch.randn(2, 24, 96, 64, generator=g, dtype=F64), torch.randn(2, 768, 96, generator=g, dtype=F64)
    want = R.attention_plain(qk, vt, 75)
    for ks in (1, 4, 8):
        assert R.rel_max(R.attention(qk, vt, 75, ks), want) <= 1e-13


# ---------------------------------------------------------------------------------------------------------------- the mutants
@pytest.fixture(scope="module")
def stored(sd):
    """CPU-made intermediates of shape S (3 clips x 16000 samples, 59 frames) in fp32, as an engine would hold them; the pad rows hold values of the
    data's own size (what an earlier, larger encode leaves)."""
    sh = R.SHAPES["S"]
    wav = _wav(sh["B"], sh["Ta"], 810)
    L = R.conv_lengths(sh["Ta"])
    T = sh["frames"]

    def stale(x):
        sc = float(x.abs().mean())
        return lambda *s: torch.randn(*s, generator=torch.Generator().manual_seed(len(s) + s[-1]), dtype=F32) * sc

    def pad(x):
        return R.padded(x.float(), stale(x))
    s = {"L": L, "T": T}
    s["c0raw"] = pad(R.conv0(sd, wav, F32))
    s["c0"] = pad(R.rownorm_gelu(sd, s["c0raw"], L[0], F32))
    x = s["c0"]
    for i in range(1, 7):
        x = s[f"c{i}"] = pad(R.conv(sd, i, x, L[i - 1], F32))
    s["x"] = pad(R.interp_linear(x, L[6], T, F32))
    s["hproj"] = pad(R.fproj(sd, s["x"], T, F32))
    s["pos"] = pad(R.posconv(sd, s["hproj"], T, F32))
    s["h0"] = pad(R.layernorm(sd, "encoder.layer_norm", s["hproj"], s["pos"], T, F32))
    qk, v = R.qkv(sd, 0, s["h0"], T, F32)
    s["qk"] = pad(qk.transpose(2, 3)).transpose(2, 3).contiguous()
    s["v"] = pad(v)
    s["o"] = pad(R.attention(s["qk"], s["v"], T, 8, F32))
    s["t1"] = pad(R.out_proj(sd, 0, s["o"], s["h0"], T, F32))
    s["h1"] = pad(R.layernorm(sd, "encoder.layers.0.layer_norm", s["t1"], None, T, F32))
    s["f"] = pad(R.ff1(sd, 0, s["h1"], T, F32))
    return s


def _mutants(sd, s):
    """name -> (the launch as a function of (dtype, defect))."""
    L, T = s["L"], s["T"]
    return {
        "a dropped last K block of one workgroup (out_proj)": (lambda dt, d: R.out_proj(sd, 0, s["o"], s["h0"], T, dt, d), "k_block"),
        "a dropped last K block of one workgroup (ff2, K = 3072)": (lambda dt, d: R.ff2(sd, 0, s["f"], s["h1"], T, dt, d), "k_block"),
        "a convolution tap shifted by one (conv2)": (lambda dt, d: R.conv(sd, 2, s["c1"], L[1], dt, d), "tap_shift"),
        "the stride-2 row start off by one (conv6)": (lambda dt, d: R.conv(sd, 6, s["c5"], L[5], dt, d), "row_start"),
        "normalisation statistics over the pitch instead of the frames": (lambda dt, d: R.rownorm_gelu(sd, s["c0raw"], L[0], dt, d), "stats_over_pitch"),
        "interpolation with align_corners flipped": (lambda dt, d: R.interp_linear(s["c6"], L[6], T, dt, defect=d), "align_corners"),
        "the positional convolution keeping the dropped last output": (lambda dt, d: R.posconv(sd, s["hproj"], T, dt, defect=d), "keep_last"),
        "a group reading its neighbour's channels": (lambda dt, d: R.posconv(sd, s["hproj"], T, dt, defect=d), "group_neighbour"),
        "the last key tile unmasked": (lambda dt, d: R.attention(s["qk"], s["v"], T, 8, dt, d), "unmasked"),
        "one key slice dropped": (lambda dt, d: R.attention(s["qk"], s["v"], T, 8, dt, d), "slice_dropped"),
        "the residual row of the neighbouring token": (lambda dt, d: R.out_proj(sd, 0, s["o"], s["h0"], T, dt, d), "res_neighbour"),
        "V read from row t + pitch": (lambda dt, d: R.attention(s["qk"], s["v"], T, 8, dt, d), "v_row"),
    }


def test_every_named_defect_fails_the_gpu_rule_by_a_wide_margin(sd, stored):
    worst = None
    for name, (fn, defect) in _mutants(sd, stored).items():
        ref64, ref32 = fn(F64, None), fn(F32, None)
        e32, bound = R.f32_bound(ref32, ref64)
        factor = R.rel_max(fn(F32, defect), ref64) / bound
        print(f"{name}: {factor:.0f} x the bound {bound:.1e} (fp32 CPU evaluation {e32:.1e})")
        assert e32 <= 1e-6, (name, e32)
        assert factor >= 50, (name, factor)
        worst = factor if worst is None else min(worst, factor)
    print(f"smallest factor: {worst:.0f}")
