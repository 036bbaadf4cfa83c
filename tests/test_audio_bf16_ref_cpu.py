"""tests/audio_bf16_ref.py (the stage-by-stage restatement the bf16 audio-encoder kernels are compared with: tests/test_gpu_audio_bf16_kernels.py)
tied to the oracle that golden G5 pins, and the sharpness of its bounds — CPU only."""
import pytest
import torch

import audio_bf16_ref as R
from oracle import wav2vec2 as ow
from said_amd.util import synth

torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def sd():
    return R.audio_sd(synth.said_state_dict(num_w2v_layers=2))


def _wav(B, Ta, seed):
    w = torch.stack([synth.synth_waveform(seed + i, Ta) for i in range(B)])
    return (w - w.mean(1, keepdim=True)) / torch.sqrt(w.var(1, unbiased=False, keepdim=True) + 1e-7)


@pytest.mark.parametrize("B,Ta,frames", [(1, 16000, 60), (2, 4000, 75)])
def test_unrounded_stage_chain_is_the_oracle(sd, B, Ta, frames):
    """Chained with rounded=False the stage functions ARE wav2vec2_forward.  The oracle runs in fp32, so the yardstick is the chain's own fp32 run (dtype=float32):
    two fp32 evaluations of one function, each compared with the float64 one — the oracle may be 4 x as far as the chain's (another summation order), floor 1e-6."""
    wav = _wav(B, Ta, 40)
    want = ow.wav2vec2_forward(sd, wav, frames)[0]
    ref64 = R.encode(sd, wav, frames, rounded=False, dtype=torch.float64)
    ref32 = R.encode(sd, wav, frames, rounded=False, dtype=torch.float32)
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32 and ref64.shape == want.shape == (B, frames, 768)
    e, bound = R.check_f32(f"oracle vs unrounded chain B={B} Ta={Ta} frames={frames}", want, ref64, ref32)
    assert e > 0   # (an fp32 result that equals the float64 one bit for bit would mean the chain did not run in float64)


def test_rounded_chain_sits_at_bf16_distance_and_key_slices_agree(sd):
    """The rounded chain differs from the unrounded one by bf16 operand rounding (1e-3 .. 5e-2 of range: DESIGN 7.2's end-to-end bound is 4.8e-2 max abs on values up to
    3.8), and the key-split restatement of the online softmax (eight slices) is the same function as the one-slice form up to the rounding of p: the two differ by a
    fraction of the rounding noise, but by more than the tenth of it that the GPU test allows a kernel — which is why the reference restates the kernel's slicing."""
    wav = _wav(1, 16000, 43)
    u = R.encode(sd, wav, 60, rounded=False)
    r1 = R.encode(sd, wav, 60, rounded=True, ks=1)
    e = R.rel_max(r1, u)
    print(f"rounded vs unrounded chain: {e:.2e} of max |ref|")
    assert 1e-4 < e < 5e-2
    x = R.conv0(sd, wav)
    for i in range(1, 7):
        x = R.conv(sd, i, x)
    h = R.fproj(sd, R.interp_ln(sd, x, 60))
    _, hb = R.ln(sd, "encoder.layer_norm", R.posconv(sd, R.tm_to_group(h), h))
    qk, vt = R.qkv(sd, 0, hb)
    a1, a8, au = R.attention(qk, vt, 1), R.attention(qk, vt, 8), R.attention(qk, vt, rounded=False)
    noise = float((au - a1).pow(2).mean().sqrt())
    d = float((a8 - a1).pow(2).mean().sqrt())
    print(f"attention: rms(unrounded - rounded) {noise:.2e}, rms(eight slices - one slice) {d:.2e}")
    assert 0 < d < noise


def test_layouts_and_roundings():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -(1.0 + 2.0 ** -8 + 2.0 ** -40), 1.0 + 3 * 2.0 ** -8, 0.0], dtype=torch.float64)
    # a tie goes to even; just above a tie goes up although the fp32 rounding of the float64 value lands ON the tie
    assert R.round_bf16(x).tolist() == [1.0, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 1.0 + 2.0 ** -6, 0.0]
    h = torch.arange(2 * 5 * 768, dtype=torch.float32).view(2, 5, 768) % 251
    g = R.tm_to_group(h)
    assert g.shape == (2, 16, 136, 48) and float(g[:, :, :64].abs().max()) == 0 and float(g[:, :, 69:].abs().max()) == 0
    assert torch.equal(g[1, 3, 64 + 2], h[1, 2, 3 * 48:4 * 48].double())
    rows = R.conv_rows(torch.arange(7 * 2, dtype=torch.float64).view(1, 7, 2), 3, 2)
    assert rows.shape == (1, 3, 6) and rows[0, 1].tolist() == [4, 5, 6, 7, 8, 9]


def test_bounds_are_sharp_against_a_dropped_k_tile_and_a_shifted_residual_row(sd):
    """What the end-to-end bf16 bound lets through must break the per-stage bounds by orders of magnitude: out_proj evaluated with the last 64-wide k-tile of its
    operand missing, and with the residual of ONE row taken from the row above."""
    g = torch.Generator().manual_seed(5)
    o = R.round_bf16(torch.randn(1, 130, 768, generator=g, dtype=torch.float64) * 0.3)
    res = (torch.randn(1, 130, 768, generator=g, dtype=torch.float64)).float().double()
    ref64, ref32 = R.out_proj(sd, 0, o, res), R.out_proj(sd, 0, o, res, dtype=torch.float32)
    e32, bound = R.f32_bound(ref32, ref64)
    o_drop = o.clone()
    o_drop[..., -64:] = 0
    res_shift = res.clone()
    res_shift[0, 129] = res[0, 128]
    r_drop = R.rel_max(R.out_proj(sd, 0, o_drop, res), ref64) / bound
    r_shift = R.rel_max(R.out_proj(sd, 0, o, res_shift), ref64) / bound
    print(f"out_proj: fp32 evaluation {e32:.2e}, bound {bound:.2e}; last k-tile dropped: {r_drop:.0f} x the bound; one residual row shifted: {r_shift:.0f} x the bound")
    assert r_drop >= 100 and r_shift >= 100
    # the same dropped k-tile through a bf16 store (ff1): far fewer than 99 % of the elements stay bit-equal
    hb = R.round_bf16(torch.randn(1, 130, 768, generator=g, dtype=torch.float64))
    hb_drop = hb.clone()
    hb_drop[..., -64:] = 0
    share, bad, _ = R.bf16_stats(R.ff1(sd, 0, hb_drop), R.ff1(sd, 0, hb), 4e-6 * float(R.ff1(sd, 0, hb).abs().max()))
    print(f"ff1 with the last k-tile dropped: {100 * share:.1f} % bit-equal, {bad} elements beyond one bf16 step")
    assert share < 0.5 and bad > 1000
