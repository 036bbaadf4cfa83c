"""The bf16 audio encoder kernel by kernel (run on the MI355X with `-m gpu`).

bf16 mode's Wav2Vec2 encoder (said_amd/csrc/audio_enc.cpp) runs on kernels of its own — the bf16 tile GEMMs of tgemm.hip, the token-major helpers of tm_kernels.hip,
conv0_gn_gelu_tm_bf16 (misc.hip), attn_kernel in bf16 product mode — and end to end it is only held to the fp32 oracle at bf16 distance (4.8e-2 max abs), which a dropped
k-tile or one wrong residual row survives.  Here every stage is stopped behind (said_debug_option "audio_stop_after"), its output and its inputs are read back AS STORED
(said_debug_audio_copy), and the output is compared with tests/audio_bf16_ref.py's evaluation of those inputs: operands rounded to bf16, float64 sums
(tests/test_audio_bf16_ref_cpu.py ties that restatement to the oracle).  Bounds (audio_bf16_ref.check_*):
  fp32 stores   max |got - ref64| / max |ref64| <= 4 max(e32, 1e-6), e32 the same figure of the torch fp32 CPU evaluation of the identical operands;
  bf16 stores   >= 99 % of the elements bit-equal to the rounded reference, every other one within one bf16 step or within the fp32 bound in absolute terms
                (the fp32 CPU evaluation itself must be >= 99.9 % bit-equal on the same inputs, else the inputs are at fault);
  layout kernels exact;
  attention     rms(got - rounded ref) <= 0.1 rms(unrounded ref - rounded ref), the reference restating the kernel's online softmax and key slicing.
All rows and all columns are compared (shape D's positional convolution: clips 0, 4 and 8 — each clip is a launch-batch entry of its own there).
Shapes (the smallest that reach every live tile; the n_tgemm_* counters are asserted):
  S  3 clips x 16000 samples, 59 frames: conv1 on tgemm_kernel<256, 256>, conv2-6 + feature projection on <128, 128>, the positional convolution on the grouped <128, 64>,
     q/k/v, out_proj, ff1, ff2 on the single-buffer <128, 128>, attention with eight key slices + cm_to_tm_bf16;
  D  9 clips x 4000 samples, 599 frames (12 feature frames interpolated to 599): q/k/v per sample (599 = 2 x 256 + 87 rows) and out_proj / ff1 / ff2 as one 5391-row
     matrix on tgemm256d_kernel, attention without key split storing token-major bf16 itself; and again with "tgemm_direct" = 0: the single-buffer tile, bit-identical.
Measured (S / D; every stage prints its own line): fp32 stores 1.2e-7 ... 7.5e-7 of range — feature projection 2.8e-7 / 3.8e-7, positional convolution 1.6e-7 / 7.5e-7, q/k/v
4.0e-7 / 4.9e-7, out_proj 2.3e-7 / 3.3e-7, ff2 4.4e-7 / 6.3e-7, LayerNorm copies and the result 1.2e-7 ... 1.9e-7 (fp32 CPU evaluation 4.9e-8 ... 2.8e-7: the bound is its
floor, 4e-6); bf16 stores 99.979 ... 100 % bit-equal (conv0 99.993 / 99.991, conv1-6 99.980 ... 99.988, ff1 99.979 / 99.980; the fp32 CPU evaluation 99.985 ... 100 %), no element
beyond one bf16 step; attention rms 6.6e-6 (max 7.6e-4) against a bound of 4.7e-5 with eight key slices, 2.7e-5 (max 1.6e-2, one bf16 step) against 1.2e-4 without key split.
"""
import pytest
import torch

import audio_bf16_ref as R
from said_amd import _engine as E
from said_amd.util import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

COUNTERS = ("n_tgemm_128", "n_tgemm_128sb", "n_tgemm_128x64", "n_tgemm_256", "n_tgemm_256x192", "n_tgemm_256d", "n_audio_attn_ks8", "n_audio_attn_tm")
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def full_sd():
    return synth.said_state_dict(num_w2v_layers=1)


@pytest.fixture(scope="module")
def sd(full_sd):
    return R.audio_sd(full_sd)


@pytest.fixture(scope="module")
def model(dev, full_sd):
    from said_amd.model.diffusion import SAID_UNet1D
    from said_amd.model.wav2vec2 import AudioConfig
    m = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=1))
    m.load_state_dict(full_sd, strict=True)
    m.to(dev).eval()
    return m


class Shape:
    def __init__(self, B, Ta, frames, seed):
        self.B, self.Ta, self.F = B, Ta, frames
        self.L = R.conv_lengths(Ta)
        self.Fp = (frames + 31) // 32 * 32
        self.Rg = R.group_rows(frames)
        w = torch.stack([synth.synth_waveform(seed + i, Ta) for i in range(B)])
        self.wav = (w - w.mean(1, keepdim=True)) / torch.sqrt(w.var(1, unbiased=False, keepdim=True) + 1e-7)


def _snap(eng, name, dtype, shape):
    n = 1
    for d in shape:
        n *= d
    raw = eng.audio_snapshot(name, n * (2 if dtype == torch.bfloat16 else 4))
    return raw.view(dtype).view(shape).cpu()


def _collect(model, dev, sh, direct=-1, stops=(2, 4, 6, 11, 15, 16, 18, -1)):
    """The stopped encodes of one shape: {name: tensor as stored}, {counter: launches of ONE complete encode}.  A stop serves every stage whose output no later stage of
    the same encode overwrote: conv outputs ping-pong between bA0 and bA1; bT is the positional convolution's, out_proj's and ff2's output in turn; bH / bHb are every
    LayerNorm's; the rest is written once per layer."""
    B, L, Fr, Fp = sh.B, sh.L, sh.F, sh.Fp
    wav = sh.wav.to(dev)
    s, cnt = {}, {}
    bf, f32 = torch.bfloat16, torch.float32
    try:
        model.set_mfma_dtype("bf16")
        eng = model._get_engine(1, 640)
        eng.debug_option("tgemm_direct", direct)
        for stop in stops:
            eng.debug_option("audio_stop_after", stop)
            c0 = {k: eng.debug_get(k) for k in COUNTERS}
            out = eng.audio_encode(wav, Fr)
            torch.cuda.synchronize()
            if stop == 2:
                s["c0"], s["c1"] = _snap(eng, "bA0", bf, (B, L[0], 512)), _snap(eng, "bA1", bf, (B, L[1], 512))
            elif stop == 4:
                s["c2"], s["c3"] = _snap(eng, "bA0", bf, (B, L[2], 512)), _snap(eng, "bA1", bf, (B, L[3], 512))
            elif stop == 6:
                s["c4"], s["c5"] = _snap(eng, "bA0", bf, (B, L[4], 512)), _snap(eng, "bA1", bf, (B, L[5], 512))
            elif stop == 11:
                s["c5@11"], s["c6"] = _snap(eng, "bA1", bf, (B, L[5], 512)), _snap(eng, "bA0", bf, (B, L[6], 512))
                s["x"], s["hproj"] = _snap(eng, "bX", bf, (B, Fr, 512)), _snap(eng, "bH", f32, (B, Fr, 768))
                s["xg"], s["pos"] = _snap(eng, "bXg", bf, (B, 16, sh.Rg, 48)), _snap(eng, "bT", f32, (B, Fr, 768))
            elif stop == 15:
                s["pos@15"], s["h0"], s["h0b"] = _snap(eng, "bT", f32, (B, Fr, 768)), _snap(eng, "bH", f32, (B, Fr, 768)), _snap(eng, "bHb", bf, (B, Fr, 768))
                s["qk"], s["vt"] = _snap(eng, "aQK", f32, (B, 24, Fp, 64)), _snap(eng, "aVT", f32, (B, 768, Fp))
                s["ao"], s["bo"] = _snap(eng, "aO", f32, (B, 2, 768, Fp))[:, 0], _snap(eng, "bO", bf, (B, Fr, 768))
            elif stop == 16:
                s["bo@16"], s["h0@16"], s["t1"] = _snap(eng, "bO", bf, (B, Fr, 768)), _snap(eng, "bH", f32, (B, Fr, 768)), _snap(eng, "bT", f32, (B, Fr, 768))
            elif stop == 18:
                s["t1@18"], s["h1"], s["h1b"] = _snap(eng, "bT", f32, (B, Fr, 768)), _snap(eng, "bH", f32, (B, Fr, 768)), _snap(eng, "bHb", bf, (B, Fr, 768))
                s["f"] = _snap(eng, "bF", bf, (B, Fr, 3072))
            else:
                s["f@end"], s["h1@end"], s["t2"] = _snap(eng, "bF", bf, (B, Fr, 3072)), _snap(eng, "bH", f32, (B, Fr, 768)), _snap(eng, "bT", f32, (B, Fr, 768))
                s["h2b"], s["out"] = _snap(eng, "bHb", bf, (B, Fr, 768)), out.cpu()
                cnt = {k: eng.debug_get(k) - c0[k] for k in COUNTERS}
        # said_debug_audio_copy refuses an unknown name and more bytes than the buffer holds
        small = torch.empty(16, dtype=torch.uint8, device=dev)
        for name, nbytes in ((b"bNone", 16), (b"bH", 1 << 40)):
            with pytest.raises(E.EngineError):
                eng._call("said_debug_audio_copy", name, E._ptr(small), nbytes, E._stream())
    finally:
        eng = model._eng
        if eng is not None:
            eng.debug_option("audio_stop_after", -1)
            eng.debug_option("tgemm_direct", -1)
        model.set_mfma_dtype("fp32")
    # a stage's input read at a later stop is what the earlier stop saw: the encoder has no atomics, every launch is deterministic
    for a, b in (("c5@11", "c5"), ("pos@15", "pos"), ("bo@16", "bo"), ("h0@16", "h0"), ("t1@18", "t1"), ("f@end", "f"), ("h1@end", "h1")):
        if a in s and b in s:
            assert torch.equal(s[a].view(torch.int16) if s[a].dtype == bf else s[a], s[b].view(torch.int16) if s[b].dtype == bf else s[b]), (a, b)
    return s, cnt


def _bf16_stage(name, got, fn):
    pre64, pre32 = fn(F64), fn(F32)
    return R.check_bf16(name, got, R.round_bf16(pre64), pre64, pre32, R.round_bf16(pre32))


def _f32_stage(name, got, fn):
    return R.check_f32(name, got, fn(F64), fn(F32))


def _flat_qkv(qk, vt):
    return torch.cat([qk.reshape(-1), vt.reshape(-1)])


def _check_front(tag, sd, sh, s, pos_clips=None):
    """conv0 .. the encoder LayerNorm."""
    _bf16_stage(f"{tag} conv0 + GroupNorm + GELU", s["c0"], lambda dt: R.conv0(sd, sh.wav, dtype=dt, store=False))
    for i in range(1, 7):
        _bf16_stage(f"{tag} conv{i} + GELU (M = {sh.L[i]})", s[f"c{i}"], lambda dt: R.conv(sd, i, s[f"c{i - 1}"], dtype=dt, store=False))
    _bf16_stage(f"{tag} interpolation {sh.L[6]} -> {sh.F} + LayerNorm", s["x"], lambda dt: R.interp_ln(sd, s["c6"], sh.F, dtype=dt, store=False))
    _f32_stage(f"{tag} feature projection", s["hproj"], lambda dt: R.fproj(sd, s["x"], dtype=dt, store=False))
    R.check_exact(f"{tag} tm_to_group_bf16", s["xg"], R.tm_to_group(s["hproj"]))
    c = list(range(sh.B)) if pos_clips is None else list(pos_clips)
    _f32_stage(f"{tag} positional convolution + GELU + hidden state (clips {c})", s["pos"][c], lambda dt: R.posconv(sd, s["xg"][c], s["hproj"][c], dtype=dt, store=False))
    _f32_stage(f"{tag} encoder LayerNorm, fp32 copy", s["h0"], lambda dt: R.ln(sd, "encoder.layer_norm", s["pos"], dtype=dt, store=False)[0])
    _bf16_stage(f"{tag} encoder LayerNorm, bf16 copy", s["h0b"], lambda dt: R.ln(sd, "encoder.layer_norm", s["pos"], dtype=dt, store=False)[1])


def _check_gemms(tag, sd, sh, s):
    """The four projection GEMMs of the layer (the ones "tgemm_direct" moves between tiles)."""
    Fr = sh.F
    _f32_stage(f"{tag} q/k/v", _flat_qkv(s["qk"][:, :, :Fr], s["vt"][:, :, :Fr]), lambda dt: _flat_qkv(*R.qkv(sd, 0, s["h0b"], dtype=dt, store=False)))
    pad = s["vt"][:, :, Fr:(Fr + 3) // 4 * 4]
    assert float(pad.abs().max()) == 0 if pad.numel() else True, "v's tokens up to the next multiple of four are written as zeros"
    _f32_stage(f"{tag} out_proj + residual", s["t1"], lambda dt: R.out_proj(sd, 0, s["bo"], s["h0"], dtype=dt, store=False))
    _bf16_stage(f"{tag} ff1 + GELU", s["f"], lambda dt: R.ff1(sd, 0, s["h1b"], dtype=dt, store=False))
    _f32_stage(f"{tag} ff2 + residual", s["t2"], lambda dt: R.ff2(sd, 0, s["f"], s["h1"], dtype=dt, store=False))


def _check_layer_rest(tag, sd, sh, s, ks):
    """Attention, cm_to_tm_bf16 and the layer's two LayerNorms."""
    Fr = sh.F
    qk, vt = s["qk"][:, :, :Fr], s["vt"][:, :, :Fr]
    ref_u = R.attention(qk, vt, rounded=False)
    if ks > 1:   # eight key slices, fp32 channel-major result, then the layout kernel
        R.check_attention(f"{tag} attention, {ks} key slices", s["ao"][:, :, :Fr].transpose(1, 2), R.attention(qk, vt, ks), ref_u)
        R.check_exact(f"{tag} cm_to_tm_bf16", s["bo"], R.cm_to_tm(s["ao"][:, :, :Fr]))
    else:        # no key split: the kernel stores token-major bf16 itself
        R.check_attention(f"{tag} attention, no key split, token-major bf16 store", s["bo"], R.attention(qk, vt, 1, out_bf16=True), ref_u)
    p = "encoder.layers.0."
    _f32_stage(f"{tag} layer_norm, fp32 copy", s["h1"], lambda dt: R.ln(sd, p + "layer_norm", s["t1"], dtype=dt, store=False)[0])
    _bf16_stage(f"{tag} layer_norm, bf16 copy", s["h1b"], lambda dt: R.ln(sd, p + "layer_norm", s["t1"], dtype=dt, store=False)[1])
    _f32_stage(f"{tag} final_layer_norm -> result", s["out"], lambda dt: R.ln(sd, p + "final_layer_norm", s["t2"], dtype=dt, store=False)[0])
    _bf16_stage(f"{tag} final_layer_norm, bf16 copy", s["h2b"], lambda dt: R.ln(sd, p + "final_layer_norm", s["t2"], dtype=dt, store=False)[1])


def test_small_batch_stages_against_the_operand_rounded_evaluation_of_their_own_inputs(model, dev, sd):
    """Shape S, every stage.  Measured (max-norm e beside its bound; bit-equal share): see DESIGN 7.2."""
    sh = Shape(3, 16000, 59, 810)
    s, cnt = _collect(model, dev, sh)
    print(f"S: launches of one encode: {cnt}")
    assert cnt == {"n_tgemm_128": 6, "n_tgemm_128sb": 4, "n_tgemm_128x64": 1, "n_tgemm_256": 1, "n_tgemm_256x192": 0, "n_tgemm_256d": 0,
                   "n_audio_attn_ks8": 1, "n_audio_attn_tm": 0}, cnt
    assert torch.isfinite(s["out"]).all()
    _check_front("S", sd, sh, s)
    _check_gemms("S single-buffer tile", sd, sh, s)
    _check_layer_rest("S", sd, sh, s, ks=8)


@pytest.fixture(scope="module")
def shape_d(model, dev):
    sh = Shape(9, 4000, 599, 830)
    s, cnt = _collect(model, dev, sh)
    return sh, s, cnt


def test_large_batch_stages_on_the_direct_to_lds_tile(model, dev, sd, shape_d):
    """Shape D, every stage: the four projections on tgemm256d_kernel, attention storing token-major bf16 itself, 12 feature frames interpolated to 599."""
    sh, s, cnt = shape_d
    print(f"D: launches of one encode: {cnt}")
    assert cnt == {"n_tgemm_128": 7, "n_tgemm_128sb": 0, "n_tgemm_128x64": 1, "n_tgemm_256": 0, "n_tgemm_256x192": 0, "n_tgemm_256d": 4,
                   "n_audio_attn_ks8": 0, "n_audio_attn_tm": 1}, cnt
    assert torch.isfinite(s["out"]).all()
    _check_front("D", sd, sh, s, pos_clips=(0, 4, 8))
    _check_gemms("D direct-to-LDS tile", sd, sh, s)
    _check_layer_rest("D", sd, sh, s, ks=1)


def test_large_batch_projections_on_the_single_buffer_tile_are_bit_identical_and_right_on_their_own(model, dev, sd, shape_d):
    """Shape D with "tgemm_direct" = 0: the same four GEMMs on tgemm_kernel<128, 128, true>, from the same stored inputs — bit-identical to the direct tile, and held to
    the reference on its own (the tiles share tile_mfma / tile_epilogue / tg_epilogue: identity alone would pass an error in the shared part)."""
    sh, s1, _ = shape_d
    s0, cnt = _collect(model, dev, sh, direct=0, stops=(15, 16, 18, -1))
    print(f"D, tgemm_direct = 0: launches of one encode: {cnt}")
    assert cnt["n_tgemm_128sb"] == 4 and cnt["n_tgemm_256d"] == 0 and cnt["n_tgemm_256"] == 0 and cnt["n_audio_attn_tm"] == 1, cnt
    Fr = sh.F
    for k in ("h0", "h0b", "bo", "t1", "h1", "h1b", "f", "t2", "h2b", "out"):
        a, b = s0[k], s1[k]
        same = torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.dtype == torch.bfloat16 else torch.equal(a, b)
        assert same, f"{k}: the single-buffer tile's run differs from the direct tile's"
    assert torch.equal(s0["qk"][:, :, :Fr], s1["qk"][:, :, :Fr]) and torch.equal(s0["vt"][:, :, :Fr], s1["vt"][:, :, :Fr])
    _check_gemms("D single-buffer tile", sd, sh, s0)
