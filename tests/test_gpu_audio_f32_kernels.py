"""The fp32 audio encoder launch by launch (run on the MI355X with `-m gpu`).

The fp32 branch of said_audio_encode (said_amd/csrc/audio_enc.cpp) — conv0_kernel, rownorm_gelu_kernel, interp_linear_kernel, layernorm_cm_kernel, cm_to_tm_kernel
(misc.hip), cgemm_kernel (gemm.hip) with its strided-convolution segment, the XF_LN operand transform, the grouped positional convolution, EPI_QKV and RES_PLAIN,
attn_kernel at head_dim 64 in product modes 2 (default: split-fp16) and 0 (strict) — feeds everything else and was only held to the oracle end to end, behind a
LayerNorm per layer.  Here every launch is stopped behind (said_debug_option "audio_stop_after"), its output and its inputs are read back AS STORED
(said_debug_audio_copy), and the output is compared with tests/audio_f32_ref.py's float64 evaluation of those inputs (tests/test_audio_f32_ref_cpu.py ties that
restatement to the oracle and shows the defects it catches).  Bounds (audio_bf16_ref.check_*; no new number):
  fp32 stores    max |got - ref64| / max |ref64| <= 4 max(e32, 1e-6), e32 the same figure of the torch fp32 CPU evaluation of the identical stored inputs —
                 attention included: both of its products are fp32-grade here;
  layout stores  exact (cm_to_tm, the features-only store).
All clips, channels and tokens t < frames are compared.  The shapes and what each reaches are audio_f32_ref.SHAPES, proved from said_amd/csrc/audio_plan.h by
tests/test_audio_plan_cpu.py; the attention counters n_audio_attn_f32_ks8 / _ks4 / _ks1 are asserted here.  Further: both fp32 modes (split-fp16 and strict,
effective_precision asserted); every byte of every encoder buffer filled with 0x00 / 0xFF / 0x7F before an encode, and a larger encode run first: the results are
finite and bit-identical to the first one and to a fresh context's; a chunked encode (passes of 2 + 1 clips) is, pass by pass, the encode of those clips alone.
Measured (max of range over the shapes; every launch prints its own line; the fp32 CPU evaluation of the same inputs is at 5.8e-8 ... 1.4e-6, so the bound is its floor, 4e-6,
but for one launch at 5.4e-6): conv0 1.7e-7, GroupNorm + GELU 1.7e-7, conv1-6 5.5e-7 (the (4, 4) tile 5.5e-7), interpolation 8.2e-8 (bit-equal to the fp32 CPU evaluation), feature
projection 8.2e-7, positional convolution 1.0e-6, LayerNorms 2.2e-7, q/k/v 5.2e-7, out_proj 2.8e-7, ff1 6.4e-7, ff2 5.7e-7, audio_proj_layer 2.2e-7; attention on split-fp16
products 2.8e-7 / 2.6e-7 / 3.9e-7 with eight / four / no key slices, on fp32 MFMAs 2.9e-7 / 3.9e-7 / 8.7e-7.  No fill value and no earlier encode changed a bit of any result.
"""
import pytest
import torch

import audio_f32_ref as R
from said_amd import _engine as E
from said_amd.util import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

COUNTERS = ("n_audio_attn_f32_ks8", "n_audio_attn_f32_ks4", "n_audio_attn_f32_ks1", "n_audio_attn_ks8", "n_audio_attn_tm")
F64, F32 = torch.float64, torch.float32
FD = 64
MODES = ("fp32", "fp32_strict")


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


def _engine(dev, state, ctx_dim=768):
    with torch.cuda.device(dev):
        e = E.Engine(dev, 2, 64, 32, ctx_dim)
        e.load_weights(state)
    return e


@pytest.fixture(scope="module")
def eng(dev, full_sd):
    e = _engine(dev, full_sd)
    yield e
    e.close()


class Shape:
    def __init__(self, name, seed, clips=None):
        d = R.SHAPES[name]
        self.name, self.Ta, self.frames, self.chunk = name, d["Ta"], d["frames"], d["chunk"]
        self.L = R.conv_lengths(self.Ta)
        self.F = self.frames or self.L[6]
        self.Fp = R.pitch_of(self.F)
        self.ks = d["plan"]["attn"]
        w = torch.stack([synth.synth_waveform(seed + i, self.Ta) for i in range(d["B"])])
        self.wav = (w - w.mean(1, keepdim=True)) / torch.sqrt(w.var(1, unbiased=False, keepdim=True) + 1e-7)
        if clips is not None:
            self.wav = self.wav[clips]
        self.B = self.wav.shape[0]


def _snap(eng, name, shape):
    n = 4
    for d in shape:
        n *= d
    return eng.audio_snapshot(name, n).view(F32).view(shape).cpu()


def _setup(eng, mode, chunk=32):
    eng.set_precision(mode)
    assert eng.effective_precision() == mode
    eng.debug_option("audio_chunk", chunk)


def _restore(eng):
    eng.debug_option("audio_stop_after", -1)
    eng.debug_option("audio_chunk", 32)
    eng.set_precision("fp32")


def _collect(eng, dev, sh, mode, stops, apply_proj=False):
    """The stopped encodes of one shape in one pass: {name: tensor as stored}, {counter: launches of the complete encode}.  A stop serves every launch whose output
    no later launch of the same encode overwrote: the conv outputs ping-pong between abufA and abufB (the GroupNorm runs in place on conv0's), the encoder LayerNorm
    and the layer's two write aH in place of their input's residual, aT is out_proj's and ff2's in turn."""
    B, L, Fr, Fp = sh.B, sh.L, sh.F, sh.Fp
    assert B <= sh.chunk, "one pass: the buffers then hold every clip"
    wav = sh.wav.to(dev)
    pL = [R.pitch_of(x) for x in L]
    s, cnt = {}, {}
    A = lambda i: _snap(eng, "abufA", (B, 512, pL[i]))   # noqa: E731
    Bb = lambda i: _snap(eng, "abufB", (B, 512, pL[i]))  # noqa: E731
    tok = lambda name, C=768: _snap(eng, name, (B, C, Fp))  # noqa: E731
    try:
        _setup(eng, mode, sh.chunk)
        for stop in stops:
            eng.debug_option("audio_stop_after", stop)
            c0 = {k: eng.debug_get(k) for k in COUNTERS}
            out = eng.audio_encode(wav, sh.frames, apply_proj)
            torch.cuda.synchronize()
            if stop == 1:
                s["c0raw"] = A(0)
            elif stop == 3:
                s["c0"], s["c1"] = A(0), Bb(1)
            elif stop == 5:
                s["c2"], s["c3"] = A(2), Bb(3)
            elif stop == 7:
                s["c4"], s["c5"] = A(4), Bb(5)
            elif stop == 11:
                s["c6"], s["hproj"], s["pos"] = A(6), tok("aH"), tok("aPOS")
                if sh.frames:
                    s["x"] = tok("aX", 512)
            elif stop == 14:   # (K: behind attention)
                s["h0"], s["qk"], s["v"] = tok("aH"), _snap(eng, "aQK", (B, 24, Fp, 64)), tok("aVT")
                s["o"] = _snap(eng, "aO", (B, 2, 768, Fp))[:, 0].contiguous()
                cnt = {k: eng.debug_get(k) - c0[k] for k in COUNTERS}
            elif stop == 15:
                s["h0"], s["qk"], s["v"] = tok("aH"), _snap(eng, "aQK", (B, 24, Fp, 64)), tok("aVT")
                s["o"], s["t1"] = _snap(eng, "aO", (B, 2, 768, Fp))[:, 0].contiguous(), tok("aT")
            elif stop == 17:
                s["t1@17"], s["h1"], s["f"] = tok("aT"), tok("aH"), tok("aF", 3072)
            elif stop == 18:
                s["h1@18"], s["f@18"], s["t2"] = tok("aH"), tok("aF", 3072), tok("aT")
            elif stop == 20:   # (apply_proj: behind audio_proj_layer)
                s["h2"], s["p"] = tok("aH"), _snap(eng, "aT", (B, FD, Fp))
            else:
                assert stop == -1
                if not apply_proj:
                    s["h2"] = tok("aH")
                s["out"] = out.cpu()
                cnt = {k: eng.debug_get(k) - c0[k] for k in COUNTERS}
    finally:
        _restore(eng)
    # a launch's input read at a later stop is what the earlier stop saw: the encoder has no atomics, every launch is deterministic
    for a, b in (("t1@17", "t1"), ("h1@18", "h1"), ("f@18", "f")):
        if a in s and b in s:
            assert torch.equal(s[a], s[b]), (a, b)
    return s, cnt


FRONT_STOPS, LAYER_STOPS = (1, 3, 5, 7, 11), (15, 17, 18, -1)


def _f32(name, got, fn):
    return R.check_f32(name, got, fn(F64), fn(F32))


def _valid(x, T):
    return x[..., :T]


def _check_convs(tag, sd, sh, s, which=range(1, 7)):
    L = sh.L
    if "c0raw" in s:
        _f32(f"{tag} conv0", _valid(s["c0raw"], L[0]), lambda dt: R.conv0(sd, sh.wav, dt))
        _f32(f"{tag} GroupNorm + GELU", _valid(s["c0"], L[0]), lambda dt: R.rownorm_gelu(sd, s["c0raw"], L[0], dt))
    for i in which:
        _f32(f"{tag} conv{i} + GELU ({L[i - 1]} -> {L[i]} rows)", _valid(s[f"c{i}"], L[i]), lambda dt: R.conv(sd, i, s[f"c{i - 1}"], L[i - 1], dt))


def _check_front(tag, sd, sh, s):
    """conv0 .. the positional convolution (the encoder LayerNorm is checked with the layer: its output is read at stop 15)."""
    L, Fr = sh.L, sh.F
    _check_convs(tag, sd, sh, s)
    feat = s["c6"]
    if sh.frames:
        _f32(f"{tag} interpolation {L[6]} -> {Fr}", _valid(s["x"], Fr), lambda dt: R.interp_linear(s["c6"], L[6], Fr, dt))
        feat = s["x"]
    _f32(f"{tag} feature projection (LayerNorm in the operand transform)", _valid(s["hproj"], Fr), lambda dt: R.fproj(sd, feat, Fr, dt))
    _f32(f"{tag} positional convolution + GELU", _valid(s["pos"], Fr), lambda dt: R.posconv(sd, s["hproj"], Fr, dt))


def _flat(qk, v):
    return torch.cat([qk.reshape(-1), v.reshape(-1)])


def _attn_ref(qk, v, T, ks, dt):
    """R.attention sixteen clips at a time (the scores of 86 clips x 250 frames in float64 are half a gigabyte)."""
    return torch.cat([R.attention(qk[b:b + 16], v[b:b + 16], T, ks, dt) for b in range(0, qk.shape[0], 16)])


def _check_qkv(tag, sd, sh, s, clips=None):
    Fr = sh.F
    c = list(range(sh.B)) if clips is None else list(clips)
    got = _flat(s["qk"][c][:, :, :Fr], s["v"][c][..., :Fr])
    _f32(f"{tag} q/k/v (clips {c if clips is not None else 'all'})", got, lambda dt: _flat(*R.qkv(sd, 0, s["h0"][c], Fr, dt)))
    # v alone: its 768 channel rows are a third of the vector above and the smaller numbers
    _f32(f"{tag} v rows alone", s["v"][c][..., :Fr], lambda dt: R.qkv(sd, 0, s["h0"][c], Fr, dt)[1])


def _check_attention(tag, sh, s):
    Fr = sh.F
    _f32(f"{tag} attention, {sh.ks} key slice(s), {sh.B * ((Fr + 31) // 32)} token tiles", _valid(s["o"], Fr), lambda dt: _attn_ref(s["qk"], s["v"], Fr, sh.ks, dt))


def _check_layer(tag, sd, sh, s):
    """The encoder LayerNorm and the layer (its input hproj / pos is read at stop 11, its output at stop 15)."""
    Fr = sh.F
    p = "encoder.layers.0."
    _f32(f"{tag} encoder LayerNorm (hidden + positional)", _valid(s["h0"], Fr), lambda dt: R.layernorm(sd, "encoder.layer_norm", s["hproj"], s["pos"], Fr, dt))
    _check_qkv(tag, sd, sh, s)
    _check_attention(tag, sh, s)
    _f32(f"{tag} out_proj + residual", _valid(s["t1"], Fr), lambda dt: R.out_proj(sd, 0, s["o"], s["h0"], Fr, dt))
    _f32(f"{tag} layer_norm", _valid(s["h1"], Fr), lambda dt: R.layernorm(sd, p + "layer_norm", s["t1"], None, Fr, dt))
    _f32(f"{tag} ff1 + GELU", _valid(s["f"], Fr), lambda dt: R.ff1(sd, 0, s["h1"], Fr, dt))
    _f32(f"{tag} ff2 + residual", _valid(s["t2"], Fr), lambda dt: R.ff2(sd, 0, s["f"], s["h1"], Fr, dt))
    _f32(f"{tag} final_layer_norm", _valid(s["h2"], Fr), lambda dt: R.layernorm(sd, p + "final_layer_norm", s["t2"], None, Fr, dt))
    R.check_exact(f"{tag} cm_to_tm -> result", s["out"], R.cm_to_tm(s["h2"], Fr))
    assert torch.isfinite(s["out"]).all()


def _attn_counts(ks, n=1):
    c = dict.fromkeys(COUNTERS, 0)
    c[f"n_audio_attn_f32_ks{ks}"] = n
    return c


def _full(eng, dev, sd, name, seed, mode, clips=None):
    sh = Shape(name, seed, clips)
    s, cnt = _collect(eng, dev, sh, mode, FRONT_STOPS + LAYER_STOPS)
    tag = f"{name}{'' if clips is None else list(clips)} {mode}"
    print(f"{tag}: attention launches of one encode: {cnt}")
    assert cnt == _attn_counts(sh.ks), cnt
    _check_front(tag, sd, sh, s)
    _check_layer(tag, sd, sh, s)
    return sh, s


# ---------------------------------------------------------------------------------------------------------------- every launch, shape by shape
@pytest.mark.parametrize("mode", MODES)
def test_small_batch_every_launch(eng, dev, sd, mode):
    """S: 3 clips x 16000 samples, 59 frames — conv1 and q/k/v on (2, 8), the rest on one tile x eight waves, attention with eight key slices."""
    _full(eng, dev, sd, "S", 810, mode)


def test_no_interpolation_every_launch(eng, dev, sd):
    """N: 2 clips x 8000 samples, no frame count — the encoder runs on the feature extractor's own 24 frames (8 pad rows), the interpolation site launches nothing."""
    sh, s = _full(eng, dev, sd, "N", 820, "fp32")
    assert sh.F == 24 and "x" not in s and s["out"].shape == (2, 24, 768)


def test_one_long_clip_every_launch(eng, dev, sd):
    """M: 1 clip x 4000 samples, 599 frames (12 feature frames interpolated to 599) — ff1 on (2, 8), everything else small."""
    _full(eng, dev, sd, "M", 825, "fp32")


@pytest.mark.parametrize("mode", MODES)
def test_large_batch_every_launch(eng, dev, sd, mode):
    """D: 9 clips x 4000 samples, 599 frames, 171 token tiles — the 768-wide GEMMs, ff1 and q/k/v on (6, 4), the positional convolution on NB 2, attention with
    four key slices (2052 workgroups > 2048)."""
    _full(eng, dev, sd, "D", 830, mode)


def test_long_convolutions_on_four_tiles(eng, dev, sd):
    """C: 9 clips x 16000 samples, front end only — conv1 has 450 token tiles and runs on (4, 4), conv2 and conv3 on (2, 8)."""
    sh = Shape("C", 840)
    s, _ = _collect(eng, dev, sh, "fp32", (3, 5))   # conv2's input is conv1's output as stop 3 stored it: the launches are deterministic
    _check_convs("C fp32", sd, sh, s, which=(1, 2, 3))


@pytest.mark.parametrize("mode", MODES)
def test_attention_without_key_split(eng, dev, sd, mode):
    """K: 86 clips x 1000 samples, 250 frames in ONE pass (audio_chunk = 86): 688 token tiles, attn_kernel<2, 1, PM> — no other test reaches it (the largest pass
    elsewhere, 32 clips x 600 frames, is 608 tiles: four slices).  Stopped behind attention: q/k/v as stored -> attention output for every clip; the q/k/v launch
    itself, on (6, 4), for three clips."""
    sh = Shape("K", 850)
    s, cnt = _collect(eng, dev, sh, mode, (14,))
    print(f"K {mode}: attention launches: {cnt}")
    assert cnt == _attn_counts(1), cnt
    _check_attention(f"K {mode}", sh, s)
    if mode == "fp32":
        # h0 at stop 14 is the q/k/v launch's input (the layer's first LayerNorm, stage 15, has not run)
        _check_qkv("K fp32", sd, sh, s, clips=(0, 42, 85))


# ---------------------------------------------------------------------------------------------------------------- audio_proj_layer and the features-only entry
def test_projection_and_features_only(dev, sd, full_sd):
    """P: shape S on a feature_dim context — audio_proj_layer on (1, 8) and the final cm_to_tm; and said_audio_extract_features with and without interpolation: its
    cm_to_tm store is exactly the stored feature buffer, which is held to the interp_linear reference."""
    psd = {k: v for k, v in full_sd.items() if k.startswith("audio_encoder.")}
    psd["null_cond_emb"] = synth.fill_tensor("null_cond_emb", (1, 1, FD))
    psd.update(synth.fill_state_dict(synth.unet_param_shapes(32, 32, FD), "denoiser."))
    W = psd["audio_proj_layer.weight"] = synth.fill_tensor("audio_proj_layer.weight", (FD, 768))
    b = psd["audio_proj_layer.bias"] = synth.fill_tensor("audio_proj_layer.bias", (FD,))
    e = _engine(dev, psd, FD)
    try:
        sh = Shape("S", 810)
        Fr = sh.F
        s, cnt = _collect(e, dev, sh, "fp32", (20, -1), apply_proj=True)
        assert cnt == _attn_counts(8), cnt
        _f32("P audio_proj_layer", _valid(s["p"], Fr), lambda dt: R.proj(W, b, s["h2"], Fr, dt))
        R.check_exact("P cm_to_tm -> result", s["out"], R.cm_to_tm(s["p"], Fr))
        assert s["out"].shape == (3, Fr, FD) and torch.isfinite(s["out"]).all()
        wav = sh.wav.to(dev)
        pL = R.pitch_of(sh.L[6])
        _setup(e, "fp32")
        # with interpolation: stages 0 .. 8, then the store
        feats = e.extract_features(wav, Fr).cpu()
        c6, x = _snap(e, "abufA", (3, 512, pL)), _snap(e, "aX", (3, 512, sh.Fp))
        _f32(f"P features: interpolation {sh.L[6]} -> {Fr}", _valid(x, Fr), lambda dt: R.interp_linear(c6, sh.L[6], Fr, dt))
        R.check_exact("P features-only store, interpolated", feats, R.cm_to_tm(x, Fr))
        _f32("P features-only result against the interp_linear reference", feats.transpose(1, 2), lambda dt: R.interp_linear(c6, sh.L[6], Fr, dt))
        # without: the store reads the last convolution's output
        feats = e.extract_features(wav, None).cpu()
        c6n = _snap(e, "abufA", (3, 512, pL))
        assert torch.equal(c6n, c6)
        R.check_exact("P features-only store, no interpolation", feats, R.cm_to_tm(c6, sh.L[6]))
        _f32("P features-only result against conv6's reference", feats.transpose(1, 2), lambda dt: R.conv(sd, 6, _snap(e, "abufB", (3, 512, R.pitch_of(sh.L[5]))), sh.L[5], dt))
        # "audio_stop_after" holds for this entry too: stopped in front of the store, the output keeps what it held
        e.debug_option("audio_stop_after", 9)
        marker = torch.full((3, Fr, 512), 7.0, device=dev)
        e._go("said_audio_extract_features", E._ptr(wav), 3, sh.Ta, Fr, E._ptr(marker), None)
        torch.cuda.synchronize()
        assert bool((marker == 7.0).all())
    finally:
        _restore(e)
        e.close()


# ---------------------------------------------------------------------------------------------------------------- memory nobody wrote
def _encode(e, dev, sh, mode="fp32"):
    _setup(e, mode, sh.chunk)
    try:
        out = e.audio_encode(sh.wav.to(dev), sh.frames)
        torch.cuda.synchronize()
        return out.cpu()
    finally:
        _restore(e)


@pytest.mark.parametrize("name,seed", [("S", 810), ("N", 820), ("D", 830), ("K", 850)])
def test_result_does_not_depend_on_what_the_buffers_held(eng, dev, full_sd, name, seed):
    """The encoder's buffers are sized lazily and are not part of the workspace list; their pad rows frames .. pitch hold whatever was there.  Every byte of every
    buffer set to 0x00, 0xFF (NaN) and 0x7F (3.4e38) before an encode: finite and bit-identical to the first result and to a fresh context's."""
    sh = Shape(name, seed)
    first = _encode(eng, dev, sh)
    assert torch.isfinite(first).all()
    for byte in (0x00, 0xFF, 0x7F):
        eng.audio_fill(byte)
        for buf in ("abufA", "abufB", "aX", "aH", "aT", "aO", "aQK", "aVT", "aF", "aPOS"):   # the fill reached it: its first and (of aF, the largest) last bytes
            assert bool((eng.audio_snapshot(buf, 256) == byte).all()), (buf, byte)
        n_f = sh.B * 3072 * sh.Fp * 4
        assert bool((eng.audio_snapshot("aF", n_f)[-256:] == byte).all())
        got = _encode(eng, dev, sh)
        assert torch.isfinite(got).all(), f"{name}: fill 0x{byte:02X}: the result is not finite"
        assert torch.equal(got, first), f"{name}: fill 0x{byte:02X}: {int((got != first).sum())} elements differ, max {float((got - first).abs().max()):.3e}"
    fresh = _engine(dev, full_sd)
    try:
        got = _encode(fresh, dev, sh)
    finally:
        fresh.close()
    assert torch.equal(got, first), f"{name}: a fresh context differs in {int((got != first).sum())} elements"
    if name == "S":   # strict mode reads the same buffers through the other product path
        eng.audio_fill(0xFF)
        a = _encode(eng, dev, sh, "fp32_strict")
        eng.audio_fill(0x7F)
        assert torch.isfinite(a).all() and torch.equal(_encode(eng, dev, sh, "fp32_strict"), a)


def test_result_does_not_depend_on_an_earlier_larger_encode(eng, dev, full_sd):
    """D then S in one context: S's pad rows and everything behind its 3 clips hold D's values."""
    d, s = Shape("D", 830), Shape("S", 810)
    fresh = _engine(dev, full_sd)
    try:
        want = _encode(fresh, dev, s)
        _encode(fresh, dev, d)
        got = _encode(fresh, dev, s)
    finally:
        fresh.close()
    assert torch.isfinite(got).all() and torch.equal(got, want), f"{int((got != want).sum())} elements differ"
    n = Shape("N", 820)
    want = _encode(eng, dev, n)
    _encode(eng, dev, d)
    assert torch.equal(_encode(eng, dev, n), want)
    # slots the small encode must leave alone: behind its 2 clips the buffers, sized by D, keep every byte of the fill
    eng.audio_fill(0x7F)
    assert torch.equal(_encode(eng, dev, n), want)
    pL = [R.pitch_of(x) for x in n.L]
    used = {"abufA": n.B * 512 * pL[0], "abufB": n.B * 512 * pL[1], "aH": n.B * 768 * n.Fp, "aT": n.B * 768 * n.Fp, "aPOS": n.B * 768 * n.Fp, "aVT": n.B * 768 * n.Fp,
            "aQK": n.B * 1536 * n.Fp, "aO": n.B * 1536 * n.Fp, "aF": n.B * 3072 * n.Fp}
    for buf, floats in used.items():
        tail = eng.audio_snapshot(buf, 4 * floats + (1 << 20))[4 * floats:]
        bad = int((tail != 0x7F).sum())
        print(f"{buf}: {bad} of the {tail.numel()} bytes behind the encode's {floats} floats were written")
        assert bad == 0, buf
    assert bool((eng.audio_snapshot("aX", 1 << 20) == 0x7F).all()), "no interpolation: aX is not written at all"


# ---------------------------------------------------------------------------------------------------------------- chunking
def test_chunked_encode_is_its_passes(eng, dev, sd):
    """S's three clips with audio_chunk = 2: passes of 2 + 1 clips.  The tile shapes follow the pass size, so the result is not asked to be the unchunked one bit for
    bit; it IS, bit for bit, the encode of each pass's clips alone, and each of those is held launch by launch to the same references."""
    sh = Shape("S2", 810)
    got = _encode(eng, dev, sh)
    a, sa = _full(eng, dev, sd, "S2", 810, "fp32", clips=[0, 1])
    b, sb = _full(eng, dev, sd, "S2", 810, "fp32", clips=[2])
    assert got.shape == (3, 59, 768) and torch.isfinite(got).all()
    assert torch.equal(got[:2], sa["out"]) and torch.equal(got[2:], sb["out"])
