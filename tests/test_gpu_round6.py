"""Round 6 (run on the MI355X with `-m gpu`): fp32 mode at the edges of its arithmetic's domain.

fp32 mode multiplies on split-fp16 operands (said_amd/csrc/split_f16.h: x = h + 2^-11 l, both planes fp16): every product operand must satisfy
|x| < 65504, and a tensor whose largest element is below 2^-14 loses relative precision.  What guards that (include/said_hip.h, "precision"):
  * weights are range-checked at said_finalize_weights: outside [2^-14, 2^15) the context runs strict fp32 (v_mfma_f32_32x32x2_f32);
  * an activation beyond the range turns into inf / NaN, reaches the step's model output, and is recorded there (said_numeric_status);
    SAID.inference / SAID.forward then run the call again in strict fp32 (policy `on_nonfinite`);
  * SAID_PREC_FP32_STRICT is a public mode of its own.
The tests rescale weights by exact powers of two in compensating pairs — to_v x 2^k with to_out x 2^-k, GEGLU's value half x 2^k with ff.net.2 x 2^-k,
to_q x 2^-k with to_k x 2^k: the function the network computes is unchanged and so (barring fp32 overflow) is every rounding of the fp32 reference —
and push un-normalised operands (attention outputs, the GEGLU product, q / k / v) towards both edges.
Also here: a "trained-like" weight fill (heavy tails, outlier channels, norm gains up to 10) through the UNet in all three precision modes.
"""
import warnings

import pytest
import torch

from oracle import pipeline as op
from oracle import unet as ou
from said_amd.util import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ST = ("input_blocks.1.1", "middle_block.1", "output_blocks.0.1", "output_blocks.1.1")
FFI = 768


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _make(sd, dev):
    from said_amd.model.diffusion import SAID_UNet1D
    from said_amd.model.wav2vec2 import AudioConfig
    m = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=2))
    m.load_state_dict(sd, strict=True)
    m.to(dev).eval()
    return m


def _base_sd():
    return synth.said_state_dict(num_w2v_layers=2)


def _rescaled(sd, k_v=0, k_ff=0, k_qk=0, k_v2=0, blocks=ST, extra=None):
    """to_v x 2^k_v / to_out x 2^-k_v (self-attention), value half of ff.net.0.proj x 2^k_ff / ff.net.2 x 2^-k_ff, to_q x 2^-k_qk / to_k x 2^k_qk
    (self-attention), attn2.to_v x 2^k_v2 / attn2.to_out x 2^-k_v2, in the named SpatialTransformers: exact in fp32, the network's function unchanged.
    extra: {parameter suffix below transformer_blocks.0: exponent} applied on top (uncompensated: the function changes, the oracle sees the same weights)."""
    sd = {k: v.clone() for k, v in sd.items()}
    for st in blocks:
        b = f"denoiser.model.{st}.transformer_blocks.0"
        sd[b + ".attn1.to_v.weight"] *= 2.0 ** k_v
        sd[b + ".attn1.to_out.0.weight"] *= 2.0 ** -k_v
        sd[b + ".ff.net.0.proj.weight"][:FFI] *= 2.0 ** k_ff
        sd[b + ".ff.net.0.proj.bias"][:FFI] *= 2.0 ** k_ff
        sd[b + ".ff.net.2.weight"] *= 2.0 ** -k_ff
        sd[b + ".attn1.to_q.weight"] *= 2.0 ** -k_qk
        sd[b + ".attn1.to_k.weight"] *= 2.0 ** k_qk
        sd[b + ".attn2.to_v.weight"] *= 2.0 ** k_v2
        sd[b + ".attn2.to_out.0.weight"] *= 2.0 ** -k_v2
        for suffix, k in (extra or {}).items():
            sd[b + "." + suffix] *= 2.0 ** k
    return sd


def _inputs(B, T, seed=1):
    return synth.synth_latents(seed, (B, T, 32)), (torch.arange(B) * 137 + 500) % 1000, synth.synth_latents(seed + 1, (B, T, 768))


def _fwd(model, dev, x, ts, c):
    return model(x.to(dev), ts.to(dev), c.to(dev)).cpu()


def _oracle(sd, x, ts, c):
    _, sd_u, _ = op.split_state_dict(sd)
    return ou.unet1d_forward(sd_u, x, ts, c)


def _rel(a, ref):
    return float((a - ref).abs().max()) / float(ref.max() - ref.min())


def test_precision_modes_are_public_and_strict_runs_no_split_kernel(dev):
    sd = _base_sd()
    m = _make(sd, dev)
    x, ts, c = _inputs(2, 60)
    ref = _oracle(sd, x, ts, c)
    out = {}
    for mode in ("fp32", "fp32_strict", "bf16"):
        m.set_mfma_dtype(mode)
        eng = m._get_engine(2, 64)
        n0 = eng.debug_get("n_stchain")
        out[mode] = _fwd(m, dev, x, ts, c)
        assert eng.get_precision() == mode and eng.effective_precision() == mode and eng.precision_note() == ""
        fused = eng.debug_get("n_stchain") - n0
        assert fused == (4 if mode == "fp32" else 0), (mode, fused)   # strict: the five-launch tail on fp32 matrix instructions
        if mode != "bf16":
            for opt in ("ugemm_split", "attn_split", "gemm_split", "st_chain"):
                assert eng.debug_get(opt) == (1 if mode == "fp32" else 0), (mode, opt)
        assert eng.numeric_status() == (-1, False)
    m.set_mfma_dtype("fp32")
    e_split, e_strict, e_bf = _rel(out["fp32"], ref), _rel(out["fp32_strict"], ref), _rel(out["bf16"], ref)
    print(f"vs oracle, of range: split-fp16 {e_split:.2e}, strict fp32 {e_strict:.2e}, bf16 {e_bf:.2e}")
    assert e_split <= 1e-4 and e_strict <= 1e-4 and e_bf <= 2e-2
    with pytest.raises(ValueError):
        m.set_mfma_dtype("fp16")
    from said_amd import _engine
    with pytest.raises(_engine.EngineError):
        eng.set_precision("tf32")


# measured (MI355X, round 6): see the printed values; the bound is the parity suite's fp32 bound
@pytest.mark.parametrize("kw", [dict(k_v=8), dict(k_ff=6), dict(k_v=8, k_ff=6, k_qk=4, k_v2=8), dict(k_v=-8, k_ff=-6, k_qk=-4, k_v2=-6), dict(k_v=12, k_ff=10)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
@pytest.mark.parametrize("B,T", [(2, 600), (3, 37)])
def test_power_of_two_rescaling_inside_the_domain_changes_nothing(dev, kw, B, T):
    """Un-normalised operands (v, attention output, GEGLU product, q, k) moved by 2^+-4 .. 2^12 inside fp16's range: the split planes scale exactly, so the
    result equals the unscaled network's to the last bits, and the fp32 oracle on the rescaled weights agrees at the usual bound."""
    base = _base_sd()
    x, ts, c = _inputs(B, T)
    m0 = _make(base, dev)
    y0 = _fwd(m0, dev, x, ts, c)
    del m0
    sd = _rescaled(base, **kw)
    m = _make(sd, dev)
    eng = m._get_engine(max(B, 2), max(T, 64))
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # no overflow, no retry
        y = _fwd(m, dev, x, ts, c)
    assert eng.effective_precision() == "fp32" and eng.numeric_status() == (-1, False)
    ref = _oracle(sd, x, ts, c)
    e_self, e_ref = _rel(y, y0), _rel(y, ref)
    print(f"{kw} B={B} T={T}: vs the unscaled network {e_self:.2e}, vs the oracle on the rescaled weights {e_ref:.2e} (of range)")
    assert e_self <= 2e-6 and e_ref <= 1e-4


# Weights stay inside [2^-14, 2^15) (a compensating pair 2^k / 2^-k leaves it from k = 13 on), the ACTIVATION leaves fp16's range: the LayerNorm in front of the
# product is given a gain of 2^5 on top (norm1 / norm3: uncompensated, the oracle evaluates the same weights), or the unscanned fp32 K / V projection carries the scale.
@pytest.mark.parametrize("kw,what", [(dict(k_v=11, blocks=ST[1:2], extra={"norm1.weight": 5, "norm1.bias": 5, "attn1.to_q.weight": -5, "attn1.to_k.weight": -5}),
                                       "self-attention v / attention output past 65504 (attn PM 2/3, stchain to_out1)"),
                                      (dict(k_ff=11, blocks=ST[2:3], extra={"norm3.weight": 5, "norm3.bias": 5}), "GEGLU product past 65504 (stchain folded proj_out)"),
                                      (dict(k_v2=11, blocks=ST[0:1], extra={"attn2.to_v.weight": 5}), "cross-attention v past 65504 (stchain window tile)"),
                                      (dict(k_v=17, blocks=ST[3:4]), "to_v x 2^17: the weight tensor itself leaves the range")],
                         ids=["attn1_v", "geglu", "attn2_v", "weights"])
def test_operand_beyond_the_split_domain_is_detected_and_rerun_in_strict_fp32(dev, kw, what):
    """|operand| >= 65504: never a silent inf / NaN / clamp.  Either the weight scan already put the context in strict fp32, or the step's last kernel records the
    non-finite model output and the host wrapper evaluates again on fp32 matrix instructions; `raise` raises; `ignore` returns the non-finite output as it is."""
    from said_amd import _engine
    base = _base_sd()
    sd = _rescaled(base, **kw)
    x, ts, c = _inputs(2, 60)
    ref = _oracle(sd, x, ts, c)
    assert bool(torch.isfinite(ref).all()), "the fp32 reference itself must be fine for this case to mean anything"
    m = _make(sd, dev)
    eng = m._get_engine(2, 64)
    by_weights = eng.effective_precision() == "fp32_strict"
    print(f"{what}: weight scan says {eng.precision_note() or 'in range'}")
    if by_weights:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            y = _fwd(m, dev, x, ts, c)
    else:
        with pytest.warns(RuntimeWarning, match="not finite"):
            y = _fwd(m, dev, x, ts, c)
        m.on_nonfinite = "raise"
        with pytest.raises(_engine.EngineError, match="fp32_strict"):
            _fwd(m, dev, x, ts, c)
        m.on_nonfinite = "ignore"
        assert not bool(torch.isfinite(_fwd(m, dev, x, ts, c)).all())
        assert eng.numeric_status()[1] is True
        m.on_nonfinite = "strict_retry"
    e = _rel(y, ref)
    print(f"  after the guard: {e:.2e} of range vs the oracle")
    assert bool(torch.isfinite(y).all()) and e <= 1e-4

    # the loop: same guard around SAID.inference, same random draws in the second attempt
    lat = synth.synth_latents(3, (2, 60, 32))
    emb = synth.synth_latents(4, (2, 60, 768)).to(dev)
    wav = torch.zeros(2, 16000, device=dev)
    kwi = dict(num_inference_steps=3, guidance_scale=2.0, eta=0.0, init_latents=lat.to(dev), audio_embedding=emb)
    if by_weights:
        got = m.inference(wav, **kwi).result.cpu()
    else:
        with pytest.warns(RuntimeWarning, match="not finite"):
            got = m.inference(wav, **kwi).result.cpu()
    m.set_mfma_dtype("fp32_strict")
    want = m.inference(wav, **kwi).result.cpu()
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want), "the retry is the strict-fp32 run on the same draws"


@pytest.mark.parametrize("kw", [dict(k_ff=-20), dict(k_qk=20), dict(k_v=-20, k_v2=-20)], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_weights_below_the_split_resolution_run_strict_fp32(dev, kw):
    """A weight tensor scaled to 2^-20 of its size (its partner to 2^20): h and l would both be fp16 denormals (2^-14 relative instead of 2^-22).  The
    weight scan at said_finalize_weights sees it and the context runs on fp32 matrix instructions; the result is the fp32 reference's."""
    base = _base_sd()
    sd = _rescaled(base, **kw)
    x, ts, c = _inputs(2, 60)
    ref = _oracle(sd, x, ts, c)
    m = _make(sd, dev)
    eng = m._get_engine(2, 64)
    assert eng.get_precision() == "fp32" and eng.effective_precision() == "fp32_strict"
    assert "outside [2^-14, 2^15)" in eng.precision_note()
    n0 = eng.debug_get("n_stchain")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y = _fwd(m, dev, x, ts, c)
    assert eng.debug_get("n_stchain") == n0
    e = _rel(y, ref)
    print(f"{kw}: {eng.precision_note()} -> {e:.2e} of range vs the oracle")
    assert e <= 1e-4


def test_small_activations_inside_the_weight_range(dev):
    """The documented floor: with every weight tensor still >= 2^-14 at its largest element, q = 2^-9 x its usual size is split with most elements below 2^-14 —
    the pair still resolves 2^-36 absolute, 2^-22 of the tensor's scale.  (to_q x 2^-9, to_k x 2^9; v and the GEGLU product likewise.)"""
    base = _base_sd()
    kw = dict(k_qk=9, k_v=-9, k_ff=-9, k_v2=-9)
    sd = _rescaled(base, **kw)
    x, ts, c = _inputs(2, 600)
    m = _make(sd, dev)
    eng = m._get_engine(2, 640)
    assert eng.effective_precision() == "fp32", eng.precision_note()
    y = _fwd(m, dev, x, ts, c)
    ref = _oracle(sd, x, ts, c)
    e = _rel(y, ref)
    print(f"{kw}: {e:.2e} of range vs the oracle")
    assert e <= 1e-4


def _f64_truth(sd, x, ts, c):
    """The oracle's op sequence in float64 on the same fp32 inputs and weights (its `.float()` casts redirected)."""
    from unittest import mock
    _, sd_u, _ = op.split_state_dict(sd)
    sd64 = {k: v.double() for k, v in sd_u.items()}
    with mock.patch.object(torch.Tensor, "float", torch.Tensor.double):
        return ou.unet1d_forward(sd64, x.double(), ts, c.double())


@pytest.mark.parametrize("B,T", [(2, 600), (3, 37), (16, 600)])
def test_trained_like_weight_statistics_through_the_unet(dev, B, T):
    """Heavy-tailed weights, outlier rows / columns (x 8), GroupNorm / LayerNorm gains up to 10 (synth.trained_like_state_dict): activations of O(100) on the
    un-normalised residual streams, and a network that is badly conditioned in fp32 — the fp32 ORACLE itself sits ~1e-3 of the output range from the float64
    evaluation of the same weights.  So the yardstick is float64, and the statement is relative: split-fp16 mode and strict fp32 are each no further from it
    than twice the fp32 oracle is, and split-fp16 no further than 1.5 x strict fp32.  bf16 mode is printed and bounded loosely.
    B = 16 runs the large-batch schedules (fgemm + stchain / rgemm + battn)."""
    sd = synth.trained_like_state_dict(num_w2v_layers=2)
    x, ts, c = _inputs(B, T, seed=11)
    n = min(B, 2)
    truth = _f64_truth(sd, x[:n], ts[:n], c[:n])
    rng = float(truth.max() - truth.min())
    e_oracle = float((_oracle(sd, x[:n], ts[:n], c[:n]).double() - truth).abs().max()) / rng
    m = _make(sd, dev)
    res = {}
    for mode in ("fp32", "fp32_strict", "bf16"):
        m.set_mfma_dtype(mode)
        eng = m._get_engine(max(B, 2), max(T, 64))
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            y = _fwd(m, dev, x, ts, c)[:n].double()
        assert eng.effective_precision() == mode and eng.numeric_status() == (-1, False)
        res[mode] = (float((y - truth).abs().max()) / rng, float(((y - truth) ** 2).mean().sqrt()) / rng)
    print(f"trained-like fill B={B} T={T} (|truth| max {float(truth.abs().max()):.1f}), of range vs float64: fp32 oracle max {e_oracle:.2e}; " +
          ", ".join(f"{k} max {v[0]:.2e} rms {v[1]:.2e}" for k, v in res.items()))
    assert res["fp32"][0] <= 2.0 * e_oracle + 1e-5 and res["fp32_strict"][0] <= 2.0 * e_oracle + 1e-5
    assert res["fp32"][0] <= 1.5 * res["fp32_strict"][0] + 1e-5, "split-fp16 products are no worse than the fp32 matrix instructions on these statistics"
    assert res["bf16"][0] <= 8e-2 and res["bf16"][1] <= 1e-2


def test_trained_like_guided_steps_split_vs_strict(dev):
    """Guided DDIM steps on the trained-like fill through the loop (shared prefix, fused scheduler), split-fp16 mode against strict fp32 from the same latents:
    1 and 2 steps (teacher-forced in effect).  A longer free-running chain of THIS network is chaotic — ten steps part by O(1) between any two fp32
    evaluations (measured: 1.0 on [0, 1]) — so nothing is claimed about it (DESIGN.md 7.2 says the same of the plain fill after 200 steps)."""
    sd = synth.trained_like_state_dict(num_w2v_layers=2)
    m = _make(sd, dev)
    lat = synth.synth_latents(5, (2, 60, 32)).to(dev)
    emb = synth.synth_latents(6, (2, 60, 768)).to(dev)
    wav = torch.zeros(2, 16000, device=dev)
    for n, bound in ((1, 1e-4), (2, 2e-3)):
        kwi = dict(num_inference_steps=n, guidance_scale=2.0, eta=0.0, init_latents=lat, audio_embedding=emb)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            m.set_mfma_dtype("fp32")
            a = m.inference(wav, **kwi).result.cpu()
            m.set_mfma_dtype("fp32_strict")
            b = m.inference(wav, **kwi).result.cpu()
        d = float((a - b).abs().max())
        print(f"trained-like fill, {n} guided step(s): split vs strict {d:.2e} abs on [0, 1]")
        assert d <= bound


# ---------------------------------------------------------------- the fused tail as two / three workgroups per token tile (stchain.hip CU<>)
@pytest.mark.parametrize("B,T,slices", [(2, 600, 3), (1, 37, 3), (3, 333, 3), (4, 600, 3), (2, 1800, 2), (5, 600, 2), (8, 600, 1)])
def test_sliced_tail_matches_one_workgroup_per_tile_and_is_bit_reproducible(dev, B, T, slices):
    """Small launches run the fused SpatialTransformer tail as three (<= 85 (sample, tile) pairs) or two (<= 128) workgroups per token tile, each with a third / half
    of the GEGLU / folded proj_out weights; the partial sums meet in memory and are added in slice order by whichever wave arrives last.  Against the one-workgroup
    kernel (said_debug_option "st_chain_slices" = 1): only the folded proj_out's K is summed in pieces (<= 1e-6 of range); repeated runs are bit-identical (the
    arrival order must not show); larger launches keep one workgroup per tile.  Where three slices run, two are checked as well (option value 2)."""
    sd = _base_sd()
    m = _make(sd, dev)
    x, ts, c = _inputs(B, T, seed=21)
    eng = m._get_engine(max(B, 2), max(T, 64))
    n0 = eng.debug_get("n_stchain")
    ys = [_fwd(m, dev, x, ts, c) for _ in range(4)]
    assert eng.debug_get("n_stchain") - n0 == 16
    for k in range(1, 4):
        assert torch.equal(ys[0], ys[k]), f"run {k} differs: {float((ys[0] - ys[k]).abs().max()):.3e}"
    variants = {}
    for opt in ((1, 2) if slices == 3 else (1,)):
        eng.debug_option("st_chain_slices", opt)
        try:
            variants[opt] = _fwd(m, dev, x, ts, c)
        finally:
            eng.debug_option("st_chain_slices", -1)
    y1 = variants[1]
    ref = _oracle(sd, x, ts, c)
    e_s1, e_s, e_1 = _rel(ys[0], y1), _rel(ys[0], ref), _rel(y1, ref)
    print(f"B={B} T={T}: {slices} slice(s) vs one workgroup {e_s1:.2e}; vs oracle {e_s:.2e} / {e_1:.2e} (of range)" +
          (f"; forced two slices vs one {_rel(variants[2], y1):.2e}" if 2 in variants else ""))
    assert e_s1 <= 1e-6 and e_s <= 1e-4 and e_1 <= 1e-4
    assert (e_s1 > 0) == (slices > 1), "sliced exactly where the launch is at most 128 tiles"
    if 2 in variants:
        assert 0 < _rel(variants[2], y1) <= 1e-6 and not torch.equal(variants[2], ys[0])


def test_three_slice_tail_in_the_guided_loop_is_bit_reproducible(dev):
    """The loop's schedule (shared prefix: one workgroup row feeds both guidance halves; unconditional samples skip the cross-attention) on the three-slice
    kernel: 12 steps twice from the same draws, bit-identical, and within the loop bound of the one-workgroup schedule."""
    sd = _base_sd()
    m = _make(sd, dev)
    lat = synth.synth_latents(7, (1, 600, 32)).to(dev)
    emb = synth.synth_latents(8, (1, 600, 768)).to(dev)
    wav = torch.zeros(1, 160000, device=dev)
    kwi = dict(num_inference_steps=12, guidance_scale=2.0, eta=0.0, init_latents=lat, audio_embedding=emb)
    a = m.inference(wav, **kwi).result.cpu()
    b = m.inference(wav, **kwi).result.cpu()
    assert torch.equal(a, b)
    eng = m._get_engine(2, 640)
    eng.debug_option("st_chain_slices", 1)
    try:
        c1 = m.inference(wav, **kwi).result.cpu()
    finally:
        eng.debug_option("st_chain_slices", -1)
    d = float((a - c1).abs().max())
    print(f"three slices vs one workgroup after 12 guided steps: {d:.2e} abs on [0, 1]")
    assert d <= 1e-4


# ---------------------------------------------------------------- fp32 large batches: fgemm_kernel's operands arrive split
def test_presplit_operands_of_the_large_batch_gemms_are_bit_identical(dev):
    """fp32 mode from 10000 UNet rows per launch on: prep_kernel writes the ResBlock convolutions' and q / k / v's activations as packed split-fp16 pairs (h | l << 16) and the
    weights have a packed copy, so fgemm_kernel<SP> unpacks with v_perm instead of converting in its k loop.  Same planes, same products: bit-identical to the in-kernel split
    (said_debug_option "gemm_presplit" = 0), and the usual bound against the oracle.  B = 20: 12000 rows, two ragged lengths."""
    sd = _base_sd()
    m = _make(sd, dev)
    for B, T in ((20, 600), (34, 333)):
        x, ts, c = _inputs(B, T, seed=31)
        eng = m._get_engine(B, max(T, 64))
        assert eng.debug_get("gemm_split") == 1
        y1 = _fwd(m, dev, x, ts, c)
        eng.debug_option("gemm_presplit", 0)
        try:
            y0 = _fwd(m, dev, x, ts, c)
        finally:
            eng.debug_option("gemm_presplit", -1)
        assert torch.equal(y0, y1), f"B={B} T={T}: {float((y0 - y1).abs().max()):.3e}"
        for i in (0, B - 1):
            ref = _oracle(sd, x[i:i + 1], ts[i:i + 1], c[i:i + 1])
            e = _rel(y1[i:i + 1], ref)
            print(f"pre-split operands B={B} T={T} sample {i}: {e:.2e} of range vs the oracle")
            assert e <= 1e-4


def test_presplit_kv_for_the_large_batch_attention_is_bit_identical(dev):
    """Large batches: the token-major q/k/v GEMM stores k and v as packed split pairs and the four-query-tile attention (attn_kernel<1, 1, 3, 4>) unpacks them instead of
    every wave splitting all of K and V for itself; so does the key-split attention of the guidance-shared first block.  Same planes: bit-identical to "attn_presplit" = 0."""
    sd = _base_sd()
    m = _make(sd, dev)
    for B, T in ((20, 600), (34, 333)):
        x, ts, c = _inputs(B, T, seed=41)
        eng = m._get_engine(B, max(T, 64))
        y1 = _fwd(m, dev, x, ts, c)
        eng.debug_option("attn_presplit", 0)
        try:
            y0 = _fwd(m, dev, x, ts, c)
        finally:
            eng.debug_option("attn_presplit", -1)
        assert torch.equal(y0, y1), f"B={B} T={T}: {float((y0 - y1).abs().max()):.3e}"
        ref = _oracle(sd, x[:1], ts[:1], c[:1])
        e = _rel(y1[:1], ref)
        print(f"pre-split K / V, large batch B={B} T={T}: {e:.2e} of range vs the oracle")
        assert e <= 1e-4
    # a guided loop step at 12 clips (24 samples: the shared first block runs the key-split attention on 12): same statement through the loop
    lat = synth.synth_latents(9, (12, 600, 32)).to(dev)
    emb = synth.synth_latents(10, (12, 600, 768)).to(dev)
    wav = torch.zeros(12, 160000, device=dev)
    kwi = dict(num_inference_steps=2, guidance_scale=2.0, eta=0.0, init_latents=lat, audio_embedding=emb)
    m.clip_groups = 1
    a = m.inference(wav, **kwi).result.cpu()
    eng = m._get_engine(24, 640)
    eng.debug_option("attn_presplit", 0)
    try:
        b = m.inference(wav, **kwi).result.cpu()
    finally:
        eng.debug_option("attn_presplit", -1)
    assert torch.equal(a, b)


# ---------------------------------------------------------------- the K-long ResBlock convolutions of the up path as straight-line blocks (gemm_lds.hip kconv_body)
@pytest.mark.parametrize("B,T,same_shape", [(2, 600, True), (1, 37, True), (3, 333, True), (5, 64, True), (2, 1800, False), (6, 600, False)])
def test_kconv_matches_the_block_loop(dev, B, T, same_shape):
    """The two- / three-segment convolutions of the up path (in_layers over [h ; skip]; out_layers + the 1x1 skip convolution) run on kconv_body in fp32 mode at small
    batch: every block of a wave requested up front, staged and multiplied as straight-line code.  Same weights, same order per accumulator, same reduction order as
    ugemm_body's block loop (said_debug_option "kconv" = 0): where both run one column tile per workgroup the UNet output is bit-identical.  Mid-size launches
    (configs[4]; 3-8 clips) used to run these convolutions with two column tiles per workgroup on the fp32 matrix instructions (no split shape exists for those) and now
    take kconv_body's shape when its rounds are no more than 1.5 x as many: there the two differ by the products' rounding.  Both sit at the oracle's distance."""
    sd = _base_sd()
    m = _make(sd, dev)
    x, ts, c = _inputs(B, T, seed=33)
    eng = m._get_engine(max(B, 2), max(T, 64))
    y = _fwd(m, dev, x, ts, c)
    eng.debug_option("kconv", 0)
    try:
        y0 = _fwd(m, dev, x, ts, c)
    finally:
        eng.debug_option("kconv", -1)
    y2 = _fwd(m, dev, x, ts, c)
    e, e0 = _rel(y, _oracle(sd, x, ts, c)), _rel(y, y0)
    print(f"B={B} T={T}: kconv vs block loop {e0:.2e} of range (max |diff| {float((y - y0).abs().max()):.3e}); vs oracle {e:.2e} of range")
    assert torch.equal(y, y2)
    if same_shape:
        assert torch.equal(y, y0)
    else:
        assert 0 < e0 <= 2e-6
    assert e <= 1e-4


# ---------------------------------------------------------------- long sequences: two / three query tiles per wave (attn.hip attn2q_kernel)
@pytest.mark.parametrize("B,T,opt", [(2, 1800, -1), (1, 1801, 1), (1, 1000, 1), (2, 600, 1), (3, 333, 1), (1, 37, 1)])
def test_several_query_tiles_per_wave_are_bit_identical(dev, B, T, opt):
    """Self-attention over pre-split K / V with a wave keeping the states of three consecutive query tiles and running them against every K / V fragment it fetches
    (configs[4]'s shape by default: launches of >= 512 (sample, head, tile) triples).  Same key tiles per wave, same per-tile arithmetic, same merge as one tile per
    wave ("attn_2q" = 0): the UNet output is bit-identical — also where the last workgroup's extra tiles are phantoms (57 tiles in threes is exact; 32, 19 and 11
    tiles leave one or two over, 2 tiles are one workgroup with a phantom)."""
    sd = _base_sd()
    m = _make(sd, dev)
    x, ts, c = _inputs(B, T, seed=35)
    eng = m._get_engine(max(B, 2), max(T, 64))
    eng.debug_option("attn_2q", 0)
    try:
        y0 = _fwd(m, dev, x, ts, c)
        eng.debug_option("attn_2q", opt)
        y = _fwd(m, dev, x, ts, c)
    finally:
        eng.debug_option("attn_2q", -1)
    e = _rel(y, _oracle(sd, x, ts, c)) if T <= 600 else 0.0
    print(f"B={B} T={T} attn_2q={opt}: max |diff| to one tile per wave {float((y - y0).abs().max()):.3e}" + (f"; vs oracle {e:.2e} of range" if T <= 600 else ""))
    assert torch.equal(y, y0)
    assert e <= 1e-4


# ---------------------------------------------------------------- the sliced fused tail takes the block input's GroupNorm coefficients from the q/k/v GEMM
@pytest.mark.parametrize("B,T", [(2, 600), (1, 37), (3, 333), (2, 1800)])
def test_sliced_tail_reads_the_groupnorm_coefficients_the_qkv_gemm_finalised(dev, B, T):
    """A SpatialTransformer's q/k/v GEMM normalises the block input (GroupNorm -> LayerNorm) and so finalises its GroupNorm coefficients; the fused tail needs the same
    coefficients for the residual of attn1.to_out.  The GEMM's first workgroup per sample stores them and the sliced stchain kernels read them (1 load per wave instead
    of 23, no finalisation in front of the first barrier).  With "chain_coef" = 0 the GEMM does not export and a gn_coef_kernel launch makes them instead (the fall-back
    for a q/k/v GEMM that took another kernel): the two finalisations sum a channel's tiles in different groupings — 1e-6 of range apart, both at the oracle's distance."""
    sd = _base_sd()
    m = _make(sd, dev)
    x, ts, c = _inputs(B, T, seed=37)
    eng = m._get_engine(max(B, 2), max(T, 64))
    y = _fwd(m, dev, x, ts, c)
    eng.debug_option("chain_coef", 0)
    try:
        y0 = _fwd(m, dev, x, ts, c)
    finally:
        eng.debug_option("chain_coef", -1)
    y2 = _fwd(m, dev, x, ts, c)
    e0 = _rel(y, y0)
    e = _rel(y, _oracle(sd, x, ts, c)) if T <= 600 else 0.0
    print(f"B={B} T={T}: coefficients from the q/k/v GEMM vs a gn_coef_kernel launch: {e0:.2e} of range; vs oracle {e:.2e}")
    assert torch.equal(y, y2)
    assert e0 <= 1e-6 and e <= 1e-4


# ---------------------------------------------------------------- bf16 audio encoder: the projections on the direct-to-LDS 256 x 256 tile (tgemm.hip tgemm256d_kernel)
@pytest.mark.parametrize("B,Ta", [(32, 160000), (9, 16000 * 3), (40, 16000)])
def test_direct_to_lds_gemm_tile_is_bit_identical_to_the_staged_tiles(dev, B, Ta):
    """bf16 mode's audio encoder runs its q/k/v, out_proj and feed-forward projections (where a pass has >= 4096 rows) on tgemm256d_kernel: 256 x 256 x 64 tiles whose
    operand tiles go global -> LDS directly (XOR-swizzled 16-byte chunks, one barrier per k-tile).  Same operands, same k order per accumulator as tgemm_kernel<128, 128>
    (said_debug_option "tgemm_direct" = 0): the embedding is bit-identical — rows past the last tile boundary (499 / 149 / 49 frames per clip), a 40-clip batch in two
    passes; and it stays at the oracle's bf16 distance (tests/test_gpu_parity.py::test_bf16_audio_encoder_vs_fp32_oracle runs on it: it is the default)."""
    m = _make(_base_sd(), dev)   # (two encoder layers: eight projection GEMMs per pass)
    F = int(Ta / 16000 * 60)
    proc = op.process_audio([synth.synth_waveform(700 + i, Ta).numpy() for i in range(B)]).to(dev)
    eng = m._get_engine(2, 64)
    try:
        m.set_mfma_dtype("bf16")
        y1 = m.get_audio_embedding(proc, F).cpu()
        eng.debug_option("tgemm_direct", 0)
        y0 = m.get_audio_embedding(proc, F).cpu()
    finally:
        eng.debug_option("tgemm_direct", -1)
        m.set_mfma_dtype("fp32")
    print(f"B={B} Ta={Ta}: direct-to-LDS tile vs staged tiles max |diff| {float((y1 - y0).abs().max()):.3e} (|y| max {float(y0.abs().max()):.2f})")
    assert torch.isfinite(y1).all() and torch.equal(y1, y0)


# ---------------------------------------------------------------- fifty steps per graph in long loops
def test_long_loop_graph_segmentation_does_not_change_the_result(dev):
    """Loops of >= 400 steps capture FIFTY steps per hipGraph (shorter ones ten: the first graph's host-side enqueue is exposed there): a 457-step guided loop as
    9 x 50 + 7, as 45 x 10 + 7 (said_debug_option "steps_per_graph" = 10) and as 3 x 128 + 73 gives bit-identical results, with eta noise from the step counter."""
    m = _make(_base_sd(), dev)
    lat = synth.synth_latents(7, (1, 60, 32)).to(dev)
    emb = synth.synth_latents(8, (1, 60, 768)).to(dev)
    wav = torch.zeros(1, 16000, device=dev)
    res = {}
    eng = m._get_engine(2, 64)
    for spg in (50, 10, 128):
        eng.debug_option("steps_per_graph", spg)
        try:
            torch.manual_seed(5)
            res[spg] = m.inference(wav, num_inference_steps=457, guidance_scale=2.0, eta=0.5, init_latents=lat, audio_embedding=emb).result.cpu()
        finally:
            eng.debug_option("steps_per_graph", 50)
    assert torch.isfinite(res[50]).all()
    assert torch.equal(res[50], res[10]) and torch.equal(res[50], res[128])
