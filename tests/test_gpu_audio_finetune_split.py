"""The fine-tuning step with the encoder's dense products on split-fp16 operands (UNetTrainer(encoder_products="split_fp16"),
said_amd/csrc/said_unet_train_products.h, enc_gemm.hip) against the float64 restatement of the step, tests/audio_ft_ref.py,
with the batches, shapes (2-layer encoders, B = 2, T = 19 and 150) and helpers of tests/test_gpu_audio_finetune.py.

Tolerance rule: that file's form, per tensor rel = |a - b|_2 / |b|_2 <= C x max(rel(fp32 restatement, fp64 restatement), 1e-6), and the same
for the scalar losses.  C starts from the project's 4: the split operands carry 22 significand bits and the emulation (tests/enc_split_ref.py)
puts their error at a fifth of an fp32 product's own accumulation error.  Every case prints its worst ratio and the tensor closest to its
bound.  Measured on the MI355X, 4 holds: the worst ratio is 3.09 (v_prediction + std + vertex, denoiser.model.output_blocks.1.0.emb_layers.1.weight,
3.09e-6 against the CPU's 0.92e-6); gradients eval 2.85 / 2.72 (T = 19 / 150), train 2.84 / 2.74, unconditional 2.56, F = 64 2.41, always a
denoiser tensor; forward output 1.28 / 1.17, conditioning 0.36 ... 0.50; three steps 0.05 ... 0.40.  An exactly zero
float64 tensor must be exactly zero here too.
"""
import os

import numpy as np
import pytest
import torch

from said_amd import _engine
from said_amd.model.wav2vec2 import AudioConfig, AudioTrainConfig
from said_amd.training import UNetTrainer, trainable_shapes
from said_amd.util.synth import said_state_dict, synth_waveform
import audio_ft_ref as aft
import audio_train_ref as atr
import test_gpu_audio_finetune as ftm
from test_gpu_audio_finetune import cli_data, ref_three_steps, refs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ROOT, DEV, L, B, P, ENC, SEED = ftm.ROOT, ftm.DEV, ftm.L, ftm.B, ftm.P, ftm.ENC, ftm.SEED
C = 4   # the bound's factor (the module's docstring)


def make(fd=-1, prediction_type="epsilon", **kw):
    return UNetTrainer(ftm.full_sd(fd), DEV, max_batch=B, max_frames=max(ftm.LENGTHS), learning_rate=1e-3, num_warmup_steps=4, dropout=P, feature_dim=fd,
                       finetune_audio_layers=L, prediction_type=prediction_type, **kw)


@pytest.fixture(scope="module")
def trainers():
    """One split-mode trainer per (feature_dim, prediction type), made on first use."""
    made = {}

    def get(fd=-1, prediction_type="epsilon"):
        key = (fd, prediction_type)
        if key not in made:
            made[key] = make(fd, prediction_type, encoder_products="split_fp16")
            assert made[key].encoder_products == "split_fp16" and made[key].eng.encoder_products() == "split_fp16"
        return made[key]

    yield get
    for t in made.values():
        t.close()


def held(what, name, got, r32, r64):
    e32, e = ftm.rel(r32, r64), ftm.rel(got, r64)
    ratio = e / max(e32, 1e-6)
    print(f"{what}: {name} split {e:.3e} cpu-fp32 {e32:.3e} ratio {ratio:.2f} (bound {C})")
    return ratio


def check_all(what, got, a32, a64):
    """Every tensor of a64 under the bound (an exactly zero float64 tensor: exactly zero here); prints the one closest to its bound."""
    ratios, bad = {}, []
    for k in a64:
        if float(a64[k].abs().max()) == 0:
            if float(got[k].abs().max()) != 0:
                bad.append((k, "not exactly zero", float(got[k].abs().max())))
            continue
        e32, e = ftm.rel(a32[k], a64[k]), ftm.rel(got[k], a64[k])
        ratios[k] = (e / max(e32, 1e-6), e, e32)
        if ratios[k][0] > C:
            bad.append((k,) + ratios[k])
    k = max(ratios, key=lambda n: ratios[n][0])
    print(f"{what}: {len(ratios)} tensors compared, closest to its bound {k} ratio {ratios[k][0]:.2f} split {ratios[k][1]:.3e} cpu-fp32 {ratios[k][2]:.3e}; "
          f"failing {len(bad)}")
    return bad


def loss_ok(got, l32, l64):
    return abs(float(got) - float(l64)) <= C * max(abs(float(l32) - float(l64)), 1e-6 * abs(float(l64)))


# ---------------------------------------------------------------------------------------------------------------- the forward
@pytest.mark.parametrize("T", ftm.LENGTHS)
def test_forward_eval(trainers, T):
    tr, d = trainers(), ftm.batch(T)
    tr.load_state_dict(ftm.full_sd())
    x = d["coeffs"] + 0.3 * d["noise"]
    got = tr.forward_only(x, d["timesteps"], d["cond"], d["feats"])
    cond_rows = torch.from_numpy(tr.eng.last_conditioning(B, T))
    with torch.no_grad():
        (r64, c64), (r32, c32) = ((aft.forward(ftm.trainable(-1, dt), x, d["timesteps"], d["feats"], d["cond"]),
                                   aft.conditioning(ftm.trainable(-1, dt), d["feats"])) for dt in (torch.float64, torch.float32))
    for name, g, a32, a64 in (("output", got, r32, r64), ("conditioning", cond_rows[0], c32[0], c64[0])):
        assert held(f"forward eval T={T}", name, g, a32, a64) <= C
    assert torch.equal(cond_rows[1], ftm.full_sd()["null_cond_emb"][0].expand(T, -1))


@pytest.mark.parametrize("T", ftm.LENGTHS)
def test_forward_train(trainers, T):
    tr, d = trainers(), ftm.batch(T)
    enc, draws = ftm.train_enc(T)
    tr.load_state_dict(ftm.full_sd())
    tr.step(d["coeffs"], [True, True], d["feats"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED, audio_draws=draws, audio_cfg=AudioTrainConfig())
    got = torch.from_numpy(tr.eng.last_conditioning(B, T))
    with torch.no_grad():
        c64, c32 = (aft.conditioning(ftm.trainable(-1, dt), d["feats"], enc) for dt in (torch.float64, torch.float32))
    assert held(f"forward train T={T}", "conditioning", got, c32, c64) <= C


# ---------------------------------------------------------------------------------------------------------------- the gradients
def grads_case(trainers, refs, what, T, fd=-1, prediction_type="epsilon", **kw):
    (l64, g64), (l32, g32) = refs(T, fd, prediction_type=prediction_type, **kw)
    out, g = ftm.gpu_grads(trainers(fd, prediction_type), T, **kw)
    assert loss_ok(out.predict, l32[0], l64[0]) and loss_ok(out.velocity, l32[1], l64[1]), (out, l32, l64)
    if kw.get("V"):
        assert loss_ok(out.vertex, l32[2], l64[2])
    assert list(g) == list(g64) == list(trainable_shapes(fd, L))
    bad = check_all(what, g, g32, g64)
    assert not bad, bad[:8]
    return g, g64


@pytest.mark.parametrize("T", ftm.LENGTHS)
def test_gradients_eval(trainers, refs, T):
    """All 203 gradients; without a mask masked_spec_embed's is exactly zero."""
    g, g64 = grads_case(trainers, refs, f"gradients eval T={T}", T)
    assert len(g) == 203
    assert float(g[ENC + "masked_spec_embed"].abs().max()) == 0 and float(g64[ENC + "masked_spec_embed"].abs().max()) == 0
    assert all(float(g[k].abs().max()) > 0 for k in g if k != ENC + "masked_spec_embed" and not k.endswith("k_proj.bias"))


@pytest.mark.parametrize("T", ftm.LENGTHS)
def test_gradients_train(trainers, refs, T):
    """Train mode with a mask and layer 1 skipped: the skipped layer's sixteen gradients are exactly 0.0."""
    g, g64 = grads_case(trainers, refs, f"gradients train T={T}", T, mode="train", p=P)
    skipped = [k for k in g if ".layers.1." in k]
    assert len(g) == 203 and len(skipped) == 16 and all(float(g[k].abs().max()) == 0 for k in skipped)
    assert float(g64[ENC + "masked_spec_embed"].abs().max()) > 0 and float(g[ENC + "masked_spec_embed"].abs().max()) > 0


def test_gradients_unconditional_batch(trainers, refs):
    """cond = [0, 0]: an all-zero gradient operand takes scale 1, and every audio_encoder.* gradient is exactly 0.0."""
    g, g64 = grads_case(trainers, refs, "gradients cond = [0, 0]", 19, cond=[False, False])
    enc = [k for k in g if k.startswith(ENC)]
    assert len(enc) == 42 and all(float(g[k].abs().max()) == 0 and float(g64[k].abs().max()) == 0 for k in enc)
    assert float(g["null_cond_emb"].abs().max()) > 0


def test_gradients_feature_dim(trainers, refs):
    g, _ = grads_case(trainers, refs, "gradients F = 64", 19, fd=64, mode="train", p=P)
    assert float(g[ftm.PW].abs().max()) > 0 and float(g[ENC + "encoder.layers.0.attention.q_proj.weight"].abs().max()) > 0


def test_gradients_v_prediction_std_vertex(trainers, refs):
    grads_case(trainers, refs, "gradients v_prediction, std, vertex", 19, prediction_type="v_prediction", V=7)


# ---------------------------------------------------------------------------------------------------------------- clip, update, EMA
def test_joint_clip_and_update(trainers, ref_three_steps):
    """tests/test_gpu_audio_finetune.py's test_joint_clip_and_update in split mode."""
    r64, r32 = ref_three_steps
    tr = trainers()
    norms = ftm.three_steps(tr)
    for k in range(3):
        print("joint gradient norm", k, norms[k], r64.norms[k], r32.norms[k])
        assert abs(norms[k] - r64.norms[k]) <= C * max(abs(r32.norms[k] - r64.norms[k]), 1e-6 * r64.norms[k]), (k, norms[k], r64.norms[k], r32.norms[k])
    bad = []
    for name, which, a64, a32 in (("parameters", _engine.UT_STATE, r64.p, r32.p), ("exp_avg", _engine.UT_EXP_AVG, r64.m, r32.m),
                                  ("exp_avg_sq", _engine.UT_EXP_AVG_SQ, r64.v, r32.v), ("ema", _engine.UT_EMA, r64.ema, r32.ema)):
        got = tr.parameters_of(which)
        for n in ftm.WATCH:
            if held("three steps " + name, n, got[n], a32[n], a64[n]) > C:
                bad.append((name, n))
    assert not bad, bad
    live = tr.parameters_of(_engine.UT_STATE)
    assert all(not torch.equal(live[n], ftm.full_sd()[n]) for n in ftm.WATCH)


def grads_and_params(tr):
    _, g = ftm.gpu_grads(tr, 150, mode="train", p=P)
    ftm.three_steps(tr)
    return g, tr.parameters_of(_engine.UT_STATE)


def same_bits(a, b):
    (g1, p1), (g2, p2) = a, b
    assert len(g1) == len(trainable_shapes(-1, L))
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
        assert torch.equal(p1[k], p2[k]), k


def test_determinism():
    """Two fresh contexts and a repetition on the first: every gradient after one step and every parameter after three, bit for bit."""
    one, two = make(encoder_products="split_fp16"), make(encoder_products="split_fp16")
    try:
        first = grads_and_params(one)
        same_bits(first, grads_and_params(two))
        same_bits(first, grads_and_params(one))
    finally:
        one.close()
        two.close()


def test_modes_switch_and_default():
    """A context switched to split and back gives the bits of one never switched; encoder_products="fp32" those of the argument left out;
    split mode gives other bits than either."""
    never, given, switched = make(), make(encoder_products="fp32"), make()
    try:
        assert never.encoder_products == given.encoder_products == "fp32" and never.eng.encoder_products() == given.eng.encoder_products() == "fp32"
        want = grads_and_params(never)
        same_bits(want, grads_and_params(given))
        switched.eng.set_encoder_products("split_fp16")
        split = grads_and_params(switched)
        q = ENC + "encoder.layers.0.attention.q_proj.weight"
        assert not torch.equal(split[0][q], want[0][q]) and not torch.equal(split[1][q], want[1][q])
        switched.eng.set_encoder_products("fp32")
        same_bits(want, grads_and_params(switched))
    finally:
        for t in (never, given, switched):
            t.close()


def test_refusals():
    frozen = UNetTrainer(ftm.full_sd(), DEV, max_batch=B, max_frames=19)
    try:
        with pytest.raises(_engine.EngineError, match="no fine-tuned encoder"):
            frozen.eng.set_encoder_products("split_fp16")
        assert frozen.encoder_products == "fp32"
    finally:
        frozen.close()
    for mode in ("split_fp16", "fp32"):
        with pytest.raises(ValueError, match="encoder_products"):
            UNetTrainer(ftm.full_sd(), DEV, max_batch=B, max_frames=19, encoder_products=mode)
    with pytest.raises(ValueError, match="encoder_products"):
        make(encoder_products="bf16")


# ---------------------------------------------------------------------------------------------------------------- the checkpoint
def test_checkpoint(trainers):
    """The inference engine's get_audio_embedding on weights trained three steps in split mode against the trainer's conditioning, within
    4 x the inference engine's own distance from the float64 restatement on the same weights."""
    from said_amd.model.diffusion import SAID_UNet1D
    T = 19
    tr = trainers()
    ftm.three_steps(tr)
    sd = tr.state_dict()
    m = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=L))
    assert list(sd) == list(m.state_dict())
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    wave = torch.stack([synth_waveform(i, 16000 * T // 60) for i in range(B)])
    emb = m.get_audio_embedding(wave.to(DEV), T).cpu()
    feats = m.get_audio_features(wave.to(DEV), T)
    d = ftm.batch(T)
    tr.forward_only(d["coeffs"], d["timesteps"], [True, True], feats)
    mine = torch.from_numpy(tr.eng.last_conditioning(B, T))
    enc = {k[len(ENC):]: v for k, v in sd.items() if k.startswith(ENC)}
    r64 = atr.forward(enc, wave, T, dtype=torch.float64)
    older = ftm.rel(emb, r64)
    print("checkpoint: inference engine vs float64", older, "trainer (split) vs float64", ftm.rel(mine, r64), "trainer vs inference engine", ftm.rel(mine, emb))
    assert ftm.rel(mine, emb) <= 4 * older


# ---------------------------------------------------------------------------------------------------------------- the command line
def test_train_cli_split_products(cli_data):
    import csv
    log = ftm._train_cli(cli_data, "out_ft_split", "--finetune_audio_encoder", "--encoder_products", "split_fp16")
    rows = list(csv.DictReader(log))
    assert len(rows) == 2
    for r in rows:
        assert r["Train/Total Loss"] != ""
        for k, v in r.items():
            if "Loss" in k and v != "":
                assert np.isfinite(float(v)), (k, v)
    sd = torch.load(str(cli_data / "out_ft_split" / "2.pth"), map_location="cpu")
    from said_amd.model.diffusion import SAID_UNet1D
    given = said_state_dict()
    model = SAID_UNet1D()
    assert list(sd) == list(model.state_dict()) and set(sd) == set(given) and all(torch.isfinite(v).all() for v in sd.values())
    model.load_state_dict(sd, strict=True)
    for k, v in given.items():
        if "feature_extractor" in k:
            assert torch.equal(sd[k], v), k
        elif k.startswith(ENC + "encoder."):
            assert not torch.equal(sd[k], v), k


def test_train_cli_refuses_the_products_without_finetuning(cli_data):
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "script", "train.py"), "--audio_dir", str(cli_data / "audio"), "--coeffs_dir",
                        str(cli_data / "coeffs"), "--output_dir", str(cli_data / "out_refused"), "--encoder_products", "split_fp16",
                        "--audio_encoder_weights", "synthetic", "--device", DEV], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "--encoder_products: needs --finetune_audio_encoder" in r.stderr
    assert not os.path.exists(cli_data / "out_refused")
