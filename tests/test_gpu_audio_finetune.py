"""Fine-tuning the Wav2Vec2 transformer with the denoiser on the MI355X (said_amd/csrc/said_unet_finetune.h, audio_ft.hip;
UNetTrainer(finetune_audio_layers=L)) against the float64 restatement of the same step (tests/audio_ft_ref.py: tests/audio_train_ref.py's
differentiable train-mode encoder in front of tests/unet_train_ref.py's step, pinned to the reference's own module by golden G18 in
tests/test_audio_finetune_cpu.py).

Tolerance rule: tests/test_gpu_unet_train.py's.  Per tensor, rel = |a - b|_2 / |b|_2; the HIP result must be within
4 x max(rel(fp32 restatement, fp64 restatement), 1e-6) of the float64 restatement; the same form for scalar losses.  A tensor is left out of
the relative comparison only when its float64 gradient is exactly zero, and then the HIP gradient must be exactly zero too.

Shapes: 2-layer encoders at base widths, B = 2, cond = [1, 0] unless stated; T = 19 (odd, below every tile size, every positional-convolution
window overhangs both ends) and T = 150 (windows wholly inside, partly inside, and the dropped last frame all occur).
"""
import os

import numpy as np
import pytest
import torch

from said_amd import _engine
from said_amd.model.wav2vec2 import AudioConfig, AudioTrainConfig, AudioTrainDraws
from said_amd.training import UNetTrainer, normalize_deltas, trainable_shapes
from said_amd.util.scheduler import constant_with_warmup_lambda, ema_decay
from said_amd.util.synth import fill_tensor, said_state_dict, synth_waveform
import audio_ft_ref as aft
import audio_train_ref as atr
import unet_train_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
L, B = 2, 2
LENGTHS = [19, 150]
SEED, ASEED = 0x1234567887654321, 0x0FEDCBA987654321
P = 0.1
PW, PB = "audio_proj_layer.weight", "audio_proj_layer.bias"
ENC = "audio_encoder."
SKIP = (False, True)   # skip_layers = 0b10
_SD, _AC = {}, []


def full_sd(fd=-1):
    if fd not in _SD:
        sd = said_state_dict(num_w2v_layers=L, ctx_dim=fd if fd > 0 else 768)
        if fd > 0:
            sd[PW], sd[PB] = fill_tensor(PW, (fd, 768)), fill_tensor(PB, (fd,))
        _SD[fd] = sd
    return dict(_SD[fd])


def trainable(fd, dtype):
    sd = full_sd(fd)
    return {k: sd[k].to(dtype) for k in trainable_shapes(fd, L)}


def batch(T, V=0):
    g = torch.Generator().manual_seed(1000 + T)
    d = dict(coeffs=torch.rand(B, T, 32, generator=g), noise=torch.randn(B, T, 32, generator=g), timesteps=torch.tensor([10, 900]),
             cond=[True, False], feats=torch.randn(B, T, 512, generator=g))
    if V:
        d["std"] = 0.5 + torch.rand(32, generator=g)
        d["deltas"] = normalize_deltas(torch.randn(B, 32, V, 3, generator=g))
    return d


def time_mask(T):
    """At least one span per sample; at T = 150 a span reaches the last frame."""
    m = np.zeros((B, T), dtype=bool)
    if T < 40:
        m[0, 3:8], m[1, 10:15] = True, True
    else:
        m[0, 20:30], m[0, 100:110], m[1, 60:70], m[1, T - 4:] = True, True, True, True
    return m


def train_enc(T, mask=True, seed=ASEED):
    """(the restatement's train-mode arguments, the engine's draws) with the published probabilities."""
    m = time_mask(T) if mask else None
    return dict(mask=m, skip=list(SKIP), seed=seed, **aft.PUBLISHED), AudioTrainDraws(mask=m, skip=SKIP, seed=seed)


def alphas():
    if not _AC:
        from said_amd.scheduler import DDIMScheduler
        _AC.append(DDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2").alphas_cumprod.float())
    return _AC[0]


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def check(name, got, r32, r64, worst):
    e32, e = rel(r32, r64), rel(got, r64)
    bound = 4 * max(e32, 1e-6)
    worst[name] = (e, e32)
    return e <= bound, (name, e, e32, bound)


def check_all(what, got, a32, a64):
    """Every tensor of a64 under the bound (an exactly zero float64 tensor: exactly zero here); prints the worst one."""
    worst, bad = {}, []
    for k in a64:
        if float(a64[k].abs().max()) == 0:
            if float(got[k].abs().max()) != 0:
                bad.append((k, "not exactly zero", float(got[k].abs().max())))
            continue
        ok, msg = check(k, got[k], a32[k], a64[k], worst)
        if not ok:
            bad.append(msg)
    k = max(worst, key=lambda n: worst[n][0] / max(worst[n][1], 1e-6))
    print(f"{what}: {len(worst)} tensors compared, closest to its bound {k} hip {worst[k][0]:.3e} cpu-fp32 {worst[k][1]:.3e}; failing {len(bad)}")
    return bad


def loss_ok(got, l32, l64):
    return abs(float(got) - float(l64)) <= 4 * max(abs(float(l32) - float(l64)), 1e-6 * abs(float(l64)))


@pytest.fixture(scope="module")
def trainers():
    """One trainer per (feature_dim, prediction type), made on first use."""
    made = {}

    def get(fd=-1, prediction_type="epsilon"):
        key = (fd, prediction_type)
        if key not in made:
            made[key] = UNetTrainer(full_sd(fd), DEV, max_batch=B, max_frames=max(LENGTHS), learning_rate=1e-3, num_warmup_steps=4, dropout=P,
                                    feature_dim=fd, finetune_audio_layers=L, prediction_type=prediction_type)
        return made[key]

    yield get
    for t in made.values():
        t.close()


@pytest.fixture(scope="module")
def refs():
    """float64 and float32 autograd of the restatement for each case, computed once."""
    cache = {}

    def get(T, fd=-1, mode="eval", p=0.0, V=0, cond=None, prediction_type="epsilon", mask=True):
        key = (T, fd, mode, p, V, None if cond is None else tuple(cond), prediction_type, mask)
        if key not in cache:
            d = batch(T, V)
            enc = train_enc(T, mask)[0] if mode == "train" else None
            cache[key] = [aft.loss_and_grads(trainable(fd, dt), alphas(), d["coeffs"], d["noise"], d["timesteps"], d["feats"],
                                             d["cond"] if cond is None else cond, prediction_type=prediction_type, std=d.get("std"),
                                             deltas=d.get("deltas"), masks=ref.dropout_masks(SEED, B, T, p), enc=enc)
                          for dt in (torch.float64, torch.float32)]
        return cache[key]

    return get


def gpu_grads(tr, T, mode="eval", p=0.0, V=0, cond=None, mask=True):
    d = batch(T, V)
    tr.load_state_dict(full_sd(tr.feature_dim))
    tr.dropout = p
    tr.std = None if "std" not in d else d["std"].numpy()
    draws = train_enc(T, mask)[1] if mode == "train" else None
    out = tr.step(d["coeffs"], d["cond"] if cond is None else cond, d["feats"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED,
                  deltas=d.get("deltas"), audio_draws=draws, audio_cfg=AudioTrainConfig() if draws is not None else None)
    tr.std = None
    return out, tr.parameters_of(_engine.UT_GRAD)


# ---------------------------------------------------------------------------------------------------------------- 1. the table
@pytest.mark.parametrize("F", [-1, 64])
@pytest.mark.parametrize("layers", [1, 2, 12])
def test_table(F, layers):
    eng = _engine.UNetTrainEngine(torch.device(DEV), 1, 2, F, layers)
    try:
        want = trainable_shapes(F, layers)
        assert eng.tensors == [(n, int(np.prod(s))) for n, s in want.items()] and eng.finetune_layers == layers
        assert int(eng.lib.said_unet_train_finetune_layers(eng.h)) == layers
        enc = [n for n, _ in eng.tensors if n.startswith(ENC)]
        assert enc == [k for k in said_state_dict(num_w2v_layers=layers) if k.startswith(ENC) and "feature_extractor" not in k]
        assert not any("feature_extractor" in n for n, _ in eng.tensors)
    finally:
        eng.close()


def test_table_without_finetuning_is_the_existing_one():
    lib = _engine.load_library("unet_finetune")
    h = _engine.c_void_p()
    assert lib.said_unet_train_create_ft(_engine.ctypes.byref(h), 0, 1, 2, -1, 0) == 0
    try:
        n = lib.said_unet_train_num_tensors(h)
        assert n == _engine.UT_NUM_TENSORS and lib.said_unet_train_finetune_layers(h) == 0
        assert [lib.said_unet_train_context_tensor_name(h, i) for i in range(n)] == [lib.said_unet_train_tensor_name(i) for i in range(n)]
    finally:
        lib.said_unet_train_destroy(h)
    with pytest.raises(_engine.EngineError, match="finetune_layers 33 above 32"):
        _engine.UNetTrainEngine(torch.device(DEV), 1, 2, -1, 33)


def test_entry_points_refuse_the_other_kind_of_context(trainers):
    tr, d = trainers(), batch(19)
    lib = tr.eng.lib
    x, ts, cd = _engine._f32(d["coeffs"].numpy()), _engine._i64(d["timesteps"].numpy()), _engine._i32(np.array([1, 0], dtype=np.int32))
    au, out = _engine._f32(np.zeros((B, 19, 768), dtype=np.float32)), np.zeros((B, 19, 32), dtype=np.float32)
    assert lib.said_unet_train_forward_only(tr.eng.h, B, 19, _engine._fp(x), _engine._lp(ts), _engine._ip(cd), _engine._vp(au), 0, 0, _engine._fp(out)) != 0
    assert b"_ft entry point" in lib.said_unet_train_last_error(tr.eng.h)
    plain = _engine.UNetTrainEngine(torch.device(DEV), B, 19)
    try:
        assert lib.said_unet_train_forward_only_ft(plain.h, B, 19, _engine._fp(x), _engine._lp(ts), _engine._ip(cd), _engine._vp(au), 0, None, 0,
                                                   _engine._fp(out)) != 0
        assert b"no fine-tuned encoder" in lib.said_unet_train_last_error(plain.h)
    finally:
        plain.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the front end
@pytest.fixture(scope="module")
def model():
    from said_amd.model.diffusion import SAID_UNet1D
    m = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=L))
    m.load_state_dict(full_sd(), strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("frames", [19, 0])
def test_extract_features(model, frames):
    """said_audio_extract_features on 1 s of audio against audio_train_ref.features in float64, with and without the interpolation.  The
    convolutions run on fp32 matrix instructions (set_mfma_dtype("fp32_strict")), the reference's arithmetic; a bf16 context refuses."""
    wave = torch.stack([synth_waveform(i, 16000) for i in range(B)])
    enc = {k[len(ENC):]: v for k, v in full_sd().items() if k.startswith(ENC)}
    r64, r32 = (atr.features(enc, wave, frames or None, dt) for dt in (torch.float64, torch.float32))
    model.set_mfma_dtype("fp32_strict")
    try:
        got = model.get_audio_features(wave.to(DEV), frames or None).cpu()
    finally:
        model.set_mfma_dtype("fp32")
    assert tuple(got.shape) == tuple(r64.shape) == (B, frames or 49, 512)
    ok, msg = check("features", got, r32, r64, {})
    print("extract_features", msg)
    assert ok, msg
    model.set_mfma_dtype("bf16")
    try:
        with pytest.raises(_engine.EngineError, match="bf16 mode"):
            model.get_audio_features(wave.to(DEV), frames or None)
    finally:
        model.set_mfma_dtype("fp32")


# ---------------------------------------------------------------------------------------------------------------- 3. the forward
@pytest.mark.parametrize("T", LENGTHS)
def test_forward_eval(trainers, T):
    tr, d = trainers(), batch(T)
    tr.load_state_dict(full_sd())
    x = d["coeffs"] + 0.3 * d["noise"]
    got = tr.forward_only(x, d["timesteps"], d["cond"], d["feats"])
    cond_rows = torch.from_numpy(tr.eng.last_conditioning(B, T))
    with torch.no_grad():
        (r64, c64), (r32, c32) = ((aft.forward(trainable(-1, dt), x, d["timesteps"], d["feats"], d["cond"]), aft.conditioning(trainable(-1, dt), d["feats"]))
                                  for dt in (torch.float64, torch.float32))
    for name, g, a32, a64 in (("output", got, r32, r64), ("conditioning", cond_rows[0], c32[0], c64[0])):
        ok, msg = check(name, g, a32, a64, {})
        print("forward eval", T, msg)
        assert ok, msg
    assert torch.equal(cond_rows[1], full_sd()["null_cond_emb"][0].expand(T, -1))


@pytest.mark.parametrize("T", LENGTHS)
def test_forward_train(trainers, T):
    """The conditioning that the step's denoiser saw, in train mode: the published probabilities, a time mask, layer 1 skipped."""
    tr, d = trainers(), batch(T)
    enc, draws = train_enc(T)
    tr.load_state_dict(full_sd())
    tr.step(d["coeffs"], [True, True], d["feats"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED, audio_draws=draws, audio_cfg=AudioTrainConfig())
    got = torch.from_numpy(tr.eng.last_conditioning(B, T))
    with torch.no_grad():
        c64, c32 = (aft.conditioning(trainable(-1, dt), d["feats"], enc) for dt in (torch.float64, torch.float32))
    ok, msg = check("conditioning", got, c32, c64, {})
    print("forward train", T, msg)
    assert ok, msg
    with torch.no_grad():
        assert rel(aft.conditioning(trainable(-1, torch.float64), d["feats"]), c64) > 0.05, "the train-mode forward must differ from the eval one"


# ---------------------------------------------------------------------------------------------------------------- 4. the gradients
def grads_case(trainers, refs, what, T, fd=-1, prediction_type="epsilon", **kw):
    (l64, g64), (l32, g32) = refs(T, fd, prediction_type=prediction_type, **kw)
    out, g = gpu_grads(trainers(fd, prediction_type), T, **{k: v for k, v in kw.items()})
    assert loss_ok(out.predict, l32[0], l64[0]) and loss_ok(out.velocity, l32[1], l64[1]), (out, l32, l64)
    if kw.get("V"):
        assert loss_ok(out.vertex, l32[2], l64[2])
    assert list(g) == list(g64) == list(trainable_shapes(fd, L))
    bad = check_all(what, g, g32, g64)
    assert not bad, bad[:8]
    return g, g64


@pytest.mark.parametrize("T", LENGTHS)
def test_gradients_eval(trainers, refs, T):
    """(a), and (d) without a mask: masked_spec_embed's gradient is exactly zero."""
    g, g64 = grads_case(trainers, refs, f"gradients eval T={T}", T)
    assert float(g[ENC + "masked_spec_embed"].abs().max()) == 0 and float(g64[ENC + "masked_spec_embed"].abs().max()) == 0
    assert all(float(g[k].abs().max()) > 0 for k in g if k != ENC + "masked_spec_embed" and not k.endswith("k_proj.bias"))


@pytest.mark.parametrize("T", LENGTHS)
def test_gradients_train(trainers, refs, T):
    """(b), and (d) with a mask: every skipped layer's 16 gradients are exactly 0.0; masked_spec_embed's matches the reference."""
    g, g64 = grads_case(trainers, refs, f"gradients train T={T}", T, mode="train", p=P)
    skipped = [k for k in g if ".layers.1." in k]
    assert len(skipped) == 16 and all(float(g[k].abs().max()) == 0 for k in skipped)
    assert float(g64[ENC + "masked_spec_embed"].abs().max()) > 0 and float(g[ENC + "masked_spec_embed"].abs().max()) > 0


def test_gradients_train_without_a_mask(trainers, refs):
    g, _ = grads_case(trainers, refs, "gradients train, no mask", 19, mode="train", p=P, mask=False)
    assert float(g[ENC + "masked_spec_embed"].abs().max()) == 0


def test_gradients_unconditional_batch(trainers, refs):
    """(c) cond = [0, 0]: every audio_encoder.* gradient is exactly 0.0 and null_cond_emb's is not."""
    g, g64 = grads_case(trainers, refs, "gradients cond = [0, 0]", 19, cond=[False, False])
    enc = [k for k in g if k.startswith(ENC)]
    assert len(enc) == 42 and all(float(g[k].abs().max()) == 0 and float(g64[k].abs().max()) == 0 for k in enc)
    assert float(g["null_cond_emb"].abs().max()) > 0


def test_gradients_feature_dim(trainers, refs):
    """(e) feature_dim = 64: the gradient reaches the encoder through W_proj."""
    g, _ = grads_case(trainers, refs, "gradients F = 64", 19, fd=64, mode="train", p=P)
    assert float(g[PW].abs().max()) > 0 and float(g[ENC + "encoder.layers.0.attention.q_proj.weight"].abs().max()) > 0


def test_gradients_v_prediction_std_vertex(trainers, refs):
    """(f) prediction_type = "v_prediction" with std and the vertex loss on."""
    grads_case(trainers, refs, "gradients v_prediction, std, vertex", 19, prediction_type="v_prediction", V=7)


# ---------------------------------------------------------------------------------------------------------------- 5. - 7. clip, update, EMA
STD = np.full(32, 0.02, dtype=np.float32)   # scales the objective so that the joint norm is above 1
WATCH = ["denoiser.model.input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight", ENC + "encoder.pos_conv_embed.conv.weight_g",
         ENC + "encoder.pos_conv_embed.conv.weight_v", ENC + "encoder.layers.0.attention.q_proj.weight"]


def three_steps(tr, T=19):
    d = batch(T)
    tr.load_state_dict(full_sd(tr.feature_dim))
    tr.dropout, tr.std = P, STD
    norms = []
    for k in range(3):
        g = torch.Generator().manual_seed(k)
        tr.enqueue_step(d["coeffs"], d["cond"], d["feats"], noise=torch.randn(B, T, 32, generator=g), timesteps=d["timesteps"], dropout_seed=SEED + k,
                        audio_draws=train_enc(T, seed=ASEED + k)[1], audio_cfg=AudioTrainConfig())
        norms.append(float(tr.eng.last_losses()[5]))
    tr.std = None
    return norms


@pytest.fixture(scope="module")
def ref_three_steps():
    """The float64 and float32 restatements of torch's AdamW + EMAModel after the three steps of three_steps()."""
    T, d = 19, batch(19)
    lam, dec = constant_with_warmup_lambda(4), (lambda n: ema_decay(n, 0.9999))
    runs = []
    for dt in (torch.float64, torch.float32):
        rt = aft.RefTrainer(trainable(-1, dt), 1e-3, lam, dec)
        rt.norms = []
        for k in range(3):
            g = torch.Generator().manual_seed(k)
            rt.step(alphas(), d["coeffs"], torch.randn(B, T, 32, generator=g), d["timesteps"], d["feats"], d["cond"], std=torch.from_numpy(STD),
                    masks=ref.dropout_masks(SEED + k, B, T, P), enc=train_enc(T, seed=ASEED + k)[0])
            rt.norms.append(float(torch.sqrt(sum((x.double().norm() ** 2 for x in rt.last_grads.values())))))
        runs.append(rt)
    return runs


def test_joint_clip_and_update(trainers, ref_three_steps):
    r64, r32 = ref_three_steps
    assert max(r64.clip_factors) < 1.0, "the joint norm must be above 1 on every step"
    tr = trainers()
    norms = three_steps(tr)
    den = float(torch.sqrt(sum((v.double().norm() ** 2 for k, v in r64.last_grads.items() if not k.startswith(ENC)))))
    assert den < 0.999 * r64.norms[-1], "the encoder must carry part of the joint norm"
    for k in range(3):
        print("joint gradient norm", k, norms[k], r64.norms[k], r32.norms[k])
        assert abs(norms[k] - r64.norms[k]) <= 4 * max(abs(r32.norms[k] - r64.norms[k]), 1e-6 * r64.norms[k]), (k, norms[k], r64.norms[k], r32.norms[k])
    bad = []
    for name, which, a64, a32 in (("parameters", _engine.UT_STATE, r64.p, r32.p), ("exp_avg", _engine.UT_EXP_AVG, r64.m, r32.m),
                                  ("exp_avg_sq", _engine.UT_EXP_AVG_SQ, r64.v, r32.v), ("ema", _engine.UT_EMA, r64.ema, r32.ema)):
        got = tr.parameters_of(which)
        for n in WATCH:
            ok, msg = check(n, got[n], a32[n], a64[n], {})
            print("three steps", name, msg)
            if not ok:
                bad.append((name,) + msg)
    assert not bad, bad
    live = tr.parameters_of(_engine.UT_STATE)
    assert all(not torch.equal(live[n], full_sd()[n]) for n in WATCH)


def test_determinism(trainers):
    """Two contexts, the same inputs and seeds: every gradient is bit-identical after one step, every parameter after three."""
    other = UNetTrainer(full_sd(), DEV, max_batch=B, max_frames=max(LENGTHS), learning_rate=1e-3, num_warmup_steps=4, dropout=P, finetune_audio_layers=L)
    try:
        res = []
        for tr in (trainers(), other):
            _, g = gpu_grads(tr, 150, mode="train", p=P)
            three_steps(tr)
            res.append((g, tr.parameters_of(_engine.UT_STATE)))
    finally:
        other.close()
    (g1, p1), (g2, p2) = res
    assert len(g1) == len(trainable_shapes(-1, L))
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
        assert torch.equal(p1[k], p2[k]), k


def test_eval_loss_on_ema(trainers):
    T = 19
    tr, d = trainers(), batch(T)
    three_steps(tr)
    ema, live = tr.parameters_of(_engine.UT_EMA), tr.parameters_of(_engine.UT_STATE)
    q = ENC + "encoder.layers.0.attention.q_proj.weight"
    assert not torch.equal(ema[q], live[q]) and not torch.equal(ema[q], full_sd()[q])
    tr.epoch_output(False)
    tr.eval_loss(d["coeffs"], d["cond"], d["feats"], noise=d["noise"], timesteps=d["timesteps"], use_ema=True)
    got = tr.epoch_output(True)
    vals = []
    for dt in (torch.float64, torch.float32):
        sd = {k: v.to(dt) for k, v in ema.items()}
        with torch.no_grad():
            noisy, answer = ref.add_noise(alphas(), d["coeffs"], d["noise"], d["timesteps"], "epsilon", dt)
            vals.append([float(x) for x in ref.objective(aft.forward(sd, noisy, d["timesteps"], d["feats"], d["cond"]), answer)[:2]])
    for g, v64, v32 in zip((got.predict, got.velocity), *vals):
        assert abs(g - v64) <= 4 * max(abs(v32 - v64), 1e-6 * abs(v64)), (g, v64, v32)
    # and it is not the loss on the live weights
    tr.eval_loss(d["coeffs"], d["cond"], d["feats"], noise=d["noise"], timesteps=d["timesteps"], use_ema=False)
    assert tr.epoch_output(True).predict != got.predict


# ---------------------------------------------------------------------------------------------------------------- 8. the checkpoint
def test_checkpoint_round_trip(trainers):
    """state_dict() after three steps loads strictly into SAID_UNet1D with the feature extractor bit for bit as given, and the inference
    engine's get_audio_embedding on it agrees with the trainer's eval-mode conditioning, within 4 x the error measured here of the inference
    engine's said_audio_encode (split-fp16 products: older code, not the code under test) against the float64 restatement on the same weights."""
    from said_amd.model.diffusion import SAID_UNet1D
    T = 19
    tr = trainers()
    three_steps(tr)
    sd = tr.state_dict()
    m = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=L))
    assert list(sd) == list(m.state_dict())
    m.load_state_dict(sd, strict=True)
    given = full_sd()
    for k, v in given.items():
        if "feature_extractor" in k:
            assert torch.equal(sd[k], v), k
        elif k.startswith(ENC) and k != ENC + "masked_spec_embed":
            assert not torch.equal(sd[k], v), k
    m.to(DEV)
    wave = torch.stack([synth_waveform(i, 16000 * T // 60) for i in range(B)])
    emb = m.get_audio_embedding(wave.to(DEV), T).cpu()
    feats = m.get_audio_features(wave.to(DEV), T)
    d = batch(T)
    tr.forward_only(d["coeffs"], d["timesteps"], [True, True], feats)
    mine = torch.from_numpy(tr.eng.last_conditioning(B, T))
    enc = {k[len(ENC):]: v for k, v in sd.items() if k.startswith(ENC)}
    r64 = atr.forward(enc, wave, T, dtype=torch.float64)
    older = rel(emb, r64)
    print("checkpoint: inference engine vs float64", older, "trainer vs float64", rel(mine, r64), "trainer vs inference engine", rel(mine, emb))
    assert rel(mine, emb) <= 4 * older


# ---------------------------------------------------------------------------------------------------------------- 9. the command line
@pytest.fixture(scope="module")
def cli_data(tmp_path_factory):
    """The synthetic 2-speaker, 2-sentence set of test_train_cli_two_epochs."""
    from scipy.io import wavfile
    from said_amd.training.vae import PERSON_IDS_TRAIN
    from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, save_blendshape_coeffs
    tmp = tmp_path_factory.mktemp("audio_finetune_cli")
    rng = np.random.default_rng(0)
    for pid in PERSON_IDS_TRAIN[:2]:
        os.makedirs(tmp / "audio" / pid)
        os.makedirs(tmp / "coeffs" / pid)
        for sid, frames in ((1, 50), (2, 63)):
            n = 16000 * frames // 60
            wave = (0.3 * np.sin(2 * np.pi * (180 + 40 * sid) * np.arange(n) / 16000) * 32767).astype(np.int16)
            wavfile.write(str(tmp / "audio" / pid / f"sentence{sid:02}.wav"), 16000, wave)
            walk = np.clip(0.3 + np.cumsum(rng.normal(0, 0.02, (frames, 32)), 0), 0, 1)
            save_blendshape_coeffs(walk, DEFAULT_BLENDSHAPE_CLASSES, str(tmp / "coeffs" / pid / f"sentence{sid:02}.csv"))
    return tmp


def _train_cli(tmp, out, *extra):
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "script", "train.py"), "--audio_dir", str(tmp / "audio"), "--coeffs_dir", str(tmp / "coeffs"),
                        "--output_dir", str(tmp / out), "--window_size_min", "40", "--epochs", "2", "--batch_size", "2", "--save_period", "2",
                        "--val_period", "1", "--num_warmup_epochs", "1", "--audio_encoder_weights", "synthetic", "--seed", "0", "--device", DEV, *extra],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return open(tmp / out / "log.csv").read().splitlines()


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_train_cli_finetunes_the_encoder(cli_data, mode):
    import csv
    log = _train_cli(cli_data, "out_ft_" + mode, "--finetune_audio_encoder", "--audio_encoder_mode", mode)
    rows = list(csv.DictReader(log))
    assert len(rows) == 2
    for r in rows:
        assert r["Train/Total Loss"] != ""
        for k, v in r.items():
            if "Loss" in k and v != "":
                assert np.isfinite(float(v)), (k, v)
    sd = torch.load(str(cli_data / ("out_ft_" + mode) / "2.pth"), map_location="cpu")
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


def test_train_cli_without_the_flag_is_unchanged(cli_data):
    assert _train_cli(cli_data, "out_plain") == open(os.path.join(ROOT, "tests", "golden", "train_log_seed0_eval.csv")).read().splitlines()
