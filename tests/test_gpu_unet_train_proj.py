"""Denoiser training with feature_dim > 0 on the MI355X: the trainable audio_proj_layer = nn.Linear(768, F) behind the frozen encoder, the F-wide
context and null_cond_emb (said_unet_train_create_dim; UNetTrainer(feature_dim=F)) against the float64 restatement of the reference step with
the projection applied in front (tests/unet_train_proj_ref.py) and against golden G17, captured from the reference's own module.

Tolerance rule: tests/test_gpu_unet_train.py's.  Per tensor, the 2-norm of the difference from the float64 run over the 2-norm of the float64
tensor must be within 4 x max(the same error of the restatement's fp32 CPU run, 1e-6); it applies to all 163 tensors.  Shapes (B, T, F):
(2, 40, 40) — F leaves a tail of 8 in the GEMM's 16-wide k tile and does not fill a 64-wide N tile — and (3, 121, 256) — M = 363 is no multiple of
64, the projection's weight gradient runs K-split over K = 363, and the cond flags are mixed.
"""
import os

import numpy as np
import pytest
import torch

from said_amd import _engine
from said_amd.training import UNetTrainer, normalize_deltas, trainable_shapes
from said_amd.util.scheduler import constant_with_warmup_lambda, ema_decay
from said_amd.util.synth import fill_tensor, said_state_dict
import unet_train_proj_ref as pref
import unet_train_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 40, 40), (3, 121, 256)]
SEED = 0x1234567887654321
P = 0.1
PW, PB = "audio_proj_layer.weight", "audio_proj_layer.bias"
_SD, _AC = {}, []


def full_sd(fd):
    """SAID_UNet1D(feature_dim=fd)'s state dict with a one-layer encoder, synth's fill (non-zero in the zero-initialised convolutions)."""
    if fd not in _SD:
        sd = said_state_dict(num_w2v_layers=1, ctx_dim=fd if fd > 0 else 768)
        if fd > 0:
            sd[PW], sd[PB] = fill_tensor(PW, (fd, 768)), fill_tensor(PB, (fd,))
        _SD[fd] = sd
    return dict(_SD[fd])


def trainable(fd, dtype):
    sd = full_sd(fd)
    return {k: sd[k].to(dtype) for k in trainable_shapes(fd)}


def batch(B, T, V=0):
    g = torch.Generator().manual_seed(100 * B + T)
    d = dict(coeffs=torch.rand(B, T, 32, generator=g), noise=torch.randn(B, T, 32, generator=g),
             timesteps=torch.tensor([10, 500, 900][:B]), cond=[True, False, True][:B], audio=torch.randn(B, T, 768, generator=g))
    if V:
        d["std"] = 0.5 + torch.rand(32, generator=g)
        d["deltas"] = normalize_deltas(torch.randn(B, 32, V, 3, generator=g))
    return d


def alphas():
    if not _AC:
        from said_amd.scheduler import DDIMScheduler
        _AC.append(DDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2").alphas_cumprod.float())
    return _AC[0]


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def check(name, got, r32, r64, worst):
    e32 = rel(r32, r64)
    e = rel(got, r64)
    bound = 4 * max(e32, 1e-6)
    worst[name] = (e, e32)
    return e <= bound, (name, e, e32, bound)


def check_all(what, got, a32, a64):
    """Every tensor of a64 under the bound; prints the worst one."""
    worst, bad = {}, []
    for k in a64:
        ok, msg = check(k, got[k], a32[k], a64[k], worst)
        if not ok:
            bad.append(msg)
    k = max(worst, key=lambda n: worst[n][0])
    print(f"{what}: {len(worst)} tensors, worst {k} hip {worst[k][0]:.3e} cpu-fp32 {worst[k][1]:.3e}; failing {len(bad)}")
    return bad


@pytest.fixture(scope="module")
def trainers():
    """One trainer per feature_dim, made on first use."""
    made = {}

    def get(fd):
        if fd not in made:
            made[fd] = UNetTrainer(full_sd(fd), "cuda:0", max_batch=3, max_frames=128, learning_rate=1e-3, num_warmup_steps=4, dropout=P, feature_dim=fd)
        return made[fd]

    yield get
    for t in made.values():
        t.close()


@pytest.fixture(scope="module")
def refs():
    """float64 and float32 autograd of the projecting restatement for each case, computed once."""
    cache = {}

    def get(B, T, fd, p=0.0, V=0, cond=None):
        key = (B, T, fd, p, V, None if cond is None else tuple(cond))
        if key not in cache:
            d = batch(B, T, V)
            cache[key] = [pref.loss_and_grads(trainable(fd, dt), alphas(), d["coeffs"], d["noise"], d["timesteps"], d["audio"],
                                              d["cond"] if cond is None else cond, std=d.get("std"), deltas=d.get("deltas"),
                                              masks=ref.dropout_masks(SEED, B, T, p)) for dt in (torch.float64, torch.float32)]
        return cache[key]

    return get


def gpu_grads(tr, B, T, p, V=0, cond=None):
    d = batch(B, T, V)
    tr.load_state_dict(full_sd(tr.feature_dim))
    tr.dropout = p
    tr.std = None if "std" not in d else d["std"].numpy()
    out = tr.step(d["coeffs"], d["cond"] if cond is None else cond, d["audio"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED,
                  deltas=d.get("deltas"))
    tr.std = None
    return out, tr.parameters_of(_engine.UT_GRAD)


def loss_ok(got, l32, l64):
    return abs(float(got) - float(l64)) <= 4 * max(abs(float(l32) - float(l64)), 1e-6 * float(l64))


def test_context_has_the_projection(trainers):
    tr = trainers(40)
    assert tr.feature_dim == 40 and tr.eng.feature_dim == 40
    assert [(n, k) for n, k in tr.eng.tensors] == [(n, int(np.prod(s))) for n, s in trainable_shapes(40).items()] and len(tr.eng.tensors) == 163
    with pytest.raises(_engine.EngineError, match="feature_dim 1025 above 1024"):
        _engine.UNetTrainEngine(torch.device("cuda:0"), 1, 2, 1025)
    sd = full_sd(40)
    sd[PW] = sd[PW][:, :700]
    with pytest.raises(ValueError, match=r"audio_proj_layer.weight: shape \(40, 700\), expected \(40, 768\)"):
        tr.load_state_dict(sd)
    with pytest.raises(ValueError, match=r"null_cond_emb: shape \(1, 1, 768\), expected \(1, 1, 40\)"):
        tr.load_state_dict({**full_sd(40), "null_cond_emb": torch.zeros(1, 1, 768)})
    tr.load_state_dict(full_sd(40))


@pytest.mark.parametrize("B,T,fd", SHAPES)
def test_forward(trainers, B, T, fd):
    tr, d = trainers(fd), batch(B, T)
    tr.load_state_dict(full_sd(fd))
    x = d["coeffs"] + 0.3 * d["noise"]
    got = tr.forward_only(x, d["timesteps"], d["cond"], d["audio"])
    with torch.no_grad():
        r64 = pref.forward(trainable(fd, torch.float64), x, d["timesteps"], d["audio"], d["cond"])
        r32 = pref.forward(trainable(fd, torch.float32), x, d["timesteps"], d["audio"], d["cond"])
    ok, msg = check("output", got, r32, r64, {})
    print("forward", msg)
    assert ok, msg


@pytest.mark.parametrize("p", [0.0, P])
@pytest.mark.parametrize("B,T,fd", SHAPES)
def test_gradients(trainers, refs, B, T, fd, p):
    (l64, g64), (l32, g32) = refs(B, T, fd, p)
    out, g = gpu_grads(trainers(fd), B, T, p)
    assert loss_ok(out.predict, l32[0], l64[0]) and loss_ok(out.velocity, l32[1], l64[1])
    assert len(g64) == 163 and set(g) == set(g64)
    assert g[PW].abs().max() > 0 and g[PB].abs().max() > 0 and g["null_cond_emb"].abs().max() > 0
    bad = check_all(f"gradients B={B} T={T} F={fd} p={p}", g, g32, g64)
    assert not bad, bad[:8]


def test_vertex_loss_with_std(trainers, refs):
    (l64, g64), (l32, g32) = refs(2, 40, 40, 0.0, V=7)
    out, g = gpu_grads(trainers(40), 2, 40, 0.0, V=7)
    assert loss_ok(out.vertex, l32[2], l64[2])
    bad = check_all("vertex loss with std", g, g32, g64)
    assert not bad, bad[:8]


def test_select_routes_the_context_gradient(trainers, refs):
    """Every sample unconditional: the projection sees no gradient (exact zeros, as torch's zero tensor) and is still decayed; every sample
    conditional: null_cond_emb sees none."""
    tr = trainers(40)
    (_, g64), (_, g32) = refs(2, 40, 40, 0.0, cond=[False, False])
    _, g = gpu_grads(tr, 2, 40, 0.0, cond=[False, False])
    assert g[PW].abs().max() == 0 and g[PB].abs().max() == 0 and g["null_cond_emb"].abs().max() > 0
    assert g64[PW].abs().max() == 0 and g64[PB].abs().max() == 0
    ok, msg = check("null_cond_emb", g["null_cond_emb"], g32["null_cond_emb"], g64["null_cond_emb"], {})
    assert ok, msg
    # the first step's learning rate is 0 under the warm-up; the second one decays: p <- p (1 - lr wd) with exp_avg = exp_avg_sq = 0
    d = batch(2, 40)
    tr.step(d["coeffs"], [False, False], d["audio"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED)
    w0, w1 = full_sd(40)[PW], tr.parameters_of(_engine.UT_STATE)[PW]
    assert tr.parameters_of(_engine.UT_GRAD)[PW].abs().max() == 0
    assert not torch.equal(w1, w0) and torch.allclose(w1, w0 * (1 - tr.lr_at(1) * tr.weight_decay), rtol=1e-6, atol=0)
    assert tr.parameters_of(_engine.UT_EXP_AVG)[PW].abs().max() == 0

    (_, g64), (_, g32) = refs(2, 40, 40, 0.0, cond=[True, True])
    _, g = gpu_grads(tr, 2, 40, 0.0, cond=[True, True])
    assert g["null_cond_emb"].abs().max() == 0 and g[PW].abs().max() > 0 and g[PB].abs().max() > 0
    for k in (PW, PB):
        ok, msg = check(k, g[k], g32[k], g64[k], {})
        assert ok, msg


def test_three_steps(trainers):
    B, T, fd = 2, 40, 40
    tr, d = trainers(fd), batch(B, T)
    lam, dec = constant_with_warmup_lambda(4), (lambda n: ema_decay(n, 0.9999))
    runs = []
    for dt in (torch.float64, torch.float32):
        rt = pref.RefTrainer(trainable(fd, dt), 1e-3, lam, dec)
        assert PW in rt.p and PB in rt.p
        for k in range(3):
            g = torch.Generator().manual_seed(k)
            rt.step(alphas(), d["coeffs"], torch.randn(B, T, 32, generator=g), d["timesteps"], d["audio"], d["cond"],
                    masks=ref.dropout_masks(SEED + k, B, T, P))
        runs.append(rt)
    r64, r32 = runs
    assert min(r64.clip_factors) < 1.0, "the clip must be active on at least one step"
    tr.load_state_dict(full_sd(fd))
    tr.dropout = P
    for k in range(3):
        g = torch.Generator().manual_seed(k)
        tr.enqueue_step(d["coeffs"], d["cond"], d["audio"], noise=torch.randn(B, T, 32, generator=g), timesteps=d["timesteps"], dropout_seed=SEED + k)
    bad = []
    for name, which, a64, a32 in (("parameters", _engine.UT_STATE, r64.p, r32.p), ("exp_avg", _engine.UT_EXP_AVG, r64.m, r32.m),
                                  ("exp_avg_sq", _engine.UT_EXP_AVG_SQ, r64.v, r32.v), ("ema", _engine.UT_EMA, r64.ema, r32.ema)):
        assert len(a64) == 163
        bad += [(name,) + m for m in check_all("three steps, " + name, tr.parameters_of(which), a32, a64)]
    assert not bad, bad[:8]
    assert not torch.equal(tr.parameters_of(_engine.UT_STATE)[PW], full_sd(fd)[PW])


def test_step_is_bit_identical(trainers):
    tr = trainers(256)
    _, g1 = gpu_grads(tr, 3, 121, P)
    p1 = tr.parameters_of(_engine.UT_STATE)
    _, g2 = gpu_grads(tr, 3, 121, P)
    p2 = tr.parameters_of(_engine.UT_STATE)
    assert len(g1) == 163
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
        assert torch.equal(p1[k], p2[k]), k


def test_eval_loss_on_ema(trainers):
    B, T, fd = 2, 40, 40
    tr, d = trainers(fd), batch(B, T)
    tr.load_state_dict(full_sd(fd))
    tr.dropout = P
    for k in range(2):
        tr.enqueue_step(d["coeffs"], d["cond"], d["audio"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED + k)
    ema, live = tr.parameters_of(_engine.UT_EMA), tr.parameters_of(_engine.UT_STATE)
    assert not torch.equal(ema[PW], live[PW])
    tr.epoch_output(False)
    tr.eval_loss(d["coeffs"], d["cond"], d["audio"], noise=d["noise"], timesteps=d["timesteps"], use_ema=True)
    got = tr.epoch_output(True)
    vals = []
    for dt in (torch.float64, torch.float32):
        sd = {k: v.to(dt) for k, v in ema.items()}
        with torch.no_grad():
            noisy, answer = ref.add_noise(alphas(), d["coeffs"], d["noise"], d["timesteps"], "epsilon", dt)
            vals.append([float(x) for x in ref.objective(pref.forward(sd, noisy, d["timesteps"], d["audio"], d["cond"]), answer)[:2]])
    for g, v64, v32 in zip((got.predict, got.velocity), *vals):
        assert abs(g - v64) <= 4 * max(abs(v32 - v64), 1e-6 * abs(v64)), (g, v64, v32)
    # and forward_only with use_ema is the EMA projection's too
    x = d["coeffs"] + 0.3 * d["noise"]
    out = tr.forward_only(x, d["timesteps"], d["cond"], d["audio"], use_ema=True)
    with torch.no_grad():
        r64, r32 = (pref.forward({k: v.to(dt) for k, v in ema.items()}, x, d["timesteps"], d["audio"], d["cond"]) for dt in (torch.float64, torch.float32))
    ok, msg = check("output on the EMA copy", out, r32, r64, {})
    assert ok, msg


def test_golden_g17():
    """Part A of golden G17: the output and all 163 gradients against the reference's own UNet1DConditionModel(32, 32, 40) behind
    nn.Linear(768, 40), to 1e-4 of each gradient's norm (G16's rule).  The golden gives the model input and the answer directly: with
    alphas_cumprod = 0 the step's add_noise gives noisy = noise and, for prediction type `sample`, answer = coeffs, both exactly."""
    G = np.load(os.path.join(ROOT, "tests", "golden", "g17_unet_train_proj.npz"))
    x, answer, audio, ts, cond = (torch.from_numpy(G[k]) for k in ("x", "answer", "audio", "timesteps", "cond"))
    tr = UNetTrainer(full_sd(40), "cuda:0", max_batch=2, max_frames=40, dropout=0.0, prediction_type="sample", feature_dim=40)
    tr.eng.set_alphas(np.zeros(1000, dtype=np.float32))
    out = tr.forward_only(x, ts, cond, audio)
    res = tr.step(answer, cond, audio, noise=x, timesteps=ts, dropout_seed=0, weight_vel=1.0)
    g = tr.parameters_of(_engine.UT_GRAD)
    tr.close()
    want = torch.from_numpy(G["out"])
    assert float((out - want).abs().max()) <= 2e-5 * float(want.abs().max())
    assert abs(float(res.predict) + float(res.velocity) - float(G["loss"])) <= 1e-5 * float(G["loss"])
    names = [str(n) for n in G["names"]]
    assert names == list(g) and len(names) == 163
    worst = 0.0
    for n, gs, gn in zip(names, G["grad_sum"], G["grad_norm"]):
        q = g[n].double()
        assert gn > 0, n
        worst = max(worst, abs(float(q.norm()) - gn) / gn)
        assert abs(float(q.norm()) - gn) <= 1e-4 * gn, (n, float(q.norm()), gn)
        assert abs(float(q.sum()) - gs) <= 1e-4 * gn * q.numel() ** 0.5, (n, float(q.sum()), gs)
        if "g:" + n in G.files:
            assert (q.reshape(-1) - torch.from_numpy(G["g:" + n]).double()).norm() <= 1e-4 * gn, n
    print("G17 worst relative norm deviation", worst)


def test_default_context_is_untouched():
    """feature_dim = -1 through said_unet_train_create_dim and the context of said_unet_train_create (feature_dim=None in the binding): the
    static 161-name table, and equal bits for the same step."""
    lib = _engine.load_library("unet_train")
    static = [(lib.said_unet_train_tensor_name(i).decode(), lib.said_unet_train_tensor_numel(i)) for i in range(_engine.UT_NUM_TENSORS)]
    d = batch(2, 40)
    res = []
    for fd in (-1, None):
        tr = UNetTrainer(full_sd(-1), "cuda:0", max_batch=2, max_frames=40, learning_rate=1e-3, dropout=P, feature_dim=fd)
        assert tr.eng.tensors == static and tr.feature_dim == -1
        tr.step(d["coeffs"], d["cond"], d["audio"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED)
        res.append((tr.parameters_of(_engine.UT_GRAD), tr.parameters_of(_engine.UT_STATE)))
        tr.close()
    (g1, p1), (g2, p2) = res
    assert list(g1) == list(trainable_shapes()) and len(g1) == 161
    for k in g1:
        assert torch.equal(g1[k], g2[k]) and torch.equal(p1[k], p2[k]), k
    assert not torch.equal(p1["null_cond_emb"], full_sd(-1)["null_cond_emb"])


@pytest.mark.parametrize("B,T,fd", SHAPES)
def test_checkpoint_round_trip(trainers, B, T, fd):
    """state_dict() after training loads strict into SAID_UNet1D(feature_dim=F) in that model's key order, and the checkpoint computes what
    the trainer computes: the model's forward on F.linear(audio, W_p, b_p) against forward_only, within 2e-4 of the output's scale (the
    figure of test_checkpoint_loads_into_the_inference_model, for the inference engine's split-fp16 products).

    The inference engine takes context widths that are multiples of 16 only (said_create refuses the others), so SAID_UNet1D(feature_dim=40)
    loads the checkpoint but cannot run it.  At F = 40 the loaded model's own state dict is therefore evaluated by the CPU oracle
    (oracle/unet.py) under the same bound; at F = 256 the model runs on the GPU, and there its get_audio_embedding(before_proj=True) is
    compared with a model without a projection."""
    from oracle import unet as oracle_unet
    from said_amd.model.diffusion import SAID_UNet1D
    from said_amd.model.wav2vec2 import AudioConfig, AudioTrainConfig, draw_audio_train
    from said_amd.util.synth import synth_waveform
    tr, d = trainers(fd), batch(B, T)
    tr.load_state_dict(full_sd(fd))
    tr.dropout = P
    tr.enqueue_step(d["coeffs"], d["cond"], d["audio"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED)
    tr.enqueue_step(d["coeffs"], d["cond"], d["audio"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED + 1)   # lr > 0
    sd = tr.state_dict()
    assert not torch.equal(sd[PW], full_sd(fd)[PW])
    model = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=1), feature_dim=fd)
    assert list(sd) == list(model.state_dict())
    model.load_state_dict(sd, strict=True)
    for k, v in full_sd(fd).items():
        if k.startswith("audio_encoder."):
            assert torch.equal(sd[k], v), k
    x = d["coeffs"] + 0.3 * d["noise"]
    want = tr.forward_only(x, d["timesteps"], [True] * B, d["audio"])
    loaded = model.state_dict()
    with torch.no_grad():
        emb = torch.nn.functional.linear(d["audio"], loaded[PW], loaded[PB])
        if fd % 16:
            got = oracle_unet.unet1d_forward({k[len("denoiser."):]: v for k, v in loaded.items() if k.startswith("denoiser.")}, x, d["timesteps"], emb)
        else:
            model.to("cuda:0")
            got = model(x.to("cuda:0"), d["timesteps"].to("cuda:0"), emb.to("cuda:0")).cpu()
    assert float((got - want).abs().max()) <= 2e-4 * float(want.abs().max()), float((got - want).abs().max())
    if fd % 16:
        return

    # the features before the projection are those of a model without one that holds the same encoder
    plain = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=1))
    plain.load_state_dict(full_sd(-1), strict=True)
    plain.to("cuda:0")
    frames = 40
    wave = model.process_audio([synth_waveform(i, 16000 * frames // 60).numpy() for i in range(2)]).to("cuda:0")
    a = model.get_audio_embedding(wave, frames, before_proj=True)
    assert tuple(a.shape) == (2, frames, 768) and torch.equal(a, plain.get_audio_embedding(wave, frames))
    assert tuple(model.get_audio_embedding(wave, frames).shape) == (2, frames, fd)
    torch.manual_seed(3)
    cfg = AudioTrainConfig()
    draws = draw_audio_train(cfg, 2, frames, 1)
    a = model.get_audio_embedding(wave, frames, train_draws=draws, train_cfg=cfg, before_proj=True)
    assert tuple(a.shape) == (2, frames, 768) and torch.equal(a, plain.get_audio_embedding(wave, frames, train_draws=draws, train_cfg=cfg))
    assert not torch.equal(a, plain.get_audio_embedding(wave, frames))


def test_train_cli_with_feature_dim(tmp_path):
    """script/train.py --unet_feature_dim 64 as a fresh child process: 2 epochs on the synthetic 2-speaker, 2-sentence set of
    test_train_cli_two_epochs; 2.pth loads into SAID_UNet1D(feature_dim=64) and its projection has moved."""
    import csv
    import subprocess
    import sys
    from scipy.io import wavfile
    from said_amd.model.diffusion import SAID_UNet1D
    from said_amd.training import unet_init_state_dict
    from said_amd.training.vae import PERSON_IDS_TRAIN
    from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, save_blendshape_coeffs
    rng = np.random.default_rng(0)
    for pid in PERSON_IDS_TRAIN[:2]:
        os.makedirs(tmp_path / "audio" / pid)
        os.makedirs(tmp_path / "coeffs" / pid)
        for sid, frames in ((1, 50), (2, 63)):
            n = 16000 * frames // 60
            wave = (0.3 * np.sin(2 * np.pi * (180 + 40 * sid) * np.arange(n) / 16000) * 32767).astype(np.int16)
            wavfile.write(str(tmp_path / "audio" / pid / f"sentence{sid:02}.wav"), 16000, wave)
            walk = np.clip(0.3 + np.cumsum(rng.normal(0, 0.02, (frames, 32)), 0), 0, 1)
            save_blendshape_coeffs(walk, DEFAULT_BLENDSHAPE_CLASSES, str(tmp_path / "coeffs" / pid / f"sentence{sid:02}.csv"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "script", "train.py"), "--audio_dir", str(tmp_path / "audio"), "--coeffs_dir",
                          str(tmp_path / "coeffs"), "--output_dir", str(tmp_path / "out"), "--window_size_min", "40", "--epochs", "2", "--batch_size", "2",
                          "--save_period", "2", "--val_period", "1", "--num_warmup_epochs", "1", "--audio_encoder_weights", "synthetic", "--seed", "0",
                          "--unet_feature_dim", "64", "--device", "cuda:0"], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    sd = torch.load(str(tmp_path / "out" / "2.pth"), map_location="cpu")
    model = SAID_UNet1D(feature_dim=64)
    assert list(sd) == list(model.state_dict())
    model.load_state_dict(sd, strict=True)
    assert all(torch.isfinite(v).all() for v in sd.values())
    # the script seeds torch and then draws the initial state before anything else draws from torch's generator
    torch.manual_seed(0)
    init = unet_init_state_dict(64)
    assert tuple(sd[PW].shape) == (64, 768) and not torch.equal(sd[PW], init[PW]) and not torch.equal(sd[PB], init[PB])
    assert float((sd[PW] - init[PW]).abs().max()) < 1e-3   # four steps at a learning rate of at most 1e-5 away from it
    rows = list(csv.DictReader(open(tmp_path / "out" / "log.csv")))
    assert len(rows) == 2
    for r in rows:   # the set has no validation speakers: those columns stay empty
        assert r["Train/Total Loss"] != "" and r["Train/Predict Loss"] != "" and r["Train/Velocity Loss"] != ""
        for k, v in r.items():
            if "Loss" in k and v != "":
                assert np.isfinite(float(v)), (k, v)
