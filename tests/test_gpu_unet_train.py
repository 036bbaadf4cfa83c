"""Denoiser training on the MI355X (include/said_unet_train.h, said_amd/csrc/unet_train.hip; said_amd.training.UNetTrainer) against the
float64 restatement of the reference step (tests/unet_train_ref.py).

Tolerance rule: for each tensor the error of the restatement's own fp32 CPU run against its float64 run is measured, as the 2-norm of the
difference over the 2-norm of the float64 tensor; the HIP result must be within 4 x that (the factor covers the different summation order),
with a floor only where the CPU fp32 error is below 1e-6: there 1e-6 stands in for it, so the bound is 4 x max(cpu error, 1e-6).  Shapes: B = 2, T = 40 (one partial 32-tile) and B = 3, T = 121 (odd T, more
than three key tiles).  The zero-initialised convolutions hold non-zero values (said_amd.util.synth's fill).
"""
import numpy as np
import pytest
import torch

from said_amd import _engine
from said_amd.training import UNetTrainer, normalize_deltas
from said_amd.training.unet import trainable_shapes
from said_amd.util.scheduler import constant_with_warmup_lambda, ema_decay
from said_amd.util.synth import said_state_dict
from train_opt_check import check_clip_adamw_ema_update
import unet_train_ref as ref

pytestmark = pytest.mark.gpu
SHAPES = [(2, 40), (3, 121)]
SEED = 0x1234567887654321
P = 0.1


def full_sd():
    return said_state_dict(num_w2v_layers=1)


def trainable(dtype):
    sd = full_sd()
    return {k: sd[k].to(dtype) for k in trainable_shapes()}


def batch(B, T, V=0):
    g = torch.Generator().manual_seed(100 * B + T)
    d = dict(coeffs=torch.rand(B, T, 32, generator=g), noise=torch.randn(B, T, 32, generator=g),
             timesteps=torch.tensor([10, 500, 900][:B]), cond=[True, False, True][:B], audio=torch.randn(B, T, 768, generator=g))
    if V:
        d["std"] = 0.5 + torch.rand(32, generator=g)
        d["deltas"] = normalize_deltas(torch.randn(B, 32, V, 3, generator=g))
    return d


def make_trainer(**kw):
    kw.setdefault("max_batch", 3)
    kw.setdefault("max_frames", 128)
    return UNetTrainer(full_sd(), "cuda:0", **kw)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def check(name, got, r32, r64, worst):
    e32 = rel(r32, r64)
    e = rel(got, r64)
    bound = 4 * max(e32, 1e-6)
    worst[name] = (e, e32)
    return e <= bound, (name, e, e32, bound)


@pytest.fixture(scope="module")
def tr():
    t = make_trainer(learning_rate=1e-3, num_warmup_steps=4, dropout=P)
    yield t
    t.close()


@pytest.fixture(scope="module")
def refs():
    """float64 and float32 autograd of the restatement for each case, computed once."""
    cache = {}

    def get(B, T, p=0.0, V=0, cond=None):
        key = (B, T, p, V, None if cond is None else tuple(cond))
        if key not in cache:
            d = batch(B, T, V)
            out = []
            for dt in (torch.float64, torch.float32):
                masks = ref.dropout_masks(SEED, B, T, p)
                kw = dict(std=d.get("std"), deltas=d.get("deltas"), masks=masks)
                ac = UNetTrainer_alphas()
                out.append(ref.loss_and_grads(trainable(dt), ac, d["coeffs"], d["noise"], d["timesteps"], d["audio"],
                                              d["cond"] if cond is None else cond, **kw))
            cache[key] = out
        return cache[key]

    return get


_AC = []


def UNetTrainer_alphas():
    if not _AC:
        from said_amd.scheduler import DDIMScheduler
        _AC.append(DDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2").alphas_cumprod.float())
    return _AC[0]


def gpu_grads(tr, B, T, p, V=0, cond=None):
    d = batch(B, T, V)
    tr.load_state_dict(full_sd())
    tr.dropout = p
    tr.std = None if "std" not in d else d["std"].numpy()
    out = tr.step(d["coeffs"], d["cond"] if cond is None else cond, d["audio"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED,
                  deltas=d.get("deltas"))
    tr.std = None
    return out, tr.parameters_of(_engine.UT_GRAD)


@pytest.mark.parametrize("B,T", SHAPES)
def test_forward(tr, B, T):
    d = batch(B, T)
    x = d["coeffs"] + 0.3 * d["noise"]
    got = tr.forward_only(x, d["timesteps"], d["cond"], d["audio"])
    with torch.no_grad():
        r64 = ref.forward(trainable(torch.float64), x, d["timesteps"], d["audio"], d["cond"])
        r32 = ref.forward(trainable(torch.float32), x, d["timesteps"], d["audio"], d["cond"])
    ok, msg = check("output", got, r32, r64, {})
    print("forward", msg)
    assert ok, msg


@pytest.mark.parametrize("p", [0.0, P])
@pytest.mark.parametrize("B,T", SHAPES)
def test_gradients(tr, refs, B, T, p):
    (l64, g64), (l32, g32) = refs(B, T, p)
    out, g = gpu_grads(tr, B, T, p)
    assert abs(float(out.predict) - float(l64[0])) <= 4 * max(abs(float(l32[0]) - float(l64[0])), 1e-6 * float(l64[0]))
    assert abs(float(out.velocity) - float(l64[1])) <= 4 * max(abs(float(l32[1]) - float(l64[1])), 1e-6 * float(l64[1]))
    worst, bad = {}, []
    for k in g64:
        ok, msg = check(k, g[k], g32[k], g64[k], worst)
        if not ok:
            bad.append(msg)
    k = max(worst, key=lambda n: worst[n][0])
    print(f"gradients B={B} T={T} p={p}: worst {k} hip {worst[k][0]:.3e} cpu-fp32 {worst[k][1]:.3e}; failing {len(bad)}")
    assert not bad, bad[:8]


def test_null_cond_emb_gradient(tr, refs):
    (_, g64), (_, g32) = refs(2, 40, 0.0)
    _, g = gpu_grads(tr, 2, 40, 0.0)
    assert g["null_cond_emb"].abs().max() > 0
    ok, msg = check("null_cond_emb", g["null_cond_emb"], g32["null_cond_emb"], g64["null_cond_emb"], {})
    assert ok, msg
    _, g = gpu_grads(tr, 2, 40, 0.0, cond=[True, True])
    assert g["null_cond_emb"].abs().max() == 0


def test_vertex_loss_with_std(tr, refs):
    (l64, g64), (l32, g32) = refs(2, 40, 0.0, V=7)
    out, g = gpu_grads(tr, 2, 40, 0.0, V=7)
    assert abs(float(out.vertex) - float(l64[2])) <= 4 * max(abs(float(l32[2]) - float(l64[2])), 1e-6 * float(l64[2]))
    worst, bad = {}, []
    for k in g64:
        ok, msg = check(k, g[k], g32[k], g64[k], worst)
        if not ok:
            bad.append(msg)
    assert not bad, bad[:8]


def test_three_steps(tr):
    B, T = 2, 40
    d = batch(B, T)
    lam, dec = constant_with_warmup_lambda(4), (lambda n: ema_decay(n, 0.9999))
    runs = []
    for dt in (torch.float64, torch.float32):
        rt = ref.RefTrainer(trainable(dt), 1e-3, lam, dec)
        for k in range(3):
            g = torch.Generator().manual_seed(k)
            rt.step(UNetTrainer_alphas(), d["coeffs"], torch.randn(B, T, 32, generator=g), d["timesteps"], d["audio"], d["cond"],
                    masks=ref.dropout_masks(SEED + k, B, T, P))
        runs.append(rt)
    r64, r32 = runs
    assert min(r64.clip_factors) < 1.0, "the clip must be active on at least one step"
    tr.load_state_dict(full_sd())
    tr.dropout = P
    for k in range(3):
        g = torch.Generator().manual_seed(k)
        tr.enqueue_step(d["coeffs"], d["cond"], d["audio"], noise=torch.randn(B, T, 32, generator=g), timesteps=d["timesteps"], dropout_seed=SEED + k)
    bad = []
    for which, a64, a32 in ((_engine.UT_STATE, r64.p, r32.p), (_engine.UT_EXP_AVG, r64.m, r32.m), (_engine.UT_EXP_AVG_SQ, r64.v, r32.v),
                            (_engine.UT_EMA, r64.ema, r32.ema)):
        got = tr.parameters_of(which)
        for k in a64:
            ok, msg = check(k, got[k], a32[k], a64[k], {})
            if not ok:
                bad.append((which,) + msg)
    assert not bad, bad[:8]


@pytest.mark.parametrize("grad_scale", [1e-4, 10.0])
def test_clip_adamw_ema_update(grad_scale):
    """The BCVAE trainer's test of the same name on this trainer (the same kernels): one clip + AdamW + EMA update from set gradients over the
    161 tensors against torch's fp32 clip_grad_norm_ and AdamW and the EMA formula.  The update touches no activation, so the context is the
    smallest there is.

    Bounds: the BCVAE test's 4 ulps for exp_avg and exp_avg_sq and 8 for the EMA shadow; 12 for the parameters.  The kernels as they were
    before both trainers shared them measured, on this trainer, a worst distance of 6 ulps for the parameters with grad_scale 1e-4 (one
    element of middle_block.2.out_layers.3.weight; the clip factor is exactly 1 there, so the norm plays no part) and 4 with grad_scale 10;
    1 for exp_avg, 1 for exp_avg_sq, 2 for the EMA shadow.  The bound for the parameters is twice that worst distance: the update
    p (1 - lr wd) - step_size m / (sqrt(v) / bc2 + eps) is rounded five times here and in another order in torch's addcdiv_, and 7.0 M
    elements reach further into the tail of that difference than the BCVAE's 0.67 M."""
    t = make_trainer(max_batch=1, max_frames=2)
    nparam = sum(int(np.prod(s)) for s in trainable_shapes().values())
    check_clip_adamw_ema_update(t, (_engine.UT_STATE, _engine.UT_GRAD, _engine.UT_EXP_AVG, _engine.UT_EXP_AVG_SQ, _engine.UT_EMA),
                                lambda k: t._scalars(1.0, 0.02, k, 0.0), grad_scale, nparam ** 0.5, bounds=(12, 4, 4, 8))
    t.close()


def test_step_is_bit_identical(tr):
    _, g1 = gpu_grads(tr, 3, 121, P)
    p1 = tr.parameters_of(_engine.UT_STATE)
    _, g2 = gpu_grads(tr, 3, 121, P)
    p2 = tr.parameters_of(_engine.UT_STATE)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
        assert torch.equal(p1[k], p2[k]), k


def test_eval_loss_on_ema(tr):
    B, T = 2, 40
    d = batch(B, T)
    tr.load_state_dict(full_sd())
    tr.dropout = P
    for k in range(2):
        tr.enqueue_step(d["coeffs"], d["cond"], d["audio"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED + k)
    ema = tr.parameters_of(_engine.UT_EMA)
    tr.epoch_output(False)
    tr.eval_loss(d["coeffs"], d["cond"], d["audio"], noise=d["noise"], timesteps=d["timesteps"], use_ema=True)
    got = tr.epoch_output(True)
    vals = []
    for dt in (torch.float64, torch.float32):
        sd = {k: v.to(dt) for k, v in ema.items()}
        with torch.no_grad():
            noisy, answer = ref.add_noise(UNetTrainer_alphas(), d["coeffs"], d["noise"], d["timesteps"], "epsilon", dt)
            vals.append([float(x) for x in ref.objective(ref.forward(sd, noisy, d["timesteps"], d["audio"], d["cond"]), answer)[:2]])
    for g, v64, v32 in zip((got.predict, got.velocity), *vals):
        assert abs(g - v64) <= 4 * max(abs(v32 - v64), 1e-6 * abs(v64)), (g, v64, v32)


@pytest.mark.parametrize("prediction_type", ["sample", "v_prediction"])
def test_gradients_of_the_other_prediction_types(prediction_type):
    """epsilon runs in every test above; the other two answers of add_noise, B = 2, T = 40, no dropout."""
    B, T = 2, 40
    d = batch(B, T)
    out = [ref.loss_and_grads(trainable(dt), UNetTrainer_alphas(), d["coeffs"], d["noise"], d["timesteps"], d["audio"], d["cond"],
                              prediction_type=prediction_type) for dt in (torch.float64, torch.float32)]
    (l64, g64), (l32, g32) = out
    t = make_trainer(max_batch=2, max_frames=40, dropout=0.0, prediction_type=prediction_type)
    res = t.step(d["coeffs"], d["cond"], d["audio"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=0)
    g = t.parameters_of(_engine.UT_GRAD)
    t.close()
    assert abs(float(res.predict) - float(l64[0])) <= 4 * max(abs(float(l32[0]) - float(l64[0])), 1e-6 * float(l64[0]))
    bad = [m for ok, m in (check(k, g[k], g32[k], g64[k], {}) for k in g64) if not ok]
    assert not bad, bad[:8]


def test_checkpoint_loads_into_the_inference_model(tr):
    """UNetTrainer.state_dict() has SAID_UNet1D's key set (audio_encoder.* passed through) and the loaded model's forward is the trainer's
    forward_only (the inference engine multiplies on split-fp16 operands: 2e-4 of the output's scale)."""
    from said_amd.model.diffusion import SAID_UNet1D
    B, T = 2, 40
    d = batch(B, T)
    tr.load_state_dict(full_sd())
    tr.dropout = P
    tr.enqueue_step(d["coeffs"], d["cond"], d["audio"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED)
    sd = tr.state_dict()
    assert set(sd) == set(full_sd()) and list(sd)[0] == "null_cond_emb"
    for k, v in full_sd().items():
        if k.startswith("audio_encoder."):
            assert torch.equal(sd[k], v), k
    from said_amd.model.wav2vec2 import AudioConfig
    model = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=1))
    model.load_state_dict(sd, strict=True)
    model.to("cuda:0")
    x = d["coeffs"] + 0.3 * d["noise"]
    want = tr.forward_only(x, d["timesteps"], [True, True], d["audio"])
    with torch.no_grad():
        got = model(x.to("cuda:0"), d["timesteps"].to("cuda:0"), d["audio"].to("cuda:0")).cpu()
    assert float((got - want).abs().max()) <= 2e-4 * float(want.abs().max()), float((got - want).abs().max())


def test_train_cli_two_epochs(tmp_path):
    """script/train.py as a fresh child process: 2 epochs on a synthetic 2-speaker, 2-sentence set; 2.pth has the full key set."""
    import os
    import subprocess
    import sys
    from scipy.io import wavfile
    from said_amd.training.vae import PERSON_IDS_TRAIN
    from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, save_blendshape_coeffs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    out = subprocess.run([sys.executable, os.path.join(root, "script", "train.py"), "--audio_dir", str(tmp_path / "audio"), "--coeffs_dir",
                          str(tmp_path / "coeffs"), "--output_dir", str(tmp_path / "out"), "--window_size_min", "40", "--epochs", "2", "--batch_size", "2",
                          "--save_period", "2", "--val_period", "1", "--num_warmup_epochs", "1", "--audio_encoder_weights", "synthetic", "--seed", "0",
                          "--device", "cuda:0"], capture_output=True, text=True, timeout=240, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    sd = torch.load(str(tmp_path / "out" / "2.pth"), map_location="cpu")
    from said_amd.util.synth import said_state_dict as full
    assert set(sd) == set(full())
    assert all(torch.isfinite(v).all() for v in sd.values())
    assert len(open(tmp_path / "out" / "log.csv").read().splitlines()) == 3
