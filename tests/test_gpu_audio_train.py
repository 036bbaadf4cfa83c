"""The audio encoder's train mode on the MI355X (include/said_audio_train.h, said_amd/csrc/audio_train.hip) against the float64 restatement
of the same forward on the same inputs (tests/audio_train_ref.py): mask, skipped layers, seed and probabilities are given to both sides.

Tolerance of the comparisons with the restatement.  Kept and dropped elements are equal by construction (the keep rule compares
integers), so what remains is fp32 arithmetic, bounded the way DESIGN.md 16.7 bounds the trainer: max abs error against float64,
relative to max(1, |ref|max), at most 4 x the error of the float32 CPU evaluation of the same restatement on the same inputs (the factor
covers reduction orders that differ from torch's), with the eval route's own bound AUDIO_TOL (tests/test_gpu_parity.py) as the floor.
The float32 error is computed here: it is the reference's error, not the code's.

Attention instantiations of the train route (audio_enc.cpp: eight key-split waves up to 2048 (clip, head, query tile) triples per
launch, four above; product mode 2 = split-fp16 under "fp32", 0 = fp32 MFMAs under "fp32_strict"):
  attn_drop_kernel<8, 2>: every case at B <= 3 in the default mode        attn_drop_kernel<8, 0>: test_strict_mode (B = 3, 70 frames)
  attn_drop_kernel<4, 2>: test_large_token_count["fp32"]                 attn_drop_kernel<4, 0>: test_large_token_count["fp32_strict"]
  (B = 22 clips of 225 frames: 22 x 8 query tiles x 12 heads = 2112 triples in one pass of up to 32 clips)
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import audio_train_ref as ref
from oracle import wav2vec2 as ow
from said_amd import _engine
from said_amd.model.diffusion import SAID_UNet1D
from said_amd.model.wav2vec2 import AudioConfig, AudioTrainConfig, AudioTrainDraws, compute_mask_indices
from said_amd.util import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
AUDIO_TOL = 4e-6          # tests/test_gpu_parity.py: the eval route's bound, x max(1, |ref|max)
SEED = 0x1234567887654321
TA = 8000                 # 0.5 s: 24 conv frames, interpolated to the frame count of each case
KINDS = ref.KINDS         # said_debug_option "audio_train_sites": isolates the three sites that share p_hidden
_REFS = {}                # run_case's references by case
ZERO = dict(feat_proj_dropout=0.0, hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, mask_time_prob=0.0, layerdrop=0.0)


@functools.lru_cache(maxsize=None)
def full_sd(layers):
    return synth.said_state_dict(num_w2v_layers=layers)


@functools.lru_cache(maxsize=None)
def w2v_sd(layers):
    return {k[len("audio_encoder."):]: v for k, v in full_sd(layers).items() if k.startswith("audio_encoder.")}


@functools.lru_cache(maxsize=None)
def model_for(layers):
    m = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=layers))
    m.load_state_dict(full_sd(layers), strict=True)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def inputs(B, frames, layers):
    """The processed waveforms and the conv features after interpolation in both precisions: computed once per shape and never modified."""
    proc = model_for(layers).process_audio([synth.synth_waveform(i, TA).numpy() for i in range(B)])
    return proc, ref.features(w2v_sd(layers), proc, frames, torch.float64), ref.features(w2v_sd(layers), proc, frames, torch.float32)


def span_mask(B, frames):
    np.random.seed(100 * B + frames)
    return compute_mask_indices((B, frames), 0.05, 10, 2)


def run_case(B, frames, layers, mask=None, skip=(), p=None, sites=-1, mode="fp32", seed=SEED):
    """One train-mode encode on the GPU and the restatement's float64 / float32 evaluations of it; returns (error, float32 error, bound)."""
    p = {**dict(p_feat_proj=0.0, p_hidden=0.0, p_attention=0.0, p_activation=0.0), **(p or {})}
    cfg = AudioTrainConfig(feat_proj_dropout=p["p_feat_proj"], hidden_dropout=p["p_hidden"], attention_dropout=p["p_attention"],
                           activation_dropout=p["p_activation"])
    proc, f64, f32 = inputs(B, frames, layers)
    model = model_for(layers)
    skip_flags = tuple(l in set(skip) for l in range(layers))
    model.set_mfma_dtype(mode)
    try:
        model._get_engine(1, frames).debug_option("audio_train_sites", sites)
        got = model.get_audio_embedding(proc.to(DEV), frames, train_draws=AudioTrainDraws(mask, skip_flags, seed), train_cfg=cfg).cpu().double()
    finally:
        model._get_engine(1, frames).debug_option("audio_train_sites", -1)
        model.set_mfma_dtype("fp32")
    key = (B, frames, layers, None if mask is None else mask.tobytes(), tuple(skip), tuple(sorted(p.items())), sites, seed)
    if key not in _REFS:   # the two precision modes of a case share their reference
        kinds = None if sites < 0 else {k for k, bit in ref.KINDS.items() if sites & bit}
        kw = dict(mask=mask, skip=skip, seed=seed, kinds=kinds, **p)
        with torch.no_grad():
            _REFS[key] = (ref.forward(w2v_sd(layers), proc, frames, dtype=torch.float64, feats=f64, **kw),
                          ref.forward(w2v_sd(layers), proc, frames, dtype=torch.float32, feats=f32, **kw))
    r64, r32 = _REFS[key]
    scale = max(1.0, float(r64.abs().max()))
    err, e32 = float((got - r64).abs().max()) / scale, float((r32.double() - r64).abs().max()) / scale
    return err, e32, max(4 * e32, AUDIO_TOL), got


def check(name, err, e32, bound):
    print(f"{name}: max abs err / max(1, |ref|max) = {err:.3e}; float32 CPU restatement {e32:.3e}; bound {bound:.3e}")
    assert err <= bound, (name, err, e32, bound)


ALL_ON = dict(p_feat_proj=0.1, p_hidden=0.1, p_attention=0.1, p_activation=0.1)
ISOLATION = {
    "mask": dict(mask=True),
    "skip_layer_0": dict(skip=(0,)),
    "skip_all": dict(skip=(0, 1)),
    "feat_proj": dict(p=dict(p_feat_proj=0.1)),
    "front": dict(p=dict(p_hidden=0.1), sites=KINDS["front"]),
    "attention": dict(p=dict(p_attention=0.1)),
    "attn_out": dict(p=dict(p_hidden=0.1), sites=KINDS["attn_out"]),
    "activation": dict(p=dict(p_activation=0.1)),
    "ffn_out": dict(p=dict(p_hidden=0.1), sites=KINDS["ffn_out"]),
    "attention_p05": dict(p=dict(p_attention=0.5)),
    "everything": dict(mask=True, skip=(1,), p=ALL_ON),
}


@pytest.mark.parametrize("run", list(ISOLATION))
@pytest.mark.parametrize("B,frames", [(2, 30), (3, 70)])
def test_site_isolation(B, frames, run):
    """Two layers; B = 2 with 30 frames is one partial 32-token tile, B = 3 with 70 frames three key tiles, the last partial."""
    spec = dict(ISOLATION[run])
    if spec.pop("mask", False):
        spec["mask"] = span_mask(B, frames)
    err, e32, bound, got = run_case(B, frames, 2, **spec)
    check(f"{run} B={B} frames={frames}", err, e32, bound)
    if run not in ("skip_all",):   # the switch must do something: the eval result differs
        proc = inputs(B, frames, 2)[0]
        assert not torch.equal(got.float(), model_for(2).get_audio_embedding(proc.to(DEV), frames).cpu())


def test_full_depth():
    """Twelve layers, B = 2, 70 frames, everything on, two layers skipped."""
    err, e32, bound, _ = run_case(2, 70, 12, mask=span_mask(2, 70), skip=(3, 7), p=ALL_ON)
    check("full depth", err, e32, bound)


def test_strict_mode():
    """fp32 matrix instructions (attn_drop_kernel<8, 0>): everything on at B = 3, 70 frames."""
    err, e32, bound, _ = run_case(3, 70, 2, mask=span_mask(3, 70), skip=(1,), p=ALL_ON, mode="fp32_strict")
    check("strict", err, e32, bound)


@pytest.mark.parametrize("mode", ["fp32", "fp32_strict"])
def test_large_token_count(mode):
    """22 clips of 225 frames on one-layer weights: 2112 (clip, head, query tile) triples in one pass, so the four-wave key split
    (attn_drop_kernel<4, PM>); 225 = 7 x 32 + 1 leaves one key in the last tile."""
    err, e32, bound, _ = run_case(22, 225, 1, mask=span_mask(22, 225), p=ALL_ON, mode=mode)
    check(f"large {mode}", err, e32, bound)


def test_chunk_independence_and_repeatability():
    B, frames = 3, 70
    proc = inputs(B, frames, 2)[0].to(DEV)
    model, cfg = model_for(2), AudioTrainConfig()
    mask = span_mask(B, frames)
    draws = AudioTrainDraws(mask, (False, False), SEED)
    one = model.get_audio_embedding(proc, frames, train_draws=draws, train_cfg=cfg)
    assert torch.equal(one, model.get_audio_embedding(proc, frames, train_draws=draws, train_cfg=cfg)), "same seed, same result"
    assert not torch.equal(one, model.get_audio_embedding(proc, frames, train_draws=AudioTrainDraws(mask, (False, False), SEED + 1), train_cfg=cfg))
    eng = model._get_engine(1, frames)
    eng.debug_option("audio_chunk", 1)
    try:
        split = model.get_audio_embedding(proc, frames, train_draws=draws, train_cfg=cfg)
    finally:
        eng.debug_option("audio_chunk", 32)
    assert torch.equal(one, split), "masks are indexed by the call's clip index, not the pass's"


def test_all_off_is_the_eval_forward():
    """Every probability 0, no mask, no skips: within the eval route's own bound of the oracle; and get_audio_embedding without draws is
    the call it always was, bit for bit."""
    B, frames = 3, 70
    proc = inputs(B, frames, 2)[0]
    model = model_for(2)
    want = ow.wav2vec2_forward(w2v_sd(2), proc, frames)[0]
    got = model.get_audio_embedding(proc.to(DEV), frames, train_draws=AudioTrainDraws(None, (False, False), 0), train_cfg=AudioTrainConfig(**ZERO)).cpu()
    err = float((got - want).abs().max())
    print(f"all off vs oracle: max abs err {err:.3e} (|ref| max {float(want.abs().max()):.2f})")
    assert err <= AUDIO_TOL * max(1.0, float(want.abs().max()))
    a = model.get_audio_embedding(proc.to(DEV), frames).cpu()
    b = model._get_engine(1, frames).audio_encode(proc.to(DEV), frames).cpu()
    assert torch.equal(a, b) and float((a - want).abs().max()) <= AUDIO_TOL * max(1.0, float(want.abs().max()))


def test_refusals():
    B, frames = 2, 30
    proc = inputs(B, frames, 2)[0].to(DEV)
    model = model_for(2)
    draws = AudioTrainDraws(span_mask(B, frames), (False, False), SEED)
    model.set_mfma_dtype("bf16")
    try:
        with pytest.raises(_engine.EngineError, match="bf16 mode"):
            model.get_audio_embedding(proc, frames, train_draws=draws)
    finally:
        model.set_mfma_dtype("fp32")
    with pytest.raises(ValueError, match=r"outside \[0, 1\)"):
        model.get_audio_embedding(proc, frames, train_draws=draws, train_cfg=AudioTrainConfig(attention_dropout=1.0))
    with pytest.raises(NotImplementedError, match="mask_feature_prob"):
        model.get_audio_embedding(proc, frames, train_draws=draws, train_cfg=AudioTrainConfig(mask_feature_prob=0.05))
    eng = model._get_engine(1, frames)
    out, got = torch.empty(B, frames, 768, device=DEV), _engine.c_int(0)
    bad = _engine.AudioTrainParams(0.1, -0.5, 0.1, 0.1, SEED, None, 0)   # the library's own check, past the Python one
    with pytest.raises(_engine.EngineError, match=r"outside \[0, 1\)"):
        eng._call("said_audio_encode_train", _engine._ptr(proc), B, proc.shape[1], frames, 0, _engine.ctypes.byref(bad), _engine._ptr(out),
                  _engine.ctypes.byref(got), _engine._stream())
    with pytest.raises(_engine.EngineError, match="does not match"):
        model.get_audio_embedding(proc, frames, train_draws=AudioTrainDraws(span_mask(B, frames + 1), (False, False), SEED))
    # a context whose weights came without masked_spec_embed: fine without a mask, a clean error with one
    bare = _engine.Engine(torch.device(DEV), 2, 64)
    try:
        bare.load_weights({k: v for k, v in full_sd(2).items() if k != "audio_encoder.masked_spec_embed"})
        with pytest.raises(_engine.EngineError, match="masked_spec_embed"):
            bare.audio_encode_train(proc, frames, draws, AudioTrainConfig())
        no_mask = bare.audio_encode_train(proc, frames, AudioTrainDraws(None, (False, False), SEED), AudioTrainConfig()).cpu()
        assert torch.equal(no_mask, model.get_audio_embedding(proc, frames, train_draws=AudioTrainDraws(None, (False, False), SEED)).cpu())
    finally:
        bare.close()


# ------------------------------------------------------------------------------------------------ trainer and CLI
def _epoch(audio_train):
    """One train_epoch on a tiny synthetic set (two clips, batch 2, one-layer encoder) from fixed seeds: (losses, parameters)."""
    import random
    from said_amd.training import TrainWindowDataset, UNetTrainer, make_unet_dataloaders
    random.seed(11)
    np.random.seed(11)
    torch.manual_seed(11)
    rng = np.random.default_rng(0)
    items = []
    for frames in (50, 63):
        n = 16000 * frames // 60
        items.append((0.3 * np.sin(2 * np.pi * 200 * np.arange(n) / 16000).astype(np.float32), np.clip(0.3 + np.cumsum(rng.normal(0, 0.02, (frames, 32)), 0), 0, 1).astype(np.float32)))
    ds = TrainWindowDataset(items=items, window_size_min=40)
    loader, _ = make_unet_dataloaders(ds, None, 2)
    tr = UNetTrainer(full_sd(1), DEV, max_batch=2, max_frames=64)
    try:
        out = tr.train_epoch(model_for(1), loader, 1.0, 0.02, audio_train=audio_train)
        return (out.total, out.predict, out.velocity), {k: v.clone() for k, v in tr.state_dict().items() if not k.startswith("audio_encoder.")}
    finally:
        tr.close()


def test_train_epoch_with_the_encoder_in_train_mode():
    l1, p1 = _epoch(AudioTrainConfig())
    l2, p2 = _epoch(AudioTrainConfig())
    l0, p0 = _epoch(None)
    assert l1 == l2 and all(torch.equal(p1[k], p2[k]) for k in p1), "same seeds: bit-identical losses and parameters"
    assert l1 != l0 and any(not torch.equal(p1[k], p0[k]) for k in p1), "the encoder's mode must reach the step"
    assert all(np.isfinite(v) for v in l1)


@pytest.fixture(scope="module")
def cli_data(tmp_path_factory):
    """The synthetic 2-speaker, 2-sentence set of tests/test_gpu_unet_train.py::test_train_cli_two_epochs."""
    from scipy.io import wavfile
    from said_amd.training.vae import PERSON_IDS_TRAIN
    from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, save_blendshape_coeffs
    tmp = tmp_path_factory.mktemp("audio_train_cli")
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "script", "train.py"), "--audio_dir", str(tmp / "audio"), "--coeffs_dir", str(tmp / "coeffs"),
                        "--output_dir", str(tmp / out), "--window_size_min", "40", "--epochs", "2", "--batch_size", "2", "--save_period", "2",
                        "--val_period", "1", "--num_warmup_epochs", "1", "--audio_encoder_weights", "synthetic", "--seed", "0", "--device", DEV, *extra],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return open(tmp / out / "log.csv").read().splitlines()


def test_train_cli_in_train_mode(cli_data):
    log = _train_cli(cli_data, "out_train", "--audio_encoder_mode", "train")
    assert len(log) == 3
    sd = torch.load(str(cli_data / "out_train" / "2.pth"), map_location="cpu")
    assert set(sd) == set(synth.said_state_dict()) and all(torch.isfinite(v).all() for v in sd.values())
    assert log != open(os.path.join(ROOT, "tests", "golden", "train_log_seed0_eval.csv")).read().splitlines()


def test_train_cli_default_log_is_unchanged(cli_data):
    """tests/golden/train_log_seed0_eval.csv: log.csv of this command at the commit before --audio_encoder_mode existed."""
    assert _train_cli(cli_data, "out_eval") == open(os.path.join(ROOT, "tests", "golden", "train_log_seed0_eval.csv")).read().splitlines()
