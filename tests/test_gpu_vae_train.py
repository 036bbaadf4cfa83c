"""BCVAE training on the MI355X (include/said_train.h, said_amd/csrc/vae_train.hip; said_amd.training; script/train_vae.py) against the
float64 restatement of the reference step (tests/vae_train_ref.py) on the golden G14 windows and noise.

Tolerances come from torch's own fp32 CPU run against fp64 on the same 20 steps (batch 8, lr 1e-4, default init): the loss components
deviate by at most 2.8e-6 (reconst), 1.9e-4 (kld: a sum of mu^2 + e^lv - lv - 1 terms that cancel), 2.4e-5 (velocity), 4.8e-6 (total).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from said_amd import _engine
from said_amd.training import BCVAETrainer, VAEWindowDataset, bcvae_init_state_dict
from said_amd.training.vae import BN_CANCELLED_BIASES
from train_opt_check import check_clip_adamw_ema_update
from vae_train_ref import RefTrainer, encode_eval, forward, split_state, windows_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G14 = np.load(os.path.join(ROOT, "tests", "golden", "g14_vae_train.npz"))
LR, N = float(G14["lr"]), 20


def golden_seqs():
    lengths, frames = G14["lengths"], G14["frames"]
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    return [frames[o:o + n] for o, n in zip(offs, lengths)]


def init_sd():
    torch.manual_seed(0)
    return bcvae_init_state_dict()


def make_trainer(max_batch=8, use_graph=True, **kw):
    tr = BCVAETrainer("cuda:0", max_batch=max_batch, learning_rate=LR, num_training_steps=N, state_dict=init_sd(), use_graph=use_graph, **kw)
    tr.set_train_data(VAEWindowDataset(sequences=golden_seqs()))
    return tr


@pytest.fixture(scope="module")
def runs():
    """20 steps on the GPU and in float64 on the CPU, with the step-1 gradients and BatchNorm statistics of both."""
    tr = make_trainer()
    rt = RefTrainer(init_sd(), lr=LR, num_training_steps=N)
    seqs, items, eps = golden_seqs(), G14["items"], G14["eps"]
    gl, rl = [], []
    for k in range(N):
        out = tr.step(items[k], eps[k])
        gl.append([float(out.reconst), float(out.regularize), float(out.velocity)])
        rl.append(rt.step(windows_of(seqs, items[k], G14["mirror"]), eps[k])[:3])
        if k == 0:
            g1, r1 = tr.parameters_of(_engine.TRAIN_GRAD), rt.last_grads
            bn1 = [tr.eng.bn_stats(i, c) for i, c in enumerate((32, 64, 64, 256, 128, 240, 32, 32))]
            sd1 = tr.state_dict(ema=False)
            ref_sd1 = rt.state()
    return dict(tr=tr, rt=rt, gl=np.array(gl), rl=np.array(rl), g1=g1, r1=r1, bn1=bn1, sd1=sd1, ref_sd1=ref_sd1)


def test_gather_matches_window_cut():
    tr = make_trainer()
    items = G14["items"][3].copy()
    items[1, 3] = 1   # a zeroed window
    items[2, 1] = -60
    np.testing.assert_array_equal(tr.eng.gather(_engine.TRAIN_SET_TRAIN, items), windows_of(golden_seqs(), items, G14["mirror"]))


def test_step1_gradients(runs):
    g1, r1 = runs["g1"], runs["r1"]
    for k, r in r1.items():
        r = r.double()
        g = g1[k].double()
        if k in BN_CANCELLED_BIASES:
            continue
        scale = r.abs().max().item()
        assert (g - r).abs().max().item() <= 3e-5 * scale, (k, (g - r).abs().max().item(), scale)
    # The nine biases followed by a BatchNorm: the BatchNorm subtracts the batch mean, so their exact gradient is 0 and any fp32 value is the
    # rounding residue of sum(da) over the B x L positions, whose terms are of the size of the layer's output gradients.  Bound: 1e-3 of the
    # largest gradient of the weight beside them (the fp32 residue is around 1e-6 of it).
    for k in BN_CANCELLED_BIASES:
        assert r1[k].abs().max().item() < 1e-9
        wscale = r1[k.replace(".bias", ".weight")].abs().max().item()
        assert g1[k].abs().max().item() <= 1e-3 * wscale, (k, g1[k].abs().max().item(), wscale)


def test_batch_and_running_statistics_after_one_step(runs):
    sd1, ref = runs["sd1"], runs["ref_sd1"]
    from vae_train_ref import BN_LAYERS
    for i, name in enumerate(BN_LAYERS):
        rm, rv = ref[name + ".running_mean"], ref[name + ".running_var"]
        assert int(sd1[name + ".num_batches_tracked"]) == 1 and sd1[name + ".num_batches_tracked"].dtype == torch.int64
        np.testing.assert_allclose(sd1[name + ".running_mean"].double(), rm, atol=2e-6 * max(1.0, rm.abs().max().item()))
        np.testing.assert_allclose(sd1[name + ".running_var"].double(), rv, rtol=2e-5)
        # the batch statistics behind them: mean = running_mean / 0.1, biased var from the unbiased one
        n = 8 * {0: 118, 1: 116, 2: 57, 6: 122, 7: 124}.get(i, 1)
        mean, invstd = runs["bn1"][i]
        var = (rv - 0.9) / 0.1 * (n - 1) / n
        np.testing.assert_allclose(mean, rm / 0.1, atol=2e-5 * max(1.0, (rm / 0.1).abs().max().item()))
        np.testing.assert_allclose(invstd, 1 / torch.sqrt(var + 1e-5), rtol=2e-5)


@pytest.mark.parametrize("grad_scale", [1e-4, 10.0])
def test_clip_adamw_ema_update(grad_scale):
    """One clip + AdamW + EMA update from set gradients against torch's fp32 clip_grad_norm_ and AdamW and the EMA formula; grad_scale 10
    makes the clip active, 1e-4 leaves it off."""
    tr = make_trainer()
    check_clip_adamw_ema_update(tr, (_engine.TRAIN_STATE, _engine.TRAIN_GRAD, _engine.TRAIN_EXP_AVG, _engine.TRAIN_EXP_AVG_SQ, _engine.TRAIN_EMA),
                                lambda k: tr._scalars(1.0, 1.0, k), grad_scale, 800.0)


def test_trajectory_against_float64(runs):
    gl, rl = runs["gl"], runs["rl"]
    rel = np.abs(gl / rl - 1).max(0)
    assert rel[0] <= 1e-5 and rel[1] <= 1e-3 and rel[2] <= 1e-4, rel
    tr, rt = runs["tr"], runs["rt"]
    got, ref = tr.state_dict(ema=False), rt.state()
    for k, r in ref.items():
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == N
            continue
        d = (got[k].double() - r.double()).abs().max().item()
        if k in BN_CANCELLED_BIASES:   # Adam turns noise-level gradients into +-lr steps: a random walk bounded by lr per step
            assert d <= 2 * LR * N, (k, d)
        elif k.endswith(("running_mean", "running_var")):
            # torch's fp32 CPU run on these windows: 2.2e-4 (running_mean: it follows the random walk of the bias before it) and 6.5e-5
            assert d <= (1e-3 if k.endswith("running_mean") else 5e-4) * max(1.0, r.abs().max().item()), (k, d)
        else:
            # torch's own fp32 CPU step on these windows ends 3.04e-2 lr N from float64 on encoder.fc_layers.0.weight (99.9th percentile
            # 1.2e-2 lr N): windows padded by replication give near-constant features whose weight gradients cancel to noise, which Adam
            # turns into +-lr steps like the nine biases.  Bound the worst element at 4e-2 lr N and the 99.9th percentile at 3e-2 lr N.
            e = (got[k].double() - r.double()).abs().flatten()
            assert d <= 4e-2 * LR * N and torch.quantile(e, 0.999).item() <= 3e-2 * LR * N, (k, d)
    ema_got, ema_ref = tr.state_dict(ema=True), rt.state(ema=True)
    for k in tr.parameters_of(_engine.TRAIN_STATE):
        d = (ema_got[k].double() - ema_ref[k].double()).abs().max().item()
        assert d <= (2 * LR * N if k in BN_CANCELLED_BIASES else 4e-2 * LR * N), (k, d)


def test_checkpoint_loads_and_encodes(runs):
    """The saved state dict loads strictly into said_amd.model.vae.BCVAE; its eval encode and decode match the restatement's."""
    from said_amd.model.vae import BCVAE
    tr, rt = runs["tr"], runs["rt"]
    sd = tr.state_dict(ema=True)
    vae = BCVAE()
    vae.load_state_dict(sd, strict=True)
    vae.to("cuda:0").eval()
    x = torch.from_numpy(windows_of(golden_seqs(), G14["items"][0], G14["mirror"]))
    p, b = split_state(sd)
    mean_r, lv_r = encode_eval(p, b, x.double())
    lat = vae.encode(x.cuda())
    for got, ref in ((lat.mean, mean_r), (lat.log_var, lv_r)):
        assert (got.cpu().double() - ref).abs().max().item() <= 2e-3 * (ref.max() - ref.min()).item()
    # decode: the restated decoder (eval) on the same latents
    z = mean_r.float()
    with torch.no_grad():
        _, _, y_r = forward(p, b, x.double(), torch.zeros(8, 64, dtype=torch.float64), train=False)
    y = vae.decode(z.cuda()).cpu().double()
    assert (y - y_r).abs().max().item() <= 2e-3 * max((y_r.max() - y_r.min()).item(), 1e-3) + 1e-5


def _state_bits(tr):
    out = {}
    for which in (_engine.TRAIN_STATE, _engine.TRAIN_EMA, _engine.TRAIN_EXP_AVG, _engine.TRAIN_EXP_AVG_SQ):
        for k, v in tr.parameters_of(which).items():
            out[(which, k)] = v.numpy().tobytes()
    for k, v in tr.state_dict(ema=False).items():
        out[("sd", k)] = v.numpy().tobytes()
    return out


def test_bit_identical_graph_direct_and_repeat():
    items, eps = G14["items"], G14["eps"]
    states, losses = [], []
    for use_graph in (True, False, True):
        tr = make_trainer(use_graph=use_graph)
        for k in range(4):
            tr._step(items[k], eps[k], 1.0, 1.0)
        losses.append(tr.eng.read_losses(False)[0].tobytes())
        assert tr.eng.graph_count() == (1 if use_graph else 0)
        states.append(_state_bits(tr))
        tr.close()
    assert states[0] == states[1] == states[2]
    assert losses[0] == losses[1] == losses[2]


def test_batch_size_edges(tmp_path):
    tr = make_trainer()
    items, eps = G14["items"][0], G14["eps"][0]
    tr.step(items, eps)
    out = tr.step(items[:5], eps[:5])   # a short last batch: its own graph
    assert tr.eng.graph_count() == 2 and np.isfinite(float(out.reconst))
    rt = RefTrainer(init_sd(), lr=LR, num_training_steps=N)
    rt.step(windows_of(golden_seqs(), items, G14["mirror"]), eps)
    ref = rt.step(windows_of(golden_seqs(), items[:5], G14["mirror"]), eps[:5])
    assert abs(float(out.reconst) / ref[0] - 1) <= 1e-5
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        tr.step(items[:1], eps[:1])
    with pytest.raises(ValueError, match="32 values"):
        make_trainer(std=np.ones(31, np.float32))
    # a std of the right width: the losses reweighted out of place
    std = np.linspace(0.2, 1.0, 32).astype(np.float32)
    trs = make_trainer(std=std)
    out = trs.step(items, eps)
    rts = RefTrainer(init_sd(), lr=LR, num_training_steps=N, std=std)
    ref = rts.step(windows_of(golden_seqs(), items, G14["mirror"]), eps)
    assert abs(float(out.reconst) / ref[0] - 1) <= 1e-5 and abs(float(out.velocity) / ref[2] - 1) <= 1e-4


def _write_tree(root, pids, sids, rng, T=200):
    from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, save_blendshape_coeffs
    for pid in pids:
        os.makedirs(os.path.join(root, pid), exist_ok=True)
        for sid in sids:
            c = np.clip(0.5 + np.cumsum(rng.normal(scale=0.05, size=(T, 32)), axis=0), 0, 1).astype(np.float32)
            save_blendshape_coeffs(c, DEFAULT_BLENDSHAPE_CLASSES, os.path.join(root, pid, f"sentence{sid:02}.csv"))


def test_cli_end_to_end(tmp_path):
    import json
    from scipy.io import wavfile
    from said_amd.training import vae as tv
    rng = np.random.default_rng(0)
    coeffs = tmp_path / "coeffs"
    _write_tree(str(coeffs), tv.PERSON_IDS_TRAIN[:2], (1, 2, 3, 4, 5), rng)   # 10 sequences: batches of 8 and 2 (a batch of 1 raises)
    _write_tree(str(coeffs), tv.PERSON_IDS_VAL[:1], (1, 2), rng)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "script", "train_vae.py"), "--coeffs_dir", str(coeffs), "--output_dir", str(out), "--epochs", "2",
           "--val_period", "1", "--save_period", "1", "--val_repeat", "2", "--seed", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (out / "1.pth").exists() and (out / "2.pth").exists()
    logs = [json.loads(ln) for ln in open(out / "log.jsonl")]
    assert [d["epoch"] for d in logs] == [1, 2]
    for d in logs:
        assert {"Train/Total", "Train/Reconst", "Train/Regular", "Train/Velocity", "Train/Beta", "Train/Learning Rate", "Val/Total", "Val/Reconst",
                "Val/Regular", "Val/Velocity"} <= set(d) and all(np.isfinite(v) for v in d.values())
    sd = torch.load(out / "2.pth", map_location="cpu")
    assert len(sd) == 70 and sd["encoder.conv_layers.1.num_batches_tracked"].item() == 2 * 2   # 2 batches per epoch
    # the evaluation driver on the trained VAE
    audio, gen = tmp_path / "audio", tmp_path / "gen"
    for pid in tv.PERSON_IDS_TEST:
        for sid in (1, 2):
            os.makedirs(audio / pid, exist_ok=True)
            wavfile.write(str(audio / pid / f"sentence{sid:02}.wav"), 16000, np.zeros(16000, np.int16))
    _write_tree(str(coeffs), tv.PERSON_IDS_TEST, (1, 2), rng, T=260)
    for pid in tv.PERSON_IDS_TEST:
        _write_tree(str(gen), [pid], (1, 2), rng, T=260)
        for sid in (1, 2):
            os.rename(gen / pid / f"sentence{sid:02}.csv", gen / pid / f"sentence{sid:02}-0.csv")
    cmd = [sys.executable, os.path.join(ROOT, "script", "test_evaluate.py"), "--audio_dir", str(audio), "--coeffs_dir", str(gen),
           "--coeffs_real_dir", str(coeffs), "--vae_weights_path", str(out / "2.pth"), "--wind_num_clusters", "2", "--wind_num_repeats", "2",
           "--window_step_size", "4", "--seed", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "EvalMetrics(frechet_distance=" in r.stdout
