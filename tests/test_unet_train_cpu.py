"""CPU checks of the denoiser trainer's host side and of its float64-capable restatement (tests/unet_train_ref.py)."""
import os

import numpy as np
import pytest
import torch

from said_amd import _engine
from said_amd.training import normalize_deltas
from said_amd.training.unet import trainable_shapes
from said_amd.util.synth import said_state_dict
import unet_train_ref as ref
from oracle import unet as oracle_unet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tensor_table_is_the_trainable_state_dict():
    lib = _engine.load_library("unet_train")
    shapes = trainable_shapes()
    names = [lib.said_unet_train_tensor_name(i).decode() for i in range(_engine.UT_NUM_TENSORS)]
    assert names == list(shapes) and lib.said_unet_train_tensor_name(_engine.UT_NUM_TENSORS) is None
    assert [lib.said_unet_train_tensor_numel(i) for i in range(len(names))] == [int(np.prod(s)) for s in shapes.values()]
    assert set(names) == {k for k in said_state_dict(num_w2v_layers=1) if not k.startswith("audio_encoder.")}


def test_restatement_eval_forward_equals_oracle():
    sd = said_state_dict(num_w2v_layers=1)
    g = torch.Generator().manual_seed(3)
    x, ts, au = torch.randn(2, 37, 32, generator=g), torch.tensor([3, 700]), torch.randn(2, 37, 768, generator=g)
    with torch.no_grad():
        a = ref.forward({k: sd[k] for k in trainable_shapes()}, x, ts, au, [True, True])
        b = oracle_unet.unet1d_forward({k[len("denoiser."):]: v for k, v in sd.items() if k.startswith("denoiser.")}, x, ts, au)
    assert (a - b).abs().max() <= 1e-5 * b.abs().max()


@pytest.mark.parametrize("prediction_type", ["epsilon", "sample", "v_prediction"])
@pytest.mark.parametrize("use_std", [False, True])
@pytest.mark.parametrize("V", [0, 7])
def test_objective_follows_the_reference_formulas(prediction_type, use_std, V):
    """The restated objective against the reference's own statements (script/train.py:112-149) written out with in-place division."""
    g = torch.Generator().manual_seed(11)
    B, T = 2, 9
    pred = torch.randn(B, T, 32, generator=g, dtype=torch.float64)
    x0, noise = torch.rand(B, T, 32, generator=g, dtype=torch.float64), torch.randn(B, T, 32, generator=g, dtype=torch.float64)
    ac = torch.linspace(0.99, 0.01, 1000)
    ts = torch.tensor([5, 800])
    std = (0.5 + torch.rand(32, generator=g)).double() if use_std else None
    deltas = normalize_deltas(torch.randn(B, 32, V, 3, generator=g)).double() if V else None
    _, answer = ref.add_noise(ac, x0, noise, ts, prediction_type, torch.float64)
    lp, lv, lx = ref.objective(pred, answer, std, deltas)
    a, p = answer.clone(), pred.clone()
    if std is not None:
        a /= std.view(1, 1, -1)
        p /= std.view(1, 1, -1)
    assert torch.allclose(lp, (p - a).abs().mean(), rtol=1e-12)
    assert torch.allclose(lv, ((p[:, 1:] - p[:, :-1]) - (a[:, 1:] - a[:, :-1])).abs().mean(), rtol=1e-12)
    if V:
        assert torch.allclose(lx, (torch.bmm(p, deltas) - torch.bmm(a, deltas)).abs().mean(), rtol=1e-12)
        assert abs(float(deltas[0].abs().mean()) - 1.0) < 1e-5
    else:
        assert lx is None
    sa = (ac[ts] ** 0.5).double().view(-1, 1, 1)
    sb = ((1 - ac[ts]) ** 0.5).double().view(-1, 1, 1)
    want = {"epsilon": noise, "sample": x0, "v_prediction": sa * noise - sb * x0}[prediction_type]
    assert torch.equal(answer, want)


def test_dropout_masks_are_the_philox_stream():
    m = ref.dropout_masks(0x0123456789ABCDEF, 2, 5, 0.1)
    assert len(m) == 5 and m[0].shape == (2, 5, 192)
    vals = torch.unique(torch.stack(m))
    assert vals.tolist() == [0.0, float(np.float32(1) / (np.float32(1) - np.float32(0.1)))]
    keep = float((torch.stack(m) > 0).double().mean())
    assert abs(keep - 0.9) < 0.02
    assert not torch.equal(m[0], m[1])
    assert ref.dropout_masks(1, 2, 5, 0.0) is None


# ---------------------------------------------------------------------------------------------------------------- golden G16
G16 = np.load(os.path.join(ROOT, "tests", "golden", "g16_unet_train.npz"))


def test_restatement_matches_golden_g16():
    """Output and every gradient of the restatement (fp32, train mode without dropout, cond select with a null_cond_emb leaf) against the
    capture from the reference's own UNet1DConditionModel.  Both sides are fp32 with different operation orders: 1e-4 of each tensor's
    gradient norm (measured: below 2e-5), full comparison for the small tensors."""
    sd = {k: v for k, v in said_state_dict(num_w2v_layers=1).items() if k in trainable_shapes()}
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    x, answer, audio = (torch.from_numpy(G16[k]) for k in ("x", "answer", "audio"))
    with torch.enable_grad():
        out = ref.forward(p, x, torch.from_numpy(G16["timesteps"]), audio, torch.from_numpy(G16["cond"]))
        lp, lv, _ = ref.objective(out, answer)
        (lp + lv).backward()
    want = torch.from_numpy(G16["out"])
    assert (out.detach() - want).abs().max() <= 2e-5 * want.abs().max()
    assert abs(float((lp + lv).detach()) - float(G16["loss"])) <= 1e-5 * float(G16["loss"])
    worst = 0.0
    for n, gs, gn in zip(G16["names"], G16["grad_sum"], G16["grad_norm"]):
        g = p[str(n)].grad.double()
        assert gn > 0, n
        worst = max(worst, abs(float(g.norm()) - gn) / gn)
        assert abs(float(g.norm()) - gn) <= 1e-4 * gn, (n, float(g.norm()), gn)
        assert abs(float(g.sum()) - gs) <= 1e-4 * gn * g.numel() ** 0.5, (n, float(g.sum()), gs)
        if "g:" + str(n) in G16.files:
            full = torch.from_numpy(G16["g:" + str(n)]).double()
            assert (g.reshape(-1) - full).norm() <= 1e-4 * gn, n
    print("G16 worst relative norm deviation", worst)


def test_init_state_dict_has_the_reference_keys_and_shapes():
    from said_amd.training import unet_init_state_dict
    torch.manual_seed(7)
    sd = unet_init_state_dict()
    assert list(sd)[1:] == [str(k) for k in G16["state_names"]] and list(sd)[0] == "null_cond_emb"
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(trainable_shapes())
    torch.manual_seed(7)
    assert torch.equal(sd["null_cond_emb"], torch.randn(1, 1, 768))
    for k, v in sd.items():
        zero = any(z in k for z in (".out_layers.3.", ".proj_out.", "model.out.2."))
        assert (float(v.abs().max()) == 0.0) == (zero or (k.endswith(".bias") and ("norm" in k or ".in_layers.0." in k or ".out_layers.0." in k or "model.out.0." in k))), k


# ---------------------------------------------------------------------------------------------------------------- windows
def _pad_cut(seq, start, length, before, after):
    s = seq if seq.dim() == 2 else seq[:, None]
    out = torch.nn.functional.pad(s.t().unsqueeze(0), (before, after), "replicate").squeeze(0).t()[start:start + length]
    return out if seq.dim() == 2 else out[:, 0]


@pytest.mark.parametrize("n,start,length,before,after", [(50, 0, 40, 20, 40), (50, 5, 40, 20, 40), (50, 69, 40, 20, 40), (30, 3, 40, 20, 40),
                                                         (7, 0, 12, 7, 13), (7, 25, 12, 7, 13)])
def test_cut_window_is_replicate_padding(n, start, length, before, after):
    from said_amd.training.unet import cut_window
    seq = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)
    assert torch.equal(cut_window(seq, start, length, before, after), _pad_cut(seq, start, length, before, after))
    assert torch.equal(cut_window(seq[:, 0], start, length, before, after), _pad_cut(seq[:, 0], start, length, before, after))


def _toy_items():
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(16000 * n // 60 + 13, generator=g), torch.rand(n, 32, generator=g)) for n in (90, 64, 47)]


def test_collate_matches_direct_padding_and_pins_the_draw_order():
    """A batch under random.seed(3): the same draws made here in the reference's order (per item: cond, hflip, zero-out; then the window
    size; then per item bdx, delay coin, delay) reproduce the windows through a direct F.pad restatement.  The sequence of 47 frames is
    shorter than the windows' padding reach, bdx goes negative, and the delay offset reaches both ends."""
    import random
    from said_amd.training import TrainWindowDataset
    for seed in (3, 4, 11):
        ds = TrainWindowDataset(items=_toy_items(), window_size_min=40, sampling_rate=16000)
        random.seed(seed)
        batch = ds.collate_fn([ds[i] for i in (0, 1, 2)])
        ds2 = TrainWindowDataset(items=_toy_items(), window_size_min=40, sampling_rate=16000)
        stored = [(w.clone(), c.clone()) for w, c, _ in ds2.data]
        random.seed(seed)
        conds = []
        for i in range(3):
            conds.append(random.uniform(0, 1) > 0.1)
            if random.uniform(0, 1) < 0.5:
                c = stored[i][1]
                c[:, ds2.mirror_indices] = c[:, ds2.mirror_indices_flip]
            assert not random.uniform(0, 1) < 0
        window = random.randrange(40, 47 + 1)
        wl, half = 16000 * window // 60, window // 2
        assert batch.blendshape_coeffs.shape == (3, window, 32) and batch.cond.tolist() == conds
        for i in range(3):
            n = stored[i][1].shape[0]
            bdx = random.randint(-half, max(0, n - half - 1))
            wdx = 16000 * bdx // 60
            if random.uniform(0, 1) < 0.5:
                wdx = random.randint(wdx - 1, wdx + 1)
            assert torch.equal(batch.blendshape_coeffs[i], _pad_cut(stored[i][1], bdx + half, window, half, window))
            want = _pad_cut(stored[i][0], max(0, wdx + wl // 2 + 1), wl, wl // 2 + 1, wl + 1)
            assert np.array_equal(batch.waveform[i], want.numpy()) and len(batch.waveform[i]) == wl


def test_draw_order_is_pinned():
    """random.seed(0), items 2 and 0: the window size, the cond flags, the first cut frames and the generator's next value are pinned, so a
    draw added, dropped or reordered shows."""
    import random
    from said_amd.training import TrainWindowDataset
    ds = TrainWindowDataset(items=_toy_items(), window_size_min=40, sampling_rate=16000)
    random.seed(0)
    b = ds.collate_fn([ds[i] for i in (2, 0)])
    assert tuple(b.blendshape_coeffs.shape) == (2, 44, 32) and b.cond.tolist() == [True, True] and len(b.waveform[0]) == 11733
    assert random.random() == 0.7558042041572239
    assert float(b.blendshape_coeffs[0, 0, 0]) == 0.4868316054344177 and float(b.blendshape_coeffs[1, 0, 0]) == 0.4884745478630066


def test_val_dataset_pads_the_waveform():
    import random
    from said_amd.training import ValWindowDataset
    ds = ValWindowDataset(items=[(torch.ones(100), torch.rand(30, 32)), (torch.ones(20000), torch.rand(30, 32))], sampling_rate=16000)
    random.seed(1)
    a, b = ds[0], ds[1]
    assert a.waveform.shape == (8000,) and float(a.waveform.sum()) == 100.0 and b.waveform.shape == (8000,) and float(b.waveform.sum()) == 8000.0
    batch = ValWindowDataset.collate_fn([a])
    assert batch.blendshape_coeffs.shape == (1, 30, 32) and batch.cond.dtype == torch.bool
