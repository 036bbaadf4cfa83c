"""Fine-tuning the Wav2Vec2 transformer with the denoiser, the parts that need no GPU: the restatement (tests/audio_ft_ref.py) against golden
G18, captured from the reference's own ModifiedWav2Vec2Model (tests/golden/make_golden_g18.py); the table of trainable tensors; the binding of
the new entry points against their headers; the command line's flag."""
import os
import sys

import numpy as np
import pytest
import torch

from said_amd.training import trainable_shapes
from said_amd.util.synth import said_state_dict, w2v_param_shapes
import audio_ft_ref as aft
import audio_train_ref as atr
import unet_train_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G18 = np.load(os.path.join(ROOT, "tests", "golden", "g18_audio_finetune.npz"))


def encoder_tensors(L, dtype=torch.float32):
    return {k: v.to(dtype) for k, v in said_state_dict(num_w2v_layers=L).items() if k.startswith("audio_encoder.")}


def test_restatement_matches_golden_g18():
    """last_hidden_state and every trainable tensor's gradient of the restatement (fp32, eval mode, on the golden's conv features) against the
    capture from the reference's own module: g16's rule, 1e-4 of each tensor's gradient norm, full comparison for the small tensors."""
    sd = encoder_tensors(2)
    names = [str(n) for n in G18["names"]]
    assert names == [k for k in sd if not k.startswith("audio_encoder.feature_extractor.")] and len(names) == 42
    # the frozen front end: the features the golden's module fed its feature projection
    wave = torch.from_numpy(G18["waveform"])
    feats = atr.features({k[len("audio_encoder."):]: v for k, v in sd.items()}, wave, int(G18["num_frames"]), torch.float32)
    want = torch.from_numpy(G18["features"])
    assert feats.shape == want.shape == (2, 19, 512) and (feats - want).abs().max() <= 2e-5 * want.abs().max()
    p = {k: sd[k].clone().requires_grad_(True) for k in names}
    p["null_cond_emb"] = torch.zeros(1, 1, 768)   # (the restatement reads the working dtype off it)
    target = torch.from_numpy(G18["target"])
    with torch.enable_grad():
        out = aft.conditioning(p, want)
        lp, lv, _ = ref.objective(out, target)
        (lp + lv).backward()
    ref_out = torch.from_numpy(G18["out"])
    assert (out.detach() - ref_out).abs().max() <= 2e-5 * ref_out.abs().max()
    assert abs(float((lp + lv).detach()) - float(G18["loss"])) <= 1e-5 * float(G18["loss"])
    worst = 0.0
    for n, gs, gn in zip(names, G18["grad_sum"], G18["grad_norm"]):
        if n == "audio_encoder.masked_spec_embed":   # no mask in eval mode: the reference leaves its gradient unset
            assert gn == 0 and p[n].grad is None
            continue
        g = p[n].grad.double()
        assert gn > 0, n
        if n.endswith("attention.k_proj.bias"):
            # a key bias shifts every score of a query alike, which softmax ignores: the exact gradient is 0 and both sides hold rounding
            # noise only.  The rule's scale is then the sibling q_proj.bias gradient's norm: both must vanish against it.
            scale = float(G18["grad_norm"][names.index(n.replace("k_proj", "q_proj"))])
            assert gn <= 1e-4 * scale and float(g.norm()) <= 1e-4 * scale, (n, float(g.norm()), gn, scale)
            continue
        worst = max(worst, abs(float(g.norm()) - gn) / gn)
        assert abs(float(g.norm()) - gn) <= 1e-4 * gn, (n, float(g.norm()), gn)
        assert abs(float(g.sum()) - gs) <= 1e-4 * gn * g.numel() ** 0.5, (n, float(g.sum()), gs)
        if "g:" + n in G18.files:
            assert (g.reshape(-1) - torch.from_numpy(G18["g:" + n]).double()).norm() <= 1e-4 * gn, n
    print("G18 worst relative norm deviation", worst)


@pytest.mark.parametrize("L", [1, 2, 12])
@pytest.mark.parametrize("F", [-1, 64])
def test_trainable_shapes_append_the_transformer(F, L):
    base, ft = trainable_shapes(F), trainable_shapes(F, L)
    assert list(ft)[:len(base)] == list(base) and all(ft[k] == base[k] for k in base)
    extra = {k: v for k, v in ft.items() if k not in base}
    want = {"audio_encoder." + k: tuple(v) for k, v in w2v_param_shapes(L).items() if not k.startswith("feature_extractor.")}
    assert list(extra.items()) == list(want.items()) and not any("feature_extractor" in k for k in ft)
    sd = said_state_dict(num_w2v_layers=L)
    assert list(extra) == [k for k in sd if k.startswith("audio_encoder.") and "feature_extractor" not in k]
    assert all(tuple(sd[k].shape) == v for k, v in extra.items())
    assert trainable_shapes(F, 0) == base and trainable_shapes(F, -3) == base


def test_restatement_routes_the_gradient():
    """The properties the GPU tests ask of the HIP step hold for the restatement: an unconditional batch sends nothing into the encoder, a
    skipped layer and an unused masked_spec_embed get no gradient."""
    L, B, T = 2, 2, 6
    sd = {k: v.double() for k, v in said_state_dict(num_w2v_layers=L).items() if k in trainable_shapes(-1, L)}
    g = torch.Generator().manual_seed(5)
    feats, coeffs, noise = torch.randn(B, T, 512, generator=g), torch.rand(B, T, 32, generator=g), torch.randn(B, T, 32, generator=g)
    ac = torch.linspace(0.99, 0.01, 1000)
    ts = torch.tensor([10, 600])
    _, grads = aft.loss_and_grads(sd, ac, coeffs, noise, ts, feats, [False, False])
    assert all(float(v.abs().max()) == 0 for k, v in grads.items() if k.startswith("audio_encoder.")) and float(grads["null_cond_emb"].abs().max()) > 0
    enc = dict(skip=[False, True], seed=3, mask=np.array([[0, 1, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0]], dtype=bool), **aft.PUBLISHED)
    _, grads = aft.loss_and_grads(sd, ac, coeffs, noise, ts, feats, [True, False], enc=enc)
    for k, v in grads.items():
        if k.startswith("audio_encoder."):
            assert (float(v.abs().max()) == 0) == (".layers.1." in k), k
    _, grads = aft.loss_and_grads(sd, ac, coeffs, noise, ts, feats, [True, False], enc=dict(enc, mask=None))
    assert float(grads["audio_encoder.masked_spec_embed"].abs().max()) == 0


@pytest.mark.parametrize("group", ["unet_finetune", "audio_features"])
def test_added_groups_match_their_headers(group):
    """tests/test_host_cpu.py's check of a binding group against its headers, for the groups of _engine.added_groups(): the names, the library's
    exports, every parameter and return value bound in kind and size; no name is bound twice."""
    import test_host_cpu as th
    from said_amd import _engine
    lib, g = _engine.load_library(group), _engine.added_groups()[group]
    declared = {name: sig for h in g.headers for name, sig in th._declarations(th._header(h)).items()}
    assert set(declared) == set(g.table) and len(declared) == {"unet_finetune": 9, "audio_features": 1}[group]
    assert not [name for o in _engine.ABI.values() for name in o.table if name in declared], "bound by two groups"
    assert [name for name in declared if not hasattr(lib, name)] == [], "declared but not exported"
    assert th._mismatches(declared, g.table) == []
    assert all(getattr(lib, name).argtypes == sig[1] for name, sig in g.table.items())
    assert not set(_engine.ABI) & set(_engine.added_groups())
    enums = th._enums(th._header("said_amd/csrc/said_unet_finetune.h"))
    assert enums["SAID_UT_FEATURE_WIDTH"] == 512 and enums["SAID_UT_MAX_FINETUNE_LAYERS"] == 32


def test_table_of_the_library_without_a_device():
    """said_unet_train_table_*_ft need no context: names and sizes are trainable_shapes', finetune_layers <= 0 is the existing table."""
    from said_amd import _engine
    lib = _engine.load_library("unet_finetune")
    _engine.load_library("unet_train")
    for F, L in ((-1, 1), (64, 2), (-1, 12)):
        want = [(k, int(np.prod(s))) for k, s in trainable_shapes(F, L).items()]
        n = lib.said_unet_train_table_size_ft(F, L)
        assert [(lib.said_unet_train_table_name_ft(F, L, i).decode(), lib.said_unet_train_table_numel_ft(F, L, i)) for i in range(n)] == want
        assert n == len(trainable_shapes(F)) + len([k for k in w2v_param_shapes(L) if not k.startswith("feature_extractor.")])
        assert lib.said_unet_train_table_name_ft(F, L, n) is None and lib.said_unet_train_table_numel_ft(F, L, -1) == -1
    for F in (-1, 64):
        for L in (0, -1):
            n = lib.said_unet_train_table_size_ft(F, L)
            assert n == lib.said_unet_train_table_size(F)
            assert all(lib.said_unet_train_table_name_ft(F, L, i) == lib.said_unet_train_table_name(F, i) for i in range(n))
    assert lib.said_unet_train_table_size_ft(-1, 33) == -1 and lib.said_unet_train_table_size_ft(1025, 2) == -1


def test_cli_flag_is_off_by_default():
    sys.path.insert(0, os.path.join(ROOT, "script"))
    try:
        import train
    finally:
        sys.path.pop(0)
    ap = train.build_parser()
    assert ap.parse_args([]).finetune_audio_encoder is False and ap.parse_args(["--finetune_audio_encoder"]).finetune_audio_encoder is True
