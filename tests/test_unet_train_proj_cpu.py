"""CPU checks of the denoiser trainer with feature_dim > 0 (the trainable audio_proj_layer): the host-side tables, the initial state, the
library's device-free table queries and the projecting restatement (tests/unet_train_proj_ref.py) against golden G17."""
import os

import numpy as np
import torch

from said_amd import _engine
from said_amd.model.diffusion import SAID_UNet1D
from said_amd.model.wav2vec2 import AudioConfig
from said_amd.training import trainable_shapes, unet_init_state_dict
from said_amd.util.synth import fill_tensor, said_state_dict
import unet_train_proj_ref as pref
import unet_train_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G17 = np.load(os.path.join(ROOT, "tests", "golden", "g17_unet_train_proj.npz"))
FD = 40


def test_shapes_and_order_are_the_models():
    model = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=1), feature_dim=FD)
    want = [(k, tuple(v.shape)) for k, v in model.state_dict().items() if not k.startswith("audio_encoder.")]
    assert list(trainable_shapes(FD).items()) == want and len(want) == 163
    s = trainable_shapes(FD)
    assert s["null_cond_emb"] == (1, 1, FD) and s["audio_proj_layer.weight"] == (FD, 768) and s["audio_proj_layer.bias"] == (FD,)
    assert list(s)[:4] == ["null_cond_emb", "audio_proj_layer.weight", "audio_proj_layer.bias", "denoiser.model.time_embed.0.weight"]
    assert all(s[k] == (192, FD) for k in s if ".attn2.to_k." in k or ".attn2.to_v." in k)
    assert sum(".attn2.to_k." in k or ".attn2.to_v." in k for k in s) == 8


def test_defaults_are_unchanged():
    assert trainable_shapes() == trainable_shapes(-1) and list(trainable_shapes()) == list(trainable_shapes(-1))
    assert len(trainable_shapes()) == _engine.UT_NUM_TENSORS == 161 and "audio_proj_layer.weight" not in trainable_shapes()
    torch.manual_seed(5)
    a = unet_init_state_dict()
    after_a = torch.rand(1)
    torch.manual_seed(5)
    b = unet_init_state_dict(-1)
    after_b = torch.rand(1)
    assert list(a) == list(b) == list(trainable_shapes()) and all(torch.equal(a[k], b[k]) for k in a) and torch.equal(after_a, after_b)
    torch.manual_seed(5)
    assert torch.equal(a["null_cond_emb"], torch.randn(1, 1, 768))   # the first draw, as before


def test_init_state_dict_reproduces_the_reference_constructor():
    """G17 part B: nn.Linear(768, 40), randn(1, 1, 40) and the reference's UNet1DConditionModel(32, 32, 40) after torch.manual_seed(17)."""
    torch.manual_seed(17)
    sd = unet_init_state_dict(FD)
    names = [str(n) for n in G17["init_names"]]
    assert list(sd) == names == list(trainable_shapes(FD))
    for n, s, f4 in zip(names, G17["init_sum"], G17["init_first4"]):
        v = sd[n]
        assert tuple(v.shape) == trainable_shapes(FD)[n], n
        assert np.array_equal(v.reshape(-1)[:4].numpy(), f4), n
        assert abs(float(v.double().sum()) - float(s)) <= 1e-12 * max(abs(float(s)), float(v.double().abs().sum())), n


def test_library_tables():
    """The per-feature_dim table queries need no device; a context's own queries answer from the same table."""
    lib = _engine.load_library("unet_train")
    static = [lib.said_unet_train_tensor_name(i).decode() for i in range(_engine.UT_NUM_TENSORS)]
    assert static == list(trainable_shapes()) and lib.said_unet_train_tensor_name(_engine.UT_NUM_TENSORS) is None
    for fd in (-1, 0, FD, 256, 1024):
        shapes = trainable_shapes(fd)
        n = lib.said_unet_train_table_size(fd)
        assert n == len(shapes) == (163 if fd > 0 else 161)
        assert [lib.said_unet_train_table_name(fd, i).decode() for i in range(n)] == list(shapes)
        assert [lib.said_unet_train_table_numel(fd, i) for i in range(n)] == [int(np.prod(s)) for s in shapes.values()]
        assert lib.said_unet_train_table_name(fd, n) is None and lib.said_unet_train_table_numel(fd, -1) == -1
    # asking for another table leaves the static one as it was
    assert [lib.said_unet_train_tensor_name(i).decode() for i in range(_engine.UT_NUM_TENSORS)] == static
    assert [lib.said_unet_train_tensor_numel(i) for i in range(161)] == [int(np.prod(s)) for s in trainable_shapes().values()]
    assert lib.said_unet_train_table_size(1025) == -1 and lib.said_unet_train_table_name(1025, 0) is None


def test_parser_takes_the_feature_dim():
    import importlib.util
    spec = importlib.util.spec_from_file_location("said_script_train", os.path.join(ROOT, "script", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    assert train.build_parser().parse_args(["--unet_feature_dim", "64"]).unet_feature_dim == 64
    assert train.build_parser().parse_args([]).unet_feature_dim == -1


def proj_state(dtype=torch.float32, fd=FD):
    sd = said_state_dict(num_w2v_layers=1, ctx_dim=fd)
    sd["audio_proj_layer.weight"] = fill_tensor("audio_proj_layer.weight", (fd, 768))
    sd["audio_proj_layer.bias"] = fill_tensor("audio_proj_layer.bias", (fd,))
    return {k: sd[k].to(dtype) for k in trainable_shapes(fd)}


def test_projecting_restatement_matches_golden_g17():
    """The restatement with the projection applied in front (fp32) against the capture from the reference's own module: G16's rule, 1e-4 of
    each gradient's norm, all 163 tensors."""
    x, answer, audio = (torch.from_numpy(G17[k]) for k in ("x", "answer", "audio"))
    with torch.enable_grad():
        p = {k: v.clone().requires_grad_(True) for k, v in proj_state().items()}
        out = pref.forward(p, x, torch.from_numpy(G17["timesteps"]), audio, torch.from_numpy(G17["cond"]))
        lp, lv, _ = ref.objective(out, answer)
        (lp + lv).backward()
    want = torch.from_numpy(G17["out"])
    assert (out.detach() - want).abs().max() <= 2e-5 * want.abs().max()
    assert abs(float((lp + lv).detach()) - float(G17["loss"])) <= 1e-5 * float(G17["loss"])
    assert [str(n) for n in G17["names"]] == list(trainable_shapes(FD))
    assert "g:audio_proj_layer.bias" in G17.files
    for n, gs, gn in zip(G17["names"], G17["grad_sum"], G17["grad_norm"]):
        g = p[str(n)].grad.double()
        assert gn > 0, n
        assert abs(float(g.norm()) - gn) <= 1e-4 * gn, (n, float(g.norm()), gn)
        assert abs(float(g.sum()) - gs) <= 1e-4 * gn * g.numel() ** 0.5, (n, float(g.sum()), gs)
        if "g:" + str(n) in G17.files:
            assert (g.reshape(-1) - torch.from_numpy(G17["g:" + str(n)]).double()).norm() <= 1e-4 * gn, n


def test_helper_leaves_the_restatement_as_it_was():
    """loss_and_grads of the helper swaps unet_train_ref.forward only while it runs, and is the plain one for a dict without a projection."""
    before = ref.forward
    sd = {k: v for k, v in said_state_dict(num_w2v_layers=1).items() if k in trainable_shapes()}
    g = torch.Generator().manual_seed(2)
    args = (torch.linspace(0.99, 0.01, 1000), torch.rand(1, 8, 32, generator=g), torch.randn(1, 8, 32, generator=g), torch.tensor([40]),
            torch.randn(1, 8, 768, generator=g), [True])
    (la, ga), (lb, gb) = pref.loss_and_grads(sd, *args), ref.loss_and_grads(sd, *args)
    assert ref.forward is before
    assert torch.equal(la[0], lb[0]) and all(torch.equal(ga[k], gb[k]) for k in ga)
