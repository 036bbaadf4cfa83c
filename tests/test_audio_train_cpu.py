"""The host side of the audio encoder's train mode (said_amd.model.wav2vec2, include/said_audio_train.h) and its float64 restatement
(tests/audio_train_ref.py), without a GPU.

tests/golden/spec_masks.npz holds the masks of transformers 5.15.0's ``_compute_mask_indices(shape, 0.05, 10, min_masks=2)`` after
``np.random.seed(1000 + i)`` for shape i of SHAPES (keys ``mask_<i>``), recorded once, so the comparison also runs where transformers is
not installed.
"""
import os

import numpy as np
import pytest
import torch

import audio_train_ref as ref
from oracle import wav2vec2 as ow
from philox_ref import philox4x32_10
from said_amd.model.wav2vec2 import AudioTrainConfig, compute_mask_indices, draw_audio_train
from said_amd.util import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 20), (3, 40), (8, 120), (2, 241), (1, 10)]
SEED = 0x0123456789ABCDEF


def w2v_sd(layers):
    return {k[len("audio_encoder."):]: v for k, v in synth.said_state_dict(num_w2v_layers=layers).items() if k.startswith("audio_encoder.")}


# ------------------------------------------------------------------------------------------------ the span mask
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_compute_mask_indices_equals_recorded_masks(i):
    g = np.load(os.path.join(ROOT, "tests", "golden", "spec_masks.npz"))
    np.random.seed(1000 + i)
    got = compute_mask_indices(SHAPES[i], 0.05, 10, 2)
    assert got.dtype == np.bool_ and np.array_equal(got, g[f"mask_{i}"])


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_compute_mask_indices_equals_transformers(i):
    m = pytest.importorskip("transformers.models.wav2vec2.modeling_wav2vec2")
    for seed in (1000 + i, 7, 8):
        np.random.seed(seed)
        want = m._compute_mask_indices(SHAPES[i], 0.05, 10, min_masks=2)
        after_want = np.random.rand()
        np.random.seed(seed)
        got = compute_mask_indices(SHAPES[i], 0.05, 10, 2)
        assert np.array_equal(got, want) and np.random.rand() == after_want, "same mask, same generator state afterwards"


def test_span_counts_at_the_training_window_sizes():
    """Two spans of ten frames at 40, 120 and 240 frames (overlaps are possible, so at most 20 frames and at least 11); at 20 frames
    likewise; at 10 frames the one possible span."""
    for frames in (20, 40, 120, 240):
        np.random.seed(frames)
        n = compute_mask_indices((64, frames), 0.05, 10, 2).sum(1)
        assert n.max() <= 20 and n.min() >= 11, (frames, n.min(), n.max())
        if frames >= 120:
            assert (n == 20).any()
    np.random.seed(0)
    assert compute_mask_indices((2, 10), 0.05, 10, 2).all()


def test_draw_order_and_layerdrop_rule():
    """np.random: the mask's draws, then one uniform per layer; torch: one randint for the seed.  skip iff draw < layerdrop."""
    cfg = AudioTrainConfig()
    np.random.seed(3)
    torch.manual_seed(3)
    d = draw_audio_train(cfg, 4, 120, 12)
    np.random.seed(3)
    torch.manual_seed(3)
    mask = compute_mask_indices((4, 120), 0.05, 10, 2)
    u = [np.random.uniform(0, 1) for _ in range(12)]
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    assert np.array_equal(d.mask, mask) and d.skip == tuple(x < 0.1 for x in u) and d.seed == seed
    draws = iter([0.05, 0.1, 0.5])
    d = draw_audio_train(cfg, 1, 40, 3, layerdrop_draw=lambda: next(draws))
    assert d.skip == (True, False, False)
    with pytest.raises(NotImplementedError, match="mask_feature_prob"):
        draw_audio_train(AudioTrainConfig(mask_feature_prob=0.1), 1, 40, 3)
    with pytest.raises(ValueError, match=r"outside \[0, 1\)"):
        draw_audio_train(AudioTrainConfig(hidden_dropout=1.0), 1, 40, 3)
    assert draw_audio_train(AudioTrainConfig(mask_time_prob=0.0), 1, 40, 3).mask is None


# ------------------------------------------------------------------------------------------------ the keep rule
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rule_matches_philox_word_for_word(p):
    n = 1 << 20
    f = ref.elementwise_factors(SEED, 19, (4, 64, n // 256), p).reshape(-1)
    e = np.arange(n, dtype=np.uint32)
    z = np.zeros_like(e)
    words = np.stack(philox4x32_10(z + np.uint32(19), e >> np.uint32(2), z, z, np.uint32(SEED & 0xFFFFFFFF), np.uint32(SEED >> 32)), axis=1)
    w = words[np.arange(n), e & 3]
    kept = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 >= float(np.float32(p))
    assert np.array_equal(f > 0, kept)
    assert set(np.unique(f)) == {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(p))}
    sigma = np.sqrt(p * (1 - p) / n)
    assert abs(kept.mean() - (1 - p)) <= 4 * sigma, (kept.mean(), sigma)
    # probabilities: query i, key j of (b, head) <- word j & 3 of counter (site, (b 12 + head) T + i, j >> 2, 0)
    B, T = 2, 37
    fa = ref.attention_factors(SEED, 16, B, 12, T, p)
    for b, h, i, j in ((0, 0, 0, 0), (1, 11, 36, 36), (1, 3, 5, 18), (0, 7, 30, 3)):
        wd = philox4x32_10(np.uint32(16), np.uint32((b * 12 + h) * T + i), np.uint32(j >> 2), np.uint32(0), np.uint32(SEED & 0xFFFFFFFF), np.uint32(SEED >> 32))[j & 3]
        assert (fa[b, h, i, j] > 0) == ((int(wd) >> 8) * 2.0 ** -24 >= float(np.float32(p)))


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_without_draws_is_the_oracle():
    sd = w2v_sd(2)
    wave = torch.stack([synth.synth_waveform(i, 8000) for i in range(2)])
    for frames in (30, None):
        want = ow.wav2vec2_forward(sd, wave, frames)[0]
        got = ref.forward(sd, wave, frames, dtype=torch.float32)
        assert torch.equal(got, want)


def _hf_model(sd, layerdrop):
    tr = pytest.importorskip("transformers")
    cfg = tr.Wav2Vec2Config(num_hidden_layers=2, hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                            final_dropout=0.0, layerdrop=layerdrop, mask_time_prob=0.05, mask_feature_prob=0.0, attn_implementation="eager")
    model = tr.Wav2Vec2Model(cfg).double()
    own = model.state_dict()
    ren = {"encoder.pos_conv_embed.conv.weight_g": "encoder.pos_conv_embed.conv.parametrizations.weight.original0",
           "encoder.pos_conv_embed.conv.weight_v": "encoder.pos_conv_embed.conv.parametrizations.weight.original1"}
    given = {(ren[k] if ren.get(k) in own else k): v.double() for k, v in sd.items()}
    model.load_state_dict(given, strict=True)
    return model.train()


def test_masking_and_layerdrop_against_transformers_in_train_mode():
    """Wav2Vec2Model.train() with every dropout 0 on float64 weights: an explicit mask_time_indices is the restatement's masking, and
    layerdrop = 1 is "every layer skipped".  Both sides are float64 evaluations of the same operations: 1e-10 of the output's scale
    (values up to ~4) leaves four orders of magnitude over float64's rounding through two layers."""
    sd = w2v_sd(2)
    wave = torch.stack([synth.synth_waveform(i, 8000) for i in range(2)]).double()
    frames = 24   # 8000 samples through the feature extractor
    np.random.seed(5)
    mask = compute_mask_indices((2, frames), 0.05, 10, 2)
    with torch.no_grad():
        want = _hf_model(sd, 0.0)(wave, mask_time_indices=torch.from_numpy(mask)).last_hidden_state
        got = ref.forward(sd, wave, None, mask=mask)
        assert got.shape == want.shape == (2, frames, 768)
        assert float((got - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max()))
        assert float((got - ref.forward(sd, wave, None)).abs().max()) > 1e-3, "the mask must matter"
        want = _hf_model(sd, 1.0)(wave, mask_time_indices=torch.zeros(2, frames, dtype=torch.bool)).last_hidden_state   # (explicit: nothing is drawn)
        got = ref.forward(sd, wave, None, skip=(0, 1))
        assert float((got - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max()))
        assert torch.equal(got, ref.forward(sd, wave, None, skip=(True, True)))
