"""The denoiser's training step on the MI355X at the batch sizes and window lengths training runs (said_amd/csrc/unet_train.hip,
unet_trainer.cpp, audio_ft.hip; UNetTrainer) against float64 autograd of the restatements tests/unet_train_ref.py, unet_train_proj_ref.py and
audio_ft_ref.py.  The neighbouring modules stop at B T = 363; here B T runs from 2 to 2400, so that every K-split count from 1 to 16, the
empty last chunk, the partial-tile buffer filled to its last float and both sides of split_small's M = 256 switch are executed, and steps of
different shapes follow each other in one context.  What each shape reaches is tests/unet_train_shapes.py's table, proved from
said_amd/csrc/ut_gemm_plan.h by tests/test_ut_gemm_plan_cpu.py.

Tolerance rule: tests/test_gpu_audio_finetune.py's check_all / loss_ok, imported.  Per tensor, rel = |a - b|_2 / |b|_2; the HIP result must be
within 4 x max(rel(fp32 CPU restatement, float64 restatement), 1e-6) of the float64 restatement; the same form for the losses.  An exactly
zero float64 gradient must be exactly zero here.  Every bit-equality is torch.equal.  k_proj.bias gradients of the fine-tuned encoder are
rounding noise in every arithmetic (softmax is invariant to them); the bound is vacuous there, as in that module.

Batches: timesteps spread over [0, 999], cond mixed (every third sample unconditional), the zero-initialised convolutions filled by synth.
References are computed once per case in a module fixture.

Measured on one MI355X (the tensor closest to its bound: HIP error, fp32 CPU error in brackets; forward output likewise; `pytest
--durations` time of the test, references included; t_e.0 = time_embed.0.weight, emb = a ResBlock's emb_layers.1.weight):
    1 x 2      middle_block.2 emb 4.35e-6 (2.36e-6)    forward 1.75e-6 (1.26e-6)   0.48 s;  unconditional: attn1.to_q 6.36e-6 (2.34e-6), 16
               gradients exactly zero in float64 and here (identical context rows: to_q / to_k / norm2 of the cross-attentions)   0.10 s
    3 x 43     output_blocks.1.0 emb 2.61e-6 (0.99e-6) forward 1.29e-6 (0.71e-6)   0.22 s
    3 x 86     middle_block.2 emb 2.64e-6 (0.96e-6)    forward 1.30e-6 (0.74e-6)   0.25 s
    3 x 129    t_e.0 2.62e-6 (1.00e-6)                 forward 1.28e-6 (0.73e-6)   0.29 s
    4 x 130    t_e.0 2.97e-6 (0.95e-6)                 forward 1.30e-6 (0.74e-6)   0.39 s
    5 x 131    t_e.0 2.22e-6 (1.01e-6)                 forward 1.19e-6 (0.72e-6)   0.38 s
    6 x 133    t_e.0 2.48e-6 (0.90e-6)                 forward 1.25e-6 (0.73e-6)   0.39 s
    8 x 120    t_e.0 2.44e-6 (0.92e-6)                 forward 1.25e-6 (0.73e-6)   0.41 s;  p = 0.1: 2.48e-6 (0.88e-6) 0.47 s;  std + vertex: 2.28e-6 (0.78e-6) 0.36 s
    7 x 147    t_e.0 2.68e-6 (0.97e-6)                 forward 1.25e-6 (0.72e-6)   0.45 s
    9 x 128    t_e.0 1.95e-6 (0.79e-6)                 forward 1.20e-6 (0.72e-6)   0.49 s
    7 x 183    t_e.0 2.52e-6 (0.91e-6)                 forward 1.29e-6 (0.73e-6)   0.52 s;  p = 0.1: 2.57e-6 (0.87e-6) 0.39 s;  std + vertex: 2.54e-6 (0.86e-6) 0.34 s
    10 x 141   t_e.0 2.04e-6 (0.78e-6)                 forward 1.22e-6 (0.74e-6)   0.63 s
    8 x 197    t_e.0 2.09e-6 (0.73e-6)                 forward 1.24e-6 (0.71e-6)   0.63 s
    13 x 130   t_e.0 2.04e-6 (0.77e-6)                 forward 1.23e-6 (0.72e-6)   0.65 s
    12 x 150   t_e.0 1.95e-6 (0.74e-6)                 forward 1.20e-6 (0.72e-6)   0.62 s
    8 x 240    t_e.0 2.08e-6 (0.71e-6)                 forward 1.25e-6 (0.72e-6)   0.92 s
    9 x 228    t_e.0 2.00e-6 (0.85e-6)                 forward 1.21e-6 (0.71e-6)   0.80 s;  p = 0.1: 2.09e-6 (0.88e-6) 0.88 s;  std + vertex: 1.77e-6 (0.67e-6) 0.91 s
    3 x 683    t_e.0 2.41e-6 (0.85e-6)                 forward 1.28e-6 (0.71e-6)   3.47 s
    4 x 600    t_e.0 2.55e-6 (0.76e-6)                 forward 1.32e-6 (0.72e-6)   3.02 s
    shape order (four shapes, twice each, four fresh contexts): every gradient and loss torch.equal   0.34 s
    eval_loss / forward_only, live and EMA weights: 9 x 228 losses within 3e-8, output 1.36e-6 / 1.35e-6 (0.83e-6 / 0.82e-6)   0.52 s;
               3 x 683 losses within 2e-8, output 1.41e-6 / 1.42e-6 (0.84e-6 / 0.83e-6)   0.88 s
    F = 1024, 9 x 228: t_e.0 1.88e-6 (0.75e-6), 163 tensors; then 3 x 43 torch.equal to a fresh context's   0.94 s
    fine-tune 9 x 228 train mode: output_blocks.0.1 norm2.bias 2.71e-6 (1.40e-6), 187 tensors compared, 16 exactly zero   3.30 s
    fine-tune 9 x 228 eval mode: t_e.0 1.99e-6 (0.76e-6)   4.11 s;  2 x 128: middle_block.0 emb 2.76e-6 (0.99e-6)   0.46 s;
               1 x 257: input_blocks.1.0 emb 3.10e-6 (0.95e-6)   0.50 s;  9 x 228 then 2 x 128: torch.equal to a fresh context's   0.21 s
The whole module: 30 s.  With the first seeds tried, three batches had a residual inside fp32's error of zero and the GPU's sign differed
from the CPU's in one element each: every gradient 5e-4 ... 1e-2 off, reproduced in float64 by flipping that one sign (see MARGIN below).
"""
import numpy as np
import pytest
import torch

from said_amd import _engine
from said_amd.model.wav2vec2 import AudioTrainConfig, AudioTrainDraws
from said_amd.training import UNetTrainer, normalize_deltas, trainable_shapes
import audio_ft_ref as aft
import test_gpu_audio_finetune as ftm
import test_gpu_unet_train_proj as prm
import unet_train_proj_ref as pref
import unet_train_ref as ref
import unet_train_shapes as uts
from test_gpu_audio_finetune import alphas, check, check_all, loss_ok

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, ASEED = 0x1234567887654321, 0x0FEDCBA987654321
P = 0.1
L = uts.FT_LAYERS
PW = "audio_proj_layer.weight"
ENC = "audio_encoder."
SKIP = (False, True)   # skip_layers = 0b10
# L1's gradient is the sign of a residual, and no arithmetic determines a sign closer to zero than its own error.  One flipped sign moves
# every gradient by 2 / sqrt(n) of its norm (n = 32 B T residuals: 1e-2 at 7 x 183), so a batch with a residual inside fp32's error of zero
# has no fp32 answer to compare with.  A case therefore takes the first batch of its seed sequence (salt 0, 1, ...) for which every residual of
# the float64 restatement (predict: R, velocity: R[t] - R[t - 1], vertex: R D) is more than MARGIN x the fp32 restatement's largest error in
# that residual away from zero.  The choice uses the two CPU references alone, never the GPU's result.
MARGIN, SALTS = 4, 24
assert L == ftm.L


def full_sd(fd=-1, layers=0):
    """The state dict of a context: one-layer frozen encoder (the proj module's), or the fine-tuning module's two-layer one."""
    return ftm.full_sd(fd) if layers else prm.full_sd(fd)


def trainable(fd, layers, dtype):
    sd = full_sd(fd, layers)
    return {k: sd[k].to(dtype) for k in trainable_shapes(fd, layers)}


def mixed_cond(B):
    return [i % 3 != 1 for i in range(B)]


def batch(B, T, V=0, width=768, salt=0):
    """`audio`: the encoder's output (B, T, 768), or with width = 512 the conv features of a fine-tuning context."""
    g = torch.Generator().manual_seed(100 * B + T + 100000 * salt)
    d = dict(coeffs=torch.rand(B, T, 32, generator=g), noise=torch.randn(B, T, 32, generator=g),
             timesteps=torch.linspace(0, 999, B).round().long() if B > 1 else torch.tensor([500]), cond=mixed_cond(B),
             audio=torch.randn(B, T, width, generator=g))
    if V:
        d["std"] = 0.5 + torch.rand(32, generator=g)
        d["deltas"] = normalize_deltas(torch.randn(B, 32, V, 3, generator=g))
    return d


def time_mask(B, T):
    """One span of ten frames per sample; the last sample's reaches the last frame."""
    m = np.zeros((B, T), dtype=bool)
    for b in range(B - 1):
        m[b, 7 + 11 * b:17 + 11 * b] = True
    m[B - 1, T - 10:] = True
    return m


def train_enc(B, T):
    """(the restatement's train-mode arguments, the engine's draws) with the published probabilities."""
    m = time_mask(B, T)
    return dict(mask=m, skip=list(SKIP), seed=ASEED, **aft.PUBLISHED), AudioTrainDraws(mask=m, skip=SKIP, seed=ASEED)


def make_trainer(max_batch, max_frames, fd=-1, layers=0):
    return UNetTrainer(full_sd(fd, layers), DEV, max_batch=max_batch, max_frames=max_frames, learning_rate=1e-3, num_warmup_steps=4, dropout=P,
                       feature_dim=fd, finetune_audio_layers=layers)


@pytest.fixture(scope="module")
def trainers():
    """One trainer per (feature_dim, fine-tuned layers), made on first use, sized for the largest batch and the longest window of its cases."""
    size = {(-1, 0): (uts.MAX_BATCH, uts.MAX_FRAMES), (uts.WIDE[2], 0): uts.WIDE[:2],
            (-1, L): (max(uts.FT_FULL[0], *(b for b, _, _ in uts.FT_SMALL)), max(uts.FT_FULL[1], *(t for _, t, _ in uts.FT_SMALL)))}
    made = {}

    def get(fd=-1, layers=0):
        if (fd, layers) not in made:
            made[fd, layers] = make_trainer(*size[fd, layers], fd=fd, layers=layers)
        return made[fd, layers]

    yield get
    for t in made.values():
        t.close()


def residual_margins(d, fd, layers, cond, masks, enc):
    """[(smallest |x| in float64, largest |x fp32 - x float64|)] for the predict, velocity and (with deltas) vertex residuals of batch d."""
    res = []
    for dt in (torch.float64, torch.float32):
        sd = trainable(fd, layers, dt)
        with torch.no_grad():
            noisy, answer = ref.add_noise(alphas(), d["coeffs"], d["noise"], d["timesteps"], "epsilon", dt)
            if layers:
                pred = aft.forward(sd, noisy, d["timesteps"], d["audio"], cond, masks, enc)
            else:
                pred = pref.forward(sd, noisy, d["timesteps"], d["audio"], cond, masks)
            R = pred - answer
            if "std" in d:
                R = pred / d["std"].to(dt).view(1, 1, -1) - answer / d["std"].to(dt).view(1, 1, -1)
            res.append([R, R[:, 1:] - R[:, :-1]] + ([torch.bmm(R, d["deltas"].to(dt))] if "deltas" in d else []))
    return [(float(a.abs().min()), float((b.double() - a).abs().max())) for a, b in zip(*res)]


@pytest.fixture(scope="module")
def refs():
    """(salt of the batch, float64 and float32 autograd of the restatement on it: [(losses, gradients)] x 2) for each case, computed once."""
    cache = {}

    def get(B, T, fd=-1, layers=0, p=0.0, V=0, cond=None, mode="eval"):
        key = (B, T, fd, layers, p, V, None if cond is None else tuple(cond), mode)
        if key not in cache:
            masks = ref.dropout_masks(SEED, B, T, p)
            enc = train_enc(B, T)[0] if mode == "train" else None
            for salt in range(SALTS):
                d = batch(B, T, V, 512 if layers else 768, salt)
                c = d["cond"] if cond is None else cond
                margins = residual_margins(d, fd, layers, c, masks, enc)
                if all(lo > MARGIN * err for lo, err in margins):
                    break
            else:
                raise AssertionError(f"no well-posed batch among {SALTS} for {key}")
            print(f"batch {key}: salt {salt}, (smallest residual, fp32 error) {margins}")
            kw = dict(std=d.get("std"), deltas=d.get("deltas"), masks=masks)
            if layers:
                kw["enc"] = enc
            fn = aft.loss_and_grads if layers else pref.loss_and_grads if fd > 0 else ref.loss_and_grads
            cache[key] = salt, [fn(trainable(fd, layers, dt), alphas(), d["coeffs"], d["noise"], d["timesteps"], d["audio"], c, **kw)
                                for dt in (torch.float64, torch.float32)]
        return cache[key]

    return get


def gpu_grads(tr, B, T, p=0.0, V=0, cond=None, mode="eval", salt=0):
    """One step from the initial parameters: (losses read back, every gradient)."""
    layers = tr.finetune_audio_layers
    d = batch(B, T, V, 512 if layers else 768, salt)
    tr.load_state_dict(full_sd(tr.feature_dim, layers))
    tr.dropout = p
    tr.std = None if "std" not in d else d["std"].numpy()
    kw = {}
    if mode == "train":
        kw = dict(audio_draws=train_enc(B, T)[1], audio_cfg=AudioTrainConfig())
    out = tr.step(d["coeffs"], d["cond"] if cond is None else cond, d["audio"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED,
                  deltas=d.get("deltas"), **kw)
    tr.std = None
    return out, tr.parameters_of(_engine.UT_GRAD)


def grads_case(trainers, refs, what, B, T, fd=-1, layers=0, **kw):
    salt, ((l64, g64), (l32, g32)) = refs(B, T, fd, layers, **kw)
    out, g = gpu_grads(trainers(fd, layers), B, T, salt=salt, **kw)
    print(f"{what}: predict hip {float(out.predict):.9g} f64 {float(l64[0]):.9g} f32 {float(l32[0]):.9g}; velocity hip {float(out.velocity):.9g} "
          f"f64 {float(l64[1]):.9g} f32 {float(l32[1]):.9g}")
    assert loss_ok(out.predict, l32[0], l64[0]) and loss_ok(out.velocity, l32[1], l64[1]), (out, l32, l64)
    if kw.get("V"):
        assert loss_ok(out.vertex, l32[2], l64[2]), (out, l32, l64)
    assert list(g) == list(g64) == list(trainable_shapes(fd, layers))
    bad = check_all(what, g, g32, g64)
    assert not bad, bad[:8]
    return g, g64


def forward_case(tr, what, B, T, fd=-1):
    """forward_only on a noisy sample against the restatement's forward."""
    d = batch(B, T)
    tr.load_state_dict(full_sd(fd))
    x = d["coeffs"] + 0.3 * d["noise"]
    got = tr.forward_only(x, d["timesteps"], d["cond"], d["audio"])
    with torch.no_grad():
        r64, r32 = (pref.forward(trainable(fd, 0, dt), x, d["timesteps"], d["audio"], d["cond"]) for dt in (torch.float64, torch.float32))
    ok, msg = check("output", got, r32, r64, {})
    print(f"{what}: forward", msg)
    assert ok, msg


def same(a, b):
    """Losses and every gradient of two steps, bit for bit."""
    (oa, ga), (ob, gb) = a, b
    assert float(oa.predict) == float(ob.predict) and float(oa.velocity) == float(ob.velocity), (oa, ob)
    assert list(ga) == list(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


# ---------------------------------------------------------------------------------------------------------------- (a) the default context
@pytest.mark.parametrize("B,T", [(s.B, s.T) for s in uts.DEFAULT], ids=[f"{s.B}x{s.T}" for s in uts.DEFAULT])
def test_gradients(trainers, refs, B, T):
    """All 161 gradients, both losses and the forward output at every shape of the table (K-split counts 1 .. 16)."""
    cond = [True] if B == 1 else None
    g, g64 = grads_case(trainers, refs, f"gradients {B} x {T}", B, T, cond=cond)
    assert len(g) == 161
    if B == 1:
        assert float(g["null_cond_emb"].abs().max()) == 0 and float(g64["null_cond_emb"].abs().max()) == 0
    else:
        assert all(float(v.abs().max()) > 0 for v in g.values())
    forward_case(trainers(), f"gradients {B} x {T}", B, T)


def test_gradients_one_unconditional_sample(trainers, refs):
    """1 x 2 again with the sample unconditional: null_cond_emb takes the whole context gradient."""
    g, _ = grads_case(trainers, refs, "gradients 1 x 2, unconditional", 1, 2, cond=[False])
    assert float(g["null_cond_emb"].abs().max()) > 0


@pytest.mark.parametrize("B,T", uts.VARIANTS, ids=[f"{b}x{t}" for b, t in uts.VARIANTS])
def test_gradients_with_dropout(trainers, refs, B, T):
    grads_case(trainers, refs, f"gradients {B} x {T}, p = {P}", B, T, p=P)


@pytest.mark.parametrize("B,T", uts.VARIANTS, ids=[f"{b}x{t}" for b, t in uts.VARIANTS])
def test_gradients_with_std_and_vertex_loss(trainers, refs, B, T):
    grads_case(trainers, refs, f"gradients {B} x {T}, std + vertex loss", B, T, V=7)


# ---------------------------------------------------------------------------------------------------------------- (b) shape order
def test_shape_order_does_not_matter(trainers):
    """9 x 228, 7 x 183, 3 x 43, 1 x 2 in one context sized 13 x 683, each step run twice: the step behind a larger one and its repetition are
    both bit-equal to the same step in a fresh context sized exactly for it that ran nothing else.  A partial tile or an arena region that
    kept a previous step's values would show here."""
    tr = trainers()
    seq = [(gpu_grads(tr, B, T, P), gpu_grads(tr, B, T, P)) for B, T in uts.ORDER]
    for (B, T), (first, again) in zip(uts.ORDER, seq):
        fresh = make_trainer(B, T)
        try:
            alone = gpu_grads(fresh, B, T, P)
        finally:
            fresh.close()
        same(first, alone)
        same(again, alone)


# ---------------------------------------------------------------------------------------------------------------- (c) eval_loss, forward_only
@pytest.mark.parametrize("B,T", [(9, 228), (3, 683)], ids=["9x228", "3x683"])
def test_eval_loss_and_forward_only(trainers, B, T):
    """After two updates: eval_loss and forward_only on the live and on the EMA weights against the restatement on the same weights."""
    tr, d = trainers(), batch(B, T)
    tr.load_state_dict(full_sd())
    tr.dropout = P
    for k in range(2):
        tr.enqueue_step(d["coeffs"], d["cond"], d["audio"], noise=d["noise"], timesteps=d["timesteps"], dropout_seed=SEED + k)
    weights = {False: tr.parameters_of(_engine.UT_STATE), True: tr.parameters_of(_engine.UT_EMA)}
    q = "denoiser.model.middle_block.1.transformer_blocks.0.attn1.to_q.weight"
    assert not torch.equal(weights[True][q], weights[False][q]) and not torch.equal(weights[False][q], full_sd()[q])
    got = {}
    tr.epoch_output(False)
    x = d["coeffs"] + 0.3 * d["noise"]
    for ema in (False, True):
        tr.eval_loss(d["coeffs"], d["cond"], d["audio"], noise=d["noise"], timesteps=d["timesteps"], use_ema=ema)
        got[ema] = tr.epoch_output(True)
        vals, outs = [], []
        for dt in (torch.float64, torch.float32):
            sd = {k: v.to(dt) for k, v in weights[ema].items()}
            with torch.no_grad():
                noisy, answer = ref.add_noise(alphas(), d["coeffs"], d["noise"], d["timesteps"], "epsilon", dt)
                vals.append([float(v) for v in ref.objective(ref.forward(sd, noisy, d["timesteps"], d["audio"], d["cond"]), answer)[:2]])
                outs.append(ref.forward(sd, x, d["timesteps"], d["audio"], d["cond"]))
        for name, g, v64, v32 in zip(("predict", "velocity"), (got[ema].predict, got[ema].velocity), *vals):
            print(f"eval_loss {B} x {T} ema={ema} {name}: hip {g:.9g} f64 {v64:.9g} f32 {v32:.9g}")
            assert loss_ok(g, v32, v64), (ema, name, g, v64, v32)
        out = tr.forward_only(x, d["timesteps"], d["cond"], d["audio"], use_ema=ema)
        ok, msg = check("output", out, outs[1], outs[0], {})
        print(f"forward_only {B} x {T} ema={ema}", msg)
        assert ok, msg
    assert got[True].predict != got[False].predict


# ---------------------------------------------------------------------------------------------------------------- feature_dim = 1024
def test_feature_dim_1024(trainers, refs):
    """9 x 228 at F = 1024: all 163 gradients; the projection's weight gradient (1024 x 768, 16 chunks) writes the partial-tile buffer to its
    last element.  Then 3 x 43 in the same context, bit-equal to a fresh context's."""
    B, T, F = uts.WIDE
    g, _ = grads_case(trainers, refs, f"gradients {B} x {T}, F = {F}", B, T, fd=F)
    assert len(g) == 163 and float(g[PW].abs().max()) > 0
    after = gpu_grads(trainers(F), 3, 43, P)
    fresh = make_trainer(3, 43, fd=F)
    try:
        same(after, gpu_grads(fresh, 3, 43, P))
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------- the fine-tuned encoder
def test_finetune_gradients_train(trainers, refs):
    """9 x 228, two encoder layers in train mode (published probabilities, a time mask with one span per sample, layer 1 skipped): every
    gradient; the positional convolution's weight gradient (16 groups x 48 x 6144, 16 chunks) fills the partial-tile buffer exactly."""
    B, T = uts.FT_FULL
    g, g64 = grads_case(trainers, refs, f"fine-tune {B} x {T}, train mode", B, T, layers=L, p=P, mode="train")
    skipped = [k for k in g if ".layers.1." in k]
    assert len(skipped) == 16 and all(float(g[k].abs().max()) == 0 and float(g64[k].abs().max()) == 0 for k in skipped)
    assert float(g[ENC + "masked_spec_embed"].abs().max()) > 0 and float(g[ENC + "encoder.pos_conv_embed.conv.weight_v"].abs().max()) > 0


@pytest.mark.parametrize("B,T", [uts.FT_FULL] + [(b, t) for b, t, _ in uts.FT_SMALL], ids=["9x228", "2x128", "1x257"])
def test_finetune_gradients_eval(trainers, refs, B, T):
    """Eval mode at 9 x 228, and at M = 256 / 257 tokens: pos_fwd and pos_dgrad with and without split_small."""
    cond = [True] if B == 1 else None
    g, _ = grads_case(trainers, refs, f"fine-tune {B} x {T}, eval mode", B, T, layers=L, cond=cond)
    assert float(g[ENC + "masked_spec_embed"].abs().max()) == 0
    assert float(g[ENC + "encoder.pos_conv_embed.conv.weight_v"].abs().max()) > 0 and float(g[ENC + "feature_projection.projection.weight"].abs().max()) > 0


def test_finetune_shape_order_does_not_matter(trainers):
    """9 x 228 then 2 x 128 in one context (16 chunks filling the buffer, then split_small's eight): bit-equal to a fresh context's."""
    tr = trainers(-1, L)
    gpu_grads(tr, *uts.FT_FULL, p=P, mode="train")
    after = gpu_grads(tr, 2, 128, P, mode="train")
    fresh = make_trainer(2, 128, layers=L)
    try:
        same(after, gpu_grads(fresh, 2, 128, P, mode="train"))
    finally:
        fresh.close()
