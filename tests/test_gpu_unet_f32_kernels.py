"""The fp32 (split-fp16) denoise step kernel by kernel (run on the MI355X with `-m gpu`).

fp32 mode with its default options — nothing switched off — is stopped behind every launch of the channel-major schedule (said_debug_stop_after), the launch's
inputs and outputs are read back AS STORED (the workspace list: Engine.ws_buffers / ws_snapshot), and the output is compared with tests/unet_f32_ref.py's evaluation
of those inputs in float64 (tests/test_unet_f32_ref_cpu.py ties that restatement to the oracle and shows that fourteen ways of being wrong exceed the bound 70 x
at least).  The rule is the project's (audio_bf16_ref.check_f32):
    max |got - ref64| / max |ref64| <= 4 max(e32, 1e-6),   e32 the same figure of the torch fp32 CPU evaluation of the identical inputs,
over all samples, channels and tokens [0, T).  Per launch: conv_in_kernel / the generic convolution (H0); ugemm_kernel with ugemm_body or kconv_body (the ResBlock
convolutions, one and two K segments, residual or 1x1 skip segments, the duplicate store); the q/k/v GEMM (q; k and v decoded from their packed split pairs, whose
low plane must be a rounded remainder of the stored high plane; the gn_coef rows); attn_kernel<PM = 3> / attn2q_kernel; stchain_kernel's whole tail; the out
convolution; out_sched_kernel<CFG> (guidance, DDIM update, eta noise, mask blend: masked elements bit-exact).  Every launch that stores GroupNorm partials: the
normalised tensor the merged partials imply against the float64 GroupNorm of the stored output.  Apart from the step: KV against the float64 projection of the
context, KVT as its exact transpose.  A buffer read again at a later stop must be bit-equal to what the earlier stop saw.  Pad tokens [T, Tp) are never compared:
instead every shape's forward pass and one guided step (with eta noise and the mask blend) run with the workspace filled with 0x00, 0xFF and 0x7F first and must be
finite and bit-identical — F, whose operand buffers have rows nobody writes, included.

Shapes (each the smallest that reaches what is named; asserted here from the stage log — kind, epi, NB, KS per launch — and the counters; what the log does not
carry — split-fp16 or fp32 matrix instructions, kconv_body or the block loop, token tiles per workgroup, the chain's slices — is held on the CPU by
tests/test_ugemm_plan_cpu.py::test_shapes_of_the_fp32_kernel_test_reach_what_they_are_named_for, from ugemm_plan.h and stchain.h):
  S      forward, 2 x 70 (6 token tiles, the last of a sample 6 tokens): every 192-wide GEMM and q/k/v at NB = 1, the concatenated convolutions on kconv_body,
         attention with 8 key slices, the three-slice chain; 24 launches.  Also on synth.trained_like_state_dict.
  G      one guided loop step, 1 clip x 70: conv_in_kernel with two copies, the duplicate stores, the shared first block, c2, out_sched_kernel<CFG>; 24 graph nodes.
  G-eta  as G with eta = 1 noise and a mask that crosses the token-tile boundary at 64.
  M1     forward, 3 x 290 (30 tiles): q/k/v NB = 3, attention with 4 key slices.
  M2     forward, 5 x 290 (50 tiles): 192-wide NB = 2, q/k/v NB = 2, the concatenated convolutions on the fp32-MFMA NB = 2 shapes.
  L      forward, 7 x 417 (98 tiles, a sample's last tile 1 token): 192-wide NB = 3, the kconv NB = 1 switch, q/k/v on the multi-tile fp32 kernel storing packed
         k / v, attn2q_kernel with a phantom query tile, the two-slice chain (98 > CHAIN3_MAX_TILES = 85).
  F      forward, 3 x 70 with said_debug_option "unet_tgemm_min_tokens" = 0: the large-batch fp32 route at toy size — prep_kernel in pack mode on its own (the
         operand buffers uPA / uPL, the raw copy uPB for the 1x1 skip, the padding rows, the gn_coef rows) and fgemm_kernel<SP, PK> for the ResBlock convolutions
         and q/k/v from those stored operands, then attention and the chain; 40 launches.
Measured (MI355X; e of max |ref| beside the fp32 CPU evaluation's own e32, over all shapes; the bound is its floor 4e-6 everywhere, e32 <= 9.4e-7): conv_in
1.6e-7 (e32 2.0e-7); ResBlock conv 1 / conv 2 on ugemm_kernel 2.9e-7 / 2.5e-7 (6.1e-7 / 6.0e-7), on fgemm_kernel 3.3e-7 / 2.1e-7; q / k / v 2.5e-7 / 3.1e-7 / 2.7e-7
(7.5e-7 / 9.1e-7 / 6.4e-7), on fgemm_kernel 1.5e-7 / 1.8e-7 / 1.7e-7; gn_coef a / b 1.9e-7 / 2.9e-7; self-attention 3.2e-7 on the plain fill, 9.7e-7 on the
trained-like one (e32 9.4e-7); the chain 3.8e-7 (6.9e-7); the out convolution 2.0e-7; out_sched_kernel<CFG> 2.9e-7, with eta noise and the mask 3.0e-7 (5.8e-7);
prep_kernel's operands 2.4e-7 ... 2.9e-7; GroupNorm from the stored partials 9e-9 ... 3.8e-8 (the fp32 CPU GroupNorm: 7e-8 ... 1.5e-7); KV 4.3e-7; no packed pair
inconsistent (one element in ~2000 has a remainder of exactly half a step); KVT, y2, conv_in's second copy, masked elements exact; the fills (S, M1, M2, L, F; forward pass and guided step with eta noise and mask) finite
and bit-identical.
Largest e per shape: S 3.1e-7, M1 2.7e-7, M2 3.2e-7, L 4.3e-7, S trained-like 9.7e-7, G 2.9e-7, G-eta 3.0e-7, F 3.3e-7.  pytest --durations: L 1.1 s,
S trained-like 0.8 s, S 0.5 s, M2 0.3 s, M1 0.2 s, F 0.14 s, G / G-eta 0.1 s, each of the five fill tests <= 0.03 s (the module's model 2 s once).
"""
import numpy as np
import pytest
import torch

import unet_f32_ref as R
from audio_bf16_ref import check_exact, check_f32
from oracle import pipeline as op
from said_amd.util import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
F64, F32 = torch.float64, torch.float32
MC = R.MC
GS = 2.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _model(dev, sd):
    from said_amd.model.diffusion import SAID_UNet1D
    from said_amd.model.wav2vec2 import AudioConfig
    m = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=1))
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def plain(dev):
    sd = synth.said_state_dict(num_w2v_layers=1)
    _, sd_u, null = op.split_state_dict(sd)
    return _model(dev, sd), sd_u, null


# ---------------------------------------------------------------- the schedule (unet_sched.cpp run_unet) and what each launch reads and writes
def _schedule(guided):
    L = [("conv_in",)]

    def res(i, in0, in1, out, shared=False):
        L.append(("conv1", i, in0, in1, shared))
        L.append(("conv2", i, in0, in1, out, shared))

    def st(j, inn, out, shared=False):
        L.append(("qkv", j, inn, shared))
        L.append(("attn", j, shared))
        L.append(("chain", j, inn, out, shared))

    res(0, "H0", None, "P", guided); st(0, "P", "H1", guided)
    res(1, "H1", None, "P"); st(1, "P", "Q")
    res(2, "Q", None, "P")
    res(3, "P", "H1", "Q"); st(2, "Q", "P")
    res(4, "P", "H0", "Q"); st(3, "Q", "P")
    L.append(("out_sched",) if guided else ("out",))
    return L


def _io(launch):
    """(buffers read, buffers written) of a launch, by workspace name."""
    k = launch[0]
    if k == "conv_in":
        return ["x"], ["H0", "stH0"]
    if k == "conv1":
        srcs = [s for s in launch[2:4] if s]
        return srcs + ["st" + s for s in srcs] + ["EO"], ["M", "stM"]
    if k == "conv2":
        srcs = [s for s in launch[2:4] if s]
        return ["M", "stM"] + srcs, [launch[4], "st" + launch[4]]
    if k == "qkv":
        return [launch[2], "st" + launch[2]], ["QK", "VT", "gn_coef"]
    if k == "attn":
        return ["QK", "VT"], ["O"]
    if k == "chain":
        return ["O", launch[2], "gn_coef", "KV"], [launch[3], "st" + launch[3]]
    if k == "out":
        return ["P", "stP"], ["eps"]
    if k == "prep0":     # operand of a ResBlock convolution from source `src` into columns [off, off + 192) of uPA (and its raw copy into uPB)
        _, i, src, off, cin, raw = launch
        return [src, "st" + src], [f"uPA:{cin}"] + ([f"uPB:{2 * MC}"] if raw else [])
    if k == "fconv1":
        return [f"uPA:{launch[2]}", "EO"], ["M", "stM"]
    if k == "fconv2":
        _, i, in0, in1, out = launch
        return [f"uPA:{MC}"] + ([f"uPB:{2 * MC}"] if in1 else [in0]), [out, "st" + out]
    if k == "prep1":
        return [launch[2], "st" + launch[2]], [f"uPL:{MC}", "gn_coef"]
    if k == "fqkv":
        return [f"uPL:{MC}"], ["QK", "VT"]
    return ["P", "stP"], []   # out_sched: its output is the loop's result


def _expected_stages(guided, nb_in, nb, nb_cat, nb_qkv, ks):
    """(kind, epi, NB, KS) per launch as unet_sched.cpp logs them: 0 the generic GEMM, 2 ugemm_kernel, 1 attention (NB = head_dim / 32; KS 34 = attn2q_kernel),
    10 stchain_kernel, 11 conv_in_kernel, 12 the out convolution.  profile_unet never logs out_sched_kernel: its stage list ends with the out convolution."""
    out = []
    for la in _schedule(False):
        k = la[0]
        if k == "conv_in":
            out.append((11, 0, 1, 4) if guided else (0, 0, nb_in, 8))
        elif k in ("conv1", "conv2"):
            out.append((2, 0, nb_cat if la[3] else nb, 8))
        elif k == "qkv":
            out.append((2, 1, nb_qkv, 8))
        elif k == "attn":
            out.append((1, -1, 1, ks))
        elif k == "chain":
            out.append((10, 0, 6, 8))
        else:
            out.append((12, 0, 1, 8))
    return out


class Stops:
    """One shape's stopped runs: `run` makes the call (forward pass or loop step), stop(k, launch) makes it with the first k launches and reads the launch's buffers."""

    def __init__(self, eng, Be, T, S, run):
        self.eng, self.Be, self.T, self.S, self.run = eng, Be, T, S, run
        self.Tp, self.Sp, self.np = R.rup(T, 32), R.rup(S, 32), (T + 31) // 32
        self.sizes = {nm: nb for _, nm, nb in eng.ws_buffers()}
        self.index = {nm: i for i, nm, _ in eng.ws_buffers()}
        self.cur = {}

    def raw(self, name, nfloat):
        assert 4 * nfloat <= self.sizes[name], (name, nfloat, self.sizes[name])
        t = self.eng.ws_snapshot(self.index[name], 4 * nfloat)
        torch.cuda.synchronize()
        return t.cpu().view(torch.float32)

    def read(self, name):
        """The buffer as stored, pad tokens removed."""
        Be, T, Tp = self.Be, self.T, self.Tp
        if name in ("H0", "H1", "P", "Q", "M"):
            return self.raw(name, Be * MC * Tp).view(Be, MC, Tp)[:, :, :T].clone()
        if name.startswith("st"):
            return self.raw(name, Be * self.np * MC * 2).view(Be, self.np, MC, 2).clone()
        if name in ("x", "eps"):
            return self.raw(name, Be * 32 * Tp).view(Be, 32, Tp)[:, :, :T].clone()
        if name == "O":
            return self.raw(name, Be * 2 * MC * Tp).view(Be, 2 * MC, Tp)[:, :MC, :T].clone()
        if name == "QK":
            return self.raw(name, Be * 12 * Tp * 32).view(Be, 12, Tp, 32)[:, :, :T].clone()
        if name == "VT":
            return self.raw(name, Be * MC * Tp).view(Be, MC, Tp)[:, :, :T].clone()
        if name == "gn_coef":
            return self.raw(name, Be * MC * 2).view(Be, MC, 2).clone()
        if name == "EO":
            n = self.sizes["EO"] // 4
            return self.raw(name, n).view(5, MC, n // (5 * MC))[:, :, :max(Be, 1)].clone()
        if name == "KV":
            return self.raw(name, Be * R.NST * 2 * MC * self.Sp).view(Be, R.NST * 2 * MC, self.Sp)[:, :, :self.S].clone()
        if name == "KVT":
            return self.raw(name, Be * self.S * R.NST * 2 * MC).view(Be, self.S, R.NST * 2 * MC).clone()
        if name.startswith("uP"):   # token-major operands of the large-batch route: [sample][rup(T + 2, 32) rows][columns] dwords
            cols = int(name.split(":")[1])
            rows = R.rup(T + 2, 32)
            return self.raw(name.split(":")[0], Be * rows * cols).view(Be, rows, cols).clone()
        raise KeyError(name)

    def stop(self, k, launch):
        """Runs the first k launches; re-reads the launch's inputs (bit-equal to what an earlier stop saw) and reads its outputs."""
        self.eng.debug_stop_after(k)
        self.run()
        ins, outs = _io(launch)
        for name in ins:
            v = self.read(name)
            if name in self.cur:
                assert torch.equal(v.view(torch.int32), self.cur[name].view(torch.int32)), f"launch {k} {launch}: {name} differs from what the earlier stop saw"
            self.cur[name] = v
        for name in outs:
            self.cur[name] = self.read(name)
        return self.cur


def _partials(tag, y, st):
    """The normalised tensor the stored partials imply against the float64 GroupNorm of the stored output (32 groups of 6 channels, eps 1e-5)."""
    got = R.norm_from_partials(y, st)
    return check_f32(f"{tag}: GroupNorm from the stored partials", got, R.group_norm(y, 32, None, None, 1e-5, F64), R.group_norm(y, 32, None, None, 1e-5, F32))


def _split(tag, packed):
    val, h, lo = R.decode_split(packed)
    bad, ties = R.split_is_consistent(h, lo)
    print(f"{tag}: {bad} of {h.numel()} packed pairs inconsistent ({ties} with a remainder of exactly half a step)")
    assert bad == 0, f"{tag}: the low plane of {bad} elements is no rounded remainder of the stored high plane"
    return val


def _check_launch(tag, sd, null, la, c, Be, Bc, rec):
    """One launch on its own stored inputs.  c: buffer name -> tensor as stored; Bc > 0: the guided step's sample layout (unconditional half first)."""
    k = la[0]
    shared = bool(la[-1]) if k in ("conv1", "conv2", "qkv", "attn", "chain") else False
    ns = Bc if shared else Be                     # samples this launch computes
    f = lambda name, fn, got: rec.append((name,) + check_f32(f"{tag} {name}", got, fn(F64), fn(F32)))
    if k == "conv_in":
        x = c["x"][:Bc] if Bc else c["x"]
        f("conv_in", lambda dt: R.conv_in(sd, x, dt), c["H0"][:x.shape[0]])
        if Bc:
            check_exact(f"{tag} conv_in: the second copy", c["H0"][Bc:], c["H0"][:Bc])
            assert torch.equal(c["stH0"][Bc:], c["stH0"][:Bc])
        rec.append(("stH0",) + _partials(f"{tag} conv_in", c["H0"], c["stH0"]))
    elif k == "conv1":
        _, i, in0, in1, _ = la
        xs = [c[s][:ns] for s in (in0, in1) if s]
        e_row = c["EO"][i][:, :1].t().expand(ns, -1) if Bc else c["EO"][i][:, :ns].t()
        f(f"res{i} conv 1 ({len(xs)} segment{'s' if len(xs) > 1 else ''})", lambda dt: R.res_conv1(sd, i, xs, e_row, dt), c["M"][:ns])
        rec.append(("stM",) + _partials(f"{tag} res{i} conv 1", c["M"][:ns], c["stM"][:ns]))
    elif k == "conv2":
        _, i, in0, in1, out, _ = la
        xs = [c[s][:ns] for s in (in0, in1) if s]
        f(f"res{i} conv 2 ({'1x1 skip segments' if in1 else 'residual'})", lambda dt: R.res_conv2(sd, i, c["M"][:ns], xs, dt)[0], c[out][:ns])
        rec.append(("st" + out,) + _partials(f"{tag} res{i} conv 2", c[out][:ns], c["st" + out][:ns]))
        if shared:
            check_exact(f"{tag} res{i} conv 2: the duplicate store y2", c[out][Bc:], c[out][:Bc])
    elif k == "qkv":
        _, j, inn, _ = la
        x = c[inn][:ns]
        kd, vd = _split(f"{tag} st{j} k", c["QK"][:ns, 6:]), _split(f"{tag} st{j} v", c["VT"][:ns])
        c["k_dec"], c["v_dec"] = kd, vd
        for n, idx, got in (("q", 0, c["QK"][:ns, :6]), ("k", 1, kd), ("v", 2, vd)):
            f(f"st{j} q/k/v: {n}", lambda dt: R.qkv(sd, j, x, dt)[idx], got)
        for n, idx in (("a", 0), ("b", 1)):
            f(f"st{j} gn_coef {n}", lambda dt: R.gn_coef(sd, j, x, dt)[..., idx], c["gn_coef"][:ns, :, idx])
    elif k == "attn":
        _, j, _ = la
        f(f"st{j} self-attention", lambda dt: R.self_attention(c["QK"][:ns, :6], c["k_dec"][:ns], c["v_dec"][:ns], dt), c["O"][:ns])
    elif k == "chain":
        _, j, inn, out, _ = la
        kv = c["KV"][:, j * 2 * MC:(j + 1) * 2 * MC].clone()
        kv[:Bc] = 0   # (the unconditional half's rows are never written, and never read)
        f(f"st{j} chain", lambda dt: R.chain(sd, j, c["O"][:ns], c[inn][:ns], c["gn_coef"][:ns], kv[:, :MC], kv[:, MC:], dt, nsamp=Be, in_mod=Bc if shared else 0,
                                            n_uncond=Bc, null=null), c[out])
        rec.append(("st" + out,) + _partials(f"{tag} st{j} chain", c[out], c["st" + out]))
    elif k == "out":
        f("out convolution", lambda dt: R.out_conv(sd, c["P"], dt), c["eps"])
    else:
        raise KeyError(k)


def _kv_checks(tag, sd, s, ctx, b0, rec):
    """KV of samples [b0, Be) against the float64 projection of their context; KVT its exact transpose."""
    kv, kvt = s.read("KV"), s.read("KVT")
    rec.append(("KV",) + check_f32(f"{tag} KV", kv[b0:], R.kv_all(sd, ctx, F64), R.kv_all(sd, ctx, F32)))
    check_exact(f"{tag} KVT (key-major copy)", kvt[b0:], kv[b0:].transpose(1, 2))


def _summary(tag, rec):
    print(f"{tag}: {len(rec)} comparisons, largest e {max(e for _, e, _ in rec):.2e}, largest e / bound {max(e / b for _, e, b in rec):.3f}")


# ---------------------------------------------------------------- forward shapes
def _forward_case(model, sd, dev, tag, B, T, seed, stages):
    x = synth.synth_latents(seed, (B, T, 32))
    ctx = synth.synth_latents(seed + 1, (B, T, 768))
    ts = (torch.arange(B) * 137 + 500) % 1000
    eng = model._get_engine(max(B, 2), max(T, 64))
    xd, cd = x.to(dev), ctx.to(dev)
    out = {}

    def run():
        out["y"] = eng.unet_forward(xd, ts, cd)
        torch.cuda.synchronize()

    s = Stops(eng, B, T, T, run)
    sched = _schedule(False)
    rec = []
    try:
        n0 = eng.debug_get("n_stchain")
        for k, la in enumerate(sched, 1):
            c = s.stop(k, la)
            if k == 1:
                check_exact(f"{tag} x (channel-major latents)", c["x"], x.transpose(1, 2))
                _kv_checks(tag, sd, s, ctx, 0, rec)
            _check_launch(tag, sd, None, la, c, B, 0, rec)
        # stop k issues the first k launches again: 3 + 2 x 5 + ... fused tails in all
        assert eng.debug_get("n_stchain") - n0 == sum(1 for k in range(1, len(sched) + 1) for la in sched[:k] if la[0] == "chain")
        eng.debug_stop_after(-1)
        run()
        check_exact(f"{tag} the unstopped call's result against the last stop's eps", out["y"].cpu().transpose(1, 2), s.cur["eps"])
        for name in ("P", "stP", "KV"):
            assert torch.equal(s.read(name).view(torch.int32), s.cur[name].view(torch.int32)), name
        log = [(d["kind"], d["epi"], d["NB"], d["KS"]) for d in eng.profile_unet(B, T, reps=1)]
    finally:
        eng.debug_stop_after(-1)
    print(f"{tag}: stage log {log}")
    assert stages is None or log == stages, f"{tag}: the launches are not the ones this shape is here for"
    _summary(tag, rec)


def _poison(model, dev, B, T, seed, opts=None):
    """Forward pass and one guided step (eta = 1 noise, initial latents, edit noise and a mask across the tile boundary at 64: everything out_sched_kernel<CFG> reads)
    with the workspace filled with 0x00, 0xFF (NaN) and 0x7F (3.4e38) first: finite and bit-identical.  opts: said_debug_option settings, restored afterwards."""
    x = synth.synth_latents(seed, (B, T, 32)).to(dev)
    ctx = synth.synth_latents(seed + 1, (B, T, 768)).to(dev)
    ts = (torch.arange(B) * 137 + 500) % 1000
    sch = model.noise_scheduler
    sch.set_timesteps(50)
    tsl = sch.timesteps.numpy()
    coef = sch.coef_table(tsl[24:26], 1.0)[:1]   # (the blend's pair is the next timestep's)
    mask = torch.zeros(B, T, 32)
    mask[:, 60:68] = 1
    mask[:, :, :5] = 1
    kw = dict(step_noise=synth.synth_latents(seed + 2, (1, B, T, 32)).to(dev), init_latents=synth.synth_latents(seed + 3, (B, T, 32)).abs().clamp(0, 1).to(dev),
              edit_noise=synth.synth_latents(seed + 4, (B, T, 32)).to(dev), mask=mask.to(dev))
    eng = model._get_engine(2 * B, max(T, 64))
    ref = None
    try:
        for k, v in (opts or {}).items():
            eng.debug_option(k, v)
        for fill in (0x00, 0xFF, 0x7F):
            eng.ws_fill(fill)
            o1 = eng.unet_forward(x, ts, ctx).cpu()
            eng.ws_fill(fill)
            o2 = eng.denoise_loop(latents=x, context=ctx, timesteps=tsl[24:25], coef=coef, prediction_type="epsilon", guidance_scale=GS, guidance_rescale=0.0,
                                  latent_scale=1.0, **kw)[1].cpu()
            assert torch.isfinite(o1).all() and torch.isfinite(o2).all(), f"fill 0x{fill:02X}: a result is not finite"
            if ref is None:
                ref = (o1, o2)
            assert torch.equal(o1, ref[0]) and torch.equal(o2, ref[1]), f"fill 0x{fill:02X}: a result depends on memory nobody wrote"
    finally:
        for k in (opts or {}):
            eng.debug_option(k, -1)
    return eng


#        tag   B  T    conv_in NB, 192-wide NB, concatenated NB, q/k/v NB, attention KS
SHAPES = {"S": (2, 70, 1, 1, 1, 1, 8), "M1": (3, 290, 1, 1, 1, 3, 4), "M2": (5, 290, 2, 2, 2, 2, 4), "L": (7, 417, 2, 3, 1, 3, 34)}


@pytest.mark.parametrize("tag", list(SHAPES))
def test_forward_launches_on_their_own_inputs(plain, dev, tag):
    """Every launch of the forward pass at shapes S, M1, M2 and L (all launches, all samples)."""
    model, sd, _ = plain
    B, T, *nbs = SHAPES[tag]
    _forward_case(model, sd, dev, tag, B, T, 400 + 10 * len(tag) + B, _expected_stages(False, *nbs))


def test_forward_launches_on_trained_like_weights(dev):
    """Shape S on synth.trained_like_state_dict (heavy tails, outlier channels, norm gains up to 10: the fill that found DESIGN 9.2's bug)."""
    full = synth.trained_like_state_dict(num_w2v_layers=1)
    _, sd_u, _ = op.split_state_dict(full)
    model = _model(dev, full)
    B, T, *nbs = SHAPES["S"]
    _forward_case(model, sd_u, dev, "S trained-like", B, T, 431, _expected_stages(False, *nbs))


@pytest.mark.parametrize("tag", list(SHAPES) + ["F"])
def test_workspace_fill_does_not_reach_a_result(plain, dev, tag):
    """The stand-in for comparing pad tokens: every shape's forward pass and one guided step from a workspace of zeros, NaNs and 3.4e38.  F: the large-batch route,
    whose token-major operands have rup(T + 2, 32) rows per sample of which prep_kernel writes T + 2 and fgemm_kernel's 64-row tiles read more."""
    model, _, _ = plain
    B, T = (3, 70) if tag == "F" else SHAPES[tag][:2]
    opts = {"unet_tgemm_min_tokens": 0} if tag == "F" else None
    eng = _poison(model, dev, B, T, 450 + B + (10 if tag == "F" else 0), opts)
    if tag == "F":   # the option reached the schedule: with it the forward pass has prep_kernel / fgemm_kernel launches (kinds 5 / 4), without it none
        try:
            eng.debug_option("unet_tgemm_min_tokens", 0)
            kinds = [d["kind"] for d in eng.profile_unet(B, T, reps=1)]
        finally:
            eng.debug_option("unet_tgemm_min_tokens", -1)
        assert kinds.count(5) == 16 and kinds.count(4) == 14, kinds


# ---------------------------------------------------------------- the guided loop step
@pytest.mark.parametrize("case", ["G", "G-eta"])
def test_guided_step_launches_on_their_own_inputs(plain, dev, case):
    """One guided loop step of one clip x 70 frames (Engine.denoise_loop, one timestep, guidance 2): every launch of the headline's own structure, then
    out_sched_kernel<CFG> against the float64 out convolution + guidance + update of its stored inputs (G-eta: with eta = 1 noise and the mask blend; the blend's
    coefficient pair is the next timestep's, from a two-step table)."""
    model, sd, null = plain
    Bc, T, k = 1, 70, 24
    Be = 2 * Bc
    eta = 1.0 if case == "G-eta" else 0.0
    lat = synth.synth_latents(461, (Bc, T, 32))
    ctx = synth.synth_latents(462, (Bc, T, 768))
    sch = model.noise_scheduler
    sch.set_timesteps(50)
    ts = sch.timesteps.numpy()
    coef = sch.coef_table(ts[k:k + 2], eta)[:1]
    kw, kwd = {}, {}
    if eta > 0:
        mask = torch.zeros(Bc, T, 32)
        mask[:, 60:68] = 1
        mask[:, :, :5] = 1
        kw = dict(noise=synth.synth_latents(463, (Bc, T, 32)), init=synth.synth_latents(464, (Bc, T, 32)).abs().clamp(0, 1), enoise=synth.synth_latents(465, (Bc, T, 32)),
                  mask=mask)
        kwd = dict(step_noise=kw["noise"][None].to(dev), init_latents=kw["init"].to(dev), edit_noise=kw["enoise"].to(dev), mask=mask.to(dev))
    eng = model._get_engine(Be, max(T, 64))
    latd, ctxd = lat.to(dev), ctx.to(dev)
    out = {}

    def run():
        out["y"] = eng.denoise_loop(latents=latd, context=ctxd, timesteps=ts[k:k + 1], coef=coef, prediction_type="epsilon", guidance_scale=GS, guidance_rescale=0.0,
                                    latent_scale=1.0, **kwd)[1]
        torch.cuda.synchronize()

    s = Stops(eng, Be, T, T, run)
    sched = _schedule(True)
    rec = []
    try:
        n0 = eng.debug_get("n_out_sched")
        for n, la in enumerate(sched[:-1], 1):
            c = s.stop(n, la)
            if n == 1:
                check_exact(f"{case} x (channel-major latents)", c["x"][:Bc], lat.transpose(1, 2))
                _kv_checks(case, sd, s, ctx, Bc, rec)
            _check_launch(case, sd, null, la, c, Be, Bc, rec)
        assert eng.debug_get("n_out_sched") == n0, "no stop so far reached the step's last launch"
        eng.debug_stop_after(-1)
        run()
        assert eng.debug_get("n_out_sched") > n0 and eng.graph_num_nodes() == 24
        for name in ("P", "stP"):
            assert torch.equal(s.read(name).view(torch.int32), s.cur[name].view(torch.int32)), name
        log = [(d["kind"], d["epi"], d["NB"], d["KS"]) for d in eng.profile_unet(Be, T, reps=1, cfg_clips=Bc)]
    finally:
        eng.debug_stop_after(-1)
    assert log == _expected_stages(True, 1, 1, 1, 1, 8), log
    got = out["y"].cpu()
    P = s.cur["P"]
    cm = {n: v.transpose(1, 2) for n, v in kw.items()}
    fn = lambda dt: R.out_sched(sd, P, lat.transpose(1, 2), coef[0], GS, dt, **cm).transpose(1, 2)
    rec.append(("out_sched",) + check_f32(f"{case} out_sched_kernel<CFG>", got, fn(F64), fn(F32)))
    rec.append(("stP",) + _partials(f"{case} st3 chain (out_sched's input)", P, s.cur["stP"]))
    if eta > 0:   # masked elements do not depend on the model output: add_noise(init, edit_noise, t_next) in fp32, bit for bit
        m = kw["mask"].bool()
        cf = torch.from_numpy(np.asarray(coef[0], dtype=np.float32))
        assert float(cf[5]) != 1.0 and float(cf[6]) != 0.0, "the blend's pair is the next timestep's"
        noisy = cf[5] * kw["init"] + cf[6] * kw["enoise"]
        assert torch.equal(got[m], noisy[m]), "a masked element is not the noised initial latent"
        assert bool(m[:, 60:68].all()) and not bool(m[:, 68:, 5:].any()), "the mask crosses the token-tile boundary at 64"
    _summary(case, rec)


# ---------------------------------------------------------------- shape F: the large-batch route (prep_kernel + fgemm_kernel) at toy size
def _schedule_f():
    L = [("conv_in",)]

    def res(i, in0, in1, out):
        cin = 2 * MC if in1 else MC
        for off, src in enumerate(s for s in (in0, in1) if s):
            L.append(("prep0", i, src, off * MC, cin, bool(in1)))
        L.append(("fconv1", i, cin))
        L.append(("prep0", i, "M", 0, MC, False))
        L.append(("fconv2", i, in0, in1, out))

    def st(j, inn, out):
        L.extend([("prep1", j, inn), ("fqkv", j), ("attn", j, False), ("chain", j, inn, out, False)])

    res(0, "H0", None, "P"); st(0, "P", "H1")
    res(1, "H1", None, "P"); st(1, "P", "Q")
    res(2, "Q", None, "P")
    res(3, "P", "H1", "Q"); st(2, "Q", "P")
    res(4, "P", "H0", "Q"); st(3, "Q", "P")
    L.append(("out",))
    return L


def _packed_operand(tag, buf, T, row_off):
    """A packed operand buffer (B, rows, columns): the T token rows decoded, the Conv1d padding rows (row_off = 1: rows 0 and T + 1) all-zero bits."""
    if row_off:
        assert int(buf[:, 0].view(torch.int32).abs().sum()) == 0 and int(buf[:, T + 1].view(torch.int32).abs().sum()) == 0, f"{tag}: a padding row is not zero"
    return _split(tag, buf[:, row_off:row_off + T])


def _check_launch_f(tag, sd, la, c, B, T, rec):
    k = la[0]
    f = lambda name, fn, got: rec.append((name,) + check_f32(f"{tag} {name}", got, fn(F64), fn(F32)))
    if k == "prep0":
        _, i, src, off, cin, raw = la
        op_ = _packed_operand(f"{tag} res{i} uPA columns [{off}, {off + MC})", c[f"uPA:{cin}"][:, :, off:off + MC], T, 1)
        if src == "M":
            f(f"res{i} prep_kernel, conv 2's operand", lambda dt: R.res_operand2(sd, i, c["M"], dt).transpose(1, 2), op_)
        else:
            c.setdefault(("srcs", i), []).append(c[src])
            if off == 0 and raw:
                return   # (GroupNorm spans both sources: checked behind the second preparation launch)
            xs = c.pop(("srcs", i))
            full = _packed_operand(f"{tag} res{i} uPA", c[f"uPA:{cin}"], T, 1)
            f(f"res{i} prep_kernel, conv 1's operand ({len(xs)} source{'s' if len(xs) > 1 else ''})", lambda dt: R.res_operand1(sd, i, xs, dt).transpose(1, 2), full)
            if raw:   # the raw copy: the same values, packed (h + 2^-11 l holds 22 significand bits)
                rawv = _packed_operand(f"{tag} res{i} uPB", c[f"uPB:{2 * MC}"], T, 0)
                want = torch.cat(xs, dim=1).transpose(1, 2).double()
                assert bool(((rawv - want).abs() <= 2.0 ** -21 * want.abs() + 2.0 ** -36).all()), f"{tag} res{i}: the raw copy for the 1x1 skip is not the input"
    elif k == "fconv1":
        _, i, cin = la
        op_ = _packed_operand(f"{tag} res{i} uPA", c[f"uPA:{cin}"], T, 1).transpose(1, 2)
        f(f"res{i} conv 1 on fgemm_kernel ({cin // MC} source{'s' if cin > MC else ''})", lambda dt: R.res_conv1(sd, i, None, c["EO"][i][:, :B].t(), dt, operand=op_), c["M"])
        rec.append(("stM",) + _partials(f"{tag} res{i} conv 1", c["M"], c["stM"]))
    elif k == "fconv2":
        _, i, in0, in1, out = la
        op_ = _packed_operand(f"{tag} res{i} uPA", c[f"uPA:{MC}"], T, 1).transpose(1, 2)
        if in1:
            rawv = _packed_operand(f"{tag} res{i} uPB", c[f"uPB:{2 * MC}"], T, 0).transpose(1, 2)
            xs = [rawv[:, :MC], rawv[:, MC:]]
        else:
            xs = [c[in0]]
        f(f"res{i} conv 2 on fgemm_kernel ({'1x1 skip segment' if in1 else 'residual'})", lambda dt: R.res_conv2(sd, i, None, xs, dt, operand=op_)[0], c[out])
        rec.append(("st" + out,) + _partials(f"{tag} res{i} conv 2", c[out], c["st" + out]))
    elif k == "prep1":
        _, j, inn = la
        op_ = _packed_operand(f"{tag} st{j} uPL", c[f"uPL:{MC}"], T, 0)
        f(f"st{j} prep_kernel, q/k/v's operand", lambda dt: R.qkv_operand(sd, j, c[inn], dt), op_)
        for n, idx in (("a", 0), ("b", 1)):
            f(f"st{j} gn_coef {n}", lambda dt: R.gn_coef(sd, j, c[inn], dt)[..., idx], c["gn_coef"][:, :, idx])
    elif k == "fqkv":
        _, j = la
        op_ = _packed_operand(f"{tag} st{j} uPL", c[f"uPL:{MC}"], T, 0)
        kd, vd = _split(f"{tag} st{j} k", c["QK"][:, 6:]), _split(f"{tag} st{j} v", c["VT"])
        c["k_dec"], c["v_dec"] = kd, vd
        for n, idx, got in (("q", 0, c["QK"][:, :6]), ("k", 1, kd), ("v", 2, vd)):
            f(f"st{j} q/k/v on fgemm_kernel: {n}", lambda dt: R.qkv(sd, j, None, dt, operand=op_)[idx], got)
    else:
        _check_launch(tag, sd, None, la, c, B, 0, rec)


def test_large_batch_route_at_toy_size(plain, dev):
    """Shape F: prep_kernel in pack mode and fgemm_kernel<SP, PK> on their own stored inputs, then attention and the chain behind them."""
    model, sd, _ = plain
    B, T, tag = 3, 70, "F"
    x = synth.synth_latents(471, (B, T, 32))
    ctx = synth.synth_latents(472, (B, T, 768))
    ts = (torch.arange(B) * 137 + 500) % 1000
    eng = model._get_engine(max(B, 2), max(T, 64))
    xd, cd = x.to(dev), ctx.to(dev)
    out = {}

    def run():
        out["y"] = eng.unet_forward(xd, ts, cd)
        torch.cuda.synchronize()

    sched = _schedule_f()
    assert len(sched) == 40
    rec = []
    try:
        eng.debug_option("unet_tgemm_min_tokens", 0)
        s = Stops(eng, B, T, T, run)
        for k, la in enumerate(sched, 1):
            c = s.stop(k, la)
            _check_launch_f(tag, sd, la, c, B, T, rec)
        eng.debug_stop_after(-1)
        run()
        check_exact(f"{tag} the unstopped call's result against the last stop's eps", out["y"].cpu().transpose(1, 2), s.cur["eps"])
        log = [(d["kind"], d["epi"], d["NB"], d["KS"]) for d in eng.profile_unet(B, T, reps=1)]
    finally:
        eng.debug_stop_after(-1)
        eng.debug_option("unet_tgemm_min_tokens", -1)
    # 5 the preparation kernel, 4 the token-major fp32 GEMM (96-column tiles, KS 32 marks fgemm_kernel); the rest as in _expected_stages
    want = {"conv_in": (0, 0, 1, 8), "prep0": (5, -2, 0, 0), "prep1": (5, -2, 0, 0), "fconv1": (4, 0, 96, 32), "fconv2": (4, 0, 96, 32), "fqkv": (4, 1, 96, 32),
            "attn": (1, -1, 1, 8), "chain": (10, 0, 6, 8), "out": (12, 0, 1, 8)}
    print(f"{tag}: stage log {log}")
    assert log == [want[la[0]] for la in sched], f"{tag}: the launches are not the ones this shape is here for"
    _summary(tag, rec)
