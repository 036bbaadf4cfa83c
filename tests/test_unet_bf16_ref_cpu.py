"""tests/unet_bf16_ref.py on the CPU: tied to the oracle, its caps measured, and its rules shown to have teeth.

* Tie: the launches chained in schedule order with rounded=False in float64 — with the fused tail and with the six-launch tail — against the oracle's op sequence in
  float64 (oracle/unet.py with its `.float()` casts redirected), for the forward pass at shape S (3 x 70) and for one guided DDIM step (2 clips x 70): 1e-14 of range.
  With the roundings on, the distance to oracle/unet.py under ROUND_OPERANDS = "bf16" / ROUND_STORES is printed, not bounded: the rounding points differ by design.
* Caps: the multi-product launches' caps (unet_bf16_ref.CAPS) are measured again — 4 x the largest pre-store |fp32 - float64| of the reference pair over 64 draws per
  launch kind and fill — and must be the recorded ones and <= 1e-2 of range.
* Teeth: every mutant of unet_bf16_ref.MUTANTS, applied to the reference of the launch it belongs to and compared by that launch's rule with the unmutated reference of
  the same stored inputs, must fail the rule at least ten times over (the worst element's distance over its bound, or the share of unequal elements over the allowed
  share, whichever is larger).  The factors are printed.
"""
import math
from unittest import mock

import pytest
import torch

import unet_bf16_ref as R
from audio_bf16_ref import bf16_step, f32_bound, rel_max, round_bf16
from oracle import pipeline as op
from oracle import scheduler as osch
from oracle import unet as ou
from said_amd.util import synth

torch.set_grad_enabled(False)
F64, F32 = torch.float64, torch.float32
B, T = 3, 70           # shape S
GS = 2.0
NDRAWS = 64


@pytest.fixture(scope="module")
def sds():
    out = {}
    for fill, make in (("plain", synth.said_state_dict), ("trained", synth.trained_like_state_dict)):
        _, sd_u, null = op.split_state_dict(make(num_w2v_layers=1))
        out[fill] = (sd_u, null)
    return out


@pytest.fixture(scope="module")
def inputs():
    return synth.synth_latents(301, (B, T, 32)), (torch.arange(B) * 137 + 500) % 1000, synth.synth_latents(302, (B, T, 768))


def _oracle64(sd_u, x, ts, c):
    with mock.patch.object(torch.Tensor, "float", torch.Tensor.double):
        return ou.unet1d_forward({k: v.double() for k, v in sd_u.items()}, x.double(), ts, c.double())


# ---------------------------------------------------------------- the tie
@pytest.mark.parametrize("six", [False, True])
def test_forward_chained_in_float64_is_the_oracle(sds, inputs, six):
    sd_u, _ = sds["plain"]
    x, ts, c = inputs
    tr = []
    out = R.forward(sd_u, x.transpose(1, 2), ts, c, False, F64, six=six, trace=tr)
    assert len(tr) == (47 if six else 32), "conv_in, 2 + 2 + 2 + 4 + 4 ResBlock launches, 3 x (q/k/v, attention, tail) + the last block's seven, out"
    e = rel_max(out, _oracle64(sd_u, x, ts, c))
    print(f"forward, launches chained in float64 ({'six-launch' if six else 'fused'} tail) vs the oracle in float64: {e:.2e} of max |ref|")
    assert e <= 1e-14


@pytest.mark.parametrize("six", [False, True])
def test_guided_step_chained_in_float64_is_the_oracle(sds, inputs, six):
    from said_amd.scheduler import DDIMScheduler
    sd_u, null = sds["plain"]
    lat, c = inputs[0][:2], inputs[2][:2]
    sch = DDIMScheduler()
    sch.set_timesteps(50)
    tsl = sch.timesteps.numpy()
    coef = sch.coef_table(tsl[24:25], 0.0)
    tt = int(tsl[24])
    with mock.patch.object(torch.Tensor, "float", torch.Tensor.double):
        pred = ou.unet1d_forward({k: v.double() for k, v in sd_u.items()}, torch.cat([lat] * 2).double(), torch.tensor([tt] * 4), torch.cat([null.repeat(2, T, 1), c]).double())
    e_u, e_c = pred.chunk(2)
    o = osch.OracleDDIM()
    o.set_timesteps(50)
    want = o.step(e_c + GS * (e_c - e_u), tt, lat.double())
    P, sP = R.forward(sd_u, lat.transpose(1, 2), torch.tensor([tt]), c, False, F64, n_clips=2, null=null, six=six)
    got = R.out_sched(sd_u, P, sP, lat, coef[0], GS, False, F64)
    e = rel_max(got, want)
    print(f"guided step, launches chained in float64 vs the oracle in float64: {e:.2e} of max |ref|")
    assert e <= 1e-14


def test_distance_to_the_rounding_oracle_is_reported(sds, inputs):
    """Roundings on: this restatement and oracle/unet.py under ROUND_OPERANDS / ROUND_STORES round at different points (by design: GroupNorm from partials, folded
    LayerNorm affines, fp32 x1 / x2 inside the fused tail, the kernel's online softmax) — reported, not bounded."""
    sd_u, _ = sds["plain"]
    x, ts, c = inputs
    ref = ou.unet1d_forward(sd_u, x, ts, c)
    got = R.forward(sd_u, x.transpose(1, 2), ts, c, True, F64)
    try:
        ou.ROUND_OPERANDS, ou.ROUND_STORES, ou.ATTN_KS = "bf16", True, None
        emu = ou.unet1d_forward(sd_u, x, ts, c)
    finally:
        ou.ROUND_OPERANDS, ou.ROUND_STORES, ou.ATTN_KS = None, False, 4
    rng = float(ref.abs().max())
    rms = lambda d: float(d.double().pow(2).mean().sqrt()) / rng
    print(f"rounded restatement vs the rounding oracle: max {float((got - emu).abs().max()) / rng:.2e} rms {rms(got - emu):.2e} of range; vs the fp32 oracle: restatement rms "
          f"{rms(got - ref):.2e}, rounding oracle rms {rms(emu - ref):.2e}")
    assert torch.isfinite(got).all()


# ---------------------------------------------------------------- draws of stored inputs for the multi-product launches
def draw(sd_u, seed, T=T, n=1, hot=0):
    """Stored inputs of one SpatialTransformer (block seed % 4) from a seeded generator: the block input and the attention output as bf16 values, the input's partials,
    the context's K / V; and q / k / v as the q/k/v launch would store them (hot: to_q / to_k scaled by 2^hot)."""
    g = torch.Generator().manual_seed(seed)
    j = seed % 4
    rn = lambda *s: torch.randn(*s, generator=g)
    xin, o, x1 = round_bf16(rn(n, T, 192) * 1.5), round_bf16(rn(n, T, 192) * 0.7), round_bf16(rn(n, T, 192) * 1.5)
    kv = R.kv_all(sd_u, rn(n, T, 768), F64).float()
    lo = j * 2 * R.MC
    sd2 = sd_u
    if hot:
        sd2 = dict(sd_u)
        for nm in "qk":
            key = R.ST[j] + f".transformer_blocks.0.attn1.to_{nm}.weight"
            sd2[key] = sd_u[key] * 2.0 ** hot
    q, k, v = R.qkv_split(R.finish(R.qkv_parts(sd2, j, xin, R.partials(xin), True, F64, scaled=True), True, False), True, True)
    return dict(j=j, xin=xin, st=R.partials(xin), o=o, x1=x1, kvf=kv.transpose(1, 2)[:, :, lo:lo + 2 * R.MC], kvt=R.kvt(kv)[:, :, lo:lo + 2 * R.MC], q=q.float(), k=k.float(), v=v.float())


def pair(kind, sd_u, d, dt, store=False, rounded=True):
    MC = R.MC
    if kind == "chain":
        return R.chain(sd_u, d["j"], d["o"], d["xin"], d["st"], d["kvt"][:, :, :MC], d["kvt"][:, :, MC:], rounded, dt, store=store)[0]
    if kind == "band":
        return R.q2_band(sd_u, d["j"], d["x1"], d["kvf"][:, :, :MC], d["kvf"][:, :, MC:], rounded, dt, store=store)
    return R.battn(d["q"], d["k"], d["v"], rounded, dt, store=store)


def network_draws(sd_u, seed, T=T, hot=0):
    """The stored inputs of the four SpatialTransformers' multi-product launches as the network itself produces them: one sample of synth latents / context (seeded)
    through the rounded float64 reference (six-launch tail, so that x1 exists in every block); hot: every attn1.to_q / to_k scaled by 2^hot."""
    sd2 = sd_u
    if hot:
        sd2 = dict(sd_u)
        for j in range(4):
            for nm in "qk":
                key = R.ST[j] + f".transformer_blocks.0.attn1.to_{nm}.weight"
                sd2[key] = sd_u[key] * 2.0 ** hot
    x, c, ts = synth.synth_latents(seed, (1, T, 32)), synth.synth_latents(seed + 5000, (1, T, 768)), torch.tensor([(seed * 137 + 11) % 1000])
    tr = []
    R.forward(sd2, x.transpose(1, 2), ts, c, True, F64, six=True, trace=tr)
    tr = dict(tr)
    kv = R.kv_all(sd_u, c, F64).float()
    out = []
    for j, src in enumerate(("res0.conv2", "res1.conv2", "res3.conv2", "res4.conv2")):
        lo = j * 2 * R.MC
        q, k, v = tr[f"st{j}.qkv"]
        xin = tr[src].float()
        out.append(dict(j=j, xin=xin, st=R.partials(xin), o=tr[f"st{j}.attn"].float(), x1=tr[f"st{j}.out1"].float(), kvf=kv.transpose(1, 2)[:, :, lo:lo + 2 * R.MC],
                        kvt=R.kvt(kv)[:, :, lo:lo + 2 * R.MC], q=q.float(), k=k.float(), v=v.float()))
    return out


def measure_caps(sds, ndraws=NDRAWS):
    """{(kind, fill): (cap, largest pre-store |fp32 - float64| of max |ref|)} over ndraws seeded evaluations of the network at T = 70, each giving the four blocks'
    launches; battn_kernel also over ndraws / 8 evaluations at T = 290 and ndraws / 8 with to_q / to_k x 8 (its rebase branch).  A cap is 4 x the largest difference,
    and at most 1e-2 of range: beyond that the fill, not the kernel, is at fault and the rule keeps its largest admissible cap."""
    out = {}
    for fill, (sd_u, _) in sds.items():
        worst = {"chain": 0.0, "band": 0.0, "battn": 0.0}
        for s in range(ndraws + ndraws // 4):
            extra = s - ndraws
            kinds = worst if extra < 0 else ("battn",)
            for d in network_draws(sd_u, 1000 + s, T=290 if extra >= 0 and extra % 2 else T, hot=3 if extra >= 0 and extra % 2 == 0 else 0):
                for kind in kinds:
                    worst[kind] = max(worst[kind], rel_max(pair(kind, sd_u, d, F32), pair(kind, sd_u, d, F64)))
        for kind, w in worst.items():
            out[kind, fill] = (min(4 * w, 1e-2), w)
    return out


def test_caps_are_the_measured_ones(sds):
    got = measure_caps(sds)
    for key, (cap, worst) in sorted(got.items()):
        print(f"cap {key}: largest pre-store |fp32 - float64| {worst:.2e} of range over {NDRAWS} draws -> cap {cap:.2e} (recorded {R.CAPS.get(key, float('nan')):.2e})")
    for key, (cap, worst) in got.items():
        if 4 * worst > 1e-2:
            print(f"cap {key}: 4 x the largest difference is {4 * worst:.2e} > 1e-2 of range — this fill is at fault for this launch kind; the rule keeps 1e-2")
        # the measured maximum is fp32 rounding noise (it moves with the BLAS's summation order): the recorded cap must cover it, stay the rule's <= 1e-2, and not have
        # drifted to more than twice what is measured
        assert key in R.CAPS and cap <= R.CAPS[key] * 1.02 and R.CAPS[key] <= 1e-2 and R.CAPS[key] <= 2 * max(cap, 1e-3), f"{key}: recorded {R.CAPS.get(key)}, measured {cap:.3e}"


# ---------------------------------------------------------------- the mutants
def _factor_single(p64, p32, got):
    """How many times over `got` fails check_bf16_allow (a lower bound: every alternative of the element rule lies inside stored_limit)."""
    st = R.single_stats(got, p64, p32)
    if st["bad"] == 0 and st["share"] >= 0.99:
        return 0.0
    f = _factor(got, st["ref_r"], R.stored_limit(st["bound"] * st["rng"], st["allow"], st["ref_r"]), 0.01)
    return max(f, (1.0 - st["share"]) / 0.01)


def _factor(got, ref_r, lim, share):
    d = (got.double() - ref_r).abs()
    if not torch.isfinite(d).all():
        return math.inf
    el = float((d / torch.maximum(torch.maximum(bf16_step(ref_r), bf16_step(got)), torch.as_tensor(lim, dtype=F64))).max())
    return max(el, float((d != 0).double().mean()) / share)


def _mutant_cases(sds):
    """{mutant: (launch, fn() -> factor by which the mutated launch fails its rule; evaluated with R.MUTANT set for the `got` side only)}."""
    sd, null = sds["plain"]
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g)
    n = 6
    x, m = round_bf16(rn(n, T, 192) * 1.3 + rn(n, 1, 192) * 0.5 * torch.arange(1, n + 1).view(n, 1, 1)), round_bf16(rn(n, T, 192))
    x = x * torch.linspace(0.5, 2.0, n).view(n, 1, 1)   # samples with different statistics: a neighbour's GroupNorm table is a different table
    x = round_bf16(x)
    stx = R.partials(x)
    e_row = rn(n, 192) * 0.1
    part = round_bf16(rn(n, T, 192))

    def single(make):
        def fn():
            mut = R.MUTANT
            R.MUTANT = None
            p64, p32 = make(F64), make(F32)
            R.MUTANT = mut
            got = R.finish(make(F64), True, True)
            R.MUTANT = None
            return _factor_single(p64, p32, got)
        return fn

    conv1 = ("res0 conv 1", single(lambda dt: R.res_conv1_parts(sd, 0, x, stx, e_row, True, dt)))
    c1b = ("res3 conv 1, source 1 + partial sum", single(lambda dt: R.cat_conv1b_parts(sd, 3, x, stx, part, e_row, True, dt)))
    geglu = ("st0 GEGLU", single(lambda dt: R.geglu_parts(sd, 0, x, True, dt)))

    def qkv_v():
        mut = R.MUTANT
        R.MUTANT = None
        mk = lambda dt: R.qkv_parts(sd, 0, x[:2], stx[:2], True, dt, scaled=True)
        p64, p32 = mk(F64), mk(F32)
        q, k, v = R.qkv_split(R.finish(p64, True, False), True, True)
        vp = torch.nn.functional.pad(v, (0, R.rup(T, 32) - T))
        R.MUTANT = mut
        stored = R.v_stored(vp)                      # what the launch would leave in VT
        R.MUTANT = None
        got = R.qkv_join(q, k, R.v_tokens(stored)[:, :, :T])   # ... read back as the GPU test reads it
        return _factor_single(p64, p32, got)

    def multi(kind, cap_key, hot=0, guided=False, T_=T):
        def fn():
            mut = R.MUTANT
            R.MUTANT = None
            d = draw(sd, 2001, T=T_, n=2, hot=hot)
            if guided:
                call = lambda: R.chain(sd, d["j"], d["o"], d["xin"], d["st"], d["kvt"][:, :, :R.MC], d["kvt"][:, :, R.MC:], True, F64, n_uncond=1, null=null)[0]
            else:
                call = lambda: pair(kind, sd, d, F64, store=True)
            ref = call()
            R.MUTANT = mut
            got = call()
            R.MUTANT = None
            f = _factor(got, ref, R.CAPS[cap_key] * float(ref.abs().max()), 0.03)
            if kind == "battn" and math.isfinite(f):   # check_attention: rms <= 0.1 rms(unrounded - rounded)
                noise = float((pair(kind, sd, d, F64, store=True, rounded=False) - ref).pow(2).mean().sqrt())
                f = max(f, float((got - ref).pow(2).mean().sqrt()) / (0.1 * noise))
            return f
        return fn

    return {
        "tap_shifted": conv1, "k_dropped": conv1, "gn_neighbour_sample": conv1, "gn_ring_wrapped": conv1, "gn_over_pitch": conv1,
        "v_permutation_undone": ("st0 q/k/v, v as stored", qkv_v),
        "last_key_tile_unmasked": ("battn_kernel", multi("battn", ("battn", "plain"))),
        "rebase_skipped": ("battn_kernel, to_q / to_k x 2^6", multi("battn", ("battn", "plain"), hot=6, T_=290)),
        "band_off_by_one": ("stchain_kernel<bf16>", multi("chain", ("chain", "plain"))),
        "geglu_swapped": geglu, "partial_sum_dropped": c1b,
        "c2_on_conditional_half": ("stchain_kernel<bf16>, guided", multi("chain", ("chain", "plain"), guided=True)),
    }


def test_every_mutant_fails_its_rule_tenfold(sds):
    cases = _mutant_cases(sds)
    assert set(cases) == set(R.MUTANTS)
    worst = math.inf
    for name in R.MUTANTS:
        launch, fn = cases[name]
        assert R.MUTANT is None
        try:
            R.MUTANT = name
            f = fn()
        finally:
            R.MUTANT = None
        print(f"mutant {name:26s} on {launch:40s}: fails its rule {f:.3g} x")
        worst = min(worst, f)
        assert f >= 10, f"{name}: fails the rule of {launch} only {f:.2f} x"
    print(f"smallest factor {worst:.3g}")
