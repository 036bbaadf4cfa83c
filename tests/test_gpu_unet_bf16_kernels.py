"""The token-major bf16 denoise step kernel by kernel at toy shapes (run on the MI355X with `-m gpu`).

bf16 mode, with said_debug_option "unet_tgemm_min_tokens" = 0 so that toy batches take the large-batch (token-major) schedule, is stopped behind every launch
(said_debug_stop_after); the launch's inputs and outputs are read back AS STORED (Engine.ws_buffers / ws_snapshot: the token-major bf16 activations tH0 tH1 tP tQ tM tX1
tX2 tO tF, their producers' GroupNorm partials stH0 ..., QK VT KVT KV EO) and the output is compared with tests/unet_bf16_ref.py's float64 evaluation of those inputs
over ALL samples, channels and tokens [0, T).  tests/test_unet_bf16_ref_cpu.py ties that restatement to the oracle and shows that twelve ways of being wrong fail the
rules below at least ten times over.  The rules are unet_bf16_ref.py's (its docstring): layout-only stores exact; single products check_bf16_allow / check_f32_allow
(>= 99 % bit-equal, one bf16 step or 4 max(e32, 1e-6) of range + the flip allowance where the kernel transforms its operand); the fused tail, the q projection + band
and attention check_multi (>= 97 % bit-equal, every element within max(one bf16 step, the CPU-measured cap)), attention also check_attention; GroupNorm partials through
the normalised tensor they imply (check_f32).  A buffer read again at a later stop must be bit-equal to what the earlier stop saw.  Plans are asserted from the stage
log (kinds 11 conv_in_kernel, 7 rgemm_kernel, 6 xgemm_kernel, 9 battn_kernel, 1 attn_kernel, 10 stchain_kernel, 12 the out convolution), from the counters n_rgemm,
n_xgemm, n_stchain, n_out_sched_tm and from graph_num_nodes(); which rgemm variant and tile walk a launch takes is held on the CPU by tests/test_rgemm_plan_cpu.py.

Shapes (each the smallest that reaches what it is named for):
  S        forward, 3 x 70 (a sample's last tile 6 tokens): every launch — the generic conv_in and its transposing launch (forward() has no clips to share a
           conv_in_kernel<TM> result among: that kernel is G's), 2 + 2 + 2 + 4 + 4 ResBlock launches, three x (q/k/v, battn, fused tail), the
           last block as q/k/v, battn and five tail launches ending in the channel-major xgemm_kernel, the out convolution; 33 launches.  Also on trained-like weights.
  G, G-eta one guided loop step, 2 clips x 70 (Be 4): conv_in with two copies, the duplicate-store convolution, the shared first block, the unconditional half skipping
           the cross-attention, out_sched_tm_kernel<CFG> (G-eta: eta = 1 noise and a mask crossing token 64); 28 graph nodes.
  T6       S and G with st_chain_bf16 = 0: rgemm's six-launch tail, with to_out + the c2 duplicate and the proj_out pair.
  A        forward, the first block's q/k/v and attention only, 2 x T for T = 20 (one key tile, masked), 290 (10 query tiles: a second workgroup per head with two live
           waves), 608 (the largest LDS image under the old cap), 640 (the largest supported: 82,432 bytes of LDS).
  P, Z     forward with the six-launch tail at 260 x 40 and 1300 x 20: rgemm_kernel's persistent tile walk (three tiles per range with ranges starting mid-sample; six
           one-tile samples per range, which wraps the four-slot ring of GroupNorm tables), over all samples: at P conv_in, res0's convolutions, the first q/k/v, the first
           attn1.to_out, res3's four launches; at Z conv_in, res0's first convolution and the first attn1.to_out (the float64 reference is the cost).
  A-hot    as A at T = 290 with attn1's to_q / to_k scaled by a power of two chosen on the CPU so that >= 1 % of the (sample, head, query) rows move their reference.
Pad tokens are never compared: instead the forward pass (S, T6, A at 640) and the guided step (G-eta) run from a workspace of 0x00, 0xFF and 0x7F bytes and must be
finite and bit-identical.  Not built: X (the T > 640 route: fp32 q/k/v + attn_kernel<.., QW = 4> on bf16 operands) and W (windows wider than 8: the band launch off rgemm_kernel).

Measured (MI355X; bit-equal share of the stored bf16 values beside the fp32 CPU evaluation's own share; differences of max |ref|):
  single products   conv_in_kernel<TM> 99.981 % (99.985); ResBlock convolutions 99.72 ... 100 % (99.71 ... 99.998); partial sums of the concatenated ones 99.65 ... 99.99 %;
                    1x1 skip 99.98 ... 99.998 %; q/k/v 99.86 ... 99.995 % (T = 20: 99.097 % beside 99.076 %); to_out + GroupNorm'ed residual, attn2.to_out 99.99 %; GEGLU
                    99.98 %; the proj_out pair 99.99 %; largest flip allowance 1.27e-3 of range (trained-like 5.9e-3), 3 ... 7 % of the operands ambiguous (trained-like to 45 %).
  multi-product     stchain_kernel<bf16> 98.92 ... 99.88 % (trained-like 99.37 ... 99.78 %), largest difference 4.1e-3 (cap 4.9e-3; trained-like 4.8e-4, cap 1e-2); q projection +
                    band 99.99 % (5.7e-4, cap 2.7e-3); battn_kernel 99.97 ... 100 %, rms 0 ... 8.7e-5 beside 5e-4 ... 4.8e-3 for the unrounded evaluation; T = 608 / 640: 99.981 /
                    99.984 %, rms 6.5e-6 / 1.4e-5; A-hot (to_q / to_k x 4): 44.91 % of the rows rebase on the stored q and k, 99.999 %, rms 2.9e-9.
  fp32 stores       generic conv_in 1.8e-7; channel-major folded proj_out 7.6e-8; out convolution 1.6e-4 inside its allowance; GroupNorm from the partials 1.1e-8 ... 5.0e-8.
  out_sched_tm      G / G-eta max 6.6e-7 / 6.3e-7, 100 % within 2e-5; T6-G max 2.7e-4, 98.95 % within 2e-5; masked elements exact.
  GEGLU's floor is asked of the elements with Phi(gate) >= 1 / 128 (99.1 ... 99.2 % of them on the plain fill: 99.93 ... 99.99 % bit-equal).  Trained-like fill: 82.15 % of
                    the elements, 99.989 % bit-equal (fp32 CPU evaluation 99.966 %); over ALL elements the kernel is 95.97 % bit-equal and the fp32 CPU evaluation 95.19 %; no element out.
  the q/k/v launch at 2 x 290 has three elements (of 334,080, one token) two bf16 steps from the rounded reference and 0.87 ... 0.96 of fp32 bound + allowance from the
                    unrounded one: inside single_stats' rule by its last alternative alone.
  P / Z (all samples): convolutions 99.93 ... 99.97 % / 99.947 %, q/k/v 99.965 %, to_out 99.99 / 99.994 %, no element out; partials <= 8.4e-8.
  exact: KVT, the transposing launch, conv_in's second copy, duplicate stores, x2 = x1 + c2, V's pad zeros, masked elements; every fill finite and bit-identical.
pytest --durations: A-hot 0.9 s, T6-G 0.8 s, S / S trained-like 0.7 / 0.9 s, T6 0.7 s, G / G-eta 0.7 s, P 2.2 s with eight of its ten launches (with ten: below the 2.5 s of the whole suite's 25th slowest test), Z 2.9 ... 3.3 s, A 0.4 ... 0.5 s each, fills <= 0.45 s (the module's model 0.5 s once).
"""
import numpy as np
import pytest
import torch

import unet_bf16_ref as R
import unet_f32_ref as R32
from audio_bf16_ref import check_attention, check_exact, check_f32, round_bf16
from oracle import pipeline as op
from said_amd.util import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
F64, F32 = torch.float64, torch.float32
MC = R.MC
GS = 2.0
TM_OPTS = {"unet_tgemm_min_tokens": 0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _model(dev, sd):
    from said_amd.model.diffusion import SAID_UNet1D
    from said_amd.model.wav2vec2 import AudioConfig
    m = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=1))
    m.load_state_dict(sd, strict=True)
    m.to(dev).eval()
    m.set_mfma_dtype("bf16")
    return m


@pytest.fixture(scope="module")
def plain(dev):
    sd = synth.said_state_dict(num_w2v_layers=1)
    _, sd_u, null = op.split_state_dict(sd)
    return _model(dev, sd), sd_u, null


class Options:
    """said_debug_option settings for the length of a with block; every one goes back to -1."""

    def __init__(self, eng, opts):
        self.eng, self.opts = eng, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.eng.debug_option(k, v)

    def __exit__(self, *exc):
        self.eng.debug_stop_after(-1)
        for k in self.opts:
            self.eng.debug_option(k, -1)


# ---------------------------------------------------------------- the schedule (unet_sched.cpp run_unet on token-major activations) and what each launch reads and writes
def _schedule(guided, six):
    # forward(): the latents are per sample — the generic channel-major convolution (fp32 products) and a transposing launch; the loop: conv_in_kernel<TM>, once per clip
    L = [("conv_in",)] if guided else [("conv_in_cm",), ("prep",)]

    def res(i, in0, out, shared=False):
        L.append(("conv1", i, in0, shared))
        L.append(("conv2", i, in0, out, shared))

    def res_cat(i, in0, in1, out):
        L.extend([("c1a", i, in0), ("c1b", i, in1), ("skip", i, in0, in1), ("c2", i, out)])

    def st(j, inn, out, shared=False, last=False):
        L.extend([("qkv", j, inn, shared), ("attn", j, shared)])
        if not six and not (last and not guided):
            L.append(("chain", j, inn, out, shared))
            return
        L.extend([("out1", j, inn, shared), ("band", j, shared), ("out2", j, shared), ("geglu", j)])
        L.extend([("proj_cm", j, inn)] if last and not guided else [("proj_h", j, inn), ("proj_x", j, out)])

    res(0, "H0", "P", guided); st(0, "P", "H1", guided)
    res(1, "H1", "P"); st(1, "P", "Q")
    res(2, "Q", "P")
    res_cat(3, "P", "H1", "Q"); st(2, "Q", "P")
    res_cat(4, "P", "H0", "Q"); st(3, "Q", "P", last=True)
    L.append(("out_sched",) if guided else ("out",))
    return L


def _io(la):
    """(buffers read, buffers written) of a launch, by workspace name."""
    k = la[0]
    t = lambda n: "t" + n
    if k == "conv_in":
        return ["x"], ["tH0", "stH0"]
    if k == "conv_in_cm":
        return ["x"], ["H0", "stH0"]
    if k == "prep":
        return ["H0"], ["tH0"]
    if k == "conv1":
        return [t(la[2]), "st" + la[2], "EO"], ["tM", "stM"]
    if k == "conv2":
        return ["tM", "stM", t(la[2])], [t(la[3]), "st" + la[3]]
    if k == "c1a":
        return [t(la[2]), "st" + la[2]], ["tX1"]
    if k == "c1b":
        return [t(la[2]), "st" + la[2], "tX1", "EO"], ["tM", "stM"]
    if k == "skip":
        return [t(la[2]), t(la[3])], ["tX1"]
    if k == "c2":
        return ["tM", "stM", "tX1"], [t(la[2]), "st" + la[2]]
    if k == "qkv":
        return [t(la[2]), "st" + la[2]], ["QK", "VT"]
    if k == "attn":
        return ["QK", "VT"], ["tO"]
    if k == "chain":
        return ["tO", t(la[2]), "st" + la[2], "KVT"], [t(la[3]), "st" + la[3]]
    if k == "out1":
        return ["tO", t(la[2]), "st" + la[2]], ["tX1", "tX2"]
    if k == "band":
        return ["tX1", "KV"], ["tO"]
    if k == "out2":
        return ["tO", "tX1"], ["tX2"]
    if k == "geglu":
        return ["tX2"], ["tF"]
    if k == "proj_cm":
        return ["tF", "tX2", t(la[2])], ["P", "stP"]
    if k == "proj_h":
        return ["tF", t(la[2])], ["tX1"]
    if k == "proj_x":
        return ["tX2", "tX1"], [t(la[2]), "st" + la[2]]
    if k == "out":
        return ["P", "stP"], ["eps"]
    return ["tP", "stP"], []   # out_sched: its output is the loop's result


KIND = {"conv_in": 11, "conv_in_cm": 0, "prep": 5, "attn": 9, "chain": 10, "proj_cm": 6, "out": 12}   # everything else: 7, rgemm_kernel


def _kinds(sched):
    return [KIND.get(la[0], 7) for la in sched if la[0] != "out_sched"]


class Stops:
    """One shape's stopped runs: `run` makes the call (forward pass or loop step), stop(k, launch) makes it with the first k launches and reads the launch's buffers."""

    def __init__(self, eng, Be, T, S, run):
        self.eng, self.Be, self.T, self.S, self.run = eng, Be, T, S, run
        self.Tp, self.Sp, self.np, self.seg = R.rup(T, 32), R.rup(S, 32), (T + 31) // 32, R.rup(T, 64)
        self.sizes = {nm: nb for _, nm, nb in eng.ws_buffers()}
        self.index = {nm: i for i, nm, _ in eng.ws_buffers()}
        self.cur = {}
        self.written = set()

    def raw(self, name, nbytes, dtype):
        assert nbytes <= self.sizes[name], (name, nbytes, self.sizes[name])
        t = self.eng.ws_snapshot(self.index[name], nbytes)
        torch.cuda.synchronize()
        return t.cpu().view(dtype)

    def bf(self, name, shape):
        return self.raw(name, 2 * int(np.prod(shape)), torch.bfloat16).view(shape).float()

    def f32(self, name, shape):
        return self.raw(name, 4 * int(np.prod(shape)), torch.float32).view(shape)

    def read(self, name):
        """The buffer as stored (bf16 values as fp32 numbers), pad tokens removed."""
        Be, T, Tp, seg = self.Be, self.T, self.Tp, self.seg
        if name in ("tH0", "tH1", "tP", "tQ", "tM", "tX1", "tX2", "tO"):
            return self.bf(name, (Be, seg, MC))[:, :T].clone()
        if name == "tF":
            return self.bf(name, (Be, seg, R.FFI))[:, :T].clone()
        if name.startswith("st"):
            return self.f32(name, (Be, self.np, MC, 2)).clone()
        if name == "QK":
            return self.bf(name, (Be, 12, Tp, 32))[:, :, :T].clone()
        if name == "VT":   # stored token-permuted per 16; the pad tokens of a sample's last tile are the zeros battn_kernel relies on
            v = self.bf(name, (Be, MC, Tp))
            return R.v_tokens(v)
        if name in ("P", "H0"):
            return self.f32(name, (Be, MC, Tp))[:, :, :T].transpose(1, 2).clone()
        if name in ("x", "eps"):
            return self.f32(name, (Be, 32, Tp))[:, :, :T].clone()
        if name == "EO":
            n = self.sizes["EO"] // 4
            return self.f32(name, (5, MC, n // (5 * MC)))[:, :, :max(Be, 1)].clone()
        if name == "KV":
            return self.f32(name, (Be, R.NST * 2 * MC, self.Sp))[:, :, :self.S].clone()
        if name == "KVT":
            return self.bf(name, (Be, self.S, R.NST * 2 * MC)).clone()
        raise KeyError(name)

    def stop(self, k, launch):
        """Runs the first k launches; re-reads the launch's inputs (bit-equal to what an earlier stop saw, unless nothing read or wrote them before) and reads its outputs."""
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


def _cm(y):
    return y.transpose(1, 2)


def _partials(tag, y, st, rec):
    """The normalised tensor the stored partials imply for y (B, T, 192) against its float64 GroupNorm (32 groups of 6 channels, eps 1e-5)."""
    got = R32.norm_from_partials(_cm(y), st)
    rec.append((tag + " partials", check_f32(f"{tag}: GroupNorm from the stored partials", got, R32.group_norm(_cm(y), 32, None, None, 1e-5, F64),
                                                 R32.group_norm(_cm(y), 32, None, None, 1e-5, F32))[0], 1.0))


def _single(tag, name, got, fn, rec, f32=False):
    """A single-product launch: fn(dtype) -> Parts of its stored inputs."""
    p64, p32 = fn(F64), fn(F32)
    if f32:
        allow, _ = R.flip_allowance(p64, p32)
        e, _ = R.check_f32_allow(f"{tag} {name}", got, R.finish(p64, True, True, bf16=False), R.finish(p32, True, True, bf16=False), allow)
        rec.append((name, e, 1.0))
    else:
        share, d, _ = R.check_bf16_allow(f"{tag} {name}", got, p64, p32)
        rec.append((name, d, share))


def _check_launch(tag, sd, null, la, c, Be, Bc, fill, rec, T):
    """One launch on its own stored inputs.  c: buffer name -> tensor as stored; Bc > 0: the guided step's sample layout (unconditional half first)."""
    k = la[0]
    shared = bool(la[-1]) if k in ("conv1", "conv2", "qkv", "attn", "chain", "out1", "band", "out2") else False
    n1 = Bc if shared else Be                        # samples through the self-attention
    x_off = Bc if (Bc and not shared) else 0           # first sample of the cross-attention range in tX1 / tO
    e_row = lambda i, n: c["EO"][i][:, :1].t().expand(n, -1) if Bc else c["EO"][i][:, :n].t()
    t = lambda n: c["t" + n]
    if k == "conv_in":
        x = c["x"][:Bc] if Bc else c["x"]
        nb = x.shape[0]
        _single(tag, "conv_in_kernel<TM>", c["tH0"][:nb], lambda dt: R.conv_in_parts(sd, x, True, dt), rec)
        pre = R.finish(R.conv_in_parts(sd, x, True, F64), True, False).float()   # the partials are those of the fp32 values
        _partials(f"{tag} conv_in", pre, c["stH0"][:nb], rec)
        if Bc:
            check_exact(f"{tag} conv_in: the second copy", c["tH0"][Bc:], c["tH0"][:Bc])
            assert torch.equal(c["stH0"][Bc:], c["stH0"][:Bc])
    elif k == "conv_in_cm":
        _single(tag, "conv_in (generic kernel, fp32 products)", c["H0"], lambda dt: R.conv_in_parts(sd, c["x"], True, dt), rec, f32=True)
        _partials(f"{tag} conv_in", c["H0"], c["stH0"], rec)
    elif k == "prep":
        check_exact(f"{tag} prep_kernel: H0 token-major in bf16", c["tH0"], round_bf16(c["H0"]))
    elif k == "conv1":
        _, i, in0, _ = la
        _single(tag, f"res{i} conv 1", c["tM"][:n1], lambda dt: R.res_conv1_parts(sd, i, t(in0)[:n1], c["st" + in0][:n1], e_row(i, n1), True, dt), rec)
        _partials(f"{tag} res{i} conv 1", c["tM"][:n1], c["stM"][:n1], rec)
    elif k == "conv2":
        _, i, in0, out, _ = la
        _single(tag, f"res{i} conv 2 + x", t(out)[:n1], lambda dt: R.res_conv2_parts(sd, i, c["tM"][:n1], c["stM"][:n1], t(in0)[:n1], True, dt), rec)
        _partials(f"{tag} res{i} conv 2", t(out)[:n1], c["st" + out][:n1], rec)
        if shared:
            check_exact(f"{tag} res{i} conv 2: the duplicate store", t(out)[Bc:], t(out)[:Bc])
    elif k == "c1a":
        _, i, in0 = la
        _single(tag, f"res{i} conv 1, source 0 -> partial sum", c["tX1"], lambda dt: R.cat_conv1a_parts(sd, i, t(in0), c["st" + in0], True, dt), rec)
    elif k == "c1b":
        _, i, in1 = la
        _single(tag, f"res{i} conv 1, source 1 + partial sum", c["tM"], lambda dt: R.cat_conv1b_parts(sd, i, t(in1), c["st" + in1], c["tX1"], e_row(i, Be), True, dt), rec)
        _partials(f"{tag} res{i} conv 1", c["tM"], c["stM"], rec)
    elif k == "skip":
        _, i, in0, in1 = la
        _single(tag, f"res{i} 1x1 skip (two chunks)", c["tX1"], lambda dt: R.cat_skip_parts(sd, i, t(in0), t(in1), True, dt), rec)
    elif k == "c2":
        _, i, out = la
        _single(tag, f"res{i} conv 2 + skip", t(out), lambda dt: R.cat_conv2_parts(sd, i, c["tM"], c["stM"], c["tX1"], True, dt), rec)
        _partials(f"{tag} res{i} conv 2", t(out), c["st" + out], rec)
    elif k == "qkv":
        _, j, inn, _ = la
        v_all = c["VT"]
        assert int(v_all[:n1, :, T:].abs().view(torch.int32).sum()) == 0, f"{tag} st{j}: V's pad tokens are not the zeros battn_kernel multiplies its masked probabilities with"
        c["q"], c["k"], c["v"] = c["QK"][:n1, :6], c["QK"][:n1, 6:], v_all[:n1, :, :T]
        _single(tag, f"st{j} q/k/v", R.qkv_join(c["q"], c["k"], c["v"]), lambda dt: R.qkv_parts(sd, j, t(inn)[:n1], c["st" + inn][:n1], True, dt, scaled=True), rec)
    elif k == "attn":
        _, j, _ = la
        _attention(f"{tag} st{j} battn_kernel", c["tO"][:n1], c["q"], c["k"], c["v"], rec, fill)
    elif k == "chain":
        _, j, inn, out, _ = la
        lo = j * 2 * MC
        kvt = c["KVT"].clone()
        kvt[:Bc] = 0   # (the unconditional half's rows are never written, and never read)
        ref, _ = R.chain(sd, j, c["tO"][:n1], t(inn)[:n1], c["st" + inn][:n1], kvt[:, :, lo:lo + MC], kvt[:, :, lo + MC:lo + 2 * MC], True, F64, nsamp=Be,
                         in_mod=Bc if shared else 0, n_uncond=Bc, null=null)
        share, d = R.check_multi(f"{tag} st{j} stchain_kernel<bf16>", t(out), ref, R.CAPS["chain", fill])
        rec.append((f"st{j} chain", d, share))
        _partials(f"{tag} st{j} chain", t(out), c["st" + out], rec)
    elif k == "out1":
        _, j, inn, _ = la
        _single(tag, f"st{j} attn1.to_out + GroupNorm(x_in)", c["tX1"][:n1], lambda dt: R.out1_parts(sd, j, c["tO"][:n1], t(inn)[:n1], c["st" + inn][:n1], True, dt), rec)
        if Bc:
            check_exact(f"{tag} st{j} to_out: the unconditional half's x2 = x1 + c2", c["tX2"][:n1], R.out1_dup(sd, j, c["tX1"][:n1], null))
    elif k == "band":
        _, j, _ = la
        lo = j * 2 * MC
        kv = c["KV"].transpose(1, 2)[Bc:]
        n2 = Be - Bc
        ref = R.q2_band(sd, j, c["tX1"][x_off:x_off + n2], kv[:, :, lo:lo + MC], kv[:, :, lo + MC:lo + 2 * MC])
        share, d = R.check_multi(f"{tag} st{j} q projection + band", c["tO"][x_off:x_off + n2], ref, R.CAPS["band", fill])
        rec.append((f"st{j} band", d, share))
    elif k == "out2":
        _, j, _ = la
        n2 = Be - Bc
        _single(tag, f"st{j} attn2.to_out + x1", c["tX2"][Bc:], lambda dt: R.out2_parts(sd, j, c["tO"][x_off:x_off + n2], c["tX1"][x_off:x_off + n2], True, dt), rec)
    elif k == "geglu":
        _, j = la
        # (the bit-equal floor is asked of the elements whose gate leaves gelu relative accuracy in fp32: geglu_parts' floor_mask; the element bound of all)
        _single(tag, f"st{j} GEGLU", c["tF"], lambda dt: R.geglu_parts(sd, j, c["tX2"], True, dt), rec)
    elif k == "proj_cm":
        _, j, inn = la
        _single(tag, f"st{j} folded proj_out, channel-major (xgemm_kernel)", c["P"], lambda dt: R.proj_out_cm_parts(sd, j, c["tF"], c["tX2"], t(inn), True, dt), rec, f32=True)
        _partials(f"{tag} st{j} proj_out", c["P"], c["stP"], rec)
    elif k == "proj_h":
        _, j, inn = la
        _single(tag, f"st{j} folded proj_out, h's four chunks + x_in -> partial sum", c["tX1"], lambda dt: R.proj_h_parts(sd, j, c["tF"], t(inn), True, dt), rec)
    elif k == "proj_x":
        _, j, out = la
        _single(tag, f"st{j} folded proj_out, x2 + partial sum", t(out), lambda dt: R.proj_x_parts(sd, j, c["tX2"], c["tX1"], True, dt), rec)
        _partials(f"{tag} st{j} proj_out", t(out), c["st" + out], rec)
    elif k == "out":
        _single(tag, "out convolution", c["eps"].transpose(1, 2), lambda dt: R.out_conv_parts(sd, c["P"], c["stP"], True, dt), rec, f32=True)
    else:
        raise KeyError(k)


def _attention(name, got, q, k, v, rec, fill):
    """battn_kernel on its stored q / k / v: check_multi against the restated online softmax, check_attention against the unrounded evaluation."""
    T = q.shape[2]
    st = {}
    ref = R.battn(q, k, v, True, F64, stats=st)
    ref_u = R.battn(q, k, v, False, F64)
    share, d = R.check_multi(name, got, ref, R.CAPS["battn", fill])
    check_attention(name, got, ref, ref_u)
    print(f"{name}: T = {T}, {100 * st['rebased']:.2f} % of the rows moved their reference after the first key tile")
    rec.append((name.split(" ", 1)[1], d, share))
    return st["rebased"]


def _kv_checks(tag, s, b0, six=False):
    """KVT (bf16 key-major copy) against KV; KV itself is an input here (its launch is not one of the step's).  The copy is made for the fused tail alone."""
    if six:
        return
    kv, kvt = s.read("KV"), s.read("KVT")
    check_exact(f"{tag} KVT (bf16 key-major copy) against KV", kvt[b0:], round_bf16(kv[b0:].transpose(1, 2)))


def _summary(tag, rec):
    worst = min(r[2] for r in rec)
    print(f"{tag}: {len(rec)} comparisons; smallest bit-equal share {100 * worst:.3f} %; largest difference {max(r[1] for r in rec):.2e} of range")
    for r in rec:
        print(f"    {tag} | {r[0]:60s} {r[1]:.2e} {r[2]:.5f}")


# ---------------------------------------------------------------- forward shapes
def _inputs(B, T, seed, S=None):
    return synth.synth_latents(seed, (B, T, 32)), synth.synth_latents(seed + 1, (B, T if S is None else S, 768)), (torch.arange(B) * 137 + 500) % 1000


def _forward_case(model, sd, dev, tag, B, T, seed, six=False, fill="plain", only=None):
    """only: (first, last) launch numbers to check (the rest of the schedule is not run)."""
    x, ctx, ts = _inputs(B, T, seed)
    eng = model._get_engine(max(B, 2), max(T, 64))
    xd, cd = x.to(dev), ctx.to(dev)
    out = {}

    def run():
        out["y"] = eng.unet_forward(xd, ts, cd)
        torch.cuda.synchronize()

    sched = _schedule(False, six)
    rec = []
    opts = dict(TM_OPTS, **({"st_chain_bf16": 0} if six else {}))
    with Options(eng, opts):
        s = Stops(eng, B, T, T, run)
        n0 = {n: eng.debug_get(n) for n in ("n_rgemm", "n_xgemm", "n_stchain")}
        for k, la in enumerate(sched, 1):
            if only and k > only[1]:
                break
            c = s.stop(k, la)
            if k == 1:
                check_exact(f"{tag} x (channel-major latents)", c["x"], x.transpose(1, 2))
                _kv_checks(tag, s, 0, six)
            if not only or k >= only[0]:
                _check_launch(tag, sd, None, la, c, B, 0, fill, rec, T)
        if only:   # (the launches checked are the ones named: the stage log of the whole schedule says which kernels they are)
            eng.debug_stop_after(-1)
            log = [d["kind"] for d in eng.profile_unet(B, T, reps=1)]
            assert [log[k - 1] for k in range(only[0], only[1] + 1)] == [KIND.get(sched[k - 1][0], 7) for k in range(only[0], only[1] + 1)], log
            return s, rec
        # stop k issues the first k launches again
        prefix = lambda kinds: sum(1 for k in range(1, len(sched) + 1) for la in sched[:k] if KIND.get(la[0], 7) in kinds)
        assert eng.debug_get("n_rgemm") - n0["n_rgemm"] == prefix({7}) and eng.debug_get("n_stchain") - n0["n_stchain"] == prefix({10})
        assert eng.debug_get("n_xgemm") > n0["n_xgemm"], "the last block ends on xgemm_kernel"
        eng.debug_stop_after(-1)
        run()
        check_exact(f"{tag} the unstopped call's result against the last stop's eps", out["y"].cpu().transpose(1, 2), s.cur["eps"])
        for name in ("P", "stP", "KV") + (() if six else ("KVT",)):
            assert torch.equal(s.read(name).view(torch.int32), s.cur[name].view(torch.int32)), name
        log = [d["kind"] for d in eng.profile_unet(B, T, reps=1)]
    print(f"{tag}: stage log {log}")
    assert log == _kinds(sched), f"{tag}: the launches are not the ones this shape is here for"
    _summary(tag, rec)


def test_forward_launches_on_their_own_inputs(plain, dev):
    """Shape S: every launch of the forward pass, all samples."""
    model, sd, _ = plain
    assert len(_schedule(False, False)) == 33
    _forward_case(model, sd, dev, "S", 3, 70, 503)


def test_forward_launches_on_trained_like_weights(dev):
    """Shape S on synth.trained_like_state_dict (heavy tails, outlier channels, norm gains up to 10)."""
    full = synth.trained_like_state_dict(num_w2v_layers=1)
    _, sd_u, _ = op.split_state_dict(full)
    _forward_case(_model(dev, full), sd_u, dev, "S trained-like", 3, 70, 531, fill="trained")


def test_forward_launches_with_the_six_launch_tail(plain, dev):
    """Shape T6 (forward): st_chain_bf16 = 0, the production route whenever a token tile's windows do not fit the fused kernel — to_out + GroupNorm'ed residual, the band,
    attn2.to_out, GEGLU and the proj_out pair over column ranges with its bf16 partial sum."""
    model, sd, _ = plain
    assert len(_schedule(False, True)) == 48
    _forward_case(model, sd, dev, "T6", 3, 70, 541, six=True)


# ---------------------------------------------------------------- the persistent tile walk of rgemm_kernel
# launch numbers of the six-launch schedule: conv_in + transposition, res0's two convolutions, st0's q/k/v, (attention runs unchecked,) st0's to_out, res3's four launches.
# The float64 reference of ALL samples is the cost (a convolution at Z: 26,000 tokens x 192 x 576 with its fp32 twin and allowance), so at Z the launches are cut, not the
# samples: it keeps the two table rings — conv 1 (the source's) and to_out (the residual's); P checks all ten
WALK_NAMES = {1: "conv_in_cm", 2: "prep", 3: "conv1", 4: "conv2", 5: "qkv", 7: "out1", 25: "c1a", 26: "c1b", 27: "skip", 28: "c2"}
WALK_LAUNCHES = {"P": (1, 2, 3, 4, 5, 7, 25, 26, 27, 28), "Z": (1, 2, 3, 7)}


@pytest.mark.parametrize("tag,B,T", [("P", 260, 40), ("Z", 1300, 20)])
def test_tile_walk_over_many_samples(plain, dev, tag, B, T):
    """Shapes P and Z with the six-launch tail: rgemm_kernel's ranges of `per` = 3 tiles over two-tile samples (ranges starting mid-sample, a new sample's GroupNorm tables
    made inside the loop) and of `per` = 6 one-tile samples (the four-slot table ring wraps) — tests/test_rgemm_plan_cpu.py holds those figures.  Checked launches
    (WALK_LAUNCHES), over all samples: at P conv_in, the first ResBlock's convolutions, the first q/k/v, the first attn1.to_out, and the first concatenated-input
    ResBlock's four launches; at Z conv_in, the first convolution (the source's table ring) and the first attn1.to_out (the residual's); the rest of the schedule
    runs on the GPU and is not re-evaluated."""
    model, sd, _ = plain
    sched = _schedule(False, True)
    launches = WALK_LAUNCHES[tag]
    assert all(sched[k - 1][0] == WALK_NAMES[k] for k in launches) and sched[24][1] == 3
    ntv = (T + 31) // 32
    per = -(-B * ntv // 256)
    assert per == {"P": 3, "Z": 6}[tag]
    x, ctx, ts = _inputs(B, T, 600 + B)
    eng = model._get_engine(B, max(T, 64))
    xd, cd = x.to(dev), ctx.to(dev)

    def run():
        eng.unet_forward(xd, ts, cd)
        torch.cuda.synchronize()

    rec = []
    with Options(eng, dict(TM_OPTS, st_chain_bf16=0)):
        s = Stops(eng, B, T, T, run)
        n0 = eng.debug_get("n_rgemm")
        for n, k in enumerate(launches):
            la = sched[k - 1]
            if n and k != launches[n - 1] + 1:
                s.cur.clear()   # (launches in between rewrote the buffers: nothing an earlier stop saw is still there)
            c = s.stop(k, la)
            _check_launch(tag, sd, None, la, c, B, 0, "plain", rec, T)
        assert eng.debug_get("n_rgemm") - n0 == sum(sum(1 for la in sched[:k] if KIND.get(la[0], 7) == 7) for k in launches)
        eng.debug_stop_after(-1)
        log = [d["kind"] for d in eng.profile_unet(B, T, reps=1)]
    assert log == _kinds(sched), f"{tag}: the launches are not the ones this shape is here for"
    _summary(tag, rec)


# ---------------------------------------------------------------- attention shapes
@pytest.mark.parametrize("T", [20, 290, 608, 640])
def test_attention_shapes(plain, dev, T):
    """Shape A: the first block's q/k/v (launch 5) and battn_kernel (launch 6) at 2 x T."""
    model, sd, _ = plain
    nkt = (T + 31) // 32                                     # key tiles = query tiles; battn_kernel: eight query tiles (waves) per workgroup
    lds = lambda t: (4 * R.rup(t, 32) + 32 * 81) * 16          # attn.hip battn_lds_bytes
    reaches = {20: nkt == 1 and T % 32 != 0,                                         # the masked last key tile is also the first
               290: (nkt + 7) // 8 == 2 and nkt - 8 == 2 and T % 32 != 0,               # a second workgroup per head with two live waves and six that only copy
               608: T % 32 == 0 and lds(T) == 80384 <= 81920 < lds(T + 1),              # the largest image under the old maximum, no masked tile
               640: lds(T) == 82432 and lds(T) > 81920 and T % 32 == 0}[T]              # the largest supported: beyond the old maximum
    assert reaches, f"T = {T} does not reach what it is here for"
    s, rec = _forward_case(model, sd, dev, f"A T={T}", 2, T, 560 + T, only=(5, 6))
    assert s.sizes["QK"] >= 2 * 12 * R.rup(T, 32) * 32 * 2
    _summary(f"A T={T}", rec)


def _hot_power(sd, x, ts, ctx, want=0.01):
    """The smallest power of two for attn1.to_q / to_k of the first block at which, by the reference's restatement of the kernel's rule, at least `want` of the rows move
    their reference after the first key tile (CPU, rounded reference chained up to the first attention)."""
    for pw in range(0, 8):
        sd2 = dict(sd)
        for n in "qk":
            key = R.ST[0] + f".transformer_blocks.0.attn1.to_{n}.weight"
            sd2[key] = sd[key] * 2.0 ** pw
        tr = []
        try:
            R.forward(sd2, x.transpose(1, 2), ts, ctx, True, F64, trace=_Until(tr, "st0.attn"))
        except StopIteration:
            pass
        q, k, v = dict(tr)["st0.qkv"]
        st = {}
        R.battn(q, k, v, True, F64, stats=st)
        if st["rebased"] >= want:
            return pw, st["rebased"]
    raise AssertionError("no power of two up to 2^7 makes 1 % of the rows rebase")


class _Until(list):
    """A trace list that ends the chained evaluation behind the named launch."""

    def __init__(self, out, name):
        super().__init__()
        self.out, self.name = out, name

    def append(self, item):
        self.out.append(item)
        if item[0] == self.name:
            raise StopIteration


def test_attention_rebase_branch(dev):
    """Shape A-hot: 2 x 290 with to_q / to_k of the first block scaled so that battn_kernel's rebase branch (a later key tile beats the reference by more than 16 in
    the exponent) is taken by >= 1 % of the rows — asserted from the q and k the GPU stored."""
    full = synth.said_state_dict(num_w2v_layers=1)
    _, sd_u, _ = op.split_state_dict(full)
    B, T, seed = 2, 290, 571
    x, ctx, ts = _inputs(B, T, seed)
    pw, share = _hot_power(sd_u, x, ts, ctx)
    print(f"A-hot: to_q / to_k x 2^{pw}: {100 * share:.2f} % of the rows rebase on the CPU")
    for n in "qk":
        full["denoiser." + R.ST[0] + f".transformer_blocks.0.attn1.to_{n}.weight"] *= 2.0 ** pw
    _, sd_u, _ = op.split_state_dict(full)
    s, rec = _forward_case(_model(dev, full), sd_u, dev, "A-hot", B, T, seed, only=(5, 6))
    st = {}
    R.battn(s.cur["q"], s.cur["k"], s.cur["v"], True, F64, stats=st)
    assert st["rebased"] >= 0.01, f"only {100 * st['rebased']:.2f} % of the rows rebase on the q and k the GPU stored"
    _summary("A-hot", rec)


# ---------------------------------------------------------------- the guided loop step
def _guided_case(model, sd, null, dev, case, six=False):
    Bc, T, k = 2, 70, 24
    Be = 2 * Bc
    eta = 1.0 if case.endswith("eta") else 0.0
    lat = synth.synth_latents(581, (Bc, T, 32))
    ctx = synth.synth_latents(582, (Bc, T, 768))
    sch = model.noise_scheduler
    sch.set_timesteps(50)
    ts = sch.timesteps.numpy()
    coef = sch.coef_table(ts[k:k + 2], eta)[:1]
    kw, kwd = {}, {}
    if eta > 0:
        mask = torch.zeros(Bc, T, 32)
        mask[:, 60:68] = 1
        mask[:, :, :5] = 1
        kw = dict(noise=synth.synth_latents(583, (Bc, T, 32)), init=synth.synth_latents(584, (Bc, T, 32)).abs().clamp(0, 1), enoise=synth.synth_latents(585, (Bc, T, 32)), mask=mask)
        kwd = dict(step_noise=kw["noise"][None].to(dev), init_latents=kw["init"].to(dev), edit_noise=kw["enoise"].to(dev), mask=mask.to(dev))
    eng = model._get_engine(Be, max(T, 64))
    latd, ctxd = lat.to(dev), ctx.to(dev)
    out = {}

    def run():
        out["y"] = eng.denoise_loop(latents=latd, context=ctxd, timesteps=ts[k:k + 1], coef=coef, prediction_type="epsilon", guidance_scale=GS, guidance_rescale=0.0,
                                    latent_scale=1.0, **kwd)[1]
        torch.cuda.synchronize()

    sched = _schedule(True, six)
    assert len(sched) == (48 if six else 28)
    rec = []
    opts = dict(TM_OPTS, **({"st_chain_bf16": 0} if six else {}))
    with Options(eng, opts):
        s = Stops(eng, Be, T, T, run)
        n0 = eng.debug_get("n_out_sched_tm")
        for n, la in enumerate(sched[:-1], 1):
            c = s.stop(n, la)
            if n == 1:
                check_exact(f"{case} x (channel-major latents)", c["x"][:Bc], lat.transpose(1, 2))
                _kv_checks(case, s, Bc, six)
            _check_launch(case, sd, null, la, c, Be, Bc, "plain", rec, T)
        assert eng.debug_get("n_out_sched_tm") == n0, "no stop so far reached the step's last launch"
        eng.debug_stop_after(-1)
        run()
        assert eng.debug_get("n_out_sched_tm") > n0 and eng.graph_num_nodes() == len(sched), eng.graph_num_nodes()
        for name in ("tP", "stP"):
            assert torch.equal(s.read(name).view(torch.int32), s.cur[name].view(torch.int32)), name
        log = [d["kind"] for d in eng.profile_unet(Be, T, reps=1, cfg_clips=Bc)]
        got = out["y"].cpu()
        # out_sched_tm_kernel<CFG>: test_gpu_round5.py's rule (test_out_sched_tm_against_the_standalone_scheduler_on_its_own_hidden_state) over all samples — the model
        # output recomputed in float64 from the stored hidden state with the kernel's roundings, pushed through said_ddim_step (bit-exact against the oracle)
        eps = R.finish(R.out_conv_parts(sd, s.cur["tP"], s.cur["stP"], True, F64), True, True, bf16=False).float()
        want = eng.ddim_step(eps[Bc:].to(dev), latd, coef[0], "epsilon", eps_uncond=eps[:Bc].to(dev), guidance_scale=GS, step_noise=kwd.get("step_noise", [None])[0],
                             init_latents=kwd.get("init_latents"), edit_noise=kwd.get("edit_noise"), mask=kwd.get("mask")).cpu()
    # profile_unet has no scheduler update to run: its last block ends as forward()'s does (five tail launches ending on xgemm_kernel, then the out convolution),
    # everything before the last block's tail is the loop's schedule
    n_same = max(i for i, la in enumerate(sched) if la[0] == "attn") + 1
    assert log[:n_same] == _kinds(sched)[:n_same] and log[n_same:] == [7, 7, 7, 7, 6, 12], log
    d = (got - want).abs()
    q = float((d <= 2e-5).double().mean())
    print(f"{case} out_sched_tm_kernel<CFG> vs emulated operands + said_ddim_step: max {float(d.max()):.2e}, {100 * q:.2f} % of elements within 2e-5, eps range {float(eps.abs().max()):.2f}")
    assert float(d.max()) <= 6e-3 and q >= 0.95
    if eta > 0:   # masked elements do not depend on the model output: bit-exact
        m = kw["mask"].bool()
        assert torch.equal(got[m], want[m]), "a masked element is not the noised initial latent"
        cf = torch.from_numpy(np.asarray(coef[0], dtype=np.float32))
        assert torch.equal(got[m], (cf[5] * kw["init"] + cf[6] * kw["enoise"])[m])
        assert bool(m[:, 60:68].all()) and not bool(m[:, 68:, 5:].any()), "the mask crosses the token-tile boundary at 64"
    _summary(case, rec)


@pytest.mark.parametrize("case", ["G", "G-eta"])
def test_guided_step_launches_on_their_own_inputs(plain, dev, case):
    """One guided loop step of two clips x 70 frames (Be 4): every launch, then out_sched_tm_kernel<CFG>."""
    model, sd, null = plain
    _guided_case(model, sd, null, dev, case)


def test_guided_step_with_the_six_launch_tail(plain, dev):
    """Shape T6 (guided): to_out with the c2 duplicate for the unconditional half, the cross-attention launches on the conditional half alone."""
    model, sd, null = plain
    _guided_case(model, sd, null, dev, "T6-G", six=True)


# ---------------------------------------------------------------- workspace fills
@pytest.mark.parametrize("tag", ["S", "T6", "A640", "G-eta"])
def test_workspace_fill_does_not_reach_a_result(plain, dev, tag):
    """The stand-in for comparing pad tokens: the forward pass (S, T6, A at T = 640) and the guided step with eta noise and mask (G-eta) from a workspace of zeros, NaNs
    and 3.4e38 — finite and bit-identical."""
    model, _, _ = plain
    B, T = (2, 640) if tag == "A640" else (3, 70)
    x, ctx, ts = _inputs(B, T, 590)
    x, ctx = x.to(dev), ctx.to(dev)
    sch = model.noise_scheduler
    sch.set_timesteps(50)
    tsl = sch.timesteps.numpy()
    coef = sch.coef_table(tsl[24:26], 1.0)[:1]
    mask = torch.zeros(B, T, 32)
    mask[:, 60:68] = 1
    mask[:, :, :5] = 1
    kw = dict(step_noise=synth.synth_latents(592, (1, B, T, 32)).to(dev), init_latents=synth.synth_latents(593, (B, T, 32)).abs().clamp(0, 1).to(dev),
              edit_noise=synth.synth_latents(594, (B, T, 32)).to(dev), mask=mask.to(dev))
    eng = model._get_engine(2 * B, max(T, 64))
    ref = None
    with Options(eng, dict(TM_OPTS, **({"st_chain_bf16": 0} if tag == "T6" else {}))):
        n0 = eng.debug_get("n_rgemm")
        for fill in (0x00, 0xFF, 0x7F):
            eng.ws_fill(fill)
            if tag == "G-eta":
                o = eng.denoise_loop(latents=x, context=ctx, timesteps=tsl[24:25], coef=coef, prediction_type="epsilon", guidance_scale=GS, guidance_rescale=0.0,
                                     latent_scale=1.0, **kw)[1].cpu()
            else:
                o = eng.unet_forward(x, ts, ctx).cpu()
            assert torch.isfinite(o).all(), f"fill 0x{fill:02X}: the result is not finite"
            ref = o if ref is None else ref
            assert torch.equal(o, ref), f"fill 0x{fill:02X}: the result depends on memory nobody wrote"
        assert eng.debug_get("n_rgemm") > n0, "the token-major schedule ran"
        if tag != "G-eta":
            kinds = [d["kind"] for d in eng.profile_unet(B, T, reps=1)]
            assert kinds.count(9) == 4 and kinds.count(10) == (0 if tag == "T6" else 3), kinds   # battn_kernel in every block; the fused tail unless switched off
