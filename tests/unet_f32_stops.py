"""What the launch-by-launch tests of the fp32 denoise step share (tests/test_gpu_unet_f32_kernels.py: the default split-fp16 mode; tests/test_gpu_unet_f32_strict_kernels.py:
strict fp32 and the routes beside the fused tail) — TEST INFRASTRUCTURE.

* the schedules as unet_sched.cpp issues them (run_unet / run_resblock / run_transformer), launch by launch, and what each launch reads and writes by workspace name;
* Stops: the stop-and-read loop (said_debug_stop_after + the workspace list), with the rule that a buffer read again at a later stop is bit-equal;
* one check per launch against tests/unet_f32_ref.py's float64 evaluation of the launch's own stored inputs under audio_bf16_ref.check_f32;
* set_band's rule restated (band_facts), for the shapes that are chosen by it.
"""
import torch

import unet_f32_ref as R
from audio_bf16_ref import check_exact, check_f32
from said_amd.util import synth

F64, F32 = torch.float64, torch.float32
MC, FFI = R.MC, R.FFI
GS = 2.0


def _model(dev, sd):
    from said_amd.model.diffusion import SAID_UNet1D
    from said_amd.model.wav2vec2 import AudioConfig
    m = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=1))
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


# ---------------------------------------------------------------- the alignment band (unet_sched.cpp set_band), restated
def band_tables(T, S):
    """(lo, hi) per query: Python's round() is the banker's rounding on doubles that set_band's nearbyint is."""
    ratio = S / T
    kh = ratio / 2 + 1
    lo = [max(round((i + 0.5) * ratio - kh), 0) for i in range(T)]
    hi = [min(round((i + 0.5) * ratio + kh), S) for i in range(T)]
    return lo, hi


def band_facts(T, S, chain_kw):
    """(wmax, the fused tail's window tile holds the band): wmax <= 8, lo non-decreasing, and max(hi) - lo[t0] <= CHAIN_KW over every 32-token tile."""
    lo, hi = band_tables(T, S)
    wmax = max(h - l for l, h in zip(lo, hi))
    ok = wmax <= 8 and all(lo[i] >= lo[i - 1] for i in range(1, T))
    ok = ok and all(max(hi[t0:t0 + 32]) - lo[t0] <= chain_kw for t0 in range(0, T, 32))
    return wmax, ok


def smallest_narrow_band_the_window_tile_cannot_hold(chain_kw):
    """The smallest (T, S) — by S, then T — with wmax <= 8 that fails the tile rule.  (max(hi) - lo[t0] <= S: no S <= CHAIN_KW fails it.)"""
    for S in range(1, 4 * chain_kw):
        for T in range(1, S + 1):
            wmax, ok = band_facts(T, S, chain_kw)
            if wmax <= 8 and not ok:
                return T, S
    raise AssertionError("no such shape")


# ---------------------------------------------------------------- the schedule (unet_sched.cpp run_unet) and what each launch reads and writes
def _schedule(guided, five=False, wide=False):
    """five: the five launches behind the self-attention instead of stchain_kernel (strict fp32; a band the window tile cannot hold; st_chain = 0), whose q/k/v GEMM
    leaves no gn_coef rows; wide: windows wider than 8 keys — the plain q projection and band_wide_kernel in place of the fused EPI_BAND epilogue."""
    L = [("conv_in",)]

    def res(i, in0, in1, out, shared=False):
        L.append(("conv1", i, in0, in1, shared))
        L.append(("conv2", i, in0, in1, out, shared))

    def st(j, inn, out, shared=False):
        if not five:
            L.extend([("qkv", j, inn, shared), ("attn", j, shared), ("chain", j, inn, out, shared)])
            return
        L.extend([("qkv5", j, inn, shared), ("attn", j, shared), ("out1", j, inn, shared)])
        L.extend([("qplain", j, shared), ("bandw", j, shared)] if wide else [("qband", j, shared)])
        L.extend([("out2", j, shared), ("geglu", j), ("ffproj", j, inn, out)])

    res(0, "H0", None, "P", guided); st(0, "P", "H1", guided)
    res(1, "H1", None, "P"); st(1, "P", "Q")
    res(2, "Q", None, "P")
    res(3, "P", "H1", "Q"); st(2, "Q", "P")
    res(4, "P", "H0", "Q"); st(3, "Q", "P")
    L.append(("out_sched",) if guided else ("out",))
    return L


def _schedule_f(five=False):
    """The large-batch route (prep_kernel + fgemm_kernel).  five: without the fused tail — attn1.to_out, the band and attn2.to_out stay channel-major (below 2048
    (sample, head, tile) triples), GEGLU and the folded proj_out run token-major behind a third preparation launch; the q/k/v preparation leaves no gn_coef rows."""
    L = [("conv_in",)]

    def res(i, in0, in1, out):
        cin = 2 * MC if in1 else MC
        for off, src in enumerate(s for s in (in0, in1) if s):
            L.append(("prep0", i, src, off * MC, cin, bool(in1)))
        L.append(("fconv1", i, cin))
        L.append(("prep0", i, "M", 0, MC, False))
        L.append(("fconv2", i, in0, in1, out))

    def st(j, inn, out):
        if not five:
            L.extend([("prep1", j, inn), ("fqkv", j), ("attn", j, False), ("chain", j, inn, out, False)])
            return
        L.extend([("prep1n", j, inn), ("fqkv", j), ("attn", j, False), ("out1", j, inn, False), ("qband", j, False), ("out2", j, False),
                  ("prep2", j), ("fgeglu", j), ("fffproj", j, inn, out)])

    res(0, "H0", None, "P"); st(0, "P", "H1")
    res(1, "H1", None, "P"); st(1, "P", "Q")
    res(2, "Q", None, "P")
    res(3, "P", "H1", "Q"); st(2, "Q", "P")
    res(4, "P", "H0", "Q"); st(3, "Q", "P")
    L.append(("out",))
    return L


def _io(launch):
    """(buffers read, buffers written) of a launch, by workspace name.  A launch that works in place (the band) lists the buffer as written only."""
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
    if k == "qkv5":
        return [launch[2], "st" + launch[2]], ["QK", "VT"]
    if k == "attn":
        return ["QK", "VT"], ["O"]
    if k == "chain":
        return ["O", launch[2], "gn_coef", "KV"], [launch[3], "st" + launch[3]]
    if k == "out1":      # (X2: the y2 = x1 + c2 duplicate, stored under guidance only; read back either way — without guidance nothing looks at it)
        return ["O", launch[2], "st" + launch[2]], ["X1", "X2"]
    if k in ("qband", "qplain"):
        return ["X1", "KV"], ["O"]
    if k == "bandw":
        return ["KV"], ["O"]
    if k == "out2":
        return ["O", "X1"], ["X2"]
    if k == "geglu":
        return ["X2"], ["F"]
    if k == "ffproj":
        return ["F", "X2", launch[2]], [launch[3], "st" + launch[3]]
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
    if k == "prep1n":
        return [launch[2], "st" + launch[2]], [f"uPL:{MC}"]
    if k == "fqkv":
        return [f"uPL:{MC}"], ["QK", "VT"]
    if k == "attn_tm":   # the four-query-tile attention storing token-major into the q/k/v operand buffer
        return ["QK", "VT"], [f"uPL:{MC}"]
    if k == "fout1":
        return [f"uPL:{MC}", launch[2], "gn_coef"], ["X1"]
    if k == "prep2":
        return ["X2"], [f"uPL:{MC}", f"uPX:{MC}"]
    if k == "fgeglu":
        return [f"uPL:{MC}"], [f"uPH:{FFI}"]
    if k == "fffproj":
        return [f"uPH:{FFI}", f"uPX:{MC}", launch[2]], [launch[3], "st" + launch[3]]
    return ["P", "stP"], []   # out_sched: its output is the loop's result


class Stops:
    """One shape's stopped runs: `run` makes the call (forward pass or loop step), stop(k, launch) makes it with the first k launches and reads the launch's buffers.
    cur: buffer name -> tensor as stored at the latest stop; prev: the same before the latest stop (what a launch that works in place read)."""

    def __init__(self, eng, Be, T, S, run):
        self.eng, self.Be, self.T, self.S, self.run = eng, Be, T, S, run
        self.Tp, self.Sp, self.np = R.rup(T, 32), R.rup(S, 32), (T + 31) // 32
        self.sizes = {nm: nb for _, nm, nb in eng.ws_buffers()}
        self.index = {nm: i for i, nm, _ in eng.ws_buffers()}
        self.cur, self.prev = {}, {}

    def raw(self, name, nfloat):
        assert 4 * nfloat <= self.sizes[name], (name, nfloat, self.sizes[name])
        t = self.eng.ws_snapshot(self.index[name], 4 * nfloat)
        torch.cuda.synchronize()
        return t.cpu().view(torch.float32)

    def read(self, name):
        """The buffer as stored, pad tokens removed."""
        Be, T, Tp = self.Be, self.T, self.Tp
        if name in ("H0", "H1", "P", "Q", "M", "X1", "X2"):
            return self.raw(name, Be * MC * Tp).view(Be, MC, Tp)[:, :, :T].clone()
        if name.startswith("st"):
            return self.raw(name, Be * self.np * MC * 2).view(Be, self.np, MC, 2).clone()
        if name in ("x", "eps"):
            return self.raw(name, Be * 32 * Tp).view(Be, 32, Tp)[:, :, :T].clone()
        if name == "O":
            return self.raw(name, Be * 2 * MC * Tp).view(Be, 2 * MC, Tp)[:, :MC, :T].clone()
        if name == "F":
            return self.raw(name, Be * FFI * Tp).view(Be, FFI, Tp)[:, :, :T].clone()
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
        self.prev = dict(self.cur)
        for name in ins:
            v = self.read(name)
            if name in self.cur:
                assert torch.equal(v.view(torch.int32), self.cur[name].view(torch.int32)), f"launch {k} {launch}: {name} differs from what the earlier stop saw"
            self.cur[name] = v
        for name in outs:
            self.cur[name] = self.read(name)
        return self.cur


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


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


def _check_launch(tag, sd, null, la, c, Be, Bc, rec, packed=True, prev=None, S=None):
    """One launch on its own stored inputs.  c: buffer name -> tensor as stored; Bc > 0: the guided step's sample layout (unconditional half first).
    packed: k and v are stored as packed split pairs (the default mode's key-split attention shapes), else as plain fp32; prev: Stops.prev; S: the context's length
    (default: T)."""
    k = la[0]
    shared = bool(la[-1]) if k in ("conv1", "conv2", "qkv", "qkv5", "attn", "chain", "out1", "qband", "qplain", "bandw", "out2") else False
    ns = Bc if shared else Be                     # samples this launch computes
    # the cross-attention range (unet_sched.cpp StRange): n2 samples, from x_off in X1 / O, from kv_off in X2 / KV
    n2, x_off, kv_off = (Bc if Bc else Be), (Bc if (Bc and not shared) else 0), Bc
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
    elif k in ("qkv", "qkv5"):
        _, j, inn, _ = la
        x = c[inn][:ns]
        if packed:
            kd, vd = _split(f"{tag} st{j} k", c["QK"][:ns, 6:]), _split(f"{tag} st{j} v", c["VT"][:ns])
        else:
            kd, vd = c["QK"][:ns, 6:].double(), c["VT"][:ns].double()
        c["k_dec"], c["v_dec"] = kd, vd
        for n, idx, got in (("q", 0, c["QK"][:ns, :6]), ("k", 1, kd), ("v", 2, vd)):
            f(f"st{j} q/k/v: {n}", lambda dt: R.qkv(sd, j, x, dt)[idx], got)
        if k == "qkv":
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
    elif k == "out1":     # attn1.to_out + the GroupNorm'ed residual from the block input's stored partials; under guidance the duplicate y2 = x1 + c2 of every sample
        _, j, inn, _ = la
        fn = lambda dt: R.to_out1(sd, j, c["O"][:ns], c[inn][:ns], c["st" + inn][:ns], dt, null=null if Bc else None)
        f(f"st{j} to_out1", lambda dt: fn(dt)[0], c["X1"][:ns])
        if Bc:
            f(f"st{j} to_out1: the duplicate y2 = x1 + c2", lambda dt: fn(dt)[1], c["X2"][:ns])
    elif k in ("qband", "qplain", "bandw"):
        _, j, _ = la
        T = c["X1"].shape[-1]
        S = T if S is None else S
        kv = c["KV"][kv_off:kv_off + n2, j * 2 * MC:(j + 1) * 2 * MC]
        x1, got = c["X1"][x_off:x_off + n2], c["O"][x_off:x_off + n2]
        if k == "qband":
            f(f"st{j} to_q + band", lambda dt: R.q_band(sd, j, x1, kv[:, :MC], kv[:, MC:], T, S, dt), got)
        elif k == "qplain":
            f(f"st{j} to_q (plain, in front of band_wide_kernel)", lambda dt: R.q2(sd, j, x1, dt), got)
        else:
            q = prev["O"][x_off:x_off + n2]
            f(f"st{j} band_wide_kernel", lambda dt: R.band(q, kv[:, :MC], kv[:, MC:], T, S, dt), got)
        if x_off:
            assert _bits_equal(c["O"][:x_off], prev["O"][:x_off]), f"{tag} st{j} {k}: the attention output of the unconditional half changed"
    elif k == "out2":
        _, j, _ = la
        f(f"st{j} to_out2", lambda dt: R.to_out2(sd, j, c["O"][x_off:x_off + n2], c["X1"], dt, x_off=x_off), c["X2"][kv_off:kv_off + n2])
        if Bc:
            assert _bits_equal(c["X2"][:Bc], prev["X2"][:Bc]), f"{tag} st{j} to_out2: an unconditional slot of X2 was written"
    elif k == "geglu":
        _, j = la
        f(f"st{j} GEGLU", lambda dt: R.geglu(sd, j, c["X2"], dt), c["F"])
    elif k == "ffproj":
        _, j, inn, out = la
        f(f"st{j} folded proj_out", lambda dt: R.ffproj(sd, j, c["F"], c["X2"], c[inn], dt), c[out])
        rec.append(("st" + out,) + _partials(f"{tag} st{j} folded proj_out", c[out], c["st" + out]))
    elif k == "out":
        f("out convolution", lambda dt: R.out_conv(sd, c["P"], dt), c["eps"])
    else:
        raise KeyError(k)


def _kv_checks(tag, sd, s, ctx, b0, rec, kvt=True):
    """KV of samples [b0, Be) against the float64 projection of their context; KVT its exact transpose (kvt: where the fused tail's key-major copy is made)."""
    kv = s.read("KV")
    rec.append(("KV",) + check_f32(f"{tag} KV", kv[b0:], R.kv_all(sd, ctx, F64), R.kv_all(sd, ctx, F32)))
    if kvt:
        check_exact(f"{tag} KVT (key-major copy)", s.read("KVT")[b0:], kv[b0:].transpose(1, 2))


def _summary(tag, rec):
    print(f"{tag}: {len(rec)} comparisons, largest e {max(e for _, e, _ in rec):.2e}, largest e / bound {max(e / b for _, e, b in rec):.3f}")
    fam = {}
    for name, e, _ in rec:
        key = name.split(" ", 1)[1] if name.startswith(("res", "st")) and " " in name else name
        fam[key] = max(fam.get(key, 0.0), e)
    print(f"{tag}: largest e per launch family: " + "; ".join(f"{k} {v:.1e}" for k, v in fam.items()))


# ---------------------------------------------------------------- the large-batch route (prep_kernel + fgemm_kernel)
def _operand(tag, buf, T, row_off, packed=True):
    """A token-major operand buffer (B, rows, columns): the T token rows (decoded where packed), the Conv1d padding rows (row_off = 1: rows 0 and T + 1) all-zero bits."""
    if row_off:
        assert int(buf[:, 0].view(torch.int32).abs().sum()) == 0 and int(buf[:, T + 1].view(torch.int32).abs().sum()) == 0, f"{tag}: a padding row is not zero"
    rows = buf[:, row_off:row_off + T]
    return _split(tag, rows) if packed else rows.double()


def _check_launch_f(tag, sd, la, c, B, T, rec, packed=True, prev=None, S=None):
    """packed: prep_kernel's pack mode and fgemm_kernel's kv_pack epilogue (the default mode); else plain fp32 operands, k and v (strict fp32).  The third
    preparation launch (GEGLU's operand and the raw x2) never packs."""
    k = la[0]
    f = lambda name, fn, got: rec.append((name,) + check_f32(f"{tag} {name}", got, fn(F64), fn(F32)))
    if k == "prep0":
        _, i, src, off, cin, raw = la
        op_ = _operand(f"{tag} res{i} uPA columns [{off}, {off + MC})", c[f"uPA:{cin}"][:, :, off:off + MC], T, 1, packed)
        if src == "M":
            f(f"res{i} prep_kernel, conv 2's operand", lambda dt: R.res_operand2(sd, i, c["M"], dt).transpose(1, 2), op_)
        else:
            c.setdefault(("srcs", i), []).append(c[src])
            if off == 0 and raw:
                return   # (GroupNorm spans both sources: checked behind the second preparation launch)
            xs = c.pop(("srcs", i))
            full = _operand(f"{tag} res{i} uPA", c[f"uPA:{cin}"], T, 1, packed)
            f(f"res{i} prep_kernel, conv 1's operand ({len(xs)} source{'s' if len(xs) > 1 else ''})", lambda dt: R.res_operand1(sd, i, xs, dt).transpose(1, 2), full)
            if raw:   # the raw copy: the same values, packed (h + 2^-11 l holds 22 significand bits) or plain
                rawv = _operand(f"{tag} res{i} uPB", c[f"uPB:{2 * MC}"], T, 0, packed)
                want = torch.cat(xs, dim=1).transpose(1, 2).double()
                if packed:
                    assert bool(((rawv - want).abs() <= 2.0 ** -21 * want.abs() + 2.0 ** -36).all()), f"{tag} res{i}: the raw copy for the 1x1 skip is not the input"
                else:
                    check_exact(f"{tag} res{i}: the raw copy for the 1x1 skip", rawv.float(), want.float())
    elif k == "fconv1":
        _, i, cin = la
        op_ = _operand(f"{tag} res{i} uPA", c[f"uPA:{cin}"], T, 1, packed).transpose(1, 2)
        f(f"res{i} conv 1 on fgemm_kernel ({cin // MC} source{'s' if cin > MC else ''})", lambda dt: R.res_conv1(sd, i, None, c["EO"][i][:, :B].t(), dt, operand=op_), c["M"])
        rec.append(("stM",) + _partials(f"{tag} res{i} conv 1", c["M"], c["stM"]))
    elif k == "fconv2":
        _, i, in0, in1, out = la
        op_ = _operand(f"{tag} res{i} uPA", c[f"uPA:{MC}"], T, 1, packed).transpose(1, 2)
        if in1:
            rawv = _operand(f"{tag} res{i} uPB", c[f"uPB:{2 * MC}"], T, 0, packed).transpose(1, 2)
            xs = [rawv[:, :MC], rawv[:, MC:]]
        else:
            xs = [c[in0]]
        f(f"res{i} conv 2 on fgemm_kernel ({'1x1 skip segment' if in1 else 'residual'})", lambda dt: R.res_conv2(sd, i, None, xs, dt, operand=op_)[0], c[out])
        rec.append(("st" + out,) + _partials(f"{tag} res{i} conv 2", c[out], c["st" + out]))
    elif k in ("prep1", "prep1n"):
        _, j, inn = la
        op_ = _operand(f"{tag} st{j} uPL", c[f"uPL:{MC}"], T, 0, packed)
        f(f"st{j} prep_kernel, q/k/v's operand", lambda dt: R.qkv_operand(sd, j, c[inn], dt), op_)
        if k == "prep1":
            for n, idx in (("a", 0), ("b", 1)):
                f(f"st{j} gn_coef {n}", lambda dt: R.gn_coef(sd, j, c[inn], dt)[..., idx], c["gn_coef"][:, :, idx])
    elif k == "fqkv":
        _, j = la
        op_ = _operand(f"{tag} st{j} uPL", c[f"uPL:{MC}"], T, 0, packed)
        if packed:
            kd, vd = _split(f"{tag} st{j} k", c["QK"][:, 6:]), _split(f"{tag} st{j} v", c["VT"])
        else:
            kd, vd = c["QK"][:, 6:].double(), c["VT"].double()
        c["k_dec"], c["v_dec"] = kd, vd
        for n, idx, got in (("q", 0, c["QK"][:, :6]), ("k", 1, kd), ("v", 2, vd)):
            f(f"st{j} q/k/v on fgemm_kernel: {n}", lambda dt: R.qkv(sd, j, None, dt, operand=op_)[idx], got)
    elif k == "attn_tm":
        _, j = la
        f(f"st{j} self-attention, token-major store", lambda dt: R.self_attention(c["QK"][:, :6], c["k_dec"], c["v_dec"], dt), c[f"uPL:{MC}"][:, :T].transpose(1, 2))
    elif k == "fout1":
        _, j, inn = la
        o = c[f"uPL:{MC}"][:, :T].transpose(1, 2)
        f(f"st{j} to_out1 on fgemm_kernel (coefficient residual)", lambda dt: R.to_out1(sd, j, o, c[inn], c["gn_coef"], dt)[0], c["X1"])
    elif k == "prep2":
        _, j = la
        f(f"st{j} prep_kernel, GEGLU's operand", lambda dt: R.geglu_operand(sd, j, c["X2"], dt), c[f"uPL:{MC}"][:, :T])
        check_exact(f"{tag} st{j} prep_kernel: the raw x2 for the folded proj_out", c[f"uPX:{MC}"][:, :T], c["X2"].transpose(1, 2))
    elif k == "fgeglu":
        _, j = la
        op_ = c[f"uPL:{MC}"][:, :T]
        f(f"st{j} GEGLU on fgemm_kernel", lambda dt: R.geglu(sd, j, None, dt, operand=op_).transpose(1, 2), c[f"uPH:{FFI}"][:, :T])
    elif k == "fffproj":
        _, j, inn, out = la
        h, x2 = c[f"uPH:{FFI}"][:, :T].transpose(1, 2), c[f"uPX:{MC}"][:, :T].transpose(1, 2)
        f(f"st{j} folded proj_out on fgemm_kernel (two operands)", lambda dt: R.ffproj(sd, j, h, x2, c[inn], dt), c[out])
        rec.append(("st" + out,) + _partials(f"{tag} st{j} folded proj_out", c[out], c["st" + out]))
    else:
        _check_launch(tag, sd, None, la, c, B, 0, rec, packed=packed, prev=prev, S=S)


# ---------------------------------------------------------------- the stand-in for comparing pad tokens
def _poison(model, dev, B, T, seed, opts=None, S=None, guided=True):
    """Forward pass and one guided step (eta = 1 noise, initial latents, edit noise and a mask across the tile boundary at 64: everything out_sched_kernel<CFG> reads)
    with the workspace filled with 0x00, 0xFF (NaN) and 0x7F (3.4e38) first: finite and bit-identical.  opts: said_debug_option settings, restored afterwards.
    S: the context's length where it is not T (forward pass only: guided = False)."""
    S = T if S is None else S
    assert S == T or not guided
    x = synth.synth_latents(seed, (B, T, 32)).to(dev)
    ctx = synth.synth_latents(seed + 1, (B, S, 768)).to(dev)
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
    eng = model._get_engine(2 * B, max(T, S, 64))
    ref = None
    try:
        for k, v in (opts or {}).items():
            eng.debug_option(k, v)
        for fill in (0x00, 0xFF, 0x7F):
            eng.ws_fill(fill)
            o1 = eng.unet_forward(x, ts, ctx).cpu()
            o2 = o1
            if guided:
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
