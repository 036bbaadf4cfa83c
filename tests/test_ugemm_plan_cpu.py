"""The host-side decisions of the UNet GEMM (said_amd/csrc/ugemm_plan.h) without a GPU: tests/ugemm_plan_main.cpp — the header behind a command line, compiled
once per session with the host compiler of the ROCm installation — against tests/golden/ugemm_plan.txt.

The fixture was recorded from the logic the header replaced (ugemm_supports and its three shape lists in gemm_lds.hip, pick_unet / best_nb / pick_tt and the body
of do_gemm in unet_sched.cpp, behind the same command line), so it holds what each launch of the channel-major schedule ran on before there was a plan: per case,
frame count, and setting of the five switches, the (kernel, NB, KS, tiles per workgroup) of every batch size of a scan, printed where it changes.  A change that
is meant to keep the schedule keeps the file; one that is meant to alter a rule records it again from the new program and says so."""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_weight_pack_cpu import _host_compiler  # noqa: E402

ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "said_amd", "csrc")
FIXTURE = os.path.join(HERE, "golden", "ugemm_plan.txt")


@pytest.fixture(scope="session")
def planner(tmp_path_factory):
    """run(*args) -> stdout of the compiled tests/ugemm_plan_main.cpp."""
    cxx, inc = _host_compiler()
    exe = str(tmp_path_factory.mktemp("ugemm_plan") / "ugemm_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-x", "c++", f"-I{inc}", "-D__HIP_PLATFORM_AMD__", "-I" + CSRC, os.path.join(HERE, "ugemm_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout
    return run


def test_split_and_multi_tile_rows_are_base_rows(planner):
    """ugemm_supports used to ask for a base-list entry beside every split-fp16 / multi-tile one; the table lookup no longer does, because every such row has one."""
    m = re.fullmatch(r"rows base=(\d+) split=(\d+) multi_tile=(\d+) bad=0\n", planner("rows"))
    assert m, planner("rows")
    assert [int(g) for g in m.groups()] == [56, 22, 16]   # 28 base shapes x (fp32, bf16), 22 split-fp16 shapes, 8 multi-tile shapes x (fp32, bf16)


def test_plans_are_the_recorded_ones(planner):
    with open(FIXTURE) as f:
        want = f.read().splitlines()
    got = planner().splitlines()
    assert len(want) == 148
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def test_fixture_covers_the_rules():
    """Every kernel, the NB 3 -> 2 fallback, the kconv NB = 1 window, every tiles-per-workgroup count up to the cap, and the unserved launches appear in the file."""
    with open(FIXTURE) as f:
        lines = f.read().splitlines()
    plans = {p.split("=")[1] for ln in lines for p in ln.split(" : ")[1].split()}
    assert {p.split("/")[0] for p in plans} == {"cgemm", "f32", "bf16", "sp"}
    assert {int(p.split("/")[3]) for p in plans} == set(range(1, 9))
    by = {}
    for ln in lines:
        head, scan = ln.split(" : ")
        name, T, codes = head.split()
        for c in codes.split(","):
            by[name, T, c] = scan
    assert len(by) == 19 * 3 * 48   # cases x frame counts x switch settings: every combination is on exactly one line
    # pick_unet_nb asks for NB = 3 from 86 tiles; the two-segment fp32 shape is not built (NB -> 2), and with split products and kconv on the launch becomes NB = 1
    assert by["in_layers_cat", "T=32", "f0100"] == "b1=f32/1/8/1 b43=f32/2/8/1"
    assert by["in_layers_cat", "T=32", "f1100"] == "b1=sp/1/8/1 b43=f32/2/8/1 b86=sp/1/8/1 b129=f32/2/8/1"
    assert by["in_layers_cat", "T=32", "f1110"] == by["in_layers_cat", "T=32", "f1101"] == by["in_layers_cat", "T=32", "f1000"] == "b1=sp/1/8/1 b43=f32/2/8/1"   # concurrent, clk, kconv = 0
    assert by["in_layers_cat", "T=32", "f1210"] == by["in_layers_cat", "T=32", "f1100"]   # kconv = 2: under concurrent clip groups too
    assert by["to_out2_no_w2", "T=32", "b0000"].startswith("b1=f32/1/8/1")   # bf16 mode without Seg::w2: the fp32 ugemm
    assert by["conv_in_step", "T=32", "f1100"] == by["conv_in", "T=32", "f1100"] == "b1=cgemm/1/8/1 b43=cgemm/2/8/1"


def test_presplit_term_is_the_plan_s(planner):
    """run_transformer stores k and v pre-split when the q/k/v GEMM runs on ugemm_kernel.  It used to work that out with two ugemm_supports calls of its own (the
    /p field, recorded from them); it now asks the plan.  In fp32 mode — the only mode that pre-splits — the two agree for every switch setting and batch size."""
    n = 0
    for ln in planner().splitlines():
        head, scan = ln.split(" : ")
        if not head.startswith("qkv") or "f" not in head.split()[2]:   # (a line lists the switch settings that share its result)
            continue
        for p in scan.split():
            kernel, *_, pre = p.split("=")[1].split("/")
            assert (kernel != "cgemm") == (pre == "p1"), ln
            n += 1
    assert n > 50


def _plan(planner, batch, T, split=True):
    """{case: "kernel/NB/KS/tt body"} at one batch and frame count, fp32 mode's default switches (split = False: ugemm_split off, what strict fp32 plans with)."""
    return dict(ln.split(" ", 1) for ln in planner("plan", str(batch), str(T), *([] if split else ["0"])).splitlines())


def test_shapes_of_the_fp32_kernel_test_reach_what_they_are_named_for(planner):
    """tests/test_gpu_unet_f32_kernels.py asserts (kind, epi, NB, KS) per launch from the engine's stage log; what the log does not carry — split-fp16 or fp32 matrix
    instructions, kconv_body or the block loop, token tiles per workgroup, the fused tail's slices — is held here, from the same header the engine plans with."""
    import test_gpu_unet_f32_kernels as K
    SP1, SP2, SP3 = "sp/1/8/1 block", "sp/2/8/1 block", "sp/3/8/1 block"
    want = {   # conv_in, in_layers, out_layers, in_layers_cat, out_layers_skip, qkv, out_conv
        "S": ("cgemm/1/8/1 block", SP1, SP1, "sp/1/8/1 kconv", "sp/1/8/1 kconv", SP1, SP1),
        "M1": ("cgemm/1/8/1 block", SP1, SP1, "sp/1/8/1 kconv", "sp/1/8/1 kconv", SP3, SP1),
        "M2": ("cgemm/2/8/1 block", SP2, SP2, "f32/2/8/1 block", "f32/2/8/1 block", SP2, SP1),            # the concatenated convolutions stay off split-fp16
        "L": ("cgemm/2/8/1 block", SP3, SP3, "sp/1/8/1 kconv", "sp/1/8/1 kconv", "f32/3/8/2 block", SP1),   # the kconv NB = 1 switch; q/k/v two token tiles per workgroup
    }
    names = ("conv_in", "in_layers", "out_layers", "in_layers_cat", "out_layers_skip", "qkv", "out_conv")
    for tag, (B, T, nb_in, nb, nb_cat, nb_qkv, _) in K.SHAPES.items():
        p = _plan(planner, B, T)
        assert tuple(p[n] for n in names) == want[tag], (tag, p)
        # ... and the NB the GPU test expects in the stage log is the plan's
        assert [int(p[n].split("/")[1]) for n in ("conv_in", "in_layers", "in_layers_cat", "qkv")] == [nb_in, nb, nb_cat, nb_qkv], tag
    # G: the shared first block runs on the clip alone (batch 1, the second convolution with the duplicate store), everything behind it on both halves as S
    p1 = _plan(planner, 1, 70)
    assert (p1["in_layers"], p1["out_layers_dup"], p1["qkv"]) == (SP1, SP1, SP1)
    # F: what stays on the channel-major kernels at 3 x 70
    p3 = _plan(planner, 3, 70)
    assert (p3["conv_in"], p3["out_conv"]) == ("cgemm/1/8/1 block", SP1)
    # slices of the fused tail by (sample, token tile) pairs (unet_sched.cpp run_transformer)
    with open(os.path.join(CSRC, "stchain.h")) as f:
        src = f.read()
    c3, c2 = (int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1)) for n in ("CHAIN3_MAX_TILES", "CHAIN2_MAX_TILES"))
    slices = lambda B, T: 3 if B * ((T + 31) // 32) <= c3 else (2 if B * ((T + 31) // 32) <= c2 else 1)
    assert {t: slices(*K.SHAPES[t][:2]) for t in K.SHAPES} == {"S": 3, "M1": 3, "M2": 3, "L": 2}
    assert slices(2, 70) == 3 and slices(3, 70) == 3   # G (both halves), F


def test_shapes_of_the_strict_fp32_kernel_test_reach_what_they_are_named_for(planner):
    """tests/test_gpu_unet_f32_strict_kernels.py's twin of the test above: with ugemm_split off (strict fp32's plan switches) every ugemm_kernel launch of S*, M1*,
    M2* and L* lands on an fp32-MFMA row — none on a split-fp16 row or on kconv_body — at the NB the GPU test expects in the stage log; and the two band shapes are
    what set_band's rule, restated in Python, says they are."""
    import test_gpu_unet_f32_strict_kernels as K
    import unet_f32_stops as H
    names = ("in_layers", "out_layers", "in_layers_cat", "out_layers_skip", "qkv", "to_out1", "q2_band", "to_out2", "geglu", "proj_out", "out_conv")
    F = lambda nb, tt=1: f"f32/{nb}/8/{tt} block"
    want = {   # in the order of `names`
        "S*": (F(1), F(1), F(1), F(1), F(1), F(1), F(1), F(1), F(1), F(1), F(1)),
        "M1*": (F(1), F(1), F(1), F(1), F(3), F(1), F(1), F(1), F(2), F(1), F(1)),                 # q/k/v NB = 3
        "M2*": (F(2), F(2), F(2), F(2), F(2), F(1), F(1), F(2), F(4), F(2), F(1)),                 # NB = 2 throughout
        "L*": (F(3), F(3), F(2), F(2), F(3, 2), F(1, 2), F(1), F(3), F(4), F(3), F(1)),            # NB = 3; q/k/v (and to_out1) two token tiles per workgroup
    }
    for tag, (B, T, nb_in, nb, nb_cat, nb_qkv, _, nb_out2, nb_geglu) in K.SHAPES.items():
        p = _plan(planner, B, T, split=False)
        assert tuple(p[n] for n in names) == want[tag], (tag, p)
        assert p["conv_in"] == f"cgemm/{nb_in}/8/1 block", (tag, p["conv_in"])   # (sample aliasing keeps the forward pass's conv_in on the generic kernel in every mode)
        assert all(v.split("/")[0] in ("f32", "cgemm") and v.endswith("block") for v in p.values()), (tag, p)   # nothing on `sp`, nothing on kconv_body
        assert [int(p[n].split("/")[1]) for n in ("in_layers", "in_layers_cat", "qkv", "to_out2", "geglu", "proj_out")] == [nb, nb_cat, nb_qkv, nb_out2, nb_geglu, nb], tag
    # L*: q/k/v is multi-tile, and does NOT pre-split: run_transformer's presplit term needs split products (sp_on(attn_split)), which strict fp32 switches off —
    # the GPU test sees plain k and v and attn_kernel with KS 4 in the log (attn2q_kernel, KS 34, needs pre-split operands)
    assert int(_plan(planner, 7, 417, split=False)["qkv"].split("/")[3].split()[0]) > 1
    with open(os.path.join(CSRC, "unet_sched.cpp")) as f:
        sched = f.read()
    assert re.search(r"presplit = !c->bf16_mode && sp_on\(c, c->attn_split\) && c->attn_presplit != 0 && key_split", sched)
    assert re.search(r"if \(presplit && ks_run == 4 && a\.o_mode == 0 && .*\) ks_run = 34;", sched)
    with open(os.path.join(CSRC, "engine_internal.h")) as f:
        assert "inline bool sp_on(const said_ctx* c, int opt) { return opt != 0 && !strict_f32(c); }" in f.read()
    # G*: the shared first block on the clip alone (to_out1 with the duplicate store), F*: what stays channel-major at 3 x 70
    p1, p3 = _plan(planner, 1, 70, split=False), _plan(planner, 3, 70, split=False)
    assert (p1["in_layers"], p1["out_layers_dup"], p1["qkv"], p1["to_out1_dup"], p1["q2_band"], p1["to_out2"]) == (F(1),) * 6
    assert (p3["to_out1"], p3["q2_band"], p3["to_out2"], p3["out_conv"]) == (F(1),) * 4
    # W, N in the default mode: the tail's GEMMs on split-fp16 operands, but for GEGLU (no one-tile split-fp16 shape) and the plain to_q projection (the generic kernel)
    for T in (10, 37):
        p = _plan(planner, 2, T)
        assert (p["to_out1"], p["q2_band"], p["to_out2"], p["proj_out"]) == ("sp/1/8/1 block",) * 4 and p["geglu"] == F(1) and p["q2_plain"] == "cgemm/1/8/1 block", p
        ps = _plan(planner, 2, T, split=False)
        assert (ps["to_out1"], ps["q2_band"], ps["to_out2"], ps["geglu"], ps["proj_out"]) == (F(1),) * 5 and ps["q2_plain"] == "cgemm/1/8/1 block", ps
    # the band shapes by set_band's rule: wmax, and max(hi) - lo[t0] <= CHAIN_KW per 32-token tile
    with open(os.path.join(CSRC, "stchain.h")) as f:
        kw = int(re.search(r"constexpr int CHAIN_KW = (\d+);", f.read()).group(1))
    assert kw == K.CHAIN_KW == 56
    assert re.search(r"ok = hmax - lo\[t0\] <= CHAIN_KW;", sched) and re.search(r"bool ok = wmax <= 8;", sched)
    for (T, S), wmax in zip(K.W_SHAPES, (12, 13)):
        assert H.band_facts(T, S, kw) == (wmax, False) and wmax > 8, (T, S, H.band_facts(T, S, kw))
    T, S = K.N_SHAPE
    wmax, ok = H.band_facts(T, S, kw)
    lo, hi = H.band_tables(T, S)
    assert (T, S) == (10, 57) and wmax == 8 and not ok
    assert all(lo[i] >= lo[i - 1] for i in range(1, T)) and max(hi) - lo[0] == 57 > kw, "N fails the tile rule, not the ordering or the width"
    assert H.band_facts(T, S - 1, kw)[1] and all(H.band_facts(t, S, kw)[0] > 8 for t in range(1, T)), "one key fewer fits; fewer tokens widen the windows past 8"
    assert H.band_facts(70, 70, kw) == (3, True) and H.band_facts(33, 33, kw) == (3, True)   # S*, Q: the fused tail's band
    # Q: 2064 (sample, head, tile) triples, and more tiles than a sliced fused tail may have
    B, T = K.Q_SHAPE
    c2 = int(re.search(r"constexpr int CHAIN2_MAX_TILES = (\d+);", open(os.path.join(CSRC, "stchain.h")).read()).group(1))
    assert B * ((T + 31) // 32) > c2 and B * ((T + 31) // 32) * 6 >= 2048
    pq = _plan(planner, B, T)
    assert (pq["conv_in"], pq["in_layers"], pq["out_layers"], pq["qkv"]) == ("cgemm/2/8/1 block", F(2, 2), F(2, 2), F(3, 2))


def _calls(src, name):
    """The argument lists of every call of `name` in a source text."""
    out = []
    for m in re.finditer(r"\b" + name + r"\(", src):
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        out.append([a.strip() for a in src[m.end():i - 1].split(",")])
    return out


def test_mode_arguments_are_umode_values():
    """The product mode is the enum UMode everywhere: no call passes a bool, a literal, or the schedule's `bf` flag."""
    n = 0
    for fn in ("gemm_lds.hip", "unet_sched.cpp", "ugemm_plan.h"):
        with open(os.path.join(CSRC, fn)) as f:
            src = f.read()
        for name, pos in (("ugemm_supports", 4), ("launch_ugemm", 6)):
            for args in _calls(src, name):
                if args[0].startswith("const GemmArgs&"):   # the declaration / definition
                    continue
                assert len(args) > pos, (fn, name, args)   # the mode has no default
                mode = args[pos]
                assert mode in ("U_F32", "U_BF16", "U_SP", "m", "mode", "p.mode()"), (fn, name, args)
                n += 1
    assert n >= 8
