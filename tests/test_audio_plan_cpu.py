"""The launch plan of the fp32 audio encoder (said_amd/csrc/audio_plan.h) without a GPU: tests/audio_plan_main.cpp — the header behind a command line,
compiled once per session with the host compiler of the ROCm installation.

tests/test_gpu_audio_f32_kernels.py names each of its shapes for the (NB, KS) tile shapes and the key-slice count it reaches (audio_f32_ref.SHAPES); here
every one of those claims is asked of the header that audio_enc.cpp launches by, so a threshold that moves shows up as a shape that no longer reaches its
instantiation, not as a silently thinner GPU test.  Also: at which token-tile counts launch_gemm would drop a requested tile shape back to (1, 8) for the
encoder's sites (none), and which passes of the suite's largest encode (32 clips x 600 frames) and of the bench's take which key-slice count.
"""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_weight_pack_cpu import _host_compiler  # noqa: E402
import audio_f32_ref as R  # noqa: E402

ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "said_amd", "csrc")


@pytest.fixture(scope="session")
def planner(tmp_path_factory):
    """run(*args) -> stdout of the compiled tests/audio_plan_main.cpp."""
    cxx, inc = _host_compiler()
    exe = str(tmp_path_factory.mktemp("audio_plan") / "audio_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-x", "c++", f"-I{inc}", "-D__HIP_PLATFORM_AMD__", "-I" + CSRC, os.path.join(HERE, "audio_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout
    return run


def plan(planner, nb, Ta, frames):
    """{site: dict(tiles, asked, runs)} and the attention line's dict(tiles, ks, ks_train) under "attn"; "frames" / "pitch" as ints."""
    head, *rows = planner("plan", nb, Ta, frames or 0).splitlines()
    out = {k: int(v) for k, v in (f.split("=") for f in head.split())}
    for ln in rows:
        name, *f = ln.split()
        d = dict(x.split("=") for x in f)
        out[name] = {k: (int(v) if "/" not in v else tuple(map(int, v.split("/")))) for k, v in d.items()}
    return out


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_every_gpu_shape_lands_where_it_is_named_for(planner, name):
    sh = R.SHAPES[name]
    passes = [min(sh["chunk"], sh["B"] - b0) for b0 in range(0, sh["B"], sh["chunk"])]
    assert passes == sh["passes"]
    p = plan(planner, passes[0], sh["Ta"], sh["frames"])
    print(name, p)
    L = R.conv_lengths(sh["Ta"])
    Fr = sh["frames"] or L[6]
    assert (p["frames"], p["pitch"]) == (Fr, (Fr + 31) // 32 * 32)
    assert p["attn"]["tiles"] == sh["tiles"] == passes[0] * ((Fr + 31) // 32)
    for site, want in sh["plan"].items():
        if site == "attn":
            assert p["attn"]["ks"] == want, (name, p["attn"])
        else:
            assert p[site]["asked"] == p[site]["runs"] == want, (name, site, p[site])
    # every site is named
    assert set(sh["plan"]) == {f"conv{i}" for i in range(1, 7)} | {"fproj", "pos", "qkv", "attn", "out", "ff1", "ff2", "proj"}


def test_shape_claims():
    """What the shapes are chosen for, beyond the plan lines."""
    S, N, M, D, C, K = (R.SHAPES[k] for k in "SNMDCK")
    assert R.conv_lengths(N["Ta"])[6] == 24 and N["frames"] is None, "N runs on its own 24 frames: 8 pad rows up to the pitch of 32"
    assert D["tiles"] * 12 == 2052, "one (clip, head, tile) triple past the eight-slice limit of 2048"
    assert D["tiles"] * 24 == 4104, "one token tile past pick_cfg's 4096 for the 768-wide GEMMs"
    assert 9 * ((R.conv_lengths(C["Ta"])[1] + 31) // 32) == 450
    assert K["tiles"] == 688 and K["tiles"] * 12 > 8192 >= 682 * 12
    assert M["tiles"] * 96 > 1536 >= M["tiles"] * 24
    assert {sh["plan"]["attn"] for sh in R.SHAPES.values()} == {8, 4, 1}
    ran = {v for sh in R.SHAPES.values() for k, v in sh["plan"].items() if k != "attn"}
    assert ran == {(1, 8), (2, 8), (4, 4), (6, 4)}, ran


def test_key_slice_thresholds(planner):
    """Eight slices up to 170 token tiles per pass, four up to 682, none above; train mode with attention dropout never drops the split."""
    def ks(tt):
        return plan(planner, tt, 400, 32)["attn"]
    assert [ks(t)["ks"] for t in (1, 170, 171, 682, 683, 5000)] == [8, 8, 4, 4, 1, 1]
    assert [ks(t)["ks_train"] for t in (1, 170, 171, 682, 683, 5000)] == [8, 8, 4, 4, 4, 4]
    # the largest pass of any other test, 32 clips x 600 frames, is 608 tiles: four slices.  No key split needs more than 682 tiles in ONE pass:
    # 32 clips of more than 11.2 s at 60 frames / s (22 tiles each), or an audio_chunk above the default
    assert plan(planner, 32, 160000, 600)["attn"] == {"tiles": 608, "ks": 4, "ks_train": 4}
    assert plan(planner, 32, 160000, 673)["attn"]["ks"] == 1 and plan(planner, 32, 160000, 672)["attn"]["ks"] == 4


def test_launch_gemm_never_falls_back_for_the_encoder(planner):
    """launch_gemm drops a tile shape that cgemm_kernel is not instantiated for back to (1, 8).  For the encoder's sites that happens at no token-tile
    count: every (NB, KS) that pick_cfg, the q/k/v rule and the positional convolution's rule can ask for is in the list."""
    rows = {ln.split()[0]: dict(f.split("=") for f in ln.split()[1:]) for ln in planner("fallback", 20000).splitlines()}
    print(rows)
    assert set(rows) == {"conv", "fproj", "pos", "qkv", "out", "ff1", "ff2", "proj"}
    assert all(r == {"n": "0", "first": "0"} for r in rows.values()), rows
