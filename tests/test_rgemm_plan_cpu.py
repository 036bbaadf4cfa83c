"""The host-side decisions of rgemm_kernel (said_amd/csrc/rgemm_plan.h) without a GPU: tests/rgemm_plan_main.cpp — the header behind a command line, compiled once per
session with the host compiler of the ROCm installation — against tests/golden/rgemm_plan.txt.

The fixture holds (variant, row tiles per range, grid, column groups) of every rgemm_kernel launch of the shapes tests/test_gpu_unet_bf16_kernels.py runs — S, G, T6
(forward and guided) — and of the two tile-walk shapes P (260 x 40) and Z (1300 x 20), recorded from the header as it was moved out of rgemm.hip unchanged.  What the
GPU test cannot see from the stage log — which of the thirteen instantiations a launch takes, how many tiles a workgroup walks and over how many samples — is
asserted here: every variant is reached by some shape, P walks three tiles per range with ranges that start in the middle of a sample, Z walks six one-tile samples
per range, so that the four-slot ring of GroupNorm tables wraps."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_weight_pack_cpu import _host_compiler  # noqa: E402

ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "said_amd", "csrc")
FIXTURE = os.path.join(HERE, "golden", "rgemm_plan.txt")
#         tag: Be, Bc, T, six-launch tail
SHAPES = {"S": (3, 0, 70, 0), "G": (4, 2, 70, 0), "T6": (3, 0, 70, 1), "T6-G": (4, 2, 70, 1), "P": (260, 0, 40, 1), "Z": (1300, 0, 20, 1)}


@pytest.fixture(scope="session")
def planner(tmp_path_factory):
    """run(*args) -> stdout of the compiled tests/rgemm_plan_main.cpp."""
    cxx, inc = _host_compiler()
    exe = str(tmp_path_factory.mktemp("rgemm_plan") / "rgemm_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-x", "c++", f"-I{inc}", "-D__HIP_PLATFORM_AMD__", "-I" + CSRC, os.path.join(HERE, "rgemm_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout
    return run


def _parse(line):
    name, v, shape, *kv = line.split()
    d = {k: int(x) for k, x in (f.split("=") for f in kv)}
    d.update(name=name, variant=int(v[1:]), shape=tuple(int(x) for x in shape.split(",")))
    return d


def _fixture():
    by = {}
    with open(FIXTURE) as f:
        for ln in f.read().splitlines():
            tag, rest = ln.split(" ", 1)
            by.setdefault(tag, []).append(rest)
    return by


def test_plans_are_the_recorded_ones(planner):
    want = _fixture()
    assert set(want) == set(SHAPES)
    for tag, args in SHAPES.items():
        got = planner(*args).splitlines()
        assert got == want[tag], tag
        assert not any("unserved" in ln for ln in got), tag


def test_launch_counts_match_the_schedules():
    """rgemm launches per shape: 14 ResBlock launches, four q/k/v; the six-launch tail adds six per block (four in forward()'s last block, which ends on xgemm_kernel);
    forward()'s last block runs its four even when the other tails are fused."""
    n = {tag: len(v) for tag, v in _fixture().items()}
    assert n == {"S": 14 + 4 + 4, "G": 14 + 4, "T6": 14 + 4 + 3 * 6 + 4, "T6-G": 14 + 4 + 4 * 6, "P": 14 + 4 + 3 * 6 + 4, "Z": 14 + 4 + 3 * 6 + 4}


def test_every_variant_is_reached():
    """The thirteen instantiations of RG_VARIANTS, each with the shape it was written for."""
    with open(os.path.join(CSRC, "rgemm_plan.h")) as f:
        src = f.read()
    assert src.count("    X(") == 13
    seen = {}
    for tag, lines in _fixture().items():
        for ln in lines:
            d = _parse(ln)
            seen.setdefault(d["variant"], set()).add(tag)
            assert d["variant"] >= 0
    assert set(seen) == set(range(13)), seen
    by_name = {(tag, _parse(ln)["name"]): _parse(ln) for tag, lines in _fixture().items() for ln in lines}
    assert by_name["G", "res0.conv2"]["shape"] == (3, 0, 1, 1, 1, 1, 1)           # the duplicate-store convolution: the guided step's shared first block
    assert by_name["T6-G", "st0.out1"]["shape"] == (1, 0, 0, 2, 1, 0, 1)          # to_out + GroupNorm'ed residual + the c2 duplicate
    assert by_name["T6", "st0.out1"]["shape"] == (1, 0, 0, 2, 0, 0, 1)
    assert by_name["S", "res3.skip"]["shape"] == (1, 0, 0, 0, 0, 0, 2) and by_name["S", "res3.conv1a"]["shape"] == (3, 0, 1, 0, 0, 0, 1)
    assert by_name["T6", "st0.proj_h"]["shape"] == (1, 0, 0, 1, 0, 0, 4) and by_name["T6", "st0.proj_x"]["shape"] == (1, 0, 0, 1, 0, 1, 1)
    assert by_name["S", "st3.band"]["shape"] == (1, 4, 2, 0, 0, 0, 1) and by_name["S", "st3.geglu"]["shape"] == (1, 2, 2, 0, 0, 0, 1) and by_name["S", "st3.geglu"]["groups"] == 4
    assert by_name["S", "st0.qkv"]["shape"] == (1, 1, 3, 0, 0, 0, 1)
    # the guided step's shared block computes the clips alone; the cross-attention launches the conditional half alone
    assert by_name["G", "res0.conv1"]["batch"] == 2 and by_name["G", "res1.conv1"]["batch"] == 4 and by_name["T6-G", "st1.band"]["batch"] == 2 and by_name["T6-G", "st1.out1"]["batch"] == 4


def test_tile_walks_of_p_and_z():
    """P: per = 3 over two-tile samples — ranges start in the middle of a sample and a new sample's GroupNorm tables are made inside the loop.  Z: per = 6 over one-tile
    samples — a range walks six samples, two more than the table ring (sample & 3) has slots.  The toy shapes walk one tile per range."""
    fx = _fixture()
    for tag in ("S", "G", "T6", "T6-G"):
        assert {_parse(ln)["per"] for ln in fx[tag]} == {1}
    for ln in fx["P"]:
        d = _parse(ln)
        if d["groups"] == 1:
            assert (d["per"], d["spr"], d["grid"]) == (3, 2, 176), ln       # 520 tiles in 174 ranges, the grid padded to a multiple of 8
        else:
            assert (d["per"], d["groups"], d["grid"]) == (9, 4, 256), ln    # GEGLU: four column groups of 64 workgroups
    B, _, T, _ = SHAPES["P"]
    ntv, per = (T + 31) // 32, _parse(fx["P"][0])["per"]
    assert ntv == 2 and sum(1 for r in range(-(-B * ntv // per)) if (r * per) % ntv) >= 80, "ranges that start in the middle of a sample (every second one)"
    for ln in fx["Z"]:
        d = _parse(ln)
        if d["groups"] == 1:
            assert (d["per"], d["spr"], d["grid"]) == (6, 6, 224), ln
            assert d["spr"] > 4, "the ring of four table slots wraps inside a range"
        else:
            assert (d["per"], d["spr"]) == (21, 21), ln
