"""The weight layouts of said_amd/csrc/weight_pack.h, byte for byte, without a GPU: tests/weight_pack_main.cpp (the header behind a command line, compiled
once per session with the host compiler of the ROCm installation) against tests/weight_pack_ref.py (the layouts as numpy index arithmetic).  No tolerance:
numpy's float16 and torch's bfloat16 roundings are the host compiler's, ties included."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import weight_pack_ref as ref  # noqa: E402


def _host_compiler():
    from said_amd.build import _hipcc
    hipcc = _hipcc()
    for d in (os.path.dirname(hipcc), os.path.dirname(os.path.realpath(hipcc))):
        for rel in ("clang++", "amdclang++", "../llvm/bin/clang++", "../lib/llvm/bin/clang++"):
            exe = os.path.join(d, rel)
            if os.path.exists(exe):
                return os.path.normpath(exe), os.path.normpath(os.path.join(d, "..", "include"))
    raise RuntimeError(f"no clang++ beside {hipcc}")


@pytest.fixture(scope="session")
def packer(tmp_path_factory):
    """run(*args): the compiled tests/weight_pack_main.cpp."""
    cxx, inc = _host_compiler()
    exe = str(tmp_path_factory.mktemp("weight_pack") / "weight_pack_main")
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-x", "c++", f"-I{inc}", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "said_amd", "csrc"),
           os.path.join(HERE, "weight_pack_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stderr)
    return run


def _weights(seed, shape, n_halfway):
    """Seeded normal draws with n_halfway elements forced onto exact fp16 half-way points."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(shape) * 0.25).astype(np.float32)
    idx = rng.choice(w.size, n_halfway, replace=False)
    w.reshape(-1)[idx] = ref.fp16_halfway(rng, n_halfway)
    return w


def _same(path, want, dtype):
    got = np.fromfile(path, dtype=dtype)
    want = np.ascontiguousarray(want).reshape(-1)
    assert want.dtype == dtype and got.shape == want.shape, (path, got.shape, want.shape)
    bits = {2: np.uint16, 4: np.uint32}[np.dtype(dtype).itemsize]
    assert np.array_equal(got.view(bits), want.view(bits)), path


@pytest.mark.parametrize("taps", [3, 1])
@pytest.mark.parametrize("c_begin", [0, 48])
def test_fragment_layouts(packer, tmp_path, taps, c_begin):
    """N = 40: two row tiles, rows 40 .. 63 zero; Ctot = 96 as two segments of 48 (the second with c_begin = 48).  C = 48 is two 24-channel blocks: with 3 taps
    5 steps per block and groups 9 and above zero, with 1 tap 2 steps and group 3 zero; the flat layout (1 tap) has 3 steps and no padding."""
    N, Ctot, C = 40, 96, 48
    W = _weights(10 + taps, (N, Ctot, taps), 300)
    W.tofile(tmp_path / "w.f32")
    out = str(tmp_path / "o")
    packer("frag", tmp_path / "w.f32", Ctot, taps, N, 0, c_begin, C, out)
    want = ref.rows(W, N, c_begin, C)
    assert want.shape == (2, taps, 24, 64) and not want[1, :, :, 8:32].any() and not want[1, :, :, 40:].any() and want[1, :, :, :8].any()
    _same(out + ".rows", want, np.float32)
    _same(out + ".rows4", ref.rows4(W, N, c_begin, C), np.float32)
    _same(out + ".bf16", ref.rows_bf16(W, N, c_begin, C), np.uint16)
    blk = ref.rows_split_block(W, N, c_begin, C)
    assert blk.shape == (2, 2, 5 if taps == 3 else 2, 2, 64, 8)
    assert not blk[:, :, -1, :, 32:].any() and blk[0, :, -1, 0, :32].any()   # the last step's upper group (9 of 0 .. 8, or 3 of 0 .. 2) is padding
    _same(out + ".split_block", blk, np.uint16)
    if taps == 1:
        _same(out + ".split_flat", ref.rows_split_flat(W, N, c_begin, C), np.uint16)
    else:
        assert not os.path.exists(out + ".split_flat")


def test_grouped_rows(packer, tmp_path):
    """rows_dense(48, 48): the positional convolution's second group — rows 48 .. 95 of a [96][48][K] weight, its second tile half empty."""
    K = 4
    W = _weights(3, (96, 48, K), 100)
    W.tofile(tmp_path / "w.f32")
    packer("frag", tmp_path / "w.f32", 48, K, 48, 48, 0, 48, tmp_path / "g")
    want = ref.rows(W, 48, 0, 48, row0=48)
    assert want.shape == (2, K, 24, 64) and want[0, 0, 0, 0] == W[48, 0, 0] and want[1, 0, 0, 15] == W[95, 0, 0] and not want[1, :, :, 16:32].any()
    _same(str(tmp_path / "g.rows"), want, np.float32)


def test_token_major_pair(packer, tmp_path):
    """upload_tm_pair's three copies: the tap-major reordering, its bf16 rounding and the packed split-fp16 words h | l << 16."""
    N, C, taps = 40, 48, 3
    W = _weights(5, (N, C, taps), 300)
    W.tofile(tmp_path / "w.f32")
    packer("tm", tmp_path / "w.f32", N, C, taps, tmp_path / "t")
    tm = ref.tap_major(W)
    assert tm.shape == (N, taps, C) and tm[7, 2, 5] == W[7, 5, 2]
    _same(str(tmp_path / "t.tm"), tm, np.float32)
    _same(str(tmp_path / "t.bf16"), ref.bf16_bits(tm), np.uint16)
    words = ref.split_words(tm)
    h, lo = ref.split_planes(tm)
    assert np.array_equal(words & 0xFFFF, h) and np.array_equal(words >> 16, lo)
    _same(str(tmp_path / "t.words"), words, np.uint32)


@pytest.fixture(scope="session")
def chain(packer, tmp_path_factory):
    """The fused tail's operands at the model's sizes (its layout is fixed to them), the packed files and the reference, made once."""
    d = tmp_path_factory.mktemp("chain")
    MC, FFI = ref.MC, ref.FFI
    rng = np.random.default_rng(77)
    t = {"out1": _weights(1, (MC, MC), 300), "q": _weights(2, (MC, MC), 300), "out2": _weights(3, (MC, MC), 300), "ff": _weights(4, (2 * FFI, MC), 600),
         "ffproj": _weights(5, (MC, FFI + MC), 600)}
    for k, n in (("b1", MC), ("b3", MC), ("c2", MC), ("ffproj_b", MC), ("ffb", 2 * FFI), ("be2", MC), ("be3", MC)):
        t[k] = (rng.standard_normal(n) * 0.3).astype(np.float32)
    for k in ("g2", "g3"):   # gammas away from 1; every fourth a power of two, so that the half-way points of those columns survive the fold
        g = (1 + 0.3 * rng.standard_normal(MC)).astype(np.float32)
        g[::4] = np.float32(2.0) ** rng.integers(-2, 3, MC // 4)
        t[k] = g
    for k, rows in (("q", MC), ("ff", 2 * FFI)):
        n = 400
        t[k][rng.integers(0, rows, n), 4 * rng.integers(0, MC // 4, n)] = ref.fp16_halfway(rng, n)
    for k, v in t.items():
        v.tofile(d / (k + ".f32"))
    packer("chain", d)
    want, mats = ref.chain_streams(t)
    return d, want, mats


def test_chain_operands_exercise_the_ties_and_the_folds(chain):
    _, _, mats = chain
    for m in mats:
        assert int(ref.is_fp16_halfway(m).sum()) >= 200
    for slices, n in ((1, 1152), (3, 3 * 528), (2, 2 * 684)):
        u = ref.chain_units(slices)
        assert len(u) == n
        # every slice count covers every (matrix, row tile, step) of GEGLU and the folded proj_out exactly once, and the three projections once per slice
        for m, tiles, steps, times in ((ref.GEGLU, 48, 12, 1), (ref.FFPROJ, 6, 60, 1), (ref.OUT1, 6, 12, slices), (ref.Q, 6, 12, slices), (ref.OUT2, 6, 12, slices)):
            sel = u[u[:, 0] == m]
            keys, counts = np.unique(sel[:, 1] // 32 * 64 + sel[:, 2], return_counts=True)
            assert len(keys) == tiles * steps and (counts == times).all(), (slices, m)


@pytest.mark.parametrize("name", ["stream1", "stream3", "stream2", "stream_bf16"])
def test_chain_stream(chain, name):
    d, want, _ = chain
    _same(str(d / (name + ".bin")), want[name], np.uint16)


def test_chain_vec(chain):
    d, want, _ = chain
    assert want["vec"].shape == (5 * ref.MC + 2 * ref.FFI,)
    _same(str(d / "vec.bin"), want["vec"], np.float32)
