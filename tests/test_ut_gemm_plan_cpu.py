"""The K-split plan of the training step's weight gradients (said_amd/csrc/ut_gemm_plan.h) without a GPU: tests/ut_gemm_plan_main.cpp — the
header behind a command line, compiled once per session with the host compiler of the ROCm installation.

What the GPU module tests/test_gpu_unet_train_shapes.py cannot see from gradients alone is asserted here: that the chunks of every K up to
20000 partition [0, K), which K leave the last chunk empty (first 1281, never more than one), that no product of any tensor table outgrows the
partial-tile buffer at 16 chunks and which two fill it exactly, and that each shape of that module reaches the chunk count, the empty chunk
or the full buffer it is there for (tests/unet_train_shapes.py).

The kernel's reduction is restated in numpy float64 (16-wide k tiles, `k < kend` masking, chunk sums added in ascending order) on one linear
and one shifted-operand (k = 3 convolution) weight gradient at K = 1281, 2049 and 2052; it equals the plain product to 1e-12, and five
defects of it — the ones a regression of gemm_kernel / gemm_reduce_kernel would be — are each at least 50 x beyond the bound the GPU module
applies, 4 x max(the fp32 product's own error, 1e-6).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_weight_pack_cpu import _host_compiler  # noqa: E402
import unet_train_shapes as uts  # noqa: E402

ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "said_amd", "csrc")
KMAX = 20000
FS, LS = [-1, 16, 40, 1024], [0, 1, 2, 12]
PROJ, POSV = "audio_proj_layer.weight", "audio_encoder.encoder.pos_conv_embed.conv.weight_v"


@pytest.fixture(scope="session")
def planner(tmp_path_factory):
    """run(*args) -> stdout of the compiled tests/ut_gemm_plan_main.cpp."""
    cxx, inc = _host_compiler()
    exe = str(tmp_path_factory.mktemp("ut_gemm_plan") / "ut_gemm_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-x", "c++", f"-I{inc}", "-D__HIP_PLATFORM_AMD__", "-I" + CSRC, os.path.join(HERE, "ut_gemm_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout
    return run


@pytest.fixture(scope="session")
def sweep(planner):
    """({K: (KS, kchunk, empty)}, printed total, printed first) for K = 1 .. KMAX."""
    *rows, tail = planner("sweep", KMAX).splitlines()
    plan = {}
    for ln in rows:
        K, KS, kchunk, empty = map(int, ln.split())
        plan[K] = (KS, kchunk, empty)
    _, total, _, first = tail.split()
    return plan, int(total), int(first)


def products(planner, F, L, B, T):
    """(capacity, [dict per K-split product]) of the (F, L) context's step at B x T."""
    cap, *rows = planner("products", F, L, B, T).splitlines()
    out = []
    for ln in rows:
        name, kind, *v = ln.split()
        out.append(dict(zip(("M", "N", "Z", "K", "KS", "kchunk", "want", "need"), map(int, v)), name=name, kind=kind))
    return int(cap.split()[1]), out


def plan_py(K):
    """Gm::ksplit restated: min(16, K / 128) chunks, at least one, of ceil(K / KS) rounded up to the 16-wide k tile."""
    KS = min(16, max(1, K // 128))
    return KS, (-(-K // KS) + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------------------------- the partition
def test_chunks_partition_every_k(sweep):
    plan, _, _ = sweep
    assert sorted(plan) == list(range(1, KMAX + 1))
    for K, (KS, kchunk, _) in plan.items():
        assert (KS, kchunk) == plan_py(K), K
        assert kchunk % 16 == 0 and 1 <= KS <= 16
        edges = [(ks * kchunk, min(K, (ks + 1) * kchunk)) for ks in range(KS)]
        assert edges[0][0] == 0 and max(e for _, e in edges) == K, K
        # consecutive and disjoint wherever a chunk holds anything; a chunk that begins at or behind K holds nothing
        covered = 0
        for b, e in edges:
            if b < K:
                assert b == covered and e > b, (K, b, e)
                covered = e
        assert covered == K, K


def test_empty_chunks(sweep):
    plan, total, first = sweep
    empty = {K: sum(1 for ks in range(plan_py(K)[0]) if ks * plan_py(K)[1] >= K) for K in range(1, KMAX + 1)}
    assert {K: v[2] for K, v in plan.items()} == empty
    with_empty = [K for K in sorted(empty) if empty[K]]
    assert total == len(with_empty) and first == with_empty[0] == 1281
    assert max(empty.values()) == 1, "never more than one chunk is empty, and then it is the last"
    assert len([K for K in with_empty if K < 3601]) == 784
    print(f"K with an empty last chunk: {total} of {KMAX}, first {first}, 784 below 3601")


def test_capacity_lowers_the_chunk_count(planner):
    """The one addition to Gm::ksplit: fewer chunks when KS Z M N floats do not fit.  (No context reaches it: test_capacity.)"""
    full = 16 * 1024 * 768
    assert planner("ksplit", 2052, 1024, 768, 1, full).split() == ["16", "144"]
    assert planner("ksplit", 2052, 1024, 768, 1, full - 1).split() == ["15", "144"]
    assert planner("ksplit", 2052, 1024, 768, 1, 8 * 1024 * 768).split() == ["8", "272"]
    assert planner("ksplit", 2052, 1024, 768, 1, 0).split() == ["1", "2064"]
    assert planner("ksplit", 2052, 48, 6144, 16, 16 * 768 * 6144).split() == ["16", "144"]


# ---------------------------------------------------------------------------------------------------------------- the buffer
def weight_tensors(F, L):
    """{name: numel} of the tensors whose gradient is a matrix product: every weight of two or more dimensions."""
    from said_amd.training.unet import trainable_shapes
    return {k: int(np.prod(s)) for k, s in trainable_shapes(F, L).items()
            if len(s) >= 2 and k != "null_cond_emb" and not k.endswith("weight_g")}


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("F", FS)
def test_capacity(planner, F, L):
    """At 16 chunks (9 x 228) every weight gradient's partial tiles fit, so the lowering never acts; the command line's product list is the
    tensor table's."""
    cap, prods = products(planner, F, L, 9, 228)
    assert cap == (16 * 768 * 48 * 128 if L > 0 else 16 * max(F, 768) * 768)
    w = [p for p in prods if p["kind"] == "w"]
    numel = weight_tensors(F, L)
    assert sorted(p["name"] for p in w) == sorted(numel)
    full = set()
    for p in w:
        assert p["Z"] * p["M"] * p["N"] == numel[p["name"]], p
        assert p["KS"] == p["want"] and p["need"] == p["want"] * numel[p["name"]] <= cap, p
        assert p["want"] == (16 if p["K"] == 9 * 228 else 1), p
        if p["need"] == cap:
            full.add(p["name"])
    assert full == ({POSV} if L > 0 else {PROJ} if F == 1024 else set()), full
    # the products over the batch alone (K = B) at the largest batch a context admits: two chunks, far below the capacity
    _, big = products(planner, F, L, 256, 2)
    assert all(p["KS"] == p["want"] and p["need"] <= cap for p in big if p["kind"] == "w")
    assert {p["want"] for p in big if p["kind"] == "w" and p["K"] == 256} == {2}


# ---------------------------------------------------------------------------------------------------------------- the GPU module's shapes
def test_shape_claims(planner, sweep):
    plan, _, first = sweep
    assert [s.KS for s in uts.DEFAULT] == [1] + list(range(1, 17)) + [16, 16], "every chunk count from 1 to 16"
    for s in uts.DEFAULT:
        K = s.B * s.T
        KS, kchunk, empty = plan[K]
        filled = [min(K, (ks + 1) * kchunk) - ks * kchunk for ks in range(KS) if ks * kchunk < K]
        assert (KS, kchunk, bool(empty), filled[-1]) == (s.KS, s.kchunk, s.empty, s.last), s
        assert s.B <= uts.MAX_BATCH and s.T <= uts.MAX_FRAMES
        # every weight gradient over the tokens of that step runs this plan
        _, prods = products(planner, -1, 0, s.B, s.T)
        assert {(p["KS"], p["kchunk"]) for p in prods if p["K"] == K} == {(KS, kchunk)} and len([p for p in prods if p["K"] == K]) == 58
    by = {(s.B, s.T): s for s in uts.DEFAULT}
    assert by[3, 129].T % 64 == 1
    assert by[5, 131].last % 16 == 15 and by[7, 147].last == 21
    assert all(by[k].KS * by[k].kchunk == k[0] * k[1] for k in ((9, 128), (8, 240))), "exact chunks"
    assert 15 * by[4, 600].kchunk == 4 * 600, "the empty chunk begins exactly at K"
    assert 7 * 183 == first and by[7, 183].last % 16 == 1
    assert by[9, 228].last == 36 and by[3, 683].last % 16 == 1 and -(-683 // 64) == 11 and by[4, 600].kchunk == 160
    assert max(s.T for s in uts.DEFAULT) == uts.MAX_FRAMES and max(s.B for s in uts.DEFAULT) == uts.MAX_BATCH
    assert sum(s.empty for s in uts.DEFAULT) == 8
    assert set(uts.VARIANTS) <= set(by) and set(uts.ORDER) <= set(by)
    # feature_dim = 1024: the projection's partial tiles end on the buffer's last float
    B, T, F = uts.WIDE
    cap, prods = products(planner, F, 0, B, T)
    proj = [p for p in prods if p["name"] == PROJ]
    assert len(proj) == 1 and proj[0]["KS"] == 16 and proj[0]["KS"] * proj[0]["M"] * proj[0]["N"] == cap and plan[B * T][2] == 1
    # the fine-tuned encoder: the positional convolution's weight gradient likewise; its forward and data gradient around M = 256
    cap, prods = products(planner, -1, uts.FT_LAYERS, *uts.FT_FULL)
    pos = [p for p in prods if p["name"] == POSV]
    assert len(pos) == 1 and pos[0]["KS"] == 16 and pos[0]["KS"] * pos[0]["Z"] * pos[0]["M"] * pos[0]["N"] == cap
    assert [p["KS"] for p in prods if p["kind"] == "s"] == [1, 1]
    for B, T, ks in uts.FT_SMALL:
        _, prods = products(planner, -1, uts.FT_LAYERS, B, T)
        small = [p for p in prods if p["kind"] == "s"]
        assert [p["name"] for p in small] == ["pos_fwd", "pos_dgrad"] and all(p["M"] == B * T and p["KS"] == ks for p in small), (B, T, small)
        assert all(p["kchunk"] == (768 if ks == 8 else 6144) for p in small)
    assert [B * T for B, T, _ in uts.FT_SMALL] == [256, 257]


# ---------------------------------------------------------------------------------------------------------------- the kernel's arithmetic
def ksplit_product(A, Bm, K, KS, kchunk, defect=None, stale=None):
    """gemm_kernel + gemm_reduce_kernel restated: A (M, Kbuf), Bm (N, Kbuf) hold the operands by k (Kbuf >= K: what lies behind K must not be
    read); chunk ks sums 16-wide tiles over [ks kchunk, min(K, (ks + 1) kchunk)) with k >= kend masked to zero and stores its partial tile;
    the partial tiles are added in ascending ks.  `stale`: what the partial-tile buffer held before the call.  `defect`: one of DEFECTS."""
    M, N = A.shape[0], Bm.shape[0]
    part = np.array(stale[:KS], dtype=np.float64) if stale is not None else np.full((KS, M, N), np.nan)
    last_filled = max(ks for ks in range(KS) if ks * kchunk < K)
    for ks in range(KS):
        kbeg = ks * kchunk
        kend = kbeg + kchunk if defect == "unclamped" else min(K, kbeg + kchunk)
        if defect == "stale" and kbeg >= K:
            continue                                   # the empty chunk's workgroup stores nothing
        acc = np.zeros((M, N))
        for k0 in range(kbeg, kend, 16):
            if defect == "tail" and ks == last_filled and k0 + 16 > kend:
                continue                               # the partly valid tile that ends the last chunk
            k = np.arange(k0, k0 + 16)
            ok = k < kend
            kc = np.minimum(k, A.shape[1] - 1)
            acc += np.where(ok, A[:, kc], 0.0) @ np.where(ok, Bm[:, kc], 0.0).T
        part[ks] = acc
    out = np.zeros((M, N))
    for ks in range(KS):
        out += part[ks]
    if defect == "twice":
        out += part[KS // 2]
    return out


DEFECTS = ["tail", "unclamped", "stale", "twice", "boundary"]


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def operands(kind, B, T, rng, boundary=True):
    """(A, Bm, plain float64 product) of a weight gradient over K = B T tokens, the operand buffers padded with values that are not part of
    the product up to the next multiple of 16 x 16 chunks.  linear: dW = dy^T x.  conv: dW[co, (ci, j)] = sum_(b, t) dy[b, t, co]
    x[b, t + j - 1, ci], zero outside the sample (boundary=False: the neighbouring sample's rows instead)."""
    K, Kbuf = B * T, (B * T // 256 + 2) * 256
    if kind == "linear":
        dy, x = rng.standard_normal((Kbuf, 37)), rng.standard_normal((Kbuf, 29))
        A, Bm = dy.T.copy(), x.T.copy()
    else:
        Co, Ci = 19, 7
        dy, x = rng.standard_normal((Kbuf, Co)), rng.standard_normal((Kbuf, Ci))
        A = dy.T.copy()
        Bm = np.zeros((Ci, 3, Kbuf))
        tok = np.arange(Kbuf)
        for j in range(3):
            src = tok + j - 1
            inside = (src >= 0) & (src < Kbuf)
            if boundary:
                inside &= (tok % T + j - 1 >= 0) & (tok % T + j - 1 < T)
            Bm[:, j, inside] = x[src[inside]].T
        Bm = Bm.reshape(Ci * 3, Kbuf)
    return A, Bm, A[:, :K] @ Bm[:, :K].T


@pytest.mark.parametrize("B,T", [(7, 183), (3, 683), (9, 228)])
@pytest.mark.parametrize("kind", ["linear", "conv"])
def test_restated_kernel_and_its_defects(sweep, kind, B, T):
    plan, _, _ = sweep
    K = B * T
    assert K in (1281, 2049, 2052)
    KS, kchunk, empty = plan[K]
    assert empty == 1
    rng = np.random.default_rng(K + len(kind))
    A, Bm, want = operands(kind, B, T, rng)
    stale = rng.standard_normal((16, A.shape[0], Bm.shape[0])) * np.abs(want).mean()     # an earlier call's partial tiles
    got = ksplit_product(A, Bm, K, KS, kchunk, stale=stale)
    assert rel(got, want) <= 1e-12, rel(got, want)
    e32 = rel((A[:, :K].astype(np.float32) @ Bm[:, :K].astype(np.float32).T).astype(np.float64), want)
    bound = 4 * max(e32, 1e-6)
    for d in DEFECTS:
        if d == "boundary":
            if kind != "conv":
                continue
            A2, B2, _ = operands(kind, B, T, np.random.default_rng(K + len(kind)), boundary=False)
            assert np.array_equal(A2, A)
            bad = ksplit_product(A2, B2, K, KS, kchunk, stale=stale)
        else:
            bad = ksplit_product(A, Bm, K, KS, kchunk, defect=d, stale=stale)
        factor = rel(bad, want) / bound
        print(f"{kind} K={K} KS={KS}: defect '{d}' is {factor:.0f} x the bound {bound:.1e}")
        assert factor >= 50, (d, factor)
