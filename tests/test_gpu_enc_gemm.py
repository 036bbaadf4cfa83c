"""enc_gemm.hip, the split-fp16 kernel of the fine-tuned encoder's dense products, through said_unet_train_dense_product
(said_amd/csrc/said_unet_train_products.h; run on the MI355X with `-m gpu`).

Each of the three layouts (forward, data gradient, weight gradient) at token rows 1 (a single row), 38 (less than a tile), 129 (one past a tile
multiple), 300 and 1281 (the first row count at which the weight gradient's K-split leaves an empty last chunk) with the weight (768, 768), and
at 300 rows with (768, 512), (3072, 768) and (768, 3072).  The result is held to tests/enc_split_ref.py's emulation of its own inputs (the
same split operands and scale rule, exact accumulation), so only the kernel's fp32 accumulation separates the two.  Bound: the kernel-test rule
of tests/test_gpu_audio_f32_kernels.py, max |got - emulation| / max |emulation| <= max(4 e32, 4e-6), e32 the same figure of numpy's fp32 product
of the same inputs against float64.  Activations are N(0, 1), weights N(0, 0.02^2), gradient operands 1e-5 N(0, 1).

Further: the scale rule (a gradient operand times 2^-40 gives 2^-40 times the result, bit for bit), exact zeros from an all-zero gradient, no
clamping of an activation past the fp16 range, the bias / residual / accumulate epilogues, bit-equal repetitions whatever the workspaces held,
and mode fp32 through the same entry: today's route (the same bits from a context that cannot run split products at all, inside the fp32
bound, and not the split result; the step-level side of it is tests/test_gpu_audio_finetune_split.py's switched-and-back case).

Measured (MI355X, kernel against the emulation; every case prints its own line): forward 2.2e-7 ... 7.4e-7 (the largest at K = 3072), data
gradient 3.1e-7 ... 9.0e-7 (N = 3072), weight gradient 2.7e-8 ... 1.8e-7, epilogues 1.1e-7 ... 1.9e-7; numpy's fp32 product is 2.7e-8 ... 9.9e-7
from float64, so the bound is its floor, 4e-6, in every case; the emulation is 7.1e-8 ... 1.2e-7 from float64.
"""
import numpy as np
import pytest
import torch

from said_amd import _engine
import enc_split_ref as esr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ["forward", "dgrad", "wgrad"]
SHAPES = [(rows, 768, 768) for rows in (1, 38, 129, 300, 1281)] + [(300, 768, 512), (300, 3072, 768), (300, 768, 3072)]


@pytest.fixture(scope="module")
def eng():
    e = _engine.UNetTrainEngine(torch.device(DEV), 2, 19, -1, 1)
    yield e
    e.close()


_OPS = {}


def operands(layout, rows, n, k, seed=0):
    """(a, b) of a layout: x / dy and W, or dy and x for the weight gradient."""
    key = (layout, rows, n, k, seed)
    if key not in _OPS:
        rng = np.random.default_rng(1000 * seed + rows + n + 7 * k)
        x = rng.standard_normal((rows, k)).astype(np.float32)
        dy = (1e-5 * rng.standard_normal((rows, n))).astype(np.float32)
        W = (0.02 * rng.standard_normal((n, k))).astype(np.float32)
        _OPS[key] = {"forward": (x, W), "dgrad": (dy, W), "wgrad": (dy, x)}[layout]
    return _OPS[key]


def held(what, got, layout, a, b, **epi):
    emu, f64, f32 = esr.emulate(layout, a, b, **epi), esr.exact(layout, a, b, **epi), esr.fp32(layout, a, b, **epi)
    e = float(np.abs(got - emu).max() / np.abs(emu).max())
    e32 = float(np.abs(f32 - f64).max() / np.abs(f64).max())
    bound = max(4 * e32, 4e-6)
    print(f"{what}: kernel vs emulation {e:.3e}, numpy fp32 vs float64 {e32:.3e}, emulation vs float64 "
          f"{float(np.abs(emu - f64).max() / np.abs(f64).max()):.3e}, bound {bound:.3e}")
    assert got.dtype == np.float32 and np.isfinite(got).all()
    assert e <= bound, (what, e, e32, bound)


@pytest.mark.parametrize("rows,n,k", SHAPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_product_against_the_emulation(eng, layout, rows, n, k):
    a, b = operands(layout, rows, n, k)
    got = eng.dense_product(layout, a, b, mode="split_fp16")
    held(f"{layout} rows {rows} W ({n}, {k})", got, layout, a, b)
    assert np.array_equal(got, eng.dense_product(layout, a, b, mode="split_fp16")), "a repetition gives other bits"


@pytest.mark.parametrize("layout", ["dgrad", "wgrad"])
def test_scale_rule(eng, layout):
    """The gradient operand times 2^-40: 2^-40 times the result, bit for bit; without the scale nothing of it would be left."""
    a, b = operands(layout, 300, 768, 768)
    a = a * np.float32(1e5)   # N(0, 1)
    small = a * np.float32(2.0 ** -40)
    want = eng.dense_product(layout, a, b, mode="split_fp16")
    got = eng.dense_product(layout, small, b, mode="split_fp16")
    assert float(np.abs(want).max()) > 0
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(want * np.float32(2.0 ** -40)))
    held(f"{layout} gradient x 2^-40", got, layout, small, b)


@pytest.mark.parametrize("layout", ["dgrad", "wgrad"])
def test_zero_gradient_gives_exact_zeros(eng, layout):
    a, b = operands(layout, 129, 768, 768)
    got = eng.dense_product(layout, np.zeros_like(a), b, mode="split_fp16")
    assert got.shape == ((129, 768) if layout == "dgrad" else (768, 768)) and not got.any()


def test_non_finite_gradient_gives_a_non_finite_result(eng):
    dy, W = operands("dgrad", 38, 768, 768)
    for bad in (np.inf, np.nan):
        g = dy.copy()
        g[5, 100] = bad
        got = eng.dense_product("dgrad", g, W, mode="split_fp16")
        assert not np.isfinite(got[5]).any(), bad
        assert np.isfinite(np.delete(got, 5, axis=0)).all(), "the scale of a non-finite operand is 1: the other rows stay finite"


def test_activation_past_the_fp16_range_is_not_clamped(eng):
    x, W = operands("forward", 129, 768, 768)
    x = x.copy()
    x[70, 300] = 1e5
    got = eng.dense_product("forward", x, W, mode="split_fp16")
    assert not np.isfinite(got[70]).any() and np.isfinite(np.delete(got, 70, axis=0)).all()
    dy, xa = operands("wgrad", 129, 768, 768)
    xa = xa.copy()
    xa[70, 300] = 1e5
    got = eng.dense_product("wgrad", dy, xa, mode="split_fp16")
    assert not np.isfinite(got[:, 300]).any() and np.isfinite(np.delete(got, 300, axis=1)).all()


def test_epilogues(eng):
    rows, n, k = 129, 768, 512
    rng = np.random.default_rng(5)
    x, W = operands("forward", rows, n, k)
    bias, res, out = (rng.standard_normal(s).astype(np.float32) for s in ((n,), (rows, n), (rows, n)))
    for what, epi in (("bias", dict(bias=bias)), ("bias + residual", dict(bias=bias, res=res)), ("residual", dict(res=res)),
                      ("bias + residual + accumulate", dict(bias=bias, res=res, out=out)), ("accumulate", dict(out=out))):
        held("forward " + what, eng.dense_product("forward", x, W, mode="split_fp16", **epi), "forward", x, W, **epi)
    # each term really is added: the bound above is relative to a range that the terms dominate
    plain = eng.dense_product("forward", x, W, mode="split_fp16").astype(np.float64)
    full = eng.dense_product("forward", x, W, mode="split_fp16", bias=bias, res=res, out=out).astype(np.float64)
    assert np.abs(full - (plain + bias + res + out)).max() <= 1e-6 * np.abs(full).max()
    dy, W = operands("dgrad", rows, n, k)
    acc = (1e-5 * rng.standard_normal((rows, k))).astype(np.float32)
    held("dgrad accumulate", eng.dense_product("dgrad", dy, W, mode="split_fp16", out=acc), "dgrad", dy, W, out=acc)
    lib = eng.lib
    for layout, kw in ((1, dict(bias=bias)), (2, dict(acc=1))):
        a, b = operands("dgrad" if layout == 1 else "wgrad", rows, n, k)
        y = np.zeros((rows, k) if layout == 1 else (n, k), dtype=np.float32)
        assert lib.said_unet_train_dense_product(eng.h, layout, rows, n, k, _engine._fp(a), _engine._fp(b), _engine._fp(kw.get("bias")), None,
                                                 kw.get("acc", 0), 1, _engine._fp(y)) != 0
    assert b"weight gradient does not accumulate" in lib.said_unet_train_last_error(eng.h)
    with pytest.raises(_engine.EngineError, match="multiples of 64"):
        eng.dense_product("forward", x[:, :96], W[:, :96], mode="split_fp16")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_result_does_not_depend_on_what_the_workspaces_held(eng, layout):
    """A product of another shape in between (it overwrites the partial tiles and the partial maxima), then the first one again."""
    a, b = operands(layout, 300, 768, 768)
    first = eng.dense_product(layout, a, b, mode="split_fp16")
    oa, ob = operands("wgrad", 1281, 3072, 768, seed=1)
    eng.dense_product("wgrad", oa * np.float32(1e9), ob, mode="split_fp16")
    oa, ob = operands("dgrad", 38, 768, 3072, seed=1)
    eng.dense_product("dgrad", oa * np.float32(1e-20), ob, mode="split_fp16")
    assert np.array_equal(first, eng.dense_product(layout, a, b, mode="split_fp16"))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_mode_fp32_is_todays_route(eng, layout):
    rows, n, k = 300, 768, 512
    a, b = operands(layout, rows, n, k)
    got = eng.dense_product(layout, a, b, mode="fp32")
    frozen = _engine.UNetTrainEngine(torch.device(DEV), 2, 19)   # no fine-tuned encoder: no split products at all
    try:
        assert np.array_equal(got, frozen.dense_product(layout, a, b, mode="fp32"))
        with pytest.raises(_engine.EngineError, match="need a context with a fine-tuned encoder"):
            frozen.dense_product(layout, a, b, mode="split_fp16")
    finally:
        frozen.close()
    f64, f32 = esr.exact(layout, a, b), esr.fp32(layout, a, b)
    e, e32 = float(np.abs(got - f64).max() / np.abs(f64).max()), float(np.abs(f32 - f64).max() / np.abs(f64).max())
    print(f"{layout} mode fp32: vs float64 {e:.3e}, numpy fp32 {e32:.3e}")
    assert e <= max(4 * e32, 4e-6)
    assert not np.array_equal(got, eng.dense_product(layout, a, b, mode="split_fp16")), "the two modes must be different arithmetic"
    # fp32 takes any width, as Gm's products do
    x, W = operands("forward", 38, 768, 768)
    y = eng.dense_product("forward", x[:, :100], W[:90, :100], mode="fp32")
    f64 = esr.exact("forward", x[:, :100], W[:90, :100])
    assert float(np.abs(y - f64).max() / np.abs(f64).max()) <= 4e-6


def test_setter_and_getter(eng):
    assert eng.encoder_products() == "fp32"
    eng.set_encoder_products("split_fp16")
    assert eng.encoder_products() == "split_fp16"
    eng.set_encoder_products("fp32")
    assert eng.encoder_products() == "fp32"
    assert eng.lib.said_unet_train_set_encoder_products(eng.h, 2) != 0 and b"unknown mode 2" in eng.lib.said_unet_train_last_error(eng.h)
    with pytest.raises(ValueError):
        eng.set_encoder_products("bf16")
