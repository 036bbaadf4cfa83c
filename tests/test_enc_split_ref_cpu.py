"""tests/enc_split_ref.py, the numpy emulation that tests/test_gpu_enc_gemm.py holds enc_gemm.hip to: what split-fp16 operands and the scale
rule of the gradient operands give (said_amd/csrc/said_unet_train_products.h).  Error is |got - f64|_2 / |f64|_2 of
N(0, 1) against N(0, 0.02^2) operands, the product taken as (R, S) = sum_k a[r, k] b[s, k] at (R, S, K) = (38, 768, 768), (300, 3072, 768) and
(768, 768, 1281): a projection's forward, a feed-forward layer's, and a weight gradient over 1281 tokens."""
import numpy as np
import pytest

import enc_split_ref as esr

SHAPES = [(38, 768, 768), (300, 3072, 768), (768, 768, 1281)]


def operands(shape, seed=0):
    R, S, K = shape
    rng = np.random.default_rng(seed)
    return rng.standard_normal((R, K)).astype(np.float32), (0.02 * rng.standard_normal((S, K))).astype(np.float32)


def err(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


@pytest.mark.parametrize("shape", SHAPES)
def test_split_product_is_below_the_fp32_products_own_error(shape):
    a, b = operands(shape)
    want = a.astype(np.float64) @ b.astype(np.float64).T
    e_split, e_f32 = err(esr.product(a, b), want), err((a @ b.T).astype(np.float64), want)
    print(shape, "split-fp16", e_split, "numpy fp32", e_f32)
    assert e_split < e_f32 and e_split < 2e-7


def test_unscaled_small_gradient_loses_its_digits():
    a, b = operands(SHAPES[0])
    for k, lo, hi in ((20, 1e-6, 1e-4), (30, 1e-3, 1e-1)):
        g = a * np.float32(2.0 ** -k)
        want = g.astype(np.float64) @ b.astype(np.float64).T
        e = err(esr.product(g, b), want)
        print(f"gradient x 2^-{k}, unscaled:", e)
        assert lo < e < hi
    g = a * np.float32(2.0 ** -40)
    assert not esr.product(g, b).any(), "at 2^-40 nothing is left of an unscaled gradient"


@pytest.mark.parametrize("k", [0, 20, 30, 40])
def test_scaled_gradient_equals_the_unscaled_magnitude_case_to_the_last_digit(k):
    dy, W = operands((38, 768, 768))   # dy (38, 768), W^T as (768, 768)
    x = operands((38, 512, 768), 1)[0]
    g = dy * np.float32(2.0 ** -k)
    s = esr.scale_of(g)
    assert 2.0 ** 14 <= float(np.abs(g).max()) * s < 2.0 ** 15 and s == esr.scale_of(dy) * 2.0 ** k
    assert np.array_equal(esr.dgrad(g, W), esr.dgrad(dy, W) * 2.0 ** -k)
    assert np.array_equal(esr.wgrad(g, x), esr.wgrad(dy, x) * 2.0 ** -k)
    want = g.astype(np.float64) @ W.astype(np.float64)
    assert err(esr.dgrad(g, W), want) < 1e-7


def test_scale_of_zero_and_non_finite_operands_is_one():
    z = np.zeros((5, 64), dtype=np.float32)
    assert esr.scale_of(z) == 1.0
    W = operands((5, 64, 64))[1]
    assert not esr.dgrad(z, W).any() and not esr.wgrad(z, W[:5]).any()
    for bad in (np.inf, -np.inf, np.nan):
        z2 = z.copy()
        z2[1, 2] = bad
        assert esr.scale_of(z2) == 1.0
        assert not np.isfinite(esr.dgrad(z2, W)[1]).any()
    tiny = np.full((2, 64), 1e-44, dtype=np.float32)   # an fp32 denormal: the scale is capped so that its inverse stays normal
    assert esr.scale_of(tiny) == 2.0 ** 126


def test_an_activation_past_the_fp16_range_is_not_clamped():
    x, W = operands((4, 64, 64))
    x[2, 7] = 1e5
    y = esr.forward(x, W)
    assert not np.isfinite(y[2]).any() and np.isfinite(np.delete(y, 2, axis=0)).all()
