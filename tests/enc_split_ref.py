"""numpy emulation of the fine-tuned encoder's split-fp16 dense products (said_amd/csrc/enc_gemm.hip, said_unet_train_products.h).

An fp32 operand x is split into two fp16 planes, h = fp16(x) and l = fp16((x - h) * 2048), fp16 denormals kept, so that x ~= h + 2^-11 l;
a product is h_a . h_b + 2^-11 (h_a . l_b + l_a . h_b).  The planes' products are exact in float64 and the sums run in float64 ("exact
accumulation"): what separates the kernel from this emulation is its fp32 accumulation alone.

A gradient operand (dy of a data or weight gradient) is multiplied before the split by the power of two that brings its largest magnitude into
[2^14, 2^15) (scale_of), and the product by the inverse.  Zero and non-finite operands take scale 1.
"""
import numpy as np


def split(x):
    """(h, l) of an fp32 array as float64 arrays; |x| >= 65520 gives h = inf and l = nan, as the conversion on the GPU does."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = x.astype(np.float16)
        l = ((x - h.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    return h.astype(np.float64), l.astype(np.float64)


def scale_of(g):
    """The power of two a gradient operand is multiplied by: its largest magnitude lands in [2^14, 2^15); 1.0 for an all-zero or a
    non-finite operand; at most 2^126, so that the inverse is a normal fp32 number."""
    amax = float(np.max(np.abs(np.asarray(g, dtype=np.float32)), initial=0.0))
    if amax == 0.0 or not np.isfinite(amax):
        return 1.0
    _, e = np.frexp(amax)   # amax = m 2^e, m in [0.5, 1)
    return float(2.0 ** min(15 - int(e), 126))


def product(a, b, scale_a=1.0):
    """sum_k a[r, k] b[s, k] on split operands, (R, S) float64; a is multiplied by scale_a before the split and the result divided by it."""
    a = (np.asarray(a, dtype=np.float32) * np.float32(scale_a)).astype(np.float32)
    ah, al = split(a)
    bh, bl = split(b)
    with np.errstate(invalid="ignore", over="ignore"):
        return (ah @ bh.T + (ah @ bl.T + al @ bh.T) / 2048.0) / scale_a


def forward(x, W, bias=None, res=None, out=None):
    """x (M, K) W^T (W: N x K) + bias (+ res) (+ out)"""
    y = product(x, W)
    for t in (bias, res, out):
        if t is not None:
            y = y + np.asarray(t, dtype=np.float64)
    return y


def dgrad(dy, W, out=None, scaled=True):
    """dy (M, N) W (N, K) (+ out); scaled=False: the gradient operand is split as it is (what the scale rule is there to avoid)"""
    y = product(dy, np.asarray(W).T, scale_of(dy) if scaled else 1.0)
    return y if out is None else y + np.asarray(out, dtype=np.float64)


def wgrad(dy, x, scaled=True):
    """dy^T (M, N) x (M, K): (N, K)"""
    return product(np.asarray(dy).T, np.asarray(x).T, scale_of(dy) if scaled else 1.0)


def exact(layout, a, b, bias=None, res=None, out=None):
    """The same product of the fp32 inputs in float64, without any split."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    y = a @ b.T if layout == "forward" else a @ b if layout == "dgrad" else a.T @ b
    for t in (bias, res, out):
        if t is not None:
            y = y + np.asarray(t, dtype=np.float64)
    return y


def fp32(layout, a, b, bias=None, res=None, out=None):
    """numpy's fp32 product of the same inputs."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    y = a @ b.T if layout == "forward" else a @ b if layout == "dgrad" else a.T @ b
    for t in (bias, res, out):
        if t is not None:
            y = y + np.asarray(t, dtype=np.float32)
    return y


def emulate(layout, a, b, bias=None, res=None, out=None):
    if layout == "forward":
        return forward(a, b, bias, res, out)
    if layout == "dgrad":
        return dgrad(a, b, out)
    return wgrad(a, b)
