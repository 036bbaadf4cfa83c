"""The weight layouts of said_amd/csrc/weight_pack.h as numpy index arithmetic, written from the layout descriptions (which lane of which fragment holds
which element), not from the C++ loops.  tests/test_weight_pack_cpu.py compares them byte for byte with what the header produces.

Every fragment layout stores 32-row tiles; lane l of a 64-lane fragment holds row 32 tile + (l & 31), and its K position depends on l >> 5 (`hi` below).
Rows past the matrix are zero.  `row0` shifts the rows (the grouped positional convolution packs rows row0 .. row0 + N - 1)."""
import numpy as np
import torch

MC, FFI = 192, 768


# ---------------------------------------------------------------- conversions
def f16_bits(x):
    return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def split_planes(x):
    """(h, l) bit patterns of w = h + 2^-11 l: h = RN16(w), l = RN16((w - h) * 2^11), the remainder taken from the stored h."""
    x = np.asarray(x, np.float32)
    h = x.astype(np.float16)
    lo = ((x - h.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    return h.view(np.uint16), lo.view(np.uint16)


def bf16_bits(x):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


def fp16_halfway(rng, n):
    """n fp32 values lying exactly half-way between two neighbouring normal fp16 numbers (both signs, exponents 2^-8 .. 2^2)."""
    bits = (rng.integers(0, 2, n) << 15 | rng.integers(7, 17, n) << 10 | rng.integers(0, 1023, n)).astype(np.uint16)
    a, b = bits.view(np.float16).astype(np.float32), (bits + np.uint16(1)).view(np.float16).astype(np.float32)
    return (a + b) * np.float32(0.5)


def is_fp16_halfway(x):
    """Elementwise: the fp32 value has exactly the bit below fp16's last significand bit set (normal fp16 range)."""
    u = np.asarray(x, np.float32).view(np.uint32)
    return ((u & 0x1FFF) == 0x1000) & (np.abs(x) >= 2.0 ** -14) & (np.abs(x) < 65504)


# ---------------------------------------------------------------- fragment layouts
def _element(W, N, row0, tile, lane, c, tap, valid=True):
    """W[row0 + n][c][tap] for n = 32 tile + (lane & 31), zero where n >= N or not `valid`; all index arguments broadcast."""
    n = 32 * tile + (lane & 31)
    ok = (n < N) & valid
    shape = np.broadcast(n, c, tap, ok).shape
    n, c, tap, ok = (np.broadcast_to(a, shape) for a in (n, c, tap, ok))
    return np.where(ok, W[np.where(ok, row0 + n, 0), np.where(ok, c, 0), np.where(ok, tap, 0)], np.float32(0))


def rows(W, N, c_begin, C, row0=0):
    """Wp[tile][tap][cpair][lane] = W[32 tile + (lane & 31)][c_begin + 2 cpair + (lane >> 5)][tap]"""
    tile, tap, cp, lane = np.ogrid[:(N + 31) // 32, :W.shape[2], :C // 2, :64]
    return _element(W, N, row0, tile, lane, c_begin + 2 * cp + (lane >> 5), tap)


def rows4(W, N, c_begin, C, row0=0):
    """Wq[tile][tap][c / 8][lane][j] = W[32 tile + (lane & 31)][c_begin + 8 cq + 2 j + (lane >> 5)][tap]"""
    tile, tap, cq, lane, j = np.ogrid[:(N + 31) // 32, :W.shape[2], :C // 8, :64, :4]
    return _element(W, N, row0, tile, lane, c_begin + 8 * cq + 2 * j + (lane >> 5), tap)


def rows_bf16(W, N, c_begin, C, row0=0):
    """Wb[tile][tap][c / 8][lane][j] = bf16(W[32 tile + (lane & 31)][c_begin + 8 cq + 4 (lane >> 5) + j][tap])"""
    tile, tap, cq, lane, j = np.ogrid[:(N + 31) // 32, :W.shape[2], :C // 8, :64, :4]
    return bf16_bits(_element(W, N, row0, tile, lane, c_begin + 8 * cq + 4 * (lane >> 5) + j, tap))


def rows_split_block(W, N, c_begin, C, row0=0):
    """[tile][24-channel block][k16 step][plane h, l][lane][8 halfs]: the block's K slice is tap-major, 3 taps x 3 groups of 8 channels (or 1 x 3); a step holds
    the two groups g = 2 step + (lane >> 5), group g = tap g / 3, channels 8 (g % 3) .. + 7; 5 steps for 3 taps, 2 for 1 tap; groups past the slice are zero."""
    taps = W.shape[2]
    tile, blk, step, lane, j = np.ogrid[:(N + 31) // 32, :C // 24, :{3: 5, 1: 2}[taps], :64, :8]
    g = 2 * step + (lane >> 5)
    h, lo = split_planes(_element(W, N, row0, tile, lane, c_begin + 24 * blk + 8 * (g % 3) + j, g // 3, valid=g < 3 * taps))
    return np.stack([h, lo], axis=3)


def rows_split_flat(W, N, c_begin, C, row0=0):
    """[tile][k16 step][plane][lane][8 halfs], one tap: the step's two groups of 8 channels are 16 step + 8 (lane >> 5) .. + 7; no padding."""
    tile, step, lane, j = np.ogrid[:(N + 31) // 32, :C // 16, :64, :8]
    h, lo = split_planes(_element(W, N, row0, tile, lane, c_begin + 16 * step + 8 * (lane >> 5) + j, 0))
    return np.stack([h, lo], axis=2)


# ---------------------------------------------------------------- token-major operands
def tap_major(W):
    """[N][C][taps] -> [N][taps][C]"""
    return np.ascontiguousarray(W.transpose(0, 2, 1))


def split_words(x):
    h, lo = split_planes(x)
    return h.astype(np.uint32) | (lo.astype(np.uint32) << 16)


# ---------------------------------------------------------------- the fused transformer tail
OUT1, Q, OUT2, GEGLU, FFPROJ = range(5)


def chain_units(slices):
    """[(matrix, first row, k16 step)] of the stream for `slices` workgroups per token tile: slice after slice, wave after wave.
    Every slice: waves 0-5 start with to_out1, to_q, to_out2 (rows 32 w .., 12 steps each).
    GEGLU pairs (hidden tiles; a pair's step = its value unit, then its gate unit 768 rows below): one slice: wave w has tiles w, w + 8, w + 16; three slices: slice
    c has tiles 8 c .. 8 c + 7, one per wave; two slices: slice c has tiles 12 c .. 12 c + 11, waves 0-3 the local tiles w and w + 4, waves 4-7 the local tile w + 4.
    Folded proj_out over [h ; x2] (60 k16 steps): a slice has its share of the first 48 steps, then its share of steps 48 .. 59; waves 0-3 take all of the
    slice's steps for column tile w, waves 4, 5 the first half for tiles 4, 5, and waves 6, 7 the second half for tiles 4, 5."""
    local_tiles = {1: lambda w: [w, w + 8, w + 16], 3: lambda w: [w], 2: lambda w: [w, w + 4] if w < 4 else [w + 4]}[slices]
    units = []
    for c in range(slices):
        steps = list(range(48 // slices * c, 48 // slices * (c + 1))) + list(range(48 + 12 // slices * c, 48 + 12 // slices * (c + 1)))
        half = len(steps) // 2
        for w in range(8):
            if w < 6:
                units += [(m, 32 * w, s) for m in (OUT1, Q, OUT2) for s in range(12)]
            for t in local_tiles(w):
                tile = 24 // slices * c + t
                units += [(GEGLU, r, s) for s in range(12) for r in (32 * tile, FFI + 32 * tile)]
            if w < 4:
                units += [(FFPROJ, 32 * w, s) for s in steps]
            elif w < 6:
                units += [(FFPROJ, 32 * w, s) for s in steps[:half]]
            else:
                units += [(FFPROJ, 32 * (w - 2), s) for s in steps[half:]]
    return np.array(units, dtype=np.int64)


def chain_values(units, mats):
    """[unit][lane][8]: lane l of a unit holds row first + (l & 31), k = 16 step + 8 (l >> 5) .. + 7 of its matrix."""
    lane, i = np.ogrid[:64, :8]
    out = np.empty((len(units), 64, 8), np.float32)
    for m, W in enumerate(mats):
        u = units[units[:, 0] == m]
        out[units[:, 0] == m] = W[u[:, 1, None, None] + (lane & 31), 16 * u[:, 2, None, None] + 8 * (lane >> 5) + i]
    return out


def fold_gamma(W, gamma):
    """W diag(gamma), formed in double and rounded once"""
    return (W.astype(np.float64) * gamma.astype(np.float64)[None, :]).astype(np.float32)


def fold_beta(W, beta, bias=None):
    """bias + W beta, accumulated in double in the order of k"""
    a = np.zeros(W.shape[0]) if bias is None else bias.astype(np.float64)
    for k in range(W.shape[1]):
        a = a + W[:, k].astype(np.float64) * np.float64(beta[k])
    return a.astype(np.float32)


def chain_streams(t):
    """{name: array} of the four streams and the vector block for the operand dict `t` (keys as in tests/weight_pack_main.cpp)."""
    mats = [t["out1"], fold_gamma(t["q"], t["g2"]), t["out2"], fold_gamma(t["ff"], t["g3"]), t["ffproj"]]
    out = {}
    for name, slices in (("stream1", 1), ("stream3", 3), ("stream2", 2)):
        h, lo = split_planes(chain_values(chain_units(slices), mats))
        out[name] = np.stack([h, lo], axis=1)   # 2 KB per unit: the h plane, then the l plane
    out["stream_bf16"] = bf16_bits(chain_values(chain_units(1), mats))
    out["vec"] = np.concatenate([t["b1"], fold_beta(t["q"], t["be2"]), t["b3"], t["c2"], t["ffproj_b"], fold_beta(t["ff"], t["be3"], t["ffb"])])
    return out, mats
