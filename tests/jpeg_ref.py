"""A float64 restatement of DESIGN.md section 15.1 (the baseline JPEG encoder of said_amd/csrc/jpeg.hip) in numpy: the header, the quantised
coefficients of an image with the set of positions whose rounding fp32 cannot be expected to reproduce, and an entropy coder that turns ANY
coefficient array into the exact bytes of the scan.  Shared by tests/test_jpeg_ref_cpu.py and the GPU tests; nothing here imports said_amd."""
import io

import numpy as np

# Annex K.1, in zigzag order (the order of a DQT payload)
QBASE = np.array([
    [16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99],
    [17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66] + [99] * 50], dtype=np.int64)
# Annex K.3: (codes per length 1 .. 16, symbols in code order)
_AC_TAIL = [h << 4 | l for h in range(0x0, 0x10) for l in range(1, 0xB)]   # not the order of the tables: only used to check their symbol sets
HUFF = {
    ("dc", 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    ("dc", 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    ("ac", 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
        0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
        0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
        0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
        0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
        0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
    ("ac", 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
        0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
        0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
        0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
        0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
        0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
}
assert all(sum(b) == len(v) for b, v in HUFF.values()) and all(set(HUFF["ac", t][1]) == set(_AC_TAIL) | {0x00, 0xF0} for t in (0, 1))
AMBIGUOUS_EPS = 4e-3   # | |F| - (k + 0.5) Q | below this: fp32 may round the other way (its error on |F| <= 1024 is a few 1e-4)


def zigzag():
    """natural index (vertical frequency * 8 + horizontal frequency) of every zigzag position."""
    out = []
    for s in range(15):
        rows = range(max(0, s - 7), min(s, 7) + 1)
        out += [r * 8 + (s - r) for r in (reversed(rows) if s % 2 == 0 else rows)]
    return np.array(out)


ZZ = zigzag()


def quant_tables(quality):
    """(2, 64) in zigzag order: clamp((base s + 50) div 100, 1, 255), s = 5000 div q below 50, else 200 - 2 q."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((QBASE * s + 50) // 100, 1, 255)


def huff_codes(kind, table):
    """{symbol: (code, length)}: canonical codes."""
    bits, vals = HUFF[kind, table]
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def header(width, height, quality):
    """SOI, APP0, DQT 0, DQT 1, SOF0, DHT DC0, AC0, DC1, AC1, SOS."""
    q = quant_tables(quality)
    out = b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    for t in (0, 1):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(q[t].tolist())
    out += b"\xff\xc0\x00\x11\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    for tc_th, key in ((0x00, ("dc", 0)), (0x10, ("ac", 0)), (0x01, ("dc", 1)), (0x11, ("ac", 1))):
        bits, vals = HUFF[key]
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([tc_th]) + bytes(bits) + bytes(vals)
    return out + b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"


def dct_matrix():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    return np.where(u == 0, np.sqrt(1 / 8), np.sqrt(2 / 8)) * np.cos((2 * x + 1) * u * np.pi / 16)


def coefficients(rgb, quality):
    """rgb (H, W, 3) uint8 R G B -> (coef (blocks, 64) int16 in zigzag order, blocks in scan order; ambiguous (blocks, 64) bool)."""
    h, w = rgb.shape[:2]
    ph, pw = -h % 16, -w % 16
    a = np.pad(rgb.astype(np.float64), ((0, ph), (0, pw), (0, 0)), mode="edge")
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b - 128.0
    cb = -0.168735892 * r - 0.331264108 * g + 0.5 * b
    cr = 0.5 * r - 0.418687589 * g - 0.081312411 * b
    my, mx = a.shape[0] // 16, a.shape[1] // 16
    yb = y.reshape(my, 2, 8, mx, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my, mx, 4, 8, 8)   # Y00 Y01 Y10 Y11

    def chroma(c):
        return c.reshape(my, 8, 2, mx, 8, 2).mean(axis=(2, 5)).transpose(0, 2, 1, 3)[:, :, None]   # (my, mx, 1, 8, 8)

    blocks = np.concatenate([yb, chroma(cb), chroma(cr)], axis=2).reshape(-1, 8, 8)
    c = dct_matrix()
    f = np.einsum("vy,nyx,ux->nvu", c, blocks, c).reshape(-1, 64)[:, ZZ]                       # natural (v, u) -> zigzag
    q = quant_tables(quality).astype(np.float64)
    qb = np.where((np.arange(len(f)) % 6 >= 4)[:, None], q[1][None], q[0][None])
    t = np.abs(f) / qb
    k = np.floor(t + 0.5)
    frac = t - np.floor(t)
    ambiguous = np.abs(frac - 0.5) * qb <= AMBIGUOUS_EPS
    return (np.sign(f) * k).astype(np.int16), ambiguous


def dc_predecessor(nblocks):
    """index of the previous block of the same component for every block in scan order (-1: none, predictor 0)."""
    b = np.arange(nblocks)
    k = b % 6
    prev = np.where((k >= 1) & (k <= 3), b - 1, np.where(k == 0, b - 3, b - 6))
    return np.where((b < 6) & ~((k >= 1) & (k <= 3)), -1, prev)


def _category(v):
    a = np.abs(v.astype(np.int64))
    return np.where(a > 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1, 0)


def entropy_code(coef):
    """coef (blocks, 64) integers in zigzag order, blocks in scan order -> the scan's bytes (padded with 1 bits, 0xFF stuffed), without EOI."""
    coef = np.asarray(coef).astype(np.int64)
    nb = len(coef)
    chroma = (np.arange(nb) % 6) >= 4
    prev = dc_predecessor(nb)
    diff = coef[:, 0] - np.where(prev >= 0, coef[np.maximum(prev, 0), 0], 0)
    lut = {}
    for kind in ("dc", "ac"):
        for t in (0, 1):
            code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
            for sym, (c, n) in huff_codes(kind, t).items():
                code[sym], length[sym] = c, n
            lut[kind, t] = (code, length)

    def look(kind, is_chroma, sym):
        c0, l0 = lut[kind, 0]
        c1, l1 = lut[kind, 1]
        ln = np.where(is_chroma, l1[sym], l0[sym])
        assert (ln > 0).all(), "a symbol without a Huffman code"
        return np.where(is_chroma, c1[sym], c0[sym]), ln

    def value_bits(v, s):
        return np.where(v < 0, v + (1 << s) - 1, v)

    SLOTS = 2 + 63 * 5 + 1
    keys, codes, lens = [], [], []

    def emit(block, slot, code, length):
        keys.append(block * SLOTS + slot)
        codes.append(code)
        lens.append(length)

    blocks = np.arange(nb)
    s = _category(diff)
    c, n = look("dc", chroma, s)
    emit(blocks, 0, c, n)
    emit(blocks, 1, value_bits(diff, s), s)
    bi, pi = np.nonzero(coef[:, 1:])                      # sorted by block, then position
    v = coef[bi, pi + 1]
    first = np.r_[True, bi[1:] != bi[:-1]] if len(bi) else np.zeros(0, bool)
    run = pi - np.where(first, -1, np.r_[0, pi[:-1]]) - 1
    for z in range(3):                                     # up to three ZRL before a coefficient
        m = (run >> 4) > z
        c, n = look("ac", chroma[bi[m]], np.full(m.sum(), 0xF0))
        emit(bi[m], 2 + pi[m] * 5 + z, c, n)
    s = _category(v)
    assert (s <= 10).all(), "an AC coefficient beyond category 10"
    c, n = look("ac", chroma[bi], ((run & 15) << 4) | s)
    emit(bi, 2 + pi * 5 + 3, c, n)
    emit(bi, 2 + pi * 5 + 4, value_bits(v, s), s)
    eob = coef[:, 63] == 0
    c, n = look("ac", chroma[eob], np.zeros(eob.sum(), np.int64))
    emit(blocks[eob], SLOTS - 1, c, n)
    keys, codes, lens = np.concatenate(keys), np.concatenate(codes), np.concatenate(lens)
    order = np.argsort(keys, kind="stable")
    codes, lens = codes[order], lens[order]
    total = int(lens.sum())
    tok = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens)      # bit index inside its token, most significant first
    bits = ((codes[tok] >> (lens[tok] - 1 - pos)) & 1).astype(np.uint8)
    bits = np.r_[bits, np.ones(-total % 8, np.uint8)]
    return np.packbits(bits).tobytes().replace(b"\xff", b"\xff\x00")


def encode(rgb, quality, coef=None):
    """The whole file of an (H, W, 3) R G B image; with `coef`, of those coefficients instead of the image's own."""
    h, w = rgb.shape[:2]
    if coef is None:
        coef = coefficients(rgb, quality)[0]
    return header(w, h, quality) + entropy_code(coef) + b"\xff\xd9"


def psnr(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return 10.0 * np.log10(255.0 ** 2 / max(float((d * d).mean()), 1e-12))


def pil_encode(rgb, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, format="JPEG", quality=quality, subsampling="4:2:0")
    return buf.getvalue()


def decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def segments(data):
    """[(marker, payload)] of a file's segments up to and including SOS."""
    out, p = [], 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        out.append((m, data[p + 4:p + 2 + n]))
        p += 2 + n
        if m == 0xDA:
            return out


# ---- the cases of the tests: name -> (R G B image, quality)
def shaded_ellipse(size=800):
    """A smooth lit head-like ellipse on black, the kind of frame the renderer draws."""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    u, v = (xx - size * 0.5) / (size * 0.3), (yy - size * 0.48) / (size * 0.4)
    r2 = u * u + v * v
    z = np.sqrt(np.clip(1.0 - r2, 0.0, None))
    shade = np.clip(0.15 + 0.75 * (0.3 * u - 0.4 * v + 0.85 * z), 0.0, 1.0) * (r2 < 1.0)
    rgb = np.stack([shade * 205.0, shade * 190.0 + 8.0 * np.sin(xx / 37.0) * (r2 < 1.0), shade * 180.0], axis=-1)
    return np.floor(np.clip(rgb, 0.0, 255.0) + 0.5).astype(np.uint8)


def cases():
    rng = np.random.default_rng(20261019)
    out = {}
    for name, level in (("black", 0), ("white", 255), ("grey", 128)):
        out[name] = (np.full((16, 16, 3), level, np.uint8), 90)
    n1 = rng.integers(0, 256, (53, 37, 3), dtype=np.uint8)      # 37 wide, 53 high
    n2 = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)      # 40 wide, 24 high
    out["noise_37x53_q90"], out["noise_40x24_q90"] = (n1, 90), (n2, 90)
    out["noise_37x53_q50"], out["noise_40x24_q50"] = (n1, 50), (n2, 50)
    n3 = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    c4 = dct_matrix()[4]
    n3[:8, :8] = np.where(np.outer(c4, c4) > 0, 255, 0)[..., None]   # the sign pattern of frequency (4, 4): |F| = 1020, AC category 10
    out["noise_64_q100"] = (n3, 100)
    yy, xx = np.mgrid[0:64, 0:64]
    out["checker_q100"] = (np.repeat((((yy // 8 + xx // 8) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2), 100)
    # 48 wide, 64 high, flat but for one luminance block that holds two single high frequencies: zigzag position 63 (so no EOB) after a run of
    # zeros that takes three ZRL, and a second block whose last coefficient lies mid-way
    flat = np.full((64, 48), 90.0)
    c = dct_matrix()
    flat[24:32, 16:24] += 160.0 * np.outer(c[7], c[7]) + 120.0 * np.outer(c[2], c[0])
    flat[40:48, 8:16] += 160.0 * np.outer(c[4], c[5])
    out["flat_textured_block"] = (np.repeat(np.floor(flat + 0.5).astype(np.uint8)[..., None], 3, axis=2), 90)
    out["ellipse_800"] = (shaded_ellipse(), 90)
    return out
