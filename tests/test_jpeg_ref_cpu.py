"""CPU checks of the JPEG restatement (tests/jpeg_ref.py): its tables are the ones PIL writes, PIL reads its files, its
quality matches PIL's own encoder, and fp32 can reproduce its rounding almost everywhere."""
import os
import struct

import numpy as np
import pytest

import jpeg_ref as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = jr.cases()


@pytest.mark.parametrize("quality", [50, 75, 90, 95, 100])
def test_tables_are_the_ones_pil_writes(quality):
    rgb = CASES["noise_40x24_q90"][0]
    ours, pil = jr.segments(jr.header(40, 24, quality)), jr.segments(jr.pil_encode(rgb, quality))
    for marker in (0xDB, 0xC4):
        a, b = [p for m, p in ours if m == marker], [p for m, p in pil if m == marker]
        assert a == b and len(a) == (2 if marker == 0xDB else 4), f"marker {marker:#x} at quality {quality}"
    assert [m for m, _ in ours] == [m for m, _ in pil] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    assert ours == pil   # every segment, SOF0 and SOS included: the layout PIL writes


def test_quality_rule_below_50_and_clamps():
    assert jr.quant_tables(50).tolist() == jr.QBASE.tolist()
    assert jr.quant_tables(100).max() == 1 and jr.quant_tables(1).max() == 255 and jr.quant_tables(25)[0, 0] == 32


@pytest.mark.parametrize("name", sorted(CASES))
def test_pil_opens_every_reference_file(name):
    rgb, quality = CASES[name]
    im = jr.decode(jr.encode(rgb, quality))
    assert im.size == (rgb.shape[1], rgb.shape[0]) and im.mode == "RGB"
    # the picture, not merely a parsable file: both encoders quantise the same transform by the same tables, so the decoded error is PIL's own
    # up to libjpeg's fixed-point arithmetic; half a decibel is far above that and far below any coding mistake
    ours, pil = jr.psnr(np.asarray(im), rgb), jr.psnr(np.asarray(jr.decode(jr.pil_encode(rgb, quality))), rgb)
    print(f"{name}: restatement {ours:.3f} dB, PIL {pil:.3f} dB")
    assert ours >= pil - 0.5


def test_psnr_of_the_smooth_case_against_pil():
    rgb, quality = CASES["ellipse_800"]
    ours, pil = jr.encode(rgb, quality), jr.pil_encode(rgb, quality)
    p_ours, p_pil = jr.psnr(np.asarray(jr.decode(ours)), rgb), jr.psnr(np.asarray(jr.decode(pil)), rgb)
    print(f"ellipse 800 x 800 at quality {quality}: restatement {p_ours:.3f} dB in {len(ours)} bytes, PIL {p_pil:.3f} dB in {len(pil)} bytes")
    assert p_ours >= p_pil - 0.1


@pytest.mark.parametrize("name", sorted(CASES))
def test_ambiguous_share_stays_under_its_cap(name):
    rgb, quality = CASES[name]
    _, amb = jr.coefficients(rgb, quality)
    share = float(amb.mean())
    print(f"{name}: {100 * share:.3f} % of {amb.size} coefficients ambiguous")
    assert share < (0.01 if quality == 100 else 0.002)


def test_the_cases_exercise_what_they_are_for():
    def symbols(name):
        coef = jr.coefficients(*CASES[name])[0].astype(np.int64)
        prev = jr.dc_predecessor(len(coef))
        return coef, coef[:, 0] - np.where(prev >= 0, coef[np.maximum(prev, 0), 0], 0)

    for name in ("black", "white", "grey"):
        coef, _ = symbols(name)
        assert not coef[:, 1:].any()                                    # EOB-only blocks
    for name in ("noise_37x53_q90", "noise_40x24_q90"):
        assert b"\xff\x00" in jr.entropy_code(jr.coefficients(*CASES[name])[0])
    _, diff = symbols("checker_q100")
    assert np.abs(diff).max() >= 1024                                   # DC difference category 11
    coef, _ = symbols("noise_64_q100")
    assert np.abs(coef[:, 1:]).max() >= 512 and (np.abs(coef[:, 1:]) >= 128).sum() > 10   # AC category 10, and many in category 8
    coef, _ = symbols("flat_textured_block")
    busy = coef[(coef[:, 1:] != 0).any(axis=1)]
    assert any(b[63] != 0 and not b[16:63].any() for b in busy)         # a run over 15 across ZRL, ending without EOB
    assert any(b[63] == 0 and np.flatnonzero(b)[-1] >= 17 and np.diff(np.flatnonzero(b)).max() > 16 for b in busy)


def test_entropy_coder_is_exact_on_arbitrary_coefficients():
    """Hand-made sparse luminance coefficients (zero runs across ZRL, a non-zero position 63, DC steps in both directions; chroma zero, Q = 1)
    go through the coder and PIL's decoder: the grey levels that come back are the inverse transform of exactly those coefficients, to within
    the decoder's integer arithmetic (one level)."""
    rng = np.random.default_rng(7)
    mcus = 4                                                     # a 32 x 32 image
    coef = np.zeros((mcus * 6, 64), np.int64)
    for b in range(mcus * 6):
        if b % 6 < 4:
            coef[b, 0] = rng.integers(-300, 301)
            pos = rng.choice(np.arange(1, 64), size=rng.integers(0, 5), replace=False)
            coef[b, pos] = rng.integers(-40, 41, size=len(pos))
    coef[1, 1:] = 0
    coef[1, 63] = -33                                            # three ZRL, no EOB
    coef[2, 1:] = 0
    coef[2, [1, 40]] = [25, 17]                                  # two ZRL inside a block that ends with EOB
    data = jr.header(32, 32, 100) + jr.entropy_code(coef) + b"\xff\xd9"
    got = np.asarray(jr.decode(data)).astype(np.float64)
    c = jr.dct_matrix()
    nat = np.zeros((mcus * 6, 64))
    nat[:, jr.ZZ] = coef
    pix = np.einsum("vy,nvu,ux->nyx", c, nat.reshape(-1, 8, 8), c) + 128.0
    for m in range(mcus):
        for k in range(4):
            y0, x0 = (m // 2) * 16 + (k // 2) * 8, (m % 2) * 16 + (k % 2) * 8
            want = np.clip(pix[m * 6 + k], 0.0, 255.0)
            assert np.abs(got[y0:y0 + 8, x0:x0 + 8, 1] - want).max() <= 1.0, (m, k)


def test_write_video_takes_encoded_chunks(tmp_path):
    """script/_common.py's write_video with encoded=True: lists of files, or (files, frames) pairs whose pixels reach on_frame."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "script"))
    try:
        from _common import write_video
    finally:
        sys.path.pop(0)
    rgb, quality = CASES["noise_40x24_q90"]
    data, bgr = jr.encode(rgb, quality), np.ascontiguousarray(rgb[..., ::-1])
    seen = []
    write_video(iter([([data], bgr[None])]), str(tmp_path / "a.avi"), 30, None, width=40, height=24,
                on_frame=lambda i, f: seen.append((i, f.copy())), encoded=True)
    assert len(seen) == 1 and seen[0][0] == 0 and np.array_equal(seen[0][1], bgr)
    path = write_video(iter([[data, data], [data]]), str(tmp_path / "b.avi"), 30, None, width=40, height=24, encoded=True)
    assert open(path, "rb").read().count(b"00dc" + struct.pack("<I", len(data)) + data) == 3
    with pytest.raises(ValueError, match="raw=True"):
        write_video(iter([[data]]), str(tmp_path / "c.avi"), 30, None, width=40, height=24, on_frame=lambda i, f: None, encoded=True)


def test_avi_writer_takes_encoded_frames(tmp_path):
    """write_encoded stores the bytes it is given as one 00dc chunk and refuses what is not a JPEG of the writer's size."""
    from said_amd.util.video import AviWriter
    rgb, quality = CASES["noise_40x24_q90"]
    data = jr.encode(rgb, quality)
    path = str(tmp_path / "a.avi")
    with AviWriter(path, 30, 40, 24) as out:
        out.write_encoded(data)
        out.write(np.ascontiguousarray(rgb[..., ::-1]))
        with pytest.raises(ValueError):
            out.write_encoded(b"\x00" + data[1:])
        with pytest.raises(ValueError):
            out.write_encoded(jr.encode(CASES["black"][0], 90))
    raw = open(path, "rb").read()
    assert raw.count(b"00dc" + struct.pack("<I", len(data)) + data) == 1
    idx = raw[raw.rindex(b"idx1") + 8:]
    assert len(idx) == 32 and struct.unpack("<4sIII", idx[:16])[3] == len(data)
