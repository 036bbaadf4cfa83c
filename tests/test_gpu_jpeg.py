"""GPU tests of the HIP baseline JPEG encoder (said_amd/csrc/jpeg.hip, include/said_jpeg.h) against the float64 restatement of DESIGN.md
section 15.1 in tests/jpeg_ref.py.  Per case: (a) the device's coefficients are the restatement's except where the restatement itself marks
the rounding as ambiguous, and there they differ by one step at most; (b) the device's bytes are, byte for byte and header included, what the
restatement's entropy coder makes of the device's own coefficients; (c) PIL decodes the file to the true size."""
import functools

import numpy as np
import pytest
import torch

import jpeg_ref as jr
from said_amd import _engine
from said_amd.render import JpegEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = jr.cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    rgb, quality = CASES[name]
    return jr.coefficients(rgb, quality)


@pytest.fixture(scope="module")
def encoders():
    made = {}

    def get(width, height, quality):
        key = (width, height, quality)
        if key not in made:
            made[key] = JpegEncoder(DEV, width, height, quality)
        return made[key]

    yield get
    for e in made.values():
        e.close()


def check_frame(rgb, quality, data, coef, ref_coef, ambiguous):
    diff = coef.astype(np.int64) - ref_coef.astype(np.int64)
    assert not diff[~ambiguous].any(), f"{np.count_nonzero(diff[~ambiguous])} unambiguous coefficients differ"          # (a)
    assert np.abs(diff[ambiguous]).max(initial=0) <= 1
    want = jr.encode(rgb, quality, coef=coef)                                                                             # (b)
    assert len(data) == len(want) and data == want
    im = jr.decode(data)                                                                                                  # (c)
    assert im.size == (rgb.shape[1], rgb.shape[0]) and im.mode == "RGB"
    return im


@pytest.mark.parametrize("name", sorted(CASES))
def test_coefficients_bytes_and_decoding(encoders, name):
    rgb, quality = CASES[name]
    enc = encoders(rgb.shape[1], rgb.shape[0], quality)
    files = enc.encode(np.ascontiguousarray(rgb[None, ..., ::-1]), bgr=True)
    assert len(files) == 1
    ref_coef, amb = reference(name)
    im = check_frame(rgb, quality, files[0], enc.engine.read_coefficients(1)[0], ref_coef, amb)
    if name.startswith("noise") and quality == 90:
        assert b"\xff\x00" in jr.entropy_code(ref_coef) and b"\xff\x00" in files[0][len(enc.header):]   # byte stuffing happened
    if name == "ellipse_800":                                      # scans longer than one workgroup; the quality of PIL's own encode
        ours, pil = jr.psnr(np.asarray(im), rgb), jr.psnr(np.asarray(jr.decode(jr.pil_encode(rgb, quality))), rgb)
        print(f"ellipse 800 x 800: device {ours:.3f} dB in {len(files[0])} bytes, PIL {pil:.3f} dB")
        assert ours >= pil - 0.1


def test_rgb_channel_order(encoders):
    rgb, quality = CASES["noise_37x53_q90"]
    enc = encoders(37, 53, quality)
    as_rgb = enc.encode(rgb[None], bgr=False)[0]
    check_frame(rgb, quality, as_rgb, enc.engine.read_coefficients(1)[0], *reference("noise_37x53_q90"))
    assert as_rgb == enc.encode(np.ascontiguousarray(rgb[None, ..., ::-1]), bgr=True)[0]
    assert as_rgb != enc.encode(rgb[None], bgr=True)[0]


def test_three_frames_in_one_call(encoders):
    """Per-frame predictor reset and offsets: each frame of a call is byte-identical to the same frame encoded alone, and to a repeated call."""
    rgb, quality = CASES["noise_37x53_q90"]
    frames = np.stack([rgb, rgb[::-1, ::-1].copy(), np.full_like(rgb, 200)])
    enc = encoders(37, 53, quality)
    together = enc.encode(frames, bgr=False)
    coef = enc.engine.read_coefficients(3)
    assert len(together) == 3 and len(set(together)) == 3
    for i in range(3):
        assert together[i] == jr.encode(frames[i], quality, coef=coef[i])
        assert together[i] == enc.encode(frames[i:i + 1], bgr=False)[0], f"frame {i} depends on its chunk"
    assert enc.encode(frames, bgr=False) == together
    assert enc.encode(frames[[2, 0, 1]], bgr=False) == [together[2], together[0], together[1]]


def test_overflow_is_reported_and_nothing_is_written_past_the_capacity(encoders):
    rgb, quality = CASES["noise_64_q100"]
    enc = encoders(64, 64, quality)
    eng = enc.engine
    frames = torch.from_numpy(np.stack([rgb, rgb[::-1].copy()])).to(DEV)
    CANARY, CAP = 0xA5, 64
    buf = torch.full((CAP + 4096,), CANARY, dtype=torch.uint8, device=DEV)
    offsets = torch.zeros(3, dtype=torch.int64, device=DEV)
    fits, required = eng.encode(frames, 2, buf, offsets, bgr=False, capacity=CAP)
    assert not fits and required > frames.numel() // 4            # also larger than JpegEncoder's first buffer: its retry is exercised below
    assert bool((buf[CAP:] == CANARY).all()), "bytes were written past the capacity"
    assert offsets.tolist()[0] == 0 and offsets.tolist()[2] == required
    out = torch.full((required + 4096,), CANARY, dtype=torch.uint8, device=DEV)
    fits2, required2 = eng.encode(frames, 2, out, offsets, bgr=False, capacity=required)
    assert fits2 and required2 == required and bool((out[required:] == CANARY).all())
    o = offsets.tolist()
    data = out[:required].cpu().numpy().tobytes()
    scans = [data[o[0]:o[1]], data[o[1]:o[2]]]
    assert all(s.endswith(b"\xff\xd9") for s in scans)
    fresh = JpegEncoder(DEV, 64, 64, quality)                      # its first buffer is a quarter of the raw size: too small for this noise
    try:
        assert fresh.encode(frames, bgr=False) == [enc.header + s for s in scans]
    finally:
        fresh.close()
    fits3, required3 = eng.encode(frames, 2, None, offsets, bgr=False)   # no buffer at all: the size query
    assert not fits3 and required3 == required


def test_errors_are_messages():
    with pytest.raises(_engine.EngineError, match="0 x 5"):
        _engine.JpegEngine(torch.device(DEV), 0, 5, 90)
    with pytest.raises(_engine.EngineError, match="quality 0"):
        _engine.JpegEngine(torch.device(DEV), 16, 16, 0)
    with pytest.raises(_engine.EngineError, match="quality 101"):
        _engine.JpegEngine(torch.device(DEV), 16, 16, 101)
    with pytest.raises(_engine.NoCpuPathError):
        _engine.JpegEngine(torch.device("cpu"), 16, 16, 90)
    eng = _engine.JpegEngine(torch.device(DEV), 16, 16, 90)
    with pytest.raises(_engine.EngineError, match="n_frames"):
        eng.read_coefficients(1)                                   # nothing encoded yet
    with pytest.raises(_engine.EngineError, match="quality 0"):
        eng.configure(16, 16, 0)                                   # a failed reconfigure leaves nothing of the old configuration behind
    assert (eng.width, eng.height, eng.quality, eng.blocks, eng.header) == (0, 0, 0, 0, b"")
    with pytest.raises(_engine.EngineError, match="not configured"):
        eng.encode(torch.zeros(768, dtype=torch.uint8, device=DEV), 1, None, torch.zeros(2, dtype=torch.int64, device=DEV))
    eng.configure(32, 16, 75)
    assert (eng.width, eng.height, eng.quality, eng.blocks) == (32, 16, 75, 12) and eng.header == jr.header(32, 16, 75)
    eng.close()
