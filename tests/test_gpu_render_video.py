"""GPU tests of the device-encoded video path: iter_encoded_frames -> AviWriter.write_encoded, and script/render.py --jpeg gpu."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import jpeg_ref as jr
import render_ref as rr
from said_amd.render import RendererObject, iter_encoded_frames, iter_rendered_frames
from said_amd.util.mesh import Mesh, save_mesh
from said_amd.util.video import AviWriter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEUTRAL, BASIS, FACES = rr.arkit_mesh(os.path.join(ROOT, "tests", "golden"))
W, _ = rr.scene_coeffs()
MESH = Mesh(NEUTRAL, FACES)
DEV = "cuda:0"
QUALITY = 90


def riff_chunks(data, start, end):
    pos = start
    while pos + 8 <= end:
        fcc, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        yield fcc, pos + 8, size
        pos += 8 + size + (size & 1)


def video_payloads(data):
    """The 00dc payloads of an AVI, after checking that idx1 and the header counts agree with the movi list."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    top = {(fcc, data[off:off + 4]) if fcc == b"LIST" else (fcc, None): (off, size) for fcc, off, size in riff_chunks(data, 12, len(data))}
    off, size = top[(b"LIST", b"movi")]
    movi = [(fcc, o, s) for fcc, o, s in riff_chunks(data, off + 4, off + size)]
    video = [(o, s) for fcc, o, s in movi if fcc == b"00dc"]
    ioff, isize = top[(b"idx1", None)]
    index = [struct.unpack("<4sIII", data[ioff + 16 * i:ioff + 16 * i + 16]) for i in range(isize // 16)]
    assert len(index) == len(movi)
    # an index entry: offset of the chunk header from the 'movi' fourcc, size of the payload
    assert [(e[2] + off + 8, e[3]) for e in index if e[0] == b"00dc"] == video
    avih = data.index(b"avih") + 8
    strh = data.index(b"strh") + 8
    assert struct.unpack("<I", data[avih + 16:avih + 20])[0] == len(video)     # dwTotalFrames
    assert data[strh:strh + 4] == b"vids" and struct.unpack("<I", data[strh + 32:strh + 36])[0] == len(video)   # dwLength
    return [data[o:o + s] for o, s in video]


@pytest.fixture(scope="module")
def renderer():
    r = RendererObject(device=DEV)
    yield r
    r.close()


def test_encoded_frames_into_the_avi_writer(renderer, tmp_path):
    """The eight frames of the plain scene: encoded on the device, written as they are, and as good as PIL's encode of the same pixels."""
    name, rot, diff = rr.CASES[0]
    assert name == "plain" and not diff
    raw = np.concatenate([f.copy() for f in iter_rendered_frames(renderer, MESH, BASIS, W, chunk=3, rot=rot)])
    assert raw.shape == (rr.N_FRAMES, 800, 800, 3)
    path = str(tmp_path / "plain.avi")
    files = []
    with AviWriter(path, 60, 800, 800, quality=QUALITY) as out:
        for chunk in iter_encoded_frames(renderer, MESH, BASIS, W, chunk=3, rot=rot, quality=QUALITY):
            for jpeg in chunk:
                out.write_encoded(jpeg)
            files += chunk
    payloads = video_payloads(open(path, "rb").read())
    assert len(payloads) == rr.N_FRAMES == 8 and payloads == files
    for i, data in enumerate(payloads):
        im = jr.decode(data)
        assert im.size == (800, 800) and im.mode == "RGB"
        rgb = np.ascontiguousarray(raw[i][..., ::-1])
        ours, pil = jr.psnr(np.asarray(im), rgb), jr.psnr(np.asarray(jr.decode(jr.pil_encode(rgb, QUALITY))), rgb)
        print(f"frame {i}: device {ours:.3f} dB in {len(data)} bytes, PIL {pil:.3f} dB")
        assert ours >= pil - 0.1
    # with raw=True the pixels come along, the very ones iter_rendered_frames gives
    got = [(f, p.copy()) for f, p in iter_encoded_frames(renderer, MESH, BASIS, W[:4], chunk=4, rot=rot, quality=QUALITY, raw=True)]
    assert len(got) == 1 and got[0][0] == files[:4] and np.array_equal(got[0][1], raw[:4])


def test_render_cli_with_the_device_encoder(tmp_path):
    """script/render.py --jpeg gpu in a fresh child process: the AVI parses, its frames decode to 800 x 800, and the PNGs are written too."""
    from PIL import Image
    from scipy.io import wavfile
    names = [str(s) for s in np.load(os.path.join(ROOT, "tests", "golden", "g13_blendshape_qp.npz"))["names32"]]
    bdir = tmp_path / "blendshapes"
    bdir.mkdir()
    save_mesh(MESH, str(tmp_path / "neutral.obj"))
    for i, s in enumerate(names):
        save_mesh(Mesh(BASIS[:, i].reshape(-1, 3), FACES), str(bdir / f"{s}.obj"))
    (tmp_path / "names.txt").write_text("\n".join(names) + "\n")
    w = W[:3]
    with open(tmp_path / "coeffs.csv", "w") as f:
        f.write(",".join(names) + "\n")
        f.writelines(",".join(repr(float(x)) for x in row) + "\n" for row in w)
    rate = 16000
    wavfile.write(str(tmp_path / "a.wav"), rate, (np.sin(np.arange(rate // 8) * 0.05) * 8000).astype(np.int16))
    imgs = tmp_path / "imgs"
    cmd = [sys.executable, os.path.join(ROOT, "script", "render.py"), "--neutral_path", str(tmp_path / "neutral.obj"), "--blendshapes_dir", str(bdir),
           "--audio_path", str(tmp_path / "a.wav"), "--blendshape_coeffs_path", str(tmp_path / "coeffs.csv"), "--blendshape_list_path",
           str(tmp_path / "names.txt"), "--output_path", str(tmp_path / "out.avi"), "--save_images", "True", "--output_images_dir", str(imgs),
           "--jpeg", "gpu", "--chunk", "2"]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    payloads = video_payloads((tmp_path / "out.avi").read_bytes())
    assert len(payloads) == 3
    for i, data in enumerate(payloads):
        im = jr.decode(data)
        assert im.size == (800, 800)
        png = np.asarray(Image.open(imgs / f"{i}.png").convert("RGB"))
        assert jr.psnr(np.asarray(im), png) > 35.0, f"frame {i}: the video's frame is not the PNG's picture"
