"""The renderer on the MI355X (said_amd.render, include/said_render.h) against tests/render_ref.py, the float64 restatement of DESIGN.md
section 15.  The mesh is the ARKit reference mesh (vertices and the 32 bases of golden G13, faces of golden G15); the scenes are those of
render_ref.CASES: 8 frames of a fixed synthetic coefficient sequence in [0, 1], without rotation and with a 0.3 rad yaw, plain and in
difference mode.  tests/test_render_cpu.py asserts that the restatement's ambiguous pixels stay under 0.1 % of the covered ones there."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_ref as rr
from said_amd import _engine
from said_amd.render import RendererObject, colormap_table, iter_rendered_frames, render_blendshape_coefficients
from said_amd.util.mesh import Mesh, save_mesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEUTRAL, BASIS, FACES = rr.arkit_mesh(os.path.join(ROOT, "tests", "golden"))
W, WT = rr.scene_coeffs()
MESH = Mesh(NEUTRAL, FACES)
CENTER = NEUTRAL.mean(axis=0)
DEV = "cuda:0"
MAX_DIFF = 0.001


@pytest.fixture(scope="module")
def renderer():
    r = RendererObject(device=DEV)
    yield r
    r.close()


def gpu_frames(renderer, w, target=None, rot=None, chunk=64, t_center=None, want_ids=True):
    out, ids = [], []
    for item in iter_rendered_frames(renderer, MESH, BASIS, w, target, max_diff=MAX_DIFF, chunk=chunk, rot=rot, t_center=t_center, face_ids=want_ids):
        fr, fi = item if want_ids else (item, None)
        out.append(fr.copy())
        if want_ids:
            ids.append(fi.copy())
    return np.concatenate(out), (np.concatenate(ids) if want_ids else None)


def test_vertices_normals_and_difference_colours(renderer):
    """Vertices within 4 fp32 ulp of max |v|; normals within 1e-5; difference colours identical to the table lookup except where the float64
    magnitude is within 1e-6 (relative) of a bin edge."""
    gpu_frames(renderer, W, WT)
    v = renderer.engine.read_vertices(rr.N_FRAMES).astype(np.float64)
    n = renderer.engine.read_normals(rr.N_FRAMES).astype(np.float64)
    col = renderer.engine.read_colors(rr.N_FRAMES)
    ref_v, mag, x = rr.blend(NEUTRAL, BASIS, W, WT, MAX_DIFF)
    ulp = float(np.spacing(np.float32(np.abs(ref_v).max())))
    err_v = np.abs(v - ref_v).max()
    err_n = max(np.abs(n[t] - rr.vertex_normals(ref_v[t], FACES)).max() for t in range(rr.N_FRAMES))
    print(f"vertices: max error {err_v:.3e} = {err_v / ulp:.2f} ulp of max |v|; normals: max error {err_n:.3e}")
    assert err_v <= 4 * ulp
    assert err_n <= 1e-5
    table = colormap_table("viridis")
    edges = np.arange(1, rr.LUT_N) / rr.LUT_N * MAX_DIFF              # magnitudes at which the bin changes (the last: the clip to the last bin)
    near_edge = (np.abs(mag[..., None] - edges) <= 1e-6 * edges).any(axis=-1)
    want = table[rr.colormap_bin(x)]
    differs = (col != want).any(axis=-1)
    print(f"difference colours: {int(differs.sum())} of {differs.size} differ, {int(near_edge.sum())} within 1e-6 of a bin edge")
    assert not (differs & ~near_edge).any()
    assert len(np.unique(rr.colormap_bin(x))) > 100   # the sequence exercises the table, not one bin


@pytest.mark.parametrize("name,rot,diff", rr.CASES, ids=[c[0] for c in rr.CASES])
def test_pixels_against_the_restatement(renderer, name, rot, diff):
    """Face ids identical at every non-ambiguous pixel; there no colour channel more than one level off (one-level flips are counted and
    printed); background exactly 0."""
    img, ids = gpu_frames(renderer, W, WT if diff else None, rot=rot)
    assert img.shape == (rr.N_FRAMES, 800, 800, 3) and img.dtype == np.uint8
    ref_v, mag, x = rr.blend(NEUTRAL, BASIS, W, WT, MAX_DIFF)
    table = colormap_table("viridis").astype(np.float64)
    sc = rr.scene()
    flips = covered = ambiguous = 0
    for t in range(rr.N_FRAMES):
        colors = table[rr.colormap_bin(x[t])] if diff else None
        ref = rr.render_frame(ref_v[t], FACES, sc, colors=colors, rot=rot, t_center=CENTER)
        clear = ~ref["ambiguous"]
        wrong = (ids[t] != ref["face"]) & clear
        assert not wrong.any(), f"{name} frame {t}: {int(wrong.sum())} non-ambiguous pixels show another face, first at {np.argwhere(wrong)[0]}"
        agree = clear & (ids[t] == ref["face"])
        delta = np.abs(img[t].astype(np.int64) - rr.to_bgr8(ref["color"]).astype(np.int64))
        assert delta[agree].max() <= 1, f"{name} frame {t}: a channel is {int(delta[agree].max())} levels off"
        flips += int((delta[agree].max(axis=-1) == 1).sum())
        covered += int((ref["face"] >= 0).sum())
        ambiguous += int(ref["ambiguous"].sum())
        assert not img[t][ids[t] < 0].any(), f"{name} frame {t}: background is not 0"
        assert (ids[t] >= 0).sum() > 100000
    print(f"{name}: {covered} covered pixels, {ambiguous} ambiguous, {flips} pixels one level off")


def test_chunks_and_runs_are_bit_identical(renderer):
    w = np.concatenate([W, W[::-1], W[:4]])   # 20 frames: chunks of 3 leave a remainder
    wt = np.concatenate([WT, WT[::-1], WT[:4]])
    for target in (None, wt):
        a, ia = gpu_frames(renderer, w, target, chunk=64)
        for chunk in (1, 3):
            b, ib = gpu_frames(renderer, w, target, chunk=chunk)
            assert np.array_equal(a, b) and np.array_equal(ia, ib), f"chunk {chunk} differs from chunk 64"
        b, ib = gpu_frames(renderer, w, target, chunk=64)
        assert np.array_equal(a, b) and np.array_equal(ia, ib)
        assert np.array_equal(a[:8], a[15:7:-1])   # the mirrored half repeats the first frames


def test_rot_and_t_center_are_honoured(renderer):
    """A rotation changes the picture; about another centre it changes it differently; both match the restatement's silhouette to the ambiguous pixels."""
    sc = rr.scene()
    v0 = rr.blend(NEUTRAL, BASIS, W[:1])[0]
    base, _ = gpu_frames(renderer, W[:1])
    other_c = CENTER + np.array([0.05, 0.0, 0.0])
    seen = [base]
    for rot, c in ((rr.YAW, CENTER), (rr.YAW, other_c), ((0.2, 0.0, 0.1), CENTER)):
        img, ids = gpu_frames(renderer, W[:1], rot=rot, t_center=c)
        assert all(not np.array_equal(img, s) for s in seen)
        seen.append(img)
        ref = rr.render_frame(v0, FACES, sc, rot=rot, t_center=c)
        assert not ((ids[0] != ref["face"]) & ~ref["ambiguous"]).any()


def test_z_offset_moves_the_lights_only():
    """The reference adds its camera with a literal pose, so z_offset leaves the geometry alone and changes the shading."""
    a, b = RendererObject(device=DEV), RendererObject(z_offset=0.3, device=DEV)
    try:
        (ia, fa), (ib, fb) = gpu_frames(a, W[:1]), gpu_frames(b, W[:1])
        assert np.array_equal(fa, fb)
        assert not np.array_equal(ia, ib)
        ref = rr.render_frame(rr.blend(NEUTRAL, BASIS, W[:1])[0], FACES, rr.scene(0.3), t_center=CENTER)
        agree = ~ref["ambiguous"] & (fb[0] == ref["face"])
        assert np.abs(ib[0].astype(np.int64) - rr.to_bgr8(ref["color"]).astype(np.int64))[agree].max() <= 1
    finally:
        a.close()
        b.close()


def test_invalid_meshes_are_errors_not_faults():
    eng = _engine.RenderEngine(torch.device(DEV))
    try:
        bad = FACES.copy()
        bad[7, 1] = len(NEUTRAL)
        with pytest.raises(_engine.EngineError, match="outside"):
            eng.set_mesh(NEUTRAL, bad, BASIS)
        bad[7, 1] = -1
        with pytest.raises(_engine.EngineError, match="outside"):
            eng.set_mesh(NEUTRAL, bad, BASIS)
        with pytest.raises(_engine.EngineError, match="faces"):
            eng.set_mesh(NEUTRAL, np.zeros((0, 3), dtype=np.int32), BASIS)
        out = torch.empty((1, 800, 800, 3), dtype=torch.uint8, device=DEV)
        with pytest.raises(_engine.EngineError, match="no mesh"):   # a refused mesh leaves nothing to draw
            eng.render(torch.zeros(1, 32, device=DEV), 0, 1, out)
        eng.set_mesh(NEUTRAL, FACES, BASIS)   # and the context still works
        with pytest.raises(_engine.EngineError, match="no scene"):
            eng.render(torch.zeros(1, 32, device=DEV), 0, 1, out)
    finally:
        eng.close()
    with pytest.raises(_engine.NoCpuPathError):
        _engine.RenderEngine(torch.device("cpu"))


def riff_chunks(data, start, end):
    pos = start
    while pos + 8 <= end:
        fcc, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        yield fcc, pos + 8, size
        pos += 8 + size + (size & 1)


def test_render_cli_end_to_end(tmp_path, renderer):
    """script/render.py in a fresh child process: the AVI parses, carries sound, and the saved PNGs equal the API's frames."""
    from PIL import Image
    from scipy.io import wavfile
    names = [str(s) for s in np.load(os.path.join(ROOT, "tests", "golden", "g13_blendshape_qp.npz"))["names32"]]
    bdir = tmp_path / "blendshapes"
    bdir.mkdir()
    save_mesh(MESH, str(tmp_path / "neutral.obj"))
    for i, s in enumerate(names):
        save_mesh(Mesh(BASIS[:, i].reshape(-1, 3), FACES), str(bdir / f"{s}.obj"))
    (tmp_path / "names.txt").write_text("\n".join(names) + "\n")
    w = W[:5]
    with open(tmp_path / "coeffs.csv", "w") as f:
        f.write(",".join(names) + "\n")
        f.writelines(",".join(repr(float(x)) for x in row) + "\n" for row in w)
    rate = 16000
    wavfile.write(str(tmp_path / "a.wav"), rate, (np.sin(np.arange(rate // 4) * 0.05) * 8000).astype(np.int16))
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    cmd = [sys.executable, os.path.join(ROOT, "script", "render.py"), "--neutral_path", str(tmp_path / "neutral.obj"), "--blendshapes_dir", str(bdir),
           "--audio_path", str(tmp_path / "a.wav"), "--blendshape_coeffs_path", str(tmp_path / "coeffs.csv"), "--blendshape_list_path",
           str(tmp_path / "names.txt"), "--output_path", str(tmp_path / "out.avi"), "--save_images", "True", "--output_images_dir", str(imgs)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    data = (tmp_path / "out.avi").read_bytes()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    top = {(fcc, data[off:off + 4]) if fcc == b"LIST" else (fcc, None): (off, size) for fcc, off, size in riff_chunks(data, 12, len(data))}
    assert (b"LIST", b"hdrl") in top and (b"LIST", b"movi") in top and (b"idx1", None) in top
    off, size = top[(b"LIST", b"movi")]
    kinds = [fcc for fcc, _, _ in riff_chunks(data, off + 4, off + size)]
    assert kinds.count(b"00dc") == 5 and kinds.count(b"01wb") >= 1
    api = render_blendshape_coefficients(renderer, MESH, BASIS, w)
    for i in range(5):
        png = np.asarray(Image.open(imgs / f"{i}.png").convert("RGB"))
        assert np.array_equal(png[..., ::-1], api[i]), f"frame {i}: the PNG differs from the API's frame"
