"""Rendering with 4 samples per pixel on the MI355X (include/said_render_ms.h): coverage and depth per sample
against closed forms on hand-made meshes of 64 x 64 and 70 x 45 pixels (partial tiles, a width that is no multiple of 4), and against
tests/render_ms_ref.py, the float64 restatement, on the two full-size ARKit scenes whose ambiguity cap tests/test_render_ms_cpu.py asserts."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_ref as jr
import render_ms_ref as ms
import render_ref as rr
from said_amd import _engine
from said_amd.render import RendererObject, colormap_table, iter_rendered_frames
from said_amd.util.mesh import Mesh, save_mesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEUTRAL, BASIS, FACES = rr.arkit_mesh(os.path.join(ROOT, "tests", "golden"))
W, WT = rr.scene_coeffs()
MESH = Mesh(NEUTRAL, FACES)
CENTER = NEUTRAL.mean(axis=0)
DEV = "cuda:0"
MAX_DIFF = 0.001
SIZES = [(64, 64), (70, 45)]
BASE = (0.2, 0.5, 0.8)   # R, G, B: bytes 51, 128, 204, none of them near a rounding boundary


# ---- small scenes: one frame, k = 1, hand-made meshes
def small_scene(width, height, f, cx, cy, lights=(), ambient=1.0, metallic=0.8, roughness=0.8):
    sc = _engine.RenderScene()
    sc.width, sc.height = width, height
    sc.fx = sc.fy = f
    sc.cx, sc.cy = cx, cy
    sc.znear, sc.zfar = 0.01, 3.0
    sc.cam_pos[:] = [0.0, 0.0, 1.0]
    sc.n_lights = len(lights)
    for i, p in enumerate(lights):
        sc.light_pos[i][:] = [float(v) for v in p]
        sc.light_intensity[i] = 2.0
    sc.ambient = ambient
    sc.base_color[:] = BASE
    sc.metallic, sc.roughness, sc.vc_metallic, sc.vc_roughness = metallic, roughness, 1.0, 1.0
    return sc


def ref_scene(sc):
    """The restatement's scene of a RenderScene."""
    return dict(width=sc.width, height=sc.height, fx=float(sc.fx), fy=float(sc.fy), cx=float(sc.cx), cy=float(sc.cy), znear=float(sc.znear),
                zfar=float(sc.zfar), cam=np.array(list(sc.cam_pos), dtype=np.float64),
                lights=np.array([list(sc.light_pos[i]) for i in range(sc.n_lights)], dtype=np.float64).reshape(-1, 3), intensity=2.0,
                ambient=float(sc.ambient), base=np.array(list(sc.base_color), dtype=np.float64), metallic=float(sc.metallic),
                roughness=float(sc.roughness), vc_metallic=1.0, vc_roughness=1.0)


def render_small(sc, verts, faces, samples):
    """One frame of a rigid mesh (k = 1, the basis shape is the neutral): (frame (H, W, 3), ids (H, W) or (H, W, 4))."""
    eng = _engine.RenderEngine(torch.device(DEV))
    try:
        eng.set_scene(sc)
        v = np.asarray(verts, dtype=np.float64)
        eng.set_mesh(v, np.asarray(faces, dtype=np.int32), v.reshape(-1, 1))
        h, w = sc.height, sc.width
        out = torch.full((1, h, w, 3), 77, dtype=torch.uint8, device=DEV)
        ids = torch.full((1, h, w, 4) if samples == 4 else (1, h, w), -7, dtype=torch.int32, device=DEV)
        coeffs = torch.zeros(1, 1, device=DEV)
        if samples == 4:
            eng.render(coeffs, 0, 1, out, samples=4, sample_ids=ids)
        else:
            eng.render(coeffs, 0, 1, out, face_ids=ids)
        torch.cuda.synchronize()
        return out[0].cpu().numpy(), ids[0].cpu().numpy()
    finally:
        eng.close()


def to_u8(c):
    """The kernel's quantisation of an fp32 colour value: floor(fma(c, 255, 0.5)), the fma rounded to fp32 once."""
    return int(np.floor(np.float32(float(np.float32(c)) * 255.0 + 0.5)))


@pytest.mark.parametrize("axis,shift", [("x", 0.25), ("x", -0.25), ("y", 0.25), ("y", -0.25)], ids=["x+", "x-", "y+", "y-"])
@pytest.mark.parametrize("width,height", SIZES, ids=["64x64", "70x45"])
def test_coverage_closed_forms(width, height, axis, shift):
    """A camera-facing quad that fills the image up to one straight edge at pixel centre + shift; one screen unit is one pixel, no lights and
    ambient 1, so an interior sample's colour is the base colour's bytes.  A sample is covered exactly when it lies before the edge: at
    + 0.25 three samples of the edge's pixels, at - 0.25 one; every sample is at least 0.125 px from the edge."""
    sc = small_scene(width, height, 1.0, 0.0, float(height))   # screen x = X, screen y = height - Y at z = 0
    col, row = width - 4, height - 3                           # the edge's pixels lie in the last, partial tile of the 70 x 45 image
    edge = (col if axis == "x" else row) + 0.5 + shift
    x1, y1 = (edge, height + 8.0) if axis == "x" else (width + 8.0, edge)
    screen = [(-8.0, -8.0), (x1, -8.0), (x1, y1), (-8.0, y1)]
    verts = np.array([[x, height - y, 0.0] for x, y in screen])
    img, ids = render_small(sc, verts, [[0, 1, 2], [0, 2, 3]], 4)
    cols, rows = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5)
    want = np.stack([(cols + ox if axis == "x" else rows + oy) < edge for ox, oy in ms.OFFSETS], axis=-1)
    assert np.array_equal(ids >= 0, want) and set(np.unique(ids)) <= {-1, 0, 1}
    # by hand, at the edge's pixels: x offsets -0.125 +0.375 -0.375 +0.125, y offsets -0.375 -0.125 +0.125 +0.375
    by_hand = {("x", 0.25): [1, 0, 1, 1], ("x", -0.25): [0, 0, 1, 0], ("y", 0.25): [1, 1, 1, 0], ("y", -0.25): [1, 0, 0, 0]}[(axis, shift)]
    at_edge = ids[:, col] if axis == "x" else ids[row]
    assert ((at_edge >= 0) == np.array(by_hand, dtype=bool)).all()
    value = np.array([to_u8(c) for c in BASE[::-1]])           # B, G, R
    n = want.sum(axis=-1)
    assert np.array_equal(img, ((n[..., None] * value + 2) >> 2).astype(np.uint8))
    assert set(np.unique(n)) == {0, sum(by_hand), 4}


def crossing_mesh(row, height):
    """Two triangles through the world line Y = Y0, z = 0, tilted by +-0.25 in z per unit of Y: equal depth along the screen line y = row + 0.5
    (64 px per unit at depth 1, principal point in the image centre), which runs between samples s1 and s2 of that row's pixels.  Above it
    face 0 is nearer, below it face 1.  Every coordinate is a dyadic fraction, exact in fp32."""
    y0 = (height / 2 - (row + 0.5)) / 64.0
    z = lambda y, sign: sign * 0.25 * (y - y0)
    verts = [[-2.0, -1.5, z(-1.5, 1)], [4.0, -1.5, z(-1.5, 1)], [-2.0, 2.5, z(2.5, 1)],
             [-2.0, 1.5, z(1.5, -1)], [4.0, 1.5, z(1.5, -1)], [-2.0, -2.5, z(-2.5, -1)]]
    return np.array(verts), np.array([[0, 1, 2], [3, 5, 4]])   # both normals towards the camera


@pytest.mark.parametrize("width,height", SIZES, ids=["64x64", "70x45"])
def test_depth_is_per_sample(width, height):
    """Sample ids are the restatement's and the crossing row's pixels mix both faces' colours (a light from above shades the two tilts apart)."""
    row = height - 9
    sc = small_scene(width, height, 64.0, width / 2, height / 2, lights=[(0.0, 1.0, 0.5)], ambient=0.2, metallic=0.0, roughness=0.5)
    verts, faces = crossing_mesh(row, height)
    img, ids = render_small(sc, verts, faces, 4)
    ref = ms.render_frame_ms(verts, faces, ref_scene(sc))
    assert not ref["ambiguous"].any()
    assert np.array_equal(ids, ref["face"])
    assert (ids[:row] == 0).all() and (ids[row + 1:] == 1).all() and (ids[row] == [0, 0, 1, 1]).all()
    delta = np.abs(img.astype(np.int64) - ref["bgr"].astype(np.int64))
    assert delta.max() <= 1
    # the row mixes both faces' colours: it lies strictly between its neighbours, which differ by many levels
    up, mid, down = (img[r].astype(np.int64) for r in (row - 1, row, row + 1))
    assert np.abs(up - down).max(axis=-1).min() > 16
    lo, hi = np.minimum(up, down), np.maximum(up, down)
    strictly = (mid > lo) & (mid < hi)
    assert strictly.any(axis=-1).all() and ((mid >= lo - 1) & (mid <= hi + 1)).all()
    one, _ = render_small(sc, verts, faces, 1)
    assert np.array_equal(one[:row], img[:row]) and np.array_equal(one[row + 1:], img[row + 1:])   # one face in all four samples: its bytes


# ---- the full-size scenes
@pytest.fixture(scope="module")
def renderers():
    r1, r4 = RendererObject(device=DEV), RendererObject(device=DEV, samples=4)
    yield r1, r4
    r1.close()
    r4.close()


def gpu_frames(renderer, w, target=None, rot=None, chunk=64):
    out, ids = [], []
    for fr, fi in iter_rendered_frames(renderer, MESH, BASIS, w, target, max_diff=MAX_DIFF, chunk=chunk, rot=rot, t_center=CENTER, face_ids=True):
        out.append(fr.copy())
        ids.append(fi.copy())
    return np.concatenate(out), np.concatenate(ids)


_GEOMETRY = {}


def geometry(t, rot):
    """The restatement's per-sample faces of a (frame, rotation), shared by the plain and the difference case."""
    if (t, rot) not in _GEOMETRY:
        _GEOMETRY[(t, rot)] = ms.sample_geometry(rr.blend(NEUTRAL, BASIS, W)[t], FACES, rr.scene(), rot=rot, t_center=CENTER)
    return _GEOMETRY[(t, rot)]


CASES = [(t, rot, diff) for t, rot in ms.SCENES for diff in (False, True)]
CASE_IDS = [f"frame{t}{'_yaw' if rot else ''}{'_difference' if diff else ''}" for t, rot, diff in CASES]


@pytest.mark.parametrize("t,rot,diff", CASES, ids=CASE_IDS)
def test_pixels_against_the_restatement(renderers, t, rot, diff):
    """Sample ids equal at every non-ambiguous sample, resolved bytes within one level at every non-ambiguous pixel, ambiguous share < 0.1 %."""
    img, ids = gpu_frames(renderers[1], W[t:t + 1], WT[t:t + 1] if diff else None, rot=rot)
    assert img.shape == (1, 800, 800, 3) and ids.shape == (1, 800, 800, 4) and ids.dtype == np.int32
    ref_v, _, x = rr.blend(NEUTRAL, BASIS, W, WT, MAX_DIFF)
    colors = colormap_table("viridis").astype(np.float64)[rr.colormap_bin(x[t])] if diff else None
    ref = ms.render_frame_ms(ref_v[t], FACES, rr.scene(), colors=colors, rot=rot, t_center=CENTER, geometry=geometry(t, rot))
    wrong = (ids[0] != ref["face"]) & ~ref["sample_ambiguous"]
    assert not wrong.any(), f"{int(wrong.sum())} non-ambiguous samples show another face, first at {np.argwhere(wrong)[0]}"
    clear = ~ref["ambiguous"]
    delta = np.abs(img[0].astype(np.int64) - ref["bgr"].astype(np.int64)).max(axis=-1)
    covered = int((ref["face"] >= 0).any(axis=-1).sum())
    ambiguous = int(ref["ambiguous"].sum())
    print(f"{covered} covered pixels, {ambiguous} ambiguous, {int((delta[clear] == 1).sum())} pixels one level off, worst {int(delta[clear].max())}")
    assert delta[clear].max() <= 1
    assert covered > 100000 and ambiguous < 1e-3 * covered
    assert not img[0][(ids[0] < 0).all(axis=-1)].any()


@pytest.mark.parametrize("t,rot,diff", CASES, ids=CASE_IDS)
def test_interior_pixels_are_the_one_sample_render(renderers, t, rot, diff):
    """Every pixel whose four samples show the face the 1-sample render draws there has that render's three bytes; the others are thousands."""
    target = WT[t:t + 1] if diff else None
    one, face = gpu_frames(renderers[0], W[t:t + 1], target, rot=rot)
    img, ids = gpu_frames(renderers[1], W[t:t + 1], target, rot=rot)
    interior = (ids[0] == face[0][..., None]).all(axis=-1)
    assert np.array_equal(img[0][interior], one[0][interior])
    mixed = ids[0].min(axis=-1) != ids[0].max(axis=-1)
    silhouette = mixed & (ids[0] < 0).any(axis=-1)
    print(f"{int(interior.sum())} interior pixels, {int(mixed.sum())} with two or more sample values, {int(silhouette.sum())} on the silhouette")
    assert mixed.sum() > 10000 and silhouette.sum() > 500
    assert not np.array_equal(img[0][mixed], one[0][mixed])


def raw_render_ms(eng, samples, coeffs, out, face_ids=None, sample_ids=None, n=1):
    """said_render_render_ms itself, whatever the arguments: (return code, message)."""
    lib = _engine.load_library("render_ms")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(eng.index):
        rc = lib.said_render_render_ms(eng.h, samples, ptr(coeffs), None, 0, n, MAX_DIFF, None, None, ptr(out), ptr(face_ids), ptr(sample_ids),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, (lib.said_render_last_error(eng.h) or b"").decode()


def test_one_sample_through_the_new_entry(renderers):
    """samples = 1 of said_render_render_ms is said_render_render: frames and face ids bit for bit."""
    r1 = renderers[0]
    want, want_ids = gpu_frames(r1, W[:2])
    coeffs = torch.from_numpy(W[:2].astype(np.float32)).to(DEV)
    out = torch.zeros((2, 800, 800, 3), dtype=torch.uint8, device=DEV)
    ids = torch.full((2, 800, 800), -5, dtype=torch.int32, device=DEV)
    lib = _engine.load_library("render_ms")
    c = np.ascontiguousarray(CENTER, dtype=np.float64)
    with torch.cuda.device(r1.engine.index):
        rc = lib.said_render_render_ms(r1.engine.h, 1, ctypes.c_void_p(coeffs.data_ptr()), None, 0, 2, MAX_DIFF, None,
                                       c.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_void_p(ids.data_ptr()), None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.said_render_last_error(r1.engine.h)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(ids.cpu().numpy(), want_ids)


def test_chunks_and_runs_are_bit_identical(renderers):
    a, ia = gpu_frames(renderers[1], W, chunk=64)
    assert a.shape == (8, 800, 800, 3) and ia.shape == (8, 800, 800, 4)
    for chunk in (3, 64, 3, 64):
        b, ib = gpu_frames(renderers[1], W, chunk=chunk)
        assert np.array_equal(a, b) and np.array_equal(ia, ib), f"chunk {chunk} differs from the first run"
    v = renderers[1].engine.read_vertices(8)   # the stage readers work after the multisampled render
    assert np.abs(v - rr.blend(NEUTRAL, BASIS, W)).max() < 1e-6


def test_wrong_arguments_are_errors_not_faults():
    eng = _engine.RenderEngine(torch.device(DEV))
    try:
        sc = small_scene(64, 64, 1.0, 0.0, 64.0)
        out = torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=DEV)
        face_ids = torch.zeros((1, 64, 64), dtype=torch.int32, device=DEV)
        sample_ids = torch.zeros((1, 64, 64, 4), dtype=torch.int32, device=DEV)
        coeffs = torch.zeros(1, 1, device=DEV)
        rc, msg = raw_render_ms(eng, 4, coeffs, out)
        assert rc != 0 and "no mesh" in msg
        with pytest.raises(_engine.EngineError, match="no mesh"):
            eng.render(coeffs, 0, 1, out, samples=4)
        verts = np.array([[0.0, 0.0, 0.0], [40.0, 0.0, 0.0], [0.0, 40.0, 0.0]])
        eng.set_mesh(verts, np.array([[0, 1, 2]], dtype=np.int32), verts.reshape(-1, 1))
        rc, msg = raw_render_ms(eng, 4, coeffs, out)
        assert rc != 0 and "no scene" in msg
        eng.set_scene(sc)
        for samples in (0, 2, 3, 8):
            rc, msg = raw_render_ms(eng, samples, coeffs, out)
            assert rc != 0 and "samples" in msg, samples
            with pytest.raises(_engine.EngineError, match="samples"):
                eng.render(coeffs, 0, 1, out, samples=samples)
        rc, msg = raw_render_ms(eng, 4, coeffs, out, face_ids=face_ids)
        assert rc != 0 and "face_ids_dev must be NULL" in msg
        with pytest.raises(_engine.EngineError, match="face_ids_dev must be NULL"):
            eng.render(coeffs, 0, 1, out, samples=4, face_ids=face_ids)
        rc, msg = raw_render_ms(eng, 1, coeffs, out, sample_ids=sample_ids)
        assert rc != 0 and "sample_ids_dev must be NULL" in msg
        with pytest.raises(_engine.EngineError, match="sample_ids_dev must be NULL"):
            eng.render(coeffs, 0, 1, out, sample_ids=sample_ids)
        rc, msg = raw_render_ms(eng, 4, coeffs, None)
        assert rc != 0 and "null" in msg
        assert not out.any() and not sample_ids.any()   # nothing was launched
        rc, msg = raw_render_ms(eng, 4, coeffs, out, sample_ids=sample_ids)   # and the context still works
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert out.any() and (sample_ids.cpu().numpy() >= -1).all()
    finally:
        eng.close()
    with pytest.raises(ValueError, match="samples"):
        RendererObject(device=DEV, samples=2)


def test_render_cli_with_four_samples(tmp_path, renderers):
    """script/render.py --samples 4 --jpeg gpu in a fresh child process: four frames of 800 x 800 in the AVI, the first within the JPEG
    tests' 35 dB of the raw 4-sample frame (and nearer to it than to the 1-sample frame)."""
    from scipy.io import wavfile
    from test_gpu_render_video import video_payloads
    names = [str(s) for s in np.load(os.path.join(ROOT, "tests", "golden", "g13_blendshape_qp.npz"))["names32"]]
    bdir = tmp_path / "blendshapes"
    bdir.mkdir()
    save_mesh(MESH, str(tmp_path / "neutral.obj"))
    for i, s in enumerate(names):
        save_mesh(Mesh(BASIS[:, i].reshape(-1, 3), FACES), str(bdir / f"{s}.obj"))
    (tmp_path / "names.txt").write_text("\n".join(names) + "\n")
    w = W[:4]
    with open(tmp_path / "coeffs.csv", "w") as f:
        f.write(",".join(names) + "\n")
        f.writelines(",".join(repr(float(x)) for x in row) + "\n" for row in w)
    wavfile.write(str(tmp_path / "a.wav"), 16000, (np.sin(np.arange(2000) * 0.05) * 8000).astype(np.int16))
    cmd = [sys.executable, os.path.join(ROOT, "script", "render.py"), "--neutral_path", str(tmp_path / "neutral.obj"), "--blendshapes_dir", str(bdir),
           "--audio_path", str(tmp_path / "a.wav"), "--blendshape_coeffs_path", str(tmp_path / "coeffs.csv"), "--blendshape_list_path",
           str(tmp_path / "names.txt"), "--output_path", str(tmp_path / "out.avi"), "--samples", "4", "--jpeg", "gpu"]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    payloads = video_payloads((tmp_path / "out.avi").read_bytes())
    assert len(payloads) == 4
    for data in payloads:
        assert jr.decode(data).size == (800, 800)
    raw4 = np.concatenate([f.copy() for f in iter_rendered_frames(renderers[1], MESH, BASIS, w[:1])])[0][..., ::-1]
    raw1 = np.concatenate([f.copy() for f in iter_rendered_frames(renderers[0], MESH, BASIS, w[:1])])[0][..., ::-1]
    first = np.asarray(jr.decode(payloads[0]))
    p4, p1 = jr.psnr(first, raw4), jr.psnr(first, raw1)
    print(f"first frame: {p4:.2f} dB to the raw 4-sample frame, {p1:.2f} dB to the 1-sample frame")
    assert p4 > 35.0 and p4 > p1
