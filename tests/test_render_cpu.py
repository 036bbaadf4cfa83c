"""The host side of the renderer, and the float64 restatement (tests/render_ref.py) against closed forms: mesh face readers, the AVI writer,
the colour-map rule, Rodrigues, coverage under the top-left rule, the BRDF by hand, the two CLIs' flags, and the ambiguity cap of the scenes
the GPU test renders."""
import importlib.util
import io
import os
import struct

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import render_ref as rr
from said_amd.render import colormap_index, colormap_table, light_positions, rodrigues
from said_amd.util import mesh as M
from said_amd.util.video import AviWriter, pcm16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUAD = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 2 0\nvt 0 0\nvn 0 0 1\n"


@pytest.mark.parametrize("faces,want", [
    ("f 1 2 3\n", [[0, 1, 2]]),
    ("f 1/1 2/1 3/1\n", [[0, 1, 2]]),
    ("f 1//1 2//1 3//1\n", [[0, 1, 2]]),
    ("f 1/1/1 2/1/1 4/1/1\n", [[0, 1, 3]]),
    ("f -5 -4 -3\n", [[0, 1, 2]]),
    ("f 1 2 3 4\n", [[0, 1, 2], [0, 2, 3]]),
    ("f 1 2 3 5 4\n", [[0, 1, 2], [0, 2, 4], [0, 4, 3]]),
], ids=["v", "v/vt", "v//vn", "v/vt/vn", "negative", "quad", "pentagon"])
def test_obj_face_forms(tmp_path, faces, want):
    p = tmp_path / "m.obj"
    p.write_text(QUAD + faces)
    m = M.load_mesh(str(p))
    assert m.faces.tolist() == want and m.vertices.shape == (5, 3)


def test_obj_negative_index_counts_vertices_read_so_far(tmp_path):
    p = tmp_path / "m.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nf -3 -2 -1\nv 0 1 0\nf -1 -2 -3\n")
    assert M.load_mesh(str(p)).faces.tolist() == [[0, 1, 2], [3, 2, 1]]


def test_obj_face_out_of_range_is_an_error(tmp_path):
    p = tmp_path / "m.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nf 1 2 4\n")
    with pytest.raises(M.MeshFormatError):
        M.load_mesh(str(p))


def test_ply_faces_ascii_and_binary(tmp_path):
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=np.float64)
    head = "ply\nformat {} 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n"
    a = tmp_path / "a.ply"
    a.write_text(head.format("ascii") + "".join(f"{x} {y} {z}\n" for x, y, z in v) + "3 0 1 2\n4 0 1 2 3\n")
    b = tmp_path / "b.ply"
    b.write_bytes(head.format("binary_little_endian").encode() + v.astype("<f4").tobytes() + struct.pack("<B3i", 3, 0, 1, 2) + struct.pack("<B4i", 4, 0, 1, 2, 3))
    for p in (a, b):
        m = M.load_mesh(str(p))
        assert m.faces.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3]] and np.array_equal(m.vertices, v)


@pytest.mark.parametrize("ext", ["obj", "ply"])
def test_save_mesh_round_trip(tmp_path, ext):
    rng = np.random.default_rng(3)
    m = M.Mesh(rng.normal(size=(17, 3)), rng.integers(0, 17, size=(9, 3)))
    p = str(tmp_path / f"m.{ext}")
    M.save_mesh(m, p)
    back = M.load_mesh(p)
    assert np.array_equal(back.vertices, m.vertices) and np.array_equal(back.faces, m.faces)
    assert np.array_equal(M.load_vertices(p), m.vertices)


def riff_chunks(data, start, end):
    pos = start
    while pos + 8 <= end:
        fcc, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        yield fcc, pos + 8, size
        pos += 8 + size + (size & 1)


@pytest.mark.parametrize("with_audio", [False, True])
def test_avi_writer(tmp_path, with_audio):
    from PIL import Image
    rng = np.random.default_rng(5)
    n, fps, rate = 7, 60, 16000
    audio = (rng.normal(size=3000) * 3000).astype(np.int16) if with_audio else None
    p = tmp_path / "v.avi"
    frames = []
    with AviWriter(str(p), fps, 800, 800, audio=audio, audio_rate=rate if with_audio else None) as w:
        for i in range(n):
            f = np.zeros((800, 800, 3), dtype=np.uint8)
            f[..., 0] = 200                    # B
            f[100 * i:100 * i + 50, :, 2] = 255  # R
            frames.append(f)
            w.write(f)
    data = p.read_bytes()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    top = list(riff_chunks(data, 12, len(data)))
    lists = {data[off:off + 4]: (off, size) for fcc, off, size in top if fcc == b"LIST"}
    assert set(lists) == {b"hdrl", b"movi"} and [fcc for fcc, _, _ in top] == [b"LIST", b"LIST", b"idx1"]
    hoff, hsize = lists[b"hdrl"]
    hdr = list(riff_chunks(data, hoff + 4, hoff + hsize))
    assert hdr[0][0] == b"avih"
    avih = struct.unpack("<14I", data[hdr[0][1]:hdr[0][1] + 56])
    assert avih[0] == round(1e6 / fps) and avih[4] == n and avih[6] == (2 if with_audio else 1) and avih[8:10] == (800, 800)
    strls = [(off, size) for fcc, off, size in hdr if fcc == b"LIST"]
    assert len(strls) == (2 if with_audio else 1)
    strh = data[strls[0][0] + 12:strls[0][0] + 12 + 56]
    assert strh[:8] == b"vidsMJPG"
    scale, r, _, length = struct.unpack("<4I", strh[20:36])
    assert r / scale == fps and length == n
    moff, msize = lists[b"movi"]
    movi = list(riff_chunks(data, moff + 4, moff + msize))
    video = [(off, size) for fcc, off, size in movi if fcc == b"00dc"]
    assert len(video) == n
    for (off, size), f in zip(video, frames):
        img = Image.open(io.BytesIO(data[off:off + size]))
        assert img.size == (800, 800) and img.format == "JPEG"
        a = np.asarray(img.convert("RGB")).astype(int)
        assert np.abs(a - f[..., ::-1]).mean() < 3   # B-G-R in, R-G-B in the JPEG
    pcm = b"".join(data[off:off + size] for fcc, off, size in movi if fcc == b"01wb")
    if with_audio:
        assert pcm == audio.astype("<i2").tobytes()
        astrh = data[strls[1][0] + 12:strls[1][0] + 12 + 56]
        assert astrh[:4] == b"auds" and struct.unpack("<I", astrh[32:36])[0] == len(audio)
        fmt = struct.unpack("<HHIIHH", data[strls[1][0] + 12 + 56 + 8:strls[1][0] + 12 + 56 + 8 + 16])
        assert fmt == (1, 1, rate, rate * 2, 2, 16)
    else:
        assert pcm == b""
    ioff, isize = next((off, size) for fcc, off, size in top if fcc == b"idx1")
    assert isize == 16 * len(movi)
    for k, (fcc, off, size) in enumerate(movi):   # idx1 offsets count from the 'movi' fourcc and point at the chunk header
        e = struct.unpack("<4sIII", data[ioff + 16 * k:ioff + 16 * k + 16])
        assert e == (fcc, 0x10, off - 8 - moff, size)
    assert pcm16(np.array([0.0, 1.0, -1.0, 2.0])).tolist() == [0, 32767, -32767, 32767]


def test_colormap_rule_matches_matplotlib():
    import matplotlib
    cmap = matplotlib.colormaps["viridis"]
    table = colormap_table("viridis")
    assert table.shape == (256, 3) and table.dtype == np.float32
    edge = 37 / 256
    xs = np.array([0.0, 1.0, np.nextafter(edge, 0), edge, np.nextafter(edge, 1), 0.5, np.nextafter(1.0, 0)])
    idx = colormap_index(xs)
    assert idx.tolist() == [0, 255, 36, 37, 37, 128, 255]
    assert np.array_equal(idx, rr.colormap_bin(xs))
    want = np.round(np.asarray(cmap(xs))[:, :3] * 255) / 255      # what matplotlib returns for the same x, as 8-bit levels
    assert np.array_equal(table[idx], want.astype(np.float32))


def test_rodrigues_against_scipy():
    rng = np.random.default_rng(7)
    for v in [np.zeros(3), [np.pi / 6, 0, 0], [0, -np.pi / 6, 0], [0, 0.3, 0], *rng.normal(size=(8, 3)), [1e-9, 0, 0], [0, np.pi, 0]]:
        assert np.abs(rodrigues(v) - Rotation.from_rotvec(v).as_matrix()).max() < 1e-14
    assert np.abs(light_positions(0.25) - rr.scene(0.25)["lights"]).max() < 1e-14
    assert np.allclose(light_positions(0.0)[1], [0, -0.5, np.sqrt(3) / 2])


def flat_scene(**kw):
    """An orthographic-like toy camera: f = 1 px per unit at depth 1, so screen x = X + cx and screen y = cy - Y for points at z = 0."""
    sc = dict(width=16, height=16, fx=1.0, fy=1.0, cx=0.0, cy=16.0, znear=0.01, zfar=3.0, cam=np.array([0.0, 0.0, 1.0]),
              lights=np.zeros((0, 3)), intensity=2.0, ambient=0.2, base=np.full(3, 0.3), metallic=0.8, roughness=0.8, vc_metallic=1.0, vc_roughness=1.0)
    sc.update(kw)
    return sc


def screen_tri(pts):
    """World vertices at z = 0 that flat_scene projects to the screen points pts (x, y)."""
    return np.array([[x, 16.0 - y, 0.0] for x, y in pts])


def test_coverage_is_the_analytic_top_left_set():
    """Two triangles that share the diagonal of the square [2, 10] x [3, 11], vertices ON pixel centres' grid lines (x.5): every sample of
    the square's top and left edges and none of its bottom and right edges is covered, and the diagonal's samples once."""
    sq = [(2.5, 3.5), (10.5, 3.5), (10.5, 11.5), (2.5, 11.5)]
    verts = screen_tri(sq)
    for faces in ([[0, 1, 2], [0, 2, 3]], [[2, 1, 0], [0, 2, 3]], [[0, 2, 3], [1, 2, 0]]):
        out = rr.render_frame(verts, np.array(faces), flat_scene(), normals=np.tile([0.0, 0.0, 1.0], (4, 1)))
        cover = out["face"] >= 0
        rows, cols = np.nonzero(cover)
        # pixel (r, c) samples (c + .5, r + .5): inside [2.5, 10.5) x [3.5, 11.5) means c in 2..9, r in 3..10
        want = np.zeros((16, 16), dtype=bool)
        want[3:11, 2:10] = True
        assert np.array_equal(cover, want)
        # exactly one owner per pixel: count coverage triangle by triangle
        total = sum((rr.render_frame(verts, np.array([f]), flat_scene(), normals=np.tile([0.0, 0.0, 1.0], (4, 1)))["face"] >= 0).astype(int) for f in faces)
        assert np.array_equal(total, want.astype(int))
        # the diagonal's samples (c - 2 == r - 3) are ambiguous by construction, interior samples are not
        assert out["ambiguous"][5, 4] and not out["ambiguous"][4, 6] and not out["ambiguous"][8, 3]


def test_depth_tie_goes_to_the_lower_face_and_nearer_wins():
    tri = [(2.5, 2.5), (12.5, 2.5), (2.5, 12.5)]
    verts = np.concatenate([screen_tri(tri), screen_tri(tri)])
    out = rr.render_frame(verts, np.array([[3, 4, 5], [0, 1, 2]]), flat_scene())
    assert set(np.unique(out["face"])) == {-1, 0} and out["ambiguous"][out["face"] == 0].all()
    verts[:3, 2] = 0.5   # now the second face is nearer (depth 0.5; its projection grows about the principal point)
    out = rr.render_frame(verts, np.array([[3, 4, 5], [0, 1, 2]]), flat_scene())
    both = rr.render_frame(verts[3:], np.array([[0, 1, 2]]), flat_scene())["face"] >= 0
    near = rr.render_frame(verts[:3], np.array([[0, 1, 2]]), flat_scene())["face"] >= 0
    assert (out["face"][near] == 1).all() and (out["face"][both & ~near] == 0).all()
    assert np.allclose(out["depth"][near], 0.5) and np.allclose(out["depth"][both & ~near], 1.0)


def test_plane_lit_head_on_equals_the_hand_computed_brdf():
    """A fronto-parallel plane at z = 0, one light at the camera (0, 0, 1): at the principal point N = V = L = H, so NdL = NdV = NdH = VdH = 1,
    d = 1, F = F0 and colour = ambient base + I ((1 - F0) c_diff / pi + F0 D Vis) with D = 1 / (pi a^2), Vis = 1 / 4, a = roughness^2."""
    sc = flat_scene(width=8, height=8, cx=3.5, cy=3.5, fx=100.0, fy=100.0, lights=np.array([[0.0, 0.0, 1.0]]))
    verts = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [-1.0, 1.0, 0.0]])
    out = rr.render_frame(verts, np.array([[0, 1, 2], [0, 2, 3]]), sc)
    base, met, rough, I = 0.3, 0.8, 0.8, 2.0
    a = rough * rough
    F0 = 0.04 * (1 - met) + base * met
    want = 0.2 * base + I * ((1 - F0) * base * 0.96 * (1 - met) / np.pi + F0 * (1 / (np.pi * a * a)) * 0.25)
    assert (out["face"] >= 0).all()
    assert np.allclose(out["color"][3, 3], want, rtol=0, atol=1e-12)     # pixel (3, 3) samples (3.5, 3.5), the principal point
    assert np.all(out["color"][0, 0] < out["color"][3, 3])               # off-axis: farther from the light and tilted
    assert np.array_equal(rr.to_bgr8(np.array([[[0.0, 0.5, 2.0]]]))[0, 0], [255, 128, 0])
    # difference mode: metallic 1, roughness 1 -> no diffuse term, F0 = vertex colour
    col = np.tile([0.2, 0.6, 1.0], (4, 1))
    out = rr.render_frame(verts, np.array([[0, 1, 2], [0, 2, 3]]), sc, colors=col)
    assert np.allclose(out["color"][3, 3], 0.2 * col[0] + I * col[0] * (1 / np.pi) * 0.25, rtol=0, atol=1e-12)


def test_normals_of_a_pyramid_and_a_flat_fan():
    v = np.array([[0, 0, 1.0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]])
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]])
    n = rr.vertex_normals(v, f)
    assert np.allclose(n[0], [0, 0, 1]) and np.allclose(np.linalg.norm(n, axis=1), 1)
    # angle weighting: a right-angle corner and a 45-degree corner of two faces with different normals
    v = np.array([[0, 0, 0.0], [1, 0, 0], [0, 1, 0], [0, 1, 1]])
    n = rr.vertex_normals(v, np.array([[0, 1, 2], [0, 2, 3]]))
    want = (np.pi / 2) * np.array([0, 0, 1.0]) + (np.pi / 4) * np.array([1.0, 0, 0])
    assert np.allclose(n[0], want / np.linalg.norm(want))
    assert np.array_equal(rr.vertex_normals(v, np.array([[0, 1, 1]])), np.zeros((4, 3)))   # no area, no normal


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "script", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags_and_defaults():
    flags = {a.dest: (a.type, a.default) for a in load_script("render").build_parser()._actions if a.dest != "help"}
    want = {"neutral_path": (str, "../BlendVOCA/templates_head/FaceTalk_170731_00024_TA.obj"),
            "blendshapes_dir": (str, "../BlendVOCA/blendshapes_head/FaceTalk_170731_00024_TA"),
            "audio_path": (str, "../BlendVOCA/audio/FaceTalk_170731_00024_TA/sentence01.wav"),
            "blendshape_coeffs_path": (str, "../BlendVOCA/blendshape_coeffs/FaceTalk_170731_00024_TA/sentence01.csv"),
            "show_difference": (bool, False),
            "target_diff_blendshape_coeffs_path": (str, "../BlendVOCA/blendshape_coeffs/FaceTalk_170731_00024_TA/sentence01.csv"),
            "max_diff": (float, 0.001), "fps": (int, 60), "output_path": (str, "../out.mp4"), "save_images": (bool, False),
            "output_images_dir": (str, "../out_imgs")}
    for k, v in want.items():
        assert flags[k] == v, k
    assert flags["blendshape_list_path"][0] is str
    mod = load_script("test_render")
    flags = {a.dest: (a.type, a.default) for a in mod.build_parser()._actions if a.dest != "help"}
    want = {"neutral_dir": (str, "../BlendVOCA/templates_head"), "audio_dir": (str, "../BlendVOCA/audio"),
            "coeffs_dir": (str, "../BlendVOCA/blendshape_coeffs"), "blendshapes_dir": (str, "../BlendVOCA/blendshapes_head"),
            "fps": (int, 60), "repeat_regex": (str, "(-.+)?"), "output_dir": (str, "../out_render")}
    for k, v in want.items():
        assert flags[k] == v, k
    assert flags["blendshape_list_path"][0] is str


def test_test_render_enumerates_like_the_reference(tmp_path):
    mod = load_script("test_render")
    pid = mod.PERSON_IDS_TEST[0]
    (tmp_path / "audio" / pid).mkdir(parents=True)
    (tmp_path / "coeffs" / pid).mkdir(parents=True)
    for s in ("sentence01.wav", "sentence03.wav"):
        (tmp_path / "audio" / pid / s).write_bytes(b"")
    for s in ("sentence01.csv", "sentence01-2.csv", "sentence02.csv", "sentence03-x.csv", "sentence03.txt"):
        (tmp_path / "coeffs" / pid / s).write_text("")
    got = mod.get_data_paths(str(tmp_path / "audio"), str(tmp_path / "coeffs"), "(-.+)?")
    assert sorted(os.path.basename(c) for _, _, c in got) == ["sentence01-2.csv", "sentence01.csv", "sentence03-x.csv"]
    assert [os.path.basename(c) for _, _, c in mod.get_data_paths(str(tmp_path / "audio"), str(tmp_path / "coeffs"), "")] == ["sentence01.csv"]


def test_ambiguous_pixels_stay_under_the_cap():
    """Over the scenes of tests/test_gpu_render.py the restatement's own ambiguous pixels are under 0.1 % of the covered ones.  (Estimate:
    2.3k triangles of about 35 px perimeter give 40k px of edge, times 2e-4 px, a handful of pixels per frame of about 1.3e5 covered.)
    The flag depends on the geometry only, so plain and difference frames share it: each (frame, rotation) is rendered once."""
    neutral, basis, faces = rr.arkit_mesh(os.path.join(ROOT, "tests", "golden"))
    w, wt = rr.scene_coeffs()
    assert w.shape == (rr.N_FRAMES, 32) and w.min() >= 0 and w.max() <= 1 and wt.min() >= 0 and wt.max() <= 1
    verts = rr.blend(neutral, basis, w)
    sc = rr.scene()
    for rot in {c[1] for c in rr.CASES}:
        covered = ambiguous = 0
        for t in range(rr.N_FRAMES):
            out = rr.render_frame(verts[t], faces, sc, rot=rot, t_center=neutral.mean(axis=0))
            covered += int((out["face"] >= 0).sum())
            ambiguous += int(out["ambiguous"].sum())
        print(f"rot {rot}: {ambiguous} ambiguous of {covered} covered pixels")
        assert covered > 8 * 100000
        assert ambiguous < 1e-3 * covered
