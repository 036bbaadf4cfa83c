"""Host halves of the blendshape-coefficient fit (said_amd.optimize, script/optimize_blendshape_coeffs.py): mesh readers, parse_list,
the problem assembly against the reference's own QP (golden G13), the driver's enumeration and head-index handling, and the optimality
certificate on a known optimum.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
from scipy.optimize import lsq_linear

from said_amd.optimize import kkt_certificate, reference_qp
from said_amd.util.mesh import MeshFormatError, load_vertices
from said_amd.util.parser import parse_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G13 = np.load(os.path.join(ROOT, "tests", "golden", "g13_blendshape_qp.npz"))
VERTS = np.array([[0.5, -1.25, 3.0], [1e-3, 2.0, -0.125], [7.0, 8.5, 9.25], [-4.0, 0.0, 1.5]])


def _driver():
    spec = importlib.util.spec_from_file_location("said_optimize_driver", os.path.join(ROOT, "script", "optimize_blendshape_coeffs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_obj_vertices_in_file_order(tmp_path):
    p = tmp_path / "m.obj"
    p.write_text("# c\no m\nv 0.5 -1.25 3.0\nvn 0 0 1\nv 0.001 2 -0.125 1.0\nvt 0.1 0.2\nv 7 8.5 9.25 0.1 0.2 0.3\nf 1 2 3\nv -4 0 1.5\n")
    assert np.array_equal(load_vertices(str(p)), VERTS)


def test_ascii_ply_with_extra_properties_and_faces(tmp_path):
    p = tmp_path / "m.ply"
    body = "".join(f"{i} {float(x)!r} {float(y)!r} {float(z)!r} 255\n" for i, (x, y, z) in enumerate(VERTS))
    p.write_text("ply\nformat ascii 1.0\ncomment x\nelement vertex 4\nproperty int id\nproperty double x\nproperty double y\nproperty double z\n"
                 "property uchar red\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n" + body + "3 0 1 2\n3 1 2 3\n")
    assert np.array_equal(load_vertices(str(p)), VERTS)


@pytest.mark.parametrize("dtype", ["float", "double"])
def test_binary_ply(tmp_path, dtype):
    p = tmp_path / "m.ply"
    npt = "<f4" if dtype == "float" else "<f8"
    rec = np.zeros(4, dtype=[("nx", "<f4"), ("x", npt), ("y", npt), ("z", npt), ("q", "u1")])
    rec["x"], rec["y"], rec["z"] = VERTS.T
    faces = b"".join(np.uint8(3).tobytes() + np.array(f, dtype="<i4").tobytes() for f in ([0, 1, 2], [1, 2, 3]))
    hdr = (f"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float nx\nproperty {dtype} x\nproperty {dtype} y\n"
           f"property {dtype} z\nproperty uchar q\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n")
    p.write_bytes(hdr.encode() + rec.tobytes() + faces)
    v = load_vertices(str(p))
    assert v.dtype == np.float64
    assert np.array_equal(v, VERTS.astype(npt).astype(np.float64))   # float32 converts to float64 exactly


def test_mesh_rejects_other_formats(tmp_path):
    p = tmp_path / "m.ply"
    p.write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n" + bytes(12))
    with pytest.raises(MeshFormatError, match="big_endian"):
        load_vertices(str(p))
    q = tmp_path / "m.stl"
    q.write_text("solid")
    with pytest.raises(MeshFormatError):
        load_vertices(str(q))


def test_parse_list(tmp_path):
    p = tmp_path / "l.txt"
    p.write_text("jawOpen\n mouthClose \n3\n")
    assert parse_list(str(p), str) == ["jawOpen", "mouthClose", "3"]
    p.write_text("5\n 7\n11\n")
    assert parse_list(str(p), int) == [5, 7, 11]


def _basis32():
    n = G13["neutral"].reshape(-1, 1)
    names51 = list(G13["names51"])
    B = np.concatenate([G13["shapes51"][names51.index(s)].reshape(-1, 1) for s in G13["names32"]], axis=1)
    return n, B


@pytest.mark.parametrize("T", [2, 3, 6])
def test_assembly_matches_reference_qp(T):
    n, B = _basis32()
    frames = [v.reshape(-1, 1) for v in G13[f"full{T}_verts"]]
    P, q, G, h, lb, ub = reference_qp(B - n, n, frames, float(G13["delta"]))
    assert np.array_equal(P, G13[f"full{T}_P"])
    assert np.array_equal(q, G13[f"full{T}_q"])
    assert np.array_equal(G, G13[f"full{T}_G"]) and np.array_equal(h, G13[f"full{T}_h"])
    assert np.array_equal(lb, G13[f"full{T}_lb"]) and np.array_equal(ub, G13[f"full{T}_ub"])


def test_single_assembly_matches_reference():
    n, B = _basis32()
    bd = B - n
    assert np.array_equal(bd.T @ bd, G13["single_P"])
    assert np.array_equal((bd.T @ (n - G13["single_verts"].reshape(-1, 1))).reshape(-1), G13["single_q"])


def test_certificate_on_known_optimum():
    """Single frames (delta None) solved exactly by BVLS: their KKT multipliers are the gradient's sign-split at the bounds."""
    n, B = _basis32()
    bd = B - n
    P = bd.T @ bd
    rng = np.random.default_rng(3)
    v = n.T + rng.uniform(-0.2, 1.2, size=(1, 32)) @ bd.T
    w = lsq_linear(bd, (v.T - n).reshape(-1), bounds=(0, 1), method="bvls", tol=1e-15).x
    q = (bd.T @ (n - v.T)).reshape(1, -1)
    g = P @ w + q[0]
    z = np.zeros((1, 4, 32))
    z[0, 0] = np.where(w <= 0, np.maximum(g, 0), 0)
    z[0, 1] = np.where(w >= 1, np.maximum(-g, 0), 0)
    c = kkt_certificate(P, q, None, w[None], z)
    assert c["stationarity"] <= 1e-12 and abs(c["gap"]) <= 1e-12 and c["min_dual"] >= 0
    z[0, 0] *= 0.5   # a wrong multiplier breaks stationarity and opens the gap
    c = kkt_certificate(P, q, None, w[None], z)
    assert c["stationarity"] > 1e-6 and c["gap"] > 1e-9


def test_driver_enumeration_and_head_indices(tmp_path):
    drv = _driver()
    pid = drv.PERSON_IDS[0]
    d = tmp_path / pid / "sentence02"
    (d / "sub").mkdir(parents=True)
    for name in ("b.obj", "a.ply", "sub/c.obj", "notes.txt"):
        (d / name).write_text("v 0 0 0\n")
    (tmp_path / pid / "sentence05").mkdir()
    assert drv.sequence_paths(str(tmp_path), pid, 1) == []
    got = drv.sequence_paths(str(tmp_path), pid, 2)
    assert got == sorted([str(d / "b.obj"), str(d / "sub" / "c.obj"), str(d / "a.ply")])
    assert drv.sequence_paths(str(tmp_path), pid, 5) == []
    f = tmp_path / "frame.obj"
    f.write_text("".join(f"v {i} {i + 0.5} {-i}\n" for i in range(6)))
    full = drv.load_frames([str(f)], None)[0]
    sub = drv.load_frames([str(f)], [4, 1])[0]
    assert full.shape == (18, 1) and np.array_equal(sub.reshape(-1), [4, 4.5, -4, 1, 1.5, -1])
    assert len(drv.PERSON_IDS) == 12 and drv.SENTENCE_IDS == list(range(1, 41))


def test_driver_flags(tmp_path, capsys):
    drv = _driver()
    a = drv.build_parser().parse_args(["--head_idx_path", ""])
    assert (a.neutrals_dir, a.blendshapes_dir, a.mesh_seqs_dir, a.blendshapes_coeffs_out_dir) == (
        "../BlendVOCA/templates_head", "../BlendVOCA/blendshapes_head", "../BlendVOCA/unposedcleaneddata", "../output_coeffs")
    assert a.delta == 0.1 and a.blendshape_list_path is None
    with pytest.raises(SystemExit):
        drv.main([])
    assert "--head_idx_path is required" in capsys.readouterr().err
    out = tmp_path / "out"
    (out / drv.PERSON_IDS[0]).mkdir(parents=True)
    with pytest.raises(FileExistsError):
        drv.main(["--head_idx_path", "", "--blendshapes_coeffs_out_dir", str(out)])
