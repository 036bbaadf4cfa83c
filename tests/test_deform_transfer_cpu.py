"""CPU checks of deformation transfer: the host-built index structures of said_amd/optimize/deformation_transfer.py
and get_submesh against the restatement (tests/deform_transfer_ref.py), the landmark fixture, the residuals pickle's layout and script/preprocess_blendvoca.py's round trip."""
import os
import pickle

import numpy as np
import pytest

import deform_transfer_ref as R
from said_amd import _engine
from said_amd.optimize import deformation_transfer as DT
from said_amd.util.blendshape import load_blendshape_deltas, save_blendshape_deltas
from said_amd.util.mesh import Mesh, get_submesh, load_mesh, save_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _arkit():
    g = np.load(os.path.join(GOLDEN, "g13_blendshape_qp.npz"))
    faces = np.load(os.path.join(GOLDEN, "g15_render.npz"))["faces"].astype(np.int64)
    return g["neutral"], faces


def _dense_equal(a, b, scale=1.0):
    d = abs(a - b)
    return d.shape == a.shape and (d.max() if d.nnz else 0.0) <= 1e-12 * scale


@pytest.mark.parametrize("mesh", ["patch", "arkit"])
def test_registration_structure_matches_the_restatement(mesh):
    verts, faces = R.grid_patch() if mesh == "patch" else _arkit()
    nv = verts.shape[0]
    st = DT.registration_structure(faces, nv)
    assert (DT.edge_pairs(faces) == R.edge_pairs(faces)).all()
    rng = np.random.default_rng(3)
    closest = rng.integers(-1, 7, nv)                    # some vertices without a closest point
    cpos = rng.standard_normal((nv, 3))
    w_s, w_i, w_c = 1.3, 0.02, 7.0
    mine = R.host_values(st, R.g_table(verts, faces), np.sqrt([w_s, w_i, w_c, 1.0]), closest)
    ref_a, _ = R.registration_system(verts, faces, w_s, w_i, w_c, cpos, closest >= 0)
    # the restatement leaves the rows of vertices without a closest point out; here they are rows of zeros
    keep = np.ones(st["m"], bool)
    keep[st["m"] - nv:] = closest >= 0
    assert _dense_equal(mine[np.nonzero(keep)[0]], ref_a, abs(ref_a).max())
    assert mine[np.nonzero(~keep)[0]].nnz == 0 or abs(mine[np.nonzero(~keep)[0]]).max() == 0.0
    # no column twice in a row, columns ascending; A' points back into A
    for i in range(st["m"]):
        c = st["col"][st["rowptr"][i]:st["rowptr"][i + 1]]
        assert (np.diff(c) > 0).all()
    import scipy.sparse as sp
    at = sp.csr_matrix((mine.data[st["at_src"]], st["at_col"], st["at_rowptr"]), shape=(st["n"], st["m"]))
    assert abs(at - mine.T).nnz == 0 or abs(at - mine.T).max() == 0.0
    # fixed columns are emptied
    fixed = np.array([0, 5, nv - 1])
    masked = R.host_values(st, R.g_table(verts, faces), np.sqrt([w_s, w_i, w_c, 1.0]), closest, fixed)
    assert abs(masked[:, fixed]).sum() == 0.0


def test_transfer_structure_matches_the_restatement():
    verts, faces = R.grid_patch()
    tv, tf = R.split_in_four(verts, faces)
    tv = R.known_map(tv)
    rng = np.random.default_rng(5)
    pairs = np.unique(np.stack([rng.integers(0, faces.shape[0], 90), rng.integers(0, tf.shape[0] - 9, 90)], axis=1), axis=0)   # the last triangles unpaired
    anchors = np.array([2, 11, 40])
    shapes = verts[None] + 0.05 * rng.standard_normal((2,) + verts.shape)
    st = DT.transfer_structure(tf, tv.shape[0], pairs, anchors)
    mine = R.host_values(st, R.g_table(tv, tf), [0.0, 0.0, 0.0, 1.0])
    ref_a, ref_b = R.transfer_system(tv, tf, pairs, anchors, verts, faces, shapes)
    assert _dense_equal(mine, ref_a, abs(ref_a).max())
    # the right-hand side's description: pair rows name 3 s + r, identity rows r, anchor rows their vertex
    q = np.stack([R.deformation_gradients(verts, s, faces) for s in shapes])
    b = np.zeros_like(ref_b)
    for i in range(st["m"]):
        cls, aux = st["rhsclass"][i], st["rowaux"][i]
        for k in range(2):
            b[i, 3 * k:3 * k + 3] = q[k, aux // 3][:, aux % 3] if cls == 0 else np.eye(3)[aux] if cls == 1 else tv[aux]
    assert np.array_equal(b, ref_b)


def test_edge_pairs_refuses_a_non_manifold_edge():
    faces = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    with pytest.raises(DT.MeshTopologyError):
        DT.edge_pairs(faces)
    with pytest.raises(ValueError):
        R.edge_pairs(faces)


def test_get_submesh_matches_the_restatement():
    verts, faces = R.grid_patch(6)
    rng = np.random.default_rng(1)
    idx = rng.permutation(verts.shape[0])[:25].tolist()
    sub = get_submesh(verts, faces, idx)
    rv, rf = R.submesh(verts, faces, idx)
    assert np.array_equal(sub.vertices, rv) and np.array_equal(sub.faces, rf) and rf.shape[0] > 0
    whole = get_submesh(verts, faces, list(range(verts.shape[0])))
    assert np.array_equal(whole.faces, faces) and np.array_equal(whole.vertices, verts)


def test_landmark_fixture():
    marks = np.loadtxt(os.path.join(GOLDEN, "g20_arkit_landmarks.txt"), dtype=np.int64)
    assert marks.shape == (68,) and np.unique(marks).size == 68 and marks.min() >= 0 and marks.max() < 1220


def test_split_mesh_keeps_the_original_vertices():
    verts, faces = _arkit()
    tv, tf = R.split_in_four(verts, faces)
    assert tv.shape == (4746, 3) and tf.shape == (9216, 3) and np.array_equal(tv[:1220], verts)
    assert R.edge_pairs(tf).shape[0] > 0   # still manifold


def test_no_cpu_path():
    import torch
    with pytest.raises(_engine.NoCpuPathError):
        _engine.TransferEngine(torch.device("cpu"))


def _import_script(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "script", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pickle_layout_and_preprocess_round_trip(tmp_path):
    """Two persons, templates larger than their heads: the pickle is {person: {name: (V, 3) float64}} of plain types, and
    preprocess_blendvoca.py writes cropped neutrals and neutral + residual blendshapes that load_mesh reads back."""
    verts, faces = R.grid_patch(6)
    head_idx = [i for i in range(verts.shape[0]) if i % 6 != 5]          # drop one column of the grid
    names = ["jawOpen", "mouthSmileLeft"]
    rng = np.random.default_rng(11)
    templates = tmp_path / "templates"
    templates.mkdir()
    residuals, heads = {}, {}
    for n, pid in enumerate(["personA", "personB"]):
        tv = verts * (1.0 + 0.1 * n)
        save_mesh(Mesh(tv, faces), str(templates / (pid + (".ply" if n == 0 else ".obj"))))
        heads[pid] = get_submesh(tv, faces, head_idx)
        residuals[pid] = {name: 0.01 * rng.standard_normal((len(head_idx), 3)) for name in names}
    path = tmp_path / "blendshape_residuals.pickle"
    save_blendshape_deltas(residuals, str(path))
    with open(path, "rb") as f:
        raw = pickle.load(f)
    assert type(raw) is dict and list(raw) == ["personA", "personB"]
    for pid in raw:
        assert type(raw[pid]) is dict and list(raw[pid]) == names
        for name in names:
            assert type(raw[pid][name]) is np.ndarray and raw[pid][name].dtype == np.float64 and raw[pid][name].shape == (len(head_idx), 3)
    assert np.array_equal(load_blendshape_deltas(str(path))["personB"]["jawOpen"], residuals["personB"]["jawOpen"])
    idx_file, list_file, out = tmp_path / "head_idx.txt", tmp_path / "names.txt", tmp_path / "out"
    idx_file.write_text("\n".join(map(str, head_idx)) + "\n")
    list_file.write_text("\n".join(names) + "\n")
    pre = _import_script("preprocess_blendvoca")
    argv = ["--templates_dir", str(templates), "--blendshape_residuals_path", str(path), "--blendshapes_out_dir", str(out), "--head_idx_path", str(idx_file),
            "--blendshape_list_path", str(list_file)]
    assert pre.main(argv) == 0
    for pid in raw:
        neutral = load_mesh(str(out / "templates_head" / (pid + ".obj")))
        assert np.array_equal(neutral.vertices, heads[pid].vertices) and np.array_equal(neutral.faces, heads[pid].faces)
        for name in names:
            m = load_mesh(str(out / "blendshapes_head" / pid / (name + ".obj")))
            assert np.array_equal(m.vertices, heads[pid].vertices + residuals[pid][name]) and np.array_equal(m.faces, heads[pid].faces)
    with pytest.raises(SystemExit):
        pre.main(argv)   # the output exists now


def test_preprocess_flags_of_the_reference():
    pre = _import_script("preprocess_blendvoca")
    args = pre.build_parser().parse_args([])
    assert args.templates_dir == "../BlendVOCA/templates" and args.blendshapes_out_dir == "../output_blendshapes"
    assert args.blendshape_residuals_path.endswith("blendshape_residuals.pickle")
