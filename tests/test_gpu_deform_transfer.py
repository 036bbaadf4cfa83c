"""GPU tests of deformation transfer (said_amd/csrc/deform_transfer.hip, include/said_transfer.h, said_amd/optimize/deformation_transfer.py,
script/transfer_blendshapes.py) against the float64 restatement of DESIGN.md section 17 in tests/deform_transfer_ref.py, which assembles with
scipy.sparse and solves with a sparse LU.

Bounds.  The solver promises |A'(b - A x)| <= tol |A'b| per column; recomputed in numpy the residual may be 10 tol (rounding of the
recomputation).  How far an iterate that meets this promise lies from the direct solution is a matter of the system's conditioning, not of
the implementation (frame inverses span 1.9e3 .. 2.2e7 on the ARKit mesh), so distances are judged against a yardstick: the distance of
scipy's Jacobi-preconditioned cg at the same tolerance from the same direct solution, times MARGIN; both distances are taken per column and relative to the
column's largest entry, since a column's error scales with its right-hand side.  Two conjugate-gradient iterations that stop under the same residual threshold stop at different iterates and with different spectral content in their last residual; a residual
of a given norm moves the solution by 1 / lambda(A'A) of its content, so their distances from the direct solution differ by a moderate
factor in either direction.  MARGIN = 10 allows one decade (DESIGN.md 17.6 records the measured ratios: 0.7 to 4.6).  The direct formulas
(frame inverses, gradients, normals) are held to 1e-12 of each matrix's norm.  Searches must agree exactly but for near ties."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import deform_transfer_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = 1e-10
MARGIN = 10.0
NAMES = ["jawOpen", "mouthSmileLeft", "browInnerUp"]
NEAR_CAP = 0.001   # at most 0.1 % of a search's entries may be near ties


@pytest.fixture(scope="module")
def arkit():
    g = np.load(os.path.join(GOLDEN, "g13_blendshape_qp.npz"))
    faces = np.load(os.path.join(GOLDEN, "g15_render.npz"))["faces"].astype(np.int64)
    names = [str(n) for n in g["names51"]]
    marks = np.loadtxt(os.path.join(GOLDEN, "g20_arkit_landmarks.txt"), dtype=np.int64)
    return {"neutral": g["neutral"], "faces": faces, "shapes51": g["shapes51"], "names": names, "marks": marks,
            "shapes3": g["shapes51"][[names.index(n) for n in NAMES]]}


@pytest.fixture(scope="module")
def targets(arkit):
    tv, tf = R.split_in_four(arkit["neutral"], arkit["faces"])
    plain = R.known_map(tv)
    return {"faces": tf, "plain": plain, "warped": R.warp(plain, plain)}


@pytest.fixture(scope="module")
def eng():
    from said_amd import _engine
    e = _engine.TransferEngine(torch.device("cuda:0"))
    yield e
    e.close()


def _session():
    from said_amd.optimize.deformation_transfer import DeformationTransfer
    return DeformationTransfer("cuda:0", TOL, 20000)


def _static_anchors(neutral, shapes):
    return np.nonzero((shapes == neutral[None]).all(axis=(0, 2)))[0]


@pytest.fixture(scope="module")
def systems(arkit):
    """The two systems of the solver test, each with 67 right-hand-side columns, the direct solution and the yardstick."""
    out = {}
    rng = np.random.default_rng(7)
    for name in ("patch", "arkit"):
        if name == "patch":
            verts, faces = R.grid_patch()
            anchors = np.array([0, 12, 24])
            shapes = verts[None] + 0.03 * rng.standard_normal((3,) + verts.shape)
        else:
            verts, faces, shapes = arkit["neutral"], arkit["faces"], arkit["shapes3"]
            anchors = _static_anchors(verts, arkit["shapes51"])
        nf = faces.shape[0]
        pairs = np.stack([np.arange(nf), np.arange(nf)], axis=1)
        a, b9 = R.transfer_system(R.known_map(verts), faces, pairs, anchors, verts, faces, shapes)
        # 67 columns: the nine of the three shapes, then combinations of them with seeded weights
        b = np.concatenate([b9, b9 @ rng.standard_normal((9, 58))], axis=1)
        x = R.solve_normal(a, b)
        out[name] = {"a": a.tocsr(), "at": a.T.tocsr(), "b": b, "x": x, "yard": R.jacobi_cg_distance(a, b, x, TOL, columns=(0, 1, 2, 66))}
    return out


def _solve(eng, s, cols, **kw):
    a, at = s["a"], s["at"]
    return eng.solve(a.indptr, a.indices, a.data, at.indptr, at.indices, at.data, s["b"][:, cols], tol=TOL, **kw)


def _check_solution(s, cols, x, status, resid, what):
    a, b = s["a"], s["b"][:, cols]
    r = a.T @ (b - a @ x)
    rel = np.linalg.norm(r, axis=0) / np.linalg.norm(a.T @ b, axis=0)
    dist = R.relative_distance(x, s["x"][:, cols]).max()
    print(f"{what}: recomputed residual {rel.max():.3e} (reported {resid.max():.3e}), relative distance to splu {dist:.3e}, yardstick {s['yard']:.3e}")
    assert (status == 0).all()
    assert (rel <= 10 * TOL).all()
    assert dist <= MARGIN * s["yard"]


@pytest.mark.parametrize("name", ["patch", "arkit"])
def test_solver_alone(eng, systems, name):
    s = systems[name]
    all67 = np.arange(67)
    x67, st, it, res = _solve(eng, s, all67)
    print(f"{name}: m {s['a'].shape[0]} n {s['a'].shape[1]} iterations {it.min()} .. {it.max()}")
    _check_solution(s, all67, x67, st, res, f"{name} R=67")
    again = _solve(eng, s, all67)
    assert np.array_equal(again[0], x67) and np.array_equal(again[2], it) and np.array_equal(again[3], res)
    x3, st3, it3, res3 = _solve(eng, s, np.arange(3))
    _check_solution(s, np.arange(3), x3, st3, res3, f"{name} R=3")
    assert np.array_equal(x3, x67[:, :3]) and np.array_equal(it3, it[:3])
    x1, st1, it1, res1 = _solve(eng, s, np.array([66]))
    _check_solution(s, np.array([66]), x1, st1, res1, f"{name} R=1")
    assert np.array_equal(x1[:, 0], x67[:, 66]) and it1[0] == it[66] and res1[0] == res[66]
    # a block of iterations of another length looks at the flags at other times and changes nothing
    other = _solve(eng, s, np.arange(3), check_every=7)
    assert np.array_equal(other[0], x3)


@pytest.mark.parametrize("name", ["patch", "arkit"])
def test_solver_max_iter_is_per_column(eng, systems, name):
    """Column 0 starts at the direct solution and passes at once; the others start at 0 and cannot get there in 5 iterations."""
    s = systems[name]
    x0 = np.zeros((s["a"].shape[1], 3))
    x0[:, 0] = s["x"][:, 0]
    x, st, it, res = _solve(eng, s, np.arange(3), x0=x0, max_iter=5)
    assert list(st) == [0, 1, 1] and list(it) == [0, 5, 5]
    assert np.array_equal(x[:, 0], x0[:, 0]) and res[0] <= TOL and (res[1:] > TOL).all()


def test_closed_form_uniform_scale(arkit):
    """Identity correspondence, the target a scaled and translated source: the residuals are 1.7 x the source's displacements."""
    src, faces, shapes = arkit["neutral"], arkit["faces"], arkit["shapes3"]
    tgt = R.known_map(src)
    nf = faces.shape[0]
    pairs = np.stack([np.arange(nf), np.arange(nf)], axis=1)
    anchors = R.default_anchors(src, shapes, tgt, tgt)
    want = 1.7 * (shapes - src[None])
    ref = R.transfer(tgt, faces, pairs, anchors, src, faces, shapes)
    ref_err = abs(ref - want).max()
    dt = _session()
    dt.set_source(src, faces, shapes)
    dt.set_target(tgt, faces)
    assert np.array_equal(dt.default_anchors(tgt), anchors)
    got, report = dt.transfer(pairs, anchors)
    dt.close()
    err = abs(got - want).max()
    print(f"closed form: error {err:.3e}, splu's {ref_err:.3e}, iterations {report.iters.max()}")
    assert got.shape == (3, src.shape[0], 3) and ref_err < 1e-7
    assert err <= MARGIN * ref_err


@pytest.mark.parametrize("mesh", ["patch", "arkit"])
def test_mesh_passes(eng, arkit, mesh):
    if mesh == "patch":
        verts, faces = R.grid_patch()
        deformed = verts[None] + 0.04 * np.random.default_rng(2).standard_normal((3,) + verts.shape)
    else:
        verts, faces, deformed = arkit["neutral"], arkit["faces"], arkit["shapes3"]
    got = eng.mesh(verts, faces)
    got["q"] = eng.gradients(verts, faces, deformed)
    want = {"w": R.frame_inverse_t(verts, faces), "gc": R.g_table(verts, faces), "fn": R.face_normals(verts, faces), "centroid": R.centroids(verts, faces),
            "vn": R.vertex_normals(verts, faces), "q": np.stack([R.deformation_gradients(verts, d, faces) for d in deformed])}
    for key, w in want.items():
        g = got[key]
        assert g.shape == w.shape, key
        axes = tuple(range(w.ndim - (2 if key in ("w", "gc", "q") else 1), w.ndim))
        norm = np.sqrt((w * w).sum(axis=axes, keepdims=True))
        worst = (abs(g - w) / norm).max()
        print(f"{mesh} {key}: worst error {worst:.2e} of the norm")
        assert worst <= 1e-12, key


def _agree(got, want, near, what):
    """Equal but for the entries the restatement itself calls near ties, of which there may be at most NEAR_CAP."""
    assert near.sum() <= NEAR_CAP * near.size, f"{what}: the restatement has {near.sum()} near ties in {near.size} entries"
    wrong = np.nonzero(got != want)[0]
    print(f"{what}: {near.sum()} near ties, {wrong.size} entries differ")
    assert near[wrong].all(), f"{what}: entries {wrong[:8]} differ without a near tie"
    return wrong.size == 0


@pytest.fixture(scope="module")
def ref_reg(arkit, targets):
    return R.register(arkit["neutral"], arkit["faces"], targets["warped"], targets["faces"], arkit["marks"], arkit["marks"])


def test_closest_without_a_compatible_point(eng):
    verts, faces = R.grid_patch()
    vn = R.vertex_normals(verts, faces)
    q = verts + 0.01
    qn = vn.copy()
    qn[::3] *= -1.0                       # every third query faces away from every target
    idx, d2 = eng.closest(q, qn, verts, vn)
    want, near = R.closest_valid(q, qn, verts, vn)
    assert (want[::3] == -1).all() and (want[1::3] >= 0).all()
    assert _agree(idx, want, near, "patch")
    plain, _ = eng.closest(q, None, verts, None)
    assert np.array_equal(plain, R.closest_valid(q, None, verts, None)[0])
    # an exact tie goes to the lower index
    tie, _ = eng.closest(np.array([[0.5, 0.0, 0.0]]), None, np.array([[1.0, 0, 0], [0.0, 0, 0], [0.0, 0, 0]]), None)
    assert tie[0] == 0


def test_closest_and_correspondence(eng, arkit, targets, ref_reg):
    xs = ref_reg[0]
    src_faces, tgt, tf = arkit["faces"], targets["warped"], targets["faces"]
    reg = xs[-1][:1220]
    tn = R.vertex_normals(tgt, tf)
    idx, _ = eng.closest(reg, R.vertex_normals(reg, src_faces), tgt, tn)
    want, near = R.closest_valid(reg, R.vertex_normals(reg, src_faces), tgt, tn)
    _agree(idx, want, near, "closest valid vertex")
    pairs, t2s, s2t, near_t, near_s = R.triangle_correspondence(reg, src_faces, tgt, tf)
    limit = 0.05 * np.linalg.norm(tgt.max(axis=0) - tgt.min(axis=0))
    cs, ct = R.centroids(reg, src_faces), R.centroids(tgt, tf)
    t2s_thr = np.where((t2s >= 0) & (np.sqrt(((ct - cs[np.maximum(t2s, 0)]) ** 2).sum(axis=1)) <= limit), t2s, -1)
    s2t_thr = np.where((s2t >= 0) & (np.sqrt(((cs - ct[np.maximum(s2t, 0)]) ** 2).sum(axis=1)) <= limit), s2t, -1)
    eng.set_source(arkit["neutral"], src_faces)
    eng.set_target(tgt, tf)
    g_t2s, g_s2t, _, _ = eng.correspond(0.05, reg)
    same = _agree(g_t2s, t2s_thr, near_t, "target to source") & _agree(g_s2t, s2t_thr, near_s, "source to target")
    dt = _session()
    dt.set_source(arkit["neutral"], src_faces)
    dt.set_target(tgt, tf)
    got = dt.triangle_correspondence(reg, 0.05)
    dt.close()
    print(f"{pairs.shape[0]} pairs, {np.unique(pairs[:, 1]).size} of {tf.shape[0]} target triangles paired")
    if same:
        assert np.array_equal(got, pairs)
    # a tighter threshold drops pairs
    assert (eng.correspond(0.001, reg)[0] >= 0).sum() < (g_t2s >= 0).sum()


def test_registration(arkit, targets, ref_reg):
    xs, closest, ref_systems = ref_reg
    src, faces, tgt, tf, marks = arkit["neutral"], arkit["faces"], targets["warped"], targets["faces"], arkit["marks"]
    dt = _session()
    dt.set_source(src, faces)
    dt.set_target(tgt, tf)
    reg = dt.register(marks, marks)
    dt.close()
    assert reg.solutions.shape == (5, 1220 + 2304, 3) and (reg.report.status == 0).all()
    truth = R.warp(R.known_map(src), targets["plain"])
    diag = np.linalg.norm(tgt.max(axis=0) - tgt.min(axis=0))
    for j in range(5):
        if j > 0:
            idx, near = closest[j]
            assert _agree(reg.closest[j], idx, near, f"solve {j}: closest points"), "a near tie was decided differently: the solves that follow solve another system"
        a, b, free = ref_systems[j]
        yard = R.jacobi_cg_distance(a, b, xs[j][free], TOL)
        dist = R.relative_distance(reg.solutions[j][free], xs[j][free]).max()
        mean = np.linalg.norm(reg.solutions[j][:1220] - truth, axis=1).mean() / diag
        print(f"solve {j}: iterations {reg.report.iters[j].max()}, distance to the restatement {dist:.3e}, yardstick {yard:.3e}, "
              f"mean distance to the known map {mean:.2e} of the diagonal")
        assert np.array_equal(reg.solutions[j][marks], tgt[marks])
        assert dist <= MARGIN * yard
    assert np.array_equal(reg.vertices, reg.solutions[-1][:1220])


@pytest.mark.parametrize("target", ["plain", "warped"])
def test_end_to_end(arkit, targets, ref_reg, target):
    from said_amd.optimize.deformation_transfer import transfer_blendshapes
    src, faces, shapes, marks = arkit["neutral"], arkit["faces"], arkit["shapes3"], arkit["marks"]
    tgt, tf = targets[target], targets["faces"]
    xs = ref_reg[0] if target == "warped" else R.register(src, faces, tgt, tf, marks, marks)[0]
    reg = xs[-1][:1220]
    pairs = R.triangle_correspondence(reg, faces, tgt, tf)[0]
    # the anchors come from the vertices static in the shapes that are transferred
    anchors = R.default_anchors(src, shapes, reg, tgt)
    a, b = R.transfer_system(tgt, tf, pairs, anchors, src, faces, shapes)
    x = R.solve_normal(a, b)
    want = x[:tgt.shape[0]].reshape(-1, 3, 3).transpose(1, 0, 2) - tgt[None]
    yard = R.jacobi_cg_distance(a, b, x, TOL, columns=(0, 4, 8))
    details = {}
    got = transfer_blendshapes(src, faces, shapes, tgt, tf, marks, marks, tol=TOL, details=details)
    assert got.shape == (3, tgt.shape[0], 3) and got.dtype == np.float64
    assert np.array_equal(details["pairs"], pairs) and np.array_equal(details["anchors"], anchors)
    nv = tgt.shape[0]
    got_x = (got + tgt[None]).transpose(1, 0, 2).reshape(nv, 9)
    dist = R.relative_distance(got_x, x[:nv]).max()
    print(f"{target}: {pairs.shape[0]} pairs, {anchors.size} anchors, transfer iterations {details['report'].iters.max()}, distance to the restatement "
          f"{dist:.3e}, yardstick {yard:.3e}")
    assert dist <= MARGIN * yard
    if target == "plain":
        known = 1.7 * (shapes - src[None])
        big = np.linalg.norm(known, axis=2).max(axis=1)                       # the largest displacement of each shape
        err_ref = np.linalg.norm(want[:, :1220] - known, axis=2) / big[:, None]
        err_got = np.linalg.norm(got[:, :1220] - known, axis=2) / big[:, None]
        for k, name in enumerate(NAMES):
            print(f"{name}: against 1.7 x source, mean {err_got[k].mean():.3%} / worst {err_got[k].max():.3%} of the largest displacement "
                  f"(restatement {err_ref[k].mean():.3%} / {err_ref[k].max():.3%})")
        slack = MARGIN * yard * abs(x[:nv]).max() / big[:, None]
        assert (err_got <= err_ref + slack).all()


def test_cli(tmp_path, arkit, targets):
    """script/transfer_blendshapes.py on OBJ files, its pickle into script/preprocess_blendvoca.py, whose meshes load_mesh reads back."""
    from said_amd.util.blendshape import load_blendshape_deltas
    from said_amd.util.mesh import Mesh, load_mesh, save_mesh
    src_dir, templates, out = tmp_path / "arkit", tmp_path / "templates", tmp_path / "out"
    src_dir.mkdir()
    templates.mkdir()
    save_mesh(Mesh(arkit["neutral"], arkit["faces"]), str(src_dir / "Neutral.obj"))
    for name, shape in zip(NAMES, arkit["shapes3"]):
        save_mesh(Mesh(shape, arkit["faces"]), str(src_dir / f"{name}.obj"))
    # a template with 20 extra, unused vertices in front: the crop list takes them away
    extra = np.zeros((20, 3))
    save_mesh(Mesh(np.vstack([extra, targets["plain"]]), targets["faces"] + 20), str(templates / "head_one.obj"))
    (tmp_path / "names.txt").write_text("\n".join(NAMES) + "\n")
    (tmp_path / "marks.txt").write_text("\n".join(map(str, arkit["marks"])) + "\n")
    (tmp_path / "crop.txt").write_text("\n".join(map(str, range(20, 20 + targets["plain"].shape[0]))) + "\n")
    pickle_path = tmp_path / "blendshape_residuals.pickle"
    cmd = [sys.executable, os.path.join(ROOT, "script", "transfer_blendshapes.py"), "--source_dir", str(src_dir), "--blendshape_list_path", str(tmp_path / "names.txt"),
           "--templates_dir", str(templates), "--head_idx_path", str(tmp_path / "crop.txt"), "--source_markers_path", str(tmp_path / "marks.txt"),
           "--target_markers_path", str(tmp_path / "marks.txt"), "--blendshape_residuals_path", str(pickle_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    print(r.stdout.strip())
    deltas = load_blendshape_deltas(str(pickle_path))
    assert type(deltas) is dict and list(deltas) == ["head_one"] and list(deltas["head_one"]) == NAMES
    known = 1.7 * (arkit["shapes3"] - arkit["neutral"][None])
    for k, name in enumerate(NAMES):
        d = deltas["head_one"][name]
        assert type(d) is np.ndarray and d.shape == targets["plain"].shape and d.dtype == np.float64
        assert np.linalg.norm(d[:1220] - known[k], axis=1).mean() <= 0.02 * np.linalg.norm(known[k], axis=1).max()
    cmd = [sys.executable, os.path.join(ROOT, "script", "preprocess_blendvoca.py"), "--templates_dir", str(templates), "--blendshape_residuals_path", str(pickle_path),
           "--blendshapes_out_dir", str(out), "--head_idx_path", str(tmp_path / "crop.txt"), "--blendshape_list_path", str(tmp_path / "names.txt")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    neutral = load_mesh(str(out / "templates_head" / "head_one.obj"))
    assert np.array_equal(neutral.vertices, targets["plain"]) and np.array_equal(neutral.faces, targets["faces"])
    for name in NAMES:
        m = load_mesh(str(out / "blendshapes_head" / "head_one" / f"{name}.obj"))
        assert np.array_equal(m.vertices, targets["plain"] + deltas["head_one"][name]) and np.array_equal(m.faces, targets["faces"])
