"""Generate golden G13 (tests/golden/g13_blendshape_qp.npz): the ARKit reference basis and the quadratic programs the reference poses.

Runs only where the reference checkout is present (never on the GPU box).  Stored:
  (a) the basis of data/ARKit_reference_blendshapes.zip: the neutral (1220 x 3 vertices) and all 51 blendshapes, their names, and the
      32 names of data/ARKit_blendshapes.txt (the columns of the 32-shape basis, in that order);
  (b) the reference's own QP: said/optimize/blendshape_coeffs.py is loaded with a stub ``qpsolvers`` module whose ``solve_qp`` records its
      arguments, and (P, q, G, h, lb, ub) are captured for seeded synthetic sequences of T = 2, 3 and 6 frames (T = 1 raises
      in the reference's compute_g) on the 32-shape basis, and
      for one OptimizationProblemSingle call.  The synthetic targets are stored too.

Usage:  python tests/golden/make_golden_g13.py
"""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"
CASES_T = (2, 3, 6)   # T = 1 cannot be captured: the reference's compute_g raises in scipy.sparse.block_diag on an empty list
DELTA = 0.1


def obj_vertices(text: str) -> np.ndarray:
    return np.array([[float(x) for x in ln.split()[1:4]] for ln in text.splitlines() if ln.startswith("v ")])


def load_basis():
    with zipfile.ZipFile(os.path.join(REF, "data", "ARKit_reference_blendshapes.zip")) as zf:
        objs = {os.path.splitext(os.path.basename(n))[0]: obj_vertices(zf.read(n).decode()) for n in zf.namelist() if n.endswith(".obj")}
    neutral = objs.pop("Neutral")
    names51 = sorted(objs)
    return neutral, names51, np.stack([objs[n] for n in names51])


def reference_module(calls):
    stub = types.ModuleType("qpsolvers")

    def solve_qp(P, q, G=None, h=None, A=None, b=None, lb=None, ub=None, solver=None, initvals=None, **kw):
        calls.append(dict(P=np.array(P, dtype=np.float64), q=np.array(q, dtype=np.float64),
                          G=None if G is None else np.asarray(G.toarray() if hasattr(G, "toarray") else G, dtype=np.float64),
                          h=None if h is None else np.array(h, dtype=np.float64), lb=np.array(lb), ub=np.array(ub), solver=solver))
        return np.full(np.shape(q), 0.5)

    stub.solve_qp = solve_qp
    sys.modules["qpsolvers"] = stub
    spec = importlib.util.spec_from_file_location("ref_blendshape_coeffs", os.path.join(REF, "said", "optimize", "blendshape_coeffs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    neutral, names51, shapes51 = load_basis()
    names32 = [ln.strip() for ln in open(os.path.join(REF, "data", "ARKit_blendshapes.txt"))]
    idx32 = [names51.index(n) for n in names32]
    n = neutral.reshape(-1, 1)
    B = np.concatenate([shapes51[i].reshape(-1, 1) for i in idx32], axis=1)
    calls = []
    ref = reference_module(calls)
    rng = np.random.default_rng(1313)
    out = {"neutral": neutral, "shapes51": shapes51, "names51": np.array(names51), "names32": np.array(names32), "delta": DELTA}
    full = ref.OptimizationProblemFull(n, B)
    for T in CASES_T:
        w = rng.uniform(-0.2, 1.2, size=(T, 32))
        verts = n.T + w @ (B - n).T + 1e-4 * rng.normal(size=(T, n.shape[0]))
        calls.clear()
        full.optimize([v.reshape(-1, 1) for v in verts], delta=DELTA)
        c = calls[0]
        out[f"full{T}_verts"] = verts
        for k in ("P", "q", "G", "h", "lb", "ub"):
            if c[k] is not None:
                out[f"full{T}_{k}"] = c[k]
    single = ref.OptimizationProblemSingle(n, B)
    v = n.T + rng.uniform(-0.2, 1.2, size=(1, 32)) @ (B - n).T
    calls.clear()
    single.optimize(v.reshape(-1, 1), None)
    out["single_verts"] = v[0]
    for k in ("P", "q", "lb", "ub"):
        out[f"single_{k}"] = calls[0][k]
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    with open(os.path.join(HERE, "g13_blendshape_qp.npz"), "wb") as f:
        f.write(buf.getvalue())
    print({k: np.shape(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
