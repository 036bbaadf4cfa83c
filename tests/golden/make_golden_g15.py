"""Generate golden G15 (tests/golden/g15_render.npz): the triangle list of the ARKit reference mesh.

Runs only where the reference checkout is present (never on the GPU box).  Stored: ``faces`` (2304, 3) int32, zero-based, from the ``f``
records of Neutral.obj in data/ARKit_reference_blendshapes.zip, in file order.  The vertices and the blendshapes of the same archive are
golden G13's (``neutral``, ``shapes51``, ``names32``): this maker asserts that the OBJ's vertices equal G13's ``neutral``, so the two
fixtures describe one mesh.

Usage:  python tests/golden/make_golden_g15.py
"""
import io
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def main():
    with zipfile.ZipFile(os.path.join(REF, "data", "ARKit_reference_blendshapes.zip")) as zf:
        name = next(n for n in zf.namelist() if os.path.basename(n) == "Neutral.obj")
        lines = zf.read(name).decode().splitlines()
    verts = np.array([[float(x) for x in ln.split()[1:4]] for ln in lines if ln.startswith("v ")])
    faces = np.array([[int(tok.split("/")[0]) - 1 for tok in ln.split()[1:]] for ln in lines if ln.startswith("f ")], dtype=np.int32)
    g13 = np.load(os.path.join(HERE, "g13_blendshape_qp.npz"))
    assert verts.shape == g13["neutral"].shape and np.array_equal(verts, g13["neutral"]), "Neutral.obj and golden G13 disagree"
    assert faces.ndim == 2 and faces.shape[1] == 3 and faces.min() >= 0 and faces.max() < len(verts)
    buf = io.BytesIO()
    np.savez_compressed(buf, faces=faces)
    with open(os.path.join(HERE, "g15_render.npz"), "wb") as f:
        f.write(buf.getvalue())
    print({"faces": faces.shape, "bytes": len(buf.getvalue())})


if __name__ == "__main__":
    main()
