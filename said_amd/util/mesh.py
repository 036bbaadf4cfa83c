"""Mesh readers and writers without trimesh (reference: said/util/mesh.py:load_mesh, trimesh.load(process=False, maintain_order=True)).

``load_vertices`` reads only the vertex positions, as (V, 3) float64 in file order: that is all the blendshape-coefficient fit
(script/optimize_blendshape_coeffs.py) uses.  ``load_mesh`` also reads the faces, for the renderer: OBJ ``f`` records in the ``v``,
``v/vt``, ``v//vn`` and ``v/vt/vn`` forms, negative (relative) indices included, and PLY ``face`` lists (``vertex_indices`` or
``vertex_index``), ascii and binary little-endian; polygons are split into a fan around their first vertex.  ``save_mesh`` writes OBJ
or PLY that both readers take back.  OBJ: every ``v x y z [...]`` line, extra components (w, vertex colours) ignored,
every other record skipped.  PLY: ``ascii`` and ``binary_little_endian`` with float / double x, y, z; other vertex properties
and every other element (faces included, list properties too) are skipped.  Anything else raises ``MeshFormatError``."""
from __future__ import annotations

import os

import numpy as np


class MeshFormatError(ValueError):
    pass


def load_vertices(path: str) -> np.ndarray:
    """(V, 3) float64 vertex positions of an OBJ or PLY file, in file order."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".obj":
        return _load_obj(path)
    if ext == ".ply":
        return _load_ply(path)
    raise MeshFormatError(f"{path}: unsupported mesh format {ext!r} (OBJ and PLY only)")


def _load_obj(path: str) -> np.ndarray:
    rows = []
    with open(path, "r") as f:
        for ln, line in enumerate(f, 1):
            if line.startswith("v ") or line.startswith("v\t"):
                parts = line.split()
                if len(parts) < 4:
                    raise MeshFormatError(f"{path}:{ln}: vertex with fewer than 3 coordinates")
                rows.append((float(parts[1]), float(parts[2]), float(parts[3])))
    return np.asarray(rows, dtype=np.float64).reshape(-1, 3)


_PLY_TYPES = {
    "char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
    "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8",
}


def _load_ply(path: str) -> np.ndarray:
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise MeshFormatError(f"{path}: not a PLY file")
    nl = data.find(b"\n", end)
    body = data[nl + 1:]
    fmt, elements = None, []   # elements: [name, count, [(prop name, dtype) or (prop name, (count dtype, item dtype))]]
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        p = line.split()
        if not p or p[0] in ("comment", "obj_info"):
            continue
        if p[0] == "format":
            fmt = p[1]
        elif p[0] == "element":
            elements.append([p[1], int(p[2]), []])
        elif p[0] == "property":
            if not elements:
                raise MeshFormatError(f"{path}: property before any element")
            if p[1] == "list":
                if p[2] not in _PLY_TYPES or p[3] not in _PLY_TYPES:
                    raise MeshFormatError(f"{path}: unknown list property types {p[2]} {p[3]}")
                elements[-1][2].append((p[4], (_PLY_TYPES[p[2]], _PLY_TYPES[p[3]])))
            else:
                if p[1] not in _PLY_TYPES:
                    raise MeshFormatError(f"{path}: unknown property type {p[1]}")
                elements[-1][2].append((p[2], _PLY_TYPES[p[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise MeshFormatError(f"{path}: PLY format {fmt!r} is not supported (ascii and binary_little_endian only)")
    vert = next((e for e in elements if e[0] == "vertex"), None)
    if vert is None:
        raise MeshFormatError(f"{path}: no vertex element")
    names = [n for n, _ in vert[2]]
    for c in "xyz":
        if c not in names:
            raise MeshFormatError(f"{path}: vertex element has no {c} property")
        if dict(vert[2])[c] not in ("f4", "f8"):
            raise MeshFormatError(f"{path}: vertex {c} is {dict(vert[2])[c]}, not float or double")
    if fmt == "ascii":
        return _ply_ascii(path, body, elements)
    return _ply_binary(path, body, elements)


def _ply_ascii(path, body, elements):
    lines = body.decode("ascii", "replace").splitlines()
    pos = 0
    for name, count, props in elements:
        if name != "vertex":
            pos += count   # one record per line, lists included
            continue
        idx = [n for n, _ in props]
        if any(isinstance(t, tuple) for _, t in props):
            raise MeshFormatError(f"{path}: list properties in the vertex element are not supported")
        cols = [idx.index(c) for c in "xyz"]
        if pos + count > len(lines):
            raise MeshFormatError(f"{path}: {count} vertices announced, file ends early")
        out = np.empty((count, 3), dtype=np.float64)
        for i in range(count):
            p = lines[pos + i].split()
            if len(p) < len(props):
                raise MeshFormatError(f"{path}: vertex {i} has {len(p)} values, expected {len(props)}")
            out[i] = [float(p[c]) for c in cols]
        return out
    raise MeshFormatError(f"{path}: no vertex element")


def _ply_binary(path, body, elements):
    off = 0
    for name, count, props in elements:
        if any(isinstance(t, tuple) for _, t in props):
            if name == "vertex":
                raise MeshFormatError(f"{path}: list properties in the vertex element are not supported")
            for _ in range(count):   # variable-length records: walk them
                for _, t in props:
                    if isinstance(t, tuple):
                        cdt, idt = np.dtype("<" + t[0]), np.dtype("<" + t[1])
                        n = int(np.frombuffer(body, dtype=cdt, count=1, offset=off)[0])
                        off += cdt.itemsize + n * idt.itemsize
                    else:
                        off += np.dtype(t).itemsize
            continue
        dt = np.dtype([(n, "<" + t) for n, t in props])
        if name == "vertex":
            if off + count * dt.itemsize > len(body):
                raise MeshFormatError(f"{path}: {count} vertices announced, file ends early")
            rec = np.frombuffer(body, dtype=dt, count=count, offset=off)
            return np.stack([rec[c].astype(np.float64) for c in "xyz"], axis=1)
        off += count * dt.itemsize
    raise MeshFormatError(f"{path}: no vertex element")


class Mesh:
    """What the renderer needs of a trimesh.Trimesh: ``vertices`` (V, 3) float64 and ``faces`` (F, 3) int64, in file order."""

    def __init__(self, vertices, faces):
        self.vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)


def _fan(poly, out) -> None:
    for i in range(1, len(poly) - 1):
        out.append((poly[0], poly[i], poly[i + 1]))


def load_mesh(path: str) -> Mesh:
    """Vertices and triangles of an OBJ or PLY file; a face that names a vertex the file does not hold raises MeshFormatError."""
    vertices = load_vertices(path)
    ext = os.path.splitext(path)[1].lower()
    faces = _obj_faces(path) if ext == ".obj" else _ply_faces(path)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(vertices)):
        raise MeshFormatError(f"{path}: a face names vertex {int(f.max() if f.max() >= len(vertices) else f.min())}, the file holds {len(vertices)}")
    return Mesh(vertices, f)


def _obj_faces(path: str):
    faces, nv = [], 0
    with open(path, "r") as f:
        for ln, line in enumerate(f, 1):
            if line.startswith("v ") or line.startswith("v\t"):
                nv += 1
            elif line.startswith("f ") or line.startswith("f\t"):
                poly = []
                for tok in line.split()[1:]:
                    try:
                        i = int(tok.split("/")[0])
                    except ValueError:
                        raise MeshFormatError(f"{path}:{ln}: face element {tok!r} does not start with a vertex index") from None
                    if i == 0:
                        raise MeshFormatError(f"{path}:{ln}: OBJ indices start at 1")
                    poly.append(i - 1 if i > 0 else nv + i)   # negative: relative to the vertices read so far
                if len(poly) < 3:
                    raise MeshFormatError(f"{path}:{ln}: face with fewer than 3 vertices")
                _fan(poly, faces)
    return faces


def _ply_faces(path: str):
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    body = data[data.find(b"\n", end) + 1:]
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        p = line.split()
        if not p:
            continue
        if p[0] == "format":
            fmt = p[1]
        elif p[0] == "element":
            elements.append([p[1], int(p[2]), []])
        elif p[0] == "property":
            elements[-1][2].append((p[4], (_PLY_TYPES[p[2]], _PLY_TYPES[p[3]])) if p[1] == "list" else (p[2], _PLY_TYPES[p[1]]))
    faces = []
    if fmt == "ascii":
        lines = body.decode("ascii", "replace").splitlines()
        pos = 0
        for name, count, props in elements:
            if name == "face":
                for i in range(count):
                    vals = lines[pos + i].split()
                    at = 0
                    for pname, t in props:
                        if isinstance(t, tuple):
                            n = int(vals[at])
                            if pname in ("vertex_indices", "vertex_index"):
                                _fan([int(v) for v in vals[at + 1:at + 1 + n]], faces)
                            at += 1 + n
                        else:
                            at += 1
            pos += count
        return faces
    off = 0
    for name, count, props in elements:
        if not any(isinstance(t, tuple) for _, t in props):
            off += count * sum(np.dtype(t).itemsize for _, t in props)
            continue
        for _ in range(count):
            for pname, t in props:
                if isinstance(t, tuple):
                    cdt, idt = np.dtype("<" + t[0]), np.dtype("<" + t[1])
                    if off + cdt.itemsize > len(body):
                        raise MeshFormatError(f"{path}: {name} element ends early")
                    n = int(np.frombuffer(body, dtype=cdt, count=1, offset=off)[0])
                    off += cdt.itemsize
                    if off + n * idt.itemsize > len(body):
                        raise MeshFormatError(f"{path}: {name} element ends early")
                    if name == "face" and pname in ("vertex_indices", "vertex_index"):
                        _fan([int(v) for v in np.frombuffer(body, dtype=idt, count=n, offset=off)], faces)
                    off += n * idt.itemsize
                else:
                    off += np.dtype(t).itemsize
    return faces


def save_mesh(mesh, path: str) -> None:
    """Write ``mesh.vertices`` and ``mesh.faces`` as OBJ (17 significant digits: float64 round-trips) or binary little-endian PLY (double x, y, z)."""
    v = np.asarray(mesh.vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(mesh.faces, dtype=np.int64).reshape(-1, 3)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".obj":
        with open(path, "w") as out:
            out.writelines(f"v {x!r} {y!r} {z!r}\n" for x, y, z in v.tolist())
            out.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f.tolist())
    elif ext == ".ply":
        head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty double x\nproperty double y\nproperty double z\n"
                f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
        rec = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
        rec["n"], rec["i"] = 3, f
        with open(path, "wb") as out:
            out.write(head.encode("ascii") + v.astype("<f8").tobytes() + rec.tobytes())
    else:
        raise MeshFormatError(f"{path}: unsupported mesh format {ext!r} (OBJ and PLY only)")


def get_submesh(vertices, faces, indices) -> Mesh:
    """The part of a mesh on the vertices ``indices`` (reference: said/util/mesh.py:get_submesh): vertex i of the result is vertex
    ``indices[i]``; a face is kept, in its place in the order, when all three of its vertices are among them (the first occurrence of an
    index that is listed twice), and is renumbered."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= len(v)):
        raise MeshFormatError(f"a sub-mesh index lies outside the mesh's {len(v)} vertices")
    new = np.full(len(v), -1, dtype=np.int64)
    new[idx[::-1]] = np.arange(len(idx))[::-1]   # the first occurrence wins
    sub = new[f] if f.size else f
    return Mesh(v[idx], sub[(sub >= 0).all(axis=1)] if f.size else f)
