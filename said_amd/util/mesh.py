"""Mesh vertex readers without trimesh (reference: said/util/mesh.py:load_mesh, trimesh.load(process=False, maintain_order=True)).

Only the vertex positions are read, as (V, 3) float64 in file order: that is all the blendshape-coefficient fit
(script/optimize_blendshape_coeffs.py) uses.  OBJ: every ``v x y z [...]`` line, extra components (w, vertex colours) ignored,
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
