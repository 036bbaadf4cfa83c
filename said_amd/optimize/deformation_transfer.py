"""Blendshapes for a new head by deformation transfer (Sumner & Popovic 2004) on the MI355X: DESIGN.md section 17, include/said_transfer.h.

Three stages share one device solver (conjugate gradients on the normal equations, said_amd/csrc/deform_transfer.hip):

1. ``register``: the source neutral is deformed onto the target neutral, markers fixed, with a rising closest-point weight;
2. ``triangle_correspondence``: triangles of the registered source and of the target are paired by centroid distance and normal;
3. ``transfer``: the source's deformation gradients of every blendshape are imposed on the paired target triangles.

This module builds the index structure of each system with numpy (which unknowns a row touches, and which frame-inverse coefficients make
up each entry); the values, the right-hand sides, the searches and the solves run on the device, in float64.  There is no CPU path.

Stated choices: the closest point of a source vertex is the closest target *vertex* with a compatible normal, not the closest surface
point; marker vertices are hard constraints; translation is fixed by soft anchors (weight 1) at target vertices near the source vertices no
blendshape moves."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import _engine

WC_SCHEDULE = (0.0, 1.0, 5000.0 ** (1.0 / 3.0), 5000.0 ** (2.0 / 3.0), 5000.0)
NONE, ONE = -1, -2   # coefficient codes of an entry: no term, the constant 1


class TransferError(_engine.EngineError):
    pass


class MeshTopologyError(TransferError, ValueError):
    """An edge shared by more than two triangles, a marker outside the mesh, ..."""


class NotConvergedError(TransferError):
    """A solve left columns unconverged; ``info`` holds the solver's report."""

    def __init__(self, message: str, info=None):
        super().__init__(message)
        self.info = info


class NoAnchorError(TransferError, ValueError):
    """No blendshape-static source vertex and no explicit anchor list: the transfer's translation would be free."""


@dataclass
class SolveReport:
    """Per right-hand-side column: status (0 converged), iterations, final relative residual |A'(b - A x)| / |A'b|."""
    status: np.ndarray
    iters: np.ndarray
    resid: np.ndarray


@dataclass
class Registration:
    vertices: np.ndarray                 # (V_s, 3): the registered source
    solutions: np.ndarray                # (solves, V_s + F_s, 3)
    closest: np.ndarray                  # (solves, V_s): target vertex used per source vertex, -1 for none
    report: SolveReport = field(repr=False, default=None)


def edge_pairs(faces: np.ndarray) -> np.ndarray:
    """(P, 2) pairs t < u of triangles that share an edge, each once, sorted; raises on an edge of more than two triangles."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nf = f.shape[0]
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    owner = np.tile(np.arange(nf), 3)
    key = np.minimum(a, b) * (int(f.max()) + 1) + np.maximum(a, b)
    order = np.lexsort((owner, key))
    key, owner = key[order], owner[order]
    same = key[1:] == key[:-1]
    if (same[1:] & same[:-1]).any():
        raise MeshTopologyError("an edge is shared by more than two triangles: non-manifold meshes are not supported")
    pairs = np.stack([owner[:-1][same], owner[1:][same]], axis=1)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    return np.unique(np.sort(pairs, axis=1), axis=0)


def _assemble(rows, cols, c0, c1, m: int, n: int, rowclass, rowaux, rhsclass=None) -> dict:
    """CSR of A with entries of one (row, column) merged, and CSR of A' pointing back into A's entries."""
    key = rows.astype(np.int64) * n + cols
    order = np.argsort(key, kind="stable")
    key, c0, c1 = key[order], c0[order], c1[order]
    first = np.ones(key.shape[0], dtype=bool)
    first[1:] = key[1:] != key[:-1]
    gid = np.cumsum(first) - 1
    ukey = key[first]
    m0 = np.full(ukey.shape[0], -3, dtype=np.int64)
    m1 = np.full(ukey.shape[0], -3, dtype=np.int64)
    np.maximum.at(m0, gid, c0)
    np.maximum.at(m1, gid, c1)
    urow, ucol = ukey // n, ukey % n
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(urow, minlength=m), out=rowptr[1:])
    at_src = np.argsort(ucol * m + urow, kind="stable")
    at_rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ucol, minlength=n), out=at_rowptr[1:])
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)   # noqa: E731
    return {"m": m, "n": n, "rowptr": i32(rowptr), "col": i32(ucol), "c0": i32(m0), "c1": i32(m1), "rowclass": i32(rowclass), "rowaux": i32(rowaux),
            "rhsclass": None if rhsclass is None else i32(rhsclass), "at_rowptr": i32(at_rowptr), "at_col": i32(urow[at_src]), "at_src": i32(at_src)}


def _g_entries(faces: np.ndarray, nv: int, tri: np.ndarray):
    """Per (triangle of tri, row r, slot): the column and the coefficient index of G_t; arrays of shape (len(tri), 3, 4)."""
    f = faces[tri]
    cols = np.stack([f[:, 0], f[:, 1], f[:, 2], nv + tri], axis=1)[:, None, :].repeat(3, axis=1)
    coef = 12 * tri[:, None, None] + 4 * np.arange(3)[None, :, None] + np.arange(4)[None, None, :]
    return cols, coef


def registration_structure(faces: np.ndarray, nv: int) -> dict:
    """The system of w_S E_S + w_I E_I + w_C E_C over the V + F unknowns of the source: three rows per edge pair (G_t - G_u), three per
    triangle (G_t), one per vertex (its closest point).  Marker columns are emptied on the device, after their part of the right-hand side."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nf = f.shape[0]
    pairs = edge_pairs(f)
    npair = pairs.shape[0]
    ct, kt = _g_entries(f, nv, pairs[:, 0])
    cu, ku = _g_entries(f, nv, pairs[:, 1])
    srow = (3 * np.arange(npair)[:, None, None] + np.arange(3)[None, :, None]).repeat(4, axis=2)
    ci, ki = _g_entries(f, nv, np.arange(nf))
    irow = 3 * npair + (3 * np.arange(nf)[:, None, None] + np.arange(3)[None, :, None]).repeat(4, axis=2)
    base = 3 * npair + 3 * nf
    none_s, none_i, none_c = np.full(srow.size, NONE), np.full(irow.size, NONE), np.full(nv, NONE)
    rows = np.concatenate([srow.ravel(), srow.ravel(), irow.ravel(), base + np.arange(nv)])
    cols = np.concatenate([ct.ravel(), cu.ravel(), ci.ravel(), np.arange(nv)])
    c0 = np.concatenate([kt.ravel(), none_s, ki.ravel(), np.full(nv, ONE)])
    c1 = np.concatenate([none_s, ku.ravel(), none_i, none_c])
    rowclass = np.concatenate([np.full(3 * npair, _engine.TRANSFER_ROW_SMOOTH), np.full(3 * nf, _engine.TRANSFER_ROW_IDENTITY), np.full(nv, _engine.TRANSFER_ROW_CLOSEST)])
    rowaux = np.concatenate([np.zeros(3 * npair, dtype=np.int64), np.tile(np.arange(3), nf), np.arange(nv)])
    return _assemble(rows, cols, c0, c1, base + nv, nv + nf, rowclass, rowaux)


def transfer_structure(faces: np.ndarray, nv: int, pairs: np.ndarray, anchors: np.ndarray) -> dict:
    """The transfer system over the V + F unknowns of the target: three rows G_t per pair (s, t), three per unpaired triangle, one per anchor."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nf = f.shape[0]
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    anchors = np.asarray(anchors, dtype=np.int64).reshape(-1)
    if pairs.size and (pairs[:, 1].min() < 0 or pairs[:, 1].max() >= nf or pairs[:, 0].min() < 0):
        raise TransferError("a pair names a triangle outside the meshes")
    if anchors.size and (anchors.min() < 0 or anchors.max() >= nv):
        raise TransferError(f"an anchor names a vertex outside the target's {nv}")
    unpaired = np.setdiff1d(np.arange(nf), pairs[:, 1])
    tri = np.concatenate([pairs[:, 1], unpaired])
    nblock = tri.shape[0]
    cg, kg = _g_entries(f, nv, tri)
    grow = (3 * np.arange(nblock)[:, None, None] + np.arange(3)[None, :, None]).repeat(4, axis=2)
    na = anchors.shape[0]
    rows = np.concatenate([grow.ravel(), 3 * nblock + np.arange(na)])
    cols = np.concatenate([cg.ravel(), anchors])
    c0 = np.concatenate([kg.ravel(), np.full(na, ONE)])
    c1 = np.full(rows.shape[0], NONE)
    m = 3 * nblock + na
    rhsclass = np.concatenate([np.full(3 * pairs.shape[0], _engine.TRANSFER_RHS_PAIR), np.full(3 * unpaired.shape[0], _engine.TRANSFER_RHS_IDENTITY),
                               np.full(na, _engine.TRANSFER_RHS_ANCHOR)])
    rowaux = np.concatenate([(3 * pairs[:, 0:1] + np.arange(3)).ravel(), np.tile(np.arange(3), unpaired.shape[0]), anchors])
    return _assemble(rows, cols, c0, c1, m, nv + nf, np.full(m, _engine.TRANSFER_ROW_UNIT), rowaux, rhsclass)


def _mesh(vertices, faces, what: str):
    v = np.ascontiguousarray(vertices, dtype=np.float64)
    f = np.ascontiguousarray(faces, dtype=np.int32)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0:
        raise TransferError(f"{what}: vertices (V, 3) and faces (F, 3) expected, got {v.shape} and {f.shape}")
    if f.min() < 0 or f.max() >= v.shape[0]:
        raise MeshTopologyError(f"{what}: a face names a vertex outside the mesh's {v.shape[0]}")
    return v, f


def _check(report: SolveReport, what: str, strict: bool) -> None:
    bad = np.nonzero(np.asarray(report.status).ravel() != _engine.TRANSFER_CONVERGED)[0]
    if strict and bad.size:
        raise NotConvergedError(f"{what}: {bad.size} right-hand-side column(s) did not converge (first: column {int(bad[0])}, relative residual "
                                f"{float(np.asarray(report.resid).ravel()[bad[0]]):.3e}); raise max_iter or loosen tol", report)


class DeformationTransfer:
    """One source (neutral, faces, K shapes) and one target at a time on one GPU."""

    def __init__(self, device="cuda", tol: float = 1e-10, max_iter: int = 20000, strict: bool = True):
        self.engine = _engine.TransferEngine(torch.device(device))
        self.tol, self.max_iter, self.strict = float(tol), int(max_iter), bool(strict)
        self.source = self.target = self.shapes = None

    def close(self) -> None:
        self.engine.close()

    def set_source(self, neutral, faces, shapes=None) -> None:
        v, f = _mesh(neutral, faces, "source")
        sh = None if shapes is None else np.ascontiguousarray(shapes, dtype=np.float64)
        if sh is not None and (sh.ndim != 3 or sh.shape[1:] != v.shape):
            raise TransferError(f"source shapes must be (K, {v.shape[0]}, 3), got {sh.shape}")
        edge_pairs(f)   # refuses a non-manifold source before anything is uploaded
        self.engine.set_source(v, f, sh)
        self.source, self.shapes = (v, f), sh

    def set_target(self, neutral, faces) -> None:
        v, f = _mesh(neutral, faces, "target")
        self.engine.set_target(v, f)
        self.target = (v, f)

    def register(self, source_markers: Sequence[int], target_markers: Sequence[int], w_s: float = 1.0, w_i: float = 0.001, schedule=WC_SCHEDULE) -> Registration:
        (sv, sf), (tv, _) = self.source, self.target
        ms, mt = np.asarray(source_markers, dtype=np.int64).reshape(-1), np.asarray(target_markers, dtype=np.int64).reshape(-1)
        if ms.shape != mt.shape or ms.size == 0:
            raise TransferError(f"{ms.size} source markers and {mt.size} target markers: equally many, at least one")
        if ms.min() < 0 or ms.max() >= sv.shape[0] or mt.min() < 0 or mt.max() >= tv.shape[0] or np.unique(ms).size != ms.size:
            raise MeshTopologyError("a marker names a vertex outside its mesh, or a source vertex twice")
        structure = registration_structure(sf, sv.shape[0])
        x, closest, st, it, res = self.engine.register(structure, ms, tv[mt], w_s, w_i, schedule, self.tol, self.max_iter)
        report = SolveReport(st, it, res)
        _check(report, "registration", self.strict)
        return Registration(x[-1, :sv.shape[0]].copy(), x, closest, report)

    def triangle_correspondence(self, registered=None, threshold: float = 0.05) -> np.ndarray:
        """(M, 2) rows (source triangle, target triangle): the union of both search directions, sorted, unique, many-to-many."""
        t2s, s2t, _, _ = self.engine.correspond(threshold, registered)
        a = np.stack([t2s, np.arange(t2s.shape[0])], axis=1)[t2s >= 0]
        b = np.stack([np.arange(s2t.shape[0]), s2t], axis=1)[s2t >= 0]
        both = np.concatenate([a, b]).astype(np.int64).reshape(-1, 2)
        return np.unique(both, axis=0) if both.size else both

    def default_anchors(self, registered) -> np.ndarray:
        """Target vertices closest to the registered positions of the source vertices that no shape moves; sorted, unique."""
        sv = self.source[0]
        if self.shapes is None:
            raise NoAnchorError("no source shapes to find static vertices from")
        static = np.nonzero((self.shapes == sv[None]).all(axis=(0, 2)))[0]
        if static.size == 0:
            raise NoAnchorError("every source vertex moves in some blendshape and no anchor list was given: pass anchors=[target vertex indices]")
        idx, _ = self.engine.closest(np.asarray(registered)[static], None, self.target[0], None)
        return np.unique(idx.astype(np.int64))

    def transfer(self, pairs: np.ndarray, anchors: Sequence[int]):
        """(residuals (K, V_t, 3), SolveReport)."""
        tv, tf = self.target
        if self.shapes is None or self.shapes.shape[0] == 0:
            raise TransferError("the source has no shapes to transfer")
        anchors = np.unique(np.asarray(anchors, dtype=np.int64).reshape(-1))
        if anchors.size == 0:
            raise NoAnchorError("an empty anchor list leaves the translation free")
        structure = transfer_structure(tf, tv.shape[0], pairs, anchors)
        out, st, it, res = self.engine.transfer(structure, self.tol, self.max_iter)
        report = SolveReport(st, it, res)
        _check(report, "transfer", self.strict)
        return out, report


def _session(source_neutral, source_faces, source_shapes, target_neutral, target_faces, device, tol, max_iter) -> DeformationTransfer:
    dt = DeformationTransfer(device, tol, max_iter)
    dt.set_source(source_neutral, source_faces, source_shapes)
    dt.set_target(target_neutral, target_faces)
    return dt


def register(source_neutral, source_faces, target_neutral, target_faces, source_markers, target_markers, w_s: float = 1.0, w_i: float = 0.001,
             schedule=WC_SCHEDULE, tol: float = 1e-10, max_iter: int = 20000, device="cuda") -> Registration:
    dt = _session(source_neutral, source_faces, None, target_neutral, target_faces, device, tol, max_iter)
    try:
        return dt.register(source_markers, target_markers, w_s, w_i, schedule)
    finally:
        dt.close()


def triangle_correspondence(registered, source_faces, target_neutral, target_faces, corr_threshold: float = 0.05, device="cuda") -> np.ndarray:
    dt = _session(registered, source_faces, None, target_neutral, target_faces, device, 1e-10, 1)
    try:
        return dt.triangle_correspondence(registered, corr_threshold)
    finally:
        dt.close()


def transfer(source_neutral, source_faces, source_shapes, target_neutral, target_faces, pairs, anchors, tol: float = 1e-10, max_iter: int = 20000,
             device="cuda") -> np.ndarray:
    dt = _session(source_neutral, source_faces, source_shapes, target_neutral, target_faces, device, tol, max_iter)
    try:
        return dt.transfer(pairs, anchors)[0]
    finally:
        dt.close()


def transfer_blendshapes(source_neutral, source_faces, source_shapes, target_neutral, target_faces, source_markers, target_markers, w_s: float = 1.0,
                         w_i: float = 0.001, schedule=WC_SCHEDULE, corr_threshold: float = 0.05, anchors: Optional[Sequence[int]] = None, tol: float = 1e-10,
                         max_iter: int = 20000, device="cuda", details: Optional[dict] = None) -> np.ndarray:
    """Residuals (K, V_t, 3) float64 of the K source shapes on the target.  ``details``, when a dict, receives the registration, the pairs, the
    anchors and the transfer's solver report."""
    dt = _session(source_neutral, source_faces, source_shapes, target_neutral, target_faces, device, tol, max_iter)
    try:
        reg = dt.register(source_markers, target_markers, w_s, w_i, schedule)
        pairs = dt.triangle_correspondence(None, corr_threshold)
        anc = dt.default_anchors(reg.vertices) if anchors is None else np.asarray(anchors, dtype=np.int64)
        out, report = dt.transfer(pairs, anc)
        if details is not None:
            details.update(registration=reg, pairs=pairs, anchors=anc, report=report)
        return out
    finally:
        dt.close()
