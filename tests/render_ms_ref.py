"""A float64 restatement of DESIGN.md section 15.2 (rendering with 4 samples per pixel), built on tests/render_ref.py.

Coverage and depth of the sample at offset (ox, oy) from the pixel centre are render_ref.render_frame with the principal point moved to
(cx - ox, cy - oy): that call gives the sample's face, its depth and its *ambiguous* flag.  Shading is per face at the pixel centre, restated
from render_frame's last block: vertices in positive-winding order, barycentrics from E_i / d_i at the centre (they extrapolate where the
centre lies outside the triangle), then render_ref.brdf_color.  Each sample's colour is quantised by render_ref.to_bgr8 and the four are
resolved as (c0 + c1 + c2 + c3 + 2) >> 2.  A pixel is ambiguous when any of its samples is, or when a shade it uses has max |b_i| > MAX_BARY.
"""
import numpy as np
from scipy.spatial.transform import Rotation

import render_ref as rr

OFFSETS = ((-0.125, -0.375), (0.375, -0.125), (-0.375, 0.125), (0.125, 0.375))   # x right, y down, from the pixel centre
MAX_BARY = 16.0


def resolve(samples):
    """(..., 4, C) uint8 sample values -> (..., C) uint8: (c0 + c1 + c2 + c3 + 2) >> 2."""
    return ((np.asarray(samples).astype(np.int64).sum(axis=-2) + 2) >> 2).astype(np.uint8)


def sample_geometry(verts, faces, sc, rot=None, t_center=None):
    """The part that does not depend on the colours: dict(face (H, W, 4) int64, depth (H, W, 4), ambiguous (H, W, 4) bool)."""
    normals = rr.vertex_normals(verts, faces)
    outs = [rr.render_frame(verts, faces, dict(sc, cx=sc["cx"] - ox, cy=sc["cy"] - oy), normals=normals, rot=rot, t_center=t_center)
            for ox, oy in OFFSETS]
    return {k: np.stack([o[k] for o in outs], axis=-1) for k in ("face", "depth", "ambiguous")}


def shade_at_centres(verts, faces, sc, face, colors=None, rot=None, t_center=None):
    """face (H, W) int, -1 for none -> (colour (H, W, 3) unrounded R, G, B, zeros where face < 0; max |b_i| (H, W), 0 where face < 0)."""
    f = np.asarray(faces)
    v = np.asarray(verts, dtype=np.float64)
    R = np.eye(3) if rot is None else Rotation.from_rotvec(np.asarray(rot, dtype=np.float64)).as_matrix()
    c = np.zeros(3) if t_center is None else np.asarray(t_center, dtype=np.float64)
    p = (v - c) @ R.T + c
    nr = rr.vertex_normals(v, f) @ R.T
    q = p - sc["cam"]
    d = -q[:, 2]
    s = np.stack([sc["fx"] * q[:, 0] / d + sc["cx"], sc["cy"] - sc["fy"] * q[:, 1] / d], axis=1)
    color = np.zeros(face.shape + (3,))
    max_b = np.zeros(face.shape)
    rows, cols = np.nonzero(face >= 0)
    if len(rows) == 0:
        return color, max_b
    tri = f[face[rows, cols]].copy()                             # (n, 3)
    S = s[tri]
    area2 = (S[:, 1, 0] - S[:, 0, 0]) * (S[:, 2, 1] - S[:, 0, 1]) - (S[:, 1, 1] - S[:, 0, 1]) * (S[:, 2, 0] - S[:, 0, 0])
    tri[area2 < 0] = tri[area2 < 0][:, [0, 2, 1]]                # positive winding
    S = s[tri]
    px, py = cols + 0.5, rows + 0.5
    E = []
    for i in range(3):
        a, b = S[:, (i + 1) % 3], S[:, (i + 2) % 3]
        E.append((a[:, 1] - b[:, 1]) * (px - a[:, 0]) + (b[:, 0] - a[:, 0]) * (py - a[:, 1]))
    wgt = np.stack(E, axis=1) / d[tri]
    bar = wgt / wgt.sum(axis=1, keepdims=True)
    P = (bar[:, :, None] * p[tri]).sum(axis=1)
    N = rr._unit((bar[:, :, None] * nr[tri]).sum(axis=1))
    if colors is None:
        color[rows, cols] = rr.brdf_color(P, N, np.broadcast_to(sc["base"], P.shape), sc, sc["metallic"], sc["roughness"])
    else:
        base = (bar[:, :, None] * np.asarray(colors, dtype=np.float64)[tri]).sum(axis=1)
        color[rows, cols] = rr.brdf_color(P, N, base, sc, sc["vc_metallic"], sc["vc_roughness"])
    max_b[rows, cols] = np.abs(bar).max(axis=1)
    return color, max_b


def render_frame_ms(verts, faces, sc, colors=None, rot=None, t_center=None, geometry=None):
    """dict(face (H, W, 4), sample_ambiguous (H, W, 4), bgr (H, W, 3) uint8 resolved, sample_bgr (H, W, 4, 3) uint8, ambiguous (H, W),
    max_b: the largest |b_i| of any shade used).  `geometry`: a cached sample_geometry of the same verts, faces, sc, rot, t_center."""
    g = sample_geometry(verts, faces, sc, rot, t_center) if geometry is None else geometry
    face = g["face"]
    sample_bgr = np.zeros(face.shape + (3,), dtype=np.uint8)
    far = np.zeros(face.shape[:2], dtype=bool)
    max_b = 0.0
    for i in range(4):   # a face that wins several samples of a pixel is shaded again with the same float64 result
        color, mb = shade_at_centres(verts, faces, sc, face[..., i], colors, rot, t_center)
        covered = face[..., i] >= 0
        sample_bgr[..., i, :] = np.where(covered[..., None], rr.to_bgr8(color), 0)
        far |= mb > MAX_BARY
        max_b = max(max_b, float(mb.max()))
    return dict(face=face, sample_ambiguous=g["ambiguous"], bgr=resolve(sample_bgr), sample_bgr=sample_bgr,
                ambiguous=g["ambiguous"].any(axis=-1) | far, max_b=max_b)


# ---- the full-size scenes of tests/test_gpu_render_ms.py and of the ambiguity cap (tests/test_render_ms_cpu.py): (frame, rotation)
SCENES = ((0, None), (5, rr.YAW))
