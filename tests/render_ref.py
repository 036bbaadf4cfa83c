"""A float64 numpy restatement of DESIGN.md section 15 (the renderer), written from the section and not from the kernels.

    blend            v_t = n + B_delta w_t, the difference magnitude |B_delta (w'_t - w_t)| and its colour bin
    vertex_normals   unit face normals weighted by the face's corner angle at the vertex, summed, normalised
    render_frame     rotation about t_center, pinhole projection, coverage at pixel centres under the top-left rule, nearest fragment with
                     ties to the lower face index, perspective-correct attributes, the metallic-roughness BRDF under the point lights

``render_frame`` returns per pixel the winning face (-1: background), its depth, the unrounded R, G, B colour and an *ambiguous* flag.  The
flag marks the pixels at which fp32 cannot be asked to agree with float64: a sample whose distance to an edge of a triangle that decides the
pixel is below EDGE_EPS = 1e-4 px — the winner's smallest edge function, or a triangle that misses the sample by less than that and would
have won or tied — or whose runner-up lies within DEPTH_EPS = 1e-6 of the winner's depth.
"""
import numpy as np
from scipy.spatial.transform import Rotation

EDGE_EPS = 1e-4    # px
DEPTH_EPS = 1e-6   # scene units
LUT_N = 256


def scene(z_offset=0.0):
    """The reference's scene (script/rendering/render_visual.py): the camera pose is the literal (0, 0, 1), z_offset moves the lights only."""
    pos = np.array([0.0, 0.0, 1.0 - z_offset])
    a = np.pi / 6.0
    rot = lambda v: Rotation.from_rotvec(v).as_matrix() @ pos
    return dict(width=800, height=800, fx=4754.97941935 / 2, fy=4754.97941935 / 2, cx=400.0, cy=400.0, znear=0.01, zfar=3.0,
                cam=np.array([0.0, 0.0, 1.0]), lights=np.stack([pos, rot([a, 0, 0]), rot([-a, 0, 0]), rot([0, -a, 0])]), intensity=2.0,
                ambient=0.2, base=np.full(3, 0.3), metallic=0.8, roughness=0.8, vc_metallic=1.0, vc_roughness=1.0)


def blend(neutral, basis, w, w_target=None, max_diff=0.001):
    """neutral (V, 3), basis (3V, K) = [b_1 | ... | b_K], w (T, K) -> vertices (T, V, 3); with w_target also (|difference| (T, V), x (T, V))
    where x = clip(|difference|, 0, max_diff) / max_diff."""
    n = np.asarray(neutral, dtype=np.float64).reshape(-1, 1)
    bd = np.asarray(basis, dtype=np.float64) - n
    w = np.asarray(w, dtype=np.float64)
    v = (w @ bd.T + n.T).reshape(len(w), -1, 3)
    if w_target is None:
        return v
    g = ((np.asarray(w_target, dtype=np.float64) - w) @ bd.T).reshape(len(w), -1, 3)
    mag = np.sqrt((g * g).sum(axis=2))
    return v, mag, np.clip(mag, 0.0, max_diff) / max_diff


def colormap_bin(x):
    """int(x 256), x == 1 in bin 255."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x >= 1.0, LUT_N - 1, np.floor(x * LUT_N).astype(np.int64))


def vertex_normals(verts, faces):
    v, f = np.asarray(verts, dtype=np.float64), np.asarray(faces)
    p = v[f]                                                   # (F, 3, 3)
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.linalg.norm(fn, axis=1)
    ok = ln > 0
    fn = np.where(ok[:, None], fn / np.where(ok, ln, 1.0)[:, None], 0.0)
    out = np.zeros_like(v)
    for c in range(3):
        a, b = p[:, (c + 1) % 3] - p[:, c], p[:, (c + 2) % 3] - p[:, c]
        ang = np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(axis=1))
        np.add.at(out, f[:, c], np.where(ok, ang, 0.0)[:, None] * fn)
    l = np.linalg.norm(out, axis=1)
    return np.where((l > 0)[:, None], out / np.where(l > 0, l, 1.0)[:, None], 0.0)


def _unit(a):
    return a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-20)


def brdf_color(P, N, base, sc, metallic, roughness):
    """Section 15's shading of points P (n, 3) with unit normals N and base colours base (n, 3) -> unrounded R, G, B (n, 3)."""
    alpha = roughness * roughness
    a2, k = alpha * alpha, alpha / 2
    F0 = 0.04 * (1 - metallic) + base * metallic
    cdiff = base * (1 - 0.04) * (1 - metallic)
    V = _unit(sc["cam"] - P)
    NdV = np.clip((N * V).sum(-1), 0, 1)
    col = sc["ambient"] * base
    for lp in sc["lights"]:
        Lv = lp - P
        d2 = (Lv * Lv).sum(-1)
        L = _unit(Lv)
        H = _unit(L + V)
        NdL, NdH, VdH = (np.clip((x * y).sum(-1), 0, 1) for x, y in ((N, L), (N, H), (V, H)))
        D = a2 / (np.pi * (NdH * NdH * (a2 - 1) + 1) ** 2)
        vis = 1 / (4 * (NdL * (1 - k) + k) * (NdV * (1 - k) + k))
        F = F0 + (1 - F0) * ((1 - VdH) ** 5)[:, None]
        col = col + (sc["intensity"] / np.maximum(d2, 1e-20) * NdL)[:, None] * ((1 - F) * cdiff / np.pi + F * (D * vis)[:, None])
    return col


def render_frame(verts, faces, sc, normals=None, colors=None, rot=None, t_center=None):
    """verts (V, 3) before the rotation, colors (V, 3) R, G, B or None (plain material).  Returns dict(face, depth, color, ambiguous, mind)."""
    W, H = sc["width"], sc["height"]
    f = np.asarray(faces)
    v = np.asarray(verts, dtype=np.float64)
    nrm = vertex_normals(v, f) if normals is None else np.asarray(normals, dtype=np.float64)
    R = np.eye(3) if rot is None else Rotation.from_rotvec(np.asarray(rot, dtype=np.float64)).as_matrix()
    c = np.zeros(3) if t_center is None else np.asarray(t_center, dtype=np.float64)
    p = (v - c) @ R.T + c
    nr = nrm @ R.T
    q = p - sc["cam"]
    d = -q[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.stack([sc["fx"] * q[:, 0] / d + sc["cx"], sc["cy"] - sc["fy"] * q[:, 1] / d], axis=1)
    best_d = np.full((H, W), np.inf)
    second = np.full((H, W), np.inf)
    near_miss = np.full((H, W), np.inf)
    face = np.full((H, W), -1, dtype=np.int64)
    mind = np.full((H, W), np.inf)
    order = np.empty((len(f), 3), dtype=np.int64)   # vertex order with positive winding
    for t, tri in enumerate(f):
        order[t] = tri
        if np.any(d[tri] < sc["znear"]) or not np.all(np.isfinite(s[tri])):
            continue
        (x0, y0), (x1, y1), (x2, y2) = s[tri]
        area2 = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        if area2 == 0:
            continue
        if area2 < 0:
            tri = tri[[0, 2, 1]]
            order[t] = tri
            (x0, y0), (x1, y1), (x2, y2) = s[tri]
        xs, ys = s[tri, 0], s[tri, 1]
        c0, c1 = max(int(np.floor(xs.min() - 0.5)) - 1, 0), min(int(np.floor(xs.max() - 0.5)) + 2, W - 1)
        r0, r1 = max(int(np.floor(ys.min() - 0.5)) - 1, 0), min(int(np.floor(ys.max() - 0.5)) + 2, H - 1)
        if c0 > c1 or r0 > r1:
            continue
        px, py = np.meshgrid(np.arange(c0, c1 + 1) + 0.5, np.arange(r0, r1 + 1) + 0.5)
        E, dist, inside = [], [], np.ones(px.shape, dtype=bool)
        for (ax, ay), (bx, by) in (((x1, y1), (x2, y2)), ((x2, y2), (x0, y0)), ((x0, y0), (x1, y1))):
            A, B = ay - by, bx - ax
            e = A * (px - ax) + B * (py - ay)
            top_left = A > 0 or (A == 0 and B > 0)
            inside &= (e > 0) | ((e == 0) & top_left)
            E.append(e)
            dist.append(e / np.hypot(A, B))
        md = np.minimum(np.minimum(dist[0], dist[1]), dist[2])
        iv = 1.0 / d[tri]
        with np.errstate(divide="ignore", invalid="ignore"):
            dep = (E[0] + E[1] + E[2]) / (E[0] * iv[0] + E[1] * iv[1] + E[2] * iv[2])
        in_range = (dep >= sc["znear"]) & (dep <= sc["zfar"])
        valid = inside & in_range
        win = (slice(r0, r1 + 1), slice(c0, c1 + 1))
        miss = ~inside & (md > -EDGE_EPS) & in_range
        near_miss[win] = np.where(miss, np.minimum(near_miss[win], dep), near_miss[win])
        bd_, sd_ = best_d[win], second[win]
        takes = valid & (dep < bd_)            # strict: a tie stays with the lower face index
        second[win] = np.where(takes, bd_, np.where(valid, np.minimum(sd_, dep), sd_))
        best_d[win] = np.where(takes, dep, bd_)
        face[win] = np.where(takes, t, face[win])
        mind[win] = np.where(takes, md, mind[win])
    covered = face >= 0
    with np.errstate(invalid="ignore"):
        ambiguous = (covered & (mind < EDGE_EPS)) | (covered & (second - best_d <= DEPTH_EPS)) | (np.isfinite(near_miss) & (near_miss <= best_d + DEPTH_EPS))
    color = np.zeros((H, W, 3))
    rows, cols = np.nonzero(covered)
    if len(rows):
        tri = order[face[rows, cols]]                         # (n, 3)
        px, py = cols + 0.5, rows + 0.5
        S = s[tri]                                            # (n, 3, 2)
        E = []
        for i in range(3):
            a, b = S[:, (i + 1) % 3], S[:, (i + 2) % 3]
            E.append((a[:, 1] - b[:, 1]) * (px - a[:, 0]) + (b[:, 0] - a[:, 0]) * (py - a[:, 1]))
        wgt = np.stack(E, axis=1) / d[tri]
        bar = wgt / wgt.sum(axis=1, keepdims=True)
        P = (bar[:, :, None] * p[tri]).sum(axis=1)
        N = _unit((bar[:, :, None] * nr[tri]).sum(axis=1))
        if colors is None:
            color[rows, cols] = brdf_color(P, N, np.broadcast_to(sc["base"], P.shape), sc, sc["metallic"], sc["roughness"])
        else:
            base = (bar[:, :, None] * np.asarray(colors, dtype=np.float64)[tri]).sum(axis=1)
            color[rows, cols] = brdf_color(P, N, base, sc, sc["vc_metallic"], sc["vc_roughness"])
    return dict(face=face, depth=best_d, color=color, ambiguous=ambiguous, mind=mind)


def to_bgr8(color):
    """clamp to [0, 1], round to nearest, B-G-R."""
    return np.floor(np.clip(color, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)[..., ::-1]


# ---- the scenes of the GPU test (tests/test_gpu_render.py) and of the ambiguity cap (tests/test_render_cpu.py)
N_FRAMES = 8
YAW = (0.0, 0.3, 0.0)
CASES = [("plain", None, False), ("plain_yaw", YAW, False), ("difference", None, True), ("difference_yaw", YAW, True)]


def arkit_mesh(golden_dir):
    """(neutral (V, 3), basis (3V, 32), faces (F, 3)) of the ARKit reference mesh: goldens G13 and G15."""
    import os
    g13, g15 = np.load(os.path.join(golden_dir, "g13_blendshape_qp.npz")), np.load(os.path.join(golden_dir, "g15_render.npz"))
    names51 = list(g13["names51"])
    basis = np.concatenate([g13["shapes51"][names51.index(s)].reshape(-1, 1) for s in g13["names32"]], axis=1)
    return g13["neutral"], basis, g15["faces"]


def scene_coeffs():
    """The fixed synthetic sequence: (w (8, 32) in [0, 1], w_target (8, 32) in [0, 1]), fp32-representable."""
    rng = np.random.default_rng(1515)
    w = rng.uniform(0.0, 1.0, size=(N_FRAMES, 32))
    wt = np.clip(w + 0.1 * (rng.uniform(0.0, 1.0, size=w.shape) - 0.5), 0.0, 1.0)
    return w.astype(np.float32).astype(np.float64), wt.astype(np.float32).astype(np.float64)
