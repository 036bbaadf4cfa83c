"""Frames per second of the renderer (said_amd.render) on the ARKit reference mesh and on the same mesh with every triangle split in four
(about 4.9k vertices, 9.2k faces: the size of a BlendVOCA head).

Two figures per mesh, each the median of `--repeats` renders of `--frames` frames after one warm-up render:
  device   frames rendered into device memory in chunks of `--chunk`, timed between two synchronisations
  host     the same through iter_rendered_frames: every chunk copied to pinned host memory and handed to the caller
Prints one JSON line.  The coefficient sequence is a seeded smooth random walk in [0, 1]; vertices and bases come from golden G13, faces from
golden G15.

Usage:  python scripts/bench_render.py [--frames 600] [--repeats 5] [--chunk 64] [--difference] [--samples {1,4}]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from said_amd.render import RendererObject, iter_rendered_frames  # noqa: E402
from said_amd.util.mesh import Mesh  # noqa: E402


def arkit():
    g13 = np.load(os.path.join(ROOT, "tests", "golden", "g13_blendshape_qp.npz"))
    faces = np.load(os.path.join(ROOT, "tests", "golden", "g15_render.npz"))["faces"].astype(np.int64)
    names51 = list(g13["names51"])
    shapes = np.stack([g13["shapes51"][names51.index(s)] for s in g13["names32"]])   # (32, V, 3)
    return g13["neutral"], shapes, faces


def split_in_four(neutral, shapes, faces):
    """Every triangle into four through its edge midpoints; the midpoints of the bases are the bases of the midpoints (the blend is linear)."""
    edges = {}
    pairs = []

    def mid(a, b):
        key = (min(a, b), max(a, b))
        if key not in edges:
            edges[key] = len(neutral) + len(pairs)
            pairs.append(key)
        return edges[key]

    out = []
    for a, b, c in faces.tolist():
        ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
        out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    p = np.array(pairs)
    grow = lambda v: np.concatenate([v, 0.5 * (v[..., p[:, 0], :] + v[..., p[:, 1], :])], axis=-2)
    return grow(neutral), grow(shapes), np.array(out, dtype=np.int64)


def sequence(frames, seed=0):
    rng = np.random.default_rng(seed)
    w = np.cumsum(rng.normal(scale=0.03, size=(frames, 32)), axis=0) + rng.uniform(0.2, 0.8, size=32)
    return np.abs(((w + 1) % 2) - 1).astype(np.float32)   # reflected into [0, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--difference", action="store_true", help="render the difference heat map against a second sequence")
    ap.add_argument("--samples", type=int, choices=[1, 4], default=1, help="samples per pixel (DESIGN.md section 15.2)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render.py needs the MI355X"
    w = sequence(args.frames)
    wt = sequence(args.frames, seed=1) if args.difference else None
    result = {"frames": args.frames, "chunk": args.chunk, "difference": bool(args.difference), "samples": args.samples, "meshes": {}}
    base = arkit()
    for name, (neutral, shapes, faces) in (("arkit", base), ("arkit_split4", split_in_four(*base))):
        mesh, basis = Mesh(neutral, faces), shapes.reshape(32, -1).T.copy()
        r = RendererObject(device=args.device, samples=args.samples)
        eng = r.engine
        r.set_mesh(neutral, faces, basis)
        if wt is not None:
            r.set_colormap("viridis")
        cw = torch.from_numpy(w).to(args.device)
        ct = torch.from_numpy(wt).to(args.device) if wt is not None else None
        out = torch.empty((min(args.chunk, args.frames), 800, 800, 3), dtype=torch.uint8, device=args.device)
        center = neutral.mean(axis=0)

        def device_pass():
            for t0 in range(0, args.frames, args.chunk):
                eng.render(cw, t0, min(args.chunk, args.frames - t0), out, target=ct, t_center=center, samples=args.samples)

        def host_pass():
            n = 0
            for frames in iter_rendered_frames(r, mesh, basis, w, wt, chunk=args.chunk):
                n += len(frames)
            assert n == args.frames

        res = {"vertices": int(len(neutral)), "faces": int(len(faces))}
        for label, fn in (("device", device_pass), ("host", host_pass)):
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t)
            med = statistics.median(ts)
            res[label] = {"median_s": med, "min_s": min(ts), "max_s": max(ts), "frames_per_s": args.frames / med, "x_real_time_60fps": args.frames / med / 60.0}
        result["meshes"][name] = res
        r.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
