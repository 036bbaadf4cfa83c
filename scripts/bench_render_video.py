"""Frames per second of a rendered Motion-JPEG video, end to end, with the frames encoded by PIL on the host (--jpeg pil of script/render.py) and
by the HIP encoder on the device (--jpeg gpu), in one process on one box.

Each pass renders `--frames` frames of the ARKit reference mesh (a seeded smooth random walk, as scripts/bench_render.py) and writes the .avi
into a temporary directory through script/_common.py's write_video, the way script/render.py does.  Per path: warm-up passes, then the median of
`--repeats` timed windows, each of as many back-to-back passes as make it last half a second (one pass for the PIL path).  Also timed, between two synchronisations: the render alone, and the render plus the device encode without the file.
Prints one JSON line.  `--encode-only N` instead runs N encodes of one rendered chunk and nothing else: the workload for a kernel trace.

Usage:  python scripts/bench_render_video.py [--frames 600] [--repeats 5] [--chunk 64] [--quality 90]
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "script"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _common import write_video  # noqa: E402
from bench_render import arkit, sequence  # noqa: E402
from said_amd.render import JpegEncoder, RendererObject, iter_encoded_frames, iter_rendered_frames  # noqa: E402
from said_amd.util.mesh import Mesh  # noqa: E402


MIN_WINDOW_S = 0.5   # a timed window shorter than this measures the clock and the scheduler as much as the work


def timed(fn, repeats):
    """Seconds per pass of fn, `repeats` times: each figure is a window of `inner` back-to-back passes between two synchronisations, divided by
    `inner`, which is chosen from a second warm-up pass so that a window lasts at least MIN_WINDOW_S.  Returns (times, inner)."""
    fn()   # warm-up
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    inner = max(1, math.ceil(MIN_WINDOW_S / max(time.perf_counter() - t, 1e-6)))
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) / inner)
    return ts, inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--encode-only", type=int, default=0, metavar="N", help="N encodes of one rendered chunk, for a kernel trace")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render_video.py needs the MI355X"
    neutral, shapes, faces = arkit()
    mesh, basis = Mesh(neutral, faces), shapes.reshape(32, -1).T.copy()
    w = sequence(args.frames)
    r = RendererObject(device=args.device)
    r.set_mesh(neutral, faces, basis)
    eng = r.engine
    cw = torch.from_numpy(w).to(args.device)
    n_chunk = min(args.chunk, args.frames)
    dev = torch.empty((n_chunk, 800, 800, 3), dtype=torch.uint8, device=args.device)
    enc = JpegEncoder(args.device, 800, 800, args.quality)
    center = neutral.mean(axis=0)

    if args.encode_only:
        eng.render(cw, 0, n_chunk, dev, t_center=center)
        for _ in range(args.encode_only):
            files = enc.encode(dev)
        print(json.dumps({"encode_only": args.encode_only, "chunk": n_chunk, "bytes_per_frame": sum(map(len, files)) / len(files)}))
        return

    sizes = {}

    def render_pass():
        for t0 in range(0, args.frames, args.chunk):
            eng.render(cw, t0, min(args.chunk, args.frames - t0), dev, t_center=center)

    def render_encode_pass():
        total = 0
        for t0 in range(0, args.frames, args.chunk):
            n = min(args.chunk, args.frames - t0)
            eng.render(cw, t0, n, dev, t_center=center)
            total += sum(map(len, enc.encode(dev[:n])))
        sizes["gpu"] = total / args.frames

    with tempfile.TemporaryDirectory() as tmp:
        def video_pass(kind):
            path = os.path.join(tmp, kind + ".avi")
            if kind == "gpu":
                frames = iter_encoded_frames(r, mesh, basis, w, chunk=args.chunk, quality=args.quality)
            else:
                frames = iter_rendered_frames(r, mesh, basis, w, chunk=args.chunk)
            write_video(frames, path, 60, None, encoded=kind == "gpu")
            sizes[kind + "_file"] = os.path.getsize(path) / args.frames

        result = {"frames": args.frames, "chunk": args.chunk, "quality": args.quality, "repeats": args.repeats}
        for label, fn in (("render_only", render_pass), ("render_and_device_encode", render_encode_pass), ("video_pil", lambda: video_pass("pil")),
                          ("video_gpu", lambda: video_pass("gpu"))):
            ts, inner = timed(fn, args.repeats)
            med = statistics.median(ts)
            result[label] = {"median_s": med, "min_s": min(ts), "max_s": max(ts), "passes_per_window": inner, "frames_per_s": args.frames / med}
    result["bytes_per_frame"] = {"device_jpeg": sizes["gpu"], "avi_pil": sizes["pil_file"], "avi_gpu": sizes["gpu_file"], "raw": 800 * 800 * 3}
    print(json.dumps(result))
    enc.close()
    r.close()


if __name__ == "__main__":
    main()
