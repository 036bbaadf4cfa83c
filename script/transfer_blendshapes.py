"""Generate the blendshapes of new heads from reference blendshapes by deformation transfer on an MI355X, and write the residuals pickle.

The first stage of the pipeline ("generate blendshapes by yourself"), which the reference leaves to a third-party tool: the source
blendshapes (<source_dir>/Neutral.obj and <source_dir>/<name>.obj for every name of the list) are carried onto every template of
--templates_dir (<person>.ply or <person>.obj, optionally cropped to --head_idx_path) with the two marker files as correspondences, and
blendshape_residuals.pickle is written in the reference's layout {person: {name: (V, 3) float64}}: what script/preprocess_blendvoca.py,
script/train.py, script/evaluate_extra.py --vertex_error and script/render.py read.  With --blendshapes_out_dir the meshes are written too
(templates_head/<person>.obj, blendshapes_head/<person>/<name>.obj).  said_amd/optimize/deformation_transfer.py and DESIGN.md section 17
describe the method; there is no CPU path."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, save_blendshape_deltas  # noqa: E402
from said_amd.util.mesh import Mesh, load_mesh, load_vertices, save_mesh  # noqa: E402
from said_amd.util.parser import parse_list  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Transfer reference blendshapes onto template heads and write blendshape_residuals.pickle")
    p.add_argument("--source_dir", type=str, default="../ARKit_reference_blendshapes", help="Directory of the source OBJ blendshapes, with Neutral.obj")
    p.add_argument("--blendshape_list_path", type=str, default=None, help="List of the blendshapes (default: the 32 built-in ARKit names)")
    p.add_argument("--templates_dir", type=str, default="../BlendVOCA/templates", help="Directory of the target template meshes (PLY or OBJ)")
    p.add_argument("--head_idx_path", type=str, default="", help="List of template vertex indices to crop to (FLAME_head_idx.txt); empty: whole templates")
    p.add_argument("--source_markers_path", type=str, required=True, help="Marker vertex indices of the source (ARKit_landmarks.txt), one per line")
    p.add_argument("--target_markers_path", type=str, required=True, help="Marker vertex indices of the (cropped) targets (FLAME_head_landmarks.txt)")
    p.add_argument("--blendshape_residuals_path", type=str, default="../blendshape_residuals.pickle", help="Output path of the blendshape residuals")
    p.add_argument("--blendshapes_out_dir", type=str, default=None, help="Also write the neutral and blendshape meshes here")
    p.add_argument("--person_ids", type=str, default=None, help="Comma-separated template names (default: every mesh of --templates_dir)")
    p.add_argument("--w_smooth", type=float, default=1.0, help="Weight of the smoothness term of the registration")
    p.add_argument("--w_identity", type=float, default=0.001, help="Weight of the identity term of the registration")
    p.add_argument("--corr_threshold", type=float, default=0.05, help="Largest centroid distance of a triangle pair, in target bounding-box diagonals")
    p.add_argument("--anchors_path", type=str, default=None, help="Target vertex indices that stay in place (default: found from the static source vertices)")
    p.add_argument("--tol", type=float, default=1e-10, help="Relative residual at which a solve stops")
    p.add_argument("--max_iter", type=int, default=20000, help="Most iterations of a solve")
    p.add_argument("--device", type=str, default="cuda:0", help="MI355X to run on")
    return p


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from said_amd.optimize.deformation_transfer import DeformationTransfer
    from said_amd.util.mesh import get_submesh
    names = parse_list(args.blendshape_list_path, str) if args.blendshape_list_path else list(DEFAULT_BLENDSHAPE_CLASSES)
    source = load_mesh(os.path.join(args.source_dir, "Neutral.obj"))
    shapes = np.stack([load_vertices(os.path.join(args.source_dir, f"{n}.obj")) for n in names])
    if shapes.shape[1:] != source.vertices.shape:
        raise SystemExit(f"the source blendshapes have {shapes.shape[1]} vertices, Neutral.obj {source.vertices.shape[0]}")
    src_markers, tgt_markers = parse_list(args.source_markers_path, int), parse_list(args.target_markers_path, int)
    head_idx = parse_list(args.head_idx_path, int) if args.head_idx_path else None
    anchors = parse_list(args.anchors_path, int) if args.anchors_path else None
    if args.person_ids:
        pids = [p for p in args.person_ids.split(",") if p]
    else:
        pids = sorted({os.path.splitext(f)[0] for f in os.listdir(args.templates_dir) if os.path.splitext(f)[1].lower() in (".ply", ".obj")})
    if not pids:
        raise SystemExit(f"no template mesh in {args.templates_dir}")
    if os.path.exists(args.blendshape_residuals_path):
        raise SystemExit(f"{args.blendshape_residuals_path} exists: choose a new --blendshape_residuals_path")
    if args.blendshapes_out_dir:
        for sub in ("templates_head", "blendshapes_head"):
            if os.path.exists(os.path.join(args.blendshapes_out_dir, sub)):
                raise SystemExit(f"{os.path.join(args.blendshapes_out_dir, sub)} exists: choose a new --blendshapes_out_dir")
    dt = DeformationTransfer(args.device, args.tol, args.max_iter)
    dt.set_source(source.vertices, source.faces, shapes)
    residuals, heads = {}, {}
    for pid in pids:
        path = next((os.path.join(args.templates_dir, pid + e) for e in (".ply", ".obj") if os.path.isfile(os.path.join(args.templates_dir, pid + e))), None)
        if path is None:
            raise SystemExit(f"no template of {pid} in {args.templates_dir}")
        head = load_mesh(path)
        if head_idx is not None:
            head = get_submesh(head.vertices, head.faces, head_idx)
        t0 = time.perf_counter()
        dt.set_target(head.vertices, head.faces)
        reg = dt.register(src_markers, tgt_markers, args.w_smooth, args.w_identity)
        t1 = time.perf_counter()
        pairs = dt.triangle_correspondence(None, args.corr_threshold)
        anc = dt.default_anchors(reg.vertices) if anchors is None else np.asarray(anchors)
        t2 = time.perf_counter()
        out, report = dt.transfer(pairs, anc)
        t3 = time.perf_counter()
        print(f"{pid}: {head.vertices.shape[0]} vertices, {pairs.shape[0]} triangle pairs, {len(anc)} anchors; registration {t1 - t0:.2f} s "
              f"({int(reg.report.iters.max(axis=1).sum())} iterations), correspondence {t2 - t1:.2f} s, transfer {t3 - t2:.2f} s "
              f"({int(report.iters.max())} iterations)", flush=True)
        residuals[pid] = {name: out[i] for i, name in enumerate(names)}
        heads[pid] = head
    dt.close()
    save_blendshape_deltas(residuals, args.blendshape_residuals_path)
    if args.blendshapes_out_dir:
        for pid, head in heads.items():
            os.makedirs(os.path.join(args.blendshapes_out_dir, "templates_head"), exist_ok=True)
            os.makedirs(os.path.join(args.blendshapes_out_dir, "blendshapes_head", pid))
            save_mesh(head, os.path.join(args.blendshapes_out_dir, "templates_head", f"{pid}.obj"))
            for name, d in residuals[pid].items():
                save_mesh(Mesh(head.vertices + d, head.faces), os.path.join(args.blendshapes_out_dir, "blendshapes_head", pid, f"{name}.obj"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
