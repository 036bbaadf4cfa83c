"""Preprocess the VOCA templates: write every person's head neutral and ARKit blendshape meshes from the templates and a residuals pickle.

Command-line compatible with the reference's script/preprocess_blendvoca.py:16-37 (--templates_dir, --blendshape_residuals_path,
--blendshapes_out_dir, same defaults but for the pickle's, which the reference takes from its data directory), and the same outputs:
<out>/templates_head/<person>.obj and <out>/blendshapes_head/<person>/<name>.obj.  As in the reference's
BlendVOCADataset.preprocess_blendshapes (script/dataset/dataset_voca.py:288-361), a template <templates_dir>/<person>.ply is cropped to the
vertices of --head_idx_path (get_submesh) and a blendshape is the cropped neutral plus the person's residual.  This is host work; it is here
because it consumes the pickle script/transfer_blendshapes.py writes.  Differences:
- --head_idx_path has no default (data/FLAME_head_idx.txt is not part of this repository): give the file, or "" for templates that are
  heads already; a template may also be <person>.obj;
- --person_ids (comma-separated) and --blendshape_list_path are optional: by default every person of the pickle and the 32 built-in names;
- an existing output directory is refused before anything is written (the reference's os.makedirs raises FileExistsError half-way)."""
import argparse
import os
import sys
from typing import Optional, Sequence

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, load_blendshape_deltas  # noqa: E402
from said_amd.util.mesh import Mesh, get_submesh, load_mesh, save_mesh  # noqa: E402
from said_amd.util.parser import parse_list  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Preprocess the VOCA dataset and generate ARKit blendshapes")
    p.add_argument("--templates_dir", type=str, default="../BlendVOCA/templates", help="Directory of the template meshes")
    p.add_argument("--blendshape_residuals_path", type=str, default="../BlendVOCA/blendshape_residuals.pickle", help="Path of the blendshape residuals")
    p.add_argument("--blendshapes_out_dir", type=str, default="../output_blendshapes", help="Directory of output blendshapes")
    p.add_argument("--head_idx_path", type=str, default=None, help="List of the head indices (required). Empty string will disable this option.")
    p.add_argument("--blendshape_list_path", type=str, default=None, help="List of the blendshapes (default: the 32 built-in ARKit names)")
    p.add_argument("--person_ids", type=str, default=None, help="Comma-separated person ids (default: every person of the residuals)")
    return p


def template_path(templates_dir: str, pid: str) -> str:
    for ext in (".ply", ".obj"):
        path = os.path.join(templates_dir, pid + ext)
        if os.path.isfile(path):
            return path
    raise SystemExit(f"no template of {pid}: neither {pid}.ply nor {pid}.obj in {templates_dir}")


def head_of(template: Mesh, head_idx: Optional[Sequence[int]]) -> Mesh:
    return template if head_idx is None else get_submesh(template.vertices, template.faces, head_idx)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if args.head_idx_path is None:
        raise SystemExit("--head_idx_path is required: a file of vertex indices (FLAME_head_idx.txt), or \"\" to use whole templates")
    head_idx = parse_list(args.head_idx_path, int) if args.head_idx_path else None
    names = parse_list(args.blendshape_list_path, str) if args.blendshape_list_path else list(DEFAULT_BLENDSHAPE_CLASSES)
    deltas = load_blendshape_deltas(args.blendshape_residuals_path)
    pids = [p for p in args.person_ids.split(",") if p] if args.person_ids else list(deltas)
    templates_head = os.path.join(args.blendshapes_out_dir, "templates_head")
    blendshapes_head = os.path.join(args.blendshapes_out_dir, "blendshapes_head")
    for d in (templates_head, blendshapes_head):
        if os.path.exists(d):
            raise SystemExit(f"{d} exists: choose a new --blendshapes_out_dir")
    for pid in pids:   # everything that can be refused, before anything is written
        if pid not in deltas:
            raise SystemExit(f"{args.blendshape_residuals_path} has no residuals of {pid}")
        missing = [n for n in names if n not in deltas[pid]]
        if missing:
            raise SystemExit(f"{args.blendshape_residuals_path} lacks {len(missing)} blendshape(s) of {pid}, the first {missing[0]}")
        template_path(args.templates_dir, pid)
    os.makedirs(templates_head)
    os.makedirs(blendshapes_head)
    for pid in pids:
        head = head_of(load_mesh(template_path(args.templates_dir, pid)), head_idx)
        save_mesh(head, os.path.join(templates_head, f"{pid}.obj"))
        os.makedirs(os.path.join(blendshapes_head, pid))
        for name in names:
            d = np.asarray(deltas[pid][name], dtype=np.float64)
            if d.shape != head.vertices.shape:
                raise SystemExit(f"{pid}/{name}: residuals of shape {d.shape} for a head of {head.vertices.shape[0]} vertices")
            save_mesh(Mesh(head.vertices + d, head.faces), os.path.join(blendshapes_head, pid, f"{name}.obj"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
