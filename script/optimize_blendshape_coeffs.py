"""Generate the pseudo-GT blendshape coefficients of mesh sequences on an MI355X.

Command-line compatible with the reference's script/optimize_blendshape_coeffs.py:16-58 (same six flags and defaults), with these
differences:
- --blendshape_list_path defaults to the 32 built-in names of said_amd/util/blendshape.py (the reference's default,
  data/ARKit_blendshapes.txt, lists the same names in the same order and is not part of this repository);
- --head_idx_path has no default: give a file of vertex indices, or "" to use every vertex of the sequences;
- an existing <out>/<person> directory is refused with a clear error before anything of that person is solved (the reference raises
  a string, which is a TypeError);
- new optional flags: --delta (the difference bound, 0.1 as in the reference), --person_ids (a comma-separated subset), --io_workers;
- one timing line per person separates mesh reading, the rhs kernel and the solve.

As in the reference (script/dataset/dataset_voca.py:1000-1087), the neutral is <neutrals_dir>/<person>.obj, the blendshapes
<blendshapes_dir>/<person>/<name>.obj, and the frames of sentence NN are sorted(glob("**/*.obj") + glob("**/*.ply")) under
<mesh_seqs_dir>/<person>/sentenceNN (a missing directory is skipped); --head_idx_path subsets the sequence vertices only.  All sentences of
one person are solved in one launch, one workgroup per sentence; the next person's meshes are read while the GPU solves.
"""
import argparse
import glob
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, save_blendshape_coeffs  # noqa: E402
from said_amd.util.mesh import load_vertices  # noqa: E402
from said_amd.util.parser import parse_list  # noqa: E402

# script/dataset/dataset_voca.py:74-95: person_ids_train + person_ids_val + person_ids_test, sentences 1..40
PERSON_IDS = ["FaceTalk_170725_00137_TA", "FaceTalk_170728_03272_TA", "FaceTalk_170811_03274_TA", "FaceTalk_170904_00128_TA",
              "FaceTalk_170904_03276_TA", "FaceTalk_170912_03278_TA", "FaceTalk_170913_03279_TA", "FaceTalk_170915_00223_TA",
              "FaceTalk_170811_03275_TA", "FaceTalk_170908_03277_TA",
              "FaceTalk_170731_00024_TA", "FaceTalk_170809_00138_TA"]
SENTENCE_IDS = list(range(1, 41))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Generate the Pseudo-GT blendshape coefficients by solving the optimization problem")
    p.add_argument("--neutrals_dir", type=str, default="../BlendVOCA/templates_head", help="Directory of the neutral meshes")
    p.add_argument("--blendshapes_dir", type=str, default="../BlendVOCA/blendshapes_head", help="Directory of the blendshape meshes")
    p.add_argument("--mesh_seqs_dir", type=str, default="../BlendVOCA/unposedcleaneddata", help="Directory of the mesh sequences")
    p.add_argument("--blendshape_list_path", type=str, default=None, help="List of the blendshapes (default: the 32 built-in ARKit names)")
    p.add_argument("--head_idx_path", type=str, default=None, help="List of the head indices (required). Empty string will disable this option.")
    p.add_argument("--blendshapes_coeffs_out_dir", type=str, default="../output_coeffs", help="Directory of the output coefficients")
    p.add_argument("--delta", type=float, default=0.1, help="Bound of |w_t - w_{t+1}|")
    p.add_argument("--person_ids", type=str, default=None, help="Comma-separated person ids (default: train + val + test)")
    p.add_argument("--io_workers", type=int, default=8, help="Threads reading mesh files")
    p.add_argument("--device", type=str, default="cuda:0", help="MI355X to run on")
    return p


def sequence_paths(mesh_seqs_dir: str, person_id: str, seq_id: int) -> List[str]:
    """The frame files of one sentence in the reference's order; [] when its directory is missing."""
    d = os.path.join(mesh_seqs_dir, person_id, f"sentence{seq_id:02}")
    if not os.path.isdir(d):
        return []
    files_obj = glob.glob(os.path.join(d, "**/*.obj"), recursive=True)
    files_ply = glob.glob(os.path.join(d, "**/*.ply"), recursive=True)
    return sorted(files_obj + files_ply)


def load_basis(neutrals_dir: str, blendshapes_dir: str, person_id: str, names: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """(neutral (3V, 1), blendshapes (3V, K)) of one person, vertices flattened row-major."""
    n = load_vertices(os.path.join(neutrals_dir, f"{person_id}.obj")).reshape(-1, 1)
    b = [load_vertices(os.path.join(blendshapes_dir, person_id, f"{name}.obj")).reshape(-1, 1) for name in names]
    return n, np.concatenate(b, axis=1)


def load_frames(paths: Sequence[str], head_idx: Optional[Sequence[int]], pool: Optional[ThreadPoolExecutor] = None) -> List[np.ndarray]:
    """(3V', 1) vertex vectors of the frames, subset to head_idx when given."""
    def one(p):
        v = load_vertices(p)
        if head_idx is not None:
            v = v[head_idx]
        return v.reshape(-1, 1)
    return list(pool.map(one, paths)) if pool is not None else [one(p) for p in paths]


def person_jobs(args, names, head_idx, person_ids, pool):
    """Yields (person_id, neutral, blendshapes, [(seq_id, frames)], seconds spent reading), reading one person ahead of the consumer."""
    def read(pid):
        t0 = time.perf_counter()
        n, b = load_basis(args.neutrals_dir, args.blendshapes_dir, pid, names)
        seqs = []
        for sid in SENTENCE_IDS:
            paths = sequence_paths(args.mesh_seqs_dir, pid, sid)
            if paths:
                seqs.append((sid, load_frames(paths, head_idx, pool)))
        return pid, n, b, seqs, time.perf_counter() - t0

    with ThreadPoolExecutor(max_workers=1) as ahead:
        fut = ahead.submit(read, person_ids[0]) if person_ids else None
        for i in range(len(person_ids)):
            job = fut.result()
            fut = ahead.submit(read, person_ids[i + 1]) if i + 1 < len(person_ids) else None
            yield job


def main(argv=None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.head_idx_path is None:
        parser.error("--head_idx_path is required: give the head vertex index file (the reference's data/FLAME_head_idx.txt is not part of "
                     "this repository), or \"\" to use every vertex")
    names = DEFAULT_BLENDSHAPE_CLASSES if args.blendshape_list_path is None else parse_list(args.blendshape_list_path, str)
    head_idx = None if args.head_idx_path == "" else parse_list(args.head_idx_path, int)
    person_ids = PERSON_IDS if args.person_ids is None else [p for p in args.person_ids.split(",") if p]
    for pid in person_ids:
        out_dir = os.path.join(args.blendshapes_coeffs_out_dir, pid)
        if os.path.exists(out_dir):
            raise FileExistsError(f"{out_dir} already exists: refusing to overwrite the coefficients of {pid}")

    from said_amd.optimize import OptimizationProblemFull

    with ThreadPoolExecutor(max_workers=max(1, args.io_workers)) as pool:
        for pid, n, b, seqs, t_io in person_jobs(args, names, head_idx, person_ids, pool):
            if not seqs:
                print(f"{pid}: no sequences", flush=True)
                continue
            prob = OptimizationProblemFull(n, b, device=args.device)
            timings = {}
            sols = prob.optimize_batch([f for _, f in seqs], delta=args.delta, timings=timings)
            out_dir = os.path.join(args.blendshapes_coeffs_out_dir, pid)
            os.makedirs(out_dir)
            for (sid, _), w in zip(seqs, sols):
                save_blendshape_coeffs(w, names, os.path.join(out_dir, f"sentence{sid:02}.csv"))
            frames = sum(len(f) for _, f in seqs)
            print(f"{pid}: {len(seqs)} sequences, {frames} frames; io {t_io:.3f} s, rhs {timings['rhs']:.4f} s, solve {timings['solve']:.4f} s "
                  f"({timings['iters_max']} IP iterations at most)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
