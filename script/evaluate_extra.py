"""script/test_evaluate.py's evaluation plus the two metrics the reference's driver keeps commented out: beat consistency and vertex error.

The reference defines evaluate_beat_consistency_score and evaluate_vertex_error (script/test_evaluate.py:142-238) and comments out only
their calls in evaluate() (:386-403).  script/test_evaluate.py is kept exactly as it is (a feature change leaves the existing test_*.py files
of this repository untouched, and that driver's name makes it one of them), so the two metrics have a driver of their own.  It takes every
flag of script/test_evaluate.py, with the same defaults, and three of its own, which are not reference flags:
- --beat_consistency: the beat consistency score of the generated sequences whose (speaker, sentence) the real set has, each against its
  sentence's audio; uses --sampling_rate, --fps and --bc_threshold (which script/test_evaluate.py accepts and leaves unused);
- --vertex_error: the vertex error of those sequences against the real ones; uses --blendshape_residuals_path;
- --only_extra: leave script/test_evaluate.py's latent metrics (and its EvalMetrics line) out.
Unless --only_extra is given it first runs script/test_evaluate.py's main() with the remaining arguments, which prints the EvalMetrics(...) line as ever, and then prints
a second line, ExtraMetrics(beat_consistency=..., vertex_error=...) (None for a metric that was not asked for).  Both metrics run on the
MI355X in float64 (said_amd.metric.beat_consistency, said_amd.metric.vertex_error); librosa is not needed.
"""
import importlib.util
import os
import pickle
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _load_test_evaluate():
    spec = importlib.util.spec_from_file_location("said_script_test_evaluate", os.path.join(ROOT, "script", "test_evaluate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ev = _load_test_evaluate()
FLAGS = ("--beat_consistency", "--vertex_error", "--only_extra")


@dataclass
class ExtraMetrics:
    """The two metrics the reference's evaluate() leaves commented out (None: not asked for)"""

    beat_consistency: Optional[float]
    vertex_error: Optional[float]


def evaluate_beat_consistency_score(audio_dir: str, eval_paths, real_paths, sampling_rate: int, fps: int, bc_threshold: float, device) -> float:
    """evaluate_beat_consistency_score (test_evaluate.py:142-189): the generated sequences whose (speaker, sentence) the real set has, each
    against its sentence's audio.  Every WAV file is loaded once, and its repeats share that one waveform object (analysed once)."""
    from said_amd.metric.beat_consistency import beat_consistency_score
    from said_amd.util.audio import load_audio
    from said_amd.util.blendshape import load_blendshape_coeffs
    real = {(pid, sid) for pid, sid, _ in real_paths}
    audio, waves, coeffs = {}, [], []
    for pid, sid, path in eval_paths:
        if (pid, sid) not in real:
            continue
        if (pid, sid) not in audio:
            audio[(pid, sid)] = load_audio(os.path.join(audio_dir, pid, f"sentence{sid:02}.wav"), sampling_rate).numpy()
        waves.append(audio[(pid, sid)])
        coeffs.append(load_blendshape_coeffs(path).numpy())
    if not waves:
        raise SystemExit("no generated sequence has a real counterpart: nothing to compute beat consistency of")
    return beat_consistency_score(waves, coeffs, sampling_rate, fps, bc_threshold, device=device)


def evaluate_vertex_error(eval_paths, real_paths, blendshape_residuals_path: str, device) -> float:
    """evaluate_vertex_error (test_evaluate.py:192-238); the deltas are read as said_amd/training/unet.py reads them: a pickle of
    {person: {blendshape: (V, 3)}}, stacked in the dictionary's order."""
    from said_amd.metric.vertex_error import mean_vertex_error
    from said_amd.util.blendshape import load_blendshape_coeffs
    if not os.path.isfile(blendshape_residuals_path):
        raise SystemExit(f"--vertex_error needs the blendshape deltas: {blendshape_residuals_path} (--blendshape_residuals_path) does not exist")
    with open(blendshape_residuals_path, "rb") as f:
        residuals = pickle.load(f)
    real = {}
    for pid, sid, path in real_paths:   # a later file of one (speaker, sentence) replaces an earlier one, as in the reference's dictionary
        real[(pid, sid)] = load_blendshape_coeffs(path).numpy()
    persons, deltas, pairs = {}, [], []
    for pid, sid, path in eval_paths:
        if (pid, sid) not in real:
            continue
        if pid not in persons:
            if pid not in residuals:
                raise SystemExit(f"{blendshape_residuals_path} has no deltas of {pid}")
            persons[pid] = len(deltas)
            deltas.append(np.stack(list(residuals[pid].values()), axis=0).astype(np.float32))
        pairs.append((real[(pid, sid)], load_blendshape_coeffs(path).numpy(), persons[pid]))
    if not pairs:
        raise SystemExit("no generated sequence has a real counterpart: nothing to compute the vertex error of")
    return mean_vertex_error(pairs, deltas, device=device)


def build_parser():
    ap = ev.build_parser()
    ap.allow_abbrev = False   # the flags below are taken out of the arguments by their full names
    ap.description = "script/test_evaluate.py's evaluation, then beat consistency and vertex error (on an MI355X)"
    ap.add_argument("--beat_consistency", action="store_true", help="also compute the beat consistency score (uses --sampling_rate, --fps, --bc_threshold)")
    ap.add_argument("--vertex_error", action="store_true", help="also compute the vertex error (uses --blendshape_residuals_path)")
    ap.add_argument("--only_extra", action="store_true", help="skip script/test_evaluate.py's FD, multimodality and WInD")
    return ap


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    if args.vertex_error and not os.path.isfile(args.blendshape_residuals_path):   # before the latent metrics, not after them
        raise SystemExit(f"--vertex_error needs the blendshape deltas: {args.blendshape_residuals_path} (--blendshape_residuals_path) does not exist")
    metrics = None if args.only_extra else ev.main([a for a in argv if a not in FLAGS])
    bc = ve = None
    if args.beat_consistency or args.vertex_error:
        eval_paths, real_paths = ev.get_data_paths(args.audio_dir, args.coeffs_dir), ev.get_data_paths(args.audio_dir, args.coeffs_real_dir)
        if args.beat_consistency:
            bc = evaluate_beat_consistency_score(args.audio_dir, eval_paths, real_paths, args.sampling_rate, args.fps, args.bc_threshold, args.device)
        if args.vertex_error:
            ve = evaluate_vertex_error(eval_paths, real_paths, args.blendshape_residuals_path, args.device)
    extra = ExtraMetrics(beat_consistency=bc, vertex_error=ve)
    print(extra)
    return metrics, extra


if __name__ == "__main__":
    main()
