"""Evaluate generated animation against the BlendVOCA test set on an MI355X: Frechet distance, multimodality and WInD of BCVAE latents.

Command-line compatible with the reference's script/test_evaluate.py:454-540 (same flags and defaults), with these differences:
- --vae_weights_path is required (no VAE checkpoint ships with this repository; `synthetic` selects the seeded test weights);
- --seed (not a reference flag) seeds numpy's global generator before the GMM fits, which draw from it as scikit-learn does;
- --wind_num_repeats is honoured (the reference's loop runs 10 times whatever the flag says, test_evaluate.py:334; 10 is the default);
- within one (speaker, sentence, window) the repeats are taken in the order of their numeric file suffix (sentenceNN-<r>.csv), where the
  reference takes os.listdir's unspecified order: multimodality pairs the first half of the repeats with the second half;
- beat consistency and vertex error stay out, as they are commented out of the reference's evaluate() (test_evaluate.py:386-403);
  --blendshape_residuals_path, --sampling_rate, --fps and --bc_threshold are accepted and unused.

Files are enumerated as BlendVOCAEvalDataset.get_data_paths does (script/dataset/dataset_voca.py:175-241): the two test speakers,
`<dir>/<pid>/sentenceNN(-.+)?.csv` kept only where `<audio_dir>/<pid>/sentenceNN.wav` exists.  Every sliding window of 120 frames is
encoded in one engine call per sequence (BCVAE.encode_windows); the real set drops the last 2 windows (padding=2) and the generated
windows are kept only where the real set has the same (speaker, sentence, first frame).  The latents stay on the device: FD's moments
and the GMM fits run in HIP (said_amd.metric), multimodality is one float64 reduction on the device.
"""
import argparse
import os
import re
import statistics
import sys
from collections import OrderedDict
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from said_amd.metric.frechet_distance import frechet_distance, get_statistic  # noqa: E402
from said_amd.metric.wind import get_statistic_gmm, wind  # noqa: E402

PERSON_IDS_TEST = ["FaceTalk_170731_00024_TA", "FaceTalk_170809_00138_TA"]   # dataset_voca.py:90-93
SENTENCE_IDS = list(range(1, 41))                                             # dataset_voca.py:95


@dataclass
class StatisticMetric:
    """Dataclass for the statistic of metric"""

    mean: float
    std: float


@dataclass
class EvalMetrics:
    """Dataclass for the evaluation metrics"""

    frechet_distance: float
    multimodality: float
    wind: StatisticMetric


def _repeat_key(filename: str, base: str):
    """Sort key of sentenceNN[-<suffix>].csv: no suffix first, then numeric suffixes ascending, then the rest by name."""
    suffix = filename[len(base):-len(".csv")]
    if not suffix:
        return (0, 0, "")
    tail = suffix[1:]
    return (1, int(tail), "") if tail.isdigit() else (2, 0, tail)


def get_data_paths(audio_dir: str, coeffs_dir: str, person_ids: Optional[List[str]] = None) -> List[Tuple[str, int, str]]:
    """(person_id, sentence_id, csv path) as BlendVOCAEvalDataset.get_data_paths, repeats sorted by their numeric suffix."""
    out = []
    for pid in person_ids or PERSON_IDS_TEST:
        coeffs_id_dir = os.path.join(coeffs_dir, pid)
        for sid in SENTENCE_IDS:
            base = f"sentence{sid:02}"
            if not os.path.exists(os.path.join(audio_dir, pid, f"{base}.wav")):
                continue
            if not os.path.isdir(coeffs_id_dir):
                continue
            pat = re.compile(rf"^{base}(-.+)?\.csv$")
            names = sorted((s for s in os.listdir(coeffs_id_dir) if pat.match(s)), key=lambda s: _repeat_key(s, base))
            out += [(pid, sid, os.path.join(coeffs_id_dir, s)) for s in names]
    return out


def generate_latents(vae, paths, window_step_size: int, device, padding: int = 0):
    """(keys [(pid, sid, frame_start)], latents (N, 64) fp32 on the device): generate_latents_info (test_evaluate.py:53-106)."""
    from said_amd.util.blendshape import load_blendshape_coeffs
    keys, chunks = [], []
    for pid, sid, path in paths:
        coeffs = load_blendshape_coeffs(path).to(device)
        lat = vae.encode_windows(coeffs, window_step_size, padding=padding)
        keys += [(pid, sid, window_step_size * w) for w in range(lat.shape[0])]
        chunks.append(lat)
    lat = torch.cat(chunks) if chunks else torch.empty(0, vae.z_dim, device=device)
    return keys, lat


def filter_latents(eval_keys, eval_lat, real_keys):
    """filter_latent_infos (test_evaluate.py:109-137): the generated windows whose key the real set has."""
    real = set(real_keys)
    keep = [i for i, k in enumerate(eval_keys) if k in real]
    idx = torch.tensor(keep, dtype=torch.long, device=eval_lat.device)
    return [eval_keys[i] for i in keep], eval_lat.index_select(0, idx)


def multimodality_pairs(keys) -> Tuple[List[int], List[int]]:
    """evalute_multimodality's grouping (test_evaluate.py:273-304): per key, in first-seen order, the first half of its repeats against the second."""
    groups = OrderedDict()
    for i, k in enumerate(keys):
        groups.setdefault(k, []).append(i)
    a, b = [], []
    for idx in groups.values():
        h = len(idx) // 2
        a += idx[:h]
        b += idx[h:2 * h]
    return a, b


def evaluate_multimodality(keys, lat: torch.Tensor) -> float:
    a, b = multimodality_pairs(keys)
    if not a:
        return 0
    ia = torch.tensor(a, dtype=torch.long, device=lat.device)
    ib = torch.tensor(b, dtype=torch.long, device=lat.device)
    d = lat.index_select(0, ia).double() - lat.index_select(0, ib).double()
    return float(torch.linalg.vector_norm(d, dim=1).mean())


def evaluate(vae, eval_paths, real_paths, window_step_size: int, wind_num_clusters: int, wind_num_repeats: int, device,
             seed: Optional[int] = None) -> EvalMetrics:
    eval_keys, eval_lat = generate_latents(vae, eval_paths, window_step_size, device)
    real_keys, real_lat = generate_latents(vae, real_paths, window_step_size, device, padding=2)
    eval_keys, eval_lat = filter_latents(eval_keys, eval_lat, real_keys)
    if eval_lat.shape[0] == 0 or real_lat.shape[0] == 0:
        raise SystemExit(f"no latents to compare: {eval_lat.shape[0]} generated windows match the {real_lat.shape[0]} real ones")

    s_eval, s_real = get_statistic(eval_lat), get_statistic(real_lat)
    fd = frechet_distance(s_eval.mean, s_eval.cov, s_real.mean, s_real.cov)
    mm = evaluate_multimodality(eval_keys, eval_lat)

    if seed is not None:
        np.random.seed(seed)
    scores = []
    for _ in range(wind_num_repeats):
        eval_stats = get_statistic_gmm(eval_lat, wind_num_clusters)
        real_stats = get_statistic_gmm(real_lat, wind_num_clusters)
        scores.append(wind(eval_stats, real_stats))
    return EvalMetrics(frechet_distance=fd, multimodality=mm, wind=StatisticMetric(mean=statistics.mean(scores), std=statistics.stdev(scores)))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Evaluate the output based on the BlendVOCA test dataset (on an MI355X)")
    ap.add_argument("--audio_dir", type=str, default="../BlendVOCA/audio", help="Directory of the audio data")
    ap.add_argument("--coeffs_dir", type=str, default="../BlendVOCA/blendshape_coeffs", help="Directory of the blendshape coefficients data")
    ap.add_argument("--coeffs_real_dir", type=str, default="../BlendVOCA/blendshape_coeffs", help="Directory of the real blendshape coefficients data")
    ap.add_argument("--vae_weights_path", type=str, required=True, help="BCVAE state dict (vae.pth layout), or 'synthetic' for the seeded test weights")
    ap.add_argument("--blendshape_residuals_path", type=str, default="../BlendVOCA/blendshape_residuals.pickle", help="accepted, unused (vertex error)")
    ap.add_argument("--sampling_rate", type=int, default=16000, help="accepted, unused (beat consistency)")
    ap.add_argument("--fps", type=int, default=60, help="accepted, unused (beat consistency)")
    ap.add_argument("--bc_threshold", type=float, default=0.1, help="accepted, unused (beat consistency)")
    ap.add_argument("--wind_num_clusters", type=int, default=5, help="The number of clusters for computing WInD")
    ap.add_argument("--wind_num_repeats", type=int, default=10, help="The number of repetitions for computing WInD")
    ap.add_argument("--window_step_size", type=int, default=1, help="Step of the window movements for the latent generation")
    ap.add_argument("--device", type=str, default="cuda:0", help="the MI355X to run on")
    ap.add_argument("--seed", type=int, default=None, help="seed numpy's global generator before the GMM fits (default: leave it alone)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    from said_amd.model.vae import BCVAE
    device = torch.device(args.device)
    if device.type == "cuda":
        torch.cuda.set_device(device)
    vae = BCVAE()
    if args.vae_weights_path == "synthetic":
        from said_amd.util import synth
        state = synth.vae_state_dict()
    else:
        state = torch.load(args.vae_weights_path, map_location="cpu")
    vae.load_state_dict(state, strict=True)
    vae.to(device).eval()
    with torch.no_grad():
        metrics = evaluate(vae, get_data_paths(args.audio_dir, args.coeffs_dir), get_data_paths(args.audio_dir, args.coeffs_real_dir),
                           args.window_step_size, args.wind_num_clusters, args.wind_num_repeats, device, seed=args.seed)
    print(metrics)
    return metrics


if __name__ == "__main__":
    main()
