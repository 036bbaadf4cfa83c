"""Beat consistency of generated animation with its audio (said/metric/beat_consistency.py), computed on the MI355X.

The audio beats restate ``librosa.onset.onset_detect`` with its defaults, the kinematic beats are the minima of the coefficients' change
rate by ``scipy.signal.find_peaks``'s rule, and a sequence scores the mean over its audio beats of exp(-d^2 / (2 sigma^2)), d being the
distance to the nearest kinematic beat.  DESIGN.md section 12.1 is the specification; every pass runs in HIP in float64
(include/said_beat.h).  librosa is not needed.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import _engine

_engines: Dict[int, _engine.BeatEngine] = {}


def engine_for(device=None, sampling_rate: Optional[int] = None) -> _engine.BeatEngine:
    """The beat context of `device` (default: the current CUDA device), its mel bank formed for `sampling_rate` when one is given."""
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise _engine.NoCpuPathError(_engine.BeatEngine.cpu_message.format(device))
    if not torch.cuda.is_available():
        raise _engine.NoCpuPathError(_engine.BeatEngine.cpu_message.format("none visible"))
    idx = device.index if device.index is not None else torch.cuda.current_device()
    e = _engines.get(idx)
    if e is None:
        e = _engines[idx] = _engine.BeatEngine(torch.device("cuda", idx))
    if sampling_rate is not None and e.sampling_rate != int(sampling_rate):
        e.set_sampling_rate(int(sampling_rate))
    return e


def analyse_clips(eng: _engine.BeatEngine, list_waveform: Sequence) -> np.ndarray:
    """Analyses the distinct waveforms on the device (waveforms that are the same object are one clip) and returns the clip of each
    waveform; the onsets stay on the device (``eng.read_onsets()`` reads them back)."""
    seen, clips, index = {}, [], []
    for w in list_waveform:
        if id(w) not in seen:
            seen[id(w)] = len(clips)
            clips.append(_engine.host_f32(w).reshape(-1))
        index.append(seen[id(w)])
    if any(c.shape[0] < 1 for c in clips):
        raise ValueError("a waveform has no samples")
    offsets = np.concatenate([[0], np.cumsum([c.shape[0] for c in clips])]).astype(np.int64)
    eng.clips(torch.from_numpy(np.concatenate(clips)).to(eng.device), offsets)
    return np.asarray(index, dtype=np.int32)


def beat_consistency_scores(list_waveform: Sequence, list_blendshape_coeffs: Sequence, sampling_rate: int, fps: int, threshold: float,
                            sigma: float = 0.1, device=None) -> np.ndarray:
    """The score of every sequence, (n,) float64: 0 without a kinematic beat, NaN without an audio beat."""
    if len(list_waveform) != len(list_blendshape_coeffs) or not len(list_waveform):
        raise ValueError(f"{len(list_waveform)} waveforms for {len(list_blendshape_coeffs)} coefficient sequences (one each, at least one)")
    seqs = [_engine.host_f32(c) for c in list_blendshape_coeffs]
    if any(c.ndim != 2 or c.shape[1] != seqs[0].shape[1] for c in seqs):
        raise ValueError("coefficient sequences must be (frames, channels) with one number of channels")
    if any(c.shape[0] < 2 for c in seqs):
        raise ValueError("a coefficient sequence has fewer than 2 frames: it has no change rate")
    eng = engine_for(device, sampling_rate)
    clip_index = analyse_clips(eng, list_waveform)
    offsets = np.concatenate([[0], np.cumsum([c.shape[0] for c in seqs])]).astype(np.int64)
    eng.coeffs(torch.from_numpy(np.concatenate(seqs)).to(eng.device), offsets, threshold)
    return eng.score(clip_index, fps, sigma)


def beat_consistency_score(list_waveform: List[np.ndarray], list_blendshape_coeffs: List[np.ndarray], sampling_rate: int, fps: int,
                           threshold: float, sigma: float = 0.1, device=None) -> float:
    """Compute the beat consistency score (the reference's signature, plus `device`).

    list_waveform: waveforms (audio_sequence_len,); list_blendshape_coeffs: the corresponding coefficients (blendshape_seq_len,
    num_blendshapes); sampling_rate of the waveforms; fps of the coefficients; threshold for the minima of the change rate; sigma of the
    score's Gaussian."""
    return float(np.mean(beat_consistency_scores(list_waveform, list_blendshape_coeffs, sampling_rate, fps, threshold, sigma, device)))
