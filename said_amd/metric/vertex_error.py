"""Vertex error of generated animation against the real one (the reference's evaluate_vertex_error, script/test_evaluate.py:192-238),
computed on the MI355X in float64 (include/said_beat.h).

For a pair, with L = min of the two lengths: max over t < L of the Euclidean norm of (real - generated)[t] @ delta over all vertices, delta
being the person's (blendshapes, vertices, 3) deltas.  The result over pairs is ``statistics.mean`` of these maxima.
"""
from __future__ import annotations

import statistics
from typing import Sequence

import numpy as np
import torch

from .._engine import host_f32
from .beat_consistency import engine_for


def vertex_errors(pairs: Sequence, blendshape_deltas: Sequence, device=None) -> np.ndarray:
    """(n,) float64 for pairs [(real (T_r, C), generated (T_g, C), person)], person indexing blendshape_deltas [(C, V, 3), ...]."""
    if not len(pairs):
        raise ValueError("no pairs")
    deltas = [np.asarray(d.detach().cpu().numpy() if isinstance(d, torch.Tensor) else d, dtype=np.float64) for d in blendshape_deltas]
    if any(d.ndim != 3 or d.shape != deltas[0].shape for d in deltas):
        raise ValueError("blendshape deltas must be (blendshapes, vertices, 3), the same shape for every person")
    c = deltas[0].shape[0]
    seqs, real_off, eval_off, length, person, rows = [], [], [], [], [], 0
    for real, gen, p in pairs:
        real, gen = host_f32(real), host_f32(gen)
        if real.ndim != 2 or gen.ndim != 2 or real.shape[1] != c or gen.shape[1] != c:
            raise ValueError(f"coefficients must be (frames, {c}), got {real.shape} and {gen.shape}")
        n = min(real.shape[0], gen.shape[0])
        if n < 1:
            raise ValueError("a pair has a sequence without frames")
        real_off.append(rows)
        eval_off.append(rows + n)
        length.append(n)
        person.append(int(p))
        seqs += [real[:n], gen[:n]]
        rows += 2 * n
    eng = engine_for(device)
    eng.set_deltas(np.stack([d.reshape(c, -1) for d in deltas]))
    return eng.vertex_error(torch.from_numpy(np.concatenate(seqs)).to(eng.device), real_off, eval_off, length, person)


def vertex_error(real, generated, blendshape_delta, device=None) -> float:
    """One pair: real (T_r, C) and generated (T_g, C) coefficients, blendshape_delta (C, V, 3)."""
    return float(vertex_errors([(real, generated, 0)], [blendshape_delta], device)[0])


def mean_vertex_error(pairs: Sequence, blendshape_deltas: Sequence, device=None) -> float:
    """``statistics.mean`` of the pairs' vertex errors, as the reference's evaluate_vertex_error returns."""
    return statistics.mean(float(e) for e in vertex_errors(pairs, blendshape_deltas, device))
