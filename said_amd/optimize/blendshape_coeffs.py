"""The optimisation problems of pseudo-GT blendshape coefficients (reference: said/optimize/blendshape_coeffs.py).

Both classes keep the reference's constructors and ``optimize`` signatures and return float64 numpy arrays after the reference's
``np.clip(w, 0, 1)``.  The right-hand sides q_t = B_delta' (n - v_t) and the interior-point solve run on the device (said_amd/csrc/blendshape_qp.hip);
there is no CPU path.  ``init_vals`` is accepted and ignored: in the reference it is only a warm start of cvxopt, and the optimum is unique
(P is positive definite for linearly independent blendshapes).  A solve that does not converge, or non-finite input, raises
``OptimizationError``; no result is returned silently."""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import _engine

DEFAULT_MAX_ITER = 100
DEFAULT_TOL = 1e-12
_STATUS = {_engine.OPT_MAX_ITER: "did not converge within max_iter iterations", _engine.OPT_NOT_FINITE: "broke down (non-finite iterate)"}


class OptimizationError(_engine.EngineError):
    pass


@dataclass
class SolveInfo:
    """Per-sequence solver report.  w: unclipped primal solutions (T, K); duals: (T, 4, K) for -w <= 0, w <= 1, w_t - w_{t+1} <= delta,
    w_{t+1} - w_t <= delta (the last two zero at the last frame and in the single problem); iters; resid: relative primal, dual residual and
    duality gap at exit."""
    w: List[np.ndarray]
    duals: List[np.ndarray]
    iters: np.ndarray
    resid: np.ndarray


def _as_vector(v: np.ndarray, n3v: int, what: str) -> np.ndarray:
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.shape[0] != n3v:
        raise OptimizationError(f"{what} has {a.shape[0]} values, the basis {n3v}")
    return a


class _Problem:
    def __init__(self, neutral_vector: np.ndarray, blendshapes_matrix: np.ndarray, device="cuda"):
        self.neutral_vector = np.asarray(neutral_vector, dtype=np.float64).reshape(-1, 1)
        blendshapes_matrix = np.asarray(blendshapes_matrix, dtype=np.float64)
        if blendshapes_matrix.ndim != 2 or blendshapes_matrix.shape[0] != self.neutral_vector.shape[0]:
            raise OptimizationError(f"blendshapes_matrix must be (3V, K) with 3V = {self.neutral_vector.shape[0]}, got {blendshapes_matrix.shape}")
        self.num_blendshapes = blendshapes_matrix.shape[1]
        if self.num_blendshapes > _engine.OPTIMIZE_MAX_K:
            raise OptimizationError(f"{self.num_blendshapes} blendshapes exceed the solver's {_engine.OPTIMIZE_MAX_K}")
        if not (np.all(np.isfinite(self.neutral_vector)) and np.all(np.isfinite(blendshapes_matrix))):
            raise OptimizationError("non-finite neutral or blendshape vertices")
        self.blendshapes_matrix_delta = blendshapes_matrix - self.neutral_vector   # B_delta, as the reference forms it
        self.P = self.blendshapes_matrix_delta.T @ self.blendshapes_matrix_delta
        self.lbw = np.zeros(self.num_blendshapes)
        self.ubw = np.ones(self.num_blendshapes)
        self._eng = _engine.OptimizeEngine(torch.device(device))
        self.device = self._eng.device
        self._eng.set_bases(self.neutral_vector.reshape(1, -1), self.blendshapes_matrix_delta[None], self.P[None])

    @property
    def btb(self) -> np.ndarray:
        return self.P

    def rhs(self, frames: Sequence[np.ndarray]) -> torch.Tensor:
        """q (frames, K) on the device for a list of (3V, 1) vertex vectors."""
        n3v = self.neutral_vector.shape[0]
        v = np.stack([_as_vector(f, n3v, "a vertices vector") for f in frames])
        if not np.all(np.isfinite(v)):
            raise OptimizationError("non-finite target vertices")
        return self._eng.rhs(0, torch.from_numpy(v).to(self.device))

    def _solve(self, q: torch.Tensor, lengths: Sequence[int], delta: float, coupled: bool, max_iter: int, tol: float, want_info: bool):
        if coupled and not (np.isfinite(delta) and delta > 0):
            raise OptimizationError(f"delta must be positive and finite, got {delta}")
        offs = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
        w, z, st, it, res = self._eng.solve(q, offs, np.zeros(len(lengths), dtype=np.int32), delta if coupled else 1.0, coupled, max_iter, tol,
                                            want_duals=want_info)
        bad = np.nonzero(st != _engine.OPT_CONVERGED)[0]
        if bad.size:
            i = int(bad[0])
            raise OptimizationError(f"sequence {i} of {len(lengths)} {_STATUS.get(int(st[i]), f'status {st[i]}')}: "
                                    f"{it[i]} iterations, relative residuals primal {res[i, 0]:.2e} dual {res[i, 1]:.2e} gap {res[i, 2]:.2e}")
        w = w.cpu().numpy()
        ws = [w[offs[i]:offs[i + 1]] for i in range(len(lengths))]
        info = None
        if want_info:
            z = z.cpu().numpy()
            info = SolveInfo(w=ws, duals=[z[offs[i]:offs[i + 1]] for i in range(len(lengths))], iters=it, resid=res)
        return [np.clip(x, 0.0, 1.0) for x in ws], info


class OptimizationProblemSingle(_Problem):
    """One frame: minimise 1/2 w' P w + q' w subject to 0 <= w <= 1."""

    def optimize(self, vertices_vector: np.ndarray, init_vals: Optional[np.ndarray] = None, *, max_iter: int = DEFAULT_MAX_ITER,
                 tol: float = DEFAULT_TOL, return_info: bool = False):
        """(K,) solution for a (3V, 1) target; with return_info also the SolveInfo."""
        out, info = self.optimize_batch([vertices_vector], max_iter=max_iter, tol=tol, return_info=True)
        return (out[0], info) if return_info else out[0]

    def optimize_batch(self, vertices_vectors: Sequence[np.ndarray], *, max_iter: int = DEFAULT_MAX_ITER, tol: float = DEFAULT_TOL,
                       return_info: bool = False):
        """(N, K): N independent frames solved in one launch."""
        q = self.rhs(vertices_vectors)
        ws, info = self._solve(q, [1] * len(vertices_vectors), 1.0, False, max_iter, tol, return_info)
        out = np.concatenate(ws, axis=0)
        return (out, info) if return_info else out


class OptimizationProblemFull(_Problem):
    """A sequence: minimise sum_t 1/2 w_t' P w_t + q_t' w_t subject to 0 <= w_t <= 1 and |w_t - w_{t+1}| <= delta."""

    def optimize(self, vertices_vector_list: List[np.ndarray], init_vals: Optional[np.ndarray] = None, delta: float = 0.1, *,
                 max_iter: int = DEFAULT_MAX_ITER, tol: float = DEFAULT_TOL, return_info: bool = False):
        """(seq_len, K) solution; with return_info also the SolveInfo."""
        out, info = self.optimize_batch([vertices_vector_list], delta=delta, max_iter=max_iter, tol=tol, return_info=True)
        return (out[0], info) if return_info else out[0]

    def optimize_batch(self, list_of_sequences: Sequence[Sequence[np.ndarray]], delta: float = 0.1, *, max_iter: int = DEFAULT_MAX_ITER,
                       tol: float = DEFAULT_TOL, return_info: bool = False, timings: Optional[dict] = None):
        """[(T_i, K)]: many sequences of this basis in one launch (one workgroup each).  timings, when given, receives the seconds of the
        rhs kernel ("rhs", upload included) and of the solve ("solve"), and the largest iteration count ("iters_max")."""
        lengths = [len(s) for s in list_of_sequences]
        if not lengths or min(lengths) < 1:
            raise OptimizationError("every sequence needs at least one frame")
        t0 = time.perf_counter()
        q = self.rhs([f for s in list_of_sequences for f in s])
        if timings is not None:
            torch.cuda.synchronize(self.device)
        t1 = time.perf_counter()
        ws, info = self._solve(q, lengths, delta, True, max_iter, tol, return_info or timings is not None)
        if timings is not None:
            timings.update(rhs=t1 - t0, solve=time.perf_counter() - t1, iters_max=int(info.iters.max()))
        return (ws, info) if return_info else ws

    def compute_g(self, seq_len: int) -> np.ndarray:
        """The reference's difference rows, dense: per frame pair a +I | -I block followed by -I | +I."""
        return reference_qp(self.blendshapes_matrix_delta, self.neutral_vector, [self.neutral_vector] * seq_len, 0.1)[2]


def reference_qp(bdelta: np.ndarray, neutral_vector: np.ndarray, vertices_vector_list: Sequence[np.ndarray], delta: float = 0.1):
    """The dense (P, q, G, h, lb, ub) that OptimizationProblemFull.optimize poses to its solver in the reference (host, float64)."""
    neutral_vector = np.asarray(neutral_vector, dtype=np.float64).reshape(-1, 1)
    K = bdelta.shape[1]
    T = len(vertices_vector_list)
    btb = bdelta.T @ bdelta
    P = np.kron(np.eye(T), btb)
    q = np.vstack([bdelta.T @ (neutral_vector - np.asarray(v, dtype=np.float64).reshape(-1, 1)) for v in vertices_vector_list]).reshape(-1)
    G = np.zeros((2 * K * max(T - 1, 0), K * T))
    eye = np.eye(K)
    for t in range(T - 1):
        r = 2 * K * t
        G[r:r + K, K * t:K * (t + 1)] = eye
        G[r:r + K, K * (t + 1):K * (t + 2)] = -eye
        G[r + K:r + 2 * K, K * t:K * (t + 1)] = -eye
        G[r + K:r + 2 * K, K * (t + 1):K * (t + 2)] = eye
    h = np.full(G.shape[0], delta)
    return P, q, G, h, np.zeros(K * T), np.ones(K * T)


def kkt_certificate(P: np.ndarray, q: np.ndarray, delta: Optional[float], w: np.ndarray, z: np.ndarray) -> dict:
    """Optimality certificate of w (T, K) with duals z (T, 4, K) for the problem with block P (K, K) and q (T, K); delta None: no
    difference rows.  Every inequality is written as G x <= h.  Returns the primal violation after the clip, the most negative dual, the
    stationarity ||P w_t + q_t + (G' z)_t||_inf relative to ||P|| + ||q|| (max norms), the duality gap f(w) - g(z) with
    g(z) = -1/2 x^ (I (x) P) x^ - h' z at x^ = -(I (x) P)^-1 (q + G' z), relative to 1 + |f|, and f."""
    w = np.clip(np.asarray(w, dtype=np.float64), 0.0, 1.0)
    q = np.asarray(q, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    T = w.shape[0]
    zlo, zhi, zdp, zdm = z[:, 0], z[:, 1], z[:, 2].copy(), z[:, 3].copy()
    zdp[T - 1] = 0.0
    zdm[T - 1] = 0.0
    if delta is None:
        zdp[:] = 0.0
        zdm[:] = 0.0
    gz = -zlo + zhi + zdp - zdm
    gz[1:] -= (zdp - zdm)[:-1]
    stat = np.abs(w @ P + q + gz).max() / (np.abs(P).max() + np.abs(q).max())
    f = float(np.sum(0.5 * w * (w @ P) + q * w))
    xh = -np.linalg.solve(P, (q + gz).T).T
    hz = float(np.sum(zhi)) + (float(delta) * float(np.sum(zdp + zdm)) if delta is not None else 0.0)
    g = -float(np.sum(0.5 * xh * (xh @ P))) - hz
    viol = 0.0 if T < 2 or delta is None else float(np.abs(np.diff(w, axis=0)).max() - delta)
    used = [z[:, 0], z[:, 1]] + ([z[:-1, 2], z[:-1, 3]] if (delta is not None and T > 1) else [])
    return {"diff_violation": viol, "min_dual": float(min(u.min() for u in used)), "stationarity": float(stat),
            "gap": (f - g) / (1.0 + abs(f)), "f": f}
