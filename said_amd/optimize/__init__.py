"""Pseudo-GT blendshape coefficients (said.optimize): the per-sequence quadratic program of said/optimize/blendshape_coeffs.py, solved on the
MI355X (include/said_optimize.h)."""
from .blendshape_coeffs import (OptimizationError, OptimizationProblemFull, OptimizationProblemSingle, SolveInfo, kkt_certificate,
                                reference_qp)

__all__ = ["OptimizationError", "OptimizationProblemFull", "OptimizationProblemSingle", "SolveInfo", "kkt_certificate", "reference_qp"]
