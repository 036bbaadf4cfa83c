"""Pseudo-GT blendshape coefficients (said.optimize): the per-sequence quadratic program of said/optimize/blendshape_coeffs.py, solved on the
MI355X (include/said_optimize.h); and blendshapes for a new head by deformation transfer (deformation_transfer.py, include/said_transfer.h)."""
from .blendshape_coeffs import (OptimizationError, OptimizationProblemFull, OptimizationProblemSingle, SolveInfo, kkt_certificate,
                                reference_qp)
from .deformation_transfer import (DeformationTransfer, MeshTopologyError, NoAnchorError, NotConvergedError, TransferError, register, transfer,
                                   transfer_blendshapes, triangle_correspondence)

__all__ = ["OptimizationError", "OptimizationProblemFull", "OptimizationProblemSingle", "SolveInfo", "kkt_certificate", "reference_qp",
           "DeformationTransfer", "MeshTopologyError", "NoAnchorError", "NotConvergedError", "TransferError", "register", "transfer",
           "transfer_blendshapes", "triangle_correspondence"]
