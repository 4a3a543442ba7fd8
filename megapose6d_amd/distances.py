"""Point-set distances between two poses, on device tensors (the reference's src/megapose/lib3d/distances.py:26-53).

Same signatures and return shapes; each is one launch of the fused kernels in csrc/pose_error.hip (no [B,S,N,3] or [B,N,N,3] tensor
is ever built).  `points` is per row, [B,N,3], as in the reference.
"""
from __future__ import annotations

import torch

from . import engine as eng


def dists_add(TXO_pred: torch.Tensor, TXO_gt: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """[B,N,3]: T_gt p - T_pred p"""
    out = eng.pose_error_sym(TXO_pred, TXO_gt.unsqueeze(1), None, None, points, with_errs=False, with_diffs=True)
    return out["diffs"]


def dists_add_symmetries(TXO_pred: torch.Tensor, TXO_gt_possible: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """[B,N,3]: T_gt_s p - T_pred p for the candidate s of TXO_gt_possible [B,S,4,4] with the smallest mean norm (lowest s on a tie)"""
    out = eng.pose_error_sym(TXO_pred, TXO_gt_possible, None, None, points, with_errs=False, with_diffs=True)
    return out["diffs"]


def dists_add_symmetric(TXO_pred: torch.Tensor, TXO_gt: torch.Tensor, points: torch.Tensor, return_assign: bool = False):
    """[B,N,3]: T_gt p_j - T_pred p_assign[j], assign[j] = the predicted point nearest to ground-truth point j (lowest index on a tie);
    with return_assign also the assignment [B,N] (int64)."""
    out = eng.pose_error_nn(TXO_pred, TXO_gt, points, with_diffs=True, with_assign=return_assign)
    if return_assign:
        return out["diffs"], out["assign"].long()
    return out["diffs"]
