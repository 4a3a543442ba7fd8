"""Pose errors between two pose tables and a mesh database, on the device.

The arithmetic of the reference's evaluation side -- src/megapose/evaluation/utils.py:50-66 (compute_pose_error), :69-154
(compute_errors), :175-238 (mssd_torch) and evaluation/meters/modelnet_meters.py:46-103 (ADD, 2D projection error, 5 deg / 5 cm) --
as launches of csrc/pose_error.hip.  Dataset readers, BOP toolkit glue, the xarray meters and plots are NOT here.

Where this departs from the reference, on purpose:
  * symmetric objects are evaluated on ALL their model points, not on the seven stand-in points of `create_default_object_pts`
    (the reference's [B,S,N,3] formulation does not fit otherwise; the fused kernel stores no pair);
  * the symmetry sets are `RigidObject.make_symmetry_poses` as batched by `MeshDataBase.batched(n_sym)` (`bop_toolkit_lib` is absent);
  * `mssd(..., reduce="max")` is the BOP definition the reference's docstring cites; `reduce="mean"` is what `mssd_torch` computes;
  * the rotation error is the angle of R2 R1^T by atan2, not the norm of a rotation vector recovered through acos.
"""
from __future__ import annotations

import re
from typing import Dict, Optional

import numpy as np
import pandas as pd
import torch

from . import engine as eng

_REDUCE = {"mean": eng.POSE_ERROR_MEAN, "max": eng.POSE_ERROR_MAX}


def mssd(T_est: torch.Tensor, T_gt: torch.Tensor, pts: torch.Tensor, syms: torch.Tensor, reduce: str = "mean") -> Dict[str, torch.Tensor]:
    """evaluation/utils.py:175-238.  T_est, T_gt [B,4,4]; pts [N,3]; syms [S,4,4] -> errs [B,S], err [B], sym [B,4,4], T_gt_sym [B,4,4],
    idx [B] (int64; -1 and NaN errors for a non-finite pose)."""
    b = T_est.shape[0]
    dev = T_est.device
    ids = torch.zeros(b, dtype=torch.int32, device=dev)
    out = eng.pose_error_sym(T_est, T_gt, syms.unsqueeze(0), None, pts.unsqueeze(0), mesh_ids=ids, reduce=_REDUCE[reduce])
    idx = out["idx"].long()
    sym = syms.to(torch.float32)[idx.clamp(min=0)]
    return {"errs": out["errs"], "err": out["err"], "sym": sym, "T_gt_sym": out["T_gt_sym"], "idx": idx}


def compute_pose_error(T1: torch.Tensor, T2: torch.Tensor) -> Dict[str, torch.Tensor]:
    """evaluation/utils.py:50-66 -> trans_err, roterr_deg [B]"""
    out = eng.pose_error_rigid(T1, T2)
    return {"trans_err": out["trans_err"], "roterr_deg": out["rot_err_deg"]}


def _mesh_tables(meshes, labels, device):
    ids = torch.as_tensor(meshes.ids(list(labels)), dtype=torch.int32, device=device)
    n_points = torch.as_tensor([meshes.infos[l]["n_points"] for l in meshes.labels], dtype=torch.int32, device=device)
    n_sym = torch.as_tensor([meshes.infos[l]["n_sym"] for l in meshes.labels], dtype=torch.int32, device=device)
    return ids, n_points, n_sym


def _diameters(meshes) -> Dict[str, float]:
    cache = getattr(meshes, "_diameters", None)
    if cache is None:
        pts = meshes.points
        cache = {}
        for n, label in enumerate(meshes.labels):
            p = pts[n, : meshes.infos[label]["n_points"]]
            cache[label] = float(torch.linalg.norm((p.max(0)[0] - p.min(0)[0]).double()).item())   # modelnet_meters.py:72-73
        object.__setattr__(meshes, "_diameters", cache)
    return cache


def pose_errors(pred, gt, meshes, K: Optional[torch.Tensor] = None, nearest: bool = True) -> pd.DataFrame:
    """Errors of `pred.poses` against `gt.poses`, row by row (`pred.infos.label` names the object; `meshes` is a BatchedMeshes on the
    device) -> a DataFrame aligned with `pred.infos`:
      add (mean over ALL model points), add_sym (the minimum of that over the object's symmetry set), mssd (the same with max),
      adds (nearest neighbour; only with nearest=True), sym_id, trans_err / rot_err_deg (against the closest symmetric ground truth),
      proj_error (with K [B,3,3]), diameter."""
    dev = meshes.points.device
    T_pred, T_gt = pred.poses.to(dev), gt.poses.to(dev)
    labels = list(pred.infos["label"])
    ids, n_points, n_sym = _mesh_tables(meshes, labels, dev)
    sym = eng.pose_error_sym(T_pred, T_gt, meshes.symmetries, n_sym, meshes.points, mesh_ids=ids, n_points=n_points, with_alt=True)
    # symmetry 0 is the identity (make_symmetries_poses puts it first), so errs[:, 0] is the plain ADD
    cols = {"add": sym["errs"][:, 0], "add_sym": sym["err"], "mssd": sym["err_alt"]}
    if nearest:
        cols["adds"] = eng.pose_error_nn(T_pred, T_gt, meshes.points, mesh_ids=ids, n_points=n_points, with_diffs=False, with_assign=False)["mean"]
    rig = eng.pose_error_rigid(sym["T_gt_sym"], T_pred)
    cols["trans_err"], cols["rot_err_deg"] = rig["trans_err"], rig["rot_err_deg"]
    if K is not None:
        # the 2D error compares the prediction with the ground truth ITSELF (modelnet_meters.py:75-79)
        cols["proj_error"] = eng.pose_error_rigid(T_gt, T_pred, K=K.to(dev), points=meshes.points, mesh_ids=ids, n_points=n_points)["proj_error"]
    names = list(cols)
    table = torch.stack([cols[n].double() for n in names] + [sym["idx"].double()], dim=1).cpu().numpy()   # the one synchronising copy
    df = pd.DataFrame({n: table[:, k] for k, n in enumerate(names)}, index=pred.infos.index)
    df.insert(names.index("trans_err"), "sym_id", table[:, -1].astype(np.int64))
    diam = _diameters(meshes)
    df["diameter"] = [diam[l] for l in labels]
    return df


def compute_errors(preds: Dict[str, object], method: str, meshes) -> Dict[str, object]:
    """evaluation/utils.py:69-154 on the dict PredictionRunner.get_predictions returns (keys prefixed by `method`): adds `trans_err` /
    `rot_err_deg` to the infos of `{method}/refiner/init` and `{method}/refiner/iteration=N`, measured against the symmetric ground
    truth closest to each prediction (`{method}/ground_truth`, row-aligned), then `trans_err_init` / `rot_err_deg_init` on the iteration
    tables.  One pass per table over all objects at once."""
    gt = preds[f"{method}/ground_truth"]
    for key, p in preds.items():
        if not key.startswith(method):
            continue
        if not (re.search(r"refiner/iteration=\d*$", key) or re.search(r"refiner/init$", key)):
            continue
        df = pose_errors(p, gt, meshes, nearest=False)
        p.infos["trans_err"] = df["trans_err"].to_numpy()
        p.infos["rot_err_deg"] = df["rot_err_deg"].to_numpy()
    p_init = preds[f"{method}/refiner/init"]
    for key, p in preds.items():
        if key.startswith(method) and re.search(r"refiner/iteration=\d*$", key):
            p.infos["trans_err_init"] = p_init.infos["trans_err"]
            p.infos["rot_err_deg_init"] = p_init.infos["rot_err_deg"]
    return preds


def summary(df: pd.DataFrame) -> Dict[str, float]:
    """modelnet_meters.py:89-103 on the table of `pose_errors` (proj2d_5px only when `proj_error` is there)."""
    out = {"add0.1d": float((df["add"].to_numpy() < 0.1 * df["diameter"].to_numpy()).mean()),
           "5deg_5cm": float(np.logical_and(df["trans_err"].to_numpy() < 0.05, df["rot_err_deg"].to_numpy() < 5).mean())}
    if "proj_error" in df:
        out["proj2d_5px"] = float((df["proj_error"].to_numpy() < 5).mean())
    return out
