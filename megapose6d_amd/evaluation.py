"""Pose errors between two pose tables and a mesh database, on the device.

The arithmetic of the reference's evaluation side -- src/megapose/evaluation/utils.py:50-66 (compute_pose_error), :69-154
(compute_errors), :175-238 (mssd_torch) and evaluation/meters/modelnet_meters.py:46-103 (ADD, 2D projection error, 5 deg / 5 cm) --
as launches of csrc/pose_error.hip -- and the three pose errors of the BOP challenge 2019, whose recalls average to the "BOP score"
the reference's tables report: VSD (csrc/vsd.hip, on depth renders of `Panda3dBatchRenderer.render_depth`), MSSD and MSPD
(`bop_errors`, `bop_recall`).  Dataset readers, BOP result-file formats, the xarray meters and plots are NOT here.

Where this departs from the reference, on purpose:
  * symmetric objects are evaluated on ALL their model points, not on the seven stand-in points of `create_default_object_pts`
    (the reference's [B,S,N,3] formulation does not fit otherwise; the fused kernel stores no pair);
  * the symmetry sets are `RigidObject.make_symmetry_poses` as batched by `MeshDataBase.batched(n_sym)` (`bop_toolkit_lib` is absent);
  * `mssd(..., reduce="max")` is the BOP definition the reference's docstring cites; `reduce="mean"` is what `mssd_torch` computes;
  * the rotation error is the angle of R2 R1^T by atan2, not the norm of a rotation vector recovered through acos;
  * VSD compares this engine's depth renders (one sample at each pixel centre, the rasteriser's fill rule), not `bop_toolkit`'s
    renderer (absent): pixels on a silhouette edge are unpinned against the toolkit.  Only BOP 2019's form is built (visibility
    "bop19", step cost).
"""
from __future__ import annotations

import re
from typing import Dict, Optional, Sequence

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


# --------------------------------------------------------------------------------------------------------------------------------
# BOP 2019 errors: VSD, MSSD, MSPD
# --------------------------------------------------------------------------------------------------------------------------------
BOP_TAUS = eng.VSD_TAUS                     # VSD misalignment tolerances, fractions of the diameter
BOP_THRESHOLDS = eng.VSD_TAUS               # thresholds of correctness of the VSD error and of MSSD / diameter
BOP_DEPTH_BYTES = 256 << 20                 # bytes of estimate depth maps `bop_errors` holds at once


def mspd(T_est: torch.Tensor, T_gt: torch.Tensor, pts: torch.Tensor, syms: torch.Tensor, K: torch.Tensor) -> Dict[str, torch.Tensor]:
    """BOP's MSPD in pixels.  T_est, T_gt [B,4,4]; pts [N,3]; syms [S,4,4]; K [B,3,3] (or [3,3]) -> the dict `mssd` returns."""
    b = T_est.shape[0]
    ids = torch.zeros(b, dtype=torch.int32, device=T_est.device)
    if K.dim() == 2:
        K = K.unsqueeze(0).expand(b, 3, 3)
    out = eng.pose_error_mspd(T_est, T_gt, syms.unsqueeze(0), None, pts.unsqueeze(0), K.to(torch.float32).contiguous(), mesh_ids=ids)
    idx = out["idx"].long()
    sym = syms.to(torch.float32)[idx.clamp(min=0)]
    return {"errs": out["errs"], "err": out["err"], "sym": sym, "T_gt_sym": out["T_gt_sym"], "idx": idx}


def _check_bop19(cost_type: str, visib_mode: str) -> None:
    if cost_type != "step":
        raise ValueError(f"cost_type {cost_type!r} is not built (only BOP 2019's 'step')")
    if visib_mode != "bop19":
        raise ValueError(f"visib_mode {visib_mode!r} is not built (only 'bop19')")


def vsd(depth_est: torch.Tensor, depth_gt: torch.Tensor, depth_test: torch.Tensor, K: torch.Tensor, diameter: torch.Tensor,
        delta: float = 0.015, taus: Optional[Sequence[float]] = None, normalized_by_diameter: bool = True,
        est_ids: Optional[torch.Tensor] = None, gt_ids: Optional[torch.Tensor] = None, im_ids: Optional[torch.Tensor] = None,
        cost_type: str = "step", visib_mode: str = "bop19") -> Dict[str, torch.Tensor]:
    """BOP 2019 VSD of rendered depth maps under observed frames, all [n,h,w] in metres (0 = nothing).  Row i compares
    depth_est[est_ids[i]] with depth_gt[gt_ids[i]] under depth_test[im_ids[i]] (ids None: map i); K [b,3,3], diameter [b]
    -> errs [b,n_tau] (taus default 0.05 ... 0.50), counts [b,2+n_tau] int32 = n_union, n_inter, n_far_t.  A non-finite K or a
    diameter that is not positive and finite gives NaN and -1."""
    _check_bop19(cost_type, visib_mode)
    dev = depth_est.device
    i32 = lambda t: None if t is None else torch.as_tensor(t, device=dev).to(torch.int32).contiguous()  # noqa: E731
    return eng.vsd(depth_est, depth_gt, depth_test, K.to(dev), torch.as_tensor(diameter, dtype=torch.float32, device=dev), delta=delta, taus=taus,
                   normalized_by_diameter=normalized_by_diameter, est_ids=i32(est_ids), gt_ids=i32(gt_ids), im_ids=i32(im_ids))


def _vsd_names(taus) -> list:
    return [f"vsd_{t:.2f}" for t in taus]


def bop_errors(pred, gt, meshes, renderer, depth: torch.Tensor, K: torch.Tensor, gt_index=None, delta: float = 0.015,
               taus: Optional[Sequence[float]] = None) -> pd.DataFrame:
    """The three BOP 2019 errors of `pred.poses` -> a DataFrame aligned with `pred.infos`: vsd_0.05 ... vsd_0.50 (one per tau), mssd
    (metres, over the symmetry set, all model points), mspd (pixels), sym_id_mssd, sym_id_mspd, diameter.
      renderer  a Panda3dBatchRenderer of the same objects (its `render_depth`: one sample at each pixel centre)
      depth     [n_im,H,W] observed frames in metres, K [n_im,3,3]; both indexed by `pred.infos.batch_im_id`
      gt_index  row of `gt` each prediction is measured against (default: row-aligned)
    Every distinct ground-truth row is rendered once, whatever the number of estimates that share it; estimates are rendered
    BOP_DEPTH_BYTES (256 MiB) of depth maps at a time (ground-truth renders in launches of the same size).  A row with a non-finite
    pose gives NaN in every error column.  One synchronising copy at the end."""
    dev = meshes.points.device
    taus = [float(t) for t in (BOP_TAUS if taus is None else taus)]
    n = len(pred.infos)
    labels = list(pred.infos["label"])
    gt_index = np.arange(n) if gt_index is None else np.asarray(gt_index, dtype=np.int64)
    if gt_index.shape != (n,) or (n and (gt_index.min() < 0 or gt_index.max() >= len(gt.infos))):
        raise ValueError("gt_index must name one row of `gt` per prediction")
    im = pred.infos["batch_im_id"].to_numpy().astype(np.int64)
    depth = depth.to(device=dev, dtype=torch.float32).contiguous()
    K = K.to(device=dev, dtype=torch.float32)
    if depth.dim() != 3 or K.shape != (depth.shape[0], 3, 3) or (n and (im.min() < 0 or im.max() >= depth.shape[0])):
        raise ValueError("depth must be [n_im,H,W], K [n_im,3,3], and batch_im_id must index them")
    H, W = int(depth.shape[1]), int(depth.shape[2])
    im_t = torch.from_numpy(im).to(dev)
    T_pred = pred.poses.to(device=dev, dtype=torch.float32).contiguous()
    T_gt = gt.poses.to(device=dev, dtype=torch.float32)[torch.from_numpy(gt_index).to(dev)].contiguous()
    K_rows = K[im_t].contiguous()
    ids, n_points, n_sym = _mesh_tables(meshes, labels, dev)
    e3 = eng.pose_error_sym(T_pred, T_gt, meshes.symmetries, n_sym, meshes.points, mesh_ids=ids, n_points=n_points, reduce=eng.POSE_ERROR_MAX,
                            with_errs=False)
    e2 = eng.pose_error_mspd(T_pred, T_gt, meshes.symmetries, n_sym, meshes.points, K_rows, mesh_ids=ids, n_points=n_points, with_errs=False)
    diam = _diameters(meshes)
    diam_rows = [diam[l] for l in labels]
    diam_t = torch.tensor(diam_rows, dtype=torch.float32, device=dev)
    # a non-finite pose is not handed to the rasteriser: a placeholder is rendered and the row's errors are set to NaN
    bad = ~(torch.isfinite(T_pred).flatten(1).all(1) & torch.isfinite(T_gt).flatten(1).all(1))
    place = torch.eye(4, device=dev)
    place[2, 3] = 1.0
    R_pred = torch.where(bad[:, None, None], place, T_pred)
    R_gt = torch.where(bad[:, None, None], place, T_gt)
    rows_per_launch = max(1, BOP_DEPTH_BYTES // (H * W * 4))
    uniq, first, inv = np.unique(gt_index, return_index=True, return_inverse=True)
    first_t = torch.from_numpy(first).to(dev)
    depth_gt = torch.empty(len(uniq), H, W, dtype=torch.float32, device=dev)
    for r0 in range(0, len(uniq), rows_per_launch):
        sel = first[r0:r0 + rows_per_launch]
        depth_gt[r0:r0 + len(sel)] = renderer.render_depth([labels[i] for i in sel], R_gt[first_t[r0:r0 + len(sel)]], K_rows[first_t[r0:r0 + len(sel)]], (H, W))
    inv_t = torch.from_numpy(inv.astype(np.int32)).to(dev)
    im32 = im_t.to(torch.int32)
    vsd_errs = torch.empty(n, len(taus), dtype=torch.float32, device=dev)
    for r0 in range(0, n, rows_per_launch):
        r1 = min(n, r0 + rows_per_launch)
        depth_est = renderer.render_depth(labels[r0:r1], R_pred[r0:r1], K_rows[r0:r1], (H, W))
        vsd_errs[r0:r1] = eng.vsd(depth_est, depth_gt, depth, K_rows[r0:r1].contiguous(), diam_t[r0:r1].contiguous(), delta=delta, taus=taus,
                                  gt_ids=inv_t[r0:r1].contiguous(), im_ids=im32[r0:r1].contiguous(), with_counts=False)["errs"]
    vsd_errs = torch.where(bad[:, None], torch.full_like(vsd_errs, float("nan")), vsd_errs)
    table = torch.cat([vsd_errs.double(), e3["err"].double()[:, None], e2["err"].double()[:, None], e3["idx"].double()[:, None],
                       e2["idx"].double()[:, None]], dim=1).cpu().numpy()   # the one synchronising copy
    names = _vsd_names(taus)
    df = pd.DataFrame({c: table[:, k] for k, c in enumerate(names + ["mssd", "mspd"])}, index=pred.infos.index)
    df["sym_id_mssd"] = table[:, -2].astype(np.int64)
    df["sym_id_mspd"] = table[:, -1].astype(np.int64)
    df["diameter"] = diam_rows
    return df


def bop_recall(df: pd.DataFrame, image_width: int = 640) -> Dict[str, float]:
    """BOP 2019 average recalls of the table of `bop_errors` (host arithmetic): ar_vsd = the share of (row, tau, theta) with vsd_tau <
    theta, ar_mssd = the share of (row, theta) with mssd < theta * diameter, both over theta = 0.05 ... 0.50; ar_mspd = the share of
    (row, theta) with mspd < theta * image_width / 640 over theta = 5 ... 50 px; ar = their mean.  NaN rows are misses."""
    thetas = np.asarray(BOP_THRESHOLDS, np.float64)
    cols = [c for c in df.columns if re.fullmatch(r"vsd_\d+\.\d+", c)]
    if not cols or len(df) == 0:
        raise ValueError("bop_recall needs a non-empty table with vsd_* columns")
    e_vsd = df[cols].to_numpy(np.float64)
    ar_vsd = float((e_vsd[:, :, None] < thetas[None, None, :]).mean())
    ar_mssd = float((df["mssd"].to_numpy(np.float64)[:, None] < thetas[None, :] * df["diameter"].to_numpy(np.float64)[:, None]).mean())
    thetas_px = np.arange(5, 51, 5).astype(np.float64) * (float(image_width) / 640.0)
    ar_mspd = float((df["mspd"].to_numpy(np.float64)[:, None] < thetas_px[None, :]).mean())
    return {"ar_vsd": ar_vsd, "ar_mssd": ar_mssd, "ar_mspd": ar_mspd, "ar": (ar_vsd + ar_mssd + ar_mspd) / 3.0}
