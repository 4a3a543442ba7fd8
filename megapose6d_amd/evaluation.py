"""Pose errors between two pose tables and a mesh database, on the device.

The arithmetic of the reference's evaluation side -- src/megapose/evaluation/utils.py:50-66 (compute_pose_error), :69-154
(compute_errors), :175-238 (mssd_torch) and evaluation/meters/modelnet_meters.py:46-103 (ADD, 2D projection error, 5 deg / 5 cm) --
as launches of csrc/pose_error.hip -- and the three pose errors of the BOP challenge 2019, whose recalls average to the "BOP score"
the reference's tables report: VSD (csrc/vsd.hip, on depth renders of `Panda3dBatchRenderer.render_depth`), MSSD and MSPD
(`bop_errors`, `bop_recall`) -- and the annotation BOP calls gt info (csrc/gt_info.hip: visibility fraction, masks, modal and
amodal boxes; `gt_info`, `detections_from_gt_info`), which the reference reads from a BOP dataset's files -- and the step that joins
detections that carry scores to ground-truth instances, BOP's greedy matching (csrc/bop_match.hip; evaluation/meters/utils.py:51-152
get_top_n_ids, add_valid_gt, get_candidate_matches, match_poses): `bop_candidates`, `bop_candidate_errors`, `bop_match`, `bop_scores`.
-- and the scores of BOP's 2D detection and 2D segmentation tasks, COCO average precision of scored boxes and masks against `gt_info`'s
modal boxes and visible masks (csrc/det_ap.hip: the pixel counts of mask pairs, COCO's greedy matching; the reference has no such meter):
`mask_iou`, `box_iou`, `coco_match`, `coco_accumulate`, `bop_detection_scores`.
-- and BOP's model info (csrc/model_info.hip: the exact diameter, the largest distance between two model points, and the bounds;
bop_toolkit's calc_model_info): `model_info`, `bop_models_info`, `save_models_info`, `load_models_info`, and the `diameters=` keyword
that scales every threshold by it instead of the default box diagonal.
-- and the symmetries all of the above minimise over, found from the mesh alone (csrc/symmetry.hip decides which candidate rotations map
the surface into itself): `find_symmetries`, `symmetry_poses`, and the `symmetries=` keyword of `bop_models_info` / `save_models_info`.
Dataset readers, BOP result-file formats, the xarray meters and plots are NOT here.

Where this departs from the reference, on purpose:
  * symmetric objects are evaluated on ALL their model points, not on the seven stand-in points of `create_default_object_pts`
    (the reference's [B,S,N,3] formulation does not fit otherwise; the fused kernel stores no pair);
  * the symmetry sets are `RigidObject.make_symmetry_poses` as batched by `MeshDataBase.batched(n_sym)` (`bop_toolkit_lib` is absent);
  * `mssd(..., reduce="max")` is the BOP definition the reference's docstring cites; `reduce="mean"` is what `mssd_torch` computes;
  * the rotation error is the angle of R2 R1^T by atan2, not the norm of a rotation vector recovered through acos;
  * VSD compares this engine's depth renders (one sample at each pixel centre, the rasteriser's fill rule), not `bop_toolkit`'s
    renderer (absent): pixels on a silhouette edge are unpinned against the toolkit.  Only BOP 2019's form is built (visibility
    "bop19", step cost);
  * `gt_info` blanks each box only when its own mask is empty; `bop_toolkit` (absent, so unpinned) blanks both boxes when nothing is
    visible.  Its silhouette pixels are this engine's fill rule, as for VSD.
  * the detection scores are unpinned against `pycocotools` and `bop_toolkit` (both absent); a ground truth's `ignore` flag is the
    caller's (stock `pycocotools` overwrites it with `iscrowd`), and a NaN IoU never matches.
  * the default diameter is the diagonal of the bounding box (the reference's ModelNet meter), which is never smaller than BOP's;
    `diameters="exact"` or a models_info.json gives BOP's.  `model_info` is unpinned against `bop_toolkit` (absent).
  * `find_symmetries` has no counterpart in the reference (BOP's symmetries are annotated by hand): rotations only, candidates from
    vertex anchors, so a scanned mesh with only approximate symmetry can be missed; unpinned against BOP's own annotations.
"""
from __future__ import annotations

import re
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import pandas as pd
import torch

from . import engine as eng
from .tcoll import PandasTensorCollection

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


def resolve_diameters(meshes, diameters, labels) -> Dict[str, float]:
    """The `diameters=` keyword of `pose_errors`, `bop_errors`, `bop_candidate_errors` and `bop_scores` -> {label: metres} covering
    `labels`.  None: the diagonal of the axis-aligned bounding box (modelnet_meters.py:72-73, the default); "exact": BOP's diameter,
    the largest distance between two model points (`model_info(meshes)`, computed once and kept on `meshes`); a mapping label ->
    metres, e.g. from `load_models_info`: a label of `labels` it lacks raises KeyError, a value that is not positive and finite
    ValueError."""
    if diameters is None:
        return _diameters(meshes)
    if isinstance(diameters, str):
        if diameters != "exact":
            raise ValueError(f"diameters {diameters!r} is not None, 'exact' or a mapping from label to metres")
        info = getattr(meshes, "_model_info", None)
        if info is None:
            info = model_info(meshes)
            object.__setattr__(meshes, "_model_info", info)
        diameters = info["diameter"].to_dict()
    out = {}
    for label in dict.fromkeys(labels):
        d = float(diameters[label])            # KeyError for a label the mapping lacks
        if not (np.isfinite(d) and d > 0.0):
            raise ValueError(f"the diameter of {label!r} is {d}: it must be positive and finite")
        out[label] = d
    return out


def pose_errors(pred, gt, meshes, K: Optional[torch.Tensor] = None, nearest: bool = True, diameters=None) -> pd.DataFrame:
    """Errors of `pred.poses` against `gt.poses`, row by row (`pred.infos.label` names the object; `meshes` is a BatchedMeshes on the
    device) -> a DataFrame aligned with `pred.infos`:
      add (mean over ALL model points), add_sym (the minimum of that over the object's symmetry set), mssd (the same with max),
      adds (nearest neighbour; only with nearest=True), sym_id, trans_err / rot_err_deg (against the closest symmetric ground truth),
      proj_error (with K [B,3,3]), diameter (of `diameters`: None the box diagonal, "exact" BOP's, or a mapping; `resolve_diameters`)."""
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
    diam = resolve_diameters(meshes, diameters, labels)
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
BOP_THETAS_PX = tuple(range(5, 51, 5))      # thresholds of correctness of MSPD, pixels at an image width of 640
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


def _bop_frames(depth: torch.Tensor, K: torch.Tensor, im: np.ndarray, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """the observed frames and their intrinsics on the device, checked against the rows' batch_im_id"""
    depth = depth.to(device=dev, dtype=torch.float32).contiguous()
    K = K.to(device=dev, dtype=torch.float32)
    if depth.dim() != 3 or K.shape != (depth.shape[0], 3, 3) or (len(im) and (im.min() < 0 or im.max() >= depth.shape[0])):
        raise ValueError("depth must be [n_im,H,W], K [n_im,3,3], and batch_im_id must index them")
    return depth, K


def _placeholder_pose(dev) -> torch.Tensor:
    """what is rendered in the place of a non-finite pose: the object one metre down the optical axis"""
    place = torch.eye(4, device=dev)
    place[2, 3] = 1.0
    return place


def _thetas_px(image_width) -> np.ndarray:
    return np.asarray(BOP_THETAS_PX, np.float64) * (float(image_width) / 640.0)


def _valid_mask(valid, index, n: int, what: str = "the ground truth") -> np.ndarray:
    if valid is None:
        return np.ones(n, np.bool_)
    valid = valid.reindex(index).to_numpy() if isinstance(valid, pd.Series) else np.asarray(valid)
    if valid.dtype != np.bool_ or valid.shape != (n,):
        raise ValueError(f"valid must be one boolean per row of {what}")
    return valid


def _bop_pair_errors(pred, gt, pid: np.ndarray, gid: np.ndarray, gt_labels, gt_im: np.ndarray, meshes, renderer, depth: torch.Tensor,
                     K: torch.Tensor, delta: float, taus, gt_blank_with: Optional[np.ndarray] = None, diameters=None):
    """The three BOP 2019 errors of the pairs (estimate pid[i] of `pred`, ground truth gid[i] of `gt`), int64 arrays [n]; the object and the
    frame of a pair are those of its estimate; depth, K as `_bop_frames` returns them.  Every distinct estimate is rendered once under its
    own label and frame, BOP_DEPTH_BYTES of depth maps at a time; the j-th distinct ground truth (in the order of np.unique(gid)) once
    under the label gt_labels[j] and the K of frame gt_im[j], in launches of the same size.  A non-finite pose is not handed to the
    rasteriser (a placeholder is rendered) and gives NaN on its pairs; with gt_blank_with (one pair per distinct ground truth) the
    placeholder also stands for a ground truth whose named pair has a non-finite estimate.  diameters as `resolve_diameters` takes it
    (the VSD tolerance is tau * diameter).
    -> vsd [n,n_tau] float32, the dicts of pose_error_sym (MSSD) and pose_error_mspd.  Nothing synchronises."""
    dev = meshes.points.device
    n = len(pid)
    H, W = int(depth.shape[1]), int(depth.shape[2])
    labels_pred = list(pred.infos["label"])
    im_pred = pred.infos["batch_im_id"].to_numpy().astype(np.int64)
    T_pred = pred.poses.to(device=dev, dtype=torch.float32).contiguous()
    T_gt = gt.poses.to(device=dev, dtype=torch.float32).contiguous()
    pid_t, gid_t = torch.from_numpy(pid).to(dev), torch.from_numpy(gid).to(dev)
    labels = [labels_pred[i] for i in pid]
    im32 = torch.from_numpy(im_pred[pid].astype(np.int32)).to(dev)
    K_rows = K[im32.long()].contiguous()
    ids, n_points, n_sym = _mesh_tables(meshes, labels, dev)
    Tp, Tg = T_pred[pid_t].contiguous(), T_gt[gid_t].contiguous()
    e3 = eng.pose_error_sym(Tp, Tg, meshes.symmetries, n_sym, meshes.points, mesh_ids=ids, n_points=n_points, reduce=eng.POSE_ERROR_MAX,
                            with_errs=False)
    e2 = eng.pose_error_mspd(Tp, Tg, meshes.symmetries, n_sym, meshes.points, K_rows, mesh_ids=ids, n_points=n_points, with_errs=False)
    diam = resolve_diameters(meshes, diameters, labels)
    diam_t = torch.tensor([diam[l] for l in labels], dtype=torch.float32, device=dev)
    bad_pred, bad_gt = ~torch.isfinite(T_pred).flatten(1).all(1), ~torch.isfinite(T_gt).flatten(1).all(1)
    rows_per_launch = max(1, BOP_DEPTH_BYTES // (H * W * 4))
    u_gt, inv_gt = np.unique(gid, return_inverse=True)
    u_pred, inv_pred = np.unique(pid, return_inverse=True)
    u_gt_t, u_pred_t = torch.from_numpy(u_gt).to(dev), torch.from_numpy(u_pred).to(dev)
    blank_gt = bad_gt[u_gt_t]
    if gt_blank_with is not None:
        blank_gt = blank_gt | bad_pred[pid_t[torch.from_numpy(gt_blank_with).to(dev)]]
    place = _placeholder_pose(dev)
    R_pred = torch.where(bad_pred[u_pred_t, None, None], place, T_pred[u_pred_t])
    R_gt = torch.where(blank_gt[:, None, None], place, T_gt[u_gt_t])
    K_gt = K[torch.from_numpy(np.asarray(gt_im, np.int64)).to(dev)]
    K_pred = K[torch.from_numpy(im_pred[u_pred]).to(dev)]
    depth_gt = torch.empty(len(u_gt), H, W, dtype=torch.float32, device=dev)
    for r0 in range(0, len(u_gt), rows_per_launch):
        r1 = min(len(u_gt), r0 + rows_per_launch)
        depth_gt[r0:r1] = renderer.render_depth(list(gt_labels[r0:r1]), R_gt[r0:r1], K_gt[r0:r1], (H, W))
    # pairs in the order of their estimate, so that a portion of estimates is a run of pairs
    order = np.argsort(inv_pred, kind="stable")
    est_sorted = inv_pred[order]
    gt_ids = torch.from_numpy(inv_gt.astype(np.int32)).to(dev)
    est_ids = torch.from_numpy(inv_pred.astype(np.int32)).to(dev)
    order_t = torch.from_numpy(order).to(dev)
    vsd_errs = torch.empty(n, len(taus), dtype=torch.float32, device=dev)
    for r0 in range(0, len(u_pred), rows_per_launch):
        r1 = min(len(u_pred), r0 + rows_per_launch)
        depth_est = renderer.render_depth([labels_pred[i] for i in u_pred[r0:r1]], R_pred[r0:r1], K_pred[r0:r1], (H, W))
        rows = order_t[int(np.searchsorted(est_sorted, r0)):int(np.searchsorted(est_sorted, r1))]
        vsd_errs[rows] = eng.vsd(depth_est, depth_gt, depth, K_rows[rows].contiguous(), diam_t[rows].contiguous(), delta=delta, taus=taus,
                                 est_ids=(est_ids[rows] - r0).contiguous(), gt_ids=gt_ids[rows].contiguous(), im_ids=im32[rows].contiguous(),
                                 with_counts=False)["errs"]
    bad = bad_pred[pid_t] | bad_gt[gid_t]
    vsd_errs = torch.where(bad[:, None], torch.full_like(vsd_errs, float("nan")), vsd_errs)
    return vsd_errs, e3, e2


def bop_errors(pred, gt, meshes, renderer, depth: torch.Tensor, K: torch.Tensor, gt_index=None, delta: float = 0.015,
               taus: Optional[Sequence[float]] = None, diameters=None) -> pd.DataFrame:
    """The three BOP 2019 errors of `pred.poses` -> a DataFrame aligned with `pred.infos`: vsd_0.05 ... vsd_0.50 (one per tau), mssd
    (metres, over the symmetry set, all model points), mspd (pixels), sym_id_mssd, sym_id_mspd, diameter.
      renderer  a Panda3dBatchRenderer of the same objects (its `render_depth`: one sample at each pixel centre)
      depth     [n_im,H,W] observed frames in metres, K [n_im,3,3]; both indexed by `pred.infos.batch_im_id`
      gt_index  row of `gt` each prediction is measured against (default: row-aligned)
      diameters None (the box diagonal), "exact" (BOP's diameter) or a mapping label -> metres (`resolve_diameters`): the VSD tolerance
                tau * diameter and the `diameter` column
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
    depth, K = _bop_frames(depth, K, im, dev)
    # a ground truth is rendered as the first estimate that names it sees it: under that estimate's label and K
    first = np.unique(gt_index, return_index=True)[1]
    vsd_errs, e3, e2 = _bop_pair_errors(pred, gt, np.arange(n, dtype=np.int64), gt_index, [labels[i] for i in first], im[first], meshes,
                                           renderer, depth, K, delta, taus, gt_blank_with=first, diameters=diameters)
    table = torch.cat([vsd_errs.double(), e3["err"].double()[:, None], e2["err"].double()[:, None], e3["idx"].double()[:, None],
                       e2["idx"].double()[:, None]], dim=1).cpu().numpy()   # the one synchronising copy
    names = _vsd_names(taus)
    df = pd.DataFrame({c: table[:, k] for k, c in enumerate(names + ["mssd", "mspd"])}, index=pred.infos.index)
    df["sym_id_mssd"] = table[:, -2].astype(np.int64)
    df["sym_id_mspd"] = table[:, -1].astype(np.int64)
    diam = resolve_diameters(meshes, diameters, labels)
    df["diameter"] = [diam[l] for l in labels]
    return df


def bop_recall(df: pd.DataFrame, image_width: int = 640, valid=None) -> Dict[str, float]:
    """BOP 2019 average recalls of the table of `bop_errors` (host arithmetic): ar_vsd = the share of (row, tau, theta) with vsd_tau <
    theta, ar_mssd = the share of (row, theta) with mssd < theta * diameter, both over theta = 0.05 ... 0.50; ar_mspd = the share of
    (row, theta) with mspd < theta * image_width / 640 over theta = 5 ... 50 px; ar = their mean.  NaN rows are misses.
      valid  optional boolean mask (array, or Series indexed like `df`) of the rows that are targets, e.g. `gt_info(...)["visib_fract"]
             >= 0.1` taken at each row's ground truth (evaluation/meters/utils.py:86-104); the recalls are those of `df[valid]`."""
    if valid is not None:
        df = df[_valid_mask(valid, df.index, len(df), "the table")]
    thetas = np.asarray(BOP_THRESHOLDS, np.float64)
    cols = [c for c in df.columns if re.fullmatch(r"vsd_\d+\.\d+", c)]
    if not cols or len(df) == 0:
        raise ValueError("bop_recall needs a non-empty table with vsd_* columns")
    e_vsd = df[cols].to_numpy(np.float64)
    ar_vsd = float((e_vsd[:, :, None] < thetas[None, None, :]).mean())
    ar_mssd = float((df["mssd"].to_numpy(np.float64)[:, None] < thetas[None, :] * df["diameter"].to_numpy(np.float64)[:, None]).mean())
    thetas_px = _thetas_px(image_width)
    ar_mspd = float((df["mspd"].to_numpy(np.float64)[:, None] < thetas_px[None, :]).mean())
    return {"ar_vsd": ar_vsd, "ar_mssd": ar_mssd, "ar_mspd": ar_mspd, "ar": (ar_vsd + ar_mssd + ar_mspd) / 3.0}


# --------------------------------------------------------------------------------------------------------------------------------
# BOP's ground-truth info: visibility, masks, boxes
# --------------------------------------------------------------------------------------------------------------------------------
GT_INFO_COUNTS = ("px_count_all", "px_count_image", "px_count_valid", "px_count_visib")


def tile_intrinsics(K: torch.Tensor, canvas: int, resolution) -> torch.Tensor:
    """K [n,3,3] -> [n,canvas*canvas,3,3]: the intrinsics of the canvas' tiles, row-major, cx' = cx - (tx - c) * w and cy' = cy - (ty - c)
    * h with c = (canvas - 1) / 2, one fp32 subtraction each (the shifts are integers: exact)."""
    if canvas not in (1, 3):
        raise ValueError(f"canvas {canvas} is not 1 or 3")
    h, w = resolution
    c = (canvas - 1) // 2
    t = torch.arange(canvas * canvas, device=K.device)
    Kt = K.to(torch.float32)[:, None].repeat(1, canvas * canvas, 1, 1)
    Kt[:, :, 0, 2] = Kt[:, :, 0, 2] - ((t % canvas - c) * w).to(torch.float32)[None]
    Kt[:, :, 1, 2] = Kt[:, :, 1, 2] - ((torch.div(t, canvas, rounding_mode="floor") - c) * h).to(torch.float32)[None]
    return Kt


def _bop_box(ext, count) -> list:
    """inclusive [xmin, ymin, xmax, ymax] -> BOP's [x, y, w, h] with w = xmax - xmin; [-1] * 4 over no pixel"""
    if count <= 0:
        return [-1, -1, -1, -1]
    return [int(ext[0]), int(ext[1]), int(ext[2] - ext[0]), int(ext[3] - ext[1])]


def gt_info_table(counts: np.ndarray, boxes: np.ndarray, visib_fract: np.ndarray, index=None) -> pd.DataFrame:
    """counts [n,4], boxes [n,8] (inclusive extents: obj, visib), visib_fract [n] of `engine.gt_info`, on the host -> the table of
    `gt_info`.  Whether a box is blank is read from its count (a one-pixel box at image pixel (-1, -1) has the blank's numbers)."""
    counts, boxes = np.asarray(counts).astype(np.int64), np.asarray(boxes).astype(np.int64)
    df = pd.DataFrame({name: counts[:, k] for k, name in enumerate(GT_INFO_COUNTS)}, index=index)
    df["visib_fract"] = np.asarray(visib_fract, np.float64)
    n_obj, n_vis = counts[:, 0], counts[:, 3]
    amodal = [[int(v) for v in boxes[i, :4]] if n_obj[i] > 0 else [-1] * 4 for i in range(len(counts))]
    modal = [[int(v) for v in boxes[i, 4:]] if n_vis[i] > 0 else [-1] * 4 for i in range(len(counts))]
    df["bbox_obj"] = [_bop_box(boxes[i, :4], n_obj[i]) for i in range(len(counts))]
    df["bbox_visib"] = [_bop_box(boxes[i, 4:], n_vis[i]) for i in range(len(counts))]
    df["bbox_amodal"] = amodal
    df["bbox_modal"] = modal
    return df


def gt_info(gt, renderer, depth: torch.Tensor, K: torch.Tensor, delta: float = 0.015, canvas: int = 3, return_masks: bool = False):
    """BOP's gt info of the objects of `gt` (`infos` with `label` and `batch_im_id`, `poses`) -> a DataFrame aligned with `gt.infos`:
      px_count_all    pixels of the object's silhouette on a canvas of canvas x canvas images around the image (BOP renders on 3 x 3, so
                      that the part outside the frame counts and visib_fract accounts for truncation)
      px_count_image  of those, the pixels inside the image; px_count_valid  of those, the pixels with an observed depth
      px_count_visib  pixels where the object is visible under the observed depth (the "bop19" rule of VSD, tolerance delta)
      visib_fract     px_count_visib / px_count_all (0 for an object off the canvas)
      bbox_obj, bbox_visib      BOP's [x, y, w, h] with w = xmax - xmin of the whole silhouette (x, y can be negative) / of the visible part
      bbox_amodal, bbox_modal   the same boxes as the reference's ObjectData holds them, [xmin, ymin, xmax, ymax]
                                (datasets/bop_scene_dataset.py:238-262)
    A box over no pixel is [-1, -1, -1, -1].  With return_masks also (mask, mask_visib), two [n,H,W] uint8 tensors (0 / 255, BOP's PNG
    format) that stay on the device.
      renderer  a Panda3dBatchRenderer of the same objects (its `render_depth`: one sample at each pixel centre)
      depth     [n_im,H,W] observed frames in metres, K [n_im,3,3]; both indexed by `gt.infos.batch_im_id`.  `depth` may just as well be
                the depth of a `Panda3dSceneRenderer.render_scenes` call: then the occluders are the other objects of a synthetic scene.
    Every row's canvas*canvas tiles are rendered, BOP_DEPTH_BYTES (256 MiB) of depth maps at a time.  A row with a non-finite pose is not
    handed to the rasteriser (a placeholder is rendered) and gives counts and boxes of -1 and NaN, as does a non-finite K.  One
    synchronising copy at the end.
    Known deviation: each box is blank only when its own mask is empty; `bop_toolkit` (absent here, so this is unpinned against it)
    blanks both boxes when nothing is visible.  Silhouette pixels are this engine's fill rule."""
    n = len(gt.infos)
    labels = list(gt.infos["label"])
    im = gt.infos["batch_im_id"].to_numpy().astype(np.int64)
    dev = depth.device if depth.is_cuda else torch.device("cuda")
    depth, K = _bop_frames(depth, K, im, dev)
    H, W = int(depth.shape[1]), int(depth.shape[2])
    n_tiles = canvas * canvas
    im_t = torch.from_numpy(im).to(dev)
    T = gt.poses.to(device=dev, dtype=torch.float32)
    K_rows = K[im_t].contiguous()
    # a non-finite pose or K is not handed to the rasteriser: a placeholder is rendered and the row's results are set to -1 / NaN
    bad = ~(torch.isfinite(T).flatten(1).all(1) & torch.isfinite(K_rows).flatten(1).all(1))
    place = _placeholder_pose(dev)
    K_place = torch.tensor([[float(W), 0.0, 0.5 * W], [0.0, float(W), 0.5 * H], [0.0, 0.0, 1.0]], device=dev)
    R = torch.where(bad[:, None, None], place, T)
    K_tiles = tile_intrinsics(torch.where(bad[:, None, None], K_place, K_rows), canvas, (H, W))
    im32 = im_t.to(torch.int32)
    counts = torch.empty(n, 4, dtype=torch.int32, device=dev)
    boxes = torch.empty(n, 8, dtype=torch.int32, device=dev)
    fract = torch.empty(n, dtype=torch.float32, device=dev)
    masks = [torch.empty(n, H, W, dtype=torch.uint8, device=dev) for _ in range(2)] if return_masks else None
    rows_per_launch = max(1, BOP_DEPTH_BYTES // (H * W * 4 * n_tiles))
    for r0 in range(0, n, rows_per_launch):
        r1 = min(n, r0 + rows_per_launch)
        tiles = renderer.render_depth([l for l in labels[r0:r1] for _ in range(n_tiles)], R[r0:r1].repeat_interleave(n_tiles, dim=0),
                                      K_tiles[r0:r1].flatten(0, 1), (H, W)).view(r1 - r0, n_tiles, H, W)
        out = eng.gt_info(tiles, depth, K_rows[r0:r1].contiguous(), canvas=canvas, delta=delta, im_ids=im32[r0:r1].contiguous(),
                          with_masks=return_masks)
        counts[r0:r1], boxes[r0:r1], fract[r0:r1] = out["counts"], out["boxes"], out["visib_fract"]
        if return_masks:
            masks[0][r0:r1], masks[1][r0:r1] = out["mask"], out["mask_visib"]
    counts = torch.where(bad[:, None], torch.full_like(counts, -1), counts)
    boxes = torch.where(bad[:, None], torch.full_like(boxes, -1), boxes)
    fract = torch.where(bad, torch.full_like(fract, float("nan")), fract)
    table = torch.cat([counts.double(), boxes.double(), fract.double()[:, None]], dim=1).cpu().numpy()   # the one synchronising copy
    df = gt_info_table(table[:, :4], table[:, 4:12], table[:, 12], index=gt.infos.index)
    if not return_masks:
        return df
    for m in masks:
        m[bad] = 0
    return df, masks[0], masks[1]


def detections_from_gt_info(gt, info: pd.DataFrame, visib_gt_min: float = 0.0) -> PandasTensorCollection:
    """Ground-truth detections for the pose estimator (the counterpart of the reference's make_detections_from_object_data,
    inference/utils.py:214-225): infos `label`, `batch_im_id`, `instance_id` of the rows of `gt` that have a visible pixel and
    visib_fract >= visib_gt_min, `bboxes` [m,4] float32 = their bbox_modal.  `info` is the table of `gt_info`, row-aligned with
    `gt.infos`; `instance_id` is the one of `gt.infos` when it has one, else the row's position in `gt`."""
    if len(info) != len(gt.infos):
        raise ValueError("info must have one row per row of gt")
    keep = (info["px_count_visib"].to_numpy() > 0) & (info["visib_fract"].to_numpy() >= float(visib_gt_min))
    src = gt.infos.reset_index(drop=True)
    inst = src["instance_id"].to_numpy() if "instance_id" in src else np.arange(len(src))
    infos = pd.DataFrame(dict(label=src["label"].to_numpy()[keep], batch_im_id=src["batch_im_id"].to_numpy()[keep], instance_id=inst[keep]))
    rows = [b for b, k in zip(info["bbox_modal"], keep) if k]
    bboxes = torch.as_tensor(np.asarray(rows, np.float32).reshape(-1, 4))
    return PandasTensorCollection(infos=infos, bboxes=bboxes)


# --------------------------------------------------------------------------------------------------------------------------------
# BOP's matching of estimates to ground truths: candidates, their errors, the greedy matching, the scores
# --------------------------------------------------------------------------------------------------------------------------------
def bop_candidates(pred_infos: pd.DataFrame, gt_infos: pd.DataFrame, valid=None, keys=("batch_im_id", "label")) -> pd.DataFrame:
    """evaluation/meters/utils.py:107-117 get_candidate_matches(only_valids=True), on the host as a pandas merge -> a DataFrame
    `pred_id`, `gt_id`, `group_id` (int64; positions in the two tables) of every (estimate, ground truth) pair that agrees on `keys`
    and whose ground truth is valid.  Rows come in the order of `pred_infos`, then of `gt_infos`; a group is one value of `keys`,
    numbered in order of first appearance.
      valid  one boolean per row of `gt_infos` (array, or Series indexed like it): the targets, e.g. `gt_info(...)["visib_fract"] >= 0.1`
             (add_valid_gt, utils.py:86-104); default all."""
    keys = list(keys)
    valid = _valid_mask(valid, gt_infos.index, len(gt_infos))
    p = pred_infos[keys].reset_index(drop=True)
    p["pred_id"] = np.arange(len(p), dtype=np.int64)
    g = gt_infos[keys].reset_index(drop=True)
    g["gt_id"] = np.arange(len(g), dtype=np.int64)
    cand = p.merge(g[valid], on=keys, how="inner")
    group = cand.groupby(keys, sort=False).ngroup().to_numpy().astype(np.int64) if len(cand) else np.zeros(0, np.int64)
    return pd.DataFrame(dict(pred_id=cand["pred_id"].to_numpy().astype(np.int64), gt_id=cand["gt_id"].to_numpy().astype(np.int64), group_id=group))


def bop_candidate_errors(pred, gt, cand: pd.DataFrame, meshes, renderer, depth: torch.Tensor, K: torch.Tensor, delta: float = 0.015,
                         taus: Optional[Sequence[float]] = None, diameters=None) -> torch.Tensor:
    """The three BOP 2019 errors of every candidate of `cand` (`bop_candidates`): estimate `pred_id` of `pred` against ground truth
    `gt_id` of `gt` -> a device tensor [C, n_tau + 2] float32: VSD per tau, MSSD in metres, MSPD in pixels (the columns of
    `bop_errors`).  Arguments as `bop_errors`; the frame and the object of a candidate are those of its estimate.  Every distinct
    estimate and every distinct ground truth is rendered once, each under its own label and its own frame's K, estimates
    BOP_DEPTH_BYTES of depth maps at a time.  A non-finite pose gives NaN on its candidates (a placeholder is rendered).  Nothing
    synchronises."""
    dev = meshes.points.device
    taus = [float(t) for t in (BOP_TAUS if taus is None else taus)]
    pid, gid = cand["pred_id"].to_numpy().astype(np.int64), cand["gt_id"].to_numpy().astype(np.int64)
    n = len(pid)
    if n and (pid.min() < 0 or pid.max() >= len(pred.infos) or gid.min() < 0 or gid.max() >= len(gt.infos)):
        raise ValueError("cand must name rows of `pred` and of `gt`")
    labels_gt = list(gt.infos["label"])
    im_pred = pred.infos["batch_im_id"].to_numpy().astype(np.int64)
    im_gt = gt.infos["batch_im_id"].to_numpy().astype(np.int64)
    depth, K = _bop_frames(depth, K, np.concatenate([im_pred, im_gt]), dev)
    if n == 0:
        return torch.empty(0, len(taus) + 2, dtype=torch.float32, device=dev)
    u_gt = np.unique(gid)
    vsd_errs, e3, e2 = _bop_pair_errors(pred, gt, pid, gid, [labels_gt[i] for i in u_gt], im_gt[u_gt], meshes, renderer, depth, K, delta, taus,
                                        diameters=diameters)
    return torch.cat([vsd_errs, e3["err"][:, None], e2["err"][:, None]], dim=1)


def bop_match_index(pred_id, gt_id, group_id, scores, n_groups: Optional[int] = None) -> Dict[str, object]:
    """The index `engine.bop_match` takes (include/mp_engine.h), on the host: `order` [C] int64 = the candidates sorted by (group,
    decreasing score of their estimate, pred_id, gt_id), then the int32 arrays `engine.BOP_MATCH_INDEX` over that order and the int
    `n_taken_words`.  scores [P], finite.  An estimate or a ground truth in two groups is refused."""
    pid, gid, grp = (np.asarray(a).astype(np.int64) for a in (pred_id, gt_id, group_id))
    scores = np.asarray(scores, np.float64)
    if scores.ndim != 1 or not np.isfinite(scores).all():
        raise ValueError("scores must be one finite number per estimate")
    if not (pid.shape == gid.shape == grp.shape) or pid.ndim != 1:
        raise ValueError("pred_id, gt_id and group_id must be three arrays of one length")
    c = len(pid)
    if c and (pid.min() < 0 or pid.max() >= len(scores) or gid.min() < 0 or gid.max() >= 2 ** 31 - 1 or grp.min() < 0):
        raise ValueError("pred_id must index scores; gt_id and group_id must not be negative")
    n_groups = (int(grp.max()) + 1 if c else 0) if n_groups is None else int(n_groups)
    if c and grp.max() >= n_groups:
        raise ValueError(f"group_id reaches {int(grp.max())} with {n_groups} groups")
    order = np.lexsort((gid, pid, -scores[pid], grp))
    pid, gid, grp = pid[order], gid[order], grp[order]
    new_est = np.ones(c, np.bool_)
    new_est[1:] = (pid[1:] != pid[:-1]) | (grp[1:] != grp[:-1])
    est_first = np.flatnonzero(new_est)
    est_row, est_grp = pid[est_first], grp[est_first]
    # the ground truths of each group, numbered by ascending gt_id
    span = (int(gid.max()) + 1) if c else 1
    u_key, lgt = np.unique(grp * span + gid, return_inverse=True)
    u_grp = u_key // span
    n_gt = np.bincount(u_grp, minlength=n_groups)
    if len(np.unique(est_row)) != len(est_row) or len(np.unique(u_key % span)) != len(u_key):
        raise ValueError("an estimate or a ground truth belongs to more than one group")
    lgt = lgt - np.concatenate([[0], np.cumsum(n_gt)])[grp]
    words = np.concatenate([[0], np.cumsum((n_gt + 31) // 32)])
    if c >= 2 ** 31 - 1 or words[-1] >= 2 ** 31 - 1:
        raise ValueError("too many candidates for an int32 index")
    i32 = lambda a: np.ascontiguousarray(a, np.int32)   # noqa: E731
    return dict(order=order, cand_gt=i32(gid), cand_lgt=i32(lgt), est_row=i32(est_row), est_off=i32(np.append(est_first, c)),
                group_est_off=i32(np.searchsorted(est_grp, np.arange(n_groups + 1))), group_n_gt=i32(n_gt), group_taken_off=i32(words),
                n_taken_words=int(words[-1]))


def bop_match(cand: pd.DataFrame, errs: torch.Tensor, scores, thresholds, n_top=None) -> torch.Tensor:
    """BOP's greedy matching (evaluation/meters/utils.py:120-152 match_poses on cand[cand.error < theta], after :51-83 get_top_n_ids),
    every (group, error column, threshold) at once on the device (csrc/bop_match.hip; the contract is csrc/bop_match_core.h).
      cand        the table of `bop_candidates` (`pred_id`, `gt_id`, `group_id`)
      errs        [C,E] float32 on the device, one row per row of `cand` (`bop_candidate_errors`)
      scores      [P], one finite number per estimate: a group's estimates are walked by decreasing score, ties by ascending pred_id
      thresholds  [n_groups,E,n_theta] float64; candidate c is admissible for (e, k) when (double)errs[c,e] < thresholds[group,e,k]
      n_top       None or 0: every estimate; an int: the first n_top of each group; an array [n_groups]: per group (0 = every)
    -> match [P,E,n_theta] int32 on the device: the gt_id the estimate was given, or -1.  Nothing synchronises."""
    if not errs.is_cuda or errs.dim() != 2 or errs.shape[0] != len(cand):
        raise ValueError("errs must be a device tensor [C,E] with one row per candidate")
    dev = errs.device
    thr = torch.as_tensor(thresholds)
    if thr.dim() != 3 or thr.shape[1] != errs.shape[1] or thr.dtype != torch.float64:
        raise ValueError(f"thresholds must be float64 [n_groups,{errs.shape[1]},n_theta]")
    n_groups = int(thr.shape[0])
    index = bop_match_index(cand["pred_id"].to_numpy(), cand["gt_id"].to_numpy(), cand["group_id"].to_numpy(), scores, n_groups)
    if n_top is not None:
        n_top = np.asarray(n_top)
        if n_top.ndim == 0 and np.issubdtype(n_top.dtype, np.integer):
            n_top = np.full(n_groups, int(n_top))
        if n_top.shape != (n_groups,) or not np.issubdtype(n_top.dtype, np.integer) or (n_groups and n_top.min() < 0):
            raise ValueError("n_top must be None, an int >= 0 or one int >= 0 per group")
        index["n_top"] = n_top.astype(np.int32)
    # one host-to-device copy for the whole index
    names = [k for k in eng.BOP_MATCH_INDEX + ("n_top",) if k in index]
    flat = torch.from_numpy(np.concatenate([index[k] for k in names])).to(dev)
    on_dev, at = {"n_taken_words": index["n_taken_words"]}, 0
    for k in names:
        on_dev[k] = flat[at:at + len(index[k])]
        at += len(index[k])
    errs_sorted = errs.to(torch.float32)[torch.from_numpy(index["order"]).to(dev)]
    return eng.bop_match(errs_sorted, on_dev, thr.to(dev), len(np.asarray(scores)), n_top=on_dev.get("n_top"))


def bop_thresholds(diameters, n_tau: int = len(BOP_TAUS), image_width: int = 640) -> np.ndarray:
    """diameters [n_groups] (metres, of each group's object) -> the thresholds of correctness [n_groups, n_tau + 2, 10] float64 of the
    columns of `bop_candidate_errors`, built by the numpy expressions of `bop_recall`: BOP_THRESHOLDS for each VSD column, theta *
    diameter for MSSD, theta_px * image_width / 640 for MSPD."""
    diameters = np.asarray(diameters, np.float64)
    thetas = np.asarray(BOP_THRESHOLDS, np.float64)
    thetas_px = _thetas_px(image_width)
    thr = np.empty((len(diameters), n_tau + 2, len(thetas)), np.float64)
    thr[:, :n_tau, :] = thetas[None, None, :]
    thr[:, n_tau, :] = thetas[None, :] * diameters[:, None]
    thr[:, n_tau + 1, :] = thetas_px[None, :]
    return thr


def bop_match_recall(match: np.ndarray, n_targets: int) -> Dict[str, float]:
    """match [P, n_tau + 2, n_theta] of `bop_match` on the host -> BOP's average recalls: the share of (target, tau, theta) / (target,
    theta) with a matched ground truth.  A ground truth is matched at most once per problem, so the matches of a problem count its
    matched targets; the targets are all valid ground truths, with a candidate or not.  Averaged as `bop_recall` averages."""
    match = np.asarray(match)
    if match.ndim != 3 or match.shape[1] < 3 or n_targets <= 0:
        raise ValueError("bop_match_recall needs match [P, n_tau + 2, n_theta] and at least one target")
    n_tau, n_theta = match.shape[1] - 2, match.shape[2]
    hit = match >= 0
    ar_vsd = float(hit[:, :n_tau, :].sum() / (n_targets * n_tau * n_theta))
    ar_mssd = float(hit[:, n_tau, :].sum() / (n_targets * n_theta))
    ar_mspd = float(hit[:, n_tau + 1, :].sum() / (n_targets * n_theta))
    return {"ar_vsd": ar_vsd, "ar_mssd": ar_mssd, "ar_mspd": ar_mspd, "ar": (ar_vsd + ar_mssd + ar_mspd) / 3.0}


def bop_n_top(n_top, group_n_gt: np.ndarray) -> np.ndarray:
    """the three forms of `bop_scores`' n_top -> one int32 per group: "targets" = the group's number of valid ground truths (BOP 2019's
    inst_count; get_top_n_ids(targets=...)), an int > 0 = that count, None or 0 = every estimate (0)"""
    group_n_gt = np.asarray(group_n_gt, np.int32)
    if n_top is None:
        return np.zeros_like(group_n_gt)
    if isinstance(n_top, str):
        if n_top != "targets":
            raise ValueError(f"n_top {n_top!r} is not 'targets', an int or None")
        return group_n_gt.copy()
    if isinstance(n_top, (bool, np.bool_)) or not isinstance(n_top, (int, np.integer)) or n_top < 0:
        raise ValueError(f"n_top {n_top!r} is not 'targets', an int >= 0 or None")
    return np.full_like(group_n_gt, int(n_top))


def bop_scores(pred, gt, meshes, renderer, depth: torch.Tensor, K: torch.Tensor, valid=None, n_top="targets", score_key: str = "score",
               image_width: int = 640, keys=("batch_im_id", "label"), delta: float = 0.015, return_matches: bool = False,
               matches_at: Tuple[str, int] = ("mssd", 0), diameters=None):
    """BOP 2019 scores of estimates that carry scores (`pred.infos[score_key]`) against the ground truths of their (image, label),
    several or none of either -> {ar_vsd, ar_mssd, ar_mspd, ar, n_targets}: candidates (`bop_candidates`), their errors
    (`bop_candidate_errors`), the greedy matching at every threshold (`bop_match` under `bop_thresholds`), and per error the share of
    (valid ground truth, threshold) that got an estimate.  The denominator counts every valid ground truth, with a candidate or not.
      valid       one boolean per row of `gt` (default all): the targets
      n_top       "targets": a group's estimates are cut to its number of valid ground truths; an int > 0: to that count; None / 0: not cut
      matches_at  with return_matches, the (column, k) whose matched pairs are also returned as a DataFrame `pred_id`, `gt_id`:
                  column one of vsd_0.05 ... vsd_0.50, mssd, mspd; k the index of the threshold
      diameters   None (the box diagonal), "exact" (BOP's diameter) or a mapping label -> metres (`resolve_diameters`): the VSD
                  tolerance tau * diameter and the MSSD thresholds theta * diameter
    Other arguments as `bop_errors`.  One synchronising copy at the end."""
    valid = _valid_mask(valid, gt.infos.index, len(gt.infos))
    n_targets = int(valid.sum())
    if n_targets == 0:
        raise ValueError("bop_scores needs at least one valid ground truth")
    names = _vsd_names(BOP_TAUS) + ["mssd", "mspd"]
    if return_matches and (matches_at[0] not in names or not 0 <= int(matches_at[1]) < len(BOP_THRESHOLDS)):
        raise ValueError(f"matches_at {matches_at!r} is not (one of {names}, an index below {len(BOP_THRESHOLDS)})")
    scores = pred.infos[score_key].to_numpy().astype(np.float64)
    cand = bop_candidates(pred.infos, gt.infos, valid=valid, keys=keys)
    errs = bop_candidate_errors(pred, gt, cand, meshes, renderer, depth, K, delta=delta, diameters=diameters)
    grp = cand["group_id"].to_numpy()
    n_groups = int(grp.max()) + 1 if len(cand) else 0
    first = np.full(n_groups, -1, np.int64)
    first[grp[::-1]] = np.arange(len(cand))[::-1]                    # a group's first candidate
    labels = pred.infos["label"].to_numpy()[cand["pred_id"].to_numpy()[first]]
    diam = resolve_diameters(meshes, diameters, labels)
    thr = bop_thresholds([diam[l] for l in labels], len(BOP_TAUS), image_width)
    group_n_gt = cand.groupby("group_id")["gt_id"].nunique().reindex(np.arange(n_groups)).to_numpy() if n_groups else np.zeros(0)
    match = bop_match(cand, errs, scores, thr, n_top=bop_n_top(n_top, group_n_gt)).cpu().numpy()   # the one synchronising copy
    out = dict(bop_match_recall(match, n_targets), n_targets=n_targets)
    if not return_matches:
        return out
    col = match[:, names.index(matches_at[0]), int(matches_at[1])]
    rows = np.flatnonzero(col >= 0)
    return out, pd.DataFrame(dict(pred_id=rows.astype(np.int64), gt_id=col[rows].astype(np.int64)))


# --------------------------------------------------------------------------------------------------------------------------------
# BOP's 2D detection / 2D segmentation scores: COCO average precision over IoU 0.50:0.05:0.95
# --------------------------------------------------------------------------------------------------------------------------------
COCO_IOU_THRS = np.linspace(0.5, 0.95, 10)       # pycocotools' Params.iouThrs
COCO_REC_THRS = np.linspace(0.0, 1.0, 101)       # pycocotools' Params.recThrs


def _cand_rows(cand, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """`cand` (the table of `bop_candidates`, or a pair of arrays / tensors pred_id, gt_id) -> two int64 device tensors [C]"""
    pid, gid = (cand["pred_id"].to_numpy(), cand["gt_id"].to_numpy()) if isinstance(cand, pd.DataFrame) else cand
    return tuple(torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device=dev, dtype=torch.int64) for a in (pid, gid))


def mask_iou(pred_masks: torch.Tensor, gt_masks: torch.Tensor, cand) -> torch.Tensor:
    """Mask IoU of every candidate -> float64 [C] on the device.  pred_masks [P,H,W], gt_masks [G,H,W] on the device, uint8 or bool (a
    pixel is set when its byte is non-zero: `Detector` masks are bool, `gt_info` masks 0 / 255; both go through a uint8 view, no copy);
    cand = the table of `bop_candidates`, or (pred_id, gt_id).  The counts are csrc/det_ap.hip's (`engine.mask_pair_counts`: inter,
    area_p, area_g, integers); IoU = inter / (area_p + area_g - inter) as one float64 division in torch, 0 where the union is 0.  A
    candidate that names no mask is refused by the kernel (counts of -1) and gives NaN, which never matches.  Nothing synchronises."""
    dev = pred_masks.device
    pid, gid = _cand_rows(cand, dev)
    counts = eng.mask_pair_counts(pred_masks, gt_masks, pid.to(torch.int32), gid.to(torch.int32)).to(torch.float64)
    inter, union = counts[:, 0], counts[:, 1] + counts[:, 2] - counts[:, 0]
    iou = torch.where(union > 0, inter / union, torch.zeros_like(inter))
    return torch.where(counts[:, 0] < 0, torch.full_like(iou, float("nan")), iou)


def box_iou(pred_boxes: torch.Tensor, gt_boxes: torch.Tensor, cand) -> torch.Tensor:
    """Box IoU of every candidate -> float64 [C] on the device of `pred_boxes`; torch elementwise ops in float64.  Boxes are [x1, y1, x2,
    y2] with w = x2 - x1 and no +1 (COCO's rule on [x, y, w, h]; it agrees with `bbox_visib`'s w = xmax - xmin of `bbox_modal`).  With p
    = pred_boxes[pred_id] and g = gt_boxes[gt_id] as float64, in this order:
      iw = clamp(min(p.x2, g.x2) - max(p.x1, g.x1), min=0);  ih = clamp(min(p.y2, g.y2) - max(p.y1, g.y1), min=0);  inter = iw * ih
      area_p = (p.x2 - p.x1) * (p.y2 - p.y1);  area_g = (g.x2 - g.x1) * (g.y2 - g.y1);  union = (area_p + area_g) - inter
      iou = inter / union, 0 where union <= 0."""
    dev = pred_boxes.device
    pid, gid = _cand_rows(cand, dev)
    p, g = pred_boxes.to(torch.float64)[pid], gt_boxes.to(device=dev, dtype=torch.float64)[gid]
    iw = (torch.minimum(p[:, 2], g[:, 2]) - torch.maximum(p[:, 0], g[:, 0])).clamp(min=0)
    ih = (torch.minimum(p[:, 3], g[:, 3]) - torch.maximum(p[:, 1], g[:, 1])).clamp(min=0)
    inter = iw * ih
    area_p = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    union = (area_p + area_g) - inter
    return torch.where(union > 0, inter / union, torch.zeros_like(inter))


def coco_match(cand: pd.DataFrame, iou: torch.Tensor, scores, gt_ignore, iou_thrs=COCO_IOU_THRS, n_top=100) -> torch.Tensor:
    """COCO's greedy matching of detections to ground truths (COCOeval.evaluateImg with iscrowd = 0 and one area range), every (group,
    IoU threshold) at once on the device (csrc/det_ap.hip; the contract is csrc/det_ap_core.h).
      cand       the table of `bop_candidates(valid=None)`: ignored ground truths take part
      iou        [C] float64 on the device, one per row of `cand` (`mask_iou`, `box_iou`)
      scores     [P], one finite number per detection: a group's detections are walked by decreasing score, ties by ascending pred_id
      gt_ignore  [G] booleans (host or device), indexed by gt_id
      iou_thrs   [T] float64, T in 1..16; the bar of threshold t is min(t, 1 - 1e-10)
      n_top      COCO's maxDets: the first n_top detections of each group take part (None or 0: all)
    -> match [P,T] int32 on the device: the gt_id the detection was given (an ignored one only where no other was admissible), or -1.
    One host-to-device copy of the index; nothing synchronises."""
    if not iou.is_cuda or iou.dim() != 1 or iou.shape[0] != len(cand) or iou.dtype != torch.float64:
        raise ValueError("iou must be a float64 device tensor [C] with one entry per candidate")
    dev = iou.device
    thr = np.asarray(iou_thrs, np.float64)
    if thr.ndim != 1 or not 1 <= len(thr) <= eng.DET_MATCH_MAX_THETAS:
        raise ValueError(f"iou_thrs must be 1 .. {eng.DET_MATCH_MAX_THETAS} thresholds")
    if n_top is not None and (isinstance(n_top, (bool, np.bool_)) or not isinstance(n_top, (int, np.integer)) or n_top < 0):
        raise ValueError(f"n_top {n_top!r} is not an int >= 0 or None")
    ign = torch.as_tensor(gt_ignore)
    if ign.dtype != torch.bool or ign.dim() != 1 or (len(cand) and int(cand["gt_id"].max()) >= ign.shape[0]):
        raise ValueError("gt_ignore must be one boolean per ground truth")
    index = bop_match_index(cand["pred_id"].to_numpy(), cand["gt_id"].to_numpy(), cand["group_id"].to_numpy(), scores)
    n_groups = len(index["group_n_gt"])
    index["n_top"] = np.full(n_groups, int(n_top or 0), np.int32)
    # one host-to-device copy for the whole index: the int32 arrays, padded to an even count, then the order (int64) and the thresholds
    # (float64) as pairs of int32
    names = list(eng.BOP_MATCH_INDEX + ("n_top",))
    n32 = sum(len(index[k]) for k in names)
    parts = [index[k] for k in names] + [np.zeros(n32 % 2, np.int32), index["order"].astype(np.int64).view(np.int32), thr.view(np.int32)]
    flat = torch.from_numpy(np.concatenate(parts)).to(dev)
    on_dev, at = {"n_taken_words": index["n_taken_words"]}, 0
    for k in names:
        on_dev[k] = flat[at:at + len(index[k])]
        at += len(index[k])
    at += n32 % 2
    order = flat[at:at + 2 * len(index["order"])].view(torch.int64)
    thr_dev = flat[at + 2 * len(index["order"]):].view(torch.float64)
    return eng.det_match(iou[order], on_dev, ign.to(dev), thr_dev, len(np.asarray(scores)), n_top=on_dev["n_top"])


def coco_kept(pred_infos: pd.DataFrame, scores, n_top=100, keys=("batch_im_id", "label")) -> np.ndarray:
    """COCO's maxDets on the host -> one boolean per detection: whether it is among the first n_top of its (image, label) by decreasing
    score, ties by ascending row (None or 0: all are).  The cut `coco_match` makes inside a group, and the same cut for the detections
    whose (image, label) has no ground truth and therefore no group."""
    scores = np.asarray(scores, np.float64)
    n = len(pred_infos)
    if scores.shape != (n,):
        raise ValueError("scores must be one number per detection")
    if not n_top or n == 0:
        return np.ones(n, np.bool_)
    grp = pred_infos.reset_index(drop=True).groupby(list(keys), sort=False).ngroup().to_numpy()
    order = np.lexsort((np.arange(n), -scores, grp))
    g = grp[order]
    run_start = np.flatnonzero(np.concatenate([[True], g[1:] != g[:-1]]))
    rank = np.arange(n) - np.repeat(run_start, np.diff(np.append(run_start, n)))
    kept = np.empty(n, np.bool_)
    kept[order] = rank < int(n_top)
    return kept


def coco_accumulate(match, scores, pred_labels, gt_labels, gt_ignore, n_top_kept, iou_thrs=COCO_IOU_THRS) -> Dict[str, object]:
    """COCOeval.accumulate and summarize, restated on the host in numpy float64, for one area range and one maxDets.
      match [P,T] int32 of `coco_match` (a device tensor is copied: the one synchronising copy); scores [P]; pred_labels [P], gt_labels
      [G]; gt_ignore [G] booleans; n_top_kept [P] booleans (`coco_kept`); iou_thrs [T].
    Per label and threshold: the kept detections of all images are taken by decreasing score, ties by ascending pred row.  One matched
    to an ignored ground truth is neither true nor false positive; an unmatched kept one is a false positive (also one whose (image,
    label) has no ground truth at all, and so no candidate); one cut by n_top is dropped.  npig = the label's ground truths that are not
    ignored; a label with npig == 0 is left out.  With tp, fp the running sums: recall = tp / npig, precision = tp / (tp + fp +
    np.spacing(1)); the precision envelope is made monotone from the right and sampled at np.linspace(0, 1, 101) with searchsorted(side=
    "left"), 0 beyond the last recall.  The samples are stored as COCO stores them, precision [T,101,K] and recall [T,K] (its last value
    per threshold, 0 without detections) over the K labels that are left, by ascending label.
    -> AP = np.mean(precision), AP50 / AP75 = np.mean(precision[t]) at the threshold closest to 0.5 / 0.75 (within 1e-9; else -1), AR =
    np.mean(recall), AP_per_label = {label: np.mean(precision[:, :, k])}, labels = the K labels.  Without any label left every score is
    -1, as in COCO."""
    if torch.is_tensor(match):
        match = match.cpu().numpy()
    match = np.asarray(match)
    scores, thr = np.asarray(scores, np.float64), np.asarray(iou_thrs, np.float64)
    pred_labels, gt_labels = np.asarray(pred_labels), np.asarray(gt_labels)
    gt_ignore, kept = np.asarray(gt_ignore), np.asarray(n_top_kept)
    P, T = len(scores), len(thr)
    if match.shape != (P, T) or pred_labels.shape != (P,) or kept.shape != (P,) or kept.dtype != np.bool_:
        raise ValueError("match must be [P,T] with one score, one label and one kept flag per detection and one threshold per column")
    if gt_ignore.dtype != np.bool_ or gt_ignore.shape != gt_labels.shape or (match.size and match.max() >= len(gt_labels)):
        raise ValueError("gt_ignore must be one boolean per ground truth, and match must name ground truths")
    labels = [l for l in np.unique(gt_labels) if np.count_nonzero(~gt_ignore[gt_labels == l]) > 0]
    K, R = len(labels), len(COCO_REC_THRS)
    precision, recall = np.zeros((T, R, K)), np.zeros((T, K))
    for k, label in enumerate(labels):
        npig = np.count_nonzero(~gt_ignore[gt_labels == label])
        rows = np.flatnonzero((pred_labels == label) & kept)
        rows = rows[np.lexsort((rows, -scores[rows]))]
        m = match[rows]
        matched = m >= 0
        to_ignored = matched & gt_ignore[np.clip(m, 0, None)]
        tp_sum = np.cumsum(matched & ~to_ignored, axis=0).astype(np.float64)
        fp_sum = np.cumsum(~matched, axis=0).astype(np.float64)
        for t in range(T):
            tp, fp = tp_sum[:, t], fp_sum[:, t]
            nd = len(tp)
            rc = tp / npig
            pr = tp / (fp + tp + np.spacing(1))
            recall[t, k] = rc[-1] if nd else 0.0
            pr = np.maximum.accumulate(pr[::-1])[::-1]
            at = np.searchsorted(rc, COCO_REC_THRS, side="left")
            inside = at < nd
            precision[t, inside, k] = pr[at[inside]]
    if K == 0:
        return dict(AP=-1.0, AP50=-1.0, AP75=-1.0, AR=-1.0, AP_per_label={}, labels=[])

    def at_thr(value):
        t = np.flatnonzero(np.abs(thr - value) < 1e-9)
        return float(np.mean(precision[t[0]])) if len(t) else -1.0

    return dict(AP=float(np.mean(precision)), AP50=at_thr(0.5), AP75=at_thr(0.75), AR=float(np.mean(recall)),
                AP_per_label={l: float(np.mean(precision[:, :, k])) for k, l in enumerate(labels)}, labels=labels)


def bop_detection_scores(pred, gt, info: pd.DataFrame, iou_type: str = "bbox", gt_masks: Optional[torch.Tensor] = None,
                         visib_gt_min: float = 0.1, n_top: int = 100, score_key: str = "score", keys=("batch_im_id", "label")):
    """The scores of BOP's 2D detection ("bbox") and 2D segmentation ("segm") tasks: COCO AP over IoU 0.50:0.05:0.95, AP50, AP75, AR and
    per-label AP (the dict of `coco_accumulate`).
      pred      detections as `Detector.get_detections(output_masks=True)` returns them: infos `label`, `batch_im_id`, `score`; `bboxes`
                [P,4] xyxy ("bbox") or `masks` [P,H,W] bool / uint8 on the device ("segm")
      gt        the ground truths (`infos` with `label`, `batch_im_id`); info  the table of `gt_info`, row-aligned with `gt.infos`
      gt_masks  "segm": `gt_info(return_masks=True)`'s mask_visib [G,H,W] on the device; "bbox" scores against `bbox_modal`
    A ground truth is ignored when visib_fract < visib_gt_min or px_count_visib == 0; ignored ground truths take part in the matching
    (`bop_candidates(valid=None)`), so a detection of one is neither true nor false positive.  n_top is COCO's maxDets per (image, label).
    One synchronising copy (the match table).
    Unpinned against pycocotools and bop_toolkit (both absent here).  Known deviation: stock pycocotools overwrites a ground truth's
    `ignore` with `iscrowd`; here the caller's flag is honoured."""
    if iou_type not in ("bbox", "segm"):
        raise ValueError(f"iou_type {iou_type!r} is not 'bbox' or 'segm'")
    if len(info) != len(gt.infos):
        raise ValueError("info must have one row per row of gt")
    scores = pred.infos[score_key].to_numpy().astype(np.float64)
    cand = bop_candidates(pred.infos, gt.infos, valid=None, keys=keys)
    gt_ignore = (info["visib_fract"].to_numpy() < float(visib_gt_min)) | (info["px_count_visib"].to_numpy() == 0)
    if iou_type == "segm":
        if gt_masks is None or not gt_masks.is_cuda or gt_masks.shape[0] != len(gt.infos):
            raise ValueError("iou_type 'segm' needs gt_masks [G,H,W] on the device")
        iou = mask_iou(pred.masks.to(gt_masks.device), gt_masks, cand)
    else:
        boxes = pred.bboxes if pred.bboxes.is_cuda else pred.bboxes.cuda()
        gt_boxes = torch.as_tensor(np.asarray(list(info["bbox_modal"]), np.float64).reshape(-1, 4))
        iou = box_iou(boxes, gt_boxes, cand)
    match = coco_match(cand, iou, scores, gt_ignore, n_top=n_top)
    kept = coco_kept(pred.infos, scores, n_top=n_top, keys=keys)
    return coco_accumulate(match, scores, pred.infos["label"].to_numpy(), gt.infos["label"].to_numpy(), gt_ignore, kept)


# --------------------------------------------------------------------------------------------------------------------------------
# BOP's model info: the exact diameter and the bounds of every object (models_info.json)
# --------------------------------------------------------------------------------------------------------------------------------
MODEL_INFO_COLUMNS = ("diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z", "pt_i", "pt_j")


def model_info_table(labels, pair, bounds, pts_i, pts_j) -> pd.DataFrame:
    """The host side of `model_info`: pair [n,2] and bounds [n,6] as the kernel gives them, pts_i / pts_j [n,3] the two fp32 points it
    named -> a DataFrame indexed by label with MODEL_INFO_COLUMNS.  `diameter` is the float64 distance of the two fp32 points, not the
    square root of the kernel's fp32 d2; an object the kernel refused (pair -1 -1) has NaN."""
    pair = np.asarray(pair, np.int64).reshape(-1, 2)
    bounds = np.asarray(bounds, np.float32).reshape(-1, 6).astype(np.float64)
    a, b = np.asarray(pts_i, np.float32).astype(np.float64), np.asarray(pts_j, np.float32).astype(np.float64)
    diameter = np.sqrt(((a - b) ** 2).sum(1))
    diameter[pair[:, 0] < 0] = np.nan
    cols = {"diameter": diameter}
    for k, name in enumerate(MODEL_INFO_COLUMNS[1:7]):
        cols[name] = bounds[:, k]
    cols["pt_i"], cols["pt_j"] = pair[:, 0], pair[:, 1]
    return pd.DataFrame(cols, index=pd.Index(list(labels), name="label"))


def model_info(meshes, tile: int = 0) -> pd.DataFrame:
    """What bop_toolkit's calc_model_info writes to models_info.json, for every object of `meshes` (a BatchedMeshes on the device), in
    metres: `diameter` = the largest distance between two model points (calc_pts_diameter's O(N^2) maximum, one launch of
    csrc/model_info.hip over all objects), min_* / size_* = the axis-aligned bounds, pt_i <= pt_j = the rows of `meshes.points` that
    are the farthest apart (on equal fp32 distances the lowest pt_i, then the lowest pt_j).  -> a DataFrame indexed by label.  tile
    as `engine.model_info` takes it.  One synchronising copy."""
    labels = list(meshes.labels)
    pts = meshes.points
    n_points = np.asarray([meshes.infos[l]["n_points"] for l in labels], np.int32)
    _, pair, bounds = eng.model_info(pts, n_points, tile=tile)
    rows = torch.arange(len(labels), device=pts.device)
    ends = pts[rows[:, None], pair.long().clamp(min=0)]                                       # [n,2,3]
    table = torch.cat([pair.double(), bounds.double(), ends.flatten(1).double()], dim=1).cpu().numpy()   # the one synchronising copy
    return model_info_table(labels, table[:, :2], table[:, 2:8], table[:, 8:11], table[:, 11:14])


def _bop_obj_key(label):
    """the key of an object in models_info.json: BOP's integer id where the label carries one ("obj_000005" or "5" -> 5)"""
    m = re.fullmatch(r"(?:obj_)?(\d+)", str(label))
    return int(m.group(1)) if m else label


def bop_models_info(info: pd.DataFrame, scale: float = 1000.0, symmetries: Optional[pd.DataFrame] = None) -> Dict[object, Dict[str, object]]:
    """The table of `model_info` -> the dict bop_toolkit saves as models_info.json: {obj_id: {diameter, min_x, min_y, min_z, size_x,
    size_y, size_z}}, every length times `scale` (BOP's files are in millimetres), keyed by the integer id where the label has one
    ("obj_000005" -> 5), else by the label.  With `symmetries` = the table of `find_symmetries`, an object it lists also gets BOP's
    `symmetries_discrete` (each a row-major 4x4 matrix as 16 numbers, the translation times `scale`) and `symmetries_continuous`
    ({"axis", "offset"}, the offset times `scale`), each only where the object has one, as in BOP's files."""
    out = {}
    for label, row in info.iterrows():
        key = _bop_obj_key(label)
        if key in out:
            raise ValueError(f"two labels give the object key {key!r}")
        out[key] = {name: float(row[name]) * float(scale) for name in MODEL_INFO_COLUMNS[:7]}
        if symmetries is not None and label in symmetries.index:
            sym = symmetries.loc[label]
            discrete = []
            for T in sym["symmetries_discrete"]:
                T = np.array(T, np.float64).reshape(4, 4)
                T[:3, 3] *= float(scale)
                discrete.append([float(v) for v in T.flatten()])
            continuous = [{"axis": [float(v) for v in s["axis"]], "offset": [float(v) * float(scale) for v in s["offset"]]}
                          for s in sym["symmetries_continuous"]]
            if discrete:
                out[key]["symmetries_discrete"] = discrete
            if continuous:
                out[key]["symmetries_continuous"] = continuous
    return out


def save_models_info(path, info, scale: float = 1000.0, symmetries: Optional[pd.DataFrame] = None) -> None:
    """Write models_info.json: `info` the table of `model_info` (scaled by `scale` through `bop_models_info`, with the symmetry fields
    of `symmetries`, the table of `find_symmetries`, if given) or a dict that is already BOP's (written as it is)."""
    import json

    data = bop_models_info(info, scale, symmetries) if isinstance(info, pd.DataFrame) else info
    with open(path, "w") as f:
        json.dump({str(k): v for k, v in data.items()}, f, indent=2, sort_keys=True)


def load_models_info(path, scale: float = 0.001, label_format: str = "obj_{:06d}", return_info: bool = False):
    """Read a BOP models_info.json -> {label: diameter in metres}, what the `diameters=` keyword takes.  An integer key becomes
    label_format.format(id) (the reference's "obj_000005", bop_object_datasets.py:40), any other key is the label itself; `scale`
    turns the file's unit into metres.  With return_info also the file's dict, keyed by label, every field as it is in the file
    (symmetries_discrete, symmetries_continuous: kept, not interpreted)."""
    import json

    with open(path) as f:
        data = json.load(f)
    diameters, infos = {}, {}
    for key, fields in data.items():
        label = label_format.format(int(key)) if re.fullmatch(r"\d+", str(key)) else str(key)
        diameters[label] = float(fields["diameter"]) * float(scale)
        infos[label] = fields
    return (diameters, infos) if return_info else diameters


# --------------------------------------------------------------------------------------------------------------------------------
# Object symmetries from the mesh alone: the two symmetry fields of models_info.json (csrc/symmetry.hip decides the candidates)
# --------------------------------------------------------------------------------------------------------------------------------
SYMMETRY_MAX_CANDIDATES = 4096        # candidates of one object by default: 64 anchors' worth of 64; a finely tessellated sphere has more
SYMMETRY_DUPLICATE_ANGLE = 1e-3       # radians: two rotations (and two axes) closer than this are one; a point at the object's radius
#                                       moves by a tenth of the default tolerance (0.01 x diameter) under such a rotation
SYMMETRY_COLUMNS = ("status", "n_candidates", "n_symmetries", "center", "rotations", "deviation", "symmetries_discrete", "symmetries_continuous")


def _unit(v: np.ndarray) -> np.ndarray:
    return v / np.linalg.norm(v)


def _anchor_frame(c: np.ndarray, p1: np.ndarray, p2: np.ndarray) -> np.ndarray:
    """the right-handed orthonormal frame of two anchors about c, as columns: e1 along p1 - c, e2 the part of p2 - c normal to it"""
    e1 = _unit(p1 - c)
    q = p2 - c
    e2 = _unit(q - (q @ e1) * e1)
    return np.stack([e1, e2, np.cross(e1, e2)], axis=1)


def surface_centroid(vertices: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """The area-weighted centroid of a triangle surface, in float64: every symmetry of the surface fixes it."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    total = area.sum()
    if not total > 0.0:
        return v.mean(0)
    return ((a + b + c) / 3.0 * area[:, None]).sum(0) / total


def symmetry_candidates(vertices: np.ndarray, faces: np.ndarray, tol: float, max_candidates: int = SYMMETRY_MAX_CANDIDATES):
    """The candidate rotations of one object, on the host in float64, O(V) per anchor -> (status, center [3], rotations [n,3,3],
    n_candidates).  The centre c is the surface centroid.  The anchor a1 is the vertex farthest from c, a2 the vertex farthest from
    the line (c, a1) (ties: the lowest index); both are maxima of convex functions over the surface, so they are attained at vertices
    and a symmetry maps them to vertices with the same invariants.  For every vertex b1 with | |b1 - c| - |a1 - c| | <= tol, every
    vertex b2 that matches a2's distance to the line, |a2 - c| and |a2 - a1| (each within tol) gives the candidate
    frame(c, b1, b2) frame(c, a1, a2)^T, a proper rotation; candidates are ordered by (b1, b2).  status "degenerate": no vertex is
    farther than tol from the line (no second anchor); "too_many_candidates": more than max_candidates (the count is returned, no
    rotation is); else "ok"."""
    v = np.asarray(vertices, np.float64)
    c = surface_centroid(v, faces)
    none = np.zeros((0, 3, 3))
    q = v - c
    r = np.linalg.norm(q, axis=1)
    i1 = int(np.argmax(r))
    if not r[i1] > tol:
        return "degenerate", c, none, 0

    def line_distance(u):
        return np.linalg.norm(q - (q @ u)[:, None] * u, axis=1)

    l1 = line_distance(q[i1] / r[i1])
    i2 = int(np.argmax(l1))
    if not l1[i2] > tol:
        return "degenerate", c, none, 0
    d12 = np.linalg.norm(v[i2] - v[i1])
    pairs = []
    for b1 in np.flatnonzero(np.abs(r - r[i1]) <= tol):
        lb = line_distance(q[b1] / r[b1])
        ok = (np.abs(lb - l1[i2]) <= tol) & (np.abs(r - r[i2]) <= tol) & (np.abs(np.linalg.norm(v - v[b1], axis=1) - d12) <= tol)
        pairs += [(int(b1), int(b2)) for b2 in np.flatnonzero(ok)]
        if len(pairs) > max_candidates:    # the count so far already refuses the object
            return "too_many_candidates", c, none, len(pairs)
    Fa = _anchor_frame(c, v[i1], v[i2])
    rotations = np.stack([_anchor_frame(c, v[b1], v[b2]) @ Fa.T for b1, b2 in pairs]) if pairs else none
    return "ok", c, rotations, len(pairs)


def _relative_angles(R: np.ndarray, Rs: np.ndarray) -> np.ndarray:
    """the rotation angles of R Rs[k]^T"""
    tr = np.einsum("ij,kij->k", R, Rs)
    return np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0))


def _axis_angle(R: np.ndarray) -> Tuple[np.ndarray, float]:
    """axis (unit, its largest component positive) and angle in (0, pi] of a rotation that is not the identity"""
    angle = float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if np.linalg.norm(w) > 1e-6:
        axis = _unit(w)
    else:                                  # a half turn: R + I = 2 a a^T
        S = (R + np.eye(3)) / 2.0
        axis = _unit(S[:, int(np.argmax(np.diag(S)))])
    k = int(np.argmax(np.abs(axis)))
    return (axis if axis[k] > 0 else -axis), angle


def symmetry_group(center: np.ndarray, rotations: np.ndarray, continuous_min_order: int = 16):
    """The accepted rotations of one object (in candidate order) -> (status, unique rotations [n,3,3] with the identity first,
    symmetries_discrete [list of 4x4], symmetries_continuous [list of {"axis", "offset"}]), float64.  Rotations within
    SYMMETRY_DUPLICATE_ANGLE of an earlier one are dropped.  The others are clustered by axis; an axis whose cyclic order (its elements
    and the identity) is at least continuous_min_order is BOP's continuous symmetry {"axis": its largest component positive, "offset":
    center}; the discrete symmetries are then one representative, the first in candidate order, of every coset of that axis' rotations
    but their own, else every element but the identity, each as T = [R | c - R c].  More than one such axis (a sphere): everything stays
    discrete, status "many_continuous_axes"."""
    c = np.asarray(center, np.float64)
    unique = [np.eye(3)]
    for R in np.asarray(rotations, np.float64).reshape(-1, 3, 3):
        if _relative_angles(R, np.stack(unique)).min() >= SYMMETRY_DUPLICATE_ANGLE:
            unique.append(R)
    axes, members = [], []                 # the clusters: axis, and the indices into unique
    for k in range(1, len(unique)):
        axis, _ = _axis_angle(unique[k])
        for n, a in enumerate(axes):
            if np.arccos(min(1.0, abs(float(a @ axis)))) < SYMMETRY_DUPLICATE_ANGLE:
                members[n].append(k)
                break
        else:
            axes.append(axis)
            members.append([k])
    continuous_axes = [n for n in range(len(axes)) if len(members[n]) + 1 >= continuous_min_order]

    def pose(R):
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = c - R @ c
        return T

    status, continuous = "ok", []
    discrete_ids = list(range(1, len(unique)))
    if len(continuous_axes) > 1:
        status = "many_continuous_axes"
    elif len(continuous_axes) == 1:
        a = axes[continuous_axes[0]]
        continuous = [{"axis": a.copy(), "offset": c.copy()}]
        reps = [0]                         # the identity stands for the axis' own rotations
        for k in range(1, len(unique)):
            # unique[k] and unique[j] are in one coset when unique[j]^T unique[k] turns about a: it fixes a
            if not any(np.linalg.norm(unique[j].T @ unique[k] @ a - a) < 2.0 * SYMMETRY_DUPLICATE_ANGLE for j in reps):
                reps.append(k)
        discrete_ids = reps[1:]
    return status, np.stack(unique), [pose(unique[k]) for k in discrete_ids], continuous


def symmetry_table(labels, problems, accept, dev2, continuous_min_order: int = 16) -> pd.DataFrame:
    """The host side of `find_symmetries`: problems = per object (status, center, rotations, n_candidates) of `symmetry_candidates`,
    accept and dev2 [C_total] what `engine.symmetry_check` gave for the candidates of all objects, one after the other -> the
    DataFrame of `find_symmetries`."""
    accept, dev2 = np.asarray(accept).astype(bool), np.asarray(dev2, np.float64)
    rows, at = [], 0
    for status, center, rotations, n_cand in problems:
        n = len(rotations)
        acc, d2 = accept[at:at + n], dev2[at:at + n]
        at += n
        group_status, unique, discrete, continuous = symmetry_group(center, rotations[acc], continuous_min_order)
        deviation = float(np.sqrt(d2[acc].max())) if acc.any() else 0.0
        rows.append(dict(status=status if status != "ok" else group_status, n_candidates=int(n_cand), n_symmetries=len(unique), center=center,
                         rotations=unique, deviation=deviation, symmetries_discrete=discrete, symmetries_continuous=continuous))
    return pd.DataFrame(rows, columns=list(SYMMETRY_COLUMNS), index=pd.Index(list(labels), name="label"))


def find_symmetries(mesh_db, rel_tol: float = 0.01, n_samples: int = 512, seed: int = 0, continuous_min_order: int = 16,
                    max_candidates: int = SYMMETRY_MAX_CANDIDATES, diameters=None, device="cuda", measure_all: bool = False, tile: int = 0,
                    backend=None) -> pd.DataFrame:
    """The rotational symmetries of every object of `mesh_db` (a MeshDataBase of objects with faces), found from the mesh alone: what
    a BOP dataset declares by hand in models_info.json.  A rotation R about the centre c is a symmetry when g(p) = R (p - c) + c takes
    every test point (the vertices, then n_samples points drawn over the surface by `engine.surface_sample` on the uniforms of a CPU
    generator seeded with `seed`, as `MeshDataBase.batched_surface` draws them) to within tol = rel_tol x diameter of the surface.  The
    candidates come from `symmetry_candidates` on the host; one `engine.symmetry_check` call on `device` decides those of all objects;
    `symmetry_group` turns the accepted ones into BOP's fields.  diameters: None = the exact diameter of `model_info` (one more launch
    on `device`), or a mapping label -> metres.  measure_all: measure every candidate (the check's mode 1) instead of screening first;
    tile as `engine.symmetry_check` takes it.  backend: what supplies surface_sample and symmetry_check (default: the engine).
    -> a DataFrame indexed by label:
      status                 "ok"; "degenerate" (no vertex farther than tol from the line through the centre and the farthest vertex);
                             "too_many_candidates" (more than max_candidates; a finely tessellated sphere); "many_continuous_axes"
                             (more than one axis of order >= continuous_min_order: everything is kept discrete).  A refused object is
                             reported as asymmetric.
      n_candidates           rotations tested
      n_symmetries           the order of the group found, the identity included
      center                 [3] float64, metres
      rotations              [n_symmetries,3,3] float64, the identity first, then in candidate order
      deviation              the largest distance, in metres, by which an accepted rotation takes a test point off the surface
      symmetries_discrete    list of [4,4] float64 in metres, T = [R | c - R c]; never the identity
      symmetries_continuous  list of {"axis": [3], "offset": [3]}: an axis whose cyclic order is at least continuous_min_order (a
                             parameter of the contract, not a measurement)
    LIMITS.  Reflections are not symmetries here (BOP's are rigid).  Candidates come from vertex anchors: a scanned mesh whose symmetry
    is only approximate, with no vertex near the image of the anchors, can be missed; CAD meshes are covered.  Unpinned against
    bop_toolkit's annotations (absent).  One synchronising copy."""
    backend = eng if backend is None else backend
    labels = list(mesh_db.labels)
    verts = [np.asarray(mesh_db.engine_meshes[l]["points"], np.float32) for l in labels]
    faces = [np.asarray(mesh_db.engine_meshes[l]["faces"], np.int32).reshape(-1, 3) for l in labels]
    for l, f in zip(labels, faces):
        if len(f) == 0:
            raise ValueError(f"object {l!r} has no faces: a symmetry is one of a surface")
    n_samples = int(n_samples)
    if n_samples < 0 or not (np.isfinite(rel_tol) and rel_tol > 0.0):
        raise ValueError(f"n_samples must not be negative and rel_tol must be positive and finite, got {n_samples} and {rel_tol}")
    if int(max_candidates) < 1 or int(continuous_min_order) < 2:
        raise ValueError(f"max_candidates must be at least 1 and continuous_min_order at least 2, got {max_candidates} and {continuous_min_order}")
    if diameters is None:
        diameters = model_info(mesh_db.batched().to(device))["diameter"].to_dict()
    tol = []
    for l in labels:
        d = float(diameters[l])
        if not (np.isfinite(d) and d > 0.0):
            raise ValueError(f"the diameter of {l!r} is {d}: it must be positive and finite")
        tol.append(float(rel_tol) * d)
    problems = [symmetry_candidates(v, f, t, int(max_candidates)) for v, f, t in zip(verts, faces, tol)]
    vert_off = np.concatenate([[0], np.cumsum([len(v) for v in verts])])
    face_off = np.concatenate([[0], np.cumsum([len(f) for f in faces])])
    test_off = np.concatenate([[0], np.cumsum([len(v) + n_samples for v in verts])])
    cand_off = np.concatenate([[0], np.cumsum([len(p[2]) for p in problems])])
    d_verts = torch.from_numpy(np.concatenate(verts)).to(device)
    h_faces = np.concatenate(faces)
    d_faces = torch.from_numpy(h_faces).to(device)
    failed = None
    if n_samples > 0:
        u = torch.rand(len(labels), n_samples, 3, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)
        sampled, face = backend.surface_sample(d_verts, d_faces, vert_off, face_off, u.to(device))
        failed = face[:, 0] < 0
        tests = torch.cat([t for n in range(len(labels)) for t in (d_verts[vert_off[n]:vert_off[n + 1]], sampled[n])])
    else:
        tests = d_verts
    cand_R = torch.from_numpy(np.concatenate([p[2] for p in problems]).astype(np.float32).reshape(-1, 3, 3)).to(device)
    centers = torch.from_numpy(np.stack([p[1] for p in problems]).astype(np.float32)).to(device)
    accept, dev2, _ = backend.symmetry_check(d_verts, h_faces, tests, cand_R, centers, vert_off, face_off, test_off, cand_off,
                                             np.asarray(tol, np.float32), mode=1 if measure_all else 0, tile=tile)
    flags = failed.float() if failed is not None else torch.zeros(len(labels), device=accept.device)
    table = torch.cat([accept.float(), dev2, flags.to(accept.device)]).cpu().numpy()   # the one synchronising copy
    n_cand = int(cand_off[-1])
    for l, bad, problem in zip(labels, table[2 * n_cand:], problems):
        if bad and problem[0] == "ok":       # an object already refused (a needle has no area) needs no test points
            raise ValueError(f"object {l!r} cannot be sampled: a non-finite vertex, a face index outside its vertices, or no area")
    return symmetry_table(labels, problems, table[:n_cand] > 0, table[n_cand:2 * n_cand], continuous_min_order)


def symmetry_poses(fields, n_symmetries_continuous: int = 64, scale: float = 1.0) -> np.ndarray:
    """The symmetry set of one object -> [n,4,4] float64.  fields: a row of `find_symmetries`' table or an object's dict of a
    models_info.json (`load_models_info(return_info=True)`): "symmetries_discrete" (4x4 matrices, or their 16 numbers) and
    "symmetries_continuous" ({"axis", "offset"}), either may be missing; translations and offsets are multiplied by `scale` (0.001
    for a BOP file in millimetres).  A continuous symmetry about ANY axis and offset is discretised into n_symmetries_continuous
    rotations by Rodrigues' formula, R = I + sin(t) K + (1 - cos(t)) K^2 about the unit axis, t = o - R o.  The order is
    `symmetries.make_symmetries_poses`': the identity first among the discrete symmetries, and with continuous ones the product
    continuous x discrete, the continuous index running inside."""
    def get(name):
        v = fields[name] if name in fields else None
        return [] if v is None else list(v)

    discrete = [np.eye(4)]
    for T in get("symmetries_discrete"):
        T = np.array(T, np.float64).reshape(4, 4)
        T[:3, 3] *= float(scale)
        discrete.append(T)
    continuous = []
    for s in get("symmetries_continuous"):
        axis = _unit(np.asarray(s["axis"], np.float64))
        offset = np.asarray(s["offset"], np.float64) * float(scale)
        K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
        for n in range(int(n_symmetries_continuous)):
            t = 2.0 * np.pi * n / int(n_symmetries_continuous)
            M = np.eye(4)
            M[:3, :3] = np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)
            M[:3, 3] = offset - M[:3, :3] @ offset
            continuous.append(M)
    if not continuous:
        return np.stack(discrete)
    return np.stack([c @ d for d in discrete for c in continuous])
