"""Depth refiners: `DepthRefiner` interface + on-device `ICPRefiner` and `TeaserppRefiner`.

Same class names / constructor / `refine_poses` contract as the reference's src/megapose/inference/depth_refiner.py:29-51 and
src/megapose/inference/icp_refiner.py:178-262: render depth at the image resolution for every prediction, mask by
|measured - rendered| <= 0.1 m, refine with ICP, keep the input pose when the refinement is rejected.  The per-object CPU loop
(numpy back-projection, cv2.inpaint/gaussian normals, OpenCV ppf_match_3d_ICP) becomes one batched device call
(`mp_icp_refine_nn`, csrc/icp_nn.hip: the reference's algorithm step for step; OpenCV's ICP is third-party, restated in
oracle/icp_opencv.py, parity unpinned) -- or the cheaper projective-association variant `mp_icp_refine` (csrc/icp.hip).

`TeaserppRefiner` is the reference's src/megapose/inference/teaserpp_refiner.py:165-289: the same rendered depth, correspondences
pixel by pixel between the rendered and the measured depth, farthest point sampling and a truncated-least-squares registration, one
batched device call (`mp_teaser_refine_ex`, csrc/teaser.hip; the rules and the deviations are in csrc/teaser_core.h,
csrc/teaser_clique_core.h and DESIGN.md 3.14).
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Optional, Tuple

import torch

from . import engine as eng
from .types import Panda3dLightData, PoseEstimatesType


class DepthRefiner(ABC):
    @abstractmethod
    def refine_poses(self, predictions: PoseEstimatesType, masks: Optional[torch.Tensor] = None, depth: Optional[torch.Tensor] = None,
                     K: Optional[torch.Tensor] = None) -> Tuple[PoseEstimatesType, dict]:
        """predictions: N rows indexing depth / masks / K through `batch_im_id`; depth [B,H,W]; masks [B,H,W]; K [B,3,3].
        Returns (refined predictions with `poses` replaced, extra_data)."""


class ICPRefiner(DepthRefiner):
    def __init__(self, mesh_db, renderer, n_iterations: int = 100, n_levels: int = 4, tolerance: float = 0.05, n_min_points: int = 1000,
                 association: str = "nn"):
        # association (engine extension): "nn" = the reference's algorithm on the device (get_normal + OpenCV-style nearest-neighbour ICP,
        # csrc/icp_nn.hip); "projective" = the cheaper projective-association ICP of csrc/icp.hip
        self.association = association
        self.mesh_db = mesh_db
        self.renderer = renderer
        self.light_datas = [Panda3dLightData("ambient")]
        self.n_iterations, self.n_levels, self.tolerance, self.n_min_points = n_iterations, n_levels, tolerance, n_min_points

    @torch.no_grad()
    def refine_poses(self, predictions: PoseEstimatesType, masks: Optional[torch.Tensor] = None, depth: Optional[torch.Tensor] = None,
                     K: Optional[torch.Tensor] = None) -> Tuple[PoseEstimatesType, dict]:
        assert depth is not None
        assert K is not None
        predictions_refined = predictions.clone()
        df = predictions.infos
        labels = df.label.tolist()
        N = len(predictions)
        device = depth.device
        im_ids = torch.as_tensor(df.batch_im_id.values.astype("int32"), device=device)
        TCO_ = predictions.poses.to(device=device, dtype=torch.float32)
        K_ = K[im_ids.long()].float()
        resolution = tuple(depth.shape[-2:])
        # depth at the pixel centres (not the off-centre sample a multisample depth resolve returns): it is back-projected below
        depth_rendered = self.renderer.render_depth(labels, TCO_, K_, resolution).contiguous()
        depth_meas = depth.float()
        if self.association == "nn":  # the caller's masks REPLACE the threshold mask (icp_refiner.py:249-250); they only select points
            refined, retval, residual, iters = eng.icp_refine(depth_meas.contiguous(), im_ids, depth_rendered, K.float(), K_, TCO_,
                                                              self.n_iterations, self.n_levels, self.tolerance, self.n_min_points,
                                                              association="nn", return_iters=True,
                                                              masks=None if masks is None else masks.reshape(depth_meas.shape))
        else:
            iters = None
            if masks is not None:
                depth_meas = depth_meas * (masks.to(depth_meas.dtype) > 0)
            refined, retval, residual = eng.icp_refine(depth_meas.contiguous(), im_ids, depth_rendered, K.float(), K_, TCO_, self.n_iterations,
                                                       self.n_levels, self.tolerance, self.n_min_points, user_masks=masks is not None,
                                                       association="projective")
        if "poses_input" in predictions_refined.tensors:
            predictions_refined.poses_input = predictions.poses.clone()
        else:
            predictions_refined.register_tensor("poses_input", predictions.poses.clone())
        predictions_refined.poses = refined
        extra = {"retval": retval, "residual": residual}
        if iters is not None:
            extra["iterations_per_level"] = iters[:, : self.n_levels]   # (telemetry; index = pyramid level, coarsest = n_levels - 1)
        return predictions_refined, extra


class TeaserppRefiner(DepthRefiner):
    def __init__(self, mesh_db, renderer, mask_type: str = "simple", depth_delta_thresh: float = 0.1, n_min_points: int = 100, n_points: int = 1000,
                 noise_bound: float = 0.01, min_num_inliers: int = 50, use_farthest_point_sampling: bool = True, *,
                 inlier_selection: str = "kcore", rotation_tim_graph: str = "chain"):
        # engine extensions (keyword-only): inlier_selection "kcore" = the vertices of the consistency graph's largest core number
        # (the default here), "max_clique" = an exact maximum clique of that graph (TEASER++'s default) searched under the step budget
        # `max_clique_steps` (an attribute: None = the engine's default budget; a row that exhausts it selects the best clique found
        # until then), "none" = every correspondence; rotation_tim_graph "chain" = consecutive pairs of the selected correspondences
        # (TEASER++'s default), "complete" = all pairs
        if mask_type not in eng.TEASER_MASK_TYPES:
            raise ValueError(f"Unknown mask type {mask_type}")
        if inlier_selection not in eng.TEASER_SELECTIONS or rotation_tim_graph not in eng.TEASER_TIM_GRAPHS:
            raise ValueError(f"inlier_selection must be one of {sorted(eng.TEASER_SELECTIONS)} and rotation_tim_graph one of {sorted(eng.TEASER_TIM_GRAPHS)}")
        if not 1 <= n_points <= eng.TEASER_MAX_POINTS:
            raise ValueError(f"n_points must be 1 .. {eng.TEASER_MAX_POINTS}, got {n_points}")
        self.mesh_db = mesh_db
        self.renderer = renderer
        self.mask_type = mask_type
        self.depth_delta_thresh = depth_delta_thresh
        self.n_min_points = n_min_points
        self.n_points = n_points
        self.noise_bound = noise_bound
        self.min_num_inliers = min_num_inliers
        self.use_farthest_point_sampling = use_farthest_point_sampling
        self.inlier_selection = inlier_selection
        self.rotation_tim_graph = rotation_tim_graph
        self.max_clique_steps: Optional[int] = None
        self.light_datas = [Panda3dLightData("ambient")]
        self.debug: dict = {}

    @torch.no_grad()
    def refine_poses(self, predictions: PoseEstimatesType, masks: Optional[torch.Tensor] = None, depth: Optional[torch.Tensor] = None,
                     K: Optional[torch.Tensor] = None) -> Tuple[PoseEstimatesType, dict]:
        """`masks` is not used (the reference keeps the argument for backward compatibility)."""
        assert depth is not None
        assert K is not None
        predictions_refined = predictions.clone()
        df = predictions.infos
        device = depth.device
        im_ids = torch.as_tensor(df.batch_im_id.values.astype("int32"), device=device)
        TCO_ = predictions.poses.to(device=device, dtype=torch.float32)
        K_ = K[im_ids.long()].float()
        depth_rendered = self.renderer.render_depth(df.label.tolist(), TCO_, K_, tuple(depth.shape[-2:])).contiguous()
        exact = self.inlier_selection == "max_clique"
        refined, retval, info, *tel = eng.teaser_refine(depth.float().contiguous(), im_ids, depth_rendered, K_, TCO_, self.mask_type, self.depth_delta_thresh,
                                                        self.n_min_points, self.n_points, self.noise_bound, self.min_num_inliers,
                                                        self.use_farthest_point_sampling, self.inlier_selection, self.rotation_tim_graph, telemetry=exact,
                                                        max_clique_steps=self.max_clique_steps)
        if "poses_input" in predictions_refined.tensors:
            predictions_refined.poses_input = predictions.poses.clone()
        else:
            predictions_refined.register_tensor("poses_input", predictions.poses.clone())
        predictions_refined.poses = refined
        extra = {"retval": retval, "n_mask_points": info[:, 0], "n_points": info[:, 1], "n_selected": info[:, 2], "gnc_iterations": info[:, 3],
                 "num_inliers": info[:, 4]}
        if exact:
            extra["clique_exact"], extra["clique_steps"] = tel[0]["clique"][:, 2], tel[0]["clique"][:, 3]
        self.debug = extra
        return predictions_refined, extra
