"""PoseEstimator: SO(3)-grid hypotheses -> coarse scores -> top-K -> iterative refinement -> re-scoring -> arg-max.

Same public API, return types, DataFrame columns and `extra_data` keys as the reference
src/megapose/inference/pose_estimator.py:52-667, so it drops into
src/megapose/scripts/run_inference_on_example.py:126-148 unchanged.  What differs is the schedule: the reference walks
three Python loops of tiny batches (bsz_images / bsz_objects are 2022-era memory workarounds), gathers one full frame
per hypothesis row and syncs to the host in every batch; here every stage runs as a few large launches over rows that
share the single observation frame by index, and the host is touched once per stage (to fill the DataFrame).
`bsz_images` / `bsz_objects` are accepted and kept as attributes; the engine batches by `max_rows_per_launch`
(set `strict_batching=True` to honour the reference batch sizes exactly).

Multi-GPU: with torch.distributed initialised and `distributed=True`, rows are sharded `rank::world`,
coarse logits are all-gathered (RCCL), every rank computes the same top-K, refine+score runs on the local shard, and
`[rows,17]` (pose + logit) is all-gathered so that every rank returns the full result.
"""
from __future__ import annotations

import time
from pathlib import Path
from typing import Any, List, Optional, Tuple

import numpy as np
import pandas as pd
import torch

from . import distributed as mpdist
from . import engine as eng
from . import tcoll as tc
from .tcoll import PandasTensorCollection
from .types import DetectionsType, ObservationTensor, PoseEstimatesType, assert_detections_valid

_DATA_DIR = Path(__file__).resolve().parent / "data"


def load_SO3_grid(resolution: int) -> torch.Tensor:
    """xyzw unit quaternions -> [N,3,3] (reference utils/transform_utils.py:27-50; roma.unitquat_to_rotmat formula,
    SURVEY.md App. A.1).  fp32 like the reference (torch.tensor of python floats)."""
    path = _DATA_DIR / f"so3_grid_{resolution}_xyzw.npy"
    assert path.is_file(), f"File {path} not found"
    q = torch.tensor(np.load(path).tolist())  # float32, same rounding as torch.tensor(list of python floats)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1)
    return R.reshape(-1, 3, 3)


def add_instance_id(inputs):
    """reference inference/utils.py:151-171"""
    if "instance_id" in inputs.infos:
        return inputs
    df = inputs.infos.copy()
    df["instance_id"] = df.groupby(["batch_im_id", "label"]).cumcount()
    inputs.infos = df
    return inputs


def filter_detections(detections, labels: Optional[List[str]] = None, one_instance_per_class: bool = False):
    """reference inference/utils.py:174-194"""
    if labels is not None:
        df = detections.infos
        detections = detections[df[df.label.isin(labels)].index.tolist()]
    if one_instance_per_class:
        df = detections.infos.sort_values("score", ascending=False).groupby(["batch_im_id", "label"]).head(1)
        detections = detections[df.index.tolist()]
    return detections


class _Timer:
    def __init__(self):
        self.t0 = time.time()

    def elapsed(self) -> float:
        return time.time() - self.t0


class _StageClock(_Timer):
    """Fences and wall clock of one stage (the "timing" block of PoseEstimator has the semantics)."""

    def __init__(self, cuda_timer: bool):
        self.cuda_timer = cuda_timer
        if cuda_timer:
            torch.cuda.synchronize()
        super().__init__()

    def stop(self, render_time: float, event_sets, timing_str: bool = True) -> dict:
        """-> the stage's render_time / model_time / time (/ timing_str); `render_time` = the host enqueue time, reported without the timer"""
        model_time = 0.0
        if self.cuda_timer:
            torch.cuda.synchronize()
            render_time, model_time = PoseEstimator._sum_events(event_sets)
        elapsed = self.elapsed()
        times = {"render_time": render_time, "model_time": model_time, "time": elapsed}
        if timing_str:
            times["timing_str"] = f"time: {elapsed:.2f}, model_time: {model_time:.2f}, render_time: {render_time:.2f}"
        return times


# One refiner row of the stage's all-gather, per iteration: (name in the returned collection, floats, trailing shape)
_REFINER_ROW = (("poses", 16, (4, 4)), ("poses_input", 16, (4, 4)), ("K_crop", 9, (3, 3)), ("boxes_rend", 4, (4,)), ("boxes_crop", 4, (4,)),
                ("pose_out", 9, (9,)))
_REFINER_ROW_WIDTH = sum(width for _, width, _ in _REFINER_ROW)
assert _REFINER_ROW_WIDTH == 58


def _refiner_row_fields(o) -> dict:
    """the tensors of one PosePredictorOutput that go into its rows of `_REFINER_ROW`"""
    pose_out = o.network_outputs["pose"] if "pose" in o.network_outputs else torch.zeros(o.TCO_output.shape[0], 9, device=o.TCO_output.device)
    return {"poses": o.TCO_output, "poses_input": o.TCO_input, "K_crop": o.K_crop, "boxes_rend": o.boxes_rend, "boxes_crop": o.boxes_crop,
            "pose_out": pose_out}


class PoseEstimator(torch.nn.Module):
    """Performs inference for pose estimation."""

    def __init__(self, refiner_model: Optional[torch.nn.Module] = None, coarse_model: Optional[torch.nn.Module] = None,
                 detector_model: Optional[torch.nn.Module] = None, depth_refiner=None, bsz_objects: int = 8, bsz_images: int = 256,
                 SO3_grid_size: int = 576, max_rows_per_launch: int = 576, strict_batching: bool = False,
                 distributed: bool = False, n_streams: int = 1) -> None:
        super().__init__()
        self.coarse_model = coarse_model
        self.refiner_model = refiner_model
        self.detector_model = detector_model
        self.depth_refiner = depth_refiner
        self.bsz_objects = bsz_objects
        self.bsz_images = bsz_images
        self.max_rows_per_launch = max_rows_per_launch
        self.strict_batching = strict_batching
        self.distributed = distributed
        self.n_streams = max(1, int(n_streams))  # chunks are interleaved over this many HIP streams (tails / HBM-bound phases of
        self.min_rows_per_stream = 64             # one chunk overlap the MFMA work of the other)
        self._side_streams: List[torch.cuda.Stream] = []
        if self.refiner_model is not None:
            self.cfg = self.refiner_model.cfg
            self.mesh_db = self.refiner_model.mesh_db
        elif self.coarse_model is not None:
            self.cfg = self.coarse_model.cfg
            self.mesh_db = self.coarse_model.mesh_db
        else:
            raise ValueError("At least one of refiner_model or coarse_model must be specified.")
        self._extents: Optional[torch.Tensor] = None
        if SO3_grid_size is not None:
            self.load_SO3_grid(SO3_grid_size)
        self.eval()
        self.keep_all_outputs = False
        self.keep_all_coarse_outputs = False
        self.refiner_outputs = None
        self.coarse_outputs = None
        self.debug_dict: dict = dict()

    def load_SO3_grid(self, grid_size: int) -> None:
        self._SO3_grid = load_SO3_grid(grid_size).cuda()
        self._extents = None

    @property
    def render_dtype(self) -> torch.dtype:
        """torch.float32 (reference arithmetic, default) or torch.float16 = the "fp16 renders" mode of BASELINE.json configs[4]: both
        pose models store their CNN input (renders + observation crop) as binary16 (`PosePredictor.render_dtype`)."""
        m = self.refiner_model if self.refiner_model is not None else self.coarse_model
        return getattr(m, "render_dtype", torch.float32)

    @render_dtype.setter
    def render_dtype(self, dtype: torch.dtype) -> None:
        for m in (self.coarse_model, self.refiner_model):
            if m is not None:
                m.render_dtype = dtype

    # -- helpers -------------------------------------------------------------------------------------------------
    def _chunk(self, reference_bsz: int) -> int:
        return reference_bsz if self.strict_batching else max(self.max_rows_per_launch, 1)

    def _plan(self, n_rows: int, reference_bsz: int) -> Tuple[int, List[torch.cuda.Stream]]:
        """(rows per chunk, streams to interleave the chunks on).  With >= 2 streams a stage is cut into at least that many
        chunks; every stream has its own CNN-input / backbone / raster workspaces (`slot`)."""
        chunk = self._chunk(reference_bsz)
        ns = 1 if self.strict_batching else self.n_streams
        if ns > 1 and n_rows >= ns * self.min_rows_per_stream:
            chunk = min(chunk, -(-n_rows // ns))
        else:
            ns = 1
        cur = torch.cuda.current_stream()
        if ns == 1:
            return chunk, [cur]
        while len(self._side_streams) < ns:
            self._side_streams.append(torch.cuda.Stream())
        streams = self._side_streams[:ns]
        for st in streams:
            st.wait_stream(cur)
        return chunk, streams

    @staticmethod
    def _join(streams: List[torch.cuda.Stream], tensors) -> None:
        """make the current stream wait for the side streams and adopt the tensors they produced"""
        cur = torch.cuda.current_stream()
        for st in streams:
            if st is not cur:
                cur.wait_stream(st)
        if len(streams) > 1 or (streams and streams[0] is not cur):
            for t in tensors:
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(cur)

    def _grid_extents(self) -> torch.Tensor:
        if self._extents is None:  # [n_obj, M, 2]: depends only on (mesh, rotation) -- cosypose_ops.py:198-208
            self._extents = eng.init_extents(self.mesh_db.points, self._SO3_grid)
        return self._extents

    def _is_sharded(self) -> bool:
        return self.distributed and mpdist.world_size() > 1

    def _shard(self, n: int) -> np.ndarray:
        return mpdist.shard_indices(n, mpdist.rank(), mpdist.world_size()) if self._is_sharded() else np.arange(n)

    def _gather(self, local: torch.Tensor, n: int) -> torch.Tensor:
        return mpdist.gather_rows(local, n, mpdist.rank(), mpdist.world_size()) if self._is_sharded() else local

    def _run_chunks(self, n_rows: int, reference_bsz: int, run_chunk) -> Tuple[list, List[torch.cuda.Stream], int]:
        """`run_chunk(rows slice, slot)` for every chunk of this rank's `n_rows` rows, chunk ci under stream ci % n_streams ->
        (per-chunk results, streams, rows per chunk).  Call it after the stage's input tensors have been enqueued: the side
        streams wait for them (`_plan`)."""
        chunk, streams = self._plan(n_rows, reference_bsz)
        results = []
        for ci, s in enumerate(range(0, n_rows, chunk)):
            slot = ci % len(streams)
            with torch.cuda.stream(streams[slot]):
                results.append(run_chunk(slice(s, min(s + chunk, n_rows)), slot))
        return results, streams, chunk

    def _row_tables(self, observation: ObservationTensor, infos: pd.DataFrame, poses: torch.Tensor):
        """Index tables of a stage over pose rows -> (labels of this rank's rows, K_all [R,3,3], and K / poses / image ids of this
        rank's rows).  The labels stay host copies: no D2H read-back inside the chunk loop."""
        device = observation.images.device
        labels_all = infos["label"].tolist()
        rows_h = self._shard(len(labels_all))
        im_all = torch.as_tensor(infos["batch_im_id"].values.astype(np.int32), device=device)
        rows = torch.as_tensor(rows_h, device=device, dtype=torch.long)
        poses = poses.to(device=device, dtype=torch.float32)
        K_all = observation.K[im_all.long()].float()
        return [labels_all[i] for i in rows_h], K_all, K_all[rows], poses[rows], im_all[rows]

    def _coarse_pass(self, observation: ObservationTensor, labels: List[str], K_rows: torch.Tensor, poses_rows: torch.Tensor,
                     im_rows: torch.Tensor, cuda_timer: bool, return_debug_data: bool):
        """The coarse model over this rank's rows, in chunks -> (logits [rows,1], scores [rows,1], debug data (crops / renders
        [rows,C,h,w], or empty), host render time, event sets, number of chunks).  An empty shard gives zero-row tensors."""
        def run(sl: slice, slot: int):
            return self.coarse_model.forward_coarse(images=observation.images, K=K_rows[sl], labels=labels[sl], TCO_input=poses_rows[sl],
                                                    cuda_timer=cuda_timer, return_debug_data=return_debug_data, im_ids=im_rows[sl],
                                                    slot=slot, defer_timing=True)
        outs, streams, _ = self._run_chunks(len(labels), self.bsz_images, run)
        keys = ("logits", "scores") + (("images_crop", "renders") if return_debug_data else ())
        parts = {k: [o[k] for o in outs] for k in keys}
        self._join(streams, [t for k in keys for t in parts[k]])
        logits, scores = (torch.cat(parts[k]) if outs else torch.zeros(0, 1, device=K_rows.device) for k in keys[:2])
        debug_data = {k: torch.cat(parts[k]) for k in keys[2:]}
        return logits, scores, debug_data, sum((o["render_time"] for o in outs), 0.0), [o["events"] for o in outs], len(outs)

    # -- timing ---------------------------------------------------------------------------------------------------
    # Reference semantics (pose_estimator.py:274-275, 422-423; training/utils.py:224-264): `model_time` is a CUDA-event time that is
    # only measured with cuda_timer=True (0.0 otherwise), `render_time` and `time` are host wall clocks around SYNCHRONOUS work.
    # Here every launch is asynchronous, so: cuda_timer=True -> each stage synchronises at its start and end and reports DEVICE
    # times (render_time / model_time = sums of per-chunk HIP-event intervals around the raster+crop launch and the backbone,
    # time = wall clock of the fenced stage); cuda_timer=False -> nothing synchronises, model_time = 0.0 like the reference and
    # render_time / time are HOST ENQUEUE times (they say how long the host was busy, not how long the GPU took).
    @staticmethod
    def _sum_events(event_sets) -> Tuple[float, float]:
        from .pose_rigid import PosePredictor

        r = m = 0.0
        for ev in event_sets:
            dr, dm = PosePredictor.step_times(ev)
            r += dr
            m += dm
        return r, m

    # -- coarse ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_coarse_model(self, observation: ObservationTensor, detections: DetectionsType, cuda_timer: bool = False,
                             return_debug_data: bool = False) -> Tuple[PoseEstimatesType, dict]:
        clock = _StageClock(cuda_timer)
        assert_detections_valid(detections)
        if return_debug_data and self._is_sharded():
            raise NotImplementedError("return_debug_data with distributed=True: crops/renders are shard-local (rows rank::world); "
                                      "run the debug call on one rank with distributed=False")
        device = observation.images.device
        B, M = len(detections), self._SO3_grid.shape[0]
        df = detections.infos
        # one row per (detection, grid rotation); detection-major, hypothesis-minor (pose_estimator.py:350-360)
        df_h = df.loc[df.index.repeat(M)].copy()
        df_h["hypothesis_id"] = np.tile(np.arange(M), B)
        df_h["bbox_id"] = np.repeat(df.index.values, M)
        n = B * M
        labels_det = df["label"].tolist()
        im_det = df["batch_im_id"].values.astype(np.int32)
        rows_h = self._shard(n)                       # host copies of every index table: no D2H read-back inside the chunk loop
        det_h = rows_h // M
        det_mesh = torch.tensor(self.mesh_db.ids(labels_det), dtype=torch.int32, device=device)
        det_of_row = torch.as_tensor(det_h, device=device, dtype=torch.long)
        rot_of_row = torch.as_tensor((rows_h % M).astype(np.int32), device=device)
        im_of_row = torch.as_tensor(im_det[det_h], device=device)
        bboxes_all = detections.bboxes.to(device=device, dtype=torch.float32)
        K_rows = observation.K[im_of_row.long()].float()
        TCO_local = eng.init_poses_from_boxes(bboxes_all[det_of_row], K_rows, det_mesh[det_of_row], rot_of_row, self._SO3_grid,
                                              self._grid_extents())
        # after the inputs above are enqueued: side streams wait for them
        logits, scores, debug_data, render_time, event_sets, n_batches = self._coarse_pass(
            observation, [labels_det[i] for i in det_h], K_rows, TCO_local, im_of_row, cuda_timer, return_debug_data)
        packed = self._gather(torch.cat([TCO_local.flatten(1), logits, scores], dim=1), n)  # [rows, 18]
        TCO = packed[:, :16].reshape(n, 4, 4).contiguous()
        logits = packed[:, 16].reshape(B, M)
        scores = packed[:, 17].reshape(B, M)
        bboxes = bboxes_all[torch.arange(n, device=device) // M]
        debug_data = {k: v.reshape([B, M, -1, *v.shape[-2:]]) for k, v in debug_data.items()}
        host = torch.stack([logits.flatten(), scores.flatten()]).cpu().numpy()  # the stage's single D2H sync
        df_h["coarse_logit"] = host[0]
        df_h["coarse_score"] = host[1]
        extra_data = {**clock.stop(render_time, event_sets), "logits": logits, "scores": scores, "TCO": TCO.reshape([B, M, 4, 4]),
                      "debug": debug_data, "n_batches": n_batches}
        return PandasTensorCollection(df_h, poses=TCO, bboxes=bboxes), extra_data

    # -- refiner --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_refiner(self, observation: ObservationTensor, data_TCO_input: PoseEstimatesType, n_iterations: int = 5,
                        keep_all_outputs: bool = False, cuda_timer: bool = False, **refiner_kwargs) -> Tuple[dict, dict]:
        clock = _StageClock(cuda_timer)
        assert self.refiner_model is not None
        if keep_all_outputs and self._is_sharded():
            raise NotImplementedError("keep_all_outputs with distributed=True: the per-batch outputs are shard-local")
        R = data_TCO_input.poses.shape[0]
        df = data_TCO_input.infos.copy()  # the reference adds these two columns to its per-batch copies (:155-156)
        labels, K_all, K_rows, poses_rows, im_rows = self._row_tables(observation, df, data_TCO_input.poses)

        def run(sl: slice, slot: int):
            return self.refiner_model(images=observation.images, K=K_rows[sl], TCO=poses_rows[sl], n_iterations=n_iterations,
                                      labels=labels[sl], im_ids=im_rows[sl], materialize=keep_all_outputs, slot=slot,
                                      cuda_timer=cuda_timer, **refiner_kwargs)
        # after the inputs above are enqueued (side streams wait for them)
        chunk_outputs, streams, chunk = self._run_chunks(len(labels), self.bsz_objects, run)
        df["refiner_batch_idx"] = np.arange(R) // chunk
        df["refiner_instance_idx"] = np.arange(R) % chunk
        steps = [o for outputs_ in chunk_outputs for o in outputs_.values()]   # chunk-major, iteration-minor
        self._join(streams, [t for o in steps for t in (o.TCO_output, o.TCO_input, o.KV_crop, o.boxes_rend, o.boxes_crop, o.renders,
                                                        o.images_crop, *o.network_outputs.values())])
        # ONE all-gather for the whole stage: the 58 floats of every iteration side by side, [rows, n_iterations * 58]
        W = _REFINER_ROW_WIDTH
        if labels:
            fields = {n: [_refiner_row_fields(outputs_[f"iteration={n}"]) for outputs_ in chunk_outputs] for n in range(1, n_iterations + 1)}
            packed_all = torch.cat([torch.cat([f[name] for f in fields[n]]).flatten(1) for n in range(1, n_iterations + 1)
                                    for name, _, _ in _REFINER_ROW], dim=1)
        else:
            packed_all = torch.zeros(0, W * n_iterations, device=observation.images.device)
        packed_all = self._gather(packed_all, R)
        preds = dict()
        pose_outputs = dict()
        for n in range(1, n_iterations + 1):
            cols, o = {}, (n - 1) * W
            for name, width, shape in _REFINER_ROW:
                cols[name] = packed_all[:, o:o + width].reshape(R, *shape).contiguous()
                o += width
                if name == "K_crop":
                    cols["K"] = K_all   # (not gathered: every rank has it; registered after K_crop, the order callers have always seen)
            pose_outputs[f"iteration={n}"] = cols.pop("pose_out")
            preds[f"iteration={n}"] = PandasTensorCollection(df, **cols)
        times = clock.stop(sum((o.timing_dict["render"] for o in steps), 0.0), [o.timing_dict.get("events") for o in steps],
                           timing_str=False)   # (this stage reports none, like the reference's)
        # `pose_outputs` (engine extension): the refiner network's raw 9-vector per row and iteration, [R, 9] -- what the parity
        # checks compare before the pose update damps it (PosePredictorOutput.network_outputs["pose"], pose_rigid.py:50-66)
        extra_data = {"n_iterations": n_iterations, "outputs": chunk_outputs if keep_all_outputs else [], **times, "pose_outputs": pose_outputs}
        return preds, extra_data

    # -- scoring --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_scoring_model(self, observation: ObservationTensor, data_TCO: PoseEstimatesType, cuda_timer: bool = False,
                              return_debug_data: bool = False) -> Tuple[PoseEstimatesType, dict]:
        """Adds 'pose_logit' / 'pose_score' to data_TCO.infos (modifies the collection in place, :217-322)."""
        clock = _StageClock(cuda_timer)
        assert self.coarse_model is not None
        if return_debug_data and self._is_sharded():
            raise NotImplementedError("return_debug_data with distributed=True: crops/renders are shard-local (rows rank::world)")
        df = data_TCO.infos
        labels, _, K_rows, poses_rows, im_rows = self._row_tables(observation, df, data_TCO.poses)
        # after the inputs above are enqueued: side streams wait for them
        logits, scores, debug_data, render_time, event_sets, n_batches = self._coarse_pass(
            observation, labels, K_rows, poses_rows, im_rows, cuda_timer, return_debug_data)
        packed = self._gather(torch.cat([logits, scores], dim=1), len(df))  # [rows, 2]
        logits, scores = packed[:, 0:1].contiguous(), packed[:, 1:2].contiguous()
        host = packed.cpu().numpy()
        df["pose_logit"] = host[:, 0]
        df["pose_score"] = host[:, 1]
        extra_data = {**clock.stop(render_time, event_sets), "logits": logits, "scores": scores, "debug": debug_data, "n_batches": n_batches}
        data_TCO.infos = df
        return data_TCO, extra_data

    @torch.no_grad()
    def forward_detection_model(self, observation: ObservationTensor, *args: Any, **kwargs: Any) -> DetectionsType:
        if self.detector_model is None:
            raise ValueError("no detector model: pass `detections` (the 2D detector is out of the hot-path scope)")
        return self.detector_model.get_detections(observation, *args, **kwargs)

    def run_depth_refiner(self, observation: ObservationTensor, predictions: PoseEstimatesType) -> Tuple[PoseEstimatesType, dict]:
        assert self.depth_refiner is not None, "You must specify a depth refiner"
        return self.depth_refiner.refine_poses(predictions, depth=observation.depth, K=observation.K)

    # -- pipeline -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def run_inference_pipeline(self, observation: ObservationTensor, detections: Optional[DetectionsType] = None,
                               run_detector: Optional[bool] = None, n_refiner_iterations: int = 5, n_pose_hypotheses: int = 1,
                               keep_all_refiner_outputs: bool = False, detection_filter_kwargs: Optional[dict] = None,
                               run_depth_refiner: bool = False, bsz_images: Optional[int] = None, bsz_objects: Optional[int] = None,
                               cuda_timer: bool = False, coarse_estimates: Optional[PoseEstimatesType] = None
                               ) -> Tuple[PoseEstimatesType, dict]:
        timing_str = ""
        timer = _Timer()
        if bsz_images is not None:
            self.bsz_images = bsz_images
        if bsz_objects is not None:
            self.bsz_objects = bsz_objects
        if coarse_estimates is None:
            assert detections is not None or run_detector, "You must either pass in `detections` or set run_detector=True"
            if detections is None and run_detector:
                t = time.time()
                detections = self.forward_detection_model(observation).cuda()
                timing_str += f"detection={time.time() - t:.2f}, "
            assert detections is not None
            detections = add_instance_id(detections)
            if detection_filter_kwargs is not None:
                detections = filter_detections(detections, **detection_filter_kwargs)
            data_TCO_coarse, coarse_extra_data = self.forward_coarse_model(observation=observation, detections=detections,
                                                                           cuda_timer=cuda_timer)
            timing_str += f"coarse={coarse_extra_data['time']:.2f}, "
            data_TCO_filtered = self.filter_pose_estimates(data_TCO_coarse, top_K=n_pose_hypotheses, filter_field="coarse_logit")
        else:
            data_TCO_coarse = coarse_estimates
            coarse_extra_data = None
            data_TCO_filtered = coarse_estimates
        preds, refiner_extra_data = self.forward_refiner(observation, data_TCO_filtered, n_iterations=n_refiner_iterations,
                                                         keep_all_outputs=keep_all_refiner_outputs, cuda_timer=cuda_timer)
        data_TCO_refined = preds[f"iteration={n_refiner_iterations}"]
        timing_str += f"refiner={refiner_extra_data['time']:.2f}, "
        data_TCO_scored, scoring_extra_data = self.forward_scoring_model(observation, data_TCO_refined, cuda_timer=cuda_timer)
        timing_str += f"scoring={scoring_extra_data['time']:.2f}, "
        data_TCO_final_scored = self.filter_pose_estimates(data_TCO_scored, top_K=1, filter_field="pose_logit")
        if run_depth_refiner:
            t = time.time()
            data_TCO_depth_refiner, _ = self.run_depth_refiner(observation, data_TCO_final_scored)
            data_TCO_final = data_TCO_depth_refiner
            timing_str += f"depth refiner={time.time() - t:.2f}"
        else:
            data_TCO_depth_refiner = None
            data_TCO_final = data_TCO_final_scored
        total = timer.elapsed()
        timing_str = f"total={total:.2f}, {timing_str}"
        extra_data: dict = dict()
        extra_data["coarse"] = {"preds": data_TCO_coarse, "data": coarse_extra_data}
        extra_data["coarse_filter"] = {"preds": data_TCO_filtered}
        extra_data["refiner_all_hypotheses"] = {"preds": preds, "data": refiner_extra_data}
        extra_data["scoring"] = {"preds": data_TCO_scored, "data": scoring_extra_data}
        extra_data["refiner"] = {"preds": data_TCO_final_scored, "data": refiner_extra_data}
        extra_data["timing_str"] = timing_str
        extra_data["time"] = total
        if run_depth_refiner:
            extra_data["depth_refiner"] = {"preds": data_TCO_depth_refiner}
        return data_TCO_final, extra_data

    def filter_pose_estimates(self, data_TCO: PoseEstimatesType, top_K: int, filter_field: str, ascending: bool = False) -> PoseEstimatesType:
        """Keep the top_K rows per (batch_im_id, label, instance_id) by `filter_field` (:643-667).  The sort is made
        stable so that exact ties resolve deterministically (lowest row first); the reference's default quicksort leaves
        tie order unspecified."""
        t0 = time.perf_counter()
        df = data_TCO.infos
        keep = _topk_rows_fast(df, top_K, filter_field, ascending)
        if keep is None:   # (scores with NaN, non-integer ids, ids beyond the packed key's range: the plain pandas form)
            group_cols = ["batch_im_id", "label", "instance_id"]
            keep = df.sort_values(filter_field, ascending=ascending, kind="stable").groupby(group_cols).head(top_K).index.to_numpy()
        out = data_TCO[keep.tolist()]
        mpdist.stats.host_s += time.perf_counter() - t0   # (replicated on every rank: bench.py reports its share of a step)
        return out


def _topk_rows_fast(df, top_K: int, field: str, ascending: bool):
    """Row positions `df.sort_values(field, kind="stable").groupby([batch_im_id, label, instance_id]).head(top_K)` keeps, in that order,
    without pandas' group-by (1.1 -> 0.2 ms on a 576-row table, 15 -> 9 ms on 36 864 rows; every rank of a multi-GPU run repeats it, so it
    is the part of a step that does not shrink with the world size).  Integer group key = batch_im_id | instance_id | factorised label;
    None when that key cannot be formed -- the caller then uses the pandas form, which this reproduces row for row (ties keep the lower
    row first, as the stable sort does: tests/test_host_cpu.py)."""
    import pandas as pd

    if len(df) == 0 or df.index.dtype.kind not in "iu" or not df.index.is_unique:
        return None
    v = df[field].to_numpy()
    c1, c3 = df["batch_im_id"].to_numpy(), df["instance_id"].to_numpy()
    if v.dtype.kind != "f" or c1.dtype.kind not in "iu" or c3.dtype.kind not in "iu" or np.isnan(v).any():
        return None
    c2 = pd.factorize(df["label"].to_numpy())[0]
    if c1.min() < 0 or c1.max() >= 1 << 22 or c3.min() < 0 or c3.max() >= 1 << 24 or c2.min() < 0 or c2.max() >= 1 << 16:
        return None
    n = len(v)
    codes = (c1.astype(np.int64) << 40) | (c3.astype(np.int64) << 16) | c2.astype(np.int64)
    order = np.argsort(v if ascending else -v, kind="stable")   # (negation keeps ties in row order, like ascending=False of a stable sort)
    cs = codes[order]
    o2 = np.argsort(cs, kind="stable")
    sc = cs[o2]
    start = np.r_[True, sc[1:] != sc[:-1]]
    first = np.maximum.accumulate(np.where(start, np.arange(n), 0))
    rank = np.empty(n, dtype=np.int64)
    rank[o2] = np.arange(n) - first
    return df.index.to_numpy()[order[rank < top_K]]


# name used by BASELINE.json's north_star; the reference snapshot only has PoseEstimator
CoarseRefinePoseEstimator = PoseEstimator
