#!/usr/bin/env python3
"""Time the TEASER++ depth refiner (engine.teaser_refine: csrc/teaser.hip) stage by stage at the shape of BASELINE config 5, next to the
ICP refiner on the same scenes and the float64 restatement on the CPU.

  workload  --frames frames (8) of 640 x 480 with --per-frame detections each (8) over 16 lathe meshes: the measured depth is the
            z-buffer of the objects at their true poses with 2 mm of noise; the input poses are 2.5 cm off along the viewing ray (the depth
            an RGB-only estimate leaves open: the refiner's correspondences assume the pose is aligned in the image), 1 mm sideways and
            a degree turned
  whole     engine.teaser_refine (six launches) with farthest point sampling, and with strided sampling instead
  sampling  engine.farthest_point_sample on the rows' mask points (the same kernel, the same point sets)
  solve     engine.teaser_solve on the sampled correspondences (graph, cores, GNC-TLS, voting, inlier count), both TIM graphs
  class     TeaserppRefiner.refine_poses and ICPRefiner.refine_poses (each renders the depth of every row first)
  cpu       the float64 numpy restatement (tests/support/teaser.py) on --cpu-rows rows, wall clock per row

Device-event times after a warm-up launch, best of --reps; one header line, then one JSON line.  No figure is a gate.

Usage: python scripts/bench_teaser_refiner.py [--reps 5] [--frames 8] [--per-frame 8] [--cpu-rows 2]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import pandas as pd
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
sys.path.insert(0, str(ROOT / "tests"))

from bench_bop_match import timed  # noqa: E402
from megapose6d_amd import engine as eng  # noqa: E402
from megapose6d_amd.icp_refiner import ICPRefiner, TeaserppRefiner  # noqa: E402
from megapose6d_amd.renderer import Panda3dBatchRenderer  # noqa: E402
from megapose6d_amd.tcoll import PandasTensorCollection  # noqa: E402
from support import synthetic as syn  # noqa: E402
from support import teaser as ts  # noqa: E402


def build_scenes(n_frames: int, per_frame: int):
    """the workload of the docstring -> dict(renderer, labels, im_ids, gt, depth [frames,H,W], ids, K_im, K_rows, TCO (the input poses), rend)"""
    H, W, n_meshes = 480, 640, 16
    ds = syn.make_object_dataset(tempfile.mkdtemp(prefix="mp_bench_teaser_"), n_objects=n_meshes, seed=40, n_theta=48, n_z=50)
    renderer = Panda3dBatchRenderer(ds, n_workers=1)
    names = [o.label for o in ds.list_objects]
    rng = np.random.RandomState(9)
    K = torch.from_numpy(syn.K_EXAMPLE.astype(np.float32)).cuda()
    labels, im_ids, gt, frames = [], [], [], []
    for f in range(n_frames):
        labs = [names[(2 * f + j) % n_meshes] for j in range(per_frame)]
        poses = np.stack([syn.random_pose(rng, (0.5, 0.8), 0.3) for _ in labs]).astype(np.float32)
        d = renderer.render_depth(labs, torch.from_numpy(poses).cuda(), K[None].repeat(len(labs), 1, 1), (H, W))
        z = torch.where(d > 0, d, torch.full_like(d, float("inf"))).min(0).values
        z = torch.where(torch.isinf(z), torch.zeros_like(z), z)
        noise = (torch.randn(H, W, generator=torch.Generator().manual_seed(f)) * 0.002).cuda()
        frames.append(torch.where(z > 0, z + noise, z))
        labels += labs
        im_ids += [f] * len(labs)
        gt.append(poses)
    gt = np.concatenate(gt)
    init = gt.copy()
    for n in range(len(init)):
        init[n, :3, :3] = (ts.rotation(rng.normal(size=3), np.deg2rad(1.0)) @ gt[n, :3, :3]).astype(np.float32)
        init[n, :3, 3] = gt[n, :3, 3] * np.float32(1.0 + 0.025 / np.linalg.norm(gt[n, :3, 3])) + np.float32([0.001, -0.001, 0.0])
    depth = torch.stack(frames)
    n = len(labels)
    ids = torch.tensor(im_ids, dtype=torch.int32).cuda()
    K_im = K[None].repeat(n_frames, 1, 1)
    K_rows = K_im[ids.long()]
    TCO = torch.from_numpy(init).cuda()
    rend = renderer.render_depth(labels, TCO, K_rows, (H, W)).contiguous()
    return dict(renderer=renderer, labels=labels, im_ids=im_ids, gt=gt, depth=depth, ids=ids, K_im=K_im, K_rows=K_rows, TCO=TCO, rend=rend, H=H, W=W)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--per-frame", type=int, default=8)
    ap.add_argument("--cpu-rows", type=int, default=2)
    args = ap.parse_args()
    n_cu, _, arch = eng.device_info()
    sc = build_scenes(args.frames, args.per_frame)
    renderer, labels, im_ids, gt, depth, ids, K_im, K_rows, TCO, rend, H, W = (sc[k] for k in ("renderer", "labels", "im_ids", "gt", "depth", "ids", "K_im", "K_rows", "TCO",
                                                                                               "rend", "H", "W"))
    n = len(labels)
    print(f"# {arch}, {n_cu} CUs; {n} detections over {args.frames} frames of {W} x {H}; best of {args.reps} after a warm-up")

    out = {}
    out["refine_fps_ms"] = timed(lambda: eng.teaser_refine(depth, ids, rend, K_rows, TCO), args.reps)
    out["refine_strided_ms"] = timed(lambda: eng.teaser_refine(depth, ids, rend, K_rows, TCO, use_farthest_point_sampling=False), args.reps)
    out["refine_complete_ms"] = timed(lambda: eng.teaser_refine(depth, ids, rend, K_rows, TCO, rotation_tim_graph="complete"), args.reps)
    poses, retval, info, tel = eng.teaser_refine(depth, ids, rend, K_rows, TCO, telemetry=True)
    # the stages on their own inputs: the rows' mask points in torch (row-major order), then the sampled correspondences
    meas = depth[ids.long()]
    mask = (meas > 0) & (rend > 0)
    v, u = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")

    def cloud(d):
        return torch.stack([(u - K_rows[:, 0, 2, None, None]) * (d / K_rows[:, 0, 0, None, None]),
                            (v - K_rows[:, 1, 2, None, None]) * (d / K_rows[:, 1, 1, None, None]), d], -1)

    src_all, dst_all = cloud(rend), cloud(meas)
    counts = mask.flatten(1).sum(1).to(torch.int32)
    stride = int(counts.max())
    packed_s, packed_d = torch.zeros(n, stride, 3, device="cuda"), torch.zeros(n, stride, 3, device="cuda")
    for r in range(n):
        packed_s[r, : int(counts[r])], packed_d[r, : int(counts[r])] = src_all[r][mask[r]], dst_all[r][mask[r]]
    same = torch.equal(counts, info[:, 0])
    out["sampling_ms"] = timed(lambda: eng.farthest_point_sample(packed_s, counts, 1000), args.reps)
    idx, m = eng.farthest_point_sample(packed_s, counts, 1000)
    same = same and torch.equal(idx, tel["sample_idx"]) and torch.equal(m, info[:, 1])
    gather = idx.clamp(min=0).long()[..., None].expand(-1, -1, 3)
    cs, cd = torch.gather(packed_s, 1, gather).contiguous(), torch.gather(packed_d, 1, gather).contiguous()
    out["solve_chain_ms"] = timed(lambda: eng.teaser_solve(cs, cd, m, min_num_inliers=50), args.reps)
    out["solve_complete_ms"] = timed(lambda: eng.teaser_solve(cs, cd, m, min_num_inliers=50, rotation_tim_graph="complete"), args.reps)
    Rt, rv = eng.teaser_solve(cs, cd, m, min_num_inliers=50)
    same = same and torch.equal(Rt, tel["Rt"]) and torch.equal(rv, retval)     # the stages timed alone did the work of the whole chain

    preds = PandasTensorCollection(pd.DataFrame(dict(label=labels, batch_im_id=im_ids)), poses=TCO)
    teaser, icp = TeaserppRefiner(None, renderer), ICPRefiner(None, renderer)
    out["teaserpp_refiner_ms"] = timed(lambda: teaser.refine_poses(preds, depth=depth, K=K_im), args.reps)
    out["icp_refiner_ms"] = timed(lambda: icp.refine_poses(preds, depth=depth, K=K_im), max(1, min(args.reps, 2)))
    out["render_depth_ms"] = timed(lambda: renderer.render_depth(labels, TCO, K_rows, (H, W)), args.reps)
    icp_poses = icp.refine_poses(preds, depth=depth, K=K_im)[0].poses

    def t_err(p):
        """translation error against the true poses: median and largest over the detections, metres"""
        e = np.linalg.norm(p.cpu().numpy()[:, :3, 3] - gt[:, :3, 3], axis=1)
        return [float(np.median(e)), float(e.max())]

    t0 = time.perf_counter()
    for r in range(args.cpu_rows):
        ref = ts.ref_refine_row(depth[im_ids[r]].cpu().numpy(), rend[r].cpu().numpy(), K_rows[r].cpu().numpy())
        same = same and ref["Rt"] is not None and float(np.abs(ref["Rt"] - tel["Rt"][r].cpu().numpy()).max()) <= ts.RT_TOL
    out["cpu_restatement_ms_per_row"] = (time.perf_counter() - t0) * 1e3 / max(1, args.cpu_rows)
    out.update(name="teaser_refiner", stages_agree=bool(same), detections=n, mask_points_mean=float(counts.float().mean()), mask_points_max=stride,
               accepted=int((retval == 0).sum()), gnc_iterations_max=int(info[:, 3].max()), translation_error_in_median_max_m=t_err(TCO),
               translation_error_teaserpp_median_max_m=t_err(poses), translation_error_icp_median_max_m=t_err(icp_poses))
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
