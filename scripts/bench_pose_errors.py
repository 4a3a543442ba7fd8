#!/usr/bin/env python3
"""Time the fused pose-error kernels against the reference's own formulation run through torch on the same GPU.

  (i)  symmetry-set error, 4 032 rows x 64 symmetries x 2 000 points (one config-2 refiner table against a can-like object)
  (ii) nearest-neighbour error (ADD-S), 576 rows x 2 000 points and 64 rows x 20 000 points

Device-event times after warm-up.  The torch route is mssd_torch (evaluation/utils.py:175-238) / dists_add_symmetric
(lib3d/distances.py:44-53) restated line by line, chunked over rows -- and over ground-truth points where one row alone does not fit --
only as far as memory forces it; the chunking is part of the printed line.  The fused kernels' rate is also given as a fraction of the
fp32 VALU lane rate (CUs x 4 SIMDs x 16 lanes x clock) at the clock the engine's probe measures under load.

Usage: python scripts/bench_pose_errors.py [--reps 5] [--quick]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from megapose6d_amd import engine as eng  # noqa: E402

SYM_OPS_PER_PAIR = 19     # 9 fma (transform) + 3 sub + 3 mul/fma + sqrt (1) + add + max + select
NN_OPS_PER_PAIR = 9       # 3 sub + 3 mul/fma + compare + 2 selects


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def poses(rng, b):
    q = rng.randn(b, 4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(b, 3, 3)
    T = np.tile(np.eye(4), (b, 1, 1))
    T[:, :3, :3] = R
    T[:, :3, 3] = rng.uniform(-0.2, 0.2, size=(b, 3)) + [0, 0, 0.8]
    return torch.from_numpy(T.astype(np.float32)).cuda()


def transform_points(T, pts):
    return pts @ T[..., :3, :3].transpose(-1, -2) + T[..., None, :3, 3]


def torch_mssd(T_est, T_gt, pts, syms, rows):
    """mssd_torch on `rows` rows at a time"""
    errs = []
    for r0 in range(0, T_est.shape[0], rows):
        Tg = torch.matmul(T_gt[r0:r0 + rows].unsqueeze(1), syms)                                    # [B,S,4,4]
        delta = transform_points(Tg, pts) - transform_points(T_est[r0:r0 + rows], pts).unsqueeze(1)   # [B,S,N,3]
        errs.append(torch.linalg.norm(delta, dim=-1).mean(dim=-1))
    errs = torch.cat(errs)
    return errs.min(dim=-1)


def torch_adds(T_pred, T_gt, pts, rows, gt_chunk):
    """dists_add_symmetric on `rows` rows and `gt_chunk` ground-truth points at a time (the arg-min runs over ALL predicted points)"""
    out = []
    for r0 in range(0, T_pred.shape[0], rows):
        p = transform_points(T_pred[r0:r0 + rows], pts[r0:r0 + rows])
        g = transform_points(T_gt[r0:r0 + rows], pts[r0:r0 + rows])
        cols = []
        for c0 in range(0, g.shape[1], gt_chunk):
            d = g[:, c0:c0 + gt_chunk].unsqueeze(1) - p.unsqueeze(2)                                 # [B, N pred, chunk gt, 3]
            assign = (d ** 2).sum(dim=-1).argmin(dim=1)
            cols.append(torch.gather(d, 1, assign[:, None, :, None].expand(-1, 1, -1, 3)).squeeze(1))
        out.append(torch.cat(cols, dim=1))
    return torch.cat(out)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a tenth of the rows (a functional check, not a measurement)")
    args = ap.parse_args()
    n_cu, _, arch = eng.device_info()
    clock_ghz = eng.clock_probe()["shader_mhz"] / 1e3     # the effective shader clock under load, measured by the engine's probe
    lane_rate = n_cu * 4 * 16 * clock_ghz * 1e9
    free = torch.cuda.mem_get_info()[0]
    budget = min(free // 4, 8 << 30)     # bytes one torch intermediate may take
    rng = np.random.RandomState(0)
    print(f"# {arch}, {n_cu} CUs, {clock_ghz:.2f} GHz -> {lane_rate / 1e12:.1f} T fp32 lane-operations/s; torch chunk budget {budget >> 20} MiB")
    results = []

    b, S, N = (4032 // (10 if args.quick else 1)), 64, 2000
    pts = torch.from_numpy((rng.uniform(-1, 1, size=(N, 3)) * [0.03, 0.03, 0.06]).astype(np.float32)).cuda()
    ang = 2 * np.pi * np.arange(S) / S
    syms = torch.eye(4).repeat(S, 1, 1)
    syms[:, 0, 0] = syms[:, 1, 1] = torch.from_numpy(np.cos(ang)).float()
    syms[:, 0, 1] = torch.from_numpy(-np.sin(ang)).float()
    syms[:, 1, 0] = torch.from_numpy(np.sin(ang)).float()
    syms = syms.cuda()
    T_gt, T_est = poses(rng, b), poses(rng, b)
    ids = torch.zeros(b, dtype=torch.int32, device="cuda")
    fused = lambda: eng.pose_error_sym(T_est, T_gt, syms[None], None, pts[None], mesh_ids=ids)  # noqa: E731
    rows = max(1, min(b, budget // (S * N * 3 * 4 * 3)))     # delta + the two transformed sets it is made of
    ref = lambda: torch_mssd(T_est, T_gt, pts, syms, rows)  # noqa: E731
    t_f, t_r = timed(fused, args.reps), timed(ref, args.reps)
    agree = float((fused()["err"] - ref()[0]).abs().max())
    pairs = b * S * N
    results.append(dict(name="sym", rows=b, S=S, N=N, fused_ms=t_f, torch_ms=t_r, torch_rows_per_chunk=rows, gpairs_per_s=pairs / t_f / 1e6,
                        valu_fraction=pairs * SYM_OPS_PER_PAIR / (t_f * 1e-3) / lane_rate, max_abs_diff=agree))

    for b, N in ((576, 2000), (64, 20000)):
        b = b // (10 if args.quick else 1) or 1
        pts = torch.from_numpy((rng.uniform(-1, 1, size=(b, N, 3)) * [0.03, 0.03, 0.06]).astype(np.float32)).cuda()
        T_gt, T_pred = poses(rng, b), poses(rng, b)
        fused = lambda: eng.pose_error_nn(T_pred, T_gt, pts)  # noqa: E731
        per_row = N * N * 3 * 4 * 3                           # d, d**2 and the gathered copy
        rows = max(1, min(b, budget // per_row))
        gt_chunk = N if per_row <= budget else max(1, budget // (N * 3 * 4 * 3))
        ref = lambda: torch_adds(T_pred, T_gt, pts, rows, gt_chunk)  # noqa: E731
        t_f, t_r = timed(fused, args.reps), timed(ref, max(1, args.reps // 2))
        agree = float((fused()["diffs"].norm(dim=-1) - ref().norm(dim=-1)).abs().max())
        pairs = b * N * N
        results.append(dict(name="adds", rows=b, N=N, fused_ms=t_f, torch_ms=t_r, torch_rows_per_chunk=rows, torch_gt_points_per_chunk=gt_chunk,
                            gpairs_per_s=pairs / t_f / 1e6, valu_fraction=pairs * NN_OPS_PER_PAIR / (t_f * 1e-3) / lane_rate, max_abs_diff=agree))
    for r in results:
        print(json.dumps(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
