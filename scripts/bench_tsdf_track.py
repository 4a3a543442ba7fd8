#!/usr/bin/env python3
"""Time tracking a depth frame against the TSDF (csrc/tsdf_track.hip) against the same arithmetic formulated in torch and against a
copy of the frame, on the same machine.

  workload  the union of three spheres of the tests seen from 16 cameras of their wobbling orbit at 0.4 m, frames of 480 x 640 (f = 600)
            with masks, fused at their true poses into 128^3 and into 256^3 nodes over [-0.066, 0.066]^3; frame 3 is then tracked from
            a pose perturbed by 5 degrees / 5 mm
  (a) the product call: engine.tsdf_track, 10 iterations (eps_rot = eps_trans = 0, so that none is skipped): 21 launches, no read-back
  (b) the same arithmetic in torch on the device: whole-frame float32 operations, eight gathers of sum and count, float64 sums, a
      Cholesky solve and the Cayley map, 10 iterations, no read-back either; its pose is compared with (a)'s and the difference reported
      (torch's sums have another order)
  Before anything is timed, pose, status, used, rms and the records of (a) at the first size are compared bit for bit with the host
  emulation of the tests (tests/tsdf_track_emul.cpp), so the table rests on checked results; a difference ends the run with exit code 1.
  (c) torch.clone of the frame's depth: the floor of anything that reads the frame once

Wall-clock times around a device synchronise, after warm-up; the runs take turns --reps times and the best and the median of each are
reported.  One header line, then one JSON line per volume.

Usage: python scripts/bench_tsdf_track.py [--reps 10] [--sizes 128 256]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from megapose6d_amd import engine as eng  # noqa: E402
from tests.support import tsdf as st  # noqa: E402
from tests.support import tsdf_track as tt  # noqa: E402

H, W, FOCAL, HALF, N_VIEWS, FRAME, ITERS = 480, 640, 600.0, 0.066, 16, 3, 10


def make_views():
    cams = tt.orbit_cameras(N_VIEWS)
    K = st.intrinsics(FOCAL, H, W)
    depth = np.stack([tt.trio_depth(T, K, H, W) for T in cams]).astype(np.float32)
    return dict(depth=depth, masks=(depth > 0).astype(np.uint8), K=np.repeat(K[None], N_VIEWS, 0).astype(np.float32), TCO=cams.astype(np.float32))


def torch_track(vol: torch.Tensor, origin, voxel: float, depth: torch.Tensor, mask: torch.Tensor, K: torch.Tensor, T: torch.Tensor, mu: float,
                iters: int) -> torch.Tensor:
    """the contract's steps (csrc/tsdf_track_core.h) as whole-frame operations: float32 per pixel, float64 sums and solve -> [4,4] float32"""
    _, nz, ny, nx = vol.shape
    dev, f32, f64 = vol.device, torch.float32, torch.float64
    fsum, cnt = vol[0].reshape(-1), vol[1].view(torch.int32).reshape(-1)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=f32), torch.arange(W, device=dev, dtype=f32), indexing="ij")
    org = torch.tensor(origin, dtype=f32, device=dev)
    dims = torch.tensor([nx, ny, nz], dtype=f32, device=dev)
    valid = torch.isfinite(depth) & (depth > 0) & (mask != 0)
    pc = torch.stack([((xs + 0.5) - K[0, 2]) / K[0, 0] * depth, ((ys + 0.5) - K[1, 2]) / K[1, 1] * depth, depth], -1).reshape(-1, 3)
    valid = valid.reshape(-1)
    T = T.clone()
    eye = torch.eye(3, dtype=f64, device=dev)
    for _ in range(iters):
        p = (pc - T[:3, 3]) @ T[:3, :3]
        q = (p - org) / voxel
        i0 = torch.floor(q)
        use = valid & ((i0 >= 0) & (i0 < dims - 1)).all(1)
        u = q - i0
        ii = torch.where(use[:, None], i0, torch.zeros_like(i0)).long()
        Fc = []
        for code in range(8):
            at = ((ii[:, 2] + ((code >> 2) & 1)) * ny + ii[:, 1] + ((code >> 1) & 1)) * nx + ii[:, 0] + (code & 1)
            c = cnt[at]
            use = use & (c >= 1)
            Fc.append(fsum[at] / c.to(f32))
        lerp = lambda a, b, t: a + t * (b - a)   # noqa: E731
        c00, c10, c01, c11 = lerp(Fc[0], Fc[1], u[:, 0]), lerp(Fc[2], Fc[3], u[:, 0]), lerp(Fc[4], Fc[5], u[:, 0]), lerp(Fc[6], Fc[7], u[:, 0])
        c0, c1 = lerp(c00, c10, u[:, 1]), lerp(c01, c11, u[:, 1])
        f = lerp(c0, c1, u[:, 2])
        use = use & (f.abs() < 1)
        dx = lerp(lerp(Fc[1] - Fc[0], Fc[3] - Fc[2], u[:, 1]), lerp(Fc[5] - Fc[4], Fc[7] - Fc[6], u[:, 1]), u[:, 2])
        gm = torch.stack([dx, lerp(c10 - c00, c11 - c01, u[:, 2]), c1 - c0], 1) / voxel * mu
        J = torch.cat([torch.cross(p, gm, dim=1), gm], 1).to(f64)
        r = (f * mu).to(f64)
        J = torch.where(use[:, None], J, torch.zeros_like(J))
        r = torch.where(use, r, torch.zeros_like(r))
        A = J.T @ J + 1e-9 * use.sum().to(f64) * torch.eye(6, dtype=f64, device=dev)
        x = -torch.cholesky_solve((J.T @ r)[:, None], torch.linalg.cholesky(A))[:, 0]
        a, v = 0.5 * x[:3], x[3:]
        zero = torch.zeros((), dtype=f64, device=dev)
        skew = torch.stack([torch.stack([zero, -a[2], a[1]]), torch.stack([a[2], zero, -a[0]]), torch.stack([-a[1], a[0], zero])])
        aa = a @ a
        Rc = ((1 - aa) * eye + 2 * torch.outer(a, a) + 2 * skew) / (1 + aa)
        R = T[:3, :3].to(f64)
        Rn = R @ Rc.T
        tn = T[:3, 3].to(f64) - Rn @ v
        r0 = Rn[0] / Rn[0].norm()
        e = Rn[1] - (Rn[1] @ r0) * r0
        r1 = e / e.norm()
        T[:3, :3] = torch.stack([r0, r1, torch.linalg.cross(r0, r1)]).to(f32)
        T[:3, 3] = tn.to(f32)
    return T


def wall_once(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    args = ap.parse_args()
    host = make_views()
    views = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    start_h = (tt.orbit_cameras(N_VIEWS)[FRAME] @ tt.perturbation(7, 5.0, 5.0)).astype(np.float32)
    start = torch.from_numpy(start_h).cuda()[None]
    depth, mask, K = views["depth"][FRAME:FRAME + 1], views["masks"][FRAME:FRAME + 1], views["K"][FRAME:FRAME + 1]
    n_cu, _, arch = eng.device_info()
    print(f"# {arch}, {n_cu} CUs; one frame of {H} x {W} ({int(mask.sum())} masked pixels, {eng.tsdf_track_groups(H, W)} groups) tracked for {ITERS} "
          f"iterations against a volume fused from {N_VIEWS} views; {args.reps} reps in turn, wall clock around a synchronise")
    ok = True
    for n in args.sizes:
        g = st.cube_grid(n, HALF)
        mu = float(g.mu3)
        vol = eng.tsdf_volume(g.dims, False, "cuda")
        eng.tsdf_integrate(vol, g.origin, g.voxel, views["depth"], views["K"], views["TCO"], views["masks"], mu=mu, z_min=st.Z_MIN)
        part = torch.zeros(1, eng.tsdf_track_groups(H, W), eng.TSDF_TRACK_RECORD, dtype=torch.float64, device="cuda")

        def track():
            return eng.tsdf_track(vol, g.origin, g.voxel, depth, K, start, mask, mu=mu, iters=ITERS, eps_rot=0.0, eps_trans=0.0, partials=part)

        pose, status, used, rms = track()
        agree_emulation = None
        if n == args.sizes[0]:                                     # the host emulation, bit for bit
            want = tt.emul_track(vol.cpu().numpy(), g, host["depth"][FRAME:FRAME + 1], host["masks"][FRAME:FRAME + 1], host["K"][FRAME:FRAME + 1],
                                 start_h[None], iters=ITERS, mu=mu, eps_rot=0.0, eps_tr=0.0)
            agree_emulation = bool(want.rc == 0 and np.array_equal(pose.cpu().numpy().reshape(1, 16).view(np.uint32), want.TCO.view(np.uint32))
                                   and status.tolist() == want.status.tolist() and used.tolist() == want.used.tolist()
                                   and np.array_equal(rms.cpu().numpy().view(np.uint32), want.rms.view(np.uint32))
                                   and np.array_equal(part.cpu().numpy().view(np.uint64), want.records.view(np.uint64)))
            ok = ok and agree_emulation
        ref = torch_track(vol, g.origin, g.voxel, depth[0], mask[0], K[0], start[0], mu, ITERS)
        pose_diff = float((ref - pose[0]).abs().max())
        truth = tt.orbit_cameras(N_VIEWS)[FRAME]
        runs = {"track": track, "torch_track": lambda: torch_track(vol, g.origin, g.voxel, depth[0], mask[0], K[0], start[0], mu, ITERS),
                "clone": lambda: depth.clone()}
        for fn in runs.values():
            fn()
        times = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, fn in runs.items():
                times[k].append(wall_once(fn))
        best = {k: min(v) for k, v in times.items()}
        median = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps(dict(name="tsdf_track", side=n, nodes=n ** 3, H=H, W=W, iters=ITERS, reps=args.reps, status=int(status[0]), used=int(used[0]),
                              rms_mm=float(rms[0]) * 1e3, start_displacement_voxel=tt.displacement(truth, start_h) / g.voxel,
                              displacement_voxel=tt.displacement(truth, pose[0].cpu().numpy()) / g.voxel,
                              **{f"{k}_ms": best[k] for k in runs}, **{f"{k}_median_ms": median[k] for k in runs},
                              ms_per_iteration=best["track"] / ITERS, torch_over_track=best["torch_track"] / best["track"],
                              track_over_clone=best["track"] / best["clone"], torch_pose_max_abs_diff=pose_diff, agree_emulation=agree_emulation)))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
