#!/usr/bin/env python3
"""Time TSDF fusion and surface extraction (csrc/tsdf.hip) against the same arithmetic formulated in torch and against a copy of the
volume's bytes, on the same machine.

  workload  64 views of 480 x 640 (f = 600) of the analytic sphere of the tests, cameras on a spiral over the sphere of directions at
            0.4 m, with masks and colours, fused into 128^3 and into 256^3 nodes over [-0.066, 0.066]^3 (6 planes of 32-bit words)
  (a) the product calls: engine.tsdf_integrate (one launch for the 64 views), engine.tsdf_extract (count, the read-back of the two
      totals, emit), and the count alone (mp_tsdf_extract_count)
  (b) the same arithmetic in torch on the device, whole-array operations view by view over slabs of 32 z-layers (integrate), and the
      number of vertex-carrying edges from shifted comparisons (the count); counts and the number of vertices are compared with (a)
      before anything is timed (torch's sums differ in low bits and are only reported).  The emit pass has no torch formulation here.
  Before anything is timed, the volume, vertices, colours and faces of (a) at the first size are compared bit for bit with the host
  emulation of the tests (tests/tsdf_emul.cpp), so the table rests on checked results; a difference ends the run with exit code 1.
  (c) torch.clone of the volume: the floor of a pass that reads and writes every plane once, which is what (a) integrate does

Wall-clock times around a device synchronise, after warm-up; the runs take turns --reps times and the best and the median of each are
reported, with visits per second (nodes x views / best time) and the bytes a call moves.  One header line, then one JSON line per
volume.

Usage: python scripts/bench_tsdf.py [--reps 10] [--views 64] [--sizes 128 256]
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

from megapose6d_amd import _lib  # noqa: E402
from megapose6d_amd import engine as eng  # noqa: E402
from tests.support import tsdf as st  # noqa: E402

H, W, FOCAL, HALF, SLAB = 480, 640, 600.0, 0.066, 32


def make_views(n: int):
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    dirs = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    cams = np.stack([st.look_at(0.4 * d, up=(0, 0, 1) if abs(d[2]) < 0.9 else (0, 1, 0)) for d in dirs])
    K = st.intrinsics(FOCAL, H, W)
    depth = np.stack([st.sphere_depth(T, K, h=H, w=W) for T in cams])
    rgb = np.stack([st._surface_rgb(d, T, K) for d, T in zip(depth, cams)])
    return dict(depth=torch.from_numpy(depth.astype(np.float32)).cuda(), masks=torch.from_numpy((depth > 0).astype(np.uint8)).cuda(),
                rgb=torch.from_numpy(rgb).cuda(), K=torch.from_numpy(np.repeat(K[None], n, 0).astype(np.float32)).cuda(),
                TCO=torch.from_numpy(cams.astype(np.float32)).cuda())


def torch_integrate(vol: torch.Tensor, origin, voxel: float, v, mu: float, z_min: float) -> None:
    """the contract's steps (csrc/tsdf_core.h) as whole-array float32 operations, in place, slab by slab"""
    _, nz, ny, nx = vol.shape
    dev = vol.device
    f32 = torch.float32
    px = (origin[0] + voxel * torch.arange(nx, device=dev, dtype=f32))[None, None, :]
    py = (origin[1] + voxel * torch.arange(ny, device=dev, dtype=f32))[None, :, None]
    cnt, ccnt = vol[1].view(torch.int32), vol[5].view(torch.int32)
    Kh, Th = v["K"].cpu().numpy(), v["TCO"].cpu().numpy()
    for k0 in range(0, nz, SLAB):
        k1 = min(nz, k0 + SLAB)
        pz = (origin[2] + voxel * torch.arange(k0, k1, device=dev, dtype=f32))[:, None, None]
        s, c = vol[0, k0:k1], cnt[k0:k1]
        for q in range(len(Kh)):
            T, fx, cx, fy, cy = Th[q], float(Kh[q, 0, 0]), float(Kh[q, 0, 2]), float(Kh[q, 1, 1]), float(Kh[q, 1, 2])
            cam = [((float(T[r, 0]) * px + float(T[r, 1]) * py) + float(T[r, 2]) * pz) + float(T[r, 3]) for r in range(3)]
            xf, yf = torch.floor((fx * cam[0]) / cam[2] + cx), torch.floor((fy * cam[1]) / cam[2] + cy)
            ok = (cam[2] > z_min) & (xf >= 0) & (xf < W) & (yf >= 0) & (yf < H)
            at = torch.where(ok, yf * W + xf, torch.zeros_like(xf)).long()
            off = v["masks"][q].reshape(-1)[at] == 0
            free = ok & off
            d = v["depth"][q].reshape(-1)[at]
            sd = d - cam[2]
            use = ok & ~off & torch.isfinite(d) & (d > 0) & (sd >= -mu)
            s += torch.where(free, torch.ones_like(sd), torch.where(use, torch.clamp(sd / mu, max=1.0), torch.zeros_like(sd)))
            c += (free | use).to(torch.int32)
            cuse = use & (sd.abs() <= mu)
            rgb = v["rgb"][q].reshape(-1, 3)[at]
            for ch in range(3):
                vol[2 + ch, k0:k1] += torch.where(cuse, rgb[..., ch].to(f32), torch.zeros_like(sd))
            ccnt[k0:k1] += cuse.to(torch.int32)


def torch_count_vertices(vol: torch.Tensor, min_views: int = 1) -> int:
    cnt = vol[1].view(torch.int32)
    nz, ny, nx = cnt.shape
    obs = cnt >= min_views
    inside = obs & (vol[0] / cnt.to(torch.float32) < 0)
    complete = torch.zeros_like(obs)
    acc = torch.ones(nz - 1, ny - 1, nx - 1, dtype=torch.bool, device=vol.device)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                acc &= obs[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    complete[:nz - 1, :ny - 1, :nx - 1] = acc
    total = 0
    for dx, dy, dz in st.KIND_DIFFS:
        a = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        b = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        cross = obs[a] & obs[b] & (inside[a] != inside[b])
        near = torch.zeros_like(obs)
        for bx in ((0,) if dx else (0, 1)):
            for by in ((0,) if dy else (0, 1)):
                for bz in ((0,) if dz else (0, 1)):
                    near[bz:, by:, bx:] |= complete[:nz - bz, :ny - by, :nx - bx]
        total += int((cross & near[a]).sum())
    return total


def wall_once(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    args = ap.parse_args()
    views = make_views(args.views)
    n_cu, _, arch = eng.device_info()
    print(f"# {arch}, {n_cu} CUs; {args.views} views of {H} x {W} of a sphere of radius {st.SPHERE_R} m, masks and colours; {args.reps} reps in turn, "
          "wall clock around a synchronise")
    lib = _lib.load()
    ok = True
    for n in args.sizes:
        g = st.cube_grid(n, HALF)
        mu = float(g.mu3)
        N = n ** 3

        def integrate(vol):
            eng.tsdf_integrate(vol, g.origin, g.voxel, views["depth"], views["K"], views["TCO"], views["masks"], views["rgb"], mu=mu, z_min=st.Z_MIN)

        vol = eng.tsdf_volume(g.dims, True, "cuda")
        integrate(vol)
        ref = torch.zeros_like(vol)
        torch_integrate(ref, [float(np.float32(o)) for o in g.origin], float(np.float32(g.voxel)), views, mu, st.Z_MIN)
        agree_counts = bool(torch.equal(vol[1].view(torch.int32), ref[1].view(torch.int32)) and torch.equal(vol[5].view(torch.int32), ref[5].view(torch.int32)))
        agree_sums = bool(torch.equal(vol[0].view(torch.int32), ref[0].view(torch.int32)))
        verts, _, faces = eng.tsdf_extract(vol, g.origin, g.voxel)
        agree_vertices = torch_count_vertices(vol) == int(verts.shape[0])
        agree_emulation = None
        if n == args.sizes[0]:                                     # the host emulation, bit for bit (one core: seconds at 128^3)
            host = {k: t.cpu().numpy() for k, t in views.items()}
            e_vol = st.new_volume(g.dims, True)
            assert st.emul_integrate(e_vol, g, host, mu=mu) == 0
            e_mesh = st.emul_extract(e_vol, g)
            colors = eng.tsdf_extract(vol, g.origin, g.voxel)[1]
            agree_emulation = all(a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
                                  for a, b in zip((vol.cpu().numpy(), verts.cpu().numpy(), colors.cpu().numpy(), faces.cpu().numpy()), (e_vol, *e_mesh)))
            ok = ok and agree_emulation
        ok = ok and agree_counts and agree_vertices
        ws = torch.empty(lib.mp_tsdf_extract_workspace_bytes(n, n, n), dtype=torch.uint8, device="cuda")
        totals = torch.zeros(2, dtype=torch.int32, device="cuda")
        scratch = torch.zeros_like(vol)

        def count():
            _lib.check(lib.mp_tsdf_extract_count(vol.data_ptr(), n, n, n, 1, 1, totals.data_ptr(), ws.data_ptr(), ws.numel(), eng._stream()))

        runs = {"integrate": lambda: integrate(scratch), "torch_integrate": lambda: torch_integrate(scratch, g.origin, g.voxel, views, mu, st.Z_MIN),
                "clone": lambda: vol.clone(), "count": count, "extract": lambda: eng.tsdf_extract(vol, g.origin, g.voxel),
                "torch_count": lambda: torch_count_vertices(vol)}
        for fn in runs.values():
            fn()
        times = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, fn in runs.items():
                times[k].append(wall_once(fn))
        best = {k: min(v) for k, v in times.items()}
        median = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps(dict(name="tsdf", nodes=N, side=n, views=args.views, H=H, W=W, reps=args.reps, volume_bytes=int(vol.numel() * 4),
                              integrate_bytes_moved=int(2 * vol.numel() * 4), extract_workspace_bytes=int(ws.numel()), vertices=int(verts.shape[0]),
                              triangles=int(faces.shape[0]), **{f"{k}_ms": best[k] for k in runs}, **{f"{k}_median_ms": median[k] for k in runs},
                              visits_per_s=N * args.views / (best["integrate"] * 1e-3), torch_visits_per_s=N * args.views / (best["torch_integrate"] * 1e-3),
                              torch_over_integrate=best["torch_integrate"] / best["integrate"], integrate_over_clone=best["integrate"] / best["clone"],
                              torch_count_over_count=best["torch_count"] / best["count"], count_over_clone=best["count"] / best["clone"],
                              extract_over_clone=best["extract"] / best["clone"], agree_counts=agree_counts, agree_sums=agree_sums,
                              agree_vertices=agree_vertices, agree_emulation=agree_emulation)))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
