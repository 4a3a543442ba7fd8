#!/usr/bin/env python3
"""Time the mesh clean-up kernels (csrc/mesh_cleanup.hip) on the meshes scripts/bench_tsdf.py reconstructs, against the same arithmetic
in torch and in numpy, and measure what decimation buys the rasteriser.

  workload  the sphere meshes of scripts/bench_tsdf.py: 64 views of 480 x 640 fused into 128^3 and 256^3 nodes, extracted by
            engine.tsdf_extract (130 288 vertices / 260 572 triangles and about four times that), with colours
  Before anything is timed, components, select (the largest component) and cluster (the grid that simplify(max_faces=20 000) chooses)
  at the first size are compared bit for bit with the host emulation of the tests (tests/mesh_cleanup_emul.cpp); a difference ends the
  run with exit code 1.
  (a) the entry points: engine.mesh_components (the totals read back), engine.mesh_select, engine.mesh_cluster_count,
      engine.mesh_cluster, and mesh_cleanup.simplify(max_faces=20 000) as a whole (bounds, at most 9 counts, one cluster)
  (b) the cluster arithmetic in torch on the device: floor, unique over the kept faces' cells, index_add_ of the coordinates in
      float64, boolean indexing of the faces (faces and vertex count are compared with (a); the means differ in low bits)
  (c) the same in numpy on the host, from host arrays
  (d) Panda3dBatchRenderer.render of the full and of the decimated object: --poses poses at 0.4 m, 240 x 320 (the benchmark's crop
      size), ambient light; milliseconds and the ratio

Wall-clock times around a device synchronise, after warm-up; the runs take turns --reps times; best and median.  One header line, then
one JSON line per mesh.

Usage: python scripts/bench_mesh_cleanup.py [--reps 10] [--views 64] [--sizes 128 256] [--max-faces 20000] [--poses 64]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import bench_tsdf  # noqa: E402
from megapose6d_amd import RigidObject, RigidObjectDataset, mesh_io  # noqa: E402
from megapose6d_amd import engine as eng  # noqa: E402
from megapose6d_amd import mesh_cleanup as mc  # noqa: E402
from tests.support import mesh_cleanup as sm  # noqa: E402
from tests.support import tsdf as st  # noqa: E402

RENDER_H, RENDER_W, RENDER_F = 240, 320, 600.0


def torch_cluster(v: torch.Tensor, f: torch.Tensor, origin, cell: float, dims):
    o = torch.tensor(origin, dtype=torch.float32, device=v.device)
    g = torch.tensor(dims, dtype=torch.int64, device=v.device)
    u = (v - o) / cell
    i = torch.floor(u)
    ok = ((i >= 0) & (i < g.to(torch.float32))).all(1)
    ii = i.long()
    cell_id = torch.where(ok, ii[:, 0] + g[0] * (ii[:, 1] + g[1] * ii[:, 2]), torch.full_like(ii[:, 0], -1))
    fc = cell_id[f.long()]
    kept = (fc >= 0).all(1) & (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    used, faces = torch.unique(fc[kept], return_inverse=True)
    rank = torch.searchsorted(used, cell_id.clamp(min=0))
    member = ok & (used[rank.clamp(max=len(used) - 1)] == cell_id)
    sums = torch.zeros(len(used), 3, dtype=torch.float64, device=v.device).index_add_(0, rank[member], u[member].double())
    count = torch.zeros(len(used), dtype=torch.float64, device=v.device).index_add_(0, rank[member], torch.ones_like(rank[member], dtype=torch.float64))
    return (o.double() + cell * sums / count[:, None]).float(), faces.to(torch.int32)


def numpy_cluster(v: np.ndarray, f: np.ndarray, origin, cell: float, dims):
    o, g = np.asarray(origin, np.float32), np.asarray(dims, np.int64)
    u = (v - o) / np.float32(cell)
    i = np.floor(u)
    ok = ((i >= 0) & (i < g.astype(np.float32))).all(1)
    ii = i.astype(np.int64)
    cell_id = np.where(ok, ii[:, 0] + g[0] * (ii[:, 1] + g[1] * ii[:, 2]), -1)
    fc = cell_id[f]
    kept = (fc >= 0).all(1) & (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    used, faces = np.unique(fc[kept], return_inverse=True)
    rank = np.searchsorted(used, cell_id)
    member = ok & (used[np.minimum(rank, len(used) - 1)] == cell_id)
    sums = np.stack([np.bincount(rank[member], u[member, k].astype(np.float64), len(used)) for k in range(3)], 1)
    count = np.bincount(rank[member], minlength=len(used))
    return (o.astype(np.float64) + cell * sums / count[:, None]).astype(np.float32), faces.reshape(-1, 3).astype(np.int32)


def render_poses(n: int) -> torch.Tensor:
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    dirs = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    return torch.from_numpy(np.stack([st.look_at(0.4 * d, up=(0, 0, 1) if abs(d[2]) < 0.9 else (0, 1, 0)) for d in dirs]).astype(np.float32)).cuda()


def same_bits(a, b) -> bool:
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def wall_once(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main() -> int:
    from megapose6d_amd.renderer import Panda3dBatchRenderer
    from megapose6d_amd.types import Panda3dLightData

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--max-faces", type=int, default=20000)
    ap.add_argument("--poses", type=int, default=64)
    args = ap.parse_args()
    views = bench_tsdf.make_views(args.views)
    n_cu, _, arch = eng.device_info()
    print(f"# {arch}, {n_cu} CUs; sphere of radius {st.SPHERE_R} m from {args.views} views; budget {args.max_faces} faces; {args.poses} poses of "
          f"{RENDER_H} x {RENDER_W}; {args.reps} reps in turn, wall clock around a synchronise")
    ok = True
    tmp = Path(tempfile.mkdtemp(prefix="mp_mesh_cleanup_"))
    TCO = render_poses(args.poses)
    K = torch.from_numpy(np.repeat(st.intrinsics(RENDER_F, RENDER_H, RENDER_W)[None], args.poses, 0).astype(np.float32)).cuda()
    lights = [[Panda3dLightData("ambient")]] * args.poses
    for n in args.sizes:
        g = st.cube_grid(n, bench_tsdf.HALF)
        vol = eng.tsdf_volume(g.dims, True, "cuda")
        eng.tsdf_integrate(vol, g.origin, g.voxel, views["depth"], views["K"], views["TCO"], views["masks"], views["rgb"], mu=float(g.mu3), z_min=st.Z_MIN)
        v, c, f = eng.tsdf_extract(vol, g.origin, g.voxel)
        del vol
        mesh = dict(vertices=v, faces=f, colors=c)
        light = mc.simplify(mesh, max_faces=args.max_faces)
        # the grid that simplify chose: replay its bisection on the counts
        lo, hi = 1, mc.BISECT_HI
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if eng.mesh_cluster_count(v, f, *mc.grid_for(mesh, mid))[1] <= args.max_faces else (lo, mid)
        grid = mc.grid_for(mesh, lo)
        labels, flabels, fcount, totals = eng.mesh_components(v, f)
        keep = (flabels == int(totals[1])).to(torch.uint8)
        agree_emulation = None
        if n == args.sizes[0]:
            hm = sm.mesh(v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy())
            want_cc = sm.emul_components(hm.V, hm["faces"])
            agree_emulation = all(same_bits(a, b) for a, b in zip((labels, flabels, fcount, totals), want_cc))
            got_s, want_s = eng.mesh_select(v, f, keep, c), sm.emul_select(hm, keep.cpu().numpy())
            got_c, want_c = eng.mesh_cluster(v, f, *grid, colors=c), sm.emul_cluster(hm, *grid)
            for got, want in ((got_s, want_s), (got_c, want_c)):
                agree_emulation = agree_emulation and all(same_bits(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]
            agree_emulation = agree_emulation and same_bits(light["vertices"], want_c[0]) and same_bits(light["faces"], want_c[1])
            ok = ok and agree_emulation
        tv, tf = torch_cluster(v, f, *grid)
        agree_torch = bool(tf.shape == light["faces"].shape and torch.equal(tf, light["faces"]) and tv.shape == light["vertices"].shape)
        torch_max_diff = float((tv - light["vertices"]).abs().max()) if agree_torch else None
        hv, hf = v.cpu().numpy(), f.cpu().numpy()
        nv_np, nf_np = numpy_cluster(hv, hf, *grid)
        agree_numpy = bool(nf_np.shape == tuple(light["faces"].shape) and np.array_equal(nf_np, light["faces"].cpu().numpy()))
        ok = ok and agree_torch and agree_numpy
        # the two objects for the rasteriser
        full_host, light_host = mc.to_host(mesh), mc.to_host(light)
        objs = [RigidObject(name, mesh_io.write_ply(tmp / f"{name}_{n}.ply", m["vertices"], m["faces"], colors=m["colors"], normals=m["normals"]), mesh_units="m")
                for name, m in (("full", full_host), ("light", light_host))]
        renderer = Panda3dBatchRenderer(RigidObjectDataset(objs))
        res = (RENDER_H, RENDER_W)
        full_img = renderer.render(["full"] * args.poses, TCO, K, lights, res).rgbs.float()
        light_img = renderer.render(["light"] * args.poses, TCO, K, lights, res).rgbs.float()
        scale = 255.0 if float(full_img.max()) > 1.5 else 1.0
        render_mean_abs_diff = float((full_img - light_img).abs().mean()) / scale

        runs = {"components": lambda: eng.mesh_components(v, f)[3].cpu(), "select": lambda: eng.mesh_select(v, f, keep, c),
                "cluster_count": lambda: eng.mesh_cluster_count(v, f, *grid), "cluster": lambda: eng.mesh_cluster(v, f, *grid, colors=c),
                "simplify": lambda: mc.simplify(mesh, max_faces=args.max_faces), "torch_cluster": lambda: torch_cluster(v, f, *grid),
                "numpy_cluster": lambda: numpy_cluster(hv, hf, *grid), "render_full": lambda: renderer.render(["full"] * args.poses, TCO, K, lights, res),
                "render_light": lambda: renderer.render(["light"] * args.poses, TCO, K, lights, res)}
        for fn in runs.values():
            fn()
        times = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, fn in runs.items():
                times[k].append(wall_once(fn))
        best = {k: min(t) for k, t in times.items()}
        median = {k: statistics.median(t) for k, t in times.items()}
        print(json.dumps(dict(name="mesh_cleanup", side=n, vertices=int(v.shape[0]), faces=int(f.shape[0]), max_faces=args.max_faces, cells_longest=lo,
                              grid=list(grid[2]), out_vertices=int(light["vertices"].shape[0]), out_faces=int(light["faces"].shape[0]),
                              components=int(totals[0]), reps=args.reps, poses=args.poses, **{f"{k}_ms": best[k] for k in runs},
                              **{f"{k}_median_ms": median[k] for k in runs}, torch_over_cluster=best["torch_cluster"] / best["cluster"],
                              numpy_over_cluster=best["numpy_cluster"] / best["cluster"], render_full_over_light=best["render_full"] / best["render_light"],
                              render_mean_abs_diff=render_mean_abs_diff, torch_max_vertex_diff=torch_max_diff, agree_emulation=agree_emulation,
                              agree_torch_faces=agree_torch, agree_numpy_faces=agree_numpy)))
        del renderer
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
