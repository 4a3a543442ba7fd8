#!/usr/bin/env python3
"""Time the surface sampler of a mesh database (engine.surface_sample: csrc/surface_sample.hip) against what a user would otherwise
write, on the same machine.

  workload  --objects objects (21, a BOP dataset's count) of --faces triangles each (100 000): a seeded triangle soup, areas spread
            over three orders of magnitude, at --counts samples per object (2 000: the reference's crop-logic subset; 100 000: an
            evaluation database)
  (a) engine.surface_sample: the five launches and the copy of the prefix array
  (b) the same arithmetic in torch on the device: float64 areas, cumsum per object, searchsorted at u0 * total, the reflection and the
      three gathers (trimesh's algorithm; a loop over the objects, as the reference loops over its meshes)
  (c) a copy of the bytes the launch touches (vertices, faces, uniforms, points, face ids, and the weights and prefix sums once written
      and once read), as one device-to-device copy: the floor of a memory-bound pass

(a), (b) and (c) are device-event times after a warm-up launch, best of --reps.  One header line, then one JSON line per count.  (a) is
checked against (b): the share of samples whose face differs (fp32 against float64 weights: about faces * 2^-22) and, where the face
agrees, the largest distance between the points over the object's extent.  This is set-up work done once per database: there is no
pass / fail time, the torch line is recorded for context.

Usage: python scripts/bench_surface_sample.py [--reps 5] [--objects 21] [--faces 100000] [--counts 2000 100000] [--block 0]
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
sys.path.insert(0, str(ROOT / "scripts"))

from bench_bop_match import timed  # noqa: E402
from megapose6d_amd import engine as eng  # noqa: E402


def soup(n_faces: int, seed: int) -> np.ndarray:
    """[n_faces,3,3] fp32: random triangles inside a 0.2 m cube, edges of 0.1 .. 10 mm"""
    rng = np.random.RandomState(seed)
    centre = rng.uniform(-0.1, 0.1, size=(n_faces, 1, 3))
    size = 10.0 ** rng.uniform(-4.0, -2.0, size=(n_faces, 1, 1))
    return (centre + size * rng.normal(size=(n_faces, 3, 3))).astype(np.float32)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--objects", type=int, default=21)
    ap.add_argument("--faces", type=int, default=100000)
    ap.add_argument("--counts", type=int, nargs="+", default=[2000, 100000])
    ap.add_argument("--block", type=int, default=0)
    args = ap.parse_args()
    n_obj, n_faces = args.objects, args.faces
    n_cu, _, arch = eng.device_info()
    print(f"# {arch}, {n_cu} CUs; {n_obj} objects of {n_faces} random triangles; block {args.block}; best of {args.reps} after a warm-up")
    tris = np.stack([soup(n_faces, o) for o in range(n_obj)])                       # [n_obj, F, 3, 3]
    vertices = torch.from_numpy(tris.reshape(-1, 3)).cuda()
    faces = torch.arange(3 * n_faces, dtype=torch.int32).reshape(-1, 3).repeat(n_obj, 1).cuda()
    vert_off = np.arange(n_obj + 1, dtype=np.int64) * 3 * n_faces
    face_off = np.arange(n_obj + 1, dtype=np.int64) * n_faces
    extent = torch.from_numpy(np.linalg.norm(tris.reshape(n_obj, -1, 3).max(1) - tris.reshape(n_obj, -1, 3).min(1), axis=1)).cuda()
    V = vertices.reshape(n_obj, n_faces, 3, 3)
    ok = True
    for count in args.counts:
        u = torch.rand(n_obj, count, 3, generator=torch.Generator().manual_seed(0)).cuda()
        launch = lambda: eng.surface_sample(vertices, faces, vert_off, face_off, u, block=args.block)  # noqa: E731

        def in_torch():
            points, face = [], []
            for o in range(n_obj):
                a = V[o, :, 0].double()
                e1, e2 = V[o, :, 1].double() - a, V[o, :, 2].double() - a
                cum = torch.cumsum(0.5 * torch.linalg.norm(torch.linalg.cross(e1, e2), dim=1), 0)
                idx = torch.searchsorted(cum, u[o, :, 0].double() * cum[-1]).clamp_(max=n_faces - 1)
                r = u[o, :, 1:].double()
                r = torch.where((r.sum(1) > 1.0)[:, None], 1.0 - r, r)
                points.append(a[idx] + e1[idx] * r[:, :1] + e2[idx] * r[:, 1:])
                face.append(idx)
            return torch.stack(points), torch.stack(face)

        touched = vertices.numel() * 4 + faces.numel() * 4 + u.numel() * 4 + n_obj * count * 16 + n_obj * n_faces * (4 + 8) * 2
        src = torch.empty(touched // 2, dtype=torch.uint8, device="cuda")          # a copy reads and writes: half the bytes each way
        dst = torch.empty_like(src)
        t_a = timed(launch, args.reps)
        t_b = timed(in_torch, max(1, min(args.reps, 3)))
        t_c = timed(lambda: dst.copy_(src), args.reps)
        points, face = launch()
        want_points, want_face = in_torch()
        same = face.long() == want_face
        failed = int((face < 0).sum())
        err = ((points.double() - want_points).norm(dim=2) / extent[:, None])[same].max().item() if bool(same.any()) else float("nan")
        differ = 1.0 - same.double().mean().item()
        agree = failed == 0 and differ <= 0.01 and err <= 1e-6
        ok = ok and agree
        print(json.dumps(dict(name="surface_sample", objects=n_obj, faces=n_faces, count=count, surface_sample_ms=t_a, torch_ms=t_b,
                              torch_over_surface_sample=t_b / t_a, copy_ms=t_c, surface_sample_over_copy=t_a / t_c, bytes=touched,
                              faces_differ=differ, points_err_over_extent=err, agree=agree)), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
