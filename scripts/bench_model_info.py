#!/usr/bin/env python3
"""Time the exact diameter of one object (engine.model_info: csrc/model_info.hip) against what a user would otherwise write, on the
same machine.

  workload  one object of N points on a unit sphere plus 1 % noise (seeded), N = 2^15 ... 2^20: the case a convex surface makes worst,
            since every point is nearly as far from its antipode as the diameter
  (a) engine.model_info (the pair pass, the reduce pass and the copy of the prefix array)
  (b) the same maximum with torch.cdist on the device, --cdist-elems distances at a time (rows x N), the maximum of each piece kept on
      the device and one read-back at the end
  (c) a row-chunked numpy maximum on the host (float32 differences, 256 rows at a time) up to --cpu-max points: the only way to the
      number before this kernel, since nothing on the device computed it

(a) and (b) are device-event times after a warm-up launch, best of --reps; (c) is one wall-clock pass.  One header line, then one JSON
line per size.  (a) is checked against (b) within 1e-5 relative (cdist's own arithmetic) at every size.

Usage: python scripts/bench_model_info.py [--reps 5] [--sizes 32768 131072 524288 1048576] [--cpu-max 32768]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

from bench_bop_match import timed  # noqa: E402
from megapose6d_amd import engine as eng  # noqa: E402


def sphere(n: int, seed: int = 0) -> np.ndarray:
    rng = np.random.RandomState(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * (1.0 + 0.01 * rng.normal(size=(n, 1)))).astype(np.float32)


def numpy_max(p: np.ndarray) -> float:
    best = np.float32(0)
    for r0 in range(0, len(p), 256):
        d = p[r0:r0 + 256, None, :] - p[None, r0:, :]
        best = max(best, np.einsum("ijk,ijk->ij", d, d).max())
    return float(np.sqrt(best))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 15, 1 << 17, 1 << 19, 1 << 20])
    ap.add_argument("--cpu-max", type=int, default=1 << 15, help="largest size the host baseline is run at")
    ap.add_argument("--cdist-elems", type=int, default=1 << 28, help="distances torch.cdist computes at a time")
    ap.add_argument("--tile", type=int, default=0)
    args = ap.parse_args()
    n_cu, _, arch = eng.device_info()
    print(f"# {arch}, {n_cu} CUs; one object of N points on a unit sphere with 1 % noise; tile {args.tile}; cdist {args.cdist_elems} distances at a time; "
          f"best of {args.reps} after a warm-up")
    ok = True
    for n in args.sizes:
        p = sphere(n)
        pts = torch.from_numpy(p).cuda()[None]
        h_n = np.asarray([n], np.int32)
        launch = lambda: eng.model_info(pts, h_n, tile=args.tile)  # noqa: E731
        rows = max(1, args.cdist_elems // n)

        def in_torch():
            best = torch.zeros((), device="cuda")
            for r0 in range(0, n, rows):
                best = torch.maximum(best, torch.cdist(pts[0, r0:r0 + rows], pts[0, r0:]).max())
            return best

        t_a = timed(launch, args.reps)
        t_b = timed(in_torch, max(1, min(args.reps, 3)))
        d2, pair, _ = launch()
        i, j = (int(v) for v in pair[0].cpu())
        diam = float(np.linalg.norm(p[i].astype(np.float64) - p[j].astype(np.float64)))
        d_torch = float(in_torch())
        agree = abs(diam - d_torch) <= 1e-5 * diam and abs(float(d2[0]) - diam * diam) <= 1e-6 * diam * diam
        out = dict(name="model_info", n=n, pairs=n * (n + 1) // 2, model_info_ms=t_a, cdist_ms=t_b, cdist_over_model_info=t_b / t_a,
                   gpairs_per_s=n * (n + 1) / 2 / t_a / 1e6, diameter=diam, pair=[i, j], agree=agree)
        if n <= args.cpu_max:
            t0 = time.perf_counter()
            d_np = numpy_max(p)
            out["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            out["numpy_over_model_info"] = out["numpy_ms"] / t_a
            agree = agree and abs(d_np - diam) <= 1e-6 * diam
            out["agree"] = agree
        ok = ok and agree
        print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
