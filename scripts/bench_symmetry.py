#!/usr/bin/env python3
"""Time one `find_symmetries`-sized symmetry check (engine.symmetry_check: csrc/symmetry.hip) against the same test written in torch, on
the same device, and against its own mode without early outs.

  workload  one tessellated cylinder (an n-gon prism with cap-centre vertices, radius 0.05 m, height 0.2 m: 4 n triangles, 2 n + 2
            vertices), the candidates `evaluation.symmetry_candidates` gives for it at tol = 0.01 x diameter (320 at n = 32), the test
            points of `find_symmetries` (the vertices, then --samples surface points), n = --sizes (128, 256 and 512 triangles by default;
            beyond n = 128 a rim segment is shorter than tol and the candidates multiply)
  (a) engine.symmetry_check mode 0: the screen with early outs, then the measurement of the accepted candidates (what find_symmetries runs)
  (b) engine.symmetry_check mode 1: every candidate measured against every triangle, no early out
  (c) the same decision in torch on the device: the transformed test points of a chunk of candidates against all triangles (the three
      edge distances and the plane distance where the foot lies inside, fp32), min over triangles, max over points, --torch-pairs
      point-triangle pairs at a time; one read-back at the end

Device-event times after a warm-up, best of --reps.  One header line, then one JSON line per size.  (a) and (b) must give the same flags;
(c) must agree with them (the fixture keeps every deviation away from tol).

Usage: python scripts/bench_symmetry.py [--reps 5] [--sizes 32 64 128] [--samples 512]
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
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

from bench_bop_match import timed  # noqa: E402
from megapose6d_amd import engine as eng  # noqa: E402
from megapose6d_amd import evaluation as ev  # noqa: E402
from support import symmetry as sy  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--torch-pairs", type=int, default=1 << 24, help="point-triangle pairs the torch formulation computes at a time")
    ap.add_argument("--tile", type=int, default=0)
    args = ap.parse_args()
    n_cu, _, arch = eng.device_info()
    print(f"# {arch}, {n_cu} CUs; an n-gon cylinder, its candidates at tol = 0.01 x diameter, vertices + {args.samples} surface points; tile {args.tile}; "
          f"torch {args.torch_pairs} pairs at a time; best of {args.reps} after a warm-up")
    ok = True
    for n in args.sizes:
        v, f = sy.prism(n, 0.05, 0.2)
        tol = sy.REL_TOL * sy.diameter(v)
        status, center, rotations, n_cand = ev.symmetry_candidates(v, f, tol, max_candidates=1 << 20)
        assert status == "ok"
        d_v, d_f = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
        u = torch.rand(1, args.samples, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float32).cuda()
        sampled, _ = eng.surface_sample(d_v, d_f, [0, len(v)], [0, len(f)], u)
        tests = torch.cat([d_v, sampled[0]])
        cand_R = torch.from_numpy(rotations.astype(np.float32)).cuda()
        d_c = torch.from_numpy(center.astype(np.float32)).cuda()[None]
        offs = ([0, len(v)], [0, len(f)], [0, len(tests)], [0, n_cand])
        check = lambda mode: eng.symmetry_check(d_v, f, tests, cand_R, d_c, *offs, [tol], mode=mode, tile=args.tile)   # noqa: E731
        a, b, c = (d_v[d_f[:, k].long()][None] for k in range(3))
        per = max(1, args.torch_pairs // (len(tests) * len(f)))

        def in_torch():
            out = []
            for k0 in range(0, n_cand, per):
                g = (tests - d_c) @ cand_R[k0:k0 + per].transpose(1, 2) + d_c                      # [k,T,3]
                d2 = sy.pair_dist2(g.reshape(-1, 1, 3), a, b, c).min(1)[0]
                out.append(d2.reshape(len(g), -1).max(1)[0])
            return torch.cat(out) <= tol * tol

        t_screen = timed(lambda: check(0), args.reps)
        t_all = timed(lambda: check(1), args.reps)
        t_torch = timed(in_torch, max(1, min(args.reps, 3)))
        acc0, acc1, acc_t = check(0)[0].bool(), check(1)[0].bool(), in_torch()
        agree = bool(torch.equal(acc0, acc1) and torch.equal(acc0, acc_t))
        ok = ok and agree
        print(json.dumps(dict(name="symmetry_check", n_gon=n, triangles=len(f), test_points=len(tests), candidates=n_cand, accepted=int(acc0.sum()),
                              pairs=n_cand * len(tests) * len(f), screen_ms=t_screen, measure_all_ms=t_all, torch_ms=t_torch,
                              torch_over_screen=t_torch / t_screen, measure_all_over_screen=t_all / t_screen,
                              gpairs_per_s_measure_all=n_cand * len(tests) * len(f) / t_all / 1e6, agree=agree)), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
