#!/usr/bin/env python3
"""Measure the maximum-clique search (engine.max_clique: csrc/teaser_clique.hip): what a step costs on the device, which step budget keeps a
worst-case row under a time cap, and what the selection costs the TEASER++ refiner.

  planted   rows of 1024 vertices launched alone (tests/support/teaser_clique.py): 300 planted in background 0.05 (the shortcut), 40
            planted in background 0.05, G(1024, 0.1): time per row, steps, steps per second; then the three in one launch
  budget    a row that exhausts any budget (300 planted vertices with internal edge probability 0.98 among 1024, background 0.05) at
            every power of two up to the ceiling an argument may ask for: time, clique size, steps.  `default_under_cap` is the largest
            power of two whose row stays under --cap-ms (100): the default budget of DESIGN.md 3.14
  fixed     the same launch with budget 0: what pack, peel, load and the greedy bound cost without a search
  refiner   engine.teaser_refine with selection "kcore" against "max_clique" on the scenes of scripts/bench_teaser_refiner.py (skipped
            with --no-refiner)

Device-event times after a warm-up launch, best of --reps; one header line, then one JSON line.  No figure is a gate.

Usage: python scripts/bench_max_clique.py [--reps 3] [--cap-ms 100] [--no-refiner]
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
sys.path.insert(0, str(ROOT / "tests"))

from bench_bop_match import timed  # noqa: E402
from megapose6d_amd import engine as eng  # noqa: E402
from support import teaser_clique as tc  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cap-ms", type=float, default=100.0)
    ap.add_argument("--no-refiner", action="store_true")
    args = ap.parse_args()
    n_cu, _, arch = eng.device_info()
    default, ceiling = eng.max_clique_step_limits()
    print(f"# {arch}, {n_cu} CUs; default budget {default} steps, ceiling {ceiling}; best of {args.reps} after a warm-up")
    out = dict(name="max_clique", default_steps=default, step_ceiling=ceiling)

    rows, _ = tc.stride1024_rows()
    dev_rows = torch.tensor(rows, dtype=torch.uint8).cuda()
    planted = []
    for r, what in enumerate(("planted300", "planted40", "gnp0.1")):
        one = dev_rows[r: r + 1]
        ms = timed(lambda: eng.max_clique(one, None, ceiling), args.reps)
        size, upper, exact, steps = eng.max_clique(one, None, ceiling)[1][0].tolist()
        planted.append(dict(row=what, ms=ms, size=size, upper_bound=upper, exact=exact, steps=steps, steps_per_s=steps / (ms * 1e-3) if steps else 0.0))
    out["planted"] = planted
    out["planted_three_rows_ms"] = timed(lambda: eng.max_clique(dev_rows, None, ceiling), args.reps)

    hard = torch.tensor(tc.exhausting_row()[None], dtype=torch.uint8).cuda()
    out["fixed_ms"] = timed(lambda: eng.max_clique(hard, None, 0), args.reps)
    table, under = [], 0
    budget = 1 << 12
    while budget <= ceiling:
        ms = timed(lambda: eng.max_clique(hard, None, budget), args.reps)
        size, upper, exact, steps = eng.max_clique(hard, None, budget)[1][0].tolist()
        table.append(dict(max_steps=budget, ms=ms, size=size, exact=exact, steps=steps, steps_per_s=steps / ((ms - out["fixed_ms"]) * 1e-3) if ms > out["fixed_ms"] else 0.0))
        if ms < args.cap_ms and not exact:
            under = budget
        if exact:      # (the budget was enough: larger ones time the same search)
            break
        budget *= 2
    out["budget"] = table
    out["default_under_cap"] = under

    if not args.no_refiner:
        from bench_teaser_refiner import build_scenes

        sc = build_scenes(8, 8)
        call = dict(depth_meas=sc["depth"], im_ids=sc["ids"], depth_rend=sc["rend"], K_rows=sc["K_rows"], TCO=sc["TCO"])
        out["refine_kcore_ms"] = timed(lambda: eng.teaser_refine(**call), args.reps)
        out["refine_max_clique_ms"] = timed(lambda: eng.teaser_refine(**call, inlier_selection="max_clique"), args.reps)
        pk, rk, ik = eng.teaser_refine(**call)
        pc, rc, ic, tel = eng.teaser_refine(**call, inlier_selection="max_clique", telemetry=True)
        gt = sc["gt"]

        def t_err(p):
            e = np.linalg.norm(p.cpu().numpy()[:, :3, 3] - gt[:, :3, 3], axis=1)
            return [float(np.median(e)), float(e.max())]

        clique = tel["clique"].cpu().numpy()
        out.update(detections=len(gt), selected_kcore_mean=float(ik[:, 2].float().mean()), selected_max_clique_mean=float(ic[:, 2].float().mean()),
                   rows_exact=int(clique[:, 2].sum()), rows_shortcut=int((clique[:, 3] == 0).sum()), steps_max=int(clique[:, 3].max()),
                   accepted_kcore=int((rk == 0).sum()), accepted_max_clique=int((rc == 0).sum()), translation_error_kcore_median_max_m=t_err(pk),
                   translation_error_max_clique_median_max_m=t_err(pc))
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
