#!/usr/bin/env python3
"""Time BOP's greedy matching on the device against the contract restated in numpy on the host and against a copy of the bytes it reads
and writes, on the same machine.

  workload  one BOP test set's worth: 1000 frames, 15 (image, label) groups per frame with 1-3 ground truths and 1-4 estimates each
            (about 50 k candidates), 12 error columns x 10 thresholds = 120 problems per group; seeded uniform errors and thresholds
  (a) mp_bop_match alone (engine.bop_match on a resident index; the -1 fill and the workspace allocation are inside, as for every caller)
  (b) evaluation.bop_match: the same plus the construction of the index on the host, its copy to the device and the gather of the errors
  (c) the contract restated in numpy on the host (tests/support/bop_match.py: restated), timed on the first --sample groups and scaled
      to all of them (it is a Python loop per problem: the full set takes minutes)
  (d) torch.clone of a tensor of the bytes (a) reads and writes: errors, index, thresholds, match table

(a) and (d) are device-event times, (b) and (c) wall-clock (host work is the point), all after warm-up, best of --reps.  One header
line, then one JSON line.

Usage: python scripts/bench_bop_match.py [--reps 5] [--quick]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import pandas as pd
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from megapose6d_amd import engine as eng  # noqa: E402
from megapose6d_amd import evaluation as ev  # noqa: E402
from support import bop_match as bm  # noqa: E402


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


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=150, help="groups the host restatement is timed on")
    ap.add_argument("--quick", action="store_true", help="a twentieth of the frames (a functional check, not a measurement)")
    args = ap.parse_args()
    E, n_theta = 12, 10
    n_frames = 1000 // (20 if args.quick else 1)
    rng = np.random.RandomState(0)
    sizes = [(int(rng.randint(1, 5)), int(rng.randint(1, 4))) for _ in range(15 * n_frames)]
    c = bm.case(0, sizes, E, n_theta, nan_share=0.0)
    n_groups, n_cand, P = len(sizes), len(c["pred_id"]), c["n_pred"]
    n_top = np.asarray([s[1] for s in sizes], np.int32)                     # BOP 2019: the group's number of targets
    cand = pd.DataFrame(dict(pred_id=c["pred_id"], gt_id=c["gt_id"], group_id=c["group_id"]))
    errs = torch.from_numpy(c["errs"]).cuda()
    index = ev.bop_match_index(c["pred_id"], c["gt_id"], c["group_id"], c["scores"], n_groups)
    on_dev = {k: torch.from_numpy(index[k]).cuda() for k in eng.BOP_MATCH_INDEX}
    on_dev["n_taken_words"] = index["n_taken_words"]
    errs_sorted = errs[torch.from_numpy(index["order"]).cuda()].contiguous()
    thr, n_top_t = torch.from_numpy(c["thr"]).cuda(), torch.from_numpy(n_top).cuda()

    launch = lambda: eng.bop_match(errs_sorted, on_dev, thr, P, n_top=n_top_t)  # noqa: E731
    whole = lambda: ev.bop_match(cand, errs, c["scores"], c["thr"], n_top=n_top)  # noqa: E731
    n_bytes = n_cand * (E * 4 + 8) + sum(index[k].nbytes for k in eng.BOP_MATCH_INDEX[2:]) + n_groups * (E * n_theta * 8 + 4) + P * E * n_theta * 4
    src = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    t_a, t_b, t_d = timed(launch, args.reps), wall(whole, args.reps), timed(lambda: src.clone(), args.reps)
    # the host restatement on the first groups
    m = min(args.sample, n_groups)
    rows = c["group_id"] < m
    t0 = time.perf_counter()
    ref = bm.restated(c["pred_id"][rows], c["gt_id"][rows], c["group_id"][rows], c["errs"][rows], c["scores"], c["thr"][:m], n_top[:m])
    t_c = (time.perf_counter() - t0) * 1e3 * n_groups / m
    got = launch().cpu().numpy()
    in_sample = np.zeros(P, bool)
    in_sample[c["pred_id"][rows]] = True
    agree = bool(np.array_equal(got[in_sample], ref[in_sample]) and np.array_equal(got, whole().cpu().numpy()))
    n_cu, _, arch = eng.device_info()
    print(f"# {arch}, {n_cu} CUs; {n_frames} frames, {n_groups} groups, {P} estimates, {c['n_gt']} ground truths, {n_cand} candidates, {E} x {n_theta} problems "
          f"per group; {int((got >= 0).sum())} matches; host restatement timed on {m} groups and scaled")
    print(json.dumps(dict(name="bop_match", frames=n_frames, groups=n_groups, candidates=n_cand, E=E, n_theta=n_theta, launch_ms=t_a, with_index_ms=t_b,
                          host_numpy_ms_scaled=t_c, clone_ms=t_d, bytes=n_bytes, launch_gb_per_s=n_bytes / t_a / 1e6, clone_gb_per_s=n_bytes / t_d / 1e6,
                          ratio_launch_over_clone=t_a / t_d, host_over_launch=t_c / t_a, host_over_with_index=t_c / t_b, agree=agree)))
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
