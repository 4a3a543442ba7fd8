#!/usr/bin/env python3
"""Time the run-length encoding of masks (csrc/rle.hip) against the same result formulated in torch and against a copy of the bytes it
reads, on the same machine.

  workload  64 masks of 480 x 640, one seeded ellipse each covering about a tenth of the frame (bytes 0 / 1)
  (a) the product call, engine.rle_encode: count, the read-back of the 64 list lengths, encode; and engine.rle_decode of its result
  (b) the same lists in torch on the device: transpose to column-major, `!=` with the copy shifted by one pixel, nonzero (its own
      synchronisation), the differences of the positions; checked equal to (a) before anything is timed
  (c) torch.clone of the mask bytes

All three are wall-clock times around a device synchronise (the read-back is part of (a), nonzero's part of (b)), after warm-up; the
three are run in turn --reps times and the best and the median of each are reported, with the ratios of the bests.  One header line, then
one JSON line.

Usage: python scripts/bench_rle.py [--reps 30] [--masks 64]
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
from tests.support import rle as sr  # noqa: E402


def torch_encode(masks: torch.Tensor):
    """counts [total] int32 and offsets [n + 1] int64 of uint8 masks [n,h,w], in torch"""
    n, h, w = masks.shape
    hw = h * w
    v = (masks != 0).transpose(1, 2).reshape(n, hw)                       # column-major
    before = torch.cat([torch.zeros(n, 1, dtype=torch.bool, device=v.device), v[:, :-1]], dim=1)
    idx = torch.nonzero(v != before)                                       # [T,2]: mask, position; sorted
    n_counts = torch.bincount(idx[:, 0], minlength=n) + 1
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=v.device), torch.cumsum(n_counts, 0)])
    ends = torch.full((int(idx.shape[0]) + n,), hw, dtype=torch.int64, device=v.device)   # each list ends at h * w
    ends[torch.arange(idx.shape[0], device=v.device) + idx[:, 0]] = idx[:, 1]
    start = torch.roll(ends, 1)
    start[offsets[:-1]] = 0
    return (ends - start).to(torch.int32), offsets


def wall_once(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--masks", type=int, default=64)
    args = ap.parse_args()
    n, h, w = args.masks, 480, 640
    host = sr.blobs(n, h, w, seed=0, share=0.1)
    masks = torch.from_numpy(host).cuda()
    counts, offsets, areas, _ = eng.rle_encode(masks)
    t_counts, t_offsets = torch_encode(masks)
    back, status = eng.rle_decode(counts, offsets, h, w)
    agree = bool(torch.equal(counts, t_counts) and torch.equal(offsets, t_offsets) and torch.equal(back, (masks != 0).to(torch.uint8))
                 and not status.any())
    h_offsets = offsets.cpu().numpy()
    runs = {"encode": lambda: eng.rle_encode(masks), "decode": lambda: eng.rle_decode(counts, h_offsets, h, w),
            "torch_encode": lambda: torch_encode(masks), "clone": lambda: masks.clone()}
    for fn in runs.values():                                               # warm-up: code objects, the allocator's pools
        for _ in range(3):
            fn()
    times = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            times[k].append(wall_once(fn))
    best = {k: min(v) for k, v in times.items()}
    median = {k: statistics.median(v) for k, v in times.items()}
    n_cu, _, arch = eng.device_info()
    print(f"# {arch}, {n_cu} CUs; {n} masks of {h} x {w} ({masks.numel() / 1e6:.1f} MB), mean coverage {float(areas.double().mean()) / (h * w):.3f}, "
          f"{int(counts.numel())} counts ({counts.numel() * 4 / 1e3:.1f} kB); {args.reps} reps in turn, wall clock around a synchronise")
    print(json.dumps(dict(name="rle", masks=n, H=h, W=w, mask_bytes=int(masks.numel()), counts=int(counts.numel()), reps=args.reps,
                          encode_ms=best["encode"], decode_ms=best["decode"], torch_encode_ms=best["torch_encode"], clone_ms=best["clone"],
                          encode_median_ms=median["encode"], decode_median_ms=median["decode"], torch_encode_median_ms=median["torch_encode"],
                          clone_median_ms=median["clone"], torch_over_encode=best["torch_encode"] / best["encode"],
                          encode_over_clone=best["encode"] / best["clone"], decode_over_clone=best["decode"] / best["clone"], agree=agree)))
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
