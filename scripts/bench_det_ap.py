#!/usr/bin/env python3
"""Time the device side of BOP's detection / segmentation scores against what a user would otherwise write in torch and against a copy
of the bytes it reads and writes, on the same machine.

  workload  one BOP test set's worth, the groups of scripts/bench_bop_match.py: 1000 frames, 15 (image, label) groups per frame with 1-3
            ground truths and 1-4 detections each (about 75 k candidates) of 480 x 640 masks.  The masks of a frame's worth of rows are
            drawn once (--distinct of each kind: seeded rectangles with holes, bytes 1 for detections and 255 for ground truths) and
            row i uses mask i % distinct through the candidate table: the launch requests 2 * C masks (46 GB) out of a resident set of
            1.3 GB, five times the last-level cache; a distinct mask per row (20 GB) would need the memory and measure the same kernel
  (a) mp_mask_pair_counts alone (engine.mask_pair_counts; the zeroing of the counts is inside, as for every caller)
  (b) the same counts in torch: ((a != 0) & (b != 0)).sum() and the two areas per pair, gathered --chunk pairs at a time
  (c) torch.clone of as many bytes as (a) requests: 2 * C * H * W + the index and the counts
  (d) evaluation.coco_match on the IoUs with the index built on the host, and engine.det_match alone on a resident index
  (e) evaluation.coco_accumulate on the host

(a), (b), (c) and the resident (d) are device-event times, the rest wall-clock (host work is the point), all after warm-up, best of
--reps.  One header line, then one JSON line.

Usage: python scripts/bench_det_ap.py [--reps 5] [--quick]
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
sys.path.insert(0, str(ROOT / "scripts"))

from bench_bop_match import timed, wall  # noqa: E402
from megapose6d_amd import engine as eng  # noqa: E402
from megapose6d_amd import evaluation as ev  # noqa: E402
from support import bop_match as bm  # noqa: E402


def blobs(rng, n, h, w, value):
    m = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        x0, y0 = rng.randint(0, w - 80), rng.randint(0, h - 80)
        bw, bh = rng.randint(30, 200), rng.randint(30, 200)
        m[i, y0:y0 + bh, x0:x0 + bw] = value
        m[i, y0 + bh // 3:y0 + bh // 2, x0 + bw // 3:x0 + bw // 2] = 0
    return m


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=2048, help="distinct masks of each kind")
    ap.add_argument("--chunk", type=int, default=512, help="pairs the torch baseline gathers at a time")
    ap.add_argument("--quick", action="store_true", help="a twentieth of the frames (a functional check, not a measurement)")
    args = ap.parse_args()
    H, W = 480, 640
    n_frames = 1000 // (20 if args.quick else 1)
    rng = np.random.RandomState(0)
    sizes = [(int(rng.randint(1, 5)), int(rng.randint(1, 4))) for _ in range(15 * n_frames)]
    c = bm.case(0, sizes, 1, 1, nan_share=0.0)
    n_groups, n_cand, P, G = len(sizes), len(c["pred_id"]), c["n_pred"], c["n_gt"]
    cand = pd.DataFrame(dict(pred_id=c["pred_id"], gt_id=c["gt_id"], group_id=c["group_id"]))
    D = args.distinct
    pred_masks = torch.from_numpy(blobs(rng, D, H, W, 1)).cuda().view(torch.bool)
    gt_masks = torch.from_numpy(blobs(rng, D, H, W, 255)).cuda()
    pid = torch.from_numpy((c["pred_id"] % D).astype(np.int32)).cuda()
    gid = torch.from_numpy((c["gt_id"] % D).astype(np.int32)).cuda()

    launch = lambda: eng.mask_pair_counts(pred_masks, gt_masks, pid, gid)  # noqa: E731

    def in_torch():
        a, b = pred_masks.view(torch.uint8), gt_masks
        out = torch.empty(n_cand, 3, dtype=torch.int64, device="cuda")
        for c0 in range(0, n_cand, args.chunk):
            ma, mb = a[pid[c0:c0 + args.chunk].long()] != 0, b[gid[c0:c0 + args.chunk].long()] != 0
            out[c0:c0 + args.chunk, 0] = (ma & mb).flatten(1).sum(1)
            out[c0:c0 + args.chunk, 1] = ma.flatten(1).sum(1)
            out[c0:c0 + args.chunk, 2] = mb.flatten(1).sum(1)
        return out

    n_bytes = n_cand * (2 * H * W + 8 + 12)
    t_a, t_b = timed(launch, args.reps), timed(in_torch, args.reps)
    # a clone of as many bytes, in pieces of at most 2 GiB
    piece = torch.empty(min(n_bytes, 1 << 31), dtype=torch.uint8, device="cuda")
    n_pieces = -(-n_bytes // piece.numel())

    def clones():
        for _ in range(n_pieces):
            piece.clone()

    t_c = timed(clones, args.reps) * n_bytes / (n_pieces * piece.numel())
    counts = launch()
    agree = bool(torch.equal(counts.long(), in_torch()))
    del piece

    # the matching and the accumulation, on the IoUs of those counts
    cf = counts.double()
    union = cf[:, 1] + cf[:, 2] - cf[:, 0]
    iou = torch.where(union > 0, cf[:, 0] / union, torch.zeros_like(union))
    gt_ignore = rng.uniform(size=G) < 0.1
    whole = lambda: ev.coco_match(cand, iou, c["scores"], gt_ignore, n_top=100)  # noqa: E731
    index = ev.bop_match_index(c["pred_id"], c["gt_id"], c["group_id"], c["scores"])
    on_dev = {k: torch.from_numpy(index[k]).cuda() for k in eng.BOP_MATCH_INDEX}
    on_dev["n_taken_words"] = index["n_taken_words"]
    iou_sorted = iou[torch.from_numpy(index["order"]).cuda()].contiguous()
    thr, ign_dev = torch.from_numpy(ev.COCO_IOU_THRS).cuda(), torch.from_numpy(gt_ignore).cuda()
    resident = lambda: eng.det_match(iou_sorted, on_dev, ign_dev, thr, P)  # noqa: E731
    t_d, t_d0 = wall(whole, args.reps), timed(resident, args.reps)
    match = whole().cpu().numpy()
    agree = agree and bool(np.array_equal(match, resident().cpu().numpy()))
    labels_g = np.asarray(["obj_%02d" % (g % 15) for g in range(n_groups)])
    pred_labels, gt_labels = np.empty(P, labels_g.dtype), np.empty(G, labels_g.dtype)
    pred_labels[c["pred_id"]], gt_labels[c["gt_id"]] = labels_g[c["group_id"]], labels_g[c["group_id"]]
    kept = np.ones(P, bool)
    acc = lambda: ev.coco_accumulate(match, c["scores"], pred_labels, gt_labels, gt_ignore, kept)  # noqa: E731
    acc()
    t0 = time.perf_counter()
    scores = acc()
    t_e = (time.perf_counter() - t0) * 1e3
    n_cu, _, arch = eng.device_info()
    print(f"# {arch}, {n_cu} CUs; {n_frames} frames, {n_groups} groups, {P} detections, {G} ground truths, {n_cand} candidates of {H} x {W} masks, "
          f"{D} distinct masks of each kind; AP {scores['AP']:.4f}, AR {scores['AR']:.4f}; torch gathers {args.chunk} pairs at a time")
    print(json.dumps(dict(name="det_ap", frames=n_frames, groups=n_groups, candidates=n_cand, H=H, W=W, distinct=D, pair_counts_ms=t_a, torch_counts_ms=t_b,
                          clone_ms=t_c, bytes=n_bytes, pair_counts_gb_per_s=n_bytes / t_a / 1e6, clone_gb_per_s=n_bytes / t_c / 1e6,
                          ratio_pair_counts_over_clone=t_a / t_c, torch_over_pair_counts=t_b / t_a, coco_match_with_index_ms=t_d, det_match_ms=t_d0,
                          coco_accumulate_host_ms=t_e, agree=agree)))
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
