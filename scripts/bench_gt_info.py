#!/usr/bin/env python3
"""Time the ground-truth-info launch against the same arithmetic written in torch and against a copy of the bytes it must read, on the
same GPU, and the render of the canvases next to it.

  workload  576 rows at 480 x 640, canvas 3: engine renders (Panda3dBatchRenderer.render_depth) of the synthetic objects on the nine
            tile intrinsics, 24 distinct ground-truth canvases shared by the rows, observed frames = the ground truths' renders plus
            noise (2 frames)
  (a) mp_gt_info alone, without and with the two masks (engine.gt_info on resident tensors; the workspace allocation is inside)
  (b) the definition restated in torch, chunked over rows only as far as memory forces it -- what a user would write otherwise
  (c) torch.clone of a tensor of the bytes (a) must read: b * 9 * h * w * 4 + n_im * h * w * 4
  render    the nine tiles of the 24 canvases (216 maps), and mp_gt_info on those 24 rows: the two parts of `evaluation.gt_info`

Device-event times after warm-up, best of --reps.  One JSON line: the times, the achieved GB/s of (a) and (c), the ratio a / c, the
render's share.

Usage: python scripts/bench_gt_info.py [--reps 5] [--quick]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from megapose6d_amd import engine as eng  # noqa: E402


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


def _first_last(flags):
    """flags [r, n] bool -> first and last set index per row (-1, -1 over none)"""
    n = flags.shape[1]
    any_ = flags.any(1)
    first = flags.int().argmax(1)
    last = n - 1 - flags.flip(1).int().argmax(1)
    neg = torch.full_like(first, -1)
    return torch.where(any_, first, neg), torch.where(any_, last, neg), any_


def _box(m, x_off, y_off):
    """m [r, H, W] bool -> [r,4] inclusive extents shifted, -1 over no pixel"""
    x0, x1, ok = _first_last(m.any(1))
    y0, y1, _ = _first_last(m.any(2))
    box = torch.stack([x0 + x_off, y0 + y_off, x1 + x_off, y1 + y_off], dim=1)
    return torch.where(ok[:, None], box, torch.full_like(box, -1))


def torch_gt_info(d_gt, d_test, gt_ids, im_ids, K, delta, rows):
    """the definition, `rows` rows at a time -> counts [b,4], boxes [b,8], visib_fract [b]"""
    _, _, h, w = d_gt.shape
    xs = torch.arange(w, device=K.device, dtype=torch.float32)[None, None, :] + 0.5
    ys = torch.arange(h, device=K.device, dtype=torch.float32)[None, :, None] + 0.5
    counts, boxes = [], []
    for r0 in range(0, K.shape[0], rows):
        sl = slice(r0, r0 + rows)
        Kc = K[sl]
        g = d_gt[gt_ids[sl].long()]                                                   # [r,9,h,w]
        n = g.shape[0]
        whole = (g > 0).view(n, 3, 3, h, w).permute(0, 1, 3, 2, 4).reshape(n, 3 * h, 3 * w)   # the canvas as one picture
        u = (xs - Kc[:, 0, 2, None, None]) / Kc[:, 0, 0, None, None]
        v = (ys - Kc[:, 1, 2, None, None]) / Kc[:, 1, 1, None, None]
        r = torch.sqrt(u * u + v * v + 1)
        t = d_test[im_ids[sl].long()]
        t = torch.where(torch.isfinite(t) & (t >= 0), t, torch.zeros_like(t)) * r
        dg = g[:, 4] * r
        obj = g[:, 4] > 0
        vis = (dg > 0) & ((t == 0) | (dg - t <= delta))
        counts.append(torch.stack([whole.flatten(1).sum(1), obj.flatten(1).sum(1), (obj & (t > 0)).flatten(1).sum(1), vis.flatten(1).sum(1)], dim=1))
        boxes.append(torch.cat([_box(whole, -w, -h), _box(vis, 0, 0)], dim=1))
    counts, boxes = torch.cat(counts), torch.cat(boxes)
    fract = torch.where(counts[:, 0] == 0, torch.zeros(len(counts), device=K.device), counts[:, 3].float() / counts[:, 0].float())
    return counts, boxes, fract


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a twelfth of the rows and a sixth of the canvases (a functional check, not a measurement)")
    args = ap.parse_args()
    from megapose6d_amd import evaluation as ev
    from megapose6d_amd.renderer import Panda3dBatchRenderer
    from tests.support import synthetic as syn

    h, w, n_im, canvas = 480, 640, 2, 3
    n_gt = 24 // (6 if args.quick else 1)
    b = 576 // (12 if args.quick else 1)
    rng = np.random.RandomState(0)
    ds = syn.make_object_dataset(tempfile.mkdtemp(prefix="mp_bench_gt_info_"), n_objects=3, seed=0)
    renderer = Panda3dBatchRenderer(ds, n_workers=1)
    labels = [o.label for o in ds.list_objects]
    K1 = torch.from_numpy(syn.K_EXAMPLE.astype(np.float32)).cuda()
    T_gt = np.stack([syn.random_pose(rng, (0.4, 0.7), 0.12) for _ in range(n_gt)]).astype(np.float32)
    T_gt[::4, 0, 3] -= 0.25                                      # every fourth object hangs over the left edge
    T_gt = torch.from_numpy(T_gt).cuda()
    lab_tiles = [labels[g % 3] for g in range(n_gt) for _ in range(canvas * canvas)]
    K_tiles = ev.tile_intrinsics(K1[None].repeat(n_gt, 1, 1), canvas, (h, w)).flatten(0, 1)
    render = lambda: renderer.render_depth(lab_tiles, T_gt.repeat_interleave(canvas * canvas, dim=0), K_tiles, (h, w))  # noqa: E731
    d_gt = render().view(n_gt, canvas * canvas, h, w)
    gt_ids = torch.arange(b, dtype=torch.int32, device="cuda") % n_gt
    im_ids = gt_ids % n_im
    frames = torch.full((n_im, h, w), 1.5, device="cuda")
    for g in range(n_gt):
        f = frames[g % n_im]
        take = (d_gt[g, 4] > 0) & (d_gt[g, 4] < f)
        f[take] = d_gt[g, 4][take]
    frames = frames + torch.randn(n_im, h, w, device="cuda") * 0.002
    K = K1[None].repeat(b, 1, 1).contiguous()
    n_cu, _, arch = eng.device_info()

    fused = lambda m: eng.gt_info(d_gt, frames, K, canvas=canvas, gt_ids=gt_ids, im_ids=im_ids, with_masks=m)  # noqa: E731
    per_gt = lambda: eng.gt_info(d_gt, frames, K[:n_gt], canvas=canvas, im_ids=im_ids[:n_gt])  # noqa: E731
    free = torch.cuda.mem_get_info()[0]
    rows = max(1, min(b, (min(free // 4, 16 << 30)) // (h * w * 4 * 16)))         # the gathered canvases and a few [rows,h,w] intermediates
    ref = lambda: torch_gt_info(d_gt, frames, gt_ids, im_ids, K, 0.015, rows)  # noqa: E731
    n_bytes = b * canvas * canvas * h * w * 4 + n_im * h * w * 4
    src = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    copy = lambda: src.clone()  # noqa: E731
    t_a, t_am = timed(lambda: fused(False), args.reps), timed(lambda: fused(True), args.reps)
    t_b, t_c = timed(ref, args.reps), timed(copy, args.reps)
    t_r, t_g = timed(render, args.reps), timed(per_gt, args.reps)
    got, (rc, rb, rf) = fused(False), ref()
    agree = int(max((got["counts"] - rc).abs().max(), (got["boxes"] - rb).abs().max()))
    covered = float((d_gt[:, 4] > 0).float().mean())
    print(f"# {arch}, {n_cu} CUs; {b} rows at {h} x {w}, canvas {canvas}, {n_gt} canvases, {n_im} frames; rendered share of the image pixels {covered:.3f}; "
          f"visib_fract {float(got['visib_fract'].min()):.3f} .. {float(got['visib_fract'].max()):.3f}; torch rows per chunk {rows}")
    print(json.dumps(dict(name="gt_info", rows=b, h=h, w=w, canvas=canvas, gt_info_ms=t_a, gt_info_masks_ms=t_am, torch_ms=t_b, clone_ms=t_c,
                          bytes_read=n_bytes, gt_info_gb_per_s=n_bytes / t_a / 1e6, clone_read_gb_per_s=n_bytes / t_c / 1e6, ratio_gt_info_over_clone=t_a / t_c,
                          ratio_masks_over_clone=t_am / t_c, torch_over_gt_info=t_b / t_a, max_abs_diff_vs_torch=agree, render_canvases=n_gt,
                          render_ms=t_r, gt_info_per_canvas_rows_ms=t_g, render_share=t_r / (t_r + t_g))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
