#!/usr/bin/env python3
"""Time the overlay launch against the same arithmetic written in torch and against a copy of the bytes it moves, on the same GPU.

  workload  n images of 480 x 640 (n = 1 and n = 32) with 8 instances each (seeded ellipses that overlap one another and the image
            border), an observed image, a render and the instance map; dilate_iterations = 1; all four outputs
  (a) mp_overlay alone (engine.overlay on resident tensors; the output allocation is inside, as for every caller): it reads 3 + 3 + 4
      bytes per pixel and writes 3 + 3 + 1 + 1
  (b) the same arithmetic in torch on the device, all labels of all images at once: conv2d Sobel on the replicated-border masks, the
      suppression rule on shifted magnitudes, max_pool2d for the dilation, `where` for the painting and the blend
  (c) torch.clone of a tensor of half the bytes (a) moves (a clone reads and writes each byte once): 9 bytes per pixel
  (d) mp_draw_boxes with 8 boxes per image

Device-event times after warm-up; a sample is the mean of --inner back-to-back calls, --reps samples per variant, the variants taken in
turn so that a drift of the machine hits all of them.  Per variant: median, fastest, and the 10th and 90th percentile.  One JSON line per n.

Usage: python scripts/bench_overlay.py [--reps 30] [--inner 20] [--quick]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from megapose6d_amd import engine as eng  # noqa: E402
from megapose6d_amd.visualization import DEFAULT_PALETTE  # noqa: E402

N_OBJECTS = 8


def make_batch(n, h, w, seed=0):
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    labels = np.full((n, h, w), -1, np.int32)
    boxes, ids = [], []
    for i in range(n):
        for l in range(N_OBJECTS):
            cy, cx = rng.uniform(0, h), rng.uniform(0, w)
            ry, rx = rng.uniform(0.08, 0.2) * h, rng.uniform(0.08, 0.2) * w
            labels[i][((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0] = l
            boxes.append([cx - rx, cy - ry, cx + rx, cy + ry])
            ids.append(i)
    images = rng.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    render = rng.randint(1, 256, size=(n, h, w, 3)).astype(np.uint8)
    render[labels < 0] = 0
    return images, render, labels, np.asarray(boxes, np.float32), np.asarray(ids, np.int32)


def torch_overlay(images, render, labels, colors, k, tables):
    """contour, canny, mask, mesh as mp_overlay defines them, for labels 0 .. N_OBJECTS - 1"""
    n, h, w = labels.shape
    ls = torch.arange(N_OBJECTS, device=labels.device, dtype=labels.dtype)
    m = (labels[:, None] == ls[None, :, None, None]).float().reshape(n * N_OBJECTS, 1, h, w)
    sob = torch.tensor([[[-1.0, 0, 1], [-2, 0, 2], [-1, 0, 1]], [[-1, -2, -1], [0, 0, 0], [1, 2, 1]]], device=m.device)[:, None]
    g = F.conv2d(F.pad(m, (1, 1, 1, 1), mode="replicate"), sob).to(torch.int32)
    gx, gy = g[:, 0], g[:, 1]
    ax, ayi = gx.abs(), gy.abs()
    mag = ax + ayi
    mz = F.pad(mag, (1, 1, 1, 1))

    def at(dx, dy):
        return mz[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    ay, t = ayi << 15, ax * 13573
    horizontal = ay < t
    vertical = ~horizontal & (ay > t + (ax << 16))
    keep = torch.where(horizontal, (mag > at(-1, 0)) & (mag >= at(1, 0)),
                       torch.where(vertical, (mag > at(0, -1)) & (mag >= at(0, 1)),
                                   torch.where((gx ^ gy) < 0, (mag > at(1, -1)) & (mag > at(-1, 1)), (mag > at(-1, -1)) & (mag > at(1, 1)))))
    edge = ((mag != 0) & keep).reshape(n, N_OBJECTS, h, w)
    e = torch.where(edge, ls[None, :, None, None].float(), torch.full((), -1.0, device=m.device)).amax(1, keepdim=True)
    out = (F.max_pool2d(e, 2 * k + 1, stride=1, padding=k) if k else e)[:, 0].long()     # max_pool2d pads with -inf: only the image counts
    on = out >= 0
    contour = torch.where(on[..., None], colors[out.clamp(min=0) % colors.shape[0]], images)
    canny = on.to(torch.uint8) * 255
    obj = labels >= 0
    mask = obj.to(torch.uint8) * 255
    mesh = torch.where(obj[..., None], tables[0][render.long()], tables[1][images.long()])
    return dict(contour=contour, canny=canny, mask=mask, mesh=mesh)


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def stats(v):
    v = np.sort(np.asarray(v))
    return dict(median_ms=float(np.median(v)), min_ms=float(v[0]), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="n = 1 and 2, few repetitions (a functional check, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_overlay.py needs the GPU", file=sys.stderr)
        return 1
    h, w, k = 480, 640, 1
    reps, inner = (3, 2) if args.quick else (args.reps, args.inner)
    n_cu, _, arch = eng.device_info()
    colors = torch.tensor(DEFAULT_PALETTE, dtype=torch.uint8, device="cuda")
    v = np.arange(256, dtype=np.uint8)
    t_obj, t_bg = np.zeros(256, np.float32), np.zeros(256, np.float32)
    t_obj[:], t_bg[:] = v * 0.8 + 255 * 0.2, v * 0.6 + 255 * 0.4
    tables = (torch.from_numpy(t_obj.astype(np.uint8)).cuda(), torch.from_numpy(t_bg.astype(np.uint8)).cuda())
    print(f"# {arch}, {n_cu} CUs; {h} x {w}, {N_OBJECTS} instances per image, dilate_iterations {k}; {reps} samples of {inner} calls per variant")
    for n in ((1, 2) if args.quick else (1, 32)):
        images, render, labels, boxes, ids = (torch.from_numpy(a).cuda() for a in make_batch(n, h, w))
        px = n * h * w
        moved = px * (10 + 8)
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        variants = dict(overlay=lambda: eng.overlay(images, render=render, labels=labels, colors=colors, dilate_iterations=k),
                        torch=lambda: torch_overlay(images, render, labels, colors, k, tables),
                        clone=lambda: src.clone(),
                        draw_boxes=lambda: eng.draw_boxes(images, boxes, ids, colors=colors, thickness=2))
        got, ref = variants["overlay"](), variants["torch"]()
        agree = all(torch.equal(got[name], ref[name]) for name in ref)
        for fn in variants.values():   # warm-up of every shape
            sample(fn, inner)
        times = {name: [] for name in variants}
        for _ in range(reps):
            for name, fn in variants.items():
                times[name].append(sample(fn, inner))
        res = {name: stats(t) for name, t in times.items()}
        a, c = res["overlay"]["median_ms"], res["clone"]["median_ms"]
        print(json.dumps(dict(name="overlay", n=n, h=h, w=w, n_objects=N_OBJECTS, dilate_iterations=k, bytes_moved=moved, **{f"{name}_{key}": val for name, r in res.items() for key, val in r.items()},
                              overlay_gb_per_s=moved / a / 1e6, clone_gb_per_s=moved / c / 1e6, fraction_of_clone_bandwidth=c / a,
                              torch_over_overlay=res["torch"]["median_ms"] / a, equals_torch=bool(agree))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
