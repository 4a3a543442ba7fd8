#!/usr/bin/env python3
"""Time the VSD launch against the same VSD written in torch and against a copy of the bytes it must read, on the same GPU.

  workload  576 rows at 480 x 640, 10 taus: engine renders (Panda3dBatchRenderer.render_depth) of the synthetic objects, 24 estimates per
            ground truth, observed frames = the ground truths' renders plus noise (2 frames)
  (a) mp_vsd alone (engine.vsd on resident tensors; the workspace allocation is inside, as for every caller)
  (b) the definition restated in torch, chunked over rows only as far as memory forces it -- what a user would write otherwise
  (c) torch.clone of a tensor of the bytes (a) must read: 2 * b * h * w * 4 + n_im * h * w * 4

Device-event times after warm-up, best of --reps.  One JSON line: the three times, the achieved GB/s of (a) and (c), the ratio a / c.

Usage: python scripts/bench_vsd.py [--reps 5] [--quick]
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


def torch_vsd(d_est, d_gt, d_test, gt_ids, im_ids, K, diam, delta, taus, rows):
    """the definition, `rows` rows at a time -> errs [b, n_tau]"""
    b, h, w = d_est.shape
    xs = torch.arange(w, device=d_est.device, dtype=torch.float32)[None, None, :] + 0.5
    ys = torch.arange(h, device=d_est.device, dtype=torch.float32)[None, :, None] + 0.5
    taus_t = torch.tensor(taus, device=d_est.device, dtype=torch.float32)
    out = []
    for r0 in range(0, b, rows):
        sl = slice(r0, r0 + rows)
        Kc = K[sl]
        u = (xs - Kc[:, 0, 2, None, None]) / Kc[:, 0, 0, None, None]
        v = (ys - Kc[:, 1, 2, None, None]) / Kc[:, 1, 1, None, None]
        r = torch.sqrt(u * u + v * v + 1)
        t = d_test[im_ids[sl].long()]
        t = torch.where(torch.isfinite(t) & (t >= 0), t, torch.zeros_like(t)) * r
        e, g = d_est[sl] * r, d_gt[gt_ids[sl].long()] * r
        vis_gt = (g > 0) & ((t == 0) | (g - t <= delta))
        vis_est = (e > 0) & ((t == 0) | (e - t <= delta) | vis_gt)
        inter, union = vis_gt & vis_est, vis_gt | vis_est
        n_un, n_in = union.flatten(1).sum(1), inter.flatten(1).sum(1)
        gap = torch.where(inter, (g - e).abs(), torch.full_like(g, -1.0))
        thr = taus_t[None, :] * diam[sl, None]
        n_far = torch.stack([(gap >= thr[:, k, None, None]).flatten(1).sum(1) for k in range(len(taus))], dim=1)
        err = (n_far + (n_un - n_in)[:, None]).float() / n_un[:, None].float()
        out.append(torch.where(n_un[:, None] == 0, torch.ones_like(err), err))
    return torch.cat(out)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a twelfth of the rows (a functional check, not a measurement)")
    args = ap.parse_args()
    from megapose6d_amd.renderer import Panda3dBatchRenderer
    from tests.support import synthetic as syn

    h, w, n_gt, n_im = 480, 640, 24, 2
    b = 576 // (12 if args.quick else 1)
    taus = list(eng.VSD_TAUS)
    rng = np.random.RandomState(0)
    ds = syn.make_object_dataset(tempfile.mkdtemp(prefix="mp_bench_vsd_"), n_objects=3, seed=0)
    renderer = Panda3dBatchRenderer(ds, n_workers=1)
    labels = [o.label for o in ds.list_objects]
    K1 = torch.from_numpy(syn.K_EXAMPLE.astype(np.float32)).cuda()
    T_gt = np.stack([syn.random_pose(rng, (0.4, 0.7), 0.12) for _ in range(n_gt)]).astype(np.float32)
    gt_ids = torch.arange(b, dtype=torch.int32, device="cuda") % n_gt
    im_ids = gt_ids % n_im
    T_est = T_gt[gt_ids.cpu().numpy()].copy()
    T_est[:, :3, 3] += rng.randn(b, 3).astype(np.float32) * 0.008
    lab_gt = [labels[g % 3] for g in range(n_gt)]
    d_gt = renderer.render_depth(lab_gt, torch.from_numpy(T_gt).cuda(), K1[None].repeat(n_gt, 1, 1), (h, w))
    d_est = renderer.render_depth([lab_gt[g] for g in gt_ids.cpu().numpy()], torch.from_numpy(T_est).cuda(), K1[None].repeat(b, 1, 1), (h, w))
    frames = torch.full((n_im, h, w), 1.5, device="cuda")
    for g in range(n_gt):
        f = frames[g % n_im]
        take = (d_gt[g] > 0) & (d_gt[g] < f)
        f[take] = d_gt[g][take]
    frames = frames + torch.randn(n_im, h, w, device="cuda") * 0.002
    K = K1[None].repeat(b, 1, 1).contiguous()
    diam = torch.full((b,), 0.15, device="cuda")
    n_cu, _, arch = eng.device_info()

    fused = lambda: eng.vsd(d_est, d_gt, frames, K, diam, taus=taus, gt_ids=gt_ids, im_ids=im_ids, with_counts=False)  # noqa: E731
    free = torch.cuda.mem_get_info()[0]
    rows = max(1, min(b, (min(free // 4, 8 << 30)) // (h * w * 4 * 12)))      # about a dozen live [rows,h,w] intermediates
    ref = lambda: torch_vsd(d_est, d_gt, frames, gt_ids, im_ids, K, diam, 0.015, taus, rows)  # noqa: E731
    n_bytes = 2 * b * h * w * 4 + n_im * h * w * 4
    src = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    copy = lambda: src.clone()  # noqa: E731
    t_a, t_b, t_c = timed(fused, args.reps), timed(ref, args.reps), timed(copy, args.reps)
    agree = float((fused()["errs"] - ref()).abs().max())
    covered = float(((d_est > 0) | (d_gt[gt_ids.long()] > 0)).float().mean())
    print(f"# {arch}, {n_cu} CUs; {b} rows at {h} x {w}, {len(taus)} taus; rendered share of the pixels {covered:.3f}; torch rows per chunk {rows}")
    print(json.dumps(dict(name="vsd", rows=b, h=h, w=w, n_tau=len(taus), vsd_ms=t_a, torch_ms=t_b, clone_ms=t_c, bytes_read=n_bytes,
                          vsd_gb_per_s=n_bytes / t_a / 1e6, clone_read_gb_per_s=n_bytes / t_c / 1e6, ratio_vsd_over_clone=t_a / t_c,
                          torch_over_vsd=t_b / t_a, max_abs_diff_vs_torch=agree)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
