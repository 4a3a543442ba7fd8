#!/usr/bin/env python3
"""Time the three launches of the training-free detector against the same arithmetic written in torch, and the match launch against the
time to read its response maps once, on the same GPU.

  workload  one 480 x 640 frame with two synthetic objects over a noise background (tests/support/scene.render_observation); templates of
            the two objects at 576 viewpoints x 3 distances (TemplateSet.from_objects, up to 63 features each); T = 8
  (a) mp_tm_quantize, mp_tm_response, mp_tm_match, each alone on resident tensors (the output allocation is inside, as for every caller)
  (b) the same arithmetic in torch on the device: conv2d for the binomial and the Sobel, integer comparisons for the bin, a 3x3 count for
      the majority; shifted ORs and a permute for the response maps; for the match a gather of every (template, feature, location) byte in
      chunks of templates, a sum and the cross-multiplied comparison.  Each is compared with the launch it restates.
  (c) torch.clone of a tensor of half the response maps' bytes (a clone reads and writes each byte once): the time to move the maps' bytes
      once, the floor of a launch that reads them once.  The match launch reads far more: `match_byte_reads` counts them from the table
      (per template f bytes at every valid location) and `match_read_gb_per_s` is that count over the launch's time; the lanes of a wave
      read 2 x 32 consecutive bytes per instruction, so `match_wave_loads` (reads / 64) is the number of vector loads that carries them.

Device-event times after warm-up; a sample is the mean of --inner back-to-back calls, --reps samples per variant, the variants taken in
turn so that a drift of the machine hits all of them.  Per variant: median, fastest, and the 10th and 90th percentile.  One JSON line.

Usage: python scripts/bench_template_match.py [--reps 20] [--inner 5] [--quick]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from megapose6d_amd import engine as eng  # noqa: E402
from megapose6d_amd.template_detector import TemplateMatchingModel, TemplateSet  # noqa: E402


def torch_quantize(images, blur, weak):
    n, h, w, _ = images.shape
    x = images.permute(0, 3, 1, 2).float().reshape(n * 3, 1, h, w)          # integers below 2^24: float32 is exact
    if blur:
        k = torch.tensor([1.0, 4, 6, 4, 1], device=x.device)
        s = F.conv2d(F.pad(x, (2, 2, 2, 2), mode="replicate"), (k[:, None] * k[None])[None, None])
        x = ((s.int() + 128) >> 8).float()
    sob = torch.tensor([[[-1.0, 0, 1], [-2, 0, 2], [-1, 0, 1]], [[-1, -2, -1], [0, 0, 0], [1, 2, 1]]], device=x.device)[:, None]
    g = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), sob).long().reshape(n, 3, 2, h, w)
    m = (g * g).sum(2)
    ch = m.argmax(1, keepdim=True)                                           # the first maximum: the lowest channel
    mag2 = m.gather(1, ch)[:, 0]
    gx, gy = g[:, :, 0].gather(1, ch)[:, 0], g[:, :, 1].gather(1, ch)[:, 0]
    flip = (gy < 0) | ((gy == 0) & (gx < 0))
    gx, gy = torch.where(flip, -gx, gx), torch.where(flip, -gy, gy)
    a, b = gx.abs(), gy
    under_22, under_67 = (b + a) ** 2 < 2 * a * a, (b < a) | ((b - a) ** 2 < 2 * a * a)
    first = torch.where(under_22, 0, torch.where(b < a, 1, torch.where(under_67, 2, 3)))
    second = torch.where(under_22, 7, torch.where(b <= a, 6, torch.where(under_67, 5, 4)))
    bins = torch.where(gx > 0, first, torch.where(gx == 0, torch.full_like(first, 4), second))
    cand = (mag2 >= weak * weak) & (mag2 > 0)
    onehot = (F.one_hot(bins, 8).permute(0, 3, 1, 2) & cand[:, None]).float()
    votes = F.conv2d(onehot.reshape(n * 8, 1, h, w), torch.ones(1, 1, 3, 3, device=x.device), padding=1).reshape(n, 8, h, w)
    ori = ((votes >= 5).long() << torch.arange(8, device=x.device)[None, :, None, None]).sum(1).to(torch.uint8)
    return ori, mag2.int()


def torch_response(ori, T):
    n, h, w = ori.shape
    gh, gw = -(-h // T), -(-w // T)
    p = F.pad(ori, (0, gw * T - w + T - 1, 0, gh * T - h + T - 1))
    s = torch.zeros((n, gh * T, gw * T), dtype=torch.uint8, device=ori.device)
    for dy in range(T):
        for dx in range(T):
            s |= p[:, dy:dy + gh * T, dx:dx + gw * T]
    inside = torch.zeros_like(s, dtype=torch.bool)
    inside[:, :h, :w] = True
    s = torch.where(inside, s, torch.zeros_like(s)).int()
    o = torch.arange(8, device=ori.device)[None, :, None, None]
    same = (s[:, None] >> o) & 1
    near = ((s[:, None] >> ((o + 1) % 8)) | (s[:, None] >> ((o + 7) % 8))) & 1
    r = torch.where(same == 1, 4, torch.where(near == 1, 1, 0)).to(torch.uint8)      # [n,8,gh T,gw T]
    return r.reshape(n, 8, gh, T, gw, T).permute(0, 1, 3, 5, 2, 4).contiguous()


def torch_match(resp, h, w, templates, features, n_objects, chunk=48):
    n, _, T, _, gh, gw = resp.shape
    dev = resp.device
    plane = gh * gw
    t = templates.long()
    n_t = t.shape[0]
    slot = torch.arange(63, device=dev)[None]
    used = slot < t[:, 2:3]                                                   # [t,63]
    fi = (t[:, 1:2] + slot).clamp(max=features.shape[0] - 1)
    f = features.long()[fi]                                                   # [t,63,4]
    base = (((f[..., 2] * T + f[..., 1] % T) * T + f[..., 0] % T) * plane + (f[..., 1] // T) * gw + f[..., 0] // T)
    gy, gx = torch.meshgrid(torch.arange(gh, device=dev), torch.arange(gw, device=dev), indexing="ij")
    loc = (gy * gw + gx).reshape(-1)
    valid = ((gx.reshape(-1)[None] * T + t[:, 3:4] <= w) & (gy.reshape(-1)[None] * T + t[:, 4:5] <= h))     # [t,L]
    best_s = torch.zeros((n, n_objects, plane), dtype=torch.long, device=dev)
    best_f = torch.zeros_like(best_s)
    best_t = torch.full_like(best_s, -1)
    for i in range(n):
        flat = resp[i].reshape(-1)
        for c0 in range(0, n_t, chunk):
            sl = slice(c0, min(c0 + chunk, n_t))
            idx = base[sl, :, None] + loc[None, None]
            ok = valid[sl, None] & used[sl, :, None]
            score = torch.where(ok, flat[torch.where(ok, idx, torch.zeros_like(idx))].long(), torch.zeros_like(idx)).sum(1)      # [c,L]
            for j in range(sl.stop - sl.start):                                # ascending index: a tie keeps the earlier template
                tt = c0 + j
                o, ff = int(t[tt, 0]), int(t[tt, 2])
                wins = valid[tt] & ((best_t[i, o] < 0) | (score[j] * best_f[i, o] > best_s[i, o] * ff))
                best_s[i, o] = torch.where(wins, score[j], best_s[i, o])
                best_f[i, o] = torch.where(wins, torch.full_like(best_f[i, o], ff), best_f[i, o])
                best_t[i, o] = torch.where(wins, torch.full_like(best_t[i, o], tt), best_t[i, o])
    shape = (n, n_objects, gh, gw)
    return best_s.to(torch.uint8).reshape(shape), best_f.to(torch.uint8).reshape(shape), best_t.int().reshape(shape)


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="72 viewpoints x 1 distance at 120 x 160, few repetitions (a functional check, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_template_match.py needs the GPU", file=sys.stderr)
        return 1
    from megapose6d_amd.renderer import Panda3dBatchRenderer
    from tests.support import scene
    from tests.support import synthetic as syn

    T = 8
    (h, w), views, distances = ((120, 160), 72, (0.5,)) if args.quick else ((480, 640), 576, (0.4, 0.55, 0.7))
    reps, inner = (2, 1) if args.quick else (args.reps, args.inner)
    K = syn.K_EXAMPLE.astype(np.float32).copy()
    if args.quick:
        K[:2] *= 0.25
    n_cu, _, arch = eng.device_info()
    ds = syn.make_object_dataset(tempfile.mkdtemp(prefix="mp_tm_bench_"), n_objects=2, seed=0)
    renderer = Panda3dBatchRenderer(ds, n_workers=1, preload_cache=True)
    t0 = time.time()
    ts = TemplateSet.from_objects(ds, K, (h, w), viewpoints=views, distances=distances, renderer=renderer)
    build_s = time.time() - t0
    labels = [o.label for o in ds.list_objects]
    rng = np.random.RandomState(100)
    poses = np.stack([syn.random_pose(rng, z_range=(0.45, 0.65), xy_frac=0.25) for _ in labels])
    obs, _ = scene.render_observation(renderer, labels, poses, K, seed=0, hw=(h, w))
    renderer.stop()
    images = torch.round(obs[:, :3] * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    model = TemplateMatchingModel(ts, T=T)
    print(f"# {arch}, {n_cu} CUs; {h} x {w}, {len(ts)} templates ({ts.n_dropped} renders dropped) of 2 objects, {len(ts.features)} features, T {T}; "
          f"templates built in {build_s:.1f} s; {reps} samples of {inner} calls per variant")
    ori, _ = eng.tm_quantize(images, blur=ts.blur, weak_threshold=ts.weak_threshold)
    resp = eng.tm_response(ori, T)
    match = lambda: eng.tm_match(resp, h, w, ts.d_templates, ts.d_features, ts.n_objects, ts.templates, ts.features)   # noqa: E731
    src = torch.empty(resp.numel() // 2, dtype=torch.uint8, device="cuda")
    variants = dict(quantize=lambda: eng.tm_quantize(images, blur=ts.blur, weak_threshold=ts.weak_threshold),
                    torch_quantize=lambda: torch_quantize(images, ts.blur, ts.weak_threshold),
                    response=lambda: eng.tm_response(ori, T), torch_response=lambda: torch_response(ori, T),
                    match=match, torch_match=lambda: torch_match(resp, h, w, ts.d_templates, ts.d_features, ts.n_objects),
                    clone_of_the_maps=lambda: src.clone())
    agree = dict(quantize=all(torch.equal(a, b) for a, b in zip(variants["quantize"](), variants["torch_quantize"]())),
                 response=torch.equal(resp, variants["torch_response"]()),
                 match=all(torch.equal(a, b) for a, b in zip(match(), variants["torch_match"]())))
    slow = {"torch_match"}                                                     # seconds per call: one call per sample, fewer samples
    for name, fn in variants.items():
        sample(fn, 1 if name in slow else inner)
    times = {name: [] for name in variants}
    for r in range(reps):
        for name, fn in variants.items():
            if name in slow and r >= max(reps // 5, 2):
                continue
            times[name].append(sample(fn, 1 if name in slow else inner))
    res = {name: stats(v) for name, v in times.items()}
    gh, gw = -(-h // T), -(-w // T)
    t = ts.templates.astype(np.int64)
    ny = np.where(t[:, 4] <= h, (h - t[:, 4]) // T + 1, 0)
    nx = np.where(t[:, 3] <= w, (w - t[:, 3]) // T + 1, 0)
    reads = int((t[:, 2] * ny * nx).sum()) * images.shape[0]
    out = model.detections_from_match(*match(), hw=(h, w))[0]
    m = res["match"]["median_ms"]
    print(json.dumps(dict(name="template_match", h=h, w=w, T=T, n_templates=len(ts), n_features=int(len(ts.features)), n_dropped=ts.n_dropped, gh=gh, gw=gw,
                          resp_bytes=resp.numel(), match_byte_reads=reads, match_wave_loads=reads // 64, match_read_gb_per_s=reads / m / 1e6,
                          match_wave_loads_per_us=reads / 64 / m / 1e3, match_over_one_read_of_the_maps=m / res["clone_of_the_maps"]["median_ms"],
                          **{f"{name}_{key}": val for name, r in res.items() for key, val in r.items()},
                          torch_over_quantize=res["torch_quantize"]["median_ms"] / res["quantize"]["median_ms"],
                          torch_over_response=res["torch_response"]["median_ms"] / res["response"]["median_ms"],
                          torch_over_match=res["torch_match"]["median_ms"] / m, equals_torch=agree,
                          detections=[dict(label=labels[int(l) - 1], score=round(float(s), 4)) for l, s in zip(out["labels"], out["scores"])])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
