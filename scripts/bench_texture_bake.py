#!/usr/bin/env python3
"""Time the texture bake (csrc/texture_bake.hip) against the same arithmetic formulated in torch and against a copy of the bytes it
touches, on the same machine.

  workload  32 views of 480 x 640 (f = 600) of the analytic sphere of the tests, cameras on a spiral over the sphere of directions at
            0.4 m, with masks and colours; the icosphere at 4 and 5 subdivisions (5 120 and 20 480 faces) with vertex colours; atlases of
            1024 and 2048 texels a side
  (a) the product call: engine.texture_bake (one launch for all views), and engine.texture_atlas_uvs
  (b) the same arithmetic in torch on the device: the contract's steps (csrc/texture_bake_core.h) as whole-atlas float32 operations,
      view by view.  `seen` and the texels are compared with (a) before anything is timed (torch may contract or reorder nothing here,
      but its results are only reported, not required).
  Before anything is timed, texels, seen and the coordinates of (a) at the first size are compared byte for byte with the host
  emulation of the tests (tests/texture_bake_emul.cpp), so the table rests on checked results; a difference ends the run with exit code 1.
  (c) torch.clone of the two outputs and of the frames (depth, masks, colours): the floor of a pass that reads every frame byte once and
      writes every output byte once.  The bake reads only the pixels the charts project to, but each of them from several texels.

Wall-clock times around a device synchronise, after warm-up; the runs take turns --reps times and the best and the median of each are
reported, with texel visits per second (chart texels x views / best time).  One header line, then one JSON line per case.

Usage: python scripts/bench_texture_bake.py [--reps 10] [--views 32] [--subdivisions 4 5] [--sizes 1024 2048]
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
from tests.support import texture_bake as tb  # noqa: E402
from tests.support import tsdf as st  # noqa: E402

H, W, FOCAL = 480, 640, 600.0
DEPTH_TOL, COS_MIN, Z_MIN = 2e-3, 0.2, 1e-3


def make_views(n: int):
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    dirs = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    cams = np.stack([st.look_at(0.4 * d, up=(0, 0, 1) if abs(d[2]) < 0.9 else (0, 1, 0)) for d in dirs])
    K = st.intrinsics(FOCAL, H, W)
    depth = np.stack([st.sphere_depth(T, K, h=H, w=W) for T in cams])
    rgb = np.stack([st._surface_rgb(d, T, K) for d, T in zip(depth, cams)])
    return dict(depth=depth.astype(np.float32), masks=(depth > 0).astype(np.uint8), rgb=rgb, K=np.repeat(K[None], n, 0).astype(np.float32),
                TCO=cams.astype(np.float32))


def torch_bake(v, f, colors, views, S: int):
    """the contract's steps as whole-atlas float32 operations (blend mode, masks and colours given, every index in range)"""
    dev, f32 = v.device, torch.float32
    T = int(f.shape[0])
    B = eng.texture_atlas_block(T, S)
    c = float(B - 3)
    gj, gi = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
    i, j = gi % B, gj % B
    upper = (i + j) > B - 1
    t = 2 * ((gj // B) * (S // B) + gi // B) + upper.long()
    present = t < T
    a = torch.where(upper, B - 1 - i, i).to(f32) / c
    b = torch.where(upper, B - 1 - j, j).to(f32) / c
    s = a + b
    a, b = torch.where(s > 1, a / s, a), torch.where(s > 1, b / s, b)
    idx = f[torch.where(present, t, torch.zeros_like(t))].long()
    v0, v1, v2 = v[idx[..., 0]], v[idx[..., 1]], v[idx[..., 2]]
    e1, e2 = v1 - v0, v2 - v0
    p = [(v0[..., k] + a * e1[..., k]) + b * e2[..., k] for k in range(3)]
    nrm = [(e1[..., (k + 1) % 3] * e2[..., (k + 2) % 3]) - (e1[..., (k + 2) % 3] * e2[..., (k + 1) % 3]) for k in range(3)]
    nn = (nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]
    acc = [torch.zeros(S, S, device=dev) for _ in range(3)]
    wsum = torch.zeros(S, S, device=dev)
    seen = torch.zeros(S, S, dtype=torch.int32, device=dev)
    Kh, Th = views["K"].cpu().numpy(), views["TCO"].cpu().numpy()
    cm2 = float(np.float32(COS_MIN) * np.float32(COS_MIN))
    for q in range(len(Kh)):
        R, fx, cx, fy, cy = Th[q], float(Kh[q, 0, 0]), float(Kh[q, 0, 2]), float(Kh[q, 1, 1]), float(Kh[q, 1, 2])
        cam = [((float(R[r, 0]) * p[0] + float(R[r, 1]) * p[1]) + float(R[r, 2]) * p[2]) + float(R[r, 3]) for r in range(3)]
        xf, yf = (fx * cam[0]) / cam[2] + cx, (fy * cam[1]) / cam[2] + cy
        xn, yn = torch.floor(xf), torch.floor(yf)
        ok = present & (cam[2] > Z_MIN) & (xn >= 0) & (xn < W) & (yn >= 0) & (yn < H)
        rn = [(float(R[r, 0]) * nrm[0] + float(R[r, 1]) * nrm[1]) + float(R[r, 2]) * nrm[2] for r in range(3)]
        g = -((rn[0] * cam[0] + rn[1] * cam[1]) + rn[2] * cam[2])
        den = nn * ((cam[0] * cam[0] + cam[1] * cam[1]) + cam[2] * cam[2])
        gg = g * g
        ok = ok & (g > 0) & (gg > cm2 * den)
        wgt = gg / den
        depth, mask, rgb = views["depth"][q].reshape(-1), views["masks"][q].reshape(-1), views["rgb"][q].reshape(-1, 3)

        def tap(x, y):
            inside = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            at = torch.where(inside, y * W + x, torch.zeros_like(x))
            d = depth[at]
            return inside & (mask[at] != 0) & torch.isfinite(d) & (d > 0) & ((d - cam[2]).abs() <= DEPTH_TOL), rgb[at].to(f32)

        tx, ty = xf - 0.5, yf - 0.5
        fxx, fyy = torch.floor(tx), torch.floor(ty)
        ax, ay = tx - fxx, ty - fyy
        x0, y0 = torch.where(ok, fxx, torch.zeros_like(fxx)).long(), torch.where(ok, fyy, torch.zeros_like(fyy)).long()
        (k00, c00), (k01, c01), (k10, c10), (k11, c11) = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
        all4 = k00 & k01 & k10 & k11
        kn, cn = tap(torch.where(ok, xn, torch.zeros_like(xn)).long(), torch.where(ok, yn, torch.zeros_like(yn)).long())
        hit = all4 | kn
        for k in range(3):
            top = c00[..., k] + ax * (c01[..., k] - c00[..., k])
            bot = c10[..., k] + ax * (c11[..., k] - c10[..., k])
            acc[k] = torch.where(hit, acc[k] + wgt * torch.where(all4, top + ay * (bot - top), cn[..., k]), acc[k])
        wsum = torch.where(hit, wsum + wgt, wsum)
        seen += hit.to(torch.int32)
    w0 = (1.0 - a) - b
    out = torch.zeros(S, S, 4, dtype=torch.uint8, device=dev)
    for k in range(3):
        fallback = (((w0 * colors[idx[..., 0], k]) + a * colors[idx[..., 1], k]) + b * colors[idx[..., 2], k]) * 255.0
        val = torch.where(seen > 0, acc[k] / wsum, fallback)
        out[..., k] = torch.where(present, torch.floor(torch.clamp(val, 0.0, 255.0) + 0.5), torch.zeros_like(val)).to(torch.uint8)
    out[..., 3] = torch.where(present, 255, 0).to(torch.uint8)
    return out, torch.clamp(seen, max=255).to(torch.uint8)


def wall_once(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--subdivisions", type=int, nargs="+", default=[4, 5])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    args = ap.parse_args()
    host = make_views(args.views)
    views = {k: torch.from_numpy(a).cuda() for k, a in host.items()}
    n_cu, _, arch = eng.device_info()
    print(f"# {arch}, {n_cu} CUs; {args.views} views of {H} x {W} of a sphere of radius {st.SPHERE_R} m, masks and colours; {args.reps} reps in turn, "
          "wall clock around a synchronise")
    ok, first = True, True
    for sub in args.subdivisions:
        hv, hf, hc = tb.ico_mesh(sub)
        v, f, c = torch.from_numpy(hv).cuda(), torch.from_numpy(hf).cuda(), torch.from_numpy(hc).cuda()
        for S in args.sizes:
            B = eng.texture_atlas_block(len(hf), S)
            if B == 0:
                continue

            def bake():
                return eng.texture_bake(v, f, views["depth"], views["K"], views["TCO"], views["masks"], views["rgb"], S, colors=c, depth_tol=DEPTH_TOL,
                                        cos_min=COS_MIN, z_min=Z_MIN)

            texels, seen = bake()
            t_texels, t_seen = torch_bake(v, f, c, views, S)
            agree_seen = bool(torch.equal(seen, t_seen))
            texel_diff = int((texels.to(torch.int32) - t_texels.to(torch.int32)).abs().max())
            agree_emulation = None
            if first:                                                  # the host emulation, byte for byte (one core: seconds)
                e_texels, e_seen = tb.emul_bake(hv, hf, host, S, colors=hc, depth_tol=DEPTH_TOL, cos_min=COS_MIN, z_min=Z_MIN)
                agree_emulation = bool(np.array_equal(texels.cpu().numpy(), e_texels) and np.array_equal(seen.cpu().numpy(), e_seen) and
                                       np.array_equal(eng.texture_atlas_uvs(len(hf), S).cpu().numpy(), tb.emul_uvs(len(hf), S)))
                ok, first = ok and agree_emulation, False
            chart = int((texels[..., 3] != 0).sum())
            covered = int(((seen != 0) & (texels[..., 3] != 0)).sum())
            frames = (views["depth"], views["masks"], views["rgb"])
            runs = {"bake": bake, "torch_bake": lambda: torch_bake(v, f, c, views, S), "uvs": lambda: eng.texture_atlas_uvs(len(hf), S),
                    "clone_outputs": lambda: (texels.clone(), seen.clone()), "clone_frames": lambda: [t.clone() for t in frames]}
            for fn in runs.values():
                fn()
            times = {k: [] for k in runs}
            for _ in range(args.reps):
                for k, fn in runs.items():
                    times[k].append(wall_once(fn))
            best = {k: min(t) for k, t in times.items()}
            median = {k: statistics.median(t) for k, t in times.items()}
            floor = best["clone_outputs"] + best["clone_frames"]
            print(json.dumps(dict(name="texture_bake", faces=len(hf), size=S, block=B, views=args.views, H=H, W=W, reps=args.reps, chart_texels=chart,
                                  covered_share=covered / max(chart, 1), output_bytes=5 * S * S, frame_bytes=int(sum(t.numel() * t.element_size() for t in frames)),
                                  **{f"{k}_ms": best[k] for k in runs}, **{f"{k}_median_ms": median[k] for k in runs},
                                  visits_per_s=chart * args.views / (best["bake"] * 1e-3), torch_over_bake=best["torch_bake"] / best["bake"],
                                  bake_over_clone=best["bake"] / floor, agree_seen=agree_seen, max_texel_difference_to_torch=texel_diff,
                                  agree_emulation=agree_emulation)))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
