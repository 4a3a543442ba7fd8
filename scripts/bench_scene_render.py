#!/usr/bin/env python
"""Scene rendering on the device: Panda3dSceneRenderer.render_scenes (one mp_raster_render_scene launch) against the route the project
used before it existed -- Panda3dBatchRenderer.render of every (frame, object) view + the per-pixel nearest composite of
tests/support/scene.py.  Workload: 8 frames of 640 x 480, 8 objects each from the synthetic meshes, 4x MSAA, depth and normals on.
Both are timed with device events after warm-up, in the same process; prints one JSON line.

    python scripts/bench_scene_render.py [--frames 8 --objects 8 --iters 20 --warmup 5]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def composite(rgb, nrm, dep, n_frames, n_obj):
    """tests/support/scene.py's composite: per frame, painter's order by the depth buffer over the frame's per-object renders"""
    h, w = dep.shape[-2:]
    out_rgb = torch.zeros(n_frames, 3, h, w, device=dep.device)
    out_nrm = torch.zeros(n_frames, 3, h, w, device=dep.device)
    zbuf = torch.zeros(n_frames, h, w, device=dep.device)
    for f in range(n_frames):
        for i in range(n_obj):
            k = f * n_obj + i
            d = dep[k, 0]
            closer = (d > 0) & ((zbuf[f] == 0) | (d < zbuf[f]))
            out_rgb[f] = torch.where(closer[None], rgb[k], out_rgb[f])
            out_nrm[f] = torch.where(closer[None], nrm[k], out_nrm[f])
            zbuf[f] = torch.where(closer, d, zbuf[f])
    return out_rgb, out_nrm, zbuf


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from megapose6d_amd import Panda3dBatchRenderer, Panda3dSceneRenderer
    from megapose6d_amd.types import make_scene_lights
    from tests.support import synthetic as syn

    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    ds = syn.make_object_dataset(Path(tempfile.mkdtemp(prefix="mp_scene_bench_")), n_objects=16, seed=40, n_theta=48, n_z=50)
    names = [o.label for o in ds.list_objects]
    rng = np.random.RandomState(9)
    labels, poses, sid = [], [], []
    for f in range(a.frames):
        for j in range(a.objects):
            labels.append(names[(2 * f + j) % len(names)])
            poses.append(syn.random_pose(rng, (0.5, 0.8), 0.3))
            sid.append(f)
    n = len(labels)
    T = torch.from_numpy(np.stack(poses).astype(np.float32)).to(dev)
    K = torch.from_numpy(np.repeat(syn.K_EXAMPLE[None].astype(np.float32), n, 0)).to(dev)
    sid_t = torch.tensor(sid)
    lights = make_scene_lights()
    res = (480, 640)
    scene = Panda3dSceneRenderer(ds, msaa=4)
    batch = Panda3dBatchRenderer(ds, n_workers=1, msaa=4)

    def run_scene():
        return scene.render_scenes(labels, T, K, sid_t, res, lights, render_depth=True, render_normals=True)

    def run_batch():
        b = batch.render(labels, T, K, [lights] * n, res, render_depth=True, render_normals=True)
        return composite(b.rgbs, b.normals, b.depths, a.frames, a.objects)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    ms_scene = timed(run_scene)
    ms_batch = timed(run_batch)
    s = run_scene()
    covered = float((s.depths > 0).float().mean())
    print(json.dumps({"bench": "scene_render", "frames": a.frames, "objects_per_frame": a.objects, "h": res[0], "w": res[1], "msaa": 4,
                      "depth": True, "normals": True, "iters": a.iters, "render_scenes_ms": round(ms_scene, 4),
                      "batch_views_plus_composite_ms": round(ms_batch, 4), "speedup": round(ms_batch / ms_scene, 3), "covered_fraction": round(covered, 4),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
