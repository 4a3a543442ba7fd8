#!/usr/bin/env python3
"""Write tests/golden/pose_errors.npz: symmetry sets and point distances computed by the REFERENCE's own functions
(lib3d/symmetries.py make_symmetries_poses, lib3d/distances.py dists_add / dists_add_symmetries / dists_add_symmetric), imported through
oracle.ref_import.  Needs the reference checkout, so it runs where that exists; the tests read the fixture only.

`transforms3d` is not installed and oracle.ref_import serves a stub for it, so the one function the reference calls in it
(`transforms3d.euler.euler2quat`, axes "sxyz") is supplied here for a rotation about ONE coordinate axis: (w, x, y, z) =
(cos(a/2), sin(a/2) axis) -- said in the fixture's `notes` field.  Every call gets FRESH symmetry objects: the reference scales the
discrete poses in place, so only its first call on an object is its answer.

Usage: python scripts/make_pose_error_golden.py
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from oracle import ref_import  # noqa: E402
from support import pose_error as pes  # noqa: E402

OUT = ROOT / "tests" / "golden" / "pose_errors.npz"


def _one_axis_euler2quat(ai, aj, ak, axes="sxyz"):
    assert axes == "sxyz"
    e = np.array([ai, aj, ak], np.float64)
    nz = np.flatnonzero(e)
    assert len(nz) <= 1, "one-axis rotations only"
    q = np.zeros(4)
    q[0] = 1.0
    if len(nz):
        q[0] = np.cos(e[nz[0]] / 2.0)
        q[1 + nz[0]] = np.sin(e[nz[0]] / 2.0)
    return q


def symmetry_cases():
    half_z = pes.pose(pes.axis_rotation(2, np.pi), [10.0, 20.0, 30.0])
    half_x = pes.pose(pes.axis_rotation(0, np.pi), [0.0, 0.0, 5.0])
    quarter_y = pes.pose(pes.axis_rotation(1, np.pi / 2), [1.0, -2.0, 0.5])
    ax = {"x": [1, 0, 0], "y": [0, 1, 0], "z": [0, 0, 1]}
    c = {}
    c["none"] = dict(discrete=[], continuous=[], n=8, units="mm", scale=None)
    c["discrete_mm"] = dict(discrete=[half_z], continuous=[], n=8, units="mm", scale=None)
    c["discrete_m"] = dict(discrete=[half_z], continuous=[], n=8, units="m", scale=None)
    c["discrete_scale"] = dict(discrete=[half_z, quarter_y], continuous=[], n=8, units="mm", scale=0.5)
    c["continuous_x_1"] = dict(discrete=[], continuous=[ax["x"]], n=1, units="mm", scale=None)
    c["continuous_y_8"] = dict(discrete=[], continuous=[ax["y"]], n=8, units="mm", scale=None)
    c["continuous_z_64"] = dict(discrete=[], continuous=[ax["z"]], n=64, units="mm", scale=None)
    c["continuous_x_8"] = dict(discrete=[], continuous=[ax["x"]], n=8, units="m", scale=None)
    c["both_z_4"] = dict(discrete=[half_x, quarter_y], continuous=[ax["z"]], n=4, units="mm", scale=None)
    c["both_scale"] = dict(discrete=[half_x], continuous=[ax["y"]], n=3, units="mm", scale=0.002)
    return c


def main() -> int:
    ref_import.install()
    import transforms3d

    transforms3d.euler.euler2quat = _one_axis_euler2quat
    import megapose.lib3d.distances as rd
    import megapose.lib3d.symmetries as rs

    out = {}
    cases = symmetry_cases()
    meta = {}
    for name, c in cases.items():
        disc = [rs.DiscreteSymmetry(pose=np.array(M, np.float64)) for M in c["discrete"]]
        cont = [rs.ContinuousSymmetry(offset=np.zeros(3), axis=np.array(a)) for a in c["continuous"]]
        res = rs.make_symmetries_poses(disc, cont, n_symmetries_continuous=c["n"], units=c["units"], scale=c["scale"])
        out[f"sym_{name}"] = np.asarray(res, np.float64)
        out[f"sym_{name}_discrete"] = np.asarray(c["discrete"], np.float64).reshape(-1, 4, 4)
        out[f"sym_{name}_continuous"] = np.asarray(c["continuous"], np.float64).reshape(-1, 3)
        meta[name] = dict(n=c["n"], units=c["units"], scale=c["scale"])

    # distances: b = 6 rows, N = 300 points per row, S = 5 candidate ground truths (fp32, as the reference runs them)
    rng = np.random.RandomState(7)
    b, N, S = 6, 300, 5
    points = (rng.uniform(-1, 1, size=(b, N, 3)) * np.array([0.05, 0.08, 0.12])).astype(np.float32)
    T_gt = pes.random_poses(rng, b)
    T_pred = pes.perturbed(rng, T_gt, angle_deg=6.0, shift=0.01)
    cand = np.stack([np.stack([(np.asarray(T_gt[i], np.float64) @ pes.pose(pes.axis_rotation(2, 2 * np.pi * s / S), [0, 0, 0])) for s in range(S)])
                     for i in range(b)]).astype(np.float32)
    # the prediction of row i sits near candidate i % S, so the arg-min is not always 0
    T_pred = np.stack([pes.perturbed(rng, cand[i, i % S][None], angle_deg=5.0, shift=0.005)[0] for i in range(b)])
    tp, tg, tc, pp = (torch.from_numpy(a) for a in (T_pred, T_gt, cand, points))
    out.update(dist_points=points, dist_T_pred=T_pred, dist_T_gt=T_gt, dist_T_gt_possible=cand,
               dists_add=rd.dists_add(tp, tg, pp).numpy(), dists_add_symmetries=rd.dists_add_symmetries(tp, tc, pp).numpy(),
               dists_add_symmetric=rd.dists_add_symmetric(tp, tg, pp).numpy())
    out["meta"] = np.array(json.dumps(meta))
    out["notes"] = np.array("symmetry sets: the reference's lib3d/symmetries.py make_symmetries_poses, first call on fresh objects, with "
                            "transforms3d.euler.euler2quat (stubbed: not installed) supplied for one-axis rotations as (cos(a/2), sin(a/2) axis); "
                            "distances: the reference's lib3d/distances.py on float32 CPU tensors")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
