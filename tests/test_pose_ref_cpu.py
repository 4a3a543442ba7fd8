"""CPU tier of the pose / camera-geometry kernel tests (tests/test_gpu_pose_kernels.py is the GPU tier).

* The float64 reference tests/support/pose_ref.py against oracle/geometry.py (torch fp32, itself pinned to the reference project's outputs
  by tests/test_oracle_golden.py) on every case family: this validates the new reference.  The oracle's error against float64, in units
  of 2^-24 * S of the error model, is the fp32 FLOOR; the bounds k of the GPU tier (pose_cases.K_BOUND) must be exactly what the rule
  "4 x floor, rounded up to a power of two, at least 8" gives for the floors measured here.
* The conditions the case generators promise, asserted on the float64 reference (no row is ever masked out of a comparison).
* Golden-free sanity of the float64 reference itself.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from oracle import geometry as og
from tests.support import pose_cases as pc
from tests.support import pose_ref as pr

MODE_NAME = {0: "TCO", 1: "TCO+front_3views", 2: "TCO+front_1view", 3: "sphere_26views"}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def oracle_prepare(case: pc.PrepareCase, inp):
    """the seven outputs of pose_prepare composed from the oracle's functions (models/pose_rigid.py:524-552), torch fp32"""
    T, K, pts = _t(inp["TCO_in"]), _t(inp["K"]), _t(inp["points"])
    ids = _t(inp["mesh_ids"]).long()
    b, V = T.shape[0], case.V
    Tn = og.normalize_T(T)
    tcr = Tn[:, :3, 3].clone()
    TV = og.make_TCO_multiview(Tn, tcr, MODE_NAME[case.mode], V, remove_TCO_rendering=case.remove, views_inplane_rotations=case.inplane and V > 1)
    P = pts[ids, :case.n_main]
    br = og.boxes_from_uv(og.project_points_robust(P, K, Tn))
    bc = og.crop_boxes_robust(br, K, Tn, tcr, P, case.im_hw, case.lamb)
    Kc = og.get_K_crop_resize(K, bc, case.out_hw)
    Pv = pts[ids, :case.n_views].unsqueeze(1).repeat(1, V, 1, 1).flatten(0, 1)
    TVf, Kf = TV.flatten(0, 1), K.unsqueeze(1).repeat(1, V, 1, 1).flatten(0, 1)
    bcv = og.crop_boxes_robust(og.boxes_from_uv(og.project_points_robust(Pv, Kf, TVf)), Kf, TVf, TVf[:, :3, 3], Pv, case.im_hw, case.lamb)
    KV = og.get_K_crop_resize(Kf, bcv, case.out_hw).view(b, V, 3, 3)
    if not case.remove:
        KV[:, 0] = Kc
    return dict(TCO_n=Tn, tCR=tcr, TCV_O=TV, KV_crop=KV, boxes_rend=br, boxes_crop=bc, K_main=Kc)


@functools.lru_cache(maxsize=None)
def prepare_floor(i: int):
    """per output, the oracle's worst error on case i in units of 2^-24 * S"""
    case = pc.PREPARE_CASES[i]
    inp = case.inputs()
    ref = case.reference(inp)
    got = {n: v.numpy() for n, v in oracle_prepare(case, inp).items()}
    return {n: float(v.max()) for n, v in pr.prepare_units(got, ref, case.out_hw).items()}


def update_floor(b: int) -> float:
    inp = pc.update_inputs(b)
    K = inp["KV_crop"][:, 0]
    ref = pr.pose_update(inp["TCO"], K, inp["out9"], inp["tCR"])
    got = og.update_pose(_t(inp["TCO"]), _t(K), _t(inp["out9"]), _t(inp["tCR"])).numpy()
    return float(pr.units(got, ref, pr.update_scales(ref, inp["out9"], inp["tCR"])).max())


def init_floor(b: int, grid: int, n_pts: int = 2000) -> float:
    inp = pc.init_inputs(b, grid, n_pts)
    P, R = inp["points"][inp["mesh_ids"]], inp["R"][inp["rot_ids"]]
    ref = pr.init_poses_from_boxes(inp["boxes"], inp["K"], P, R)
    got = og.TCO_init_from_boxes_autodepth_with_R(_t(inp["boxes"]), _t(P), _t(inp["K"]), _t(R)).numpy()
    return float(pr.units(got, ref, pr.init_poses_scales(ref, inp["boxes"], inp["K"])).max())


def extents_floor(grid: int, n_pts: int) -> float:
    """fp32 side: the rotated points as lib3d/cosypose_ops.py:197 forms them (a batched fp32 matrix product), then min / max"""
    pts, R = pc.make_points(n_pts, n_pts), pc.so3_grid(grid)
    rp = (_t(R)[None, :, None] @ _t(pts)[:, None, :, :, None]).squeeze(-1)          # [mesh, rot, n, 3]
    got = (rp.max(dim=2).values - rp.min(dim=2).values)[..., :2].numpy()
    ref = pr.init_extents(pts, R)
    return float(pr.units(got, ref, pr.init_extents_scale(pts, R)[..., None] * np.ones(2)).max())


def normalize_floor(b: int) -> float:
    T = pc.normalize_T_inputs(b)
    ref = pr.normalize_T(T)
    return float(pr.units(og.normalize_T(_t(T)).numpy(), ref, pr._T_scale(ref)).max())


# --------------------------------------------------------------------------- #
# 1. the float64 reference agrees with the fp32 oracle to fp32 round-off
@pytest.mark.parametrize("i", range(len(pc.PREPARE_CASES)), ids=[c.name for c in pc.PREPARE_CASES])
def test_reference_vs_oracle_pose_prepare(i):
    """fp32 round-off here means: within the bound the GPU tier grants the kernel for this family.  (The bound follows from the floors
    of all cases of the family -- test_bounds_follow_from_the_oracle_floor -- so this asserts that no case is wildly off its family.)"""
    case = pc.PREPARE_CASES[i]
    floor = prepare_floor(i)
    print(case.name, {n: round(v, 2) for n, v in floor.items()})
    for n, v in floor.items():
        assert v <= pc.K_BOUND[case.family][n], (case.name, n, v)


def test_bounds_follow_from_the_oracle_floor():
    """pose_cases.K_BOUND is not tuned: every entry is k_from_floor(worst oracle error of the family), measured here."""
    fam = {}
    for i, case in enumerate(pc.PREPARE_CASES):
        for n, v in prepare_floor(i).items():
            fam.setdefault(case.family, {}).setdefault(n, 0.0)
            fam[case.family][n] = max(fam[case.family][n], v)
    fam["update"] = {"TCO_out": max(update_floor(b) for b in pc.BATCHES)}
    fam["init"] = {"TCO_init": max(init_floor(b, g) for b, g in zip(pc.BATCHES, (72, 576, 4608, 72, 576, 4608))),
                   "extents": max(extents_floor(g, n) for g, n in pc.EXTENT_CASES)}
    fam["normalize"] = {"T": max(normalize_floor(b) for b in pc.BATCHES)}
    print("\nfp32 floor (units of 2^-24 * S) -> k")
    derived = {}
    for f, d in fam.items():
        derived[f] = {n: pr.k_from_floor(v) for n, v in d.items()}
        print(f"  {f:12s} " + "  ".join(f"{n} {v:.2f}->{derived[f][n]}" for n, v in d.items()))
    assert derived == pc.K_BOUND


# --------------------------------------------------------------------------- #
# 2. the conditions the generators promise
@pytest.mark.parametrize("i", range(len(pc.PREPARE_CASES)), ids=[c.name for c in pc.PREPARE_CASES])
def test_generator_conditions_pose_prepare(i):
    case = pc.PREPARE_CASES[i]
    inp = case.inputs()
    ref = case.reference(inp)
    b = case.b
    for bx in (ref["boxes_crop"], ref["boxes_crop_views"]):
        assert (bx[..., 2] - bx[..., 0]).min() >= 4.0 and (bx[..., 3] - bx[..., 1]).min() >= 3.0     # height = width / aspect >= 4 * 3/4
    assert np.linalg.norm(ref["tCR"], axis=-1).min() >= 0.05
    assert ref["cross_norm_min"].min() >= 0.1
    T = inp["TCO_in"].astype(np.float64)
    assert pr.ortho6d_sin(T[:, :3, 0], T[:, :3, 1]).min() >= 0.1
    K = inp["K"]
    assert (K == pc.K_EXAMPLE.astype(np.float32)).all(axis=(1, 2)).sum() == 1
    if b > 4:
        assert len(np.unique(K[:, 0, 0])) >= b - 1 and (K[:, 0, 1] != 0).sum() >= b - 1 and (K[:, 1, 0] != 0).sum() >= b - 1
        assert (K[:, 0, 0] != K[:, 1, 1]).all()
    if b >= 2 * pc.N_MESH:
        assert set(inp["mesh_ids"].tolist()) == set(range(pc.N_MESH)) and (np.diff(inp["mesh_ids"]) < 0).any()
    pts = inp["points"]
    n_used = max(case.n_main, case.n_views)
    assert np.linalg.norm(pts[:, :n_used], axis=-1).max() <= pc.MESH_RADIUS * (1 + 1e-6)
    if case.stride > n_used:
        assert np.linalg.norm(pts[:, n_used:], axis=-1).min() > 2.9 * pc.MESH_RADIUS
    w = ref["boxes_crop"][:, 2] - ref["boxes_crop"][:, 0]
    fc, cc = ref["frac_clamped"], ref["centre_clamped"]
    if case.pose in ("mid", "mid_offaxis", "far", "offscreen"):
        assert fc.max() == 0 and not cc.any()
    if case.pose == "far":
        assert 8.0 <= w.min() and w.max() <= 30.0, (w.min(), w.max())
    if case.pose == "close":
        k = np.arange(b) % 3
        assert ((fc[k == 0] > 0) & (fc[k == 0] < 1)).all() and not cc[k == 0].any()      # some points behind z = 0.1
        assert cc[k == 1].all() and (fc[k == 1] < 1).all()                               # the centre behind it, points in front
        assert (fc[k == 2] == 1).all() and cc[k == 2].all()                              # everything behind
    if case.pose == "offscreen":
        c = (ref["boxes_crop"][:, :2] + ref["boxes_crop"][:, 2:]) / 2
        h_im, w_im = case.im_hw
        out = np.maximum(np.maximum(-c[:, 0], c[:, 0] - w_im) / w_im, np.maximum(-c[:, 1], c[:, 1] - h_im) / h_im)
        assert out.min() > 0.5, out.min()          # the centre is more than a frame from the image centre: > half a frame outside the border


def test_generator_conditions_extreme_points():
    """mesh 0 has its farthest point at index 0, mesh 1 at the last used index, and dropping either changes extents of every rotation
    grid by far more than round-off"""
    for grid, n in pc.EXTENT_CASES:
        if n < 3:
            continue
        pts, R = pc.make_points(n, n), pc.so3_grid(grid)
        r = np.linalg.norm(pts.astype(np.float64), axis=-1)
        assert r[0].argmax() == 0 and r[1].argmax() == n - 1
        full = pr.init_extents(pts, R)
        assert (np.abs(pr.init_extents(pts[:1, 1:], R) - full[:1]).max(axis=2) > 1e-4).mean() > 0.5
        assert (np.abs(pr.init_extents(pts[1:2, :-1], R) - full[1:2]).max(axis=2) > 1e-4).mean() > 0.5


def test_generator_conditions_update_and_init():
    for b in pc.BATCHES:
        u = pc.update_inputs(b, V=3)
        o = u["out9"].astype(np.float64)
        s = pr.ortho6d_sin(o[:, :3], o[:, 3:6])
        assert s.min() >= 0.1 and (s.min() < 0.6 or b < 16)
        n1, n2 = np.linalg.norm(o[:, :3], axis=1), np.linalg.norm(o[:, 3:6], axis=1)
        assert n1.min() >= 0.29 and n1.max() <= 3.01 and n2.min() >= 0.29 and n2.max() <= 3.01
        assert o[:, 8].min() >= 0.5 and o[:, 8].max() <= 2.0 and np.linalg.norm(u["tCR"], axis=1).min() >= 0.05
        assert (u["KV_crop"][:, 0, 0, 0] != u["KV_crop"][:, 1, 0, 0]).all()
        i = pc.init_inputs(b, 576)
        bx = i["boxes"]
        assert (bx[2::3, 0] == bx[2::3, 2]).all() and (bx[1::3, 0] < 0).all() and (bx[1::3, 3] > 480).all()
        assert (bx[:, 2] >= bx[:, 0]).all() and (bx[:, 3] > bx[:, 1]).all()
    for g in (72, 512, 576, 4608):
        R = pc.so3_grid(g).astype(np.float64)
        assert R.shape[0] >= g and R.shape[1:] == (3, 3) and np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6


# --------------------------------------------------------------------------- #
# 3. golden-free sanity of the float64 reference
SANITY = [c for c in pc.PREPARE_CASES if c.name.startswith(("views-", "pose-", "shape-"))]


@pytest.mark.parametrize("case", SANITY, ids=[c.name for c in SANITY])
def test_reference_sanity(case):
    inp = case.inputs()
    ref = case.reference(inp)
    TV, Tn = ref["TCV_O"], ref["TCO_n"]
    b, V = TV.shape[:2]
    for T in (Tn, TV):
        R = T[..., :3, :3]
        assert np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(R) - 1).max() < 1e-12
        assert (T[..., 3, :] == np.array([0, 0, 0, 1.0])).all()
    # every look-at view has the object origin (the reference point tCR) on its optical axis; |t| = distance camera - origin
    look = np.ones(V, bool)
    if V == 1:
        look[:] = False
    elif not case.remove:
        look[0] = False
    t = TV[:, look, :3, 3]
    if t.size:
        assert (np.abs(t[..., :2]).max(axis=-1) <= 1e-12 * np.abs(t[..., 2])).all() and (t[..., 2] > 0).all()
    if not case.remove or V == 1:
        assert (TV[:, 0] == Tn).all()
    if case.mode in (1, 2) and V > 1:
        # the first offset is zero: that camera stands where the real one does, at distance |tCR|
        first = 0 if case.remove else 1
        assert np.abs(TV[:, first, 2, 3] - np.linalg.norm(ref["tCR"], axis=1)).max() < 1e-12
    if case.inplane:
        g = TV.reshape(b, V // 4, 4, 4, 4)
        Rq = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
        for q in range(1, 4):
            assert (g[:, :, q, :3, :3] == np.linalg.matrix_power(Rq, q) @ g[:, :, 0, :3, :3]).all()       # exact quarter turns
            assert (g[:, :, q, :3, 3] == g[:, :, 0, :3, 3]).all()
    # K_crop maps the crop box centre to the output centre and scales by out / crop
    fw, fh = max(case.out_hw), min(case.out_hw)
    for Kc, bx, K in ((ref["K_main"], ref["boxes_crop"], inp["K"].astype(np.float64)),
                      (ref["KV_crop"], ref["boxes_crop_views"], inp["K"].astype(np.float64)[:, None])):
        cw, ch = bx[..., 2] - bx[..., 0], bx[..., 3] - bx[..., 1]
        cen = np.stack([(bx[..., 0] + bx[..., 2]) / 2, (bx[..., 1] + bx[..., 3]) / 2, np.ones_like(cw)], axis=-1)
        # a pixel of the original image as a ray of the original camera, re-projected by the crop camera (skew terms are kept as they
        # are by get_K_crop_resize, so compare along x with the ray's y on the principal row and vice versa)
        assert np.abs(Kc[..., 0, 0] / K[..., 0, 0] - fw / cw).max() < 1e-12 and np.abs(Kc[..., 1, 1] / K[..., 1, 1] - fh / ch).max() < 1e-12
        u = (fw / cw) * (cen[..., 0] - K[..., 0, 2]) + Kc[..., 0, 2]
        v = (fh / ch) * (cen[..., 1] - K[..., 1, 2]) + Kc[..., 1, 2]
        assert np.abs(u - (fw - 1) / 2).max() < 1e-9 and np.abs(v - (fh - 1) / 2).max() < 1e-9
        assert (Kc[..., 0, 1] == K[..., 0, 1]).all() and (Kc[..., 1, 0] == K[..., 1, 0]).all() and (Kc[..., 2, :] == K[..., 2, :]).all()
        assert np.abs(cw / ch - max(case.im_hw) / min(case.im_hw)).max() < 1e-9
    # the crop holds the rendered box scaled by lamb about the projected centre
    br, bc = ref["boxes_rend"], ref["boxes_crop"]
    c = (bc[:, :2] + bc[:, 2:]) / 2
    half = np.maximum(np.abs(br[:, :2] - c), np.abs(br[:, 2:] - c)) * case.lamb
    assert (half <= (bc[:, 2:] - bc[:, :2]) / 2 * (1 + 1e-12)).all()
    assert (np.abs(half - (bc[:, 2:] - bc[:, :2]) / 2).min(axis=1) < 1e-9 * np.abs(bc).max()).all()   # and is tight on one axis


def test_reference_sanity_update_and_init():
    u = pc.update_inputs(129)
    K = u["KV_crop"][:, 0]
    ref = pr.pose_update(u["TCO"], K, u["out9"], u["tCR"])
    R = ref[:, :3, :3]
    Rin = u["TCO"][:, :3, :3].astype(np.float64)
    dR = R @ np.linalg.inv(Rin)
    assert np.abs(dR @ dR.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(dR) - 1).max() < 1e-12
    # identity update: 6D = (e1, e2), no pixel offset, vz = 1 -> the pose is returned
    ident = np.tile(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float32), (129, 1))
    assert np.abs(pr.pose_update(u["TCO"], K, ident, u["tCR"]) - u["TCO"].astype(np.float64)).max() < 1e-15
    # the reference point moves by (vx, vy) pixels of the crop camera and its depth scales by vz
    o, c = u["out9"].astype(np.float64), u["tCR"].astype(np.float64)
    moved = pr.pose_update(np.tile(np.eye(4), (129, 1, 1)) + np.pad(c[:, :, None], ((0, 0), (0, 1), (3, 0))), K, u["out9"], u["tCR"])[:, :3, 3]
    assert np.abs(moved[:, 2] / c[:, 2] - o[:, 8]).max() < 1e-12
    assert np.abs(K[:, 0, 0] * (moved[:, 0] / moved[:, 2] - c[:, 0] / c[:, 2]) - o[:, 6]).max() < 1e-9
    # init: the box centre re-projects onto itself and the projected extents average to the box size
    i = pc.init_inputs(129, 576)
    T = pr.init_poses_from_boxes(i["boxes"], i["K"], i["points"][i["mesh_ids"]], i["R"][i["rot_ids"]])
    Kd, bx = i["K"].astype(np.float64), i["boxes"].astype(np.float64)
    assert np.abs(Kd[:, 0, 0] * T[:, 0, 3] / T[:, 2, 3] + Kd[:, 0, 2] - (bx[:, 0] + bx[:, 2]) / 2).max() < 1e-9
    assert (T[:, :3, :3] == i["R"][i["rot_ids"]].astype(np.float64)).all()
    ext = pr.init_extents(i["points"], i["R"])[i["mesh_ids"], i["rot_ids"]]
    z = (Kd[:, 1, 1] * ext[:, 1] / (bx[:, 3] - bx[:, 1] + 1) + Kd[:, 0, 0] * ext[:, 0] / (bx[:, 2] - bx[:, 0] + 1)) / 2
    assert np.abs(T[:, 2, 3] - z).max() < 1e-12 * z.max()
