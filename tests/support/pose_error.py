"""TEST SUPPORT: ctypes wrapper of the host emulation of the pose-error kernels (tests/pose_error_emul.cpp; support/emul.py builds it), the
float64 restatement the emulation is held to, and the derived distance bound."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np

from .emul import CSRC, TESTS, _f32, _i32, _p, build

ULP = 2.0 ** -24


def load():
    lib = build("pose_error_emul", [TESTS / "pose_error_emul.cpp", CSRC / "pose_error_core.h"])
    for n in ("pose_error_emul_sym", "mspd_emul", "pose_error_emul_nn", "pose_error_emul_rigid"):
        getattr(lib, n).restype = None
    return lib


def _points(points, mesh_ids, b):
    points = _f32(points)
    assert points.ndim == 3 and points.shape[2] == 3
    if mesh_ids is None:
        assert points.shape[0] == b
        mesh_ids = np.arange(b)
    return points, _i32(mesh_ids)


def sym(T_pred, T_gt, symmetries, n_sym, points, mesh_ids=None, n_points=None, reduce_max=False, with_diffs=True, K=None) -> Dict[str, np.ndarray]:
    """Same addressing as megapose6d_amd.engine.pose_error_sym (symmetries None: T_gt = candidates [b,S,4,4]); with K [b,3,3] as
    engine.pose_error_mspd: the distances are taken between projections, and there are no difference vectors."""
    T_pred, T_gt, symmetries = _f32(T_pred), _f32(T_gt), _f32(symmetries)
    b = T_pred.shape[0]
    points, mesh_ids = _points(points, mesh_ids, b)
    n_sym, n_points = _i32(n_sym), _i32(n_points)
    S = symmetries.shape[1] if symmetries is not None else T_gt.shape[1]
    n = points.shape[1]
    out = dict(err=np.empty(b, np.float32), err_alt=np.empty(b, np.float32), idx=np.empty(b, np.int32), T_gt_sym=np.empty((b, 4, 4), np.float32),
               errs=np.empty((b, S), np.float32))
    if K is not None:
        K = _f32(K)
        assert K.shape == (b, 3, 3)
        load().mspd_emul(_p(T_pred), _p(T_gt), _p(symmetries), _p(n_sym), C.c_int(S), _p(points), C.c_int(n), _p(mesh_ids), _p(n_points),
                                    C.c_int(n), C.c_int(b), C.c_int(int(reduce_max)), _p(K), _p(out["err"]), _p(out["err_alt"]), _p(out["idx"]),
                                    _p(out["T_gt_sym"]), _p(out["errs"]))
        return out
    if with_diffs:
        out["diffs"] = np.empty((b, n, 3), np.float32)
    load().pose_error_emul_sym(_p(T_pred), _p(T_gt), _p(symmetries), _p(n_sym), C.c_int(S), _p(points), C.c_int(n), _p(mesh_ids), _p(n_points),
                               C.c_int(n), C.c_int(b), C.c_int(int(reduce_max)), _p(out["err"]), _p(out["err_alt"]), _p(out["idx"]),
                               _p(out["T_gt_sym"]), _p(out["errs"]), _p(out.get("diffs")))
    return out


def nn(T_pred, T_gt, points, mesh_ids=None, n_points=None) -> Dict[str, np.ndarray]:
    T_pred, T_gt = _f32(T_pred), _f32(T_gt)
    b = T_pred.shape[0]
    points, mesh_ids = _points(points, mesh_ids, b)
    n_points = _i32(n_points)
    n = points.shape[1]
    out = dict(diffs=np.empty((b, n, 3), np.float32), assign=np.empty((b, n), np.int32), mean=np.empty(b, np.float32), max=np.empty(b, np.float32))
    load().pose_error_emul_nn(_p(T_pred), _p(T_gt), _p(points), C.c_int(n), _p(mesh_ids), _p(n_points), C.c_int(n), C.c_int(b), _p(out["diffs"]),
                              _p(out["assign"]), _p(out["mean"]), _p(out["max"]))
    return out


def rigid(T_a, T_b, K=None, points=None, mesh_ids=None, n_points=None) -> Dict[str, np.ndarray]:
    T_a, T_b, K = _f32(T_a), _f32(T_b), _f32(K)
    b = T_a.shape[0]
    out = dict(trans_err=np.empty(b, np.float32), rot_err_deg=np.empty(b, np.float32))
    n = 0
    if K is not None:
        points, mesh_ids = _points(points, mesh_ids, b)
        n_points = _i32(n_points)
        n = points.shape[1]
        out["proj_error"] = np.empty(b, np.float32)
    else:
        points = mesh_ids = n_points = None
    load().pose_error_emul_rigid(_p(T_a), _p(T_b), C.c_int(b), _p(K), _p(points), C.c_int(n), _p(mesh_ids), _p(n_points), C.c_int(n),
                                 _p(out["trans_err"]), _p(out["rot_err_deg"]), _p(out.get("proj_error")))
    return out


# --------------------------------------------------------------------------------------------------------------------------------
def beta(*poses, points, symmetries=None) -> float:
    """The derived distance bound: 64 * 2^-24 * sigma, sigma = the largest |translation| among the given poses (and symmetries) + 2 x the
    bounding radius of the points (about the origin of the object frame)."""
    t = max(float(np.abs(np.asarray(T, np.float64)[..., :3, 3]).max()) for T in poses if T is not None)
    if symmetries is not None:
        t = max(t, float(np.abs(np.asarray(symmetries, np.float64)[..., :3, 3]).max()))
    radius = float(np.linalg.norm(np.asarray(points, np.float64), axis=-1).max())
    return 64.0 * ULP * (t + 2.0 * radius)


def random_rotation(rng: np.random.RandomState) -> np.ndarray:
    q = rng.randn(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def axis_rotation(axis: int, angle: float) -> np.ndarray:
    c, s = np.cos(angle), np.sin(angle)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def pose(R: np.ndarray, t) -> np.ndarray:
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def random_poses(rng: np.random.RandomState, b: int, depth: float = 0.8) -> np.ndarray:
    """[b,4,4] float32 poses in front of a camera"""
    return np.stack([pose(random_rotation(rng), [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), depth + rng.uniform(-0.2, 0.2)]) for _ in range(b)]).astype(np.float32)


def perturbed(rng: np.random.RandomState, T: np.ndarray, angle_deg: float = 4.0, shift: float = 0.01) -> np.ndarray:
    out = []
    for Ti in np.asarray(T, np.float64):
        ax = rng.randn(3)
        ax /= np.linalg.norm(ax)
        a = np.deg2rad(angle_deg) * rng.uniform(0.3, 1.0)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        dR = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
        out.append(pose(dR @ Ti[:3, :3], Ti[:3, 3] + rng.randn(3) * shift))
    return np.stack(out).astype(np.float32)


# float64 restatement (the plain definition, no fused anything) on the same fp32 inputs -----------------------------------------------
def f64_transform(T: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """T [...,4,4], pts [N,3] -> [...,N,3]"""
    T = np.asarray(T, np.float64)
    pts = np.asarray(pts, np.float64)
    return np.einsum("...ij,nj->...ni", T[..., :3, :3], pts) + T[..., None, :3, 3]


def f64_rot_err_deg(Ta: np.ndarray, Tb: np.ndarray) -> float:
    dR = np.asarray(Tb, np.float64)[:3, :3] @ np.asarray(Ta, np.float64)[:3, :3].T
    v = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    return float(np.rad2deg(np.arctan2(np.linalg.norm(v) / 2.0, (np.trace(dR) - 1.0) / 2.0)))
