"""Object symmetry sets (the reference's src/megapose/lib3d/symmetries.py:32-88), float64 on the host.

`make_symmetries_poses` keeps the reference's ordering: the identity first among the discrete symmetries, and for an object with
continuous symmetries the product `sym_c * sym_d` with the continuous index running inside each discrete one.  Two differences:
  * the reference scales `sym_d.pose[:3, -1]` IN PLACE (symmetries.py:72), so a second call on the same objects returns other poses;
    this returns what the reference's FIRST call returns, every time, and leaves its input alone;
  * the Euler -> quaternion step (`transforms3d.euler.euler2quat`, axes "sxyz") is written out for a rotation about ONE coordinate
    axis, q = (sin(a/2) axis, cos(a/2)) -- all that the reference's `axis.sum() == 1` assert admits in practice; any other axis raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np


@dataclass
class ContinuousSymmetry:
    """offset: (3,), axis: (3,) -- see bop_toolkit_lib/misc.py"""

    offset: np.ndarray
    axis: np.ndarray


@dataclass
class DiscreteSymmetry:
    """pose: (4, 4) homogeneous matrix"""

    pose: np.ndarray


def _quat_xyzw_to_matrix(q: np.ndarray) -> np.ndarray:
    """Unit quaternion -> rotation matrix, Eigen's formula (what pinocchio's Quaternion.matrix() evaluates)."""
    q = np.asarray(q, np.float64)
    q = q / np.sqrt((q * q).sum())
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def _one_axis_euler2quat(euler: np.ndarray) -> np.ndarray:
    """sxyz Euler angles with ONE non-zero axis -> xyzw quaternion."""
    euler = np.asarray(euler, np.float64)
    nz = np.flatnonzero(euler)
    if len(nz) > 1:
        raise NotImplementedError("continuous symmetries are supported about one coordinate axis (x, y or z) only")
    q = np.zeros(4)
    if len(nz) == 0:
        q[3] = 1.0
        return q
    half = euler[nz[0]] / 2.0
    q[nz[0]] = np.sin(half)
    q[3] = np.cos(half)
    return q


def make_symmetries_poses(symmetries_discrete: Sequence[DiscreteSymmetry] = (), symmetries_continuous: Sequence[ContinuousSymmetry] = (),
                          n_symmetries_continuous: int = 8, units: str = "mm", scale: Optional[float] = None) -> np.ndarray:
    """-> (num_symmetries, 4, 4) float64"""
    if scale is None:
        scale = {"m": 1, "mm": 0.001}[units]
    all_discrete: List[np.ndarray] = [np.eye(4)]
    for sym_d in symmetries_discrete:
        M = np.array(sym_d.pose, dtype=np.float64)   # a copy: the caller's pose is not scaled in place
        assert M.shape == (4, 4)
        out = np.eye(4)
        out[:3, :3] = M[:3, :3]
        out[:3, 3] = M[:3, 3] * scale
        all_discrete.append(out)
    all_continuous: List[np.ndarray] = []
    for sym_c in symmetries_continuous:
        assert np.allclose(sym_c.offset, 0)
        axis = np.array(sym_c.axis)
        assert axis.sum() == 1
        if sorted(np.abs(axis).tolist()) != [0, 0, 1]:
            raise NotImplementedError("continuous symmetries are supported about one coordinate axis (x, y or z) only")
        for n in range(n_symmetries_continuous):
            euler = axis * 2 * np.pi * n / n_symmetries_continuous
            M = np.eye(4)
            M[:3, :3] = _quat_xyzw_to_matrix(_one_axis_euler2quat(euler))
            all_continuous.append(M)
    all_M = []
    for sym_d in all_discrete:
        if len(all_continuous) > 0:
            for sym_c in all_continuous:
                M = np.eye(4)
                M[:3, :3] = sym_c[:3, :3] @ sym_d[:3, :3]
                M[:3, 3] = sym_c[:3, :3] @ sym_d[:3, 3] + sym_c[:3, 3]
                all_M.append(M)
        else:
            all_M.append(sym_d.copy())
    return np.array(all_M)
