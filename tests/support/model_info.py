"""TEST SUPPORT: ctypes wrapper of the host emulation of the model-info kernels (tests/model_info_emul.cpp), built on first use; the
float64 brute force the emulation and the kernel are held against; and the seeded point sets the CPU contract test and the GPU test
share.  Every set is fp32, generated here, with coordinates of at most a few metres."""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from typing import Dict, Optional, Tuple

import numpy as np

from .emul import CSRC, TESTS, _p, build

TILES = (0, 64, 128, 256)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)
REL_BOUND = 1e-6   # each fp32 difference is exact to 2^-24 relative, the three-term sum adds at most 3 ulp: a pair whose fp32 d2 wins can
#                    be short of the true maximum by about 4 * 2^-24 = 2.4e-7 relative; 1e-6 is that with a factor 4 of margin
CYL_R, CYL_H = 0.05, 0.2


def load():
    lib = build("model_info_emul", [TESTS / "model_info_emul.cpp", CSRC / "model_info_core.h"])
    lib.model_info_emul.restype = C.c_int
    lib.model_info_emul_prefix.restype = C.c_longlong
    lib.model_info_emul_decode.restype = None
    lib.model_info_emul_limits.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_int * 5)()
    load().model_info_emul_limits(v)
    return dict(block=int(v[0]), tile_step=int(v[1]), max_tile=int(v[2]), default_tile=int(v[3]), default_chunk=int(v[4]))


def prefix(n_points, tile: int) -> Optional[np.ndarray]:
    """the prefix array of job counts [n_obj + 1] int32, None for arguments the launch rejects"""
    n = np.ascontiguousarray(n_points, np.int32)
    off = np.full(len(n) + 1, -1, np.int32)
    total = load().model_info_emul_prefix(C.c_int(len(n)), _p(n), C.c_int(tile), _p(off))
    if total < 0:
        return None
    assert off[-1] == total
    return off


def decode(local: int, tile: int, n: int) -> Tuple[int, int, int, int]:
    """job `local` of an object of n points -> (i-block, j-chunk, first j, end j)"""
    out = np.empty(4, np.int32)
    load().model_info_emul_decode(C.c_longlong(local), C.c_int(tile), C.c_int(n), _p(out))
    return tuple(int(v) for v in out)


def emul(points: np.ndarray, n_points, tile: int = 0, job_order=None):
    """the emulation on the arguments of the C ABI: points [n_obj,stride,3] fp32 -> d2 [n_obj] fp32, pair [n_obj,2] int32, bounds
    [n_obj,6] fp32; job_order a permutation of the launch's jobs (default: ascending)"""
    points = np.ascontiguousarray(points, np.float32)
    assert points.ndim == 3 and points.shape[2] == 3
    n = np.ascontiguousarray(n_points, np.int32)
    n_obj = points.shape[0]
    order = None if job_order is None else np.ascontiguousarray(job_order, np.int64)
    d2, pair, bounds = np.empty(n_obj, np.float32), np.empty((n_obj, 2), np.int32), np.empty((n_obj, 6), np.float32)
    rc = load().model_info_emul(_p(points), C.c_int(points.shape[1]), _p(n), C.c_int(n_obj), C.c_int(tile), _p(order), _p(d2), _p(pair), _p(bounds))
    assert rc == 0
    return d2, pair, bounds


def brute_force(points: np.ndarray) -> float:
    """the largest distance between two of the points [n,3], in float64 (numpy; scipy's pdist gives the same on these sizes)"""
    p = np.asarray(points, np.float32).astype(np.float64)
    best = 0.0
    for r0 in range(0, len(p), 256):
        d = p[r0:r0 + 256, None, :] - p[None, :, :]
        best = max(best, float((d * d).sum(-1).max()))
    return float(np.sqrt(best))


def pair_distance(points: np.ndarray, pair) -> float:
    p = np.asarray(points, np.float32).astype(np.float64)
    return float(np.linalg.norm(p[int(pair[0])] - p[int(pair[1])]))


def numpy_bounds(points: np.ndarray) -> np.ndarray:
    """min x y z, then max - min in fp32: what the kernel must give bit for bit"""
    p = np.asarray(points, np.float32)
    lo, hi = p.min(0), p.max(0)
    return np.concatenate([lo, (hi - lo).astype(np.float32)]).astype(np.float32)


# the point sets ---------------------------------------------------------------------------------------------------------------------
def cylinder_points() -> np.ndarray:
    """300 points of a thin cylinder shell of radius CYL_R and height CYL_H: 100 on each rim and 100 half-way, at 100 even angles (so
    every point has its antipode: the diameter is sqrt(4 r^2 + h^2), the box diagonal sqrt(8 r^2 + h^2))"""
    a = np.arange(100) * (2.0 * np.pi / 100.0)
    ring = np.stack([CYL_R * np.cos(a), CYL_R * np.sin(a)], 1)
    return np.concatenate([np.concatenate([ring, np.full((100, 1), z)], 1) for z in (-CYL_H / 2, CYL_H / 2, 0.0)]).astype(np.float32)


def _ball(rng, n: int, radius: float) -> np.ndarray:
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * radius * rng.uniform(0.2, 1.0, size=(n, 1))).astype(np.float32)


def _with_extremes(seed: int, n: int, i: int, j: int) -> np.ndarray:
    rng = np.random.RandomState(seed)
    p = _ball(rng, n, 0.5)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    p[i], p[j] = (3.0 * axis).astype(np.float32), (-3.0 * axis).astype(np.float32)
    return p


@lru_cache(maxsize=None)
def cases() -> Dict[str, Dict[str, object]]:
    """name -> dict(points [n,3] fp32, pair = the pair the tie-break or the construction names, or None)"""
    out: Dict[str, Dict[str, object]] = {}
    for n in SIZES:
        out[f"random_{n}"] = dict(points=np.random.RandomState(n).uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32), pair=None)
    out["random_1"]["pair"] = (0, 0)
    out["random_2"]["pair"] = (0, 1)
    cube = np.asarray([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], np.float32)
    out["cube"] = dict(points=cube, pair=(0, 7))          # four equal diagonals (0,7) (1,6) (2,5) (3,4): the lowest i
    rng = np.random.RandomState(77)
    dup = _ball(rng, 300, 0.5)
    a, b = np.asarray([-2.0, 0.25, 0.0], np.float32), np.asarray([2.0, -0.5, 0.125], np.float32)
    dup[[10, 200, 290]] = a
    dup[[5, 150]] = b
    out["duplicates"] = dict(points=dup, pair=(5, 10))    # (5,10) (5,200) (5,290) (10,150) (150,200) (150,290) are equal: lowest i, then j
    out["cylinder"] = dict(points=cylinder_points(), pair=None)
    out["extremes_one_block"] = dict(points=_with_extremes(1, 1025, 300, 400), pair=(300, 400))
    out["extremes_first_last"] = dict(points=_with_extremes(2, 1025, 3, 1024), pair=(3, 1024))
    out["extremes_last_partial"] = dict(points=_with_extremes(3, 1100, 1030, 1090), pair=(1030, 1090))
    for c in out.values():
        c["points"].setflags(write=False)
    return out


@lru_cache(maxsize=None)
def three_objects(with_nan: bool = False):
    """three objects of 300, 1025 and 65 points in one tensor [3,1100,3]; the rows beyond n_points hold points 100 m away, which must
    never be read as points; with_nan: a NaN coordinate in the middle object -> points, n_points"""
    cs = cases()
    sets = [cs["duplicates"]["points"], cs["extremes_first_last"]["points"], cs["random_65"]["points"]]
    rng = np.random.RandomState(5)
    points = (100.0 + rng.uniform(-1.0, 1.0, size=(3, 1100, 3))).astype(np.float32)
    for o, p in enumerate(sets):
        points[o, :len(p)] = p
    if with_nan:
        points[1, 700, 1] = np.nan
    points.setflags(write=False)
    return points, np.asarray([len(p) for p in sets], np.int32)


@lru_cache(maxsize=None)
def emul_case(name: str, tile: int):
    """the emulation's result on one case, computed once: (d2 fp32 scalar, pair (i, j), bounds [6])"""
    p = cases()[name]["points"]
    d2, pair, bounds = emul(p[None], [len(p)], tile)
    return d2[0], (int(pair[0, 0]), int(pair[0, 1])), bounds[0]
