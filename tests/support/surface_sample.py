"""TEST SUPPORT: ctypes wrapper of the host emulation of the surface-sampling kernels (tests/surface_sample_emul.cpp), built on first
use; a float64 numpy restatement of trimesh.sample.sample_surface on the same uniforms, which the emulation and the kernel are held
against (trimesh itself is not a dependency); the on-face check; and the seeded meshes the CPU contract test and the GPU test share.

Every mesh is fp32, generated here.  The random triangles of the soups are well shaped and as large as the object (edges of 0.5 .. 1
around centres within 0.25 of the origin), and the triangles of the soup whose areas span 2^-30 .. 1 are scaled about the origin, so
their coordinates shrink with them: barycentric coordinates are in units of the triangle, so the bound ON_FACE, which is reasoned
for coordinates of the size of the extent, is meaningful on them."""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .emul import CSRC, TESTS, _p, build

BLOCKS = (0, 64, 128, 256)
COUNTS = (1, 63, 64, 65, 4096)
SOUP_FACES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2049, 4097)
ON_FACE = 1e-6     # three fp32 roundings (the two edges' fmaf and the edge differences) on values bounded by the extent are a few times
#                    2^-24 = 6e-8 of it; 1e-6 is that with a factor 4 of margin (the reasoning of REL_BOUND in support/model_info.py)
FACE_CAP = 0.01    # share of a case's samples whose face may differ from the float64 restatement: each of the F boundaries of the
#                    cumulative sum moves by about 2^-22 of the total under fp32 weights, so the share is about F * 2^-22 (1e-3 at 4097
#                    faces); 1 % is a cap, not a measurement


def load():
    lib = build("surface_sample_emul", [TESTS / "surface_sample_emul.cpp", CSRC / "surface_sample_core.h"])
    lib.surface_sample_emul.restype = C.c_int
    lib.surface_sample_emul_prefix.restype = C.c_longlong
    lib.surface_sample_emul_limits.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_int * 5)()
    load().surface_sample_emul_limits(v)
    return dict(block_step=int(v[0]), max_block=int(v[1]), default_block=int(v[2]), max_blocks=int(v[3]), max_faces=int(v[4]))


def prefix(vert_off, face_off, count: int, block: int) -> Optional[np.ndarray]:
    """the prefix array of job counts [n_obj + 1] int32, None for arguments the launch refuses"""
    vo, fo = np.ascontiguousarray(vert_off, np.int32), np.ascontiguousarray(face_off, np.int32)
    assert len(vo) == len(fo) >= 1
    off = np.full(len(fo), -1, np.int32)
    total = load().surface_sample_emul_prefix(C.c_int(len(fo) - 1), _p(vo), _p(fo), C.c_int(count), C.c_int(block), _p(off))
    if total < 0:
        return None
    assert off[-1] == total
    return off


def emul(vertices, faces, vert_off, face_off, u, block: int = 0, job_order=None, with_weights: bool = False):
    """the emulation on the arguments of the C ABI -> points [n_obj,count,3] fp32, face [n_obj,count] int32 (and the fp32 weights and
    the quantised weights [F_total] with with_weights); job_order a permutation of the launch's jobs (default: ascending)"""
    v, f = np.ascontiguousarray(vertices, np.float32), np.ascontiguousarray(faces, np.int32)
    vo, fo = np.ascontiguousarray(vert_off, np.int32), np.ascontiguousarray(face_off, np.int32)
    u = np.ascontiguousarray(u, np.float32)
    n_obj, count = u.shape[0], u.shape[1]
    assert u.shape == (n_obj, count, 3) and len(vo) == len(fo) == n_obj + 1 and vo[-1] == len(v) and fo[-1] == len(f)
    order = None if job_order is None else np.ascontiguousarray(job_order, np.int64)
    points, face = np.empty((n_obj, count, 3), np.float32), np.empty((n_obj, count), np.int32)
    w, q = (np.empty(len(f), np.float32), np.empty(len(f), np.uint64)) if with_weights else (None, None)
    rc = load().surface_sample_emul(_p(v), _p(f), _p(vo), _p(fo), C.c_int(n_obj), _p(u), C.c_int(count), C.c_int(block), _p(order), _p(points),
                                    _p(face), _p(w), _p(q))
    assert rc == 0
    return (points, face, w, q) if with_weights else (points, face)


def pack(meshes: Sequence[Tuple[np.ndarray, np.ndarray]]):
    """[(vertices [V,3], faces [F,3])] -> vertices, faces, vert_off, face_off of one launch"""
    vo = np.concatenate([[0], np.cumsum([len(v) for v, _ in meshes])]).astype(np.int32)
    fo = np.concatenate([[0], np.cumsum([len(f) for _, f in meshes])]).astype(np.int32)
    return (np.concatenate([v for v, _ in meshes]).astype(np.float32), np.concatenate([f for _, f in meshes]).astype(np.int32), vo, fo)


def emul_one(mesh, u, block: int = 0, **kw):
    """one object: u [count,3] -> points [count,3], face [count] (and the weights)"""
    out = emul(*pack([mesh]), np.asarray(u, np.float32)[None], block, **kw)
    return (out[0][0], out[1][0]) + tuple(out[2:])


def uniforms(shape, seed: int, edges: bool = False) -> np.ndarray:
    """[*shape, 3] fp32 multiples of 2^-24 in [0, 1), what torch.rand gives; edges: the first rows of every object are replaced by the
    values the rules name (0, the largest, beyond both ends, NaN, sums of exactly and just above 1), as many as fit"""
    rng = np.random.RandomState(seed)
    u = (rng.randint(0, 1 << 24, size=tuple(shape) + (3,)).astype(np.float64) / float(1 << 24)).astype(np.float32)
    if edges:
        top = np.float32(1.0 - 2.0 ** -24)
        e = np.asarray([[0.0, 0.0, 0.0], [top, top, top], [-0.5, -1.0, 2.0], [1.0, 1.0, 0.0], [2.0, 0.25, 0.75], [np.nan, np.nan, np.nan],
                        [0.5, np.nan, 0.75], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5 + 2.0 ** -24], [0.5, 0.5, 0.5 + 2.0 ** -23], [0.25, 1.0, 1.0],
                        [np.inf, -np.inf, np.inf]], np.float32)
        n = min(len(e), u.shape[-2])
        u[..., :n, :] = e[:n]
    return u


# the float64 restatement of trimesh.sample.sample_surface ----------------------------------------------------------------------------
def trimesh_sample(vertices, faces, u):
    """trimesh's algorithm in float64 on the uniforms u [count,3] in [0, 1): the cumulative sum of the areas, searchsorted at
    u0 * total, the reflection of (u1, u2) whose sum exceeds 1, a + e1 * r1 + e2 * r2 -> points [count,3] float64, face [count]"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces)
    u = np.asarray(u, np.float32).astype(np.float64)
    a, e1, e2 = v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
    cum = np.cumsum(area)
    idx = np.searchsorted(cum, u[:, 0] * cum[-1])
    r = u[:, 1:].copy()
    flip = r.sum(1) > 1.0
    r[flip] = np.abs(r[flip] - 1.0)
    return a[idx] + e1[idx] * r[:, :1] + e2[idx] * r[:, 1:], idx


def on_face(vertices, faces, points, face) -> Tuple[float, float, float, float]:
    """in float64, for points [n,3] on faces face [n]: (the lowest barycentric coordinate, the largest sum of the two edge coordinates,
    the largest distance to the face's plane, the largest distance by which a point lies beyond an edge of its face: a negative
    barycentric coordinate times the height it is a fraction of, 0 if none does)"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces)[np.asarray(face)]
    p = np.asarray(points, np.float32).astype(np.float64)
    a, e1, e2 = v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    n = np.cross(e1, e2)
    d = p - a
    dist = np.abs((d * n).sum(1)) / np.linalg.norm(n, axis=1)
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    b1, b2 = (d * e1).sum(1), (d * e2).sum(1)
    det = g11 * g22 - g12 * g12
    r1, r2 = (g22 * b1 - g12 * b2) / det, (g11 * b2 - g12 * b1) / det
    e3 = e2 - e1
    twice_area = np.linalg.norm(n, axis=1)
    beyond = np.maximum.reduce([-r1 * twice_area / np.linalg.norm(e2, axis=1), -r2 * twice_area / np.linalg.norm(e1, axis=1),
                                -(1.0 - r1 - r2) * twice_area / np.linalg.norm(e3, axis=1), np.zeros_like(r1)])
    return float(min(r1.min(), r2.min(), (1.0 - r1 - r2).min())), float((r1 + r2).max()), float(dist.max()), float(beyond.max())


def extent(vertices) -> float:
    v = np.asarray(vertices, np.float64)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


# the meshes --------------------------------------------------------------------------------------------------------------------------
def cube():
    """the unit cube: 8 vertices (vertex k = the bits of k), 12 equal triangles"""
    v = np.asarray([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.asarray([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
    return v, f


def cylinder(n_seg: int = 64, radius: float = 0.5, height: float = 1.0):
    """a closed cylinder of n_seg segments: 2 n_seg side triangles, n_seg per cap around a centre vertex"""
    a = np.arange(n_seg) * (2.0 * np.pi / n_seg)
    ring = np.stack([radius * np.cos(a), radius * np.sin(a)], 1)
    v = np.concatenate([np.concatenate([ring, np.full((n_seg, 1), -height / 2)], 1), np.concatenate([ring, np.full((n_seg, 1), height / 2)], 1),
                        [[0.0, 0.0, -height / 2], [0.0, 0.0, height / 2]]]).astype(np.float32)
    f = []
    for k in range(n_seg):
        k1 = (k + 1) % n_seg
        f += [(k, k1, n_seg + k1), (k, n_seg + k1, n_seg + k), (2 * n_seg, k1, k), (2 * n_seg + 1, n_seg + k, n_seg + k1)]
    return v, np.asarray(f, np.int32)


def _rotations(rng, n: int) -> np.ndarray:
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def _triangles(rng, n: int) -> np.ndarray:
    """[n,3,3]: near-equilateral triangles with edges of 0.5 .. 1, randomly turned, centred within 0.25 of the origin"""
    ang = np.asarray([0.0, 2.0, 4.0]) * np.pi / 3.0 + rng.uniform(-0.2, 0.2, size=(n, 3))
    flat = np.stack([np.cos(ang), np.sin(ang), np.zeros_like(ang)], 2) * rng.uniform(0.3, 0.55, size=(n, 1, 1))
    return np.einsum("nij,nkj->nki", _rotations(rng, n), flat) + rng.uniform(-0.25, 0.25, size=(n, 1, 3))


def soup(n_faces: int, seed: Optional[int] = None):
    """n_faces random triangles, three vertices of their own each"""
    t = _triangles(np.random.RandomState(1000 + n_faces if seed is None else seed), n_faces)
    return t.reshape(-1, 3).astype(np.float32), np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


def soup_degenerate(n_faces: int = 300):
    """a soup where every third face has no area: by turns a repeated vertex and three collinear vertices on a grid of 1/64, whose
    differences and products are exact in fp32, so their weight is exactly zero"""
    v, f = soup(n_faces, seed=7)
    v = v.copy().reshape(n_faces, 3, 3)
    rng = np.random.RandomState(8)
    for k in range(2, n_faces, 3):
        a = rng.randint(-32, 33, size=3) / 64.0
        d = rng.randint(-8, 9, size=3) / 64.0
        v[k] = [a, a + d, a] if (k // 3) % 2 == 0 else [a, a + d, a + 2 * d]
    return v.reshape(-1, 3).astype(np.float32), f


def soup_spanning(n_faces: int = 257):
    """a soup whose areas span 2^-30 .. 1: triangle k is one right triangle of legs 1 next to the origin, randomly turned and scaled
    about the origin by 2^(-15 k / (n_faces - 1))"""
    rng = np.random.RandomState(9)
    base = np.asarray([[0.25, 0.25, 0.25], [1.25, 0.25, 0.25], [0.25, 1.25, 0.25]])
    s = 2.0 ** (-15.0 * np.arange(n_faces) / (n_faces - 1))
    t = np.einsum("nij,kj->nki", _rotations(rng, n_faces), base) * s[:, None, None]
    return t.reshape(-1, 3).astype(np.float32), np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


def with_nan_vertex():
    v, f = soup(65, seed=11)
    v = v.copy()
    v[100, 1] = np.nan
    return v, f


def with_bad_index():
    """one index equal to the vertex count (the first past the end) and one negative"""
    v, f = soup(65, seed=12)
    f = f.copy()
    f[40, 2] = len(v)
    f[7, 0] = -1
    return v, f


FAILED = ("nan_vertex", "bad_index")


@lru_cache(maxsize=None)
def meshes() -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
    """name -> (vertices [V,3] fp32, faces [F,3] int32), read-only"""
    out = {"cube": cube(), "cylinder": cylinder()}
    for n in SOUP_FACES:
        out[f"soup_{n}"] = soup(n)
    out["degenerate"] = soup_degenerate()
    out["spanning"] = soup_spanning()
    out["nan_vertex"] = with_nan_vertex()
    out["bad_index"] = with_bad_index()
    for v, f in out.values():
        v.setflags(write=False)
        f.setflags(write=False)
    return out


MULTI = ("soup_257", "nan_vertex", "cube", "soup_2049", "bad_index", "degenerate", "soup_1")   # the objects of the multi-object launch


@lru_cache(maxsize=None)
def case_uniforms(name: str, count: int) -> np.ndarray:
    """the uniforms [count,3] of one mesh at one count, edge values included, the same for every block"""
    u = uniforms((count,), seed=sorted(meshes()).index(name) * 10007 + count, edges=True)
    u.setflags(write=False)
    return u


@lru_cache(maxsize=None)
def emul_case(name: str, count: int, block: int):
    """the emulation's result on one mesh, computed once: points [count,3], face [count]"""
    return emul_one(meshes()[name], case_uniforms(name, count), block)


@lru_cache(maxsize=None)
def multi_case(count: int, block: int):
    """the multi-object launch: (vertices, faces, vert_off, face_off), u [n_obj,count,3], and the emulation's points and face"""
    packed = pack([meshes()[n] for n in MULTI])
    u = np.stack([case_uniforms(n, count) for n in MULTI])
    return packed, u, emul(*packed, u, block)
