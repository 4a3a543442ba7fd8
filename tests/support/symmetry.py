"""TEST SUPPORT: ctypes wrapper of the host emulation of the symmetry kernels (tests/symmetry_emul.cpp), built on first use; the float64
brute force the emulation and the kernel are held against; a backend that lets `evaluation.find_symmetries` run on the emulations; and
the meshes the CPU contract test and the GPU test share.  Every mesh is fp32, generated here, with extents of 0.1 .. 0.3 m."""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import surface_sample as ss
from .emul import CSRC, TESTS, _f32, _i32, _p, build

ULP = 2.0 ** -24
REL_TOL = 0.01
N_SAMPLES = 512
# the order of the rotation group every fixture must give
ORDERS = {"cube": 24, "box_123": 4, "square_prism": 8, "tetrahedron": 12, "hex_prism": 12, "pent_pyramid": 5, "cylinder_32": 64, "cone_32": 32,
          "box_dented": 1, "box_near_cube": 8, "cube_moved": 24, "cylinder_32_moved": 64}


def load():
    lib = build("symmetry_emul", [TESTS / "symmetry_emul.cpp", CSRC / "symmetry_core.h"])
    lib.symmetry_emul.restype = C.c_int
    lib.symmetry_emul_check.restype = C.c_int
    lib.symmetry_emul_tri_dist2.restype = C.c_float
    lib.symmetry_emul_limits.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_int * 5)()
    load().symmetry_emul_limits(v)
    return dict(block=int(v[0]), tile_step=int(v[1]), max_tile=int(v[2]), default_tile=int(v[3]), max_candidates=int(v[4]))


def tri_dist2(a, b, c, p) -> float:
    """the kernel's squared distance of p to the triangle a b c (fp32)"""
    return float(load().symmetry_emul_tri_dist2(_p(_f32(a)), _p(_f32(b)), _p(_f32(c)), _p(_f32(p))))


def emul(vertices, faces, tests, cand_R, centers, vert_off, face_off, test_off, cand_off, tol, mode: int = 0, tile: int = 0, cand_order=None):
    """the emulation on the arguments of the C ABI -> (rc, accept [C] uint8, dev2 [C] fp32, worst [C] int32); rc != 0: the arguments
    break a rule of mp_symmetry_check, nothing was computed; cand_order a permutation of the candidates (default: ascending)"""
    v, f, t = _f32(vertices).reshape(-1, 3), _i32(faces).reshape(-1, 3), _f32(tests).reshape(-1, 3)
    R, c = _f32(cand_R).reshape(-1, 9), _f32(centers).reshape(-1, 3)
    offs = [_i32(o) for o in (vert_off, face_off, test_off, cand_off)]
    tol = _f32(tol).reshape(-1)
    n_obj = len(c)
    assert all(len(o) == n_obj + 1 for o in offs) and len(tol) == n_obj
    order = None if cand_order is None else np.ascontiguousarray(cand_order, np.int64)
    n_cand = len(R)
    accept, dev2, worst = np.zeros(n_cand, np.uint8), np.full(n_cand, np.nan, np.float32), np.full(n_cand, -1, np.int32)
    rc = load().symmetry_emul(_p(v), _p(f), _p(t), _p(R), _p(c), _p(offs[0]), _p(offs[1]), _p(offs[2]), _p(offs[3]), _p(tol), C.c_int(n_obj),
                              C.c_int(tile), C.c_int(mode), _p(order), _p(accept), _p(dev2), _p(worst))
    return int(rc), accept, dev2, worst


class EmulBackend:
    """what `evaluation.find_symmetries(backend=...)` needs, on the host emulations and CPU tensors (device="cpu")"""

    def __init__(self, cand_order_seed: Optional[int] = None):
        self.cand_order_seed = cand_order_seed
        self.calls: List[dict] = []

    @staticmethod
    def surface_sample(vertices, faces, vert_off, face_off, u):
        points, face = ss.emul(vertices.numpy(), faces.numpy(), vert_off, face_off, u.numpy())
        return torch.from_numpy(points), torch.from_numpy(face)

    def symmetry_check(self, vertices, faces, tests, cand_R, centers, vert_off, face_off, test_off, cand_off, tol, mode=0, tile=0):
        n_cand = int(np.asarray(cand_off)[-1])
        order = None if self.cand_order_seed is None else np.random.RandomState(self.cand_order_seed).permutation(n_cand)
        args = (vertices.numpy(), np.asarray(faces), tests.numpy(), cand_R.numpy(), centers.numpy(), vert_off, face_off, test_off, cand_off, tol)
        rc, accept, dev2, worst = emul(*args, mode=mode, tile=tile, cand_order=order)
        assert rc == 0, rc
        self.calls.append(dict(args=args, mode=mode, tile=tile, accept=accept, dev2=dev2, worst=worst))
        return torch.from_numpy(accept), torch.from_numpy(dev2), torch.from_numpy(worst)


# the float64 brute force ---------------------------------------------------------------------------------------------------------------
def _seg_dist2(p, a, b):
    """[n,1,3] points against [1,m,3] segments a .. b -> [n,m] squared distances"""
    e = b - a
    ee = (e * e).sum(-1)
    t = torch.where(ee > 0.0, ((p - a) * e).sum(-1) / torch.where(ee > 0.0, ee, torch.ones_like(ee)), torch.zeros_like(ee))
    r = p - a - t.clamp(0.0, 1.0)[..., None] * e
    return (r * r).sum(-1)


def pair_dist2(p: torch.Tensor, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """[n,1,3] points against [1,m,3] triangles a b c -> [n,m] squared distances, NOT by the kernel's case analysis: the smallest of the
    distances to the three edges and, where the foot of the perpendicular lies inside a triangle with area, the distance to its plane.
    Any device and floating type."""
    d2 = torch.minimum(torch.minimum(_seg_dist2(p, a, b), _seg_dist2(p, b, c)), _seg_dist2(p, c, a))
    n = torch.cross(b - a, c - a, dim=-1)
    nn = (n * n).sum(-1)
    has_area = nn > 0.0
    safe = torch.where(has_area, nn, torch.ones_like(nn))
    h = ((p - a) * n).sum(-1)
    foot = p - (h / safe)[..., None] * n

    def side(x, y):     # the foot lies on the inner side of edge x -> y
        return (torch.cross((y - x).expand_as(foot), foot - x, dim=-1) * n).sum(-1) >= 0.0

    inside = has_area & side(a, b) & side(b, c) & side(c, a)
    return torch.where(inside, torch.minimum(d2, h * h / safe), d2)


def surface_dist2(points, vertices, faces) -> np.ndarray:
    """[n] float64: the squared distance of every point to the nearest triangle (pair_dist2 over points x triangles, float64, CPU)"""
    p = torch.from_numpy(np.ascontiguousarray(points, np.float64))[:, None, :]
    v = torch.from_numpy(np.asarray(vertices, np.float32).astype(np.float64))
    f = torch.from_numpy(np.asarray(faces).astype(np.int64))
    return pair_dist2(p, v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]).min(1)[0].numpy()


def deviations_f64(vertices, faces, tests, cand_R, center) -> np.ndarray:
    """[C] float64: for every candidate (the fp32 rotation and centre the kernel gets) the largest distance of g(p) to the surface"""
    t = np.asarray(tests, np.float32).astype(np.float64)
    c = np.asarray(center, np.float32).astype(np.float64)
    out = []
    for R in np.asarray(cand_R, np.float32).astype(np.float64).reshape(-1, 3, 3):
        out.append(np.sqrt(surface_dist2((t - c) @ R.T + c, vertices, faces).max()))
    return np.asarray(out)


def deviation_bound(vertices, faces, center) -> float:
    """the derived bound, in metres, on |fp32 deviation - float64 deviation| of one object (tests/test_symmetry_contract_cpu.py derives
    it): 2^-24 * (24 S + 16 K), S = |centre| + diameter, K = the largest over the triangles of kappa^2 D^2 / e_max with kappa =
    e_max^2 / (2 area), e_max the triangle's longest edge, D the diameter"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces)
    d = diameter(v)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e_max = np.max([np.linalg.norm(b - a, axis=1), np.linalg.norm(c - b, axis=1), np.linalg.norm(a - c, axis=1)], axis=0)
    twice_area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    kappa = e_max ** 2 / twice_area
    return ULP * (24.0 * (np.linalg.norm(center) + d) + 16.0 * float((kappa ** 2 * d * d / e_max).max()))


def diameter(vertices) -> float:
    """the largest distance between two vertices, float64 (what evaluation.model_info gives)"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    d = v[:, None, :] - v[None, :, :]
    return float(np.sqrt((d * d).sum(-1).max()))


# the meshes ------------------------------------------------------------------------------------------------------------------------------
def box(sx: float, sy: float, sz: float):
    """a box centred at the origin: 8 vertices (vertex k = the bits of k), 12 triangles"""
    v = (np.asarray([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], np.float64) - 0.5) * [sx, sy, sz]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v.astype(np.float32), np.asarray([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)


def _ring(n: int, radius: float, z: float) -> np.ndarray:
    a = np.arange(n) * (2.0 * np.pi / n)
    return np.stack([radius * np.cos(a), radius * np.sin(a), np.full(n, z)], 1)


def prism(n: int, radius: float, height: float):
    """a closed prism over a regular n-gon (a cylinder for large n): 2 n side triangles, n per cap around a cap-centre vertex"""
    v = np.concatenate([_ring(n, radius, -height / 2), _ring(n, radius, height / 2), [[0.0, 0.0, -height / 2], [0.0, 0.0, height / 2]]])
    f = []
    for k in range(n):
        k1 = (k + 1) % n
        f += [(k, k1, n + k1), (k, n + k1, n + k), (2 * n, k1, k), (2 * n + 1, n + k, n + k1)]
    return v.astype(np.float32), np.asarray(f, np.int32)


def cone(n: int, radius: float, height: float, closed: bool = True):
    """a cone (a pyramid for small n) over a regular n-gon: n side triangles and, closed, n base triangles around a base-centre vertex;
    open, it has exactly n triangles"""
    v = np.concatenate([_ring(n, radius, 0.0), [[0.0, 0.0, height]], [[0.0, 0.0, 0.0]] if closed else np.zeros((0, 3))])
    f = [(k, (k + 1) % n, n) for k in range(n)]
    if closed:
        f += [(n + 1, (k + 1) % n, k) for k in range(n)]
    return v.astype(np.float32), np.asarray(f, np.int32)


def tetrahedron(edge_half: float = 0.1):
    v = np.asarray([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * edge_half
    return v.astype(np.float32), np.asarray([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.int32)


MOTION_R = ss._rotations(np.random.RandomState(31), 1)[0]         # the fixed rigid motion of the moved fixtures
MOTION_T = np.asarray([0.05, -0.03, 0.08])


def moved(mesh):
    v, f = mesh
    return (np.asarray(v, np.float64) @ MOTION_R.T + MOTION_T).astype(np.float32), f


def dented_box():
    v, f = box(0.1, 0.2, 0.3)
    v = v.copy()
    v[7] += np.asarray([0.03, 0.02, 0.025], np.float32)
    return v, f


def needle():
    """three vertices on one line: a degenerate triangle, no second anchor"""
    return np.asarray([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.25, 0.0, 0.0]], np.float32), np.asarray([(0, 1, 2)], np.int32)


@lru_cache(maxsize=None)
def meshes() -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
    """name -> (vertices [V,3] fp32, faces [F,3] int32), read-only; the names of ORDERS"""
    out = {"cube": box(0.2, 0.2, 0.2), "box_123": box(0.1, 0.2, 0.3), "square_prism": box(0.1, 0.1, 0.2), "tetrahedron": tetrahedron(),
           "hex_prism": prism(6, 0.1, 0.2), "pent_pyramid": cone(5, 0.1, 0.15), "cylinder_32": prism(32, 0.05, 0.2), "cone_32": cone(32, 0.08, 0.2),
           "box_dented": dented_box(), "box_near_cube": box(0.1, 0.1, 0.106)}
    out["cube_moved"] = moved(out["cube"])
    out["cylinder_32_moved"] = moved(out["cylinder_32"])
    assert set(out) == set(ORDERS)
    for v, f in out.values():
        v.setflags(write=False)
        f.setflags(write=False)
    return out


class MeshSet:
    """the two attributes of a MeshDataBase that `find_symmetries` reads when it is given the diameters, for meshes held in memory"""

    def __init__(self, named: Dict[str, Tuple[np.ndarray, np.ndarray]]):
        self.labels = list(named)
        self.engine_meshes = {l: {"points": np.asarray(v, np.float32), "faces": np.asarray(f, np.int32)} for l, (v, f) in named.items()}

    def diameters(self) -> Dict[str, float]:
        return {l: diameter(self.engine_meshes[l]["points"]) for l in self.labels}


def mesh_database(named: Dict[str, Tuple[np.ndarray, np.ndarray]], out_dir):
    """a real MeshDataBase of the meshes, through PLY files in metres under out_dir (fp32 coordinates are kept bit for bit)"""
    from megapose6d_amd.mesh_db import MeshDataBase
    from megapose6d_amd.object_dataset import RigidObject

    from .synthetic import write_ply

    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    objs = []
    for label, (v, f) in named.items():
        write_ply(out_dir / f"{label}.ply", np.asarray(v, np.float32), np.asarray(f, np.int32))
        objs.append(RigidObject(label=label, mesh_path=out_dir / f"{label}.ply", mesh_units="m"))
    return MeshDataBase(objs)


def fixture_set(names: Optional[Sequence[str]] = None) -> MeshSet:
    ms = meshes()
    return MeshSet({n: ms[n] for n in (list(ORDERS) if names is None else names)})


@lru_cache(maxsize=None)
def found():
    """`find_symmetries` on all fixtures through the emulations, every candidate measured (mode 1), computed once -> (table, the
    backend with its one recorded call)"""
    from megapose6d_amd import evaluation as ev

    ms = fixture_set()
    backend = EmulBackend()
    table = ev.find_symmetries(ms, rel_tol=REL_TOL, n_samples=N_SAMPLES, diameters=ms.diameters(), device="cpu", measure_all=True, backend=backend)
    assert len(backend.calls) == 1
    return table, backend


def split_call(call) -> List[dict]:
    """one recorded symmetry_check call -> per object dict(vertices, faces, tests, cand_R, center, tol, accept, dev2, worst)"""
    v, f, t, R, c, vo, fo, to, co, tol = call["args"]
    out = []
    for o in range(len(c)):
        out.append(dict(vertices=v[vo[o]:vo[o + 1]], faces=f[fo[o]:fo[o + 1]], tests=t[to[o]:to[o + 1]], cand_R=R[co[o]:co[o + 1]], center=c[o],
                        tol=float(np.float32(tol[o])), accept=call["accept"][co[o]:co[o + 1]], dev2=call["dev2"][co[o]:co[o + 1]],
                        worst=call["worst"][co[o]:co[o + 1]]))
    return out
