"""TEST SUPPORT: ctypes wrapper of the host emulation of the mesh clean-up kernels (tests/mesh_cleanup_emul.cpp), built on first use; an
independent numpy restatement of the contract written from its text and not from csrc/mesh_cleanup_core.h (components by repeated
minimum over the faces until nothing changes, clustering with np.floor in float32, np.unique and Python-integer sums); the fixtures the
CPU contract test and the GPU test share; the backend that lets megapose6d_amd.mesh_cleanup run on the emulation; and the mesh checks."""
from __future__ import annotations

import ctypes as C
import functools
from typing import Dict, Optional, Tuple

import numpy as np

from . import tsdf as T
from .emul import CSRC, TESTS, _p, build

F32 = np.float32
SENTINEL = -7
RANK_SPAN = 256 * 16          # bytes one workgroup of the rank pass takes (kRankSpan of csrc/mesh_cleanup.hip)
SCAN_ROUND = 256              # workgroup totals one round of the scan takes (kMcBlock)


def load():
    lib = build("mesh_cleanup_emul", [TESTS / "mesh_cleanup_emul.cpp", CSRC / "mesh_cleanup_core.h"], fma=False)
    for name in ("mesh_components_emul", "mesh_select_count_emul", "mesh_select_emul", "mesh_cluster_count_emul", "mesh_cluster_emul"):
        getattr(lib, name).restype = C.c_int
    lib.mesh_cleanup_emul_limits.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_longlong * 3)()
    load().mesh_cleanup_emul_limits(v)
    return dict(max_count=int(v[0]), max_dim=int(v[1]), max_cells=int(v[2]))


class Mesh(dict):
    """vertices [V,3] f32, faces [F,3] i32, colors [V,3] f32 or None"""

    @property
    def V(self):
        return len(self["vertices"])

    @property
    def F(self):
        return len(self["faces"])


def mesh(vertices, faces, colors=None) -> Mesh:
    return Mesh(vertices=np.ascontiguousarray(vertices, F32).reshape(-1, 3), faces=np.ascontiguousarray(faces, np.int32).reshape(-1, 3),
                colors=None if colors is None else np.ascontiguousarray(colors, F32).reshape(-1, 3))


def _grid_args(origin, cell, dims):
    return [C.c_float(float(v)) for v in origin] + [C.c_float(float(cell))] + [C.c_int(int(v)) for v in dims]


# the emulation --------------------------------------------------------------------------------------------------------------------------
def emul_components(V: int, faces: np.ndarray):
    """-> labels [V], face_labels [F], face_count [V], totals [4] on arrays of exactly those sizes"""
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nf = len(faces)
    labels, fcount = np.full(V, SENTINEL, np.int32), np.full(V, SENTINEL, np.int32)
    flabels, totals = np.full(nf, SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)
    rc = load().mesh_components_emul(C.c_int(V), _p(faces) if nf else None, C.c_int(nf), _p(labels) if V else None, _p(flabels) if nf else None,
                                     _p(fcount) if V else None, _p(totals))
    assert rc == 0
    return labels, flabels, fcount, totals


def emul_select_count(V: int, faces, keep) -> Tuple[int, np.ndarray]:
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    keep = np.ascontiguousarray(keep, np.uint8)
    totals = np.full(3, SENTINEL, np.int32)
    rc = load().mesh_select_count_emul(C.c_int(V), _p(faces) if len(faces) else None, C.c_int(len(faces)), _p(keep) if len(faces) else None, _p(totals))
    return rc, totals


def emul_select(m: Mesh, keep, caps=None):
    """-> vertices, faces, colors (or None), n_bad; caps = (cap_vertices, cap_faces) to provoke a refusal (then -> the return code)"""
    keep = np.ascontiguousarray(keep, np.uint8)
    rc, totals = emul_select_count(m.V, m["faces"], keep)
    assert rc == 0
    nv, nf = int(totals[0]), int(totals[1])
    cv, cf = (nv, nf) if caps is None else caps
    ov, of = np.full((max(cv, 0), 3), SENTINEL, F32), np.full((max(cf, 0), 3), SENTINEL, np.int32)
    oc = None if m["colors"] is None else np.full((max(cv, 0), 3), SENTINEL, F32)
    rc = load().mesh_select_emul(_p(m["vertices"]) if m.V else None, _p(m["colors"]), C.c_int(m.V), _p(m["faces"]) if m.F else None, C.c_int(m.F),
                                 _p(keep) if m.F else None, C.c_int(nv), C.c_int(nf), _p(ov) if len(ov) else None,
                                 _p(oc) if oc is not None and len(oc) else None, _p(of) if len(of) else None, C.c_longlong(cv), C.c_longlong(cf))
    if caps is not None:
        return rc
    assert rc == 0
    return ov, of, oc, int(totals[2])


def emul_cluster_count(m: Mesh, origin, cell, dims) -> Tuple[int, np.ndarray]:
    totals = np.full(3, SENTINEL, np.int32)
    rc = load().mesh_cluster_count_emul(_p(m["vertices"]) if m.V else None, C.c_int(m.V), _p(m["faces"]) if m.F else None, C.c_int(m.F),
                                        *_grid_args(origin, cell, dims), _p(totals))
    return rc, totals


def emul_cluster(m: Mesh, origin, cell, dims, caps=None):
    rc, totals = emul_cluster_count(m, origin, cell, dims)
    assert rc == 0
    nv, nf = int(totals[0]), int(totals[1])
    cv, cf = (nv, nf) if caps is None else caps
    ov, of = np.full((max(cv, 0), 3), SENTINEL, F32), np.full((max(cf, 0), 3), SENTINEL, np.int32)
    oc = None if m["colors"] is None else np.full((max(cv, 0), 3), SENTINEL, F32)
    rc = load().mesh_cluster_emul(_p(m["vertices"]) if m.V else None, _p(m["colors"]), C.c_int(m.V), _p(m["faces"]) if m.F else None, C.c_int(m.F),
                                  *_grid_args(origin, cell, dims), C.c_int(nv), C.c_int(nf), _p(ov) if len(ov) else None,
                                  _p(oc) if oc is not None and len(oc) else None, _p(of) if len(of) else None, C.c_longlong(cv), C.c_longlong(cf))
    if caps is not None:
        return rc
    assert rc == 0
    return ov, of, oc, int(totals[2])


class EmulBackend:
    """megapose6d_amd.mesh_cleanup on the host emulation: the interface of its DeviceBackend on numpy arrays"""

    def __init__(self):
        self.count_calls = []

    def mesh(self, m):
        return mesh(m["vertices"], m["faces"], m.get("colors"))

    def bounds(self, vertices):
        ok = np.isfinite(vertices).all(1)
        return (vertices[ok].min(0), vertices[ok].max(0)) if ok.any() else None

    def components(self, n_vertices, faces):
        labels, flabels, fcount, totals = emul_components(n_vertices, faces)
        return labels, flabels, fcount, [int(v) for v in totals]

    def keep_bytes(self, face_labels, face_count, largest, min_faces):
        keep = face_labels >= 0
        if largest is not None:
            keep &= face_labels == largest
        if min_faces is not None:
            keep &= face_count[np.maximum(face_labels, 0)] >= min_faces
        return keep.astype(np.uint8)

    def select(self, vertices, faces, keep, colors):
        return emul_select(mesh(vertices, faces, colors), keep)

    def cluster_count(self, vertices, faces, origin, cell, dims):
        rc, totals = emul_cluster_count(mesh(vertices, faces), origin, cell, dims)
        assert rc == 0
        self.count_calls.append((tuple(origin), cell, tuple(dims), int(totals[1])))
        return tuple(int(v) for v in totals)

    def cluster(self, vertices, faces, origin, cell, dims, colors):
        return emul_cluster(mesh(vertices, faces, colors), origin, cell, dims)


# the restatement ------------------------------------------------------------------------------------------------------------------------
def _good(faces: np.ndarray, V: int) -> np.ndarray:
    return ((faces >= 0) & (faces < V)).all(1) if len(faces) else np.zeros(0, bool)


def restated_components(V: int, faces: np.ndarray):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if V == 0 or len(faces) == 0:
        return np.arange(V, dtype=np.int32), np.full(len(faces), -1, np.int32), np.zeros(V, np.int32), np.array([0, -1, 0, 0], np.int32)
    good = _good(faces, V)
    g = faces[good]
    lab = np.arange(V, dtype=np.int64)
    while True:
        before = lab.copy()
        if len(g):
            low = lab[g].min(1)                      # the smallest label on each face ...
            for k in range(3):
                np.minimum.at(lab, g[:, k], low)     # ... goes to its three vertices
        while True:                                  # and along the labels themselves (a label is a vertex)
            nxt = lab[lab]
            if (nxt == lab).all():
                break
            lab = nxt
        if (lab == before).all():
            break
    flab = np.where(good, lab[np.where(good, faces[:, 0], 0)], -1)
    count = np.bincount(flab[good], minlength=V)
    owners = np.nonzero(count)[0]
    largest = int(owners[np.argmax(count[owners])]) if len(owners) else -1       # argmax takes the first: the smaller label
    return lab.astype(np.int32), flab.astype(np.int32), count.astype(np.int32), np.array([len(owners), largest, int((~good).sum()), 0], np.int32)


def restated_select(m: Mesh, keep):
    if m.V == 0 or m.F == 0:
        return np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), None if m["colors"] is None else np.zeros((0, 3), F32), 0
    good = _good(m["faces"], m.V)
    kept = m["faces"][good & (np.asarray(keep) != 0)]
    ref = np.unique(kept)                            # ascending = input order
    faces = np.searchsorted(ref, kept).astype(np.int32).reshape(-1, 3)
    return m["vertices"][ref], faces, None if m["colors"] is None else m["colors"][ref], int((~good).sum())


def restated_cluster(m: Mesh, origin, cell, dims):
    if m.V == 0 or m.F == 0:
        return np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), None if m["colors"] is None else np.zeros((0, 3), F32), 0
    o, c, g = np.asarray(origin, F32), F32(cell), np.asarray(dims, np.int64)
    with np.errstate(all="ignore"):
        u = (m["vertices"] - o[None, :]) / c
        assert u.dtype == F32
        i = np.floor(u)
        ok = ((i >= 0) & (i < g[None, :].astype(F32))).all(1)
        ii = np.where(ok[:, None], i, 0).astype(np.int64)
    cell_id = np.where(ok, ii[:, 0] + g[0] * (ii[:, 1] + g[1] * ii[:, 2]), -1)
    good = _good(m["faces"], m.V)
    fc = np.where(good[:, None], cell_id[np.where(good[:, None], m["faces"], 0)], -1)
    usable = good & (fc >= 0).all(1)
    kept = usable & (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    used = np.unique(fc[kept])
    faces = np.searchsorted(used, fc[kept]).astype(np.int32).reshape(-1, 3)
    rank_of = {int(k): r for r, k in enumerate(used)}
    sums = [[0, 0, 0, 0, 0, 0] for _ in used]
    counts = [0] * len(used)
    with np.errstate(all="ignore"):
        fixed = (u * F32(65536.0)).astype(F32)
        q = None if m["colors"] is None else (np.fmin(np.fmax(m["colors"], F32(0)), F32(1)) * F32(65535.0) + F32(0.5)).astype(F32)
    for v in np.nonzero(ok)[0]:
        r = rank_of.get(int(cell_id[v]))
        if r is None:
            continue
        counts[r] += 1
        for k in range(3):
            sums[r][k] += int(fixed[v, k])           # int() truncates
            if q is not None:
                sums[r][3 + k] += int(q[v, k])
    verts = np.zeros((len(used), 3), F32)
    cols = None if m["colors"] is None else np.zeros((len(used), 3), F32)
    for r in range(len(used)):
        for k in range(3):
            verts[r, k] = F32(float(o[k]) + float(c) * (sums[r][k] / (counts[r] * 65536.0)))
            if cols is not None:
                cols[r, k] = F32(sums[r][3 + k] / (counts[r] * 65535.0))
    return verts, faces, cols, int((~usable).sum())


# mesh checks ----------------------------------------------------------------------------------------------------------------------------
def edge_balance(faces: np.ndarray, V: int) -> Dict[str, object]:
    """for every directed edge (a, b): is its multiplicity that of (b, a)?  plus the index range and the unreferenced vertices"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fwd, fc = np.unique(d[:, 0] * V + d[:, 1], return_counts=True)
    rev, rc = np.unique(d[:, 1] * V + d[:, 0], return_counts=True)
    return dict(balanced=bool(len(fwd) == len(rev) and (fwd == rev).all() and (fc == rc).all()),
                index_ok=bool(len(f) == 0 or (f.min() >= 0 and f.max() < V)), unreferenced=int(V - len(np.unique(f))),
                no_loop=bool((d[:, 0] != d[:, 1]).all()))


def signed_volume(vertices, faces) -> float:
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# fixtures -------------------------------------------------------------------------------------------------------------------------------
def _tsdf_mesh(name: str) -> Mesh:
    g, views = T.fixture(name)
    vol = T.new_volume(g.dims, True)
    assert T.emul_integrate(vol, g, views) == 0
    v, c, f = T.emul_extract(vol, g)
    return mesh(v, f, c)


@functools.lru_cache(None)
def sphere() -> Mesh:
    return _tsdf_mesh("sphere")          # 7754 vertices, 15 504 faces


@functools.lru_cache(None)
def torus() -> Mesh:
    return _tsdf_mesh("torus")           # 6054 vertices, 12 108 faces


SPHERE_VOXEL = T.cube_grid().voxel
SPHERE_ORIGIN = T.cube_grid().origin
SCENE_SHIFT = 0.2                        # the torus sits this far along x from the sphere
TETRA = np.array([[0, 0, 0], [0.004, 0, 0], [0, 0.004, 0], [0, 0, 0.004]], F32) + F32(0.1)
TETRA_FACES = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
LOOSE = np.array([[0.3, 0.3, 0.3], [-0.3, 0.1, 0.2], [0.0, 0.0, 0.0]], F32)


@functools.lru_cache(None)
def scene_parts() -> Mesh:
    """sphere, torus (shifted), tetrahedron, three vertices on no face: in this order, not yet permuted, no bad face"""
    s, t = sphere(), torus()
    tv = t["vertices"].copy()
    tv[:, 0] += F32(SCENE_SHIFT)
    vertices = np.concatenate([s["vertices"], tv, TETRA, LOOSE])
    colors = np.concatenate([s["colors"], t["colors"], np.full((4, 3), 0.25, F32), np.array([[2.0, -1.0, np.nan]] * 3, F32)])
    faces = np.concatenate([s["faces"], t["faces"] + s.V, TETRA_FACES + s.V + t.V])
    return mesh(vertices, faces, colors)


@functools.lru_cache(None)
def scene() -> Mesh:
    """the parts with the vertices renumbered by a seeded permutation, and two bad faces (index -1, index V) in the middle and at the end"""
    p = scene_parts()
    rng = np.random.default_rng(20240611)
    new_of_old = rng.permutation(p.V)
    vertices, colors = np.empty_like(p["vertices"]), np.empty_like(p["colors"])
    vertices[new_of_old], colors[new_of_old] = p["vertices"], p["colors"]
    faces = new_of_old[p["faces"]].astype(np.int32)
    half = len(faces) // 2
    faces = np.concatenate([faces[:half], [[3, -1, 5]], faces[half:], [[7, 8, p.V]]]).astype(np.int32)
    return mesh(vertices, faces, colors)


def scene_sphere_label() -> int:
    """the label the sphere's component must get: the smallest new index of its vertices"""
    rng = np.random.default_rng(20240611)
    return int(rng.permutation(scene_parts().V)[:sphere().V].min())


def _bit_reverse(k: np.ndarray, bits: int) -> np.ndarray:
    out = np.zeros_like(k)
    for b in range(bits):
        out |= ((k >> b) & 1) << (bits - 1 - b)
    return out


@functools.lru_cache(None)
def chain(order: str, n: int = 5000) -> Mesh:
    """a strip of n triangles (k, k+1, k+2), its vertices numbered in order, in reverse or by bit reversal: the longest parent chains"""
    k = np.arange(n + 2)
    pos = np.stack([(k // 2) * 0.01, (k % 2) * 0.01, np.zeros(n + 2)], 1).astype(F32)
    if order == "forward":
        new = k
    elif order == "reverse":
        new = n + 1 - k
    elif order == "bitrev":
        new = np.argsort(np.argsort(_bit_reverse(k, 13), kind="stable"), kind="stable")
    else:
        raise ValueError(order)
    vertices = np.empty_like(pos)
    vertices[new] = pos
    t = np.arange(n)
    faces = np.stack([new[t], new[t + 1], new[t + 2]], 1)
    return mesh(vertices, faces)


@functools.lru_cache(None)
def star(n: int = 4000) -> Mesh:
    """n triangles around vertex V - 1: every union meets the same vertex"""
    a = np.linspace(0, 2 * np.pi, n + 1)
    vertices = np.concatenate([np.stack([np.cos(a), np.sin(a), np.zeros(n + 1)], 1), [[0, 0, 0]]]).astype(F32)
    t = np.arange(n)
    return mesh(vertices, np.stack([np.full(n, n + 1), t, t + 1], 1))


LARGE_MIN_FACES = RANK_SPAN * SCAN_ROUND + 1     # more than 256 workgroups' worth of faces: the scan's second round


@functools.lru_cache(None)
def large() -> Mesh:
    """the scene tiled along y until its faces fill more than 256 workgroups of the rank pass; two bad faces at the end"""
    s = scene()
    good = s["faces"][_good(s["faces"], s.V)]
    copies = -(-LARGE_MIN_FACES // len(good))
    vertices = np.concatenate([s["vertices"] + np.array([0, 0.2 * k, 0], F32) for k in range(copies)])
    colors = np.concatenate([s["colors"]] * copies)
    faces = np.concatenate([good + k * s.V for k in range(copies)] + [np.array([[0, 1, -5], [copies * s.V, 0, 1]])])
    return mesh(vertices, faces, colors)


def keep_variants(m: Mesh) -> Dict[str, np.ndarray]:
    labels, flabels, fcount, totals = emul_components(m.V, m["faces"])
    third = np.zeros(m.F, np.uint8)
    third[::3] = 200                                  # any non-zero byte keeps
    return dict(all=np.ones(m.F, np.uint8), none=np.zeros(m.F, np.uint8), third=third, largest=(flabels == totals[1]).astype(np.uint8))


CELLS_VOXELS = (1.5, 2.0, 3.0, 4.0)
SHIFTS = (0.0, 0.37)


def grid_of(m: Mesh, cell_voxels: float, shift_voxels: float, voxel: float = SPHERE_VOXEL):
    """a grid of cells of cell_voxels voxels that holds the finite vertices of m, its origin `shift_voxels` voxels before their minimum
    (0: aligned with it)"""
    ok = np.isfinite(m["vertices"]).all(1)
    lo, hi = m["vertices"][ok].min(0), m["vertices"][ok].max(0)
    cell = F32(cell_voxels) * F32(voxel)
    origin = (lo - F32(shift_voxels) * F32(voxel)).astype(F32)
    dims = tuple(int(v) for v in np.floor((hi - origin) / cell).astype(np.int64) + 1)
    return tuple(float(v) for v in origin), float(cell), dims
