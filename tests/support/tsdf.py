"""TEST SUPPORT: ctypes wrapper of the host emulation of the TSDF kernels (tests/tsdf_emul.cpp), built on first use; an independent numpy
restatement of the contract written from its text and not from csrc/tsdf_core.h (float32 numpy operations one by one, whole volumes at
a time; the triangle cases from the wording of the rule with the winding decided by a cross product in float64, not from the header's
table); the fixtures the CPU contract test and the GPU test share (analytic sphere, sphere-traced torus, a field set directly, odd
volumes, awkward views); and the mesh checks (directed edges, Euler characteristic, signed volume)."""
from __future__ import annotations

import ctypes as C
import functools
import itertools
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np

from .emul import CSRC, TESTS, _p, build

F = np.float32
Z_MIN = 1e-3
KIND_DIFFS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)]      # +x +y +z +x+y +y+z +x+z +x+y+z
AXIS_ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


class Grid(NamedTuple):
    origin: Tuple[float, float, float]
    voxel: float
    dims: Tuple[int, int, int]          # nx, ny, nz

    @property
    def mu3(self) -> np.float32:
        return F(3.0) * F(self.voxel)


def load():
    lib = build("tsdf_emul", [TESTS / "tsdf_emul.cpp", CSRC / "tsdf_core.h"], fma=False)
    for name in ("tsdf_integrate_emul", "tsdf_extract_count_emul", "tsdf_extract_emul"):
        getattr(lib, name).restype = C.c_int
    lib.tsdf_emul_limits.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_longlong * 6)()
    load().tsdf_emul_limits(v)
    return dict(min_dim=int(v[0]), max_dim=int(v[1]), max_nodes=int(v[2]), max_side=int(v[3]), edge_kinds=int(v[4]), tets=int(v[5]))


def new_volume(dims, color: bool) -> np.ndarray:
    """[2 or 6, nz, ny, nx] float32 zeros; the count planes (1 and 5) hold int32 bits"""
    nx, ny, nz = dims
    return np.zeros((6 if color else 2, nz, ny, nx), F)


def counts_of(vol: np.ndarray) -> np.ndarray:
    return vol[1].view(np.int32)


def _grid_args(g: Grid):
    nx, ny, nz = g.dims
    return [C.c_int(nx), C.c_int(ny), C.c_int(nz)], [C.c_float(g.origin[0]), C.c_float(g.origin[1]), C.c_float(g.origin[2]), C.c_float(g.voxel)]


def view_arrays(views, sel=slice(None)):
    depth = np.ascontiguousarray(views["depth"][sel], F)
    masks = None if views.get("masks") is None else np.ascontiguousarray(views["masks"][sel], np.uint8)
    rgb = None if views.get("rgb") is None else np.ascontiguousarray(views["rgb"][sel], np.uint8)
    K = np.ascontiguousarray(views["K"][sel], F).reshape(-1, 9)
    TCO = np.ascontiguousarray(views["TCO"][sel], F).reshape(len(K), int(np.prod(views["TCO"].shape[1:])))
    return depth, masks, rgb, K, TCO


def emul_integrate(vol: np.ndarray, g: Grid, views, sel=slice(None), carve=True, mu=None, z_min=Z_MIN) -> int:
    """in place; -> the return code"""
    depth, masks, rgb, K, TCO = view_arrays(views, sel)
    n, h, w = depth.shape
    dims, grid = _grid_args(g)
    assert vol.flags.c_contiguous and vol.dtype == F
    return load().tsdf_integrate_emul(_p(vol), *dims, C.c_int(int(vol.shape[0] == 6)), *grid, _p(depth), _p(masks), _p(rgb), _p(K), _p(TCO),
                                      C.c_int(TCO.shape[1]), C.c_int(n), C.c_int(h), C.c_int(w), C.c_float(g.mu3 if mu is None else mu),
                                      C.c_float(z_min), C.c_int(int(carve)))


def emul_extract(vol: np.ndarray, g: Grid, min_views=1):
    """-> vertices [nv,3] f32, colors [nv,3] f32, faces [nt,3] i32, on arrays of exactly the counted sizes"""
    dims, grid = _grid_args(g)
    color = C.c_int(int(vol.shape[0] == 6))
    totals = np.full(2, -1, np.int32)
    assert load().tsdf_extract_count_emul(_p(vol), *dims, color, C.c_int(min_views), _p(totals)) == 0
    nv, nt = int(totals[0]), int(totals[1])
    v, c, f = np.full((nv, 3), -7, F), np.full((nv, 3), -7, F), np.full((nt, 3), -7, np.int32)
    rc = load().tsdf_extract_emul(_p(vol), *dims, color, *grid, C.c_int(min_views), C.c_int(nv), C.c_int(nt), _p(v) if nv else None,
                                  _p(c) if nv else None, _p(f) if nt else None, C.c_longlong(nv), C.c_longlong(nt))
    assert rc == 0
    return v, c, f


# the restatement ----------------------------------------------------------------------------------------------------------------------
def _node_coords(g: Grid):
    nx, ny, nz = g.dims
    ox, oy, oz = (F(v) for v in g.origin)
    vx = F(g.voxel)
    px = (ox + vx * np.arange(nx).astype(F))[None, None, :]
    py = (oy + vx * np.arange(ny).astype(F))[None, :, None]
    pz = (oz + vx * np.arange(nz).astype(F))[:, None, None]
    return px, py, pz


def restated_integrate(vol: np.ndarray, g: Grid, views, sel=slice(None), carve=True, mu=None, z_min=Z_MIN) -> None:
    """the contract's five steps per view on the whole volume at once, in place"""
    depth, masks, rgb, K, TCO = view_arrays(views, sel)
    n, h, w = depth.shape
    mu, z_min = F(g.mu3 if mu is None else mu), F(z_min)
    px, py, pz = _node_coords(g)
    color = vol.shape[0] == 6
    cnt = vol[1].view(np.int32)
    ccnt = vol[5].view(np.int32) if color else None
    with np.errstate(all="ignore"):
        for v in range(n):
            if not (np.isfinite(K[v]).all() and np.isfinite(TCO[v, :12]).all()):
                continue
            T = TCO[v]
            fx, cx, fy, cy = K[v, 0], K[v, 2], K[v, 4], K[v, 5]
            cam = [((T[4 * r + 0] * px + T[4 * r + 1] * py) + T[4 * r + 2] * pz) + T[4 * r + 3] for r in range(3)]
            assert all(c.dtype == F for c in cam)
            ok = cam[2] > z_min
            xf = np.floor((fx * cam[0]) / cam[2] + cx)
            yf = np.floor((fy * cam[1]) / cam[2] + cy)
            ok = ok & (xf >= 0) & (xf < F(w)) & (yf >= 0) & (yf < F(h))
            xi = np.where(ok, xf, 0).astype(np.int64)
            yi = np.where(ok, yf, 0).astype(np.int64)
            off_mask = (masks[v][yi, xi] == 0) if masks is not None else np.zeros_like(ok)
            if carve:
                free = ok & off_mask
                vol[0][free] = vol[0][free] + F(1)
                cnt[free] += 1
            d = depth[v][yi, xi]
            meas = ok & ~off_mask & np.isfinite(d) & (d > 0)
            sd = d - cam[2]
            use = meas & (sd >= -mu)
            vol[0][use] = vol[0][use] + np.minimum(F(1), sd / mu)[use]
            cnt[use] += 1
            if color and rgb is not None:
                cuse = use & (np.abs(sd) <= mu)
                for c in range(3):
                    vol[2 + c][cuse] = vol[2 + c][cuse] + rgb[v][yi, xi, c].astype(F)[cuse]
                ccnt[cuse] += 1


@functools.lru_cache(None)
def _case_triangles(order, case):
    """the triangles of the tetrahedron of axis order `order` whose inside corners are the bits of `case`, as the rule words them: a
    list of three (corner code of the owner, kind) each, wound by the cross product so that the normal points from the inside corners'
    centroid to the outside corners'"""
    e = np.eye(3, dtype=int)
    corners = [np.zeros(3, int), e[order[0]], e[order[0]] + e[order[1]], np.ones(3, int)]
    ins = [q for q in range(4) if (case >> q) & 1]
    out = [q for q in range(4) if not (case >> q) & 1]
    if len(ins) in (1, 3):
        a = (ins if len(ins) == 1 else out)[0]
        b, c, d = [q for q in range(4) if q != a]
        tris = [[(a, b), (a, c), (a, d)]]
    elif len(ins) == 2:
        (a, b), (c, d) = ins, out
        tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    else:
        return ()
    towards = np.mean([corners[q] for q in out], 0) - np.mean([corners[q] for q in ins], 0)
    res = []
    for tri in tris:
        mid = [(corners[p] + corners[q]) / 2.0 for p, q in tri]
        if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), towards) < 0:
            tri = [tri[0], tri[2], tri[1]]
        edges = []
        for p, q in tri:
            lo, hi = corners[min(p, q)], corners[max(p, q)]
            edges.append((tuple(int(t) for t in lo), KIND_DIFFS.index(tuple(int(t) for t in hi - lo))))
        res.append(tuple(edges))
    return tuple(res)


def restated_extract(vol: np.ndarray, g: Grid, min_views=1):
    nx, ny, nz = g.dims
    color = vol.shape[0] == 6
    cnt = vol[1].view(np.int32)
    obs = cnt >= min_views
    with np.errstate(all="ignore"):
        f = vol[0] / cnt.astype(F)
        inside = obs & (f < 0)
        col = [np.where(vol[5].view(np.int32) > 0, (vol[2 + c] / vol[5].view(np.int32).astype(F)) / F(255), F(1)).astype(F) if color
               else np.ones_like(f) for c in range(3)]
    complete = np.zeros((nz, ny, nx), bool)             # complete[k,j,i]: the cell whose c0 is (i,j,k)
    acc = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        acc &= obs[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    complete[:nz - 1, :ny - 1, :nx - 1] = acc
    carries = np.zeros((nz, ny, nx, 7), bool)
    for kind, (dx, dy, dz) in enumerate(KIND_DIFFS):
        a = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        b = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        cross = obs[a] & obs[b] & (inside[a] != inside[b])
        near = np.zeros((nz, ny, nx), bool)
        for bx, by, bz in itertools.product(*[(0,) if d else (0, 1) for d in (dx, dy, dz)]):
            sh = np.zeros((nz, ny, nx), bool)           # sh[k,j,i] = complete[k-bz, j-by, i-bx]
            sh[bz:, by:, bx:] = complete[:nz - bz, :ny - by, :nx - bx]
            near |= sh
        carries[..., kind][a] = cross & near[a]
    flat = carries.reshape(-1)
    vid = np.where(flat, np.cumsum(flat) - 1, -1).reshape(nz, ny, nx, 7)
    kk, jj, ii, kinds = np.nonzero(carries)              # in the order of node * 7 + kind
    diffs = np.asarray(KIND_DIFFS)[kinds]
    fa, fb = f[kk, jj, ii], f[kk + diffs[:, 2], jj + diffs[:, 1], ii + diffs[:, 0]]
    t = fa / (fa - fb)
    org, vx = [F(v) for v in g.origin], F(g.voxel)
    verts = np.empty((len(t), 3), F)
    cols = np.empty((len(t), 3), F)
    for c, idx in enumerate((ii, jj, kk)):
        pa = org[c] + vx * idx.astype(F)
        pb = org[c] + vx * (idx + diffs[:, c]).astype(F)
        verts[:, c] = pa + t * (pb - pa)
        ca, cb = col[c][kk, jj, ii], col[c][kk + diffs[:, 2], jj + diffs[:, 1], ii + diffs[:, 0]]
        cols[:, c] = ca + t * (cb - ca)
    ck, cj, ci = np.nonzero(complete)
    cell_lin = (ck * ny + cj) * nx + ci
    rows, keys = [], []
    for T, order in enumerate(AXIS_ORDERS):
        e = np.eye(3, dtype=int)
        corners = [np.zeros(3, int), e[order[0]], e[order[0]] + e[order[1]], np.ones(3, int)]
        case = np.zeros(len(ci), int)
        for q, cn in enumerate(corners):
            case |= inside[ck + cn[2], cj + cn[1], ci + cn[0]].astype(int) << q
        for m in range(1, 15):
            sel = case == m
            if not sel.any():
                continue
            for n_tri, tri in enumerate(_case_triangles(order, m)):
                rows.append(np.stack([vid[ck[sel] + lo[2], cj[sel] + lo[1], ci[sel] + lo[0], kind] for lo, kind in tri], 1))
                keys.append((cell_lin[sel] * 6 + T) * 2 + n_tri)
    if rows:
        faces = np.concatenate(rows)[np.argsort(np.concatenate(keys), kind="stable")].astype(np.int32)
    else:
        faces = np.zeros((0, 3), np.int32)
    return verts, cols, faces


# mesh checks --------------------------------------------------------------------------------------------------------------------------
def mesh_report(vertices, faces) -> Dict[str, float]:
    """closed and consistently wound (every directed edge once, its reverse once), V - E + F, the signed volume, unreferenced vertices"""
    f = np.asarray(faces, np.int64)
    nv = len(vertices)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = d[:, 0] * nv + d[:, 1]
    rev = d[:, 1] * nv + d[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    v = np.asarray(vertices, np.float64)
    vol = float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)
    return dict(directed_once=bool((counts == 1).all()), reverse_present=bool(np.isin(rev, uniq).all()), no_loop=bool((d[:, 0] != d[:, 1]).all()),
                euler=nv - len(uniq) // 2 + len(f), volume=vol, unreferenced=int(nv - len(np.unique(f))),
                index_ok=bool(len(f) == 0 or (f.min() >= 0 and f.max() < nv)))


# fixtures -----------------------------------------------------------------------------------------------------------------------------
SPHERE_R = 0.05
TORUS_R, TORUS_r = 0.04, 0.015
H, W = 48, 64


def look_at(position, up=(0.0, 0.0, 1.0)) -> np.ndarray:
    """TCO [4,4] float64 of a camera at `position` looking at the origin (x right, y down, z forward)"""
    c = np.asarray(position, np.float64)
    z = -c / np.linalg.norm(c)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])                  # rows: camera axes in the object frame = R_co
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ c
    return T


def intrinsics(f=200.0, h=H, w=W) -> np.ndarray:
    return np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1]], np.float64)


def corner_cameras(dist=0.4) -> np.ndarray:
    return np.stack([look_at(dist * np.array(s, np.float64) / np.sqrt(3.0)) for s in itertools.product((-1, 1), repeat=3)])


def _rays(K, h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([(xs + 0.5 - K[0, 2]) / K[0, 0], (ys + 0.5 - K[1, 2]) / K[1, 1], np.ones((h, w))], -1)     # z = 1: the parameter is the depth


def sphere_depth(TCO, K, r=SPHERE_R, h=H, w=W) -> np.ndarray:
    """exact ray-sphere intersection at pixel centres, float64; 0 where the ray misses"""
    d = _rays(K, h, w)
    c = TCO[:3, 3]
    dd, dc = (d * d).sum(-1), d @ c
    disc = dc * dc - dd * (c @ c - r * r)
    s = (dc - np.sqrt(np.maximum(disc, 0))) / dd
    return np.where((disc > 0) & (s > 0), s, 0.0)


def torus_depth(TCO, K, h=H, w=W) -> np.ndarray:
    """sphere tracing of the torus around z (float64): 0 where the ray misses"""
    d = _rays(K, h, w)
    ln = np.linalg.norm(d, axis=-1)
    Roc = TCO[:3, :3].T
    o = -Roc @ TCO[:3, 3]
    dirs = (d / ln[..., None]) @ Roc.T
    s = np.zeros((h, w))
    hit = np.zeros((h, w), bool)
    for _ in range(256):
        p = o + s[..., None] * dirs
        dist = np.hypot(np.hypot(p[..., 0], p[..., 1]) - TORUS_R, p[..., 2]) - TORUS_r
        hit = dist < 1e-9
        s = np.where(hit | (s > 1.0), s, s + dist)
    return np.where(hit, s / ln, 0.0)


def _surface_rgb(depth, TCO, K) -> np.ndarray:
    """a colour per pixel from the surface point in the object frame, so that the views agree with each other"""
    pts = (_rays(K, *depth.shape) * depth[..., None] - TCO[:3, 3]) @ TCO[:3, :3]
    rgb = np.clip(128.0 + 2000.0 * pts, 0, 255).astype(np.uint8)
    rgb[depth <= 0] = 0
    return rgb


def _views(depth_fn, cams, K=None) -> Dict[str, np.ndarray]:
    K = intrinsics() if K is None else K
    depth = np.stack([depth_fn(T, K) for T in cams])
    return dict(depth=depth.astype(F), masks=(depth > 0).astype(np.uint8), rgb=np.stack([_surface_rgb(d, T, K) for d, T in zip(depth, cams)]),
                K=np.repeat(K[None], len(cams), 0).astype(F), TCO=cams.astype(F))


def cube_grid(n=32, half=0.066) -> Grid:
    return Grid((-half, -half, -half), float(F(2 * half) / F(n - 1)), (n, n, n))


@functools.lru_cache(None)
def sphere_views():
    return _views(sphere_depth, corner_cameras())


@functools.lru_cache(None)
def torus_views():
    cams = np.concatenate([corner_cameras(), np.stack([look_at((0.02, 0.0, 0.4), up=(0, 1, 0)), look_at((0.0, 0.02, -0.4), up=(0, 1, 0))])])
    return _views(torus_depth, cams)


@functools.lru_cache(None)
def many_views(n=40):
    """n different views of the sphere from a spiral over the sphere of directions, view 35 with a non-finite K: more views in one call
    than the integrate kernel stages at a time (32), with a partial last round, and no two views alike, so that a view taken from the
    wrong round shows"""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    dirs = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    cams = np.stack([look_at((0.35 + 0.002 * i) * d, up=(0, 0, 1) if abs(d[2]) < 0.9 else (0, 1, 0)) for i, d in enumerate(dirs)])
    views = _views(sphere_depth, cams)
    views["K"][35, 1, 1] = np.nan
    return views


TORUS_GRID = Grid((-0.066, -0.066, -0.0275), float(F(0.132) / F(31)), (32, 32, 14))
ODD_GRID = Grid((-0.07, -0.04, -0.02), 0.0045, (33, 17, 9))
TINY_GRID = Grid((0.042, -0.004, -0.003), 0.012, (2, 2, 2))          # eight nodes across the sphere's surface: fewer than one wave


@functools.lru_cache(None)
def awkward_views():
    """a sphere half outside the image; a camera inside the volume; depth with NaN, inf, 0 and negative values; a non-finite K and a
    non-finite TCO; then two ordinary views so that something is integrated at all"""
    K = intrinsics()
    cams = corner_cameras()
    views = _views(sphere_depth, cams[:6])
    K_shift = K.copy()
    K_shift[0, 2] = 2.0                                     # the sphere's centre at the left edge
    d0 = sphere_depth(cams[0], K_shift)
    views["depth"][0], views["masks"][0], views["K"][0] = d0, d0 > 0, K_shift
    inside = look_at((0.03, 0.005, 0.0))                    # a camera inside every test volume: nodes behind it, nodes at z <= z_min
    views["TCO"][1] = inside
    views["depth"][1] = 0.02
    views["masks"][1] = 1
    bad = views["depth"][2].copy()
    bad[::3, ::5], bad[1::3, ::5], bad[2::3, 1::5], bad[::4, 2::5] = np.nan, np.inf, 0.0, -0.3
    views["depth"][2], views["masks"][2] = bad, 1           # the mask says object everywhere: the depth rules decide
    views["K"][3, 0, 0] = np.nan
    views["TCO"][4, 1, 3] = np.inf
    return views


def plane_volume(g: Grid = ODD_GRID, color=True) -> np.ndarray:
    """a field set directly: a tilted plane through the volume with zeros exactly on nodes, counts 1 .. 3, a block of unobserved nodes,
    colours on part of the nodes"""
    nx, ny, nz = g.dims
    vol = new_volume(g.dims, color)
    kk, jj, ii = np.mgrid[0:nz, 0:ny, 0:nx]
    cnt = (1 + (ii + jj + kk) % 3).astype(np.int32)
    f = (0.25 * ii + 0.5 * jj - 2.0 * kk + 1.0).astype(F)          # zero on nodes with i + 2 j - 8 k + 4 = 0
    cnt[2:4, 3:6, 10:14] = 0
    vol[0] = f * cnt.astype(F)
    vol[1] = cnt.view(F)
    if color:
        cc = ((ii + 2 * jj) % 4).astype(np.int32)
        for c in range(3):
            vol[2 + c] = ((37 * ii + 11 * jj + 5 * kk + 60 * c) % 256).astype(F) * cc.astype(F)
        vol[5] = cc.view(F)
    return vol


def corner_volume() -> Tuple[np.ndarray, Grid]:
    """the worked example: 2 x 2 x 2 nodes, node 0 inside (f = -1), the others outside (f = +1)"""
    g = Grid((0.0, 0.0, 0.0), 1.0, (2, 2, 2))
    vol = new_volume(g.dims, False)
    vol[0] = 1.0
    vol[0, 0, 0, 0] = -1.0
    vol[1] = np.ones((2, 2, 2), np.int32).view(F)
    return vol, g


CORNER_VERTICES = [[.5, 0, 0], [0, .5, 0], [0, 0, .5], [.5, .5, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, .5]]
CORNER_FACES = [[0, 3, 6], [0, 6, 5], [1, 6, 3], [1, 4, 6], [2, 5, 6], [2, 6, 4]]

FIXTURES = ("sphere", "torus", "odd", "awkward", "many", "tiny")


def fixture(name: str) -> Tuple[Grid, Dict[str, np.ndarray]]:
    if name == "sphere":
        return cube_grid(), sphere_views()
    if name == "torus":
        return TORUS_GRID, torus_views()
    if name == "odd":                                        # the sphere's views into 33 x 17 x 9: the surface leaves the volume
        return ODD_GRID, sphere_views()
    if name == "awkward":
        return cube_grid(24), awkward_views()
    if name == "many":                                       # 48^3 = 110 592 nodes: 432 workgroups of 256, two rounds of the scan over them
        return cube_grid(48), many_views()
    if name == "tiny":
        return TINY_GRID, sphere_views()
    raise ValueError(name)


def without(views, *names):
    return {k: (None if k in names else v) for k, v in views.items()}


def icosphere(radius=SPHERE_R, subdivisions=3) -> Tuple[np.ndarray, np.ndarray]:
    """vertices [V,3] float64 on the sphere, faces [T,3] int32 wound outwards (642 vertices at 3 subdivisions)"""
    p = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(q, np.float64) / np.linalg.norm(q) for q in v]
    for _ in range(subdivisions):
        mid: Dict[Tuple[int, int], int] = {}

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                q = v[a] + v[b]
                v.append(q / np.linalg.norm(q))
                mid[key] = len(v) - 1
            return mid[key]

        f = [t for a, b, c in f for t in ((a, m(a, b), m(c, a)), (b, m(b, c), m(a, b)), (c, m(c, a), m(b, c)), (m(a, b), m(b, c), m(c, a)))]
    return np.asarray(v) * radius, np.asarray(f, np.int32)
