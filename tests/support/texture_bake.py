"""TEST SUPPORT: ctypes wrapper of the host emulation of the texture-atlas kernels (tests/texture_bake_emul.cpp), built on first use; an
independent numpy restatement of the contract written from its text and not from csrc/texture_bake_core.h (numpy operations one by
one on the whole atlas at a time, in float32 to be compared byte for byte, or in float64 to measure what the arithmetic itself costs);
an integer restatement of the four taps the rasteriser's tex_sample reads at level 0; and the fixtures the CPU tests and the GPU test
share (the icosphere under the sphere's views, single triangles, broken meshes, a checkered sphere rendered analytically)."""
from __future__ import annotations

import ctypes as C
import functools
from typing import Dict, Optional, Tuple

import numpy as np

from .emul import CSRC, TESTS, _p, build
from .tsdf import (SPHERE_R, Z_MIN, _rays, awkward_views, corner_cameras, icosphere, intrinsics, look_at, many_views, sphere_depth,  # noqa: F401
                   sphere_views, torus_views)

F = np.float32
BLOCKS = (64, 32, 16, 8, 4)
DEPTH_TOL = 2e-3          # the tests' tolerance: the icosphere's faces lie within 0.2 mm of the sphere the depth was traced from
COS_MIN = 0.2


def load():
    lib = build("texture_bake_emul", [TESTS / "texture_bake_emul.cpp", CSRC / "texture_bake_core.h", CSRC / "tsdf_core.h"], fma=False)
    for name in ("texture_atlas_block_emul", "texture_atlas_uvs_emul", "texture_bake_emul"):
        getattr(lib, name).restype = C.c_int
    lib.texture_bake_emul_limits.restype = None
    return lib


def emul_block(T: int, S: int) -> int:
    return int(load().texture_atlas_block_emul(C.c_longlong(T), C.c_int(S)))


def emul_uvs(T: int, S: int) -> np.ndarray:
    uvs = np.full((T, 3, 2), -7, F)
    assert load().texture_atlas_uvs_emul(C.c_int(T), C.c_int(S), _p(uvs)) == 0
    return uvs


def bake_arrays(vertices, faces, views, colors=None, sel=slice(None), masks=True):
    """the arrays of a bake as the C ABI takes them"""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    c = None if colors is None else np.ascontiguousarray(colors, F).reshape(-1, 3)
    depth = np.ascontiguousarray(views["depth"][sel], F)
    m = np.ascontiguousarray(views["masks"][sel], np.uint8) if masks and views.get("masks") is not None else None
    rgb = np.ascontiguousarray(views["rgb"][sel], np.uint8)
    K = np.ascontiguousarray(views["K"][sel], F).reshape(-1, 9)
    TCO = np.ascontiguousarray(views["TCO"][sel], F).reshape(len(K), int(np.prod(views["TCO"].shape[1:])))
    return v, f, c, depth, m, rgb, K, TCO


def emul_bake(vertices, faces, views, S, colors=None, sel=slice(None), masks=True, depth_tol=DEPTH_TOL, cos_min=COS_MIN, z_min=Z_MIN,
              best_view=False) -> Tuple[np.ndarray, np.ndarray]:
    """-> texels uint8 [S,S,4], seen uint8 [S,S]"""
    v, f, c, depth, m, rgb, K, TCO = bake_arrays(vertices, faces, views, colors, sel, masks)
    n, h, w = depth.shape
    texels, seen = np.full((S, S, 4), 0xA5, np.uint8), np.full((S, S), 0xA5, np.uint8)
    rc = load().texture_bake_emul(_p(v), C.c_int(len(v)), _p(f), C.c_int(len(f)), _p(c), _p(depth), _p(m), _p(rgb), _p(K), _p(TCO),
                                  C.c_int(TCO.shape[1] if n else 16), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(S), C.c_float(depth_tol),
                                  C.c_float(cos_min), C.c_float(z_min), C.c_int(int(best_view)), _p(texels), _p(seen))
    assert rc == 0
    return texels, seen


# the restatement ----------------------------------------------------------------------------------------------------------------------
def restated_block(T: int, S: int) -> int:
    for B in BLOCKS:
        if T >= 1 and S % B == 0 and -(-T // 2) <= (S // B) ** 2:
            return B
    return 0


def chart_texels(T: int, S: int):
    """per texel of the atlas ([S,S], row j, column i): its triangle (-1: none), whether it is of the upper chart, its local (i, j)"""
    B = restated_block(T, S)
    gj, gi = np.mgrid[0:S, 0:S]
    i, j = gi % B, gj % B
    upper = (i + j) > B - 1
    t = 2 * ((gj // B) * (S // B) + gi // B) + upper
    return B, np.where(t < T, t, -1), upper, i, j


def restated_uvs(T: int, S: int) -> np.ndarray:
    B = restated_block(T, S)
    c = B - 3
    uvs = np.zeros((T, 3, 2), F)
    for t in range(T):
        X, Y = ((t // 2) % (S // B)) * B, ((t // 2) // (S // B)) * B
        lower = [(0, 0), (c, 0), (0, c)]
        for k, (di, dj) in enumerate(lower):
            i, j = (B - 1 - di, B - 1 - dj) if t % 2 else (di, dj)
            uvs[t, k] = (F(X + i) + F(0.5)) / F(S), (F(Y + j) + F(0.5)) / F(S)
    return uvs


def chart_coordinates(T: int, S: int, dt=F):
    """a, b per texel [S,S] as the contract states them"""
    B, t, upper, i, j = chart_texels(T, S)
    c = dt(B - 3)
    a = np.where(upper, B - 1 - i, i).astype(dt) / c
    b = np.where(upper, B - 1 - j, j).astype(dt) / c
    a, b = np.maximum(a, dt(0)), np.maximum(b, dt(0))
    s = a + b
    over = s > 1
    with np.errstate(all="ignore"):
        a, b = np.where(over, a / s, a), np.where(over, b / s, b)
    return t, a.astype(dt), b.astype(dt)


def _q255(v):
    return np.floor(np.fmin(np.fmax(v, 0), 255) + v.dtype.type(0.5)).astype(np.uint8)


def restated_bake(vertices, faces, views, S, colors=None, sel=slice(None), masks=True, depth_tol=DEPTH_TOL, cos_min=COS_MIN, z_min=Z_MIN,
                  best_view=False, dt=F, details=False):
    """the contract on the whole atlas at once -> texels uint8 [S,S,4], seen uint8 [S,S] (details: also t, the surface points and the
    unquantised colours)"""
    v, f, cols, depth, m, rgb, K, TCO = bake_arrays(vertices, faces, views, colors, sel, masks)
    v, K, TCO, depth = v.astype(dt), K.astype(dt), TCO.astype(dt), depth.astype(dt)
    depth_tol, cos_min, z_min = dt(depth_tol), dt(cos_min), dt(z_min)
    n, h, w = depth.shape
    T, V = len(f), len(v)
    t, a, b = chart_coordinates(T, S, dt)
    present = t >= 0
    idx = f[np.where(present, t, 0)]                                    # [S,S,3]
    indexed = present & ((idx >= 0) & (idx < V)).all(-1)
    idx = np.where(indexed[..., None], idx, 0)
    with np.errstate(all="ignore"):
        if V:
            v0, v1, v2 = v[idx[..., 0]], v[idx[..., 1]], v[idx[..., 2]]
        else:
            v0 = v1 = v2 = np.zeros((S, S, 3), dt)
        visits = indexed & np.isfinite(v0).all(-1) & np.isfinite(v1).all(-1) & np.isfinite(v2).all(-1)
        e1, e2 = v1 - v0, v2 - v0
        p = [(v0[..., k] + a * e1[..., k]) + b * e2[..., k] for k in range(3)]
        nrm = [(e1[..., (k + 1) % 3] * e2[..., (k + 2) % 3]) - (e1[..., (k + 2) % 3] * e2[..., (k + 1) % 3]) for k in range(3)]
        nn = (nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]
        cm2 = cos_min * cos_min
        acc = [np.zeros((S, S), dt) for _ in range(3)]
        wsum = np.zeros((S, S), dt)
        seen = np.zeros((S, S), np.int64)
        for q in range(n):
            if not (np.isfinite(K[q]).all() and np.isfinite(TCO[q, :12]).all()):
                continue
            R = TCO[q]
            fx, cx, fy, cy = K[q, 0], K[q, 2], K[q, 4], K[q, 5]
            cam = [((R[4 * r + 0] * p[0] + R[4 * r + 1] * p[1]) + R[4 * r + 2] * p[2]) + R[4 * r + 3] for r in range(3)]
            assert all(c.dtype == dt for c in cam)
            ok = visits & (cam[2] > z_min)
            xf = (fx * cam[0]) / cam[2] + cx
            yf = (fy * cam[1]) / cam[2] + cy
            xn, yn = np.floor(xf), np.floor(yf)
            ok = ok & (xn >= 0) & (xn < dt(w)) & (yn >= 0) & (yn < dt(h))
            rn = [(R[4 * r + 0] * nrm[0] + R[4 * r + 1] * nrm[1]) + R[4 * r + 2] * nrm[2] for r in range(3)]
            g = -((rn[0] * cam[0] + rn[1] * cam[1]) + rn[2] * cam[2])
            pp = (cam[0] * cam[0] + cam[1] * cam[1]) + cam[2] * cam[2]
            den = nn * pp
            gg = g * g
            ok = ok & (g > 0) & (gg > cm2 * den)
            wgt = gg / den

            def tap(x, y):
                """x, y integer arrays -> passes, colour [3] as dt"""
                inside = ok & (x >= 0) & (x < w) & (y >= 0) & (y < h)
                xi, yi = np.where(inside, x, 0), np.where(inside, y, 0)
                d = depth[q][yi, xi]
                passes = inside & np.isfinite(d) & (d > 0) & (np.abs(d - cam[2]) <= depth_tol)
                if m is not None:
                    passes = passes & (m[q][yi, xi] != 0)
                return passes, [rgb[q][yi, xi, k].astype(dt) for k in range(3)]

            tx, ty = xf - dt(0.5), yf - dt(0.5)
            fxx, fyy = np.floor(tx), np.floor(ty)
            ax, ay = tx - fxx, ty - fyy
            x0, y0 = np.where(ok, fxx, 0).astype(np.int64), np.where(ok, fyy, 0).astype(np.int64)
            (k00, c00), (k01, c01), (k10, c10), (k11, c11) = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
            all4 = k00 & k01 & k10 & k11
            kn, cn = tap(np.where(ok, xn, 0).astype(np.int64), np.where(ok, yn, 0).astype(np.int64))
            hit = all4 | (ok & kn)
            for k in range(3):
                top = c00[k] + ax * (c01[k] - c00[k])
                bot = c10[k] + ax * (c11[k] - c10[k])
                col = np.where(all4, top + ay * (bot - top), cn[k])
                if best_view:
                    better = hit & ((seen == 0) | (wgt > wsum))
                    acc[k] = np.where(better, col, acc[k])
                else:
                    acc[k] = np.where(hit, acc[k] + wgt * col, acc[k])
            if best_view:
                wsum = np.where(hit & ((seen == 0) | (wgt > wsum)), wgt, wsum)
            else:
                wsum = np.where(hit, wsum + wgt, wsum)
            seen += hit
        w0 = (dt(1) - a) - b
        out = np.zeros((S, S, 4), np.uint8)
        raw = np.zeros((S, S, 3), dt)
        for k in range(3):
            if cols is not None:
                cc = [np.where(indexed, cols.astype(dt)[idx[..., r], k], dt(1)) for r in range(3)]
            else:
                cc = [np.ones((S, S), dt)] * 3
            fallback = (((w0 * cc[0]) + a * cc[1]) + b * cc[2]) * dt(255)
            raw[..., k] = np.where(seen > 0, acc[k] if best_view else acc[k] / wsum, fallback)
            out[..., k] = np.where(present, _q255(raw[..., k]), 0)
    out[..., 3] = np.where(present, 255, 0)
    seen8 = np.minimum(seen, 255).astype(np.uint8)
    if details:
        return out, seen8, dict(t=t, p=np.stack(p, -1), raw=raw, a=a, b=b)
    return out, seen8


# the rasteriser's level-0 taps, restated on integers -------------------------------------------------------------------------------------
def level0_taps(u, v, S):
    """the four texels tex_sample (csrc/raster_core.h) reads at level 0 of an S x S texture for float32 u, v, and their bilinear weights:
    -> x [N,4], y [N,4] integers, weight [N,4] float64.  fmaf(u - floor(u), S, -0.5) as one rounding."""
    u, v = np.asarray(u, F), np.asarray(v, F)
    fu = ((u - np.floor(u)).astype(np.float64) * S - 0.5).astype(F)
    fv = ((v - np.floor(v)).astype(np.float64) * S - 0.5).astype(F)
    flu, flv = np.floor(fu), np.floor(fv)
    au, av = (fu - flu).astype(np.float64), (fv - flv).astype(np.float64)
    x0, y0 = flu.astype(np.int64), flv.astype(np.int64)
    x0, y0 = np.where(x0 < 0, S - 1, np.minimum(x0, S - 1)), np.where(y0 < 0, S - 1, np.minimum(y0, S - 1))
    x1, y1 = np.where(x0 + 1 == S, 0, x0 + 1), np.where(y0 + 1 == S, 0, y0 + 1)
    x = np.stack([x0, x1, x0, x1], 1)
    y = np.stack([y0, y0, y1, y1], 1)
    wgt = np.stack([(1 - au) * (1 - av), au * (1 - av), (1 - au) * av, au * av], 1)
    return x, y, wgt


# fixtures -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def ico_mesh(subdivisions=3):
    """vertices float32, faces int32, vertex colours float32 in 0 .. 1 (a smooth function of the position that no view's colour equals)"""
    v, f = icosphere(subdivisions=subdivisions)
    v = v.astype(F)
    colors = np.clip(0.5 + 8.0 * v[:, [2, 0, 1]].astype(np.float64), 0, 1).astype(F)
    return v, f, colors


def analytic_rgb(p) -> np.ndarray:
    """the colour `_surface_rgb` of tests/support/tsdf.py paints at the object-frame point p [.., 3], before it is cut to a byte"""
    return np.clip(128.0 + 2000.0 * np.asarray(p, np.float64), 0, 255)


def single_triangles(T: int):
    """T triangles on the sphere facing camera 0 of the sphere's views: the first T faces of the icosphere sorted by how squarely
    they face it"""
    v, f, c = ico_mesh()
    cam = -sphere_views()["TCO"][0][:3, :3].T @ sphere_views()["TCO"][0][:3, 3]
    centre = v[f].mean(1)
    order = np.argsort(-(centre @ cam) / np.linalg.norm(centre, axis=1))
    return v, np.ascontiguousarray(f[order[:T]]), c


def one_pixel_views() -> Dict[str, np.ndarray]:
    """1 x 1 frames: three cameras whose only pixel looks at the sphere's centre"""
    K = np.array([[200.0, 0, 0.5], [0, 200.0, 0.5], [0, 0, 1]])
    cams = corner_cameras()[:3]
    depth = np.stack([sphere_depth(T, K, h=1, w=1) for T in cams])
    rgb = np.stack([np.full((1, 1, 3), 40 + 70 * q, np.uint8) for q in range(len(cams))])
    return dict(depth=depth.astype(F), masks=(depth > 0).astype(np.uint8), rgb=rgb, K=np.repeat(K[None], len(cams), 0).astype(F), TCO=cams.astype(F))


def broken_mesh():
    """the icosphere with a zero-area triangle (face 3: two corners alike), a NaN vertex (vertex of face 10), an infinite one (face 20) and
    face indices out of range (face 30: V, face 31: -1, face 32: 2^31 - 1) -> vertices, faces, colours, the faces that must bake unseen"""
    v, f, c = ico_mesh()
    v, f = v.copy(), f.copy()
    f[3, 2] = f[3, 1]
    v[f[10, 0], 1] = np.nan
    v[f[20, 2], 0] = np.inf
    f[30, 1], f[31, 0], f[32, 2] = len(v), -1, 2 ** 31 - 1
    bad_vertices = {int(f[10, 0]), int(f[20, 2])}
    unseen = [t for t in range(len(f)) if t in (3, 30, 31, 32) or bad_vertices & {int(q) for q in f[t]}]
    return v, f, c, np.asarray(unseen)


# the checkered sphere of the end-to-end test ----------------------------------------------------------------------------------------------
CHECK_PERIOD = 0.008
CHECK_H, CHECK_W, CHECK_F = 120, 160, 200.0


def checker_rgb(pts) -> np.ndarray:
    """a 3-D checker of CHECK_PERIOD: cells of half a period, dark or light by the parity of their integer coordinates, tinted by axis"""
    q = np.floor(np.asarray(pts, np.float64) / (CHECK_PERIOD / 2.0)).astype(np.int64)
    on = (q.sum(-1) % 2) == 0
    return np.where(on[..., None], np.array([230.0, 210.0, 60.0]), np.array([30.0, 60.0, 200.0]))


def checker_views(cams, K=None, h=CHECK_H, w=CHECK_W, supersample=3) -> Dict[str, np.ndarray]:
    """the sphere with the checker, rendered analytically: depth at pixel centres, colour the mean over supersample^2 rays a pixel"""
    K = intrinsics(CHECK_F, h, w) if K is None else K
    depth = np.stack([sphere_depth(T, K, h=h, w=w) for T in cams])
    rgb = np.zeros((len(cams), h, w, 3), np.float64)
    Ks = K.copy()
    Ks[:2] *= supersample
    for q, T in enumerate(cams):
        ds = sphere_depth(T, Ks, h=h * supersample, w=w * supersample)
        pts = (_rays(Ks, h * supersample, w * supersample) * ds[..., None] - T[:3, 3]) @ T[:3, :3]
        col = np.where((ds > 0)[..., None], checker_rgb(pts), 0.0)
        cnt = (ds > 0).reshape(h, supersample, w, supersample).sum((1, 3))
        rgb[q] = col.reshape(h, supersample, w, supersample, 3).sum((1, 3)) / np.maximum(cnt, 1)[..., None]
    rgb8 = np.clip(np.rint(rgb), 0, 255).astype(np.uint8)
    rgb8[depth <= 0] = 0
    return dict(depth=depth.astype(F), masks=(depth > 0).astype(np.uint8), rgb=rgb8, K=np.repeat(K[None], len(cams), 0).astype(F),
                TCO=np.asarray(cams).astype(F))


def checker_cameras(n=24, dist=0.3) -> np.ndarray:
    """n cameras on a spiral over the sphere of directions"""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    dirs = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    return np.stack([look_at(dist * d, up=(0, 0, 1) if abs(d[2]) < 0.9 else (0, 1, 0)) for d in dirs])
