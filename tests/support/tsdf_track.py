"""TEST SUPPORT: ctypes wrapper of the host emulation of the camera-tracking kernels (tests/tsdf_track_emul.cpp), built on first use; an
independent numpy restatement of the contract written from its text and not from csrc/tsdf_track_core.h (float32 numpy operations one
by one for the per-pixel terms, whole frames at a time; the butterfly by index arithmetic; the solve in Python floats); and the fixtures
the CPU contract test and the GPU test share (the union of three spheres seen from a wobbling orbit, the same views cropped, the analytic
sphere, views that leave the volume, awkward frames, one pixel)."""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Dict, Optional

import numpy as np

from . import tsdf as st
from .emul import CSRC, TESTS, _p, build
from .tsdf import Grid, emul_integrate, new_volume  # noqa: F401

F = np.float32
GROUP, BLOCK, SUMS, RECORD, ROW = 1024, 256, 29, 32, 11
MIN_PIXELS = 64
EPS_ROT = 1e-5


def load():
    lib = build("tsdf_track_emul", [TESTS / "tsdf_track_emul.cpp", CSRC / "tsdf_track_core.h", CSRC / "tsdf_core.h"], fma=False)
    for name in ("tsdf_track_emul", "tsdf_track_rows_emul", "tsdf_track_groups_emul"):
        getattr(lib, name).restype = C.c_int
    lib.tsdf_track_emul_limits.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_longlong * 6)()
    load().tsdf_track_emul_limits(v)
    return dict(group_pixels=int(v[0]), block=int(v[1]), sums=int(v[2]), record=int(v[3]), max_iters=int(v[4]), max_frames=int(v[5]))


def groups(h: int, w: int) -> int:
    return int(load().tsdf_track_groups_emul(C.c_int(h), C.c_int(w)))


def eps_trans(g: Grid) -> float:
    return float(F(1e-3) * F(g.voxel))


class Tracked(dict):
    """TCO [n,16] f32, status [n] i32, used [n] i32, rms [n] f32, records [n,groups,32] f64, rc"""
    __getattr__ = dict.__getitem__


def new_outputs(n: int, h: int, w: int) -> Tracked:
    return Tracked(TCO=np.full((n, 16), -7, F), status=np.full(n, -7, np.int32), used=np.full(n, -7, np.int32), rms=np.full(n, -7, F),
                   records=np.full((n, max(groups(h, w), 0), RECORD), -7.0, np.float64), rc=None)


def emul_track(vol: np.ndarray, g: Grid, depth, masks, K, TCO, iters=10, min_views=1, min_pixels=MIN_PIXELS, mu=None, eps_rot=EPS_ROT,
               eps_tr=None, out: Optional[Tracked] = None) -> Tracked:
    depth = np.ascontiguousarray(depth, F)
    masks = None if masks is None else np.ascontiguousarray(masks, np.uint8)
    K = np.ascontiguousarray(K, F).reshape(-1, 9)
    TCO = np.ascontiguousarray(TCO, F).reshape(-1, 16)
    n, h, w = depth.shape
    out = new_outputs(n, h, w) if out is None else out
    nx, ny, nz = g.dims
    assert vol.flags.c_contiguous and vol.dtype == F
    out["rc"] = load().tsdf_track_emul(
        _p(vol), C.c_int(nx), C.c_int(ny), C.c_int(nz), C.c_int(int(vol.shape[0] == 6)), *(C.c_float(o) for o in g.origin), C.c_float(g.voxel),
        _p(depth), _p(masks), _p(K), _p(TCO), C.c_int(n), C.c_int(h), C.c_int(w), C.c_float(g.mu3 if mu is None else mu), C.c_int(min_views),
        C.c_int(min_pixels), C.c_int(iters), C.c_float(eps_rot), C.c_float(eps_trans(g) if eps_tr is None else eps_tr), _p(out["TCO"]),
        _p(out["status"]), _p(out["used"]), _p(out["rms"]), _p(out["records"]), C.c_longlong(out["records"].shape[0] * out["records"].shape[1]))
    return out


def emul_rows(vol: np.ndarray, g: Grid, depth, mask, K, TCO, min_views=1, mu=None):
    """one frame -> used [h*w] bool, rows [h*w, 11] f32 (zeros where not used), or None for a non-finite view"""
    depth = np.ascontiguousarray(depth, F)
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    K, TCO = np.ascontiguousarray(K, F).reshape(9), np.ascontiguousarray(TCO, F).reshape(16)
    h, w = depth.shape
    used, rows = np.zeros(h * w, np.uint8), np.zeros((h * w, ROW), F)
    nx, ny, nz = g.dims
    rc = load().tsdf_track_rows_emul(_p(vol), C.c_int(nx), C.c_int(ny), C.c_int(nz), *(C.c_float(o) for o in g.origin), C.c_float(g.voxel), _p(depth),
                                     _p(mask), _p(K), _p(TCO), C.c_int(h), C.c_int(w), C.c_float(g.mu3 if mu is None else mu), C.c_int(min_views),
                                     _p(used), _p(rows))
    if rc == 2:
        return None
    assert rc == 0
    return used.astype(bool), rows


# the restatement ----------------------------------------------------------------------------------------------------------------------
def _lerp(a, b, t):
    return a + t * (b - a)


def restated_rows(vol: np.ndarray, g: Grid, depth, mask, K, TCO, min_views=1, mu=None):
    """the contract's steps 1 .. 8 on a whole frame at once -> used [h*w] bool, rows [h*w, 11] f32 (f, g, r, J; zeros where not used)"""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    K, T = np.asarray(K, F).reshape(9), np.asarray(TCO, F).reshape(16)
    mu = F(g.mu3 if mu is None else mu)
    nx, ny, nz = g.dims
    vox = F(g.voxel)
    cnt = vol[1].view(np.int32).reshape(-1)
    fsum = vol[0].reshape(-1)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        d = depth
        use = np.isfinite(d) & (d > 0)
        if mask is not None:
            use &= np.asarray(mask) != 0
        pc = [(((xs.astype(F) + F(0.5)) - K[2]) / K[0]) * d, (((ys.astype(F) + F(0.5)) - K[5]) / K[4]) * d, d]
        e = [pc[c] - T[4 * c + 3] for c in range(3)]
        p = [(T[0 + c] * e[0] + T[4 + c] * e[1]) + T[8 + c] * e[2] for c in range(3)]
        q = [(p[c] - F(g.origin[c])) / vox for c in range(3)]
        i0 = [np.floor(v) for v in q]
        for c, dim in enumerate((nx, ny, nz)):
            use &= (i0[c] >= 0) & (i0[c] < F(dim - 1))
        u = [q[c] - i0[c] for c in range(3)]
        ii = [np.where(use, v, 0).astype(np.int64) for v in i0]
        Fc = []
        for code in range(8):
            at = ((ii[2] + ((code >> 2) & 1)) * ny + ii[1] + ((code >> 1) & 1)) * nx + ii[0] + (code & 1)
            use &= cnt[at] >= min_views
            Fc.append(fsum[at] / cnt[at].astype(F))
        c00, c10, c01, c11 = _lerp(Fc[0], Fc[1], u[0]), _lerp(Fc[2], Fc[3], u[0]), _lerp(Fc[4], Fc[5], u[0]), _lerp(Fc[6], Fc[7], u[0])
        c0, c1 = _lerp(c00, c10, u[1]), _lerp(c01, c11, u[1])
        f = _lerp(c0, c1, u[2])
        use &= np.abs(f) < F(1)
        dx = _lerp(_lerp(Fc[1] - Fc[0], Fc[3] - Fc[2], u[1]), _lerp(Fc[5] - Fc[4], Fc[7] - Fc[6], u[1]), u[2])
        dy = _lerp(c10 - c00, c11 - c01, u[2])
        dz = c1 - c0
        gr = [dx / vox, dy / vox, dz / vox]
        gm = [v * mu for v in gr]
        J = [p[1] * gm[2] - p[2] * gm[1], p[2] * gm[0] - p[0] * gm[2], p[0] * gm[1] - p[1] * gm[0]] + gm
        rows = np.stack([f, *gr, f * mu, *J], -1).astype(F)
    assert all(v.dtype == F for v in (f, dx, *J))
    use = use.reshape(-1)
    rows = rows.reshape(-1, ROW)
    rows[~use] = 0
    return use, rows


def restated_records(used: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """[groups, 32] float64: lane, butterfly, waves, as the contract orders them"""
    hw = len(used)
    n_groups = -(-hw // GROUP)
    J = rows[:, 5:11].astype(np.float64)
    r = rows[:, 4].astype(np.float64)
    rec = np.zeros((n_groups * GROUP, SUMS))
    cols = [J[:, i] * J[:, j] for i in range(6) for j in range(i, 6)] + [J[:, i] * r for i in range(6)] + [r * r, np.ones(hw)]
    rec[:hw] = np.where(used[:, None], np.stack(cols, 1), 0.0)
    per = rec.reshape(n_groups, GROUP // BLOCK, BLOCK, SUMS)
    lane = np.zeros((n_groups, BLOCK, SUMS))
    for q in range(GROUP // BLOCK):
        lane = lane + per[:, q]
    wave = lane.reshape(n_groups, BLOCK // 64, 64, SUMS)
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        wave = wave + wave[:, :, idx ^ off]
    out = np.zeros((n_groups, RECORD))
    s = np.zeros((n_groups, SUMS))
    for wv in range(BLOCK // 64):
        s = s + wave[:, wv, 0]
    out[:, :SUMS] = s
    return out


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def restated_solve(S, T, min_pixels, eps_rot, eps_tr):
    """the solve in Python floats (IEEE doubles, one rounding an operation) -> status, pose [12] f32 or None, used, rms"""
    S = [float(v) for v in S]
    T = [float(v) for v in np.asarray(T, F)[:12]]
    cnt = S[28]
    used = int(cnt)
    rms = F(math.sqrt(S[27] / cnt)) if used > 0 else F(0)
    if used < min_pixels:
        return -1, None, used, rms
    A = [[0.0] * 6 for _ in range(6)]
    at = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = S[at]
            at += 1
    damp = 1e-9 * cnt
    for i in range(6):
        A[i][i] = A[i][i] + damp
    b = S[21:27]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not d > 0.0:
            return -1, None, used, rms
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y, z = [0.0] * 6, [0.0] * 6
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * z[k]
        z[i] = s / L[i][i]
    w, v = [-z[0], -z[1], -z[2]], [-z[3], -z[4], -z[5]]
    a = [w[0] * 0.5, w[1] * 0.5, w[2] * 0.5]
    aa = _dot(a, a)
    s1, c1 = 1.0 + aa, 1.0 - aa
    skew = [[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]]
    Rc = [[(c1 + 2.0 * (a[i] * a[i])) / s1 if i == j else (2.0 * (a[i] * a[j]) + 2.0 * skew[i][j]) / s1 for j in range(3)] for i in range(3)]
    R = [[T[4 * i + j] for j in range(3)] for i in range(3)]
    t = [T[4 * i + 3] for i in range(3)]
    Rn = [[_dot(R[i], Rc[j]) for j in range(3)] for i in range(3)]
    m = [(Rc[0][k] * v[0] + Rc[1][k] * v[1]) + Rc[2][k] * v[2] for k in range(3)]
    tn = [t[i] - _dot(R[i], m) for i in range(3)]
    try:
        n0 = math.sqrt(_dot(Rn[0], Rn[0]))
        r0 = [Rn[0][k] / n0 for k in range(3)]
        pr = _dot(Rn[1], r0)
        e = [Rn[1][k] - pr * r0[k] for k in range(3)]
        n1 = math.sqrt(_dot(e, e))
        r1 = [e[k] / n1 for k in range(3)]
    except (ZeroDivisionError, ValueError):
        return -1, None, used, rms
    r2 = [r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]]
    with np.errstate(all="ignore"):
        pose = np.array([*r0, tn[0], *r1, tn[1], *r2, tn[2]], np.float64).astype(F)
    if not np.isfinite(pose).all():
        return -1, None, used, rms
    conv = math.sqrt(_dot(w, w)) < float(F(eps_rot)) and math.sqrt(_dot(v, v)) < float(F(eps_tr))
    return (1 if conv else 0), pose, used, rms


def restated_track(vol, g: Grid, depth, masks, K, TCO, iters=10, min_views=1, min_pixels=MIN_PIXELS, mu=None, eps_rot=EPS_ROT, eps_tr=None) -> Tracked:
    depth = np.asarray(depth, F)
    K, TCO = np.asarray(K, F).reshape(-1, 9), np.asarray(TCO, F).reshape(-1, 16)
    n, h, w = depth.shape
    out = new_outputs(n, h, w)
    eps_tr = eps_trans(g) if eps_tr is None else eps_tr
    for v in range(n):
        out["TCO"][v] = TCO[v]
        out["used"][v], out["rms"][v] = 0, 0
        if not (np.isfinite(K[v]).all() and np.isfinite(TCO[v, :12]).all()):
            out["status"][v] = -2
            continue
        out["status"][v] = 0
        for _ in range(iters):
            use, rows = restated_rows(vol, g, depth[v], None if masks is None else masks[v], K[v], out["TCO"][v], min_views, mu)
            out["records"][v] = restated_records(use, rows)
            S = np.zeros(RECORD)
            for G in range(out["records"].shape[1]):
                S = S + out["records"][v, G]
            status, pose, used, rms = restated_solve(S, out["TCO"][v], min_pixels, eps_rot, eps_tr)
            out["status"][v], out["used"][v], out["rms"][v] = status, used, rms
            if status == -1:
                out["TCO"][v] = TCO[v]
            else:
                out["TCO"][v, :12] = pose
            if status != 0:
                break
    out["rc"] = 0
    return out


# fixtures -----------------------------------------------------------------------------------------------------------------------------
TRIO_CENTRES = np.array([[0.02, 0.0, 0.0], [-0.02, 0.012, 0.005], [0.0, -0.02, 0.022]])
TRIO_RADII = (0.03, 0.025, 0.02)
N_ORBIT = 24
PROBE_R = 0.05


def orbit_cameras(n=N_ORBIT, dist=0.4) -> np.ndarray:
    """TCO [n,4,4] float64 on the wobbling orbit: azimuth 2 pi k / n, elevation 0.5 + 0.3 sin(2 azimuth) rad, looking at the origin"""
    cams = []
    for k in range(n):
        az = 2.0 * np.pi * k / n
        el = 0.5 + 0.3 * np.sin(2.0 * az)
        cams.append(st.look_at(dist * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])))
    return np.stack(cams)


def trio_depth(TCO, K, h=st.H, w=st.W) -> np.ndarray:
    """exact depth of the union of the three spheres at pixel centres, float64; 0 where the ray misses"""
    best = np.full((h, w), np.inf)
    for c, r in zip(TRIO_CENTRES, TRIO_RADII):
        T = TCO.copy()
        T[:3, 3] = TCO[:3, :3] @ c + TCO[:3, 3]
        d = st.sphere_depth(T, K, r=r, h=h, w=w)
        best = np.where(d > 0, np.minimum(best, d), best)
    return np.where(np.isfinite(best), best, 0.0)


def perturbation(seed: int, deg: float, mm: float) -> np.ndarray:
    """[4,4] float64: a rotation of `deg` about a seeded axis and a translation of `mm` along a seeded direction, in the object's frame"""
    rs = np.random.RandomState(seed)
    ax, tr = rs.randn(3), rs.randn(3)
    ax, tr = ax / np.linalg.norm(ax), tr / np.linalg.norm(tr)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    P = np.eye(4)
    P[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    P[:3, 3] = tr * mm * 1e-3
    return P


def perturbed(cams: np.ndarray, deg=5.0, mm=5.0, seed0=100) -> np.ndarray:
    return np.stack([T @ perturbation(seed0 + k, deg, mm) for k, T in enumerate(cams)])


def displacement(T_true, T_est) -> float:
    """the largest distance between the images of the points of the sphere of radius PROBE_R under the two poses (metres)"""
    pts, _ = st.icosphere(PROBE_R, 3)
    A, B = np.asarray(T_true, np.float64).reshape(-1, 4)[:3], np.asarray(T_est, np.float64).reshape(-1, 4)[:3]
    return float(np.linalg.norm(pts @ (A[:, :3] - B[:, :3]).T + (A[:, 3] - B[:, 3]), axis=1).max())


def _trio_frames(h=st.H, w=st.W, K=None):
    cams = orbit_cameras()
    K = st.intrinsics() if K is None else K
    depth = np.stack([trio_depth(T, K, h, w) for T in cams]).astype(F)
    return dict(depth=depth, masks=(depth > 0).astype(np.uint8), K=np.repeat(K[None], len(cams), 0).astype(F), TCO=cams.astype(F), rgb=None)


@functools.lru_cache(None)
def trio_views():
    return _trio_frames()


@functools.lru_cache(None)
def fused(name: str):
    """the volume a fixture tracks against: its views fused at their true poses by the TSDF emulation (computed once, never written)"""
    g, views = {"trio": (st.cube_grid(32), trio_views()), "leaving": (st.ODD_GRID, trio_views()),
                "sphere": (st.cube_grid(32), st.without(st.sphere_views(), "rgb"))}[name]
    vol = new_volume(g.dims, False)
    assert emul_integrate(vol, g, views) == 0
    vol.setflags(write=False)
    return g, vol


FIXTURES = ("trio", "cropped", "sphere", "leaving", "awkward", "pixel")


@functools.lru_cache(None)
def fixture(name: str):
    """-> grid, volume, frames: depth [n,h,w], masks [n,h,w], K [n,9], TCO_true [n,16] (what the frames were made from), TCO [n,16] (where
    tracking starts)"""
    def pack(g, vol, depth, masks, K, true, start):
        fr = dict(depth=np.array(depth, F), masks=np.array(masks, np.uint8), K=np.array(K, F).reshape(-1, 9),          # copies: made read-only below
                  TCO_true=np.array(true, F).reshape(-1, 16), TCO=np.array(start, F).reshape(-1, 16))
        for a in fr.values():
            a.setflags(write=False)
        return g, vol, fr

    tv = trio_views()
    cams = orbit_cameras()
    if name in ("trio", "leaving"):                          # leaving: most samples fall outside 33 x 17 x 9 or on incomplete cells
        g, vol = fused(name)
        return pack(g, vol, tv["depth"], tv["masks"], tv["K"], cams, perturbed(cams))
    if name == "cropped":                                    # 53 x 37 = 1961 pixels: a partial last group
        g, vol = fused("trio")
        K = tv["K"].copy()
        K[:, 0, 2] -= 5
        K[:, 1, 2] -= 6
        return pack(g, vol, tv["depth"][:, 6:43, 5:58], tv["masks"][:, 6:43, 5:58], K, cams, perturbed(cams))
    if name == "sphere":                                     # rotation is unobservable: the damping keeps the solve finite
        g, vol = fused("sphere")
        sv = st.sphere_views()
        true = sv["TCO"].astype(np.float64)
        start = true.copy()
        start[:, :3, 3] += np.array([0.003, -0.003, 0.0027])    # about 5 mm
        return pack(g, vol, sv["depth"], sv["masks"], sv["K"], true, start)
    if name == "awkward":
        g, vol = fused("trio")
        depth, masks, K = tv["depth"][:6].copy(), tv["masks"][:6].copy(), tv["K"][:6].copy()
        true, start = cams[:6].copy(), perturbed(cams)[:6].copy()
        bad = depth[0]
        bad[::3, ::5], bad[1::3, ::5], bad[2::3, 1::5], bad[::4, 2::5] = np.nan, np.inf, 0.0, -0.3
        masks[0] = 1                                         # the mask says object everywhere: the depth rules decide
        masks[1] = 0                                         # nothing to align: lost, the pose returned bit for bit
        K[2, 1, 1] = np.nan
        start[3, 1, 3] = np.inf
        start[4] = true[4] = st.look_at((0.03, 0.005, 0.0))  # a camera inside the volume
        depth[4], masks[4] = 0.02, 1
        return pack(g, vol, depth, masks, K, true, start)
    if name == "pixel":                                      # a frame of 1 x 1
        g, vol = fused("trio")
        K = np.array([[200.0, 0, 0.5], [0, 200.0, 0.5], [0, 0, 1]])
        depth = np.stack([trio_depth(T, K, 1, 1) for T in cams[:3]])
        return pack(g, vol, depth, depth > 0, np.repeat(K[None], 3, 0), cams[:3], cams[:3])
    raise ValueError(name)
