"""TEST SUPPORT: ctypes wrapper of the host emulation of the TEASER++ refiner kernels (tests/teaser_emul.cpp), built on first use; an
independent numpy restatement of the algorithm stated in megapose6d_amd/csrc/teaser_core.h (fp32 where the contract is fp32: mask,
points, sampling, graph; float64 with numpy's own sums, SVD and sort for the registration), which the emulation and the kernels are
held against (teaserpp_python and pytorch3d are not dependencies); and the seeded fixtures the CPU contract test and the GPU test share.
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from typing import Dict, Optional, Tuple

import numpy as np

from .emul import CSRC, TESTS, _f32, _i32, _p, build

MASK_TYPES = {"simple": 0, "threshold": 1}
SELECTIONS = {"kcore": 0, "none": 1}
TIM_GRAPHS = {"chain": 0, "complete": 1}
NOISE_BOUND = 0.01
GRAPH_MARGIN = 1e-5   # metres: pairs whose |difference of the pair distances| is this close to 2 * noise_bound are left out of the float64 comparison
GRAPH_CAP = 0.01      # ... and they may be at most this share of a fixture's pairs (a cap, not a measurement)
# The emulation's [R t] against the float64 restatement, largest absolute difference of an entry over the fixtures of
# tests/test_teaser_contract_cpu.py::test_registration_tolerance_is_the_measured_one: measured 9.2e-15 (the two sides end the GNC loop
# on the same iteration; the difference is the eigenvector solve against numpy's SVD and the order of the sums), times the factor 4 of
# margin the other support modules use.
RT_TOL = 3.7e-14


def load():
    lib = build("teaser_emul", [TESTS / "teaser_emul.cpp", CSRC / "teaser_core.h"])
    for name in ("teaser_emul_fps", "teaser_emul_solve", "teaser_emul_refine", "teaser_emul_cores"):
        getattr(lib, name).restype = C.c_int
    lib.teaser_emul_limits.restype = None
    lib.teaser_emul_graph.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_int * 5)()
    load().teaser_emul_limits(v)
    return dict(threads=int(v[0]), max_points=int(v[1]), fps_resident=int(v[2]), gnc_max_iter=int(v[3]), info=int(v[4]))


# the emulation ---------------------------------------------------------------------------------------------------------------------------
def emul_fps(points, counts, n_points: int, use_fps: bool = True):
    """points [n,stride,3], counts [n] -> idx [n,n_points] int32 (-1 past M), M [n]"""
    p, c = _f32(points), _i32(counts)
    n, stride = p.shape[0], p.shape[1]
    idx, m = np.empty((n, n_points), np.int32), np.empty(n, np.int32)
    assert load().teaser_emul_fps(_p(p), _p(c), C.c_int(n), C.c_int(stride), C.c_int(n_points), C.c_int(int(use_fps)), _p(idx), _p(m)) == 0
    return idx, m


def emul_graph(src, dst, noise_bound: float = NOISE_BOUND) -> np.ndarray:
    s, d = _f32(src), _f32(dst)
    adj = np.empty((len(s), len(s)), np.uint8)
    load().teaser_emul_graph(_p(s), _p(d), C.c_int(len(s)), C.c_float(noise_bound), _p(adj))
    return adj


def emul_cores(adj) -> Tuple[np.ndarray, int]:
    a = np.ascontiguousarray(adj, np.uint8)
    core = np.zeros(len(a), np.int32)
    k = load().teaser_emul_cores(_p(a), C.c_int(len(a)), _p(core))
    return core, int(k)


def emul_solve(src, dst, counts, noise_bound: float = NOISE_BOUND, min_num_inliers: int = 0, inlier_selection: str = "kcore",
               rotation_tim_graph: str = "chain"):
    """src, dst [n,stride,3], counts [n] -> dict of Rt [n,3,4] float64, retval [n], degree, core, selected [n,stride], info [n,5]"""
    s, d, c = _f32(src), _f32(dst), _i32(counts)
    n, stride = s.shape[0], s.shape[1]
    out = dict(Rt=np.empty((n, 3, 4), np.float64), retval=np.empty(n, np.int32), degree=np.empty((n, stride), np.int32),
               core=np.empty((n, stride), np.int32), selected=np.empty((n, stride), np.int32), info=np.empty((n, 5), np.int32))
    rc = load().teaser_emul_solve(_p(s), _p(d), _p(c), C.c_int(n), C.c_int(stride), C.c_float(noise_bound), C.c_int(SELECTIONS[inlier_selection]),
                                  C.c_int(TIM_GRAPHS[rotation_tim_graph]), C.c_int(min_num_inliers), _p(out["Rt"]), _p(out["retval"]), _p(out["degree"]),
                                  _p(out["core"]), _p(out["selected"]), _p(out["info"]))
    assert rc == 0
    return out


def emul_refine(depth_meas, im_ids, depth_rend, K_rows, TCO, mask_type="simple", depth_delta_thresh=0.1, n_min_points=100, n_points=1000,
                noise_bound=NOISE_BOUND, min_num_inliers=50, use_farthest_point_sampling=True, inlier_selection="kcore", rotation_tim_graph="chain"):
    dm, dr, K, T, ids = _f32(depth_meas), _f32(depth_rend), _f32(K_rows), _f32(TCO), _i32(im_ids)
    n, (B, H, W) = len(T), dm.shape
    assert dr.shape == (n, H, W) and K.shape == (n, 3, 3) and T.shape == (n, 4, 4)
    out = dict(TCO=np.empty((n, 4, 4), np.float32), retval=np.empty(n, np.int32), Rt=np.empty((n, 3, 4), np.float64),
               sample_idx=np.empty((n, n_points), np.int32), degree=np.empty((n, n_points), np.int32), core=np.empty((n, n_points), np.int32),
               selected=np.empty((n, n_points), np.int32), info=np.empty((n, 5), np.int32))
    rc = load().teaser_emul_refine(_p(dm), C.c_int(B), _p(ids), _p(dr), _p(K), _p(T), C.c_int(n), C.c_int(H), C.c_int(W), C.c_int(MASK_TYPES[mask_type]),
                                   C.c_float(depth_delta_thresh), C.c_int(n_min_points), C.c_int(n_points), C.c_float(noise_bound), C.c_int(min_num_inliers),
                                   C.c_int(int(use_farthest_point_sampling)), C.c_int(SELECTIONS[inlier_selection]), C.c_int(TIM_GRAPHS[rotation_tim_graph]),
                                   _p(out["TCO"]), _p(out["retval"]), _p(out["Rt"]), _p(out["sample_idx"]), _p(out["degree"]), _p(out["core"]),
                                   _p(out["selected"]), _p(out["info"]))
    assert rc == 0
    return out


# the restatement ---------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 is exact in float64, and the one rounding of the sum to float64 before the rounding
    to fp32 changes the result only on a tie of the second rounding"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def dist2_f32(p, q):
    d = np.asarray(p, np.float32) - np.asarray(q, np.float32)
    return _fma32(d[..., 2], d[..., 2], _fma32(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))


def ref_fps(points, n_points: int) -> np.ndarray:
    """pytorch3d's sample_farthest_points (no random start) in plain numpy fp32 -> M = min(n_points, N) indices"""
    p = np.asarray(points, np.float32)
    N = len(p)
    M = min(n_points, N)
    idx = np.zeros(M, np.int64)
    mn = np.full(N, np.inf, np.float32)
    for k in range(1, M):
        mn = np.minimum(mn, dist2_f32(p, p[idx[k - 1]]))
        idx[k] = int(np.argmax(mn))          # the first of the largest
    return idx


def ref_stride(N: int, n_points: int) -> np.ndarray:
    M = min(n_points, N)
    return (np.arange(M, dtype=np.int64) * N) // M


def ref_mask(meas, rend, mask_type: str, thresh: float) -> np.ndarray:
    m = np.logical_and(meas > 0, rend > 0)
    if mask_type == "threshold":
        m = m & ~(np.abs(meas - rend) > np.float32(thresh))
    return m


def ref_points(depth, K) -> np.ndarray:
    """get_pointcloud in fp32 -> [H,W,3]"""
    d, K = np.asarray(depth, np.float32), np.asarray(K, np.float32)
    H, W = d.shape
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    return np.stack([(u - K[0, 2]) * (d / K[0, 0]), (v - K[1, 2]) * (d / K[1, 1]), d], -1).astype(np.float32)


def ref_graph_f32(src, dst, noise_bound: float = NOISE_BOUND) -> np.ndarray:
    s, d = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    ns = np.sqrt(dist2_f32(s[None, :], s[:, None]))
    nd = np.sqrt(dist2_f32(d[None, :], d[:, None]))
    adj = np.abs(ns - nd) <= np.float32(2.0) * np.float32(noise_bound)
    np.fill_diagonal(adj, False)
    return adj


def ref_graph_f64(src, dst, noise_bound: float = NOISE_BOUND):
    """-> (adjacency, the pairs whose test is decided by more than GRAPH_MARGIN) in float64"""
    s, d = np.asarray(src, np.float32).astype(np.float64), np.asarray(dst, np.float32).astype(np.float64)
    diff = np.abs(np.linalg.norm(s[None] - s[:, None], axis=-1) - np.linalg.norm(d[None] - d[:, None], axis=-1))
    thr = 2.0 * float(np.float32(noise_bound))
    adj = diff <= thr
    clear = np.abs(diff - thr) > GRAPH_MARGIN
    np.fill_diagonal(adj, False)
    np.fill_diagonal(clear, False)
    return adj, clear


def ref_cores(adj) -> np.ndarray:
    """core numbers by the sequential peel: remove a vertex of the smallest degree, one at a time; its core number is the largest such
    smallest degree seen so far"""
    a = np.asarray(adj).astype(bool)
    n = len(a)
    deg = a.sum(1).astype(np.int64)
    alive = np.ones(n, bool)
    core = np.zeros(n, np.int64)
    k = 0
    for _ in range(n):
        cand = np.where(alive)[0]
        v = cand[np.argmin(deg[cand])]
        k = max(k, int(deg[v]))
        core[v] = k
        alive[v] = False
        deg[a[v] & alive] -= 1
    return core


def kabsch(a, b, w=None) -> np.ndarray:
    """R maximising trace(R sum w a b^T) over rotations, by SVD with the determinant fixed (no centring: TIMs have no translation)"""
    w = np.ones(len(a)) if w is None else w
    H = (a * w[:, None]).T @ b
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    return Vt.T @ D @ U.T


def ref_gnc(a, b, beta: float):
    """GNC-TLS over the TIMs a -> b -> (R, iterations)"""
    beta2 = beta * beta
    w = np.ones(len(a))
    mu, prev, its = 0.0, np.inf, 0
    R = np.eye(3)
    for i in range(100):
        R = kabsch(a, b, w)
        r2 = ((b - a @ R.T) ** 2).sum(1)
        if i == 0:
            mu = 1.0 / (2.0 * r2.max() / beta2 - 1.0)
            if not mu > 0:
                break
        cost = float((w * r2).sum())
        hi, lo = (mu + 1.0) / mu * beta2, mu / (mu + 1.0) * beta2
        with np.errstate(divide="ignore", invalid="ignore"):
            mid = np.sqrt(beta2 * mu * (mu + 1.0) / r2) - mu
        w = np.where(r2 >= hi, 0.0, np.where(r2 <= lo, 1.0, mid))
        its += 1
        if abs(cost - prev) < 1e-12:
            break
        prev = cost
        mu *= 1.4
    return R, its


def ref_tls_1d(x, beta: float) -> float:
    ends = np.sort(np.concatenate([x - beta, x + beta]), kind="stable")
    best, best_cost = 0.0, None
    for c in 0.5 * (ends[:-1] + ends[1:]):
        cons = np.abs(x - c) <= beta
        if not cons.any():
            continue
        xh = x[cons].mean()
        cost = np.minimum((x - xh) ** 2, beta * beta).sum()
        if best_cost is None or cost < best_cost:
            best, best_cost = xh, cost
    return float(best)


def ref_solve(src, dst, noise_bound: float = NOISE_BOUND, min_num_inliers: int = 0, inlier_selection: str = "kcore", rotation_tim_graph: str = "chain"):
    """one row -> dict(Rt [3,4] float64 or None when rejected, selected [M] bool, core, n_selected, gnc_iterations, num_inliers, retval)"""
    s32, d32 = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    beta = float(np.float32(noise_bound))
    adj = ref_graph_f32(s32, d32, noise_bound)
    core = ref_cores(adj)
    sel = np.ones(len(s32), bool) if inlier_selection == "none" else core == (core.max() if len(core) else 0)
    out = dict(Rt=None, selected=sel, core=core, n_selected=int(sel.sum()), gnc_iterations=0, num_inliers=0, retval=-1)
    if sel.sum() < 3:
        return out
    s, d = s32[sel].astype(np.float64), d32[sel].astype(np.float64)
    if rotation_tim_graph == "chain":
        p, q = np.arange(len(s) - 1), np.arange(1, len(s))
    else:
        p, q = np.triu_indices(len(s), 1)
    R, its = ref_gnc(s[q] - s[p], d[q] - d[p], beta)
    x = d - s @ R.T
    t = np.asarray([ref_tls_1d(x[:, k], beta) for k in range(3)])
    res = np.linalg.norm(s32.astype(np.float64) @ R.T + t - d32.astype(np.float64), axis=1)
    n_in = int((res < beta).sum())
    out.update(Rt=np.concatenate([R, t[:, None]], 1), gnc_iterations=its, num_inliers=n_in, retval=0 if n_in >= min_num_inliers else -1)
    return out


def ref_refine_row(depth_meas, depth_rend, K, mask_type="simple", depth_delta_thresh=0.1, n_min_points=100, n_points=1000, noise_bound=NOISE_BOUND,
                   min_num_inliers=50, use_farthest_point_sampling=True, inlier_selection="kcore", rotation_tim_graph="chain"):
    """the whole chain on one row's frames -> ref_solve's dict plus N, sample_idx (None for a row under n_min_points)"""
    dm, dr = np.asarray(depth_meas, np.float32), np.asarray(depth_rend, np.float32)
    mask = ref_mask(dm, dr, mask_type, depth_delta_thresh)
    N = int(mask.sum())
    if N < n_min_points or N < 1:
        return dict(N=N, sample_idx=None, Rt=None, retval=-1, num_inliers=0, n_selected=0, gnc_iterations=0)
    src, dst = ref_points(dr, K)[mask], ref_points(dm, K)[mask]
    idx = ref_fps(src, n_points) if use_farthest_point_sampling else ref_stride(N, n_points)
    out = ref_solve(src[idx], dst[idx], noise_bound, min_num_inliers, inlier_selection, rotation_tim_graph)
    out.update(N=N, sample_idx=idx)
    return out


# fixtures ------------------------------------------------------------------------------------------------------------------------------------
def rotation(axis, angle: float) -> np.ndarray:
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.asarray([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


@lru_cache(maxsize=None)
def correspondences(n: int, outliers: float, seed: int):
    """n correspondences in a 0.3 m box at 0.6 m: dst = R src + t + noise within NOISE_BOUND / 4 (uniform in a ball), a share `outliers`
    of them replaced by points of another box (0.2 m to the side).  -> src, dst [n,3] fp32, R, t, inlier flags.  Read-only."""
    rng = np.random.RandomState(seed)
    src = rng.uniform(-0.15, 0.15, size=(n, 3)) + [0.0, 0.0, 0.6]
    R = rotation(rng.normal(size=3), np.deg2rad(rng.uniform(10.0, 40.0)))
    t = rng.uniform(-0.05, 0.05, size=3)
    dirs = rng.normal(size=(n, 3))
    noise = dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * (NOISE_BOUND / 4 * rng.uniform(0, 1, size=(n, 1)) ** (1 / 3))
    dst = src @ R.T + t + noise
    n_out = int(round(outliers * n))
    bad = rng.permutation(n)[:n_out]
    dst[bad] = rng.uniform(-0.15, 0.15, size=(n_out, 3)) + [0.2, 0.0, 0.6]
    inl = np.ones(n, bool)
    inl[bad] = False
    out = (src.astype(np.float32), dst.astype(np.float32), R, t, inl)
    for a in out:
        a.setflags(write=False)
    return out


SOLVE_CASES = tuple((n, o, 100 * n + int(10 * o)) for n in (50, 120, 200) for o in (0.0, 0.3, 0.6))   # (n, outlier share, seed)


def pose_error(Rt, R, t, centre) -> Tuple[float, float]:
    """-> (rotation angle between Rt's rotation and R, distance of the two images of `centre`)"""
    dR = Rt[:, :3] @ R.T
    ang = float(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return ang, float(np.linalg.norm(Rt[:, :3] @ centre + Rt[:, 3] - (R @ centre + t)))


K_SMALL = np.asarray([[120.0, 0.0, 0.0], [0.0, 120.0, 0.0], [0.0, 0.0, 1.0]], np.float32)


def surface(H: int, W: int, phase: float = 0.0) -> np.ndarray:
    """a bumpy depth surface around 0.6 m, fp32 [H,W]"""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return (0.6 + 0.05 * np.sin(0.31 * u + phase) * np.cos(0.27 * v) + 0.04 * (u / W) - 0.03 * (v / H) ** 2).astype(np.float32)


@lru_cache(maxsize=None)
def frame_case(H: int, W: int, counts: Tuple[int, ...], kinds: Tuple[str, ...], seed: int):
    """One launch: 2 measured frames (the surface, frame 1 with another phase), len(counts) rows.  Row r renders the surface of its image
    moved 8 mm towards the camera on counts[r] pixels (a seeded scattered set; 0 elsewhere), so every mask pixel is a near-rigid
    correspondence; kind "noise": the rendered values are random instead (all outliers); kind "far": half the pixels are rendered
    0.5 m off (the threshold mask drops them).  -> depth_meas [2,H,W], im_ids, depth_rend [n,H,W], K_rows, TCO; read-only."""
    rng = np.random.RandomState(seed)
    meas = np.stack([surface(H, W), surface(H, W, 1.3)])
    n = len(counts)
    im_ids = (np.arange(n) % 2).astype(np.int32)
    rend = np.zeros((n, H, W), np.float32)
    for r, (cnt, kind) in enumerate(zip(counts, kinds)):
        px = np.sort(rng.permutation(H * W)[:cnt])
        val = meas[im_ids[r]].reshape(-1)[px] - np.float32(0.008)
        if kind == "noise":
            val = rng.uniform(0.3, 0.9, size=cnt).astype(np.float32)
        if kind == "far":
            val = val + np.where(np.arange(cnt) % 2 == 0, np.float32(0.5), np.float32(0.0))
        rend[r].reshape(-1)[px] = val
    K = np.repeat(K_SMALL[None], n, 0).copy()
    K[:, 0, 2], K[:, 1, 2] = W / 2.0, H / 2.0
    K[:, 0, 0] += np.arange(n)          # every row its own intrinsics
    TCO = np.repeat(np.eye(4, dtype=np.float32)[None], n, 0)
    for r in range(n):
        TCO[r, :3, :3] = rotation(rng.normal(size=3), 0.3 * (r + 1)).astype(np.float32)
        TCO[r, :3, 3] = [0.01 * r, -0.02, 0.6]
    out = (meas, im_ids, rend, K, TCO)
    for a in out:
        a.setflags(write=False)
    return out


FPS_RESIDENT = 16384   # points of a row the sampling kernel keeps in registers (teaser_core.h kFpsResident; the CPU test holds it to limits())
# The launches from depth frames both test files run: name -> (frame_case arguments, keywords of the refiner).  Frames of 32 x 24 to
# 160 x 120, 3 to 5 rows over 2 images, mask counts around the wave (63, 64, 65) and the workgroup (1023, 1025), one more than the
# register-resident points of the sampling kernel and every pixel of a frame, an empty mask, rows under n_min_points, a row of
# outliers only ("noise") and one whose threshold mask drops half the pixels ("far"); n_points 64, 65, 100 and 1000.  "odd": a frame of
# 7 x 37 = 259 pixels, no multiple of the wave or the workgroup, whose masks keep 65 pixels, every pixel and none (the compaction's edges).
FRAME_CASES = {
    "tiny": ((24, 32, (1, 63, 64, 65, 0), ("",) * 5, 3), dict(n_min_points=1, n_points=64, min_num_inliers=20)),
    "odd": ((7, 37, (65, 7 * 37, 0), ("",) * 3, 11), dict(n_min_points=1, n_points=64, min_num_inliers=20)),
    "small": ((24, 32, (700, 64, 0, 300, 500), ("", "", "", "far", "noise"), 5), dict(n_min_points=100, n_points=100, min_num_inliers=50)),
    "mid": ((48, 64, (1023, 1025, 3000, 2000), ("", "", "noise", "far"), 7), dict(n_min_points=100, n_points=65, min_num_inliers=30)),
    "big": ((120, 160, (FPS_RESIDENT + 1, 120 * 160, 5000), ("", "", ""), 9), dict(n_min_points=100, n_points=1000, min_num_inliers=50)),
}
FRAME_VARIANTS = (dict(), dict(mask_type="threshold"), dict(rotation_tim_graph="complete"), dict(inlier_selection="none"),
                  dict(use_farthest_point_sampling=False))


@lru_cache(maxsize=None)
def emul_frames(name: str, variant: int):
    """the emulation's result of one launch, computed once"""
    frames, kw = FRAME_CASES[name]
    return emul_refine(*frame_case(*frames), **kw, **FRAME_VARIANTS[variant])
