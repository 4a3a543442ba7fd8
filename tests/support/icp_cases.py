"""Analytic cases for the depth refiners (csrc/icp_nn.hip, csrc/icp.hip): no renderer, no mesh.

`engine.icp_refine` takes the rendered depth as an argument, so a case is just arrays: measured frames [B,H,W], K [B,3,3], im_ids [N],
rendered depth [N,H,W], TCO [N,4,4], optional caller masks [B,H,W] and the parameters.  The surfaces are smooth bumpy bowls
z = z0 + a (u^2 + c v^2) + b sin(.) cos(.) over a disc or the whole frame; the measured side carries seeded millimetre noise (so that no two
candidate distances tie: no tie-break is asserted anywhere), the rendered side is the same function shifted by under a pixel and a few
millimetres.  Every K has a fractional principal point: `x - cx` is negative and non-integer on part of the frame, where the reference's
cast to int16 truncates toward zero.

tests/test_icp_cases_cpu.py proves on the restatement alone that every case does what its name says; tests/test_gpu_icp_edges.py runs them
on the device.  The restatement's answers are computed once per process (`nn_reference`, `projective_reference`) and shared.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

F32 = np.float32
DEFAULTS = dict(n_iterations=100, n_levels=4, tolerance=0.05, n_min_points=50)


@dataclass
class IcpCase:
    name: str
    depth: np.ndarray                 # [B,H,W] float32 measured frames
    K: np.ndarray                     # [B,3,3] float32
    im_ids: np.ndarray                # [N] int32
    rend: np.ndarray                  # [N,H,W] float32 rendered depth
    TCO: np.ndarray                   # [N,4,4] float32
    masks: Optional[np.ndarray] = None   # [B,H,W] bool: the caller's masks (None: the 0.1 m threshold mask)
    params: dict = field(default_factory=lambda: dict(DEFAULTS))
    m: Optional[list] = None          # designed scene / model point counts per row (None: not designed, only measured)
    n: Optional[list] = None
    over_capacity: tuple = ()         # rows with more mask pixels than the device's 2^18 points: rejected there, not run on the CPU
    notes: dict = field(default_factory=dict)


# ---- surfaces -----------------------------------------------------------------------------------------------------------------------
def intrinsics(H: int, W: int, k: int = 0) -> np.ndarray:
    """fractional principal point; fx, fy, cx, cy all change with k"""
    K = np.eye(3, dtype=np.float64)
    K[0, 0], K[1, 1] = W * (1.10 + 0.07 * k), W * (1.04 + 0.05 * k)
    K[0, 2], K[1, 2] = W / 2 + 0.37 - 1.25 * k, H / 2 - 0.41 + 0.75 * k
    return K.astype(F32)


def bowl(H: int, W: int, k: int = 0, dx: float = 0.0, dy: float = 0.0, dz: float = 0.0, radius: Optional[float] = 0.9,
         centre=(0.0, 0.0), tilt: float = 0.0) -> np.ndarray:
    """z at the pixel centres of an H x W frame; (dx, dy) shifts the surface in pixels, dz in metres; radius (normalised; None = whole
    frame) cuts a disc around `centre`; tilt adds a plane (a different shape: for the rows that must be rejected by their residual)"""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = (xs - dx - (W - 1) / 2) / (W / 2), (ys - dy - (H - 1) / 2) / (H / 2)
    z = (0.55 + 0.04 * k) + (0.06 + 0.01 * k) * (u * u + (0.6 + 0.2 * k) * v * v) + 0.012 * np.sin(3.1 * u + 0.4 + k) * np.cos(2.3 * v - 0.7 * k)
    z = z + dz + tilt * u
    if radius is not None:
        z = np.where((u - centre[0]) ** 2 + (v - centre[1]) ** 2 < radius * radius, z, 0.0)
    return z.astype(F32)


def noisy(z: np.ndarray, seed: int) -> np.ndarray:
    return np.where(z > 0, z + np.random.RandomState(seed).randn(*z.shape).astype(F32) * F32(0.001), z).astype(F32)


def pose(k: int = 0) -> np.ndarray:
    from oracle.icp import _rodrigues

    T = np.eye(4)
    T[:3, :3] = _rodrigues(np.array([0.3 + 0.1 * k, -0.5, 0.2 * k + 0.1]))
    T[:3, 3] = [0.01 * k, -0.02, 0.6 + 0.03 * k]
    return T.astype(F32)


def _single(name, H, W, *, k=0, radius=0.9, masks=None, rend=None, depth=None, **params) -> IcpCase:
    depth = noisy(bowl(H, W, k, radius=radius), 11 + k) if depth is None else depth
    rend = bowl(H, W, k, dx=0.4, dy=-0.3, dz=0.004, radius=radius) if rend is None else rend
    return IcpCase(name, depth[None], intrinsics(H, W, k)[None], np.zeros(1, np.int32), rend[None], pose(k)[None],
                   None if masks is None else masks[None], dict(DEFAULTS, **params))


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def frame_cases() -> list:
    """default parameters, threshold mask.  7 x 200: axis 0 shorter than the Gaussian radius (the reflection wraps more than once);
    96 x 128: more than one model chunk and more than one scene segment in the search; 64 x 64 = 4 * 1024 pixels"""
    return [_single(f"frame_{H}x{W}", H, W) for H, W in ((7, 200), (17, 23), (37, 53), (64, 64), (96, 128))]


def _scattered_pixels(H: int, W: int, count: int) -> np.ndarray:
    """`count` distinct pixels spread over the whole frame (a seeded permutation), as flat indices: a cloud as wide as the frame keeps
    the 6 x 6 system well conditioned however few points it has"""
    return np.random.RandomState(5).permutation(H * W)[:count]


def count_case(m: int, n: int) -> IcpCase:
    """64 x 64, surface over the whole frame; the caller's mask selects exactly m pixels, the rendered depth is zero under the last
    m - n of them; n_min_points = 200"""
    H = W = 64
    order = _scattered_pixels(H, W, m)
    mask = np.zeros(H * W, bool)
    mask[order] = True
    rend = bowl(H, W, dx=0.4, dy=-0.3, dz=0.004, radius=None).ravel().copy()
    rend[order[n:]] = 0
    c = _single(f"count_m{m}_n{n}", H, W, radius=None, masks=mask.reshape(H, W), rend=rend.reshape(H, W), n_min_points=200)
    c.m, c.n = [m], [n]
    return c


COUNTS = ((199, 199), (200, 200), (260, 199), (260, 200), (1024, 1024), (1025, 1025), (1300, 1024), (1300, 1025), (1800, 600))


def count_cases() -> list:
    return [count_case(m, n) for m, n in COUNTS]


def tenth_pair():
    """float32 (m, r) with r in (0.1, 0.125), m = r + 0.1f just above 0.2 and fabsf(m - r) == 0.1f EXACTLY: the threshold mask keeps the
    pixel (its rule is "not greater than"), the range test keeps it too (m > 0.2f).  Found by walking r upward one ulp at a time."""
    tenth, r = F32(0.1), np.nextafter(F32(0.1), F32(1))
    while r < F32(0.125):
        m = F32(r + tenth)
        if F32(m - r) == tenth and m > F32(0.2):
            return m, r
        r = np.nextafter(r, F32(1))
    raise AssertionError("no such pair")


def content_cases() -> list:
    H, W = 48, 64
    out = []
    d = noisy(bowl(H, W), 11)
    d[11:37, 19:45] = 0                                    # wider than 2 x the 10 fill rings: its middle is never filled
    out.append(_single("content_hole26", H, W, depth=d))
    d = noisy(bowl(H, W, radius=None), 11)
    d[:3, :3] = 0
    out.append(_single("content_corner_hole", H, W, radius=None, depth=d, rend=bowl(H, W, dx=0.4, dy=-0.3, dz=0.004, radius=None)))
    d = noisy(bowl(H, W), 11)
    d[20, 30], d[30, 40], d[24, 5], d[10, 52] = np.nan, -0.3, np.inf, -np.inf   # (the infinities: just outside the disc, inside the Gaussian's reach)
    c = _single("content_nonfinite", H, W, depth=d)
    c.notes["pixels"] = [(20, 30), (30, 40), (24, 5), (10, 52)]
    out.append(c)
    d = noisy(bowl(H, W), 11)
    mask = d > 0
    d[22, 28], d[26, 36] = F32(0.2), F32(5.0)              # selected by the caller's mask, excluded by the strict range test
    c = _single("content_range_ends", H, W, depth=d, masks=mask)
    c.m, c.n = [int(mask.sum()) - 2], [int((mask & (c.rend[0] > 0)).sum()) - 2]
    assert c.rend[0][22, 28] > 0 and c.rend[0][26, 36] > 0
    c.notes["pixels"] = [(22, 28), (26, 36)]
    out.append(c)
    d, r = noisy(bowl(H, W), 11), bowl(H, W, dx=0.4, dy=-0.3, dz=0.004)
    base = int(((d > 0) & (r > 0)).sum())
    assert d[1, 2] == 0 and r[1, 2] == 0
    d[1, 2], r[1, 2] = tenth_pair()                        # a lone pixel off the disc
    c = _single("content_tenth_exact", H, W, depth=d, rend=r)
    c.m = c.n = [base + 1]
    c.notes["pixels"] = [(1, 2)]
    out.append(c)
    return out


PARAMS = ((100, 1), (100, 2), (100, 8), (7, 4), (2, 4), (1, 4), (3, 8))
# iterations per level of the three (n_iterations, n_levels) whose coarse levels have an iteration cap of 0 (or, from level 4 up, a
# stop band 0.05 * (level + 1)^2 > 1 that already holds fval_perc = 0): levels that run no iteration at all
ZERO_CAP_ITERS = {(2, 4): [2, 1, 1, 0], (1, 4): [1, 0, 0, 0], (3, 8): [3, 2, 1, 1, 0, 0, 0, 0]}


def param_cases() -> list:
    out = [_single(f"param_it{ni}_lv{nl}", 48, 64, n_iterations=ni, n_levels=nl) for ni, nl in PARAMS]
    # tolerance 1.5: every band reaches past 1, no level iterates at all -- the identity, residual 9999999999, rejected
    return out + [_single(f"param_tol{t}", 48, 64, tolerance=t) for t in (0.01, 0.2, 1.5)]


def _residual_reject_row(H, W, k, depth, K, T, params):
    """a rendered depth that the restatement runs to the end and then rejects by its residual.  The residual is the Frobenius norm of the
    matched 6-d rows over the number of model points, so only a SMALL cloud of the wrong shape gets past 0.05: the surface, tilted, kept at
    a seeded scatter of about 120 pixels (the normals of such a sparse image are rough, which is the point).  The first candidate that
    does it, in a fixed order."""
    from oracle import icp_opencv as ocv

    for seed in (2, 0, 1, 3, 4, 5, 6, 7):
        for tilt in (0.1, 0.05):
            keep = np.zeros(H * W, bool)
            keep[np.random.RandomState(seed).permutation(H * W)[:120]] = True
            r = np.where(keep.reshape(H, W), bowl(H, W, k, dx=0.4, dy=-0.3, dz=0.004, tilt=tilt), 0).astype(F32)
            _, rv, res = ocv.icp_refinement(depth, r, ocv.compute_masks_threshold(r, depth), K, T, n_min_points=params["n_min_points"],
                                            **{q: params[q] for q in ("n_iterations", "n_levels", "tolerance")})
            if rv == -1 and params["tolerance"] * 1.05 < res < 1.0:   # (a level 0 that ran: not the 9999999999 of a level without a pass)
                return r
    raise AssertionError("no candidate is rejected by its residual")


def compact_cases() -> list:
    """the ordered compaction of the mask pixels at its edges, on a frame of 7 x 37 = 259 pixels (no multiple of the wave or of the
    workgroup), surface over the whole frame: the caller's mask keeps 65 scattered pixels of which the rendered depth covers 61 (scene
    and model counts differ, neither a multiple of 64; one pyramid level, so that all of them enter the solve), every pixel (two levels),
    and none.  The first two are accepted: their poses depend on every point and on the order of the compacted lists."""
    H, W = 7, 37
    order = _scattered_pixels(H, W, 65)
    mask = np.zeros(H * W, bool)
    mask[order] = True
    rend = bowl(H, W, dx=0.4, dy=-0.3, dz=0.004, radius=None).ravel().copy()
    rend[order[61:]] = 0
    some = _single("compact_7x37_keep65", H, W, radius=None, masks=mask.reshape(H, W), rend=rend.reshape(H, W), n_levels=1)
    some.m, some.n = [65], [61]
    every = _single("compact_7x37_keep_all", H, W, radius=None, masks=np.ones((H, W), bool), n_levels=2)
    every.m = every.n = [H * W]
    none = _single("compact_7x37_keep_none", H, W, radius=None, masks=np.zeros((H, W), bool))
    none.m = none.n = [0]
    return [some, every, none]


@functools.lru_cache(maxsize=None)
def batch_case() -> IcpCase:
    """3 frames of 96 x 128, each its own surface and K; 6 rows in the order [2, 0, 2, 1, 0, 2] (frame 2 is used three times); row 1 has
    too few model points, row 3 is rejected by its residual, the others are accepted from different offsets"""
    H, W = 96, 128
    depth = np.stack([noisy(bowl(H, W, k), 20 + k) for k in range(3)])
    K = np.stack([intrinsics(H, W, k) for k in range(3)])
    im_ids = np.array([2, 0, 2, 1, 0, 2], np.int32)
    TCO = np.stack([pose(k) for k in range(6)])
    shifts = [(0.4, -0.3, 0.004), None, (-0.45, 0.2, -0.006), None, (0.15, 0.45, 0.008), (0.3, 0.3, -0.003)]
    rend = np.zeros((6, H, W), F32)
    for row, s in enumerate(shifts):
        if s is not None:
            rend[row] = bowl(H, W, int(im_ids[row]), dx=s[0], dy=s[1], dz=s[2])
    rend[1] = bowl(H, W, 0, dx=0.4, dy=-0.3, dz=0.004, radius=0.05)     # 49 pixels at most: under n_min_points
    rend[3] = _residual_reject_row(H, W, 1, depth[1], K[1], TCO[3], DEFAULTS)
    return IcpCase("batch", depth, K, im_ids, rend, TCO)


@functools.lru_cache(maxsize=None)
def capacity_case() -> IcpCase:
    """two 513 x 512 frames, depth everywhere.  Row 0: a mask of all ones = 262,656 points, more than the 2^18 the nearest-neighbour key
    indexes -> retval -1, the input pose, residual -1.  Row 1 (the other frame): a mask of 1,500 pixels, refined as usual."""
    H, W = 513, 512
    depth = np.stack([noisy(bowl(H, W, k, radius=None), 30 + k) for k in range(2)])
    masks = np.ones((2, H, W), bool)
    masks[1] = False
    masks[1].reshape(-1)[_scattered_pixels(H, W, 1500)] = True
    rend = np.stack([bowl(H, W, k, dx=0.4, dy=-0.3, dz=0.004, radius=None) for k in range(2)])
    c = IcpCase("capacity", depth, np.stack([intrinsics(H, W, k) for k in range(2)]), np.array([0, 1], np.int32), rend,
                np.stack([pose(0), pose(1)]), masks, over_capacity=(0,))
    c.m = c.n = [H * W, 1500]
    return c


@functools.lru_cache(maxsize=None)
def nn_cases() -> tuple:
    return tuple(frame_cases() + count_cases() + content_cases() + param_cases() + [batch_case(), capacity_case()] + compact_cases())


def nn_case(name: str) -> IcpCase:
    return next(c for c in nn_cases() if c.name == name)


NN_CASE_NAMES = ([f"frame_{H}x{W}" for H, W in ((7, 200), (17, 23), (37, 53), (64, 64), (96, 128))] + [f"count_m{m}_n{n}" for m, n in COUNTS]
                 + ["content_hole26", "content_corner_hole", "content_nonfinite", "content_range_ends", "content_tenth_exact"]
                 + [f"param_it{ni}_lv{nl}" for ni, nl in PARAMS] + ["param_tol0.01", "param_tol0.2", "param_tol1.5", "batch", "capacity"]
                 + ["compact_7x37_keep65", "compact_7x37_keep_all", "compact_7x37_keep_none"])


# ---- the restatement's answers ------------------------------------------------------------------------------------------------------
def row_mask(c: IcpCase, row: int) -> np.ndarray:
    from oracle import icp_opencv as ocv

    f = int(c.im_ids[row])
    return c.masks[f] if c.masks is not None else ocv.compute_masks_threshold(c.rend[row], c.depth[f])


def run_nn_oracle(c: IcpCase) -> list:
    """oracle/icp_opencv.py on every row with that row's own frame and K -> [dict(T, retval, residual, iters, ends, caps, n_model, n_scene)]
    (None for the rows over the device's capacity)"""
    from oracle import icp_opencv as ocv

    out = []
    p = c.params
    for row in range(len(c.im_ids)):
        if row in c.over_capacity:
            out.append(None)
            continue
        f = int(c.im_ids[row])
        info = {}
        T, rv, res = ocv.icp_refinement(c.depth[f], c.rend[row], row_mask(c, row), c.K[f], c.TCO[row], n_min_points=p["n_min_points"], info=info,
                                        n_iterations=p["n_iterations"], n_levels=p["n_levels"], tolerance=p["tolerance"])
        out.append(dict(T=np.asarray(T), retval=rv, residual=float(res), **info))
    return out


@functools.lru_cache(maxsize=None)
def nn_reference(name: str) -> list:
    return run_nn_oracle(nn_case(name))


# ---- projective association (csrc/icp.hip against oracle/icp.py) ------------------------------------------------------------------------
def projective_count(c: IcpCase, row: int, user_masks: bool = False) -> int:
    """the number of pixels csrc/icp.hip's point-count rule sees (an integer sum below 2^24: exact in float32)"""
    dm, dr = c.depth[int(c.im_ids[row])], c.rend[row]
    return int(((dm > 0) & (dr > 0) & ((np.abs(dm - dr) <= F32(0.1)) | user_masks) & (dm > F32(0.2)) & (dm < F32(5.0))).sum())


@functools.lru_cache(maxsize=None)
def projective_cases() -> tuple:
    """(case, user_masks) pairs.  With user_masks the measured depth is already multiplied by the caller's mask."""
    out = [(_single("proj_96x128", 96, 128), False), (_single("proj_97x131", 97, 131), False), (batch_case(), False)]
    base = _single("x", 96, 128)
    cnt = projective_count(base, 0)
    out += [(_single(f"proj_min_points_{tag}", 96, 128, n_min_points=cnt + extra), False) for tag, extra in (("count", 0), ("count_plus_1", 1))]
    # caller masks: the object's pixels without every 16th column (off the coarsest level's stride-8 lattice and its +-2 normal stencil, so
    # that level keeps its 50 inliers); the rendered depth has a 16 x 20 block 12 cm in front of the surface, which the threshold mask
    # would drop and the caller's mask keeps
    d = noisy(bowl(96, 128), 11)
    band = (d > 0) & (np.arange(128)[None, :] % 16 != 5)
    r = bowl(96, 128, dx=0.4, dy=-0.3, dz=0.004)
    r[40:56, 50:70] -= F32(0.12)
    out.append((_single("proj_user_masks", 96, 128, depth=np.where(band, d, 0).astype(F32), rend=r), True))
    out += [(_single(f"proj_it{ni}_lv{nl}", 96, 128, n_iterations=ni, n_levels=nl), False) for ni, nl in ((7, 4), (100, 1))]
    return tuple(out)


PROJECTIVE_CASE_NAMES = ["proj_96x128", "proj_97x131", "batch", "proj_min_points_count", "proj_min_points_count_plus_1", "proj_user_masks",
                         "proj_it7_lv4", "proj_it100_lv1"]


def projective_case(name: str):
    return next((c, um) for c, um in projective_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def projective_reference(name: str) -> list:
    from oracle import icp as oicp

    c, um = projective_case(name)
    out = []
    for row in range(len(c.im_ids)):
        f = int(c.im_ids[row])
        T, rv, res = oicp.icp_refine(c.depth[f], c.rend[row], c.K[f], c.TCO[row], user_masks=um, **c.params)
        out.append(dict(T=np.asarray(T), retval=rv, residual=float(res)))
    return out
