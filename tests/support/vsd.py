"""TEST SUPPORT: ctypes wrapper of the host emulation of the VSD and MSPD kernels (tests/vsd_emul.cpp), built on first use, and an
independent float64 restatement of the two definitions (written from the definitions, not from the arithmetic headers) with the
borderline-pixel census and the derived MSPD bound the emulation is held to."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np

from . import pose_error as _pe
from .emul import CSRC, TESTS, _f32, _i32, _p, build

ULP = 2.0 ** -24
BAND_ROUNDINGS = 16          # band of a borderline pixel = 16 * 2^-24 * D_max (derived in tests/test_vsd_contract_cpu.py)
DEFAULT_TAUS = tuple(np.arange(0.05, 0.51, 0.05))


def load():
    lib = build("vsd_emul", [TESTS / "vsd_emul.cpp", CSRC / "vsd_core.h"])
    lib.vsd_emul.restype = None
    return lib


def vsd(depth_est, depth_gt, depth_test, K, diameter, delta=0.015, taus=DEFAULT_TAUS, normalized=True, est_ids=None, gt_ids=None,
        im_ids=None) -> Dict[str, np.ndarray]:
    """Same addressing as megapose6d_amd.engine.vsd -> errs [b,n_tau] float32, counts [b,2+n_tau] int32."""
    depth_est, depth_gt, depth_test, K, diameter = _f32(depth_est), _f32(depth_gt), _f32(depth_test), _f32(K), _f32(diameter)
    est_ids, gt_ids, im_ids = _i32(est_ids), _i32(gt_ids), _i32(im_ids)
    taus = _f32(taus)
    b, n_tau = K.shape[0], taus.shape[0]
    h, w = depth_est.shape[1:]
    assert depth_gt.shape[1:] == (h, w) and depth_test.shape[1:] == (h, w) and K.shape == (b, 3, 3) and diameter.shape == (b,)
    for ids, maps in ((est_ids, depth_est), (gt_ids, depth_gt), (im_ids, depth_test)):
        assert (maps.shape[0] >= b) if ids is None else (ids.shape == (b,) and (b == 0 or (ids.min() >= 0 and ids.max() < maps.shape[0])))
    out = dict(errs=np.empty((b, n_tau), np.float32), counts=np.empty((b, 2 + n_tau), np.int32))
    load().vsd_emul(_p(depth_est), _p(est_ids), _p(depth_gt), _p(gt_ids), _p(depth_test), _p(im_ids), _p(K), _p(diameter), C.c_int(b), C.c_int(h),
                    C.c_int(w), C.c_float(delta), _p(taus), C.c_int(n_tau), C.c_int(int(normalized)), _p(out["errs"]), _p(out["counts"]))
    return out


def mspd(T_pred, T_gt, symmetries, n_sym, points, K, mesh_ids=None, n_points=None, reduce_max=True) -> Dict[str, np.ndarray]:
    """Same addressing as megapose6d_amd.engine.pose_error_mspd (symmetries None: T_gt = candidates [b,S,4,4])."""
    return _pe.sym(T_pred, T_gt, symmetries, n_sym, points, mesh_ids, n_points, reduce_max=reduce_max, with_diffs=False, K=K)


# float64 restatement of the definitions on the same fp32 inputs ---------------------------------------------------------------------
def f64_vsd(depth_est, depth_gt, depth_test, K, diameter, delta=0.015, taus=DEFAULT_TAUS, normalized=True, est_ids=None, gt_ids=None,
            im_ids=None) -> Dict[str, np.ndarray]:
    """-> counts [b,2+n_tau] int64, errs [b,n_tau] float64, borderline [b,2+n_tau] (pixels of each counter whose compared quantity lies
    within 16 * 2^-24 * D_max of its threshold), d_max [b].  Thresholds are the fp32 values the kernel is given, widened."""
    K = np.asarray(np.asarray(K, np.float32), np.float64)
    diameter = np.asarray(np.asarray(diameter, np.float32), np.float64)
    taus = np.asarray(np.asarray(taus, np.float32), np.float64)
    delta = float(np.float32(delta))
    b, n_tau = K.shape[0], taus.shape[0]
    h, w = np.asarray(depth_est).shape[1:]
    counts = np.zeros((b, 2 + n_tau), np.int64)
    border = np.zeros((b, 2 + n_tau), np.int64)
    errs = np.full((b, n_tau), np.nan)
    d_max = np.zeros(b)
    xs, ys = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    for i in range(b):
        if not (np.isfinite(K[i]).all() and np.isfinite(diameter[i]) and diameter[i] > 0):
            counts[i] = -1
            continue
        u = (xs + 0.5 - K[i, 0, 2]) / K[i, 0, 0]
        v = (ys + 0.5 - K[i, 1, 2]) / K[i, 1, 1]
        r = np.sqrt(u * u + v * v + 1.0)
        z_test = np.asarray(depth_test[i if im_ids is None else im_ids[i]], np.float64)
        z_test = np.where(np.isfinite(z_test) & (z_test >= 0), z_test, 0.0)
        d_est = np.asarray(depth_est[i if est_ids is None else est_ids[i]], np.float64) * r
        d_gt = np.asarray(depth_gt[i if gt_ids is None else gt_ids[i]], np.float64) * r
        d_test = z_test * r
        d_max[i] = max(d_est.max(), d_gt.max(), d_test.max())
        band = BAND_ROUNDINGS * ULP * d_max[i]
        unobserved = d_test == 0
        vis_gt = (d_gt > 0) & (unobserved | (d_gt - d_test <= delta))
        vis_est = (d_est > 0) & (unobserved | (d_est - d_test <= delta) | vis_gt)
        inter, union = vis_gt & vis_est, vis_gt | vis_est
        near_vis = ((d_gt > 0) & ~unobserved & (np.abs(d_gt - d_test - delta) <= band)) | ((d_est > 0) & ~unobserved & (np.abs(d_est - d_test - delta) <= band))
        counts[i, 0], counts[i, 1] = union.sum(), inter.sum()
        border[i, 0] = border[i, 1] = near_vis.sum()
        gap = np.abs(d_gt - d_est)
        for t in range(n_tau):
            thr = taus[t] * diameter[i] if normalized else taus[t]
            counts[i, 2 + t] = (inter & (gap >= thr)).sum()
            border[i, 2 + t] = (near_vis | ((d_gt > 0) & (d_est > 0) & (np.abs(gap - thr) <= band))).sum()
            errs[i, t] = 1.0 if counts[i, 0] == 0 else (counts[i, 2 + t] + (counts[i, 0] - counts[i, 1])) / counts[i, 0]
    return dict(counts=counts, errs=errs, borderline=border, d_max=d_max)


def f64_project(K, T, pts):
    """K [3,3], T [...,4,4], pts [N,3] -> pixel positions [...,N,2] and camera-frame depths [...,N]"""
    K, T, pts = np.asarray(K, np.float64), np.asarray(T, np.float64), np.asarray(pts, np.float64)
    cam = np.einsum("...ij,nj->...ni", T[..., :3, :3], pts) + T[..., None, :3, 3]
    hom = np.einsum("ij,...nj->...ni", K, cam)
    return hom[..., :2] / hom[..., 2:3], cam[..., 2]


def f64_mspd_errs(T_pred, T_gt, syms, pts, K):
    """one row: T_pred, T_gt [4,4], syms [S,4,4], pts [N,3], K [3,3] -> errs [S] (max over the points), the smallest camera-frame depth"""
    G = np.asarray(T_gt, np.float64) @ np.asarray(syms, np.float64)
    uv_p, z_p = f64_project(K, T_pred, pts)
    uv_g, z_g = f64_project(K, G, pts)
    return np.linalg.norm(uv_g - uv_p[None], axis=-1).max(-1), float(min(z_p.min(), z_g.min()))


MSPD_K, MSPD_C = 32.0, 16.0


def mspd_bound(K, sigma: float, z_min: float, U: float) -> float:
    """2^-24 * (32 * (f + U) * sigma / z_min + 16 * U): derived in tests/test_vsd_contract_cpu.py"""
    K = np.asarray(K, np.float64)
    f = max(abs(K[0, 0]), abs(K[1, 1]))
    return ULP * (MSPD_K * (f + U) * sigma / z_min + MSPD_C * U)


# seeded cases shared by the CPU contract test and the GPU test ------------------------------------------------------------------------
def intrinsics(f, cx, cy):
    return np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]], np.float32)


def scene(seed, b, h, w, n_im=None, n_gt=None, share=False, n_est=None):
    """seeded maps: a large blob at 0.5 - 2.5 m as ground truth, estimates = the blob shifted by a few pixels with a smooth offset of
    centimetres, observed frames = the ground truth + millimetre noise, a nearer occluder, a hole of zeros and a few invalid values"""
    rng = np.random.RandomState(seed)
    n_gt = n_gt or b
    n_im = n_im or n_gt
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    gts = []
    for g in range(n_gt):
        z0 = rng.uniform(0.6, 2.2)
        surf = z0 + 0.08 * np.sin(xx / max(w, 2) * 3 + g) + 0.06 * np.cos(yy / max(h, 2) * 2 + g)
        mask = ((xx - w * 0.5) / (w * 0.49)) ** 2 + ((yy - h * 0.5) / (h * 0.49)) ** 2 <= 1.0
        gts.append(np.where(mask, surf, 0.0))
    gts = np.stack(gts).astype(np.float32)
    gt_ids = (np.arange(b) % n_gt).astype(np.int32) if share else None
    gi = gt_ids if share else np.arange(b)
    n_est = n_est or b                                    # n_est < b: rows share estimate maps too (n_est a multiple of n_gt)
    est_ids = (np.arange(b) % n_est).astype(np.int32) if n_est < b else None
    ests = []
    for i in range(n_est):
        dx, dy = rng.randint(-3, 4), rng.randint(-2, 3)
        src = np.roll(np.roll(gts[gi[i]].astype(np.float64), dy, axis=0), dx, axis=1)
        off = rng.uniform(-0.06, 0.06) + 0.05 * np.sin(xx / max(w, 2) * 5 + i) * np.cos(yy / max(h, 2) * 4)
        ests.append(np.where(src > 0, src + off, 0.0))
    ests = np.stack(ests).astype(np.float32)
    im_ids = (gi % n_im).astype(np.int32) if share else None
    tests = []
    for m in range(n_im):
        base = gts[m % n_gt].astype(np.float64)
        t = np.where(base > 0, base + rng.randn(h, w) * 0.004, rng.uniform(2.6, 3.0))
        t[: h // 4, : w // 3] -= 0.2                      # an occluder
        t[h - h // 5:, w - w // 4:] = 0.0                  # a hole
        flat = t.reshape(-1)
        k = max(1, flat.size // 200)
        flat[rng.choice(flat.size, k, replace=False)] = np.nan
        flat[rng.choice(flat.size, k, replace=False)] = -0.5
        tests.append(t)
    tests = np.stack(tests).astype(np.float32)
    f = 0.9 * max(w, h)
    K = np.stack([intrinsics(f * rng.uniform(0.9, 1.1), w / 2 + rng.uniform(-2, 2), h / 2 + rng.uniform(-2, 2)) for _ in range(b)])
    diam = rng.uniform(0.1, 0.3, size=b).astype(np.float32)
    return dict(est=ests, gt=gts, test=tests, K=K, diam=diam, est_ids=est_ids, gt_ids=gt_ids, im_ids=im_ids)


def taus_of(n):
    return DEFAULT_TAUS if n == 10 else ([0.2] if n == 1 else list(np.linspace(0.02, 0.5, 16)))


def mspd_case(b, N, S, seed, n_mesh=1, ragged=False):
    rng = np.random.RandomState(seed)
    n_points = np.array([N if (not ragged or m == 0) else max(1, N - 1 - 97 * m) for m in range(n_mesh)], np.int32)
    n_sym = np.array([S if (not ragged or m == 0) else max(1, S // (3 * m)) for m in range(n_mesh)], np.int32)
    pts = (rng.uniform(-1, 1, size=(n_mesh, N, 3)) * np.array([0.04, 0.06, 0.1])).astype(np.float32)
    syms = np.tile(np.eye(4, dtype=np.float32), (n_mesh, S, 1, 1))
    for m in range(n_mesh):
        for s in range(n_sym[m]):
            syms[m, s] = _pe.pose(_pe.axis_rotation(2, 2 * np.pi * s / n_sym[m]), [0.0, 0.0, 0.002 * (s % 2)])
    ids = ((np.arange(b) + n_mesh - 1) % n_mesh).astype(np.int32)
    T_gt = _pe.random_poses(rng, b)
    T_pred = np.stack([_pe.perturbed(rng, (T_gt[i].astype(np.float64) @ syms[ids[i], (3 * i + 1) % n_sym[ids[i]]].astype(np.float64))[None], 1.5, 0.003)[0]
                       for i in range(b)])
    K = np.stack([intrinsics(600.0 * rng.uniform(0.9, 1.1), 320.0 + rng.uniform(-5, 5), 240.0 + rng.uniform(-5, 5)) for _ in range(b)])
    return dict(T_pred=T_pred, T_gt=T_gt, syms=syms, n_sym=n_sym, pts=pts, ids=ids, n_points=n_points, K=K)
