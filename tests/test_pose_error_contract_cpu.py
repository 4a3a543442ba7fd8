"""CPU: the arithmetic contract of the pose-error kernels (megapose6d_amd/csrc/pose_error_core.h), through the host emulation built
from that header (tests/pose_error_emul.cpp; reductions in double, rounded once).

The distance bound beta(sigma) = 64 * 2^-24 * sigma, sigma = the largest |translation| among pred, gt and the symmetries + 2 x the
mesh's bounding radius, is derived and not measured: each transformed coordinate takes <= 4 roundings at magnitude <= sigma, composing
T_gt * Sym adds 4 more on the gt side, the difference 1, the norm <= sqrt(3) x that + 2 -- about 24 roundings; 64 leaves ~2.5x for a
pairwise mean.  Arg-mins are held to the rule "the float64 error AT the returned index is within beta of the float64 minimum" (near
ties may resolve differently in fp32); on EXACT ties the lowest index must come back.
"""
from pathlib import Path

import numpy as np
import pytest

from support import pose_error as pes

GOLDEN = Path(__file__).resolve().parent / "golden" / "pose_errors.npz"


def _object_points(rng, n, n_valid=None):
    pts = (rng.uniform(-1, 1, size=(n, 3)) * np.array([0.04, 0.06, 0.1])).astype(np.float32)
    if n_valid is not None and n_valid < n:
        pts[n_valid:] = pts[rng.choice(n_valid, size=n - n_valid)]   # BatchedMeshes' padding: re-drawn points of the same object
    return pts


def _sym_set(S, translation=(0.0, 0.0, 0.0)):
    return np.stack([pes.pose(pes.axis_rotation(2, 2 * np.pi * s / S), np.asarray(translation) * (s > 0)) for s in range(S)]).astype(np.float32)


def _f64_sym_errs(T_pred, T_gt, syms, pts):
    """-> norms [S, N] float64 of (T_gt Sym_s p - T_pred p), and the difference vectors [S, N, 3]"""
    G = np.asarray(T_gt, np.float64) @ np.asarray(syms, np.float64)
    d = pes.f64_transform(G, pts) - pes.f64_transform(T_pred, pts)[None]
    return np.linalg.norm(d, axis=-1), d


@pytest.mark.parametrize("b,N,S,n_valid", [(1, 1, 1, None), (3, 7, 1, None), (5, 63, 2, None), (4, 300, 8, 257), (2, 1031, 16, None)])
def test_symmetry_set_error_against_float64(b, N, S, n_valid):
    rng = np.random.RandomState(N + S)
    pts = np.stack([_object_points(rng, N, n_valid), _object_points(rng, N, n_valid)])
    syms = np.stack([_sym_set(S, (0.0, 0.0, 0.01)), _sym_set(S)])
    n_sym = np.array([S, max(1, S // 2)])
    n_points = np.array([n_valid or N, n_valid or N])
    ids = np.arange(b) % 2
    T_gt = pes.random_poses(rng, b)
    T_pred = np.stack([pes.perturbed(rng, (T_gt[i].astype(np.float64) @ syms[ids[i], i % n_sym[ids[i]]])[None], 5.0, 0.004)[0] for i in range(b)])
    worst = 0.0
    for reduce_max in (False, True):
        out = pes.sym(T_pred, T_gt, syms, n_sym, pts, ids, n_points, reduce_max=reduce_max)
        for i in range(b):
            m, ns, nv = ids[i], n_sym[ids[i]], n_points[ids[i]]
            beta = pes.beta(T_pred[i], T_gt[i], points=pts[m], symmetries=syms[m])
            norms, d = _f64_sym_errs(T_pred[i], T_gt[i], syms[m, :ns], pts[m, :nv])
            errs64 = norms.max(1) if reduce_max else norms.mean(1)
            alt64 = norms.mean(1) if reduce_max else norms.max(1)
            dev = np.abs(out["errs"][i, :ns] - errs64).max()
            worst = max(worst, dev / beta * 64)
            assert dev <= beta
            assert np.all(np.isposinf(out["errs"][i, ns:]))
            s = out["idx"][i]
            assert 0 <= s < ns
            assert errs64[s] - errs64.min() <= beta                       # rule (ii)
            assert abs(out["err"][i] - errs64[s]) <= beta and out["err"][i] == out["errs"][i, s]
            assert abs(out["err_alt"][i] - alt64.min()) <= beta
            assert np.abs(out["diffs"][i, :nv] - d[s]).max() <= beta
            assert np.all(out["diffs"][i, nv:] == 0)
            G = T_gt[i].astype(np.float64) @ syms[m, s].astype(np.float64)
            assert np.abs(out["T_gt_sym"][i] - G).max() <= beta
    print(f"sym ({b},{N},{S}): largest deviation {worst:.2f} x 2^-24 sigma")


def test_explicit_candidates_equal_the_composed_form_and_s1_is_dists_add():
    rng = np.random.RandomState(3)
    b, N, S = 4, 200, 6
    pts = _object_points(rng, N)[None]
    syms = _sym_set(S)[None]
    ids = np.zeros(b, np.int32)
    T_gt = pes.random_poses(rng, b)
    T_pred = pes.perturbed(rng, T_gt, 30.0, 0.01)
    comp = pes.sym(T_pred, T_gt, syms, None, pts, ids)
    cand = np.stack([pes.sym(T_pred, T_gt, syms[:, s:s + 1], None, pts, ids)["T_gt_sym"] for s in range(S)], axis=1)   # T_gt * Sym_s as the contract composes it
    expl = pes.sym(T_pred, cand, None, None, pts, ids)
    for k in ("err", "idx", "errs", "diffs", "T_gt_sym"):
        assert np.array_equal(comp[k], expl[k]), k
    one = pes.sym(T_pred, T_gt[:, None], None, None, pts, ids)
    assert np.array_equal(one["errs"][:, 0], comp["errs"][:, 0]) and np.all(one["idx"] == 0)


def test_exact_ties_return_the_lowest_index():
    rng = np.random.RandomState(5)
    # a symmetry listed twice: the prediction IS the ground truth times that symmetry
    A = pes.pose(pes.axis_rotation(2, np.pi / 2), [0, 0, 0])
    syms = np.stack([np.eye(4), A, A, np.eye(4)]).astype(np.float32)[None]
    pts = _object_points(rng, 50)[None]
    T_gt = pes.random_poses(rng, 3)
    T_pred = pes.sym(T_gt, T_gt, syms[:, 1:2], None, pts, np.zeros(3, np.int32))["T_gt_sym"]
    out = pes.sym(T_pred, T_gt, syms, None, pts, np.zeros(3, np.int32))
    assert np.all(out["idx"] == 1) and np.all(out["errs"][:, 1] == out["errs"][:, 2]) and np.all(out["err"] == 0)
    ident = pes.sym(T_gt, T_gt, syms, None, pts, np.zeros(3, np.int32))
    assert np.all(ident["idx"] == 0) and np.all(ident["errs"][:, 0] == ident["errs"][:, 3])
    # duplicated points (the padding of BatchedMeshes): every copy of a point is at distance 0, the first one must be assigned
    base = _object_points(rng, 40)
    dup = np.concatenate([base, base[rng.choice(40, size=25)], base[:5]])[None]
    first = np.array([int(np.flatnonzero((dup[0] == p).all(1))[0]) for p in dup[0]])
    nn = pes.nn(T_gt[:1], T_gt[:1], dup)
    assert np.array_equal(nn["assign"][0], first)
    assert np.all(nn["diffs"] == 0) and nn["mean"][0] == 0 and nn["max"][0] == 0
    # with only the first 40 valid the padded tail is not assigned at all
    nn40 = pes.nn(T_gt[:1], T_gt[:1], dup, None, np.array([40]))
    assert np.array_equal(nn40["assign"][0, :40], np.arange(40)) and np.all(nn40["assign"][0, 40:] == -1)
    # a row whose points are all the same point
    same = np.repeat(base[:1], 33, axis=0)[None]
    T_p = pes.perturbed(rng, T_gt[:1], 10.0, 0.02)
    nn1 = pes.nn(T_p, T_gt[:1], same)
    assert np.all(nn1["assign"] == 0) and nn1["mean"][0] == nn1["max"][0] > 0


@pytest.mark.parametrize("b,N,n_valid", [(1, 1, None), (3, 7, None), (2, 63, None), (2, 700, 611)])
def test_nearest_neighbour_error_against_float64(b, N, n_valid):
    rng = np.random.RandomState(11 + N)
    pts = np.stack([_object_points(rng, N, n_valid) for _ in range(b)])
    n_points = np.full(b, n_valid or N)
    T_gt = pes.random_poses(rng, b)
    T_pred = pes.perturbed(rng, T_gt, 25.0, 0.02)
    out = pes.nn(T_pred, T_gt, pts, None, n_points)
    worst = 0.0
    for i in range(b):
        nv = n_points[i]
        beta = pes.beta(T_pred[i], T_gt[i], points=pts[i])
        g = pes.f64_transform(T_gt[i], pts[i, :nv])
        q = pes.f64_transform(T_pred[i], pts[i, :nv])
        dist = np.linalg.norm(g[:, None] - q[None], axis=-1)      # [gt j, pred k]
        a = out["assign"][i, :nv]
        assert a.min() >= 0 and a.max() < nv and np.all(out["assign"][i, nv:] == -1)
        at = dist[np.arange(nv), a]
        assert np.all(at - dist.min(1) <= beta)                      # rule (ii)
        d64 = g - q[a]
        dev = max(np.abs(out["diffs"][i, :nv] - d64).max(), np.abs(np.linalg.norm(out["diffs"][i, :nv].astype(np.float64), axis=-1) - at).max())
        worst = max(worst, dev / beta * 64)
        assert dev <= beta
        assert abs(out["mean"][i] - dist.min(1).mean()) <= beta and abs(out["max"][i] - dist.min(1).max()) <= beta
        assert np.all(out["diffs"][i, nv:] == 0)
    print(f"nn ({b},{N}): largest deviation {worst:.2f} x 2^-24 sigma")


def test_against_the_reference_golden():
    g = np.load(GOLDEN)
    T_pred, T_gt, cand, pts = g["dist_T_pred"], g["dist_T_gt"], g["dist_T_gt_possible"], g["dist_points"]
    b = T_pred.shape[0]
    betas = np.array([pes.beta(T_pred[i], T_gt[i], cand[i], points=pts[i]) for i in range(b)])
    add = pes.sym(T_pred, T_gt[:, None], None, None, pts)
    assert np.all(np.abs(add["diffs"] - g["dists_add"]).max(axis=(1, 2)) <= 2 * betas)     # both sides fp32
    nn = pes.nn(T_pred, T_gt, pts)
    n_emul = np.linalg.norm(nn["diffs"].astype(np.float64), axis=-1)
    n_ref = np.linalg.norm(g["dists_add_symmetric"].astype(np.float64), axis=-1)
    assert np.all(np.abs(n_emul - n_ref).max(axis=1) <= 2 * betas)                        # by the norm: near ties may pick another neighbour
    sy = pes.sym(T_pred, cand, None, None, pts)
    for i in range(b):
        norms = np.linalg.norm(pes.f64_transform(cand[i], pts[i]) - pes.f64_transform(T_pred[i], pts[i])[None], axis=-1).mean(1)
        assert norms[sy["idx"][i]] - norms.min() <= betas[i]
        assert sy["idx"][i] == i % cand.shape[1]
    assert np.all(np.abs(sy["diffs"] - g["dists_add_symmetries"]).max(axis=(1, 2)) <= 2 * betas)


@pytest.mark.parametrize("angle_deg", [0.0, 1e-3, 5.0, 90.0, 179.999, 180.0])
def test_rotation_and_translation_error(angle_deg):
    rng = np.random.RandomState(int(angle_deg * 10) % 1000)
    Ta, Tb = [], []
    for _ in range(16):
        ax = rng.randn(3)
        ax /= np.linalg.norm(ax)
        a = np.deg2rad(angle_deg)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        dR = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
        A = pes.random_poses(rng, 1)[0].astype(np.float64)
        Ta.append(A)
        Tb.append(pes.pose(dR @ A[:3, :3], A[:3, 3] + rng.randn(3) * 0.02))
    Ta, Tb = np.stack(Ta).astype(np.float32), np.stack(Tb).astype(np.float32)
    out = pes.rigid(Ta, Tb)
    for i in range(16):
        want = pes.f64_rot_err_deg(Ta[i], Tb[i])      # float64 atan2 on the same fp32 inputs
        assert abs(out["rot_err_deg"][i] - want) <= 1e-4, (angle_deg, out["rot_err_deg"][i], want)
        assert abs(want - angle_deg) <= 1e-4 + (0.05 if angle_deg >= 179 else 0.0)   # fp32 rotation matrices are only orthonormal to ~1e-7
        t64 = np.linalg.norm(Ta[i, :3, 3].astype(np.float64) - Tb[i, :3, 3].astype(np.float64))
        assert abs(out["trans_err"][i] - t64) <= pes.beta(Ta[i], Tb[i], points=np.zeros((1, 3)))


def test_projection_error_against_float64():
    rng = np.random.RandomState(9)
    b, N, nv = 5, 400, 333
    pts = np.stack([_object_points(rng, N, nv) for _ in range(2)])
    ids = np.arange(b) % 2
    K = np.tile(np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1.0]], np.float32), (b, 1, 1))
    Ta = pes.random_poses(rng, b)
    Tb = pes.perturbed(rng, Ta, 5.0, 0.01)
    out = pes.rigid(Ta, Tb, K, pts, ids, np.array([nv, nv]))
    for i in range(b):
        uv = []
        for T in (Ta[i], Tb[i]):
            s = pes.f64_transform(T, pts[ids[i], :nv]) @ K[i].astype(np.float64).T
            uv.append(s[:, :2] / s[:, 2:])
        want = np.linalg.norm(uv[0] - uv[1], axis=-1).mean()
        # the distance bound with sigma in pixels: every (u, v) is a quotient of two <= 8-rounding sums, at magnitude <= max |u|, |v|
        bound = 64 * pes.ULP * max(np.abs(uv[0]).max(), np.abs(uv[1]).max())
        assert abs(out["proj_error"][i] - want) <= bound


def test_non_finite_poses_give_nan_and_minus_one():
    rng = np.random.RandomState(1)
    pts = _object_points(rng, 20)[None]
    ids = np.zeros(3, np.int32)
    T_gt = pes.random_poses(rng, 3)
    T_pred = pes.perturbed(rng, T_gt)
    T_pred[1, 0, 3] = np.nan
    T_pred[2, 1, 1] = np.inf
    syms = _sym_set(4)[None]
    out = pes.sym(T_pred, T_gt, syms, None, pts, ids)
    assert out["idx"][0] >= 0 and np.isfinite(out["err"][0])
    assert np.all(out["idx"][1:] == -1) and np.all(np.isnan(out["err"][1:])) and np.all(np.isnan(out["errs"][1:])) and np.all(np.isnan(out["T_gt_sym"][1:]))
    nn = pes.nn(T_pred, T_gt, pts, ids)
    assert np.all(nn["assign"][0] >= 0) and np.all(nn["assign"][1:] == -1) and np.all(np.isnan(nn["mean"][1:])) and np.all(np.isnan(nn["max"][1:]))
    rg = pes.rigid(T_gt, T_pred)
    assert np.isfinite(rg["rot_err_deg"][0]) and np.all(np.isnan(rg["rot_err_deg"][1:])) and np.all(np.isnan(rg["trans_err"][1:]))
