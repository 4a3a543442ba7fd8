"""CPU: the contract of the VSD and MSPD arithmetic (megapose6d_amd/csrc/vsd_core.h, the projection of pose_error_core.h) through the host
emulation (tests/vsd_emul.cpp), against hand-written counts and against an independent float64 restatement of the definitions
(tests/support/vsd.py).  Reads nothing outside the tree.

THE BORDERLINE BAND (VSD).  The emulation's counts may differ from float64's only by pixels whose compared quantity sits within
16 * 2^-24 * D_max of its threshold, D_max the row's largest distance.  With eps = 2^-24 the relative error of one rounding:
  u = ((x + 0.5) - cx) / fx     x + 0.5 is exact (x < 1024), the subtraction and the division round: 2 eps
  u*u                           2 * 2 eps + 1 eps = 5 eps; the same for v*v
  (u*u + v*v) + 1               positive terms: 5 eps + 1 eps = 6 eps, then at most 6 eps + 1 eps = 7 eps
  r = sqrtf(.)                  the square root halves: 3.5 eps + 1 eps = 4.5 eps
  dist = depth * r              5.5 eps, relative to a distance <= D_max
  dist_a - dist_b               5.5 eps (dist_a + dist_b) + 1 eps |dist_a - dist_b| <= 12 eps D_max
so 12 roundings' worth on the compared difference, as the issue counts; delta is the same fp32 value on both sides, thr_t = tau_t *
diameter adds one rounding of a threshold that the cases keep below D_max: 13 eps D_max <= the band of 16.  float64's own error is
2^-29 times that.  dist > 0 and dist_test == 0 are exact on both sides (a positive depth times r >= 1).

THE GUARD.  In every seeded case n_inter >= 1000 and the borderline pixels, summed over all counters, are at most 1 % of n_inter
(measured from the float64 restatement alone: 0.1 - 0.3 % on the 240 x 320 scene, a borderline pixel of a visibility test
counting once in each of the 2 + n_tau counters), so the rule cannot hide a wrong count.  The 1 x 1 map has
no thousand pixels: it is held to exact equality instead (its scene has no borderline pixel).

THE MSPD BOUND.  With f = max(fx, fy), U the largest pixel coordinate of the image, sigma = the largest |translation| + 2 x the
bounding radius (so that every sum of |T_kj p_j| is <= sigma) and z_min the smallest camera-frame depth of a point:
  P = K T[:3]                   three products accumulated by fmaf: |dP_0j| <= 3 eps (f + U) |T|; row 2 of K is (0 0 1): exact
  su = P_0 . (x y z 1)          three fmaf: 3 eps more on a sum of magnitudes <= (f + U) sigma      -> |d su| <= 6 eps (f + U) sigma
  sw = P_2 . (x y z 1)          |d sw| <= 3 eps sigma
  u = su / sw                   |d u| <= |d su| / z + |u| |d sw| / z + eps |u| <= eps (9 (f + U) sigma / z_min + U)
  du = u_a - u_b                twice that + eps |du| (|du| <= 2 U)                               -> eps (18 (f + U) sigma / z_min + 4 U)
  sqrtf(fmaf(dv, dv, du * du))  sqrt(2) x the coordinate error + 3 eps |d| (|d| <= 2 sqrt(2) U)    -> eps (25.5 (f + U) sigma / z_min + 14.2 U)
A maximum over points moves by at most the largest movement of a term, so |err_emul - err_f64| <= 2^-24 (32 (f + U) sigma / z_min +
16 U): k = 32, c = 16, with (f + U) where the issue expected f (1 + tan theta_max) because the principal point enters the products of
P = K T (U ~ cx + f tan theta_max).  Cases keep z_min >= 0.2 m.  The largest observed multiple is printed (and recorded in DESIGN 3.8).
"""
import numpy as np
import pytest

from support import pose_error as pes
from support import vsd as vs

TAUS10 = vs.DEFAULT_TAUS
_K, scene, taus_of, mspd_case = vs.intrinsics, vs.scene, vs.taus_of, vs.mspd_case


def _both(est, gt, test, K, diameter, on_threshold=False, **kw):
    """emulation and float64 on the same inputs; the hand-made cases have no borderline pixel, so the two must agree exactly (the
    exact-hit cases sit ON a threshold with operands that are binary fractions: there every operation is exact in both)"""
    a = vs.vsd(est, gt, test, K, diameter, **kw)
    r = vs.f64_vsd(est, gt, test, K, diameter, **kw)
    assert np.array_equal(a["counts"], r["counts"])
    ok = r["counts"][:, 0] >= 0
    assert on_threshold or np.all(r["borderline"][ok] == 0)
    assert np.array_equal(np.isnan(a["errs"]), np.isnan(r["errs"])) and np.allclose(a["errs"][ok], r["errs"][ok], rtol=2.0 ** -23, atol=0)
    return a


def _patch(h, w, y0, y1, x0, x1, z):
    m = np.zeros((1, h, w), np.float32)
    m[0, y0:y1, x0:x1] = z
    return m


K8 = _K(100.0, 4.0, 4.0)[None]
D02 = np.array([0.2], np.float32)


def test_identical_renders_unoccluded_score_zero():
    gt = _patch(8, 8, 2, 6, 2, 6, 1.0)
    for test in (gt.copy(), np.zeros_like(gt)):          # observed at the surface / not observed at all (bop19: visible)
        out = _both(gt.copy(), gt, test, K8, D02)
        assert list(out["counts"][0]) == [16, 16] + [0] * 10 and np.all(out["errs"] == 0)


def test_disjoint_masks_score_one():
    gt, est = _patch(8, 8, 2, 6, 0, 3, 1.0), _patch(8, 8, 2, 6, 4, 8, 1.0)
    out = _both(est, gt, np.zeros_like(gt), K8, D02)
    assert list(out["counts"][0]) == [28, 0] + [0] * 10 and np.all(out["errs"] == 1)


def test_plane_displaced_in_depth_steps_between_the_neighbouring_taus():
    gt, est = _patch(8, 8, 2, 6, 2, 6, 1.0), _patch(8, 8, 2, 6, 2, 6, 1.025)
    out = _both(est, gt, np.zeros_like(gt), K8, D02)     # 0.025 / 0.2 = 0.125: far for tau 0.05 and 0.10, not from 0.15 on (r <= 1.0005)
    assert list(out["counts"][0]) == [16, 16, 16, 16] + [0] * 8
    assert list(out["errs"][0]) == [1.0, 1.0] + [0.0] * 8
    # not normalised: thr = tau itself, every tau >= 0.05 is beyond 0.025
    out = _both(est, gt, np.zeros_like(gt), K8, D02, normalized=False)
    assert np.all(out["errs"] == 0)


def test_an_occluder_removes_pixels_from_vis_gt_and_the_estimate_passes_only_its_own_test():
    gt = _patch(8, 8, 2, 6, 2, 6, 1.0)
    test = gt.copy()
    test[0, 2:6, 2:4] = 0.9                               # nearer than gt by 0.1 > delta on 8 of the 16 pixels
    out = _both(gt.copy(), gt, test, K8, D02)             # the estimate is as far behind the occluder: hidden there too
    assert list(out["counts"][0]) == [8, 8] + [0] * 10 and np.all(out["errs"] == 0)
    est = gt.copy()
    est[0, 2:6, 2:4] = 0.91                               # within delta of the occluder: visible by its own test, gt is not
    out = _both(est, gt, test, K8, D02)
    assert list(out["counts"][0]) == [16, 8] + [0] * 10 and np.all(out["errs"] == 0.5)
    est[0, 2:6, 2:4] = 0.8                                # in front of the occluder (negative difference <= delta): visible
    out = _both(est, gt, test, K8, D02)
    assert list(out["counts"][0]) == [16, 8] + [0] * 10
    # vis_gt lends visibility to the estimate: behind the observed surface by more than delta, but gt is visible there
    est2 = _patch(8, 8, 2, 6, 2, 6, 1.1)
    out = _both(est2, gt, gt.copy(), K8, D02)
    assert list(out["counts"][0][:2]) == [16, 16] and list(out["errs"][0]) == [1.0] * 10       # 0.1 / 0.2 = 0.5 >= every tau


def test_empty_union_scores_one():
    z = np.zeros((1, 8, 8), np.float32)
    out = _both(z, z, _patch(8, 8, 0, 8, 0, 8, 1.0), K8, D02)
    assert list(out["counts"][0]) == [0] * 12 and np.all(out["errs"] == 1)


def test_exact_hits_on_delta_and_on_the_threshold():
    K1 = _K(50.0, 0.5, 0.5)[None]                          # a 1 x 1 map whose ray is the optical axis: r = 1 exactly
    one = lambda z: np.full((1, 1, 1), z, np.float32)      # noqa: E731
    d = np.array([0.5], np.float32)
    # dist_gt - dist_test == delta exactly (0.25, 0.75 and 1 are binary fractions): visible; one ulp further: not
    out = _both(one(1.0), one(1.0), one(0.75), K1, d, on_threshold=True, delta=0.25, taus=[0.5])
    assert list(out["counts"][0]) == [1, 1, 0]
    out = _both(one(1.0), one(1.0), one(np.float32(0.75) - np.float32(2.0 ** -24)), K1, d, on_threshold=True, delta=0.25, taus=[0.5])
    assert list(out["counts"][0]) == [0, 0, 0] and out["errs"][0, 0] == 1
    # |dist_gt - dist_est| == thr exactly (0.5 * 0.5): far; one ulp nearer: not
    out = _both(one(0.75), one(1.0), one(0.0), K1, d, on_threshold=True, taus=[0.5])
    assert list(out["counts"][0]) == [1, 1, 1] and out["errs"][0, 0] == 1
    out = _both(one(np.float32(0.75) + np.float32(2.0 ** -24)), one(1.0), one(0.0), K1, d, on_threshold=True, taus=[0.5])
    assert list(out["counts"][0]) == [1, 1, 0] and out["errs"][0, 0] == 0


def test_nan_negative_and_infinite_observed_depths_behave_as_zero():
    gt, est = _patch(8, 8, 2, 6, 2, 6, 1.0), _patch(8, 8, 2, 6, 3, 7, 1.037)
    ref = _both(est, gt, np.zeros_like(gt), K8, D02)
    for bad in (np.nan, -1.0, np.inf, -np.inf):
        out = _both(est, gt, np.full_like(gt, bad), K8, D02)
        assert np.array_equal(out["counts"], ref["counts"]) and np.array_equal(out["errs"], ref["errs"])


def test_invalid_rows_give_nan_and_minus_one():
    gt = np.repeat(_patch(8, 8, 2, 6, 2, 6, 1.0), 6, axis=0)
    K = np.repeat(K8, 6, axis=0)
    K[1, 0, 0] = np.nan
    K[2, 2, 1] = np.inf
    diam = np.array([0.2, 0.2, 0.2, 0.0, -0.1, np.inf], np.float32)
    out = _both(gt.copy(), gt, gt.copy(), K, diam)
    assert np.all(out["counts"][1:] == -1) and np.all(np.isnan(out["errs"][1:]))
    assert list(out["counts"][0]) == [16, 16] + [0] * 10 and np.all(out["errs"][0] == 0)


# --------------------------------------------------------------------------------------------------------------------------------
def check_against_f64(c, got, n_tau, delta=0.015, guard=True):
    r = vs.f64_vsd(c["est"], c["gt"], c["test"], c["K"], c["diam"], delta=delta, taus=taus_of(n_tau), gt_ids=c["gt_ids"], im_ids=c["im_ids"])
    assert np.all(np.array(taus_of(n_tau)).max() * c["diam"] <= r["d_max"])            # thr < D_max: the band's last rounding
    diff = np.abs(got["counts"].astype(np.int64) - r["counts"])
    print(f"counts differ from float64 at {int(diff.sum())} of {int(r['counts'][:, 1].sum())} intersection pixels; borderline "
          f"{int(r['borderline'].sum())} ({100.0 * r['borderline'].sum() / max(1, r['counts'][:, 1].sum()):.4f} % of n_inter)")
    assert np.all(diff <= r["borderline"])
    if guard:
        assert np.all(r["counts"][:, 1] >= 1000), r["counts"][:, 1].min()
        assert np.all(r["borderline"].sum(1) <= 0.01 * r["counts"][:, 1])
    else:
        assert np.all(r["borderline"] == 0) and np.all(diff == 0)
    # err_t is one division of the counts the emulation found
    n_un, n_in, n_far = got["counts"][:, :1].astype(np.float64), got["counts"][:, 1:2].astype(np.float64), got["counts"][:, 2:].astype(np.float64)
    want = np.where(n_un == 0, 1.0, (n_far + (n_un - n_in)) / np.maximum(n_un, 1)).astype(np.float32)
    assert np.array_equal(got["errs"], want)
    assert np.any(got["errs"] > 0) and np.any(got["errs"] < 1)
    return r


@pytest.mark.parametrize("b,h,w,n_tau,share", [(3, 37, 53, 10, False), (4, 37, 53, 16, True), (2, 96, 128, 1, False), (5, 120, 160, 10, True)])
def test_emulation_against_float64_on_seeded_maps(b, h, w, n_tau, share):
    # (on a 37 x 53 map with 16 taus ONE pixel on the edge of a visibility test already counts 18 times against a guard of 13: that
    # case's seed is one whose float64 restatement alone has no such pixel -- the scene changes, the cap does not)
    c = scene(10 * b + n_tau + (1 if n_tau == 16 else 0), b, h, w, n_im=2 if share else None, n_gt=2 if share else None, share=share)
    got = vs.vsd(c["est"], c["gt"], c["test"], c["K"], c["diam"], taus=taus_of(n_tau), gt_ids=c["gt_ids"], im_ids=c["im_ids"])
    check_against_f64(c, got, n_tau)


def test_the_float64_restatement_alone_keeps_the_borderline_share_small():
    """the guard's premise, measured before it is relied on: borderline pixels are a tiny share of the intersection"""
    c = scene(77, 3, 240, 320)
    r = vs.f64_vsd(c["est"], c["gt"], c["test"], c["K"], c["diam"])
    share = r["borderline"].sum(1) / r["counts"][:, 1]
    print("borderline share of n_inter per row:", share)
    assert np.all(r["counts"][:, 1] >= 1000) and np.all(share <= 0.01)


def test_one_by_one_map_against_float64():
    K = _K(50.0, 0.3, 0.6)[None]
    one = lambda z: np.full((1, 1, 1), z, np.float32)      # noqa: E731
    c = dict(est=one(1.04), gt=one(1.0), test=one(1.001), K=K, diam=np.array([0.23], np.float32), gt_ids=None, im_ids=None)
    got = vs.vsd(c["est"], c["gt"], c["test"], c["K"], c["diam"])
    r = vs.f64_vsd(c["est"], c["gt"], c["test"], c["K"], c["diam"])
    assert np.all(r["borderline"] == 0) and np.array_equal(got["counts"], r["counts"])
    assert list(got["counts"][0]) == [1, 1, 1, 1, 1] + [0] * 7                         # 0.04 / 0.23 = 0.174: far up to tau 0.15


# --------------------------------------------------------------------------------------------------------------------------------
# MSPD
# --------------------------------------------------------------------------------------------------------------------------------
def mspd_f64_rows(c, U=640.0):
    """per row: float64 errs over the row's symmetry set and the derived bound"""
    rows = []
    for i in range(len(c["ids"])):
        m = c["ids"][i]
        P = c["pts"][m, : c["n_points"][m]]
        e64, z_min = vs.f64_mspd_errs(c["T_pred"][i], c["T_gt"][i], c["syms"][m, : c["n_sym"][m]], P, c["K"][i])
        sigma = max(np.abs(c["T_pred"][i][:3, 3]).max(), np.abs(c["T_gt"][i][:3, 3]).max(), np.abs(c["syms"][m][:, :3, 3]).max()) \
            + 2.0 * np.linalg.norm(P.astype(np.float64), axis=-1).max()
        assert z_min >= 0.2
        rows.append((e64, vs.mspd_bound(c["K"][i], float(sigma), z_min, U)))
    return rows


@pytest.mark.parametrize("b,N,S,n_mesh,ragged", [(1, 1, 1, 1, False), (5, 63, 2, 1, False), (4, 1500, 64, 3, True), (24, 500, 8, 1, False)])
def test_mspd_emulation_against_float64(b, N, S, n_mesh, ragged):
    c = mspd_case(b, N, S, seed=300 + N, n_mesh=n_mesh, ragged=ragged)
    got = vs.mspd(c["T_pred"], c["T_gt"], c["syms"], c["n_sym"], c["pts"], c["K"], c["ids"], c["n_points"])
    worst, clear = 0.0, 0
    for i, (e64, bound) in enumerate(mspd_f64_rows(c)):
        ns = len(e64)
        assert np.all(np.abs(got["errs"][i, :ns] - e64) <= bound) and np.all(np.isposinf(got["errs"][i, ns:]))
        worst = max(worst, float(np.abs(got["errs"][i, :ns] - e64).max() / bound))
        assert abs(got["err"][i] - e64.min()) <= bound
        srt = np.sort(e64)
        if ns == 1 or srt[1] - srt[0] > 2 * bound:
            clear += 1
            assert got["idx"][i] == int(np.argmin(e64))
        else:
            assert e64[got["idx"][i]] - e64.min() <= 2 * bound
        G = (c["T_gt"][i].astype(np.float64) @ c["syms"][c["ids"][i], got["idx"][i]].astype(np.float64))
        assert np.abs(got["T_gt_sym"][i] - G).max() <= 8 * vs.ULP * 2.0
    assert clear >= 0.9 * b
    print(f"mspd ({b},{N},{S}): largest |emulation - float64| = {worst:.4f} x the bound = {worst * vs.MSPD_K:.3f} in units of the k term")


def test_mspd_lowest_index_wins_a_tie_and_non_finite_poses_give_nan():
    c = mspd_case(4, 200, 4, seed=9)
    c["syms"][0, 2] = c["syms"][0, 1]                        # an exact duplicate: index 1 must win over 2
    c["T_pred"] = np.stack([(c["T_gt"][i].astype(np.float64) @ c["syms"][0, 1].astype(np.float64)).astype(np.float32) for i in range(4)])
    c["T_pred"][1, 0, 3] = np.nan
    c["T_gt"][2, 1, 1] = np.inf
    got = vs.mspd(c["T_pred"], c["T_gt"], c["syms"], c["n_sym"], c["pts"], c["K"], c["ids"], c["n_points"])
    assert list(got["idx"]) == [1, -1, -1, 1]
    assert np.all(np.isnan(got["err"][1:3])) and np.all(np.isnan(got["errs"][1:3])) and np.all(np.isnan(got["T_gt_sym"][1:3]))
    assert got["errs"][0, 1] == got["errs"][0, 2] and got["err"][0] <= 0.01


def test_mspd_uses_the_projection_of_the_rigid_launch():
    """one formula: the mean form of the projected error over a one-element symmetry set is proj_error of the rigid emulation"""
    c = mspd_case(6, 400, 1, seed=11)
    mean = vs.mspd(c["T_pred"], c["T_gt"], c["syms"], c["n_sym"], c["pts"], c["K"], c["ids"], c["n_points"], reduce_max=False)
    rig = pes.rigid(c["T_pred"], c["T_gt"], c["K"], c["pts"], c["ids"], c["n_points"])
    assert np.array_equal(mean["err"].view(np.uint32), rig["proj_error"].view(np.uint32))
