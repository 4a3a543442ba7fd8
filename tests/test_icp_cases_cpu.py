"""CPU: the analytic depth-refiner cases of tests/support/icp_cases.py do what their names say -- on the restatement alone
(oracle/icp_opencv.py for the nearest-neighbour refiner, oracle/icp.py for the projective one).  tests/test_gpu_icp_edges.py then runs the
same cases on the device; a case that does not reach the edge it is named after would test nothing there."""
import numpy as np
import pytest

from tests.support import icp_cases as ic

F32 = np.float32


def _in_range(d):
    return (d > F32(0.2)) & (d < F32(5.0))


@pytest.mark.parametrize("name", ic.NN_CASE_NAMES)
def test_point_counts_are_the_designed_ones(name):
    """m (scene) and n (model) points per row, counted here from the arrays, are what the restatement sees and what the case names"""
    c, ref = ic.nn_case(name), ic.nn_reference(name)
    assert [x.name for x in ic.nn_cases()] == ic.NN_CASE_NAMES
    for row, r in enumerate(ref):
        sel = ic.row_mask(c, row) & _in_range(c.depth[int(c.im_ids[row])])
        m, n = int(sel.sum()), int((sel & (c.rend[row] > 0)).sum())
        if c.m is not None:
            assert (m, n) == (c.m[row], c.n[row]), (name, row, m, n)
        if r is None:
            assert m > 1 << 18 and n > 1 << 18          # over the device's capacity: the restatement is not run
            continue
        assert (r["n_scene"], r["n_model"]) == (m, n), (name, row)
        lo = c.params["n_min_points"]
        assert (r["retval"] == -1 and r["residual"] == -1.0) == (m < lo or n < lo), (name, row, m, n)
        # OpenCV itself divides by zero when the coarsest level has no sample
        assert m < lo or n < lo or int(np.rint(n / 2.0 ** (c.params["n_levels"] - 1))) >= 1


def test_count_cases_sit_on_their_boundaries():
    ref = {(m, n): ic.nn_reference(f"count_m{m}_n{n}")[0] for m, n in ic.COUNTS}
    for key in ((199, 199), (260, 199)):                 # one point under n_min_points = 200: scene and model, model alone
        assert ref[key]["retval"] == -1 and ref[key]["residual"] == -1.0
    for key in ((200, 200), (260, 200), (1024, 1024), (1025, 1025), (1300, 1024), (1300, 1025), (1800, 600)):
        assert ref[key]["retval"] == 0, key


def test_frame_cases_reach_the_shapes_they_are_there_for():
    shapes = [ic.nn_case(n).depth.shape[1:] for n in ic.NN_CASE_NAMES if n.startswith("frame_")]
    assert shapes == [(7, 200), (17, 23), (37, 53), (64, 64), (96, 128)]
    assert shapes[0][0] < 8                              # shorter than the Gaussian radius
    assert all((h * w) % 256 and (h * w) % 1024 for h, w in shapes[:3]) and (64 * 64) % 1024 == 0
    big = ic.nn_reference("frame_96x128")[0]
    assert big["n_model"] > 2 * 512 and big["n_scene"] > 2 * 1024      # several model chunks and scene segments in the search
    for name in ic.NN_CASE_NAMES:                        # every K has a fractional principal point left of / above part of the frame
        K = ic.nn_case(name).K
        assert np.all(K[:, 0, 2] % 1 != 0) and np.all(K[:, 1, 2] % 1 != 0) and np.all(K[:, 0, 2] > 1) and np.all(K[:, 1, 2] > 1)


def test_content_cases_hold_what_they_name():
    from oracle import icp_opencv as ocv

    c = ic.nn_case("content_hole26")
    hole = c.depth[0] == 0
    assert hole[11:37, 19:45].all() and c.rend[0][11:37, 19:45].all()          # 26 x 26 > 2 x 10 fill rings, inside the object
    c = ic.nn_case("content_corner_hole")
    assert (c.depth[0][:3, :3] == 0).all() and (c.depth[0] == 0).sum() == 9 and (c.rend[0] > 0).all()
    c = ic.nn_case("content_nonfinite")
    vals = [c.depth[0][p] for p in c.notes["pixels"]]
    assert np.isnan(vals[0]) and vals[1] == F32(-0.3) and vals[2] == np.inf and vals[3] == -np.inf
    sel = ic.row_mask(c, 0)
    assert not any(sel[p] for p in c.notes["pixels"])
    # ... and the infinities are within the Gaussian's reach (8) of pixels that are used
    ys, xs = np.nonzero(sel)
    for p in c.notes["pixels"][2:]:
        assert (np.maximum(np.abs(ys - p[0]), np.abs(xs - p[1])) <= 8).any()
    c = ic.nn_case("content_range_ends")
    (a, b) = c.notes["pixels"]
    assert c.depth[0][a] == F32(0.2) and c.depth[0][b] == F32(5.0) and c.masks[0][a] and c.masks[0][b]
    assert ic.nn_reference("content_range_ends")[0]["n_scene"] == int(c.masks[0].sum()) - 2      # both excluded: the range test is strict
    c = ic.nn_case("content_tenth_exact")
    (p,) = c.notes["pixels"]
    m, r = c.depth[0][p], c.rend[0][p]
    assert m.dtype == F32 and r.dtype == F32 and F32(0.1) < r < F32(0.125) and m > F32(0.2)
    assert np.abs(m - r) == F32(0.1) and (m - r).dtype == F32                   # equal, not greater: kept
    assert np.abs(np.nextafter(m, F32(1)) - r) > F32(0.1)                        # (one ulp more would be dropped)
    assert ocv.compute_masks_threshold(c.rend[0], c.depth[0])[p]
    assert ic.nn_reference("content_tenth_exact")[0]["n_scene"] == c.m[0]            # the disc's pixels and this one


def test_the_table_covers_every_way_a_level_and_a_row_can_end():
    ends, rows = set(), []
    for name in ic.NN_CASE_NAMES:
        for r in ic.nn_reference(name):
            if r is None or "iters" not in r:
                rows.append("count" if r is not None else "capacity")
                continue
            rows.append("accepted" if r["retval"] == 0 else "residual")
            for it, end, cap in zip(r["iters"], r["ends"], r["caps"]):
                ends.add("cap0" if cap == 0 else "band0" if it == 0 and end == "stop" else end)
    # stop rule, iteration cap, `break` with fewer than 6 matches, a cap of 0, a stop band that already holds before the first pass
    assert {"stop", "cap", "few", "cap0", "band0"} <= ends, ends
    assert {"accepted", "count", "residual", "capacity"} <= set(rows)
    for key, iters in ic.ZERO_CAP_ITERS.items():
        assert ic.nn_reference("param_it%d_lv%d" % key)[0]["iters"] == iters
    assert ic.nn_reference("param_tol0.2")[0]["iters"][2:] == [0, 0]            # 0.2 * 9 and 0.2 * 16 are > 1
    none = ic.nn_reference("param_tol1.5")[0]                                   # no level iterates: rejected with the residual nothing lowered
    assert none["iters"] == [0, 0, 0, 0] and none["retval"] == -1 and none["residual"] == 9999999999.0


def test_batch_rows_differ():
    c, ref = ic.batch_case(), ic.nn_reference("batch")
    assert c.im_ids.tolist() == [2, 0, 2, 1, 0, 2] and c.depth.shape == (3, 96, 128)
    for a in range(3):
        for b in range(a + 1, 3):
            assert all(c.K[a][i] != c.K[b][i] for i in ((0, 0), (1, 1), (0, 2), (1, 2)))
            assert not np.array_equal(c.depth[a], c.depth[b])
    assert ref[1]["retval"] == -1 and ref[1]["residual"] == -1.0 and ref[1]["n_model"] < 50          # position 1: its point count
    tol = c.params["tolerance"]
    assert ref[3]["retval"] == -1 and tol < ref[3]["residual"] < 1.0                                  # by its residual, after a level 0 that ran
    accepted = [r for r in ref if r["retval"] == 0]
    assert len(accepted) == 4
    assert len({tuple(r["iters"]) for r in accepted}) == 4                                             # rows retire at different times
    # a row's answer depends on its OWN frame and K: with a neighbour's K the restatement gives another pose
    from oracle import icp_opencv as ocv

    T_wrong, _, _ = ocv.icp_refinement(c.depth[2], c.rend[0], ic.row_mask(c, 0), c.K[0], c.TCO[0], n_min_points=50)
    assert np.abs(T_wrong - ref[0]["T"]).max() > 1e-4


def _point_to_plane_cholesky(src, dst):
    """the device's solve: the 6 x 6 normal equations by Cholesky, float64; a failed factorisation is a non-finite solution (`break`)"""
    A = np.concatenate([np.cross(src[:, :3], dst[:, 3:6]), dst[:, 3:6]], axis=1)
    b = ((dst[:, :3] - src[:, :3]) * dst[:, 3:6]).sum(1)
    try:
        L = np.linalg.cholesky(A.T @ A)
    except np.linalg.LinAlgError:
        return np.full(3, np.nan), np.full(3, np.nan)
    x = np.linalg.solve(L.T, np.linalg.solve(L, A.T @ b))
    return x[:3], x[3:]


@pytest.mark.parametrize("name", ic.NN_CASE_NAMES)
def test_the_solve_is_well_conditioned_in_every_case(name, monkeypatch):
    """The device solves the normal equations by Cholesky, the restatement by an SVD least-squares solve.  Every case is run a second time
    with the restatement's solve replaced: the same verdict, the same iterations on every level, poses within 1e-7 -- a tenth of the
    bound the device is held to, so the reference's own choice of solver stays inside it."""
    from oracle import icp_opencv as ocv

    ref = ic.nn_reference(name)
    monkeypatch.setattr(ocv, "_point_to_plane", _point_to_plane_cholesky)
    for row, (a, b) in enumerate(zip(ref, ic.run_nn_oracle(ic.nn_case(name)))):
        if a is None:
            continue
        assert a["retval"] == b["retval"] and a.get("iters") == b.get("iters") and a.get("ends") == b.get("ends"), (name, row, a, b)
        err = float(np.abs(a["T"].astype(np.float64) - b["T"]).max())
        assert err <= 1e-7, (name, row, err)
        assert abs(a["residual"] - b["residual"]) <= 1e-7 * max(1.0, abs(a["residual"]))


@pytest.mark.parametrize("name", ic.PROJECTIVE_CASE_NAMES)
def test_projective_cases_are_decided_with_a_margin(name):
    """oracle/icp.py accepts or rejects by residual <= tolerance: no case may sit near that line (the device sums in float32), and the mask
    counts around n_min_points are exact"""
    c, um = ic.projective_case(name)
    assert [x.name for x, _ in ic.projective_cases()] == ic.PROJECTIVE_CASE_NAMES
    tol = c.params["tolerance"]
    for row, r in enumerate(ic.projective_reference(name)):
        cnt = ic.projective_count(c, row, um)
        assert (r["retval"] == -1 and r["residual"] == -1.0) or not (0.8 * tol <= r["residual"] <= 1.25 * tol), (name, row, r["residual"])
        if cnt < c.params["n_min_points"]:
            assert r["retval"] == -1 and r["residual"] == -1.0, (name, row)
    one = ic.projective_reference(name)[0]
    if name == "proj_min_points_count":
        assert c.params["n_min_points"] == ic.projective_count(c, 0) and one["retval"] == 0
    if name == "proj_min_points_count_plus_1":
        assert c.params["n_min_points"] == ic.projective_count(c, 0) + 1 and one["retval"] == -1
    if name == "proj_user_masks":
        assert um and one["retval"] == 0 and ic.projective_count(c, 0, True) - ic.projective_count(c, 0, False) == 288   # the 16 x 20 block, less its two masked columns
    if name in ("proj_96x128", "proj_97x131", "proj_it7_lv4", "proj_it100_lv1"):
        assert one["retval"] == 0
    if name == "batch":
        assert sorted(r["retval"] for r in ic.projective_reference(name)).count(0) >= 3
