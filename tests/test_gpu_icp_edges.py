"""-m gpu: the two on-device depth refiners (csrc/icp_nn.hip, csrc/icp.hip) on the analytic cases of tests/support/icp_cases.py -- small
and odd frames, per-frame intrinsics, rows out of frame order, point counts on their boundaries, holes / non-finite / boundary pixels,
n_iterations / n_levels / tolerance other than (100, 4, 0.05), an over-capacity mask, masks of 65 of 259 pixels, all and none (the
ordered compaction's edges), an uninitialised workspace -- through the engine
entry, against the CPU restatements.  tests/test_icp_cases_cpu.py shows on the restatements alone that every case reaches the edge it
is named after and that the reference's choice of solver (SVD against the device's Cholesky) moves no pose by more than 1e-7.

What the nearest-neighbour cases found is in the docstring of test_nn_refiner_matches_the_restatement."""
import numpy as np
import pytest
import torch

from tests.support import icp_cases as ic

pytestmark = pytest.mark.gpu


def _dev(c):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    K = t(c.K)
    im_ids = t(c.im_ids)
    return t(c.depth), im_ids, t(c.rend), K, K[im_ids.long()].contiguous(), t(c.TCO)


def _engine_nn(c):
    from megapose6d_amd import engine as eng

    depth, im_ids, rend, K, K_rows, TCO = _dev(c)
    p = c.params
    out = eng.icp_refine(depth, im_ids, rend, K, K_rows, TCO, p["n_iterations"], p["n_levels"], p["tolerance"], p["n_min_points"], association="nn",
                         return_iters=True, masks=None if c.masks is None else torch.from_numpy(c.masks).cuda())
    return [o.cpu().numpy() for o in out]


def _engine_projective(c, user_masks):
    from megapose6d_amd import engine as eng

    depth, im_ids, rend, K, K_rows, TCO = _dev(c)
    p = c.params
    out = eng.icp_refine(depth, im_ids, rend, K, K_rows, TCO, p["n_iterations"], p["n_levels"], p["tolerance"], p["n_min_points"], user_masks=user_masks,
                         association="projective")
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("name", ic.NN_CASE_NAMES)
def test_nn_refiner_matches_the_restatement(name):
    """association="nn", every row against oracle/icp_opencv.py on that row's own frame and K, with the bounds of
    test_default_refiner_is_the_reference_algorithm_step_for_step_on_12_scenes: equal retval, equal iterations on all n_levels levels (zero
    past them), residual within 1e-6 * max(1, |res|), pose within 1e-6, a rejected row's input pose bit for bit, a second call
    bit-identical.

    Measured on the device: every case bit-identical to the restatement (max |pose - restatement| 0 on every accepted row).  Before
    icp_nn.hip skipped the levels that OpenCV's `while` never enters, five cases failed, each with equal retval but other iterations
    (restatement -> device) and a pose off by up to 2.7e-2:
      param_it2_lv4   [2, 1, 1, 0] -> [0, 1, 1, 1]                              pose 2.7e-2
      param_it1_lv4   [1, 0, 0, 0] -> [0, 0, 0, 1]                              pose 2.1e-2
      param_it3_lv8   [3, 2, 1, 1, 0, 0, 0, 0] -> [0, 2, 1, 1, 1, 1, 1, 1]      pose 2.5e-2
      param_it100_lv8 [100, 2, 2, 2, 0, 0, 0, 0] -> [2, 2, 2, 2, 1, 1, 1, 1]    pose 3.1e-3
      param_tol0.2    [6, 4, 0, 0] -> [24, 2, 1, 1]                             pose 7.0e-3
    (a level whose cap rounds to 0, or whose stop band tolerance * (level + 1)^2 > 1 already holds, ran one pass; in the first three
    the enqueued train then ended before level 0 did, the row never retired and its pose stayed in the normalised frame)."""
    c, ref = ic.nn_case(name), ic.nn_reference(name)
    T, retval, residual, iters = _engine_nn(c)
    again = _engine_nn(c)
    for a, b in zip((T, retval, residual, iters), again):
        assert np.array_equal(a, b, equal_nan=True), name                        # deterministic
    nl = c.params["n_levels"]
    worst = 0.0
    for row, r in enumerate(ref):
        if r is None:                                                            # more mask pixels than the search can index: rejected up front
            assert retval[row] == -1 and residual[row] == -1.0 and np.array_equal(T[row], c.TCO[row]) and not iters[row].any(), (name, row)
            continue
        err = float(np.abs(T[row].astype(np.float64) - r["T"]).max())
        line = (name, row, r["retval"], int(retval[row]), r["residual"], float(residual[row]), r.get("iters"), iters[row].tolist(), err)
        print(line)
        assert retval[row] == r["retval"], line
        assert iters[row, :nl].tolist() == r.get("iters", [0] * nl) and not iters[row, nl:].any(), line
        assert abs(float(residual[row]) - r["residual"]) <= 1e-6 * max(1.0, abs(r["residual"])), line
        if r["retval"] == 0:
            worst = max(worst, err)
            assert err <= 1e-6, line
        else:
            assert np.array_equal(T[row], c.TCO[row]), line
    print(f"{name}: max |pose - restatement| over the accepted rows {worst:.3e}")


@pytest.mark.parametrize("name", ic.PROJECTIVE_CASE_NAMES)
def test_projective_refiner_matches_its_oracle(name):
    """association="projective" against oracle/icp.py with the bounds of test_icp_refiner_vs_oracle_and_ground_truth: equal retval, pose
    within 2e-4, residual within 1e-4, a rejected row's input pose bit for bit, a second call bit-identical"""
    c, um = ic.projective_case(name)
    ref = ic.projective_reference(name)
    T, retval, residual = _engine_projective(c, um)
    for a, b in zip((T, retval, residual), _engine_projective(c, um)):
        assert np.array_equal(a, b), name
    worst_T = worst_r = 0.0
    for row, r in enumerate(ref):
        err = float(np.abs(T[row].astype(np.float64) - r["T"]).max())
        line = (name, row, r["retval"], int(retval[row]), r["residual"], float(residual[row]), err)
        print(line)
        assert retval[row] == r["retval"], line
        if r["retval"] == 0:
            worst_T, worst_r = max(worst_T, err), max(worst_r, abs(float(residual[row]) - r["residual"]))
            assert err < 2e-4 and abs(float(residual[row]) - r["residual"]) < 1e-4, line
        else:
            assert np.array_equal(T[row], c.TCO[row]), line
            if ic.projective_count(c, row, um) < c.params["n_min_points"]:
                assert residual[row] == -1.0, line
    print(f"{name}: max |pose - oracle| {worst_T:.3e}, max |residual - oracle| {worst_r:.3e}")


@pytest.mark.parametrize("association", ["nn", "projective"])
def test_refiners_read_nothing_of_the_workspace_they_have_not_written(association):
    """engine.icp_refine hands the kernels a torch.empty workspace.  The batch case (rows rejected up front, rows that retire early) run
    through the C entry on a workspace of the reported size filled with 0xFF and then with 0x00: bit-identical outputs, equal to the
    engine's, and the 4,096 bytes behind the reported size untouched."""
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    lib = _lib.load()
    c = ic.batch_case()
    depth, im_ids, rend, K, K_rows, TCO = _dev(c)
    B, H, W = c.depth.shape
    N = len(c.im_ids)
    p = c.params
    nn = association == "nn"
    want = _engine_nn(c) if nn else _engine_projective(c, False)
    n_bytes = (lib.mp_icp_nn_workspace_bytes if nn else lib.mp_icp_workspace_bytes)(B, N, H, W)
    runs = []
    for fill in (0xFF, 0x00):
        ws = torch.full((n_bytes + 4096,), fill, dtype=torch.uint8, device="cuda")
        ws[n_bytes:] = 0xA5
        out = torch.empty_like(TCO)
        retval = torch.empty(N, dtype=torch.int32, device="cuda")
        residual = torch.empty(N, dtype=torch.float32, device="cuda")
        if nn:
            iters = torch.zeros(N, 8, dtype=torch.int32, device="cuda")
            _lib.check(lib.mp_icp_refine_nn(depth.data_ptr(), B, im_ids.data_ptr(), rend.data_ptr(), K.data_ptr(), K_rows.data_ptr(), TCO.data_ptr(), N, H, W,
                                            p["n_iterations"], p["n_levels"], p["tolerance"], p["n_min_points"], None, out.data_ptr(), retval.data_ptr(),
                                            residual.data_ptr(), iters.data_ptr(), ws.data_ptr(), n_bytes, eng._stream()))
            got = [out, retval, residual, iters]
        else:
            _lib.check(lib.mp_icp_refine(depth.data_ptr(), B, im_ids.data_ptr(), rend.data_ptr(), K.data_ptr(), K_rows.data_ptr(), TCO.data_ptr(), N, H, W,
                                         p["n_iterations"], p["n_levels"], p["tolerance"], p["n_min_points"], 0, out.data_ptr(), retval.data_ptr(),
                                         residual.data_ptr(), ws.data_ptr(), n_bytes, eng._stream()))
            got = [out, retval, residual]
        torch.cuda.synchronize()
        assert bool((ws[n_bytes:] == 0xA5).all()), (association, fill)
        runs.append([g.cpu().numpy() for g in got])
    for a, b, w in zip(runs[0], runs[1], want):
        assert np.array_equal(a, b) and np.array_equal(a, w), association
