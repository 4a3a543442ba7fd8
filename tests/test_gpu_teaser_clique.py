"""GPU: the maximum-clique search (csrc/teaser_clique.hip) through engine.max_clique, teaser_solve and teaser_refine against the host
emulation of the same rule (tests/teaser_clique_emul.cpp), bit for bit: members, info and steps.  One launch at stride 70 with rows of
1 to 70 vertices (the word and wave edges, the counter-example of the k-core rule), one at stride 1024 (bits above 992, the full LDS
footprint, a search of about 1e5 steps), a row that exhausts its budget, rows of a batch against the same rows alone and permuted,
the refiner's two entry points in the new mode, and the refusals."""
import numpy as np
import pytest
import torch

from support import teaser as ts
from support import teaser_clique as tc

pytestmark = pytest.mark.gpu


def _t(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _same(got: torch.Tensor, want: np.ndarray, what):
    g = got.cpu().numpy()
    assert g.shape == want.shape and g.dtype == want.dtype, (what, g.shape, want.shape, g.dtype, want.dtype)
    if g.dtype.kind == "f":
        assert np.array_equal(g.view(np.uint64 if g.dtype == np.float64 else np.uint32), np.ascontiguousarray(want).view(np.uint64 if g.dtype == np.float64 else np.uint32)), what
    else:
        assert np.array_equal(g, want), (what, int((g != want).sum()), g[g != want][:8], want[g != want][:8])


@pytest.mark.parametrize("which", ("stride70", "stride1024"))
def test_search_matches_the_emulation(which):
    from megapose6d_amd import engine as eng

    a, counts = tc.stride70_rows() if which == "stride70" else tc.stride1024_rows()
    want_members, want_info = tc.emul_rows(which)
    members, info = eng.max_clique(_t(a, torch.uint8), _t(counts, torch.int32), tc.FULL_BUDGET)
    print(which, "info", info.cpu().numpy().tolist())
    _same(info, want_info, "info")
    _same(members, want_members, "members")
    assert want_info[:, 2].all() and want_info[:, 3].max() > (10000 if which == "stride70" else 50000) and (want_info[:, 3] == 0).any()
    if which == "stride1024":
        assert want_members[0].max() > 992 and want_info[0].tolist() == [300, 300, 1, 0]


def test_budget_row_and_permuted_batches():
    from megapose6d_amd import engine as eng

    a = tc.gnp(*tc.BUDGET_GRAPH)
    for budget in (tc.SMALL_BUDGET, 0, tc.FULL_BUDGET):
        want_members, want_info = tc.emul_max_clique(a, None, budget)
        members, info = eng.max_clique(_t(a[None], torch.uint8), None, budget)
        _same(info, want_info, ("info", budget))
        _same(members, want_members, ("members", budget))
        assert want_info[0, 2] == (1 if budget == tc.FULL_BUDGET else 0)
    # the rows of a batch equal the same rows launched alone and in another order (a float adjacency: any non-zero is an edge)
    rows, counts = tc.stride70_rows()
    want_members, want_info = tc.emul_rows("stride70")
    order = np.asarray([5, 8, 0, 2, 7, 1, 6, 3, 4])
    members, info = eng.max_clique(_t(rows[order] * 0.5), _t(counts[order], torch.int32), tc.FULL_BUDGET)
    _same(info, want_info[order], "permuted info")
    _same(members, want_members[order], "permuted members")
    for r in (2, 8):
        members, info = eng.max_clique(_t(rows[r: r + 1], torch.uint8), _t(counts[r: r + 1], torch.int32), tc.FULL_BUDGET)
        _same(info, want_info[r: r + 1], ("alone info", r))
        _same(members, want_members[r: r + 1], ("alone members", r))
    # more rows than the grid has workgroups (256): a workgroup takes several rows, one after the other, on one search stack
    rep = np.tile(np.arange(9), 34)[:300]
    members, info = eng.max_clique(_t(rows[rep], torch.uint8), _t(counts[rep], torch.int32), tc.FULL_BUDGET)
    _same(info, want_info[rep], "300 rows info")
    _same(members, want_members[rep], "300 rows members")


@pytest.mark.parametrize("graph", ("chain", "complete"))
def test_solve_matches_the_emulation_in_the_new_mode(graph):
    from megapose6d_amd import engine as eng

    stride = 200
    S, D = np.zeros((len(ts.SOLVE_CASES) + 1, stride, 3), np.float32), np.zeros((len(ts.SOLVE_CASES) + 1, stride, 3), np.float32)
    counts = []
    for r, case in enumerate(ts.SOLVE_CASES + ((2, 0.0, 7),)):
        src, dst, _, _, _ = ts.correspondences(*case)
        S[r, : len(src)], D[r, : len(src)] = src, dst
        counts.append(len(src))
    want = tc.emul_solve(S, D, counts, min_num_inliers=25, inlier_selection="max_clique", rotation_tim_graph=graph)
    Rt, retval, tel = eng.teaser_solve(_t(S), _t(D), _t(counts, torch.int32), ts.NOISE_BOUND, 25, "max_clique", graph, telemetry=True,
                                       max_clique_steps=tc.FULL_BUDGET)
    _same(retval, want["retval"], "retval")
    for key in ("clique", "info", "degree", "core", "selected"):
        _same(tel[key], want[key], key)
    _same(Rt, want["Rt"], "Rt")
    assert want["retval"].tolist()[-1] == -1 and 0 in want["retval"].tolist() and want["clique"][:, 2].all()
    plain = eng.teaser_solve(_t(S), _t(D), _t(counts, torch.int32), ts.NOISE_BOUND, 25, "max_clique", graph, max_clique_steps=tc.FULL_BUDGET)
    assert len(plain) == 2 and torch.equal(plain[0], Rt) and torch.equal(plain[1], retval)
    # the other selections return what they returned: no new key
    assert set(eng.teaser_solve(_t(S), _t(D), _t(counts, torch.int32), ts.NOISE_BOUND, 25, "kcore", graph, telemetry=True)[2]) == {"degree", "core", "selected", "info"}


def test_refine_matches_the_emulation_in_the_new_mode():
    from megapose6d_amd import engine as eng

    frames, kw = ts.FRAME_CASES["tiny"]
    meas, im_ids, rend, K, TCO = ts.frame_case(*frames)
    want = tc.emul_refine(meas, im_ids, rend, K, TCO, **kw)
    out, retval, info, tel = eng.teaser_refine(_t(meas), _t(im_ids, torch.int32), _t(rend), _t(K), _t(TCO), noise_bound=ts.NOISE_BOUND, telemetry=True,
                                               inlier_selection="max_clique", max_clique_steps=tc.FULL_BUDGET, **kw)
    _same(info, want["info"], "info")
    _same(retval, want["retval"], "retval")
    for key in ("clique", "sample_idx", "degree", "core", "selected", "Rt"):
        _same(tel[key], want[key], key)
    _same(out, want["TCO"], "TCO")
    plain = eng.teaser_refine(_t(meas), _t(im_ids, torch.int32), _t(rend), _t(K), _t(TCO), noise_bound=ts.NOISE_BOUND, inlier_selection="max_clique",
                              max_clique_steps=tc.FULL_BUDGET, **kw)
    assert len(plain) == 3 and torch.equal(plain[0], out) and torch.equal(plain[1], retval) and torch.equal(plain[2], info)


def test_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import engine as eng

    default, ceiling = eng.max_clique_step_limits()
    assert ceiling == 16 * default == tc.limits()["step_ceiling"]
    a = torch.zeros(2, 8, 8, dtype=torch.uint8).cuda()
    for kw in (dict(max_steps=-1), dict(max_steps=ceiling + 1), dict(adjacency=torch.zeros(2, 1025, 1025, dtype=torch.uint8).cuda()),
               dict(adjacency=torch.zeros(2, 8, 7, dtype=torch.uint8).cuda()), dict(counts=torch.zeros(3, dtype=torch.int32).cuda())):
        with pytest.raises(eng.EngineError):
            eng.max_clique(**dict(dict(adjacency=a, max_steps=10), **kw))
    s, c = torch.zeros(2, 8, 3).cuda(), torch.zeros(2, dtype=torch.int32).cuda()
    for steps in (-1, ceiling + 1):
        with pytest.raises(eng.EngineError):
            eng.teaser_solve(s, s, c, inlier_selection="max_clique", max_clique_steps=steps)
    meas, im_ids, rend, K, TCO = (_t(x, torch.int32 if x.dtype == np.int32 else torch.float32) for x in ts.frame_case(*ts.FRAME_CASES["tiny"][0]))
    with pytest.raises(eng.EngineError):
        eng.teaser_refine(meas, im_ids, rend, K, TCO, inlier_selection="max_clique", max_clique_steps=ceiling + 1)
    # the C entries themselves
    lib = eng._lib.load()
    assert lib.mp_max_clique_workspace_bytes(2, 8) > 0 and lib.mp_max_clique_workspace_bytes(2, 1025) == 0 and lib.mp_max_clique_workspace_bytes(-1, 8) == 0
    assert lib.mp_teaser_workspace_bytes_ex(2, 0, 0, 8, 2) > lib.mp_teaser_workspace_bytes_ex(2, 0, 0, 8, 0) > 0      # only the new mode has a search stack
    assert lib.mp_teaser_workspace_bytes_ex(2, 0, 0, 8, 3) == 0 and lib.mp_teaser_workspace_bytes_ex(2, 0, 0, 1025, 2) == 0
    assert lib.mp_teaser_workspace_bytes_ex(4, 24, 32, 64, 0) == lib.mp_teaser_workspace_bytes(4, 24, 32)
    ws = torch.empty(lib.mp_max_clique_workspace_bytes(2, 8), dtype=torch.uint8).cuda()
    members, info = torch.zeros(2, 8, dtype=torch.int32).cuda(), torch.zeros(2, 4, dtype=torch.int32).cuda()

    def call(adj=a.data_ptr(), n=2, stride=8, steps=10, mem=members.data_ptr(), inf=info.data_ptr(), w=ws.data_ptr(), nbytes=ws.numel()):
        return lib.mp_max_clique(adj, None, n, stride, steps, mem, inf, w, nbytes, eng._stream())

    assert call() == 0
    for bad in (dict(steps=-1), dict(steps=ceiling + 1), dict(stride=1025), dict(stride=0), dict(mem=None), dict(inf=None), dict(adj=None), dict(w=None),
                dict(nbytes=1024), dict(n=-1)):
        assert call(**bad) != 0, bad
    # the old entry accepts the new selection with the default budget when the workspace has the new size, and refuses the old size
    Rt, rv = torch.zeros(2, 12, dtype=torch.float64).cuda(), torch.zeros(2, dtype=torch.int32).cuda()
    big = torch.empty(lib.mp_teaser_workspace_bytes_ex(2, 0, 0, 8, 2), dtype=torch.uint8).cuda()
    args = (s.data_ptr(), s.data_ptr(), c.data_ptr(), 2, 8, 0.01, 2, 0, 0, Rt.data_ptr(), rv.data_ptr(), None, None, None, None)
    assert lib.mp_teaser_solve(*args, big.data_ptr(), big.numel(), eng._stream()) == 0
    assert lib.mp_teaser_solve(*args, big.data_ptr(), lib.mp_teaser_workspace_bytes_ex(2, 0, 0, 8, 0), eng._stream()) != 0
    assert lib.mp_teaser_solve_ex(*args, -1, None, big.data_ptr(), big.numel(), eng._stream()) != 0
    assert lib.mp_teaser_solve_ex(*args, ceiling + 1, None, big.data_ptr(), big.numel(), eng._stream()) != 0
    torch.cuda.synchronize()


def test_refiner_reports_the_search():
    """TeaserppRefiner in the new mode under run_inference_pipeline: the budget is an attribute, the extra data names the search"""
    from megapose6d_amd import TeaserppRefiner
    from tests.support.scene import make_scene

    est, obs, det, gt = make_scene(n_objects=1, seed=0, SO3_grid_size=72, rgbd=True)
    est.depth_refiner = TeaserppRefiner(est.mesh_db, est.refiner_model.renderer, inlier_selection="max_clique")
    est.depth_refiner.max_clique_steps = budget = 20000
    final, extra = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=1, n_pose_hypotheses=1, run_depth_refiner=True)
    debug = est.depth_refiner.debug
    print({k: v.tolist() for k, v in debug.items()})
    assert len(final) == 1 and torch.isfinite(final.poses).all() and debug["n_mask_points"].item() > 0
    # (a dense consistency graph: the search may well run out of this budget; then it says so and has overshot by less than a node)
    exact, steps = debug["clique_exact"].item(), debug["clique_steps"].item()
    assert (exact == 1 and 0 <= steps <= budget + debug["n_points"].item()) or (exact == 0 and budget < steps <= budget + debug["n_points"].item())
    assert 0 <= debug["n_selected"].item() <= debug["n_points"].item()
    est.depth_refiner = TeaserppRefiner(est.mesh_db, est.refiner_model.renderer)
    est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=1, n_pose_hypotheses=1, run_depth_refiner=True)
    assert "clique_exact" not in est.depth_refiner.debug and set(est.depth_refiner.debug) | {"clique_exact", "clique_steps"} == set(debug)
