"""CPU: the contract of the TEASER++ refiner (megapose6d_amd/csrc/teaser_core.h) on the host emulation built from that header
(tests/teaser_emul.cpp), against the independent numpy restatement of tests/support/teaser.py: sampling indices exactly, the graph
bit for bit in fp32 and against float64 outside a margin, core numbers against a sequential peel, the registration against known
transforms under 0 / 30 / 60 % outliers and against the float64 restatement, the accept rule at its threshold, and rows of one launch
against single launches.  The GPU test (tests/test_gpu_teaser.py) holds the kernels to this emulation bit for bit."""
import inspect

import numpy as np
import pytest

from support import teaser as ts

REFERENCE_SIGNATURE = ("(self, mesh_db, renderer, mask_type='simple', depth_delta_thresh=0.1, n_min_points=100, n_points=1000, noise_bound=0.01, "
                       "min_num_inliers=50, use_farthest_point_sampling=True)")   # teaserpp_refiner.py:166-177, annotations dropped


def test_constructor_is_the_references():
    from megapose6d_amd import TeaserppRefiner
    from megapose6d_amd.icp_refiner import DepthRefiner

    assert issubclass(TeaserppRefiner, DepthRefiner)
    params = list(inspect.signature(TeaserppRefiner.__init__).parameters.values())
    positional = [p for p in params if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    got = "(" + ", ".join(p.name if p.default is inspect.Parameter.empty else f"{p.name}={p.default!r}" for p in positional) + ")"
    assert got == REFERENCE_SIGNATURE
    extensions = {p.name: p.default for p in params if p.kind is inspect.Parameter.KEYWORD_ONLY}
    assert extensions == {"inlier_selection": "kcore", "rotation_tim_graph": "chain"}
    with pytest.raises(ValueError):
        TeaserppRefiner(None, None, mask_type="other")
    with pytest.raises(ValueError):
        TeaserppRefiner(None, None, n_points=1025)
    with pytest.raises(ValueError):
        TeaserppRefiner(None, None, inlier_selection="clique")


def test_load_model_names_the_refiner():
    from megapose6d_amd import TeaserppRefiner
    from megapose6d_amd import load_model as lm

    assert isinstance(lm.make_depth_refiner("teaserpp", None, None), TeaserppRefiner)
    assert lm.make_depth_refiner(None, None, None) is None
    with pytest.raises(ValueError):
        lm.make_depth_refiner("teaser", None, None)
    assert inspect.signature(lm.load_named_model).parameters["depth_refiner"].default is None


# sampling --------------------------------------------------------------------------------------------------------------------------------
def _cloud(N, seed):
    return np.random.RandomState(seed).uniform(-0.2, 0.2, size=(N, 3)).astype(np.float32) + np.float32([0, 0, 0.6])


@pytest.mark.parametrize("N", (1, 2, 63, 64, 65, 1023, 1025, 5000))
def test_sampling_equals_the_numpy_restatement(N):
    p = _cloud(N, N)
    for n_points in (1, 7, 64, 100):
        idx, m = ts.emul_fps(p[None], [N], n_points)
        want = ts.ref_fps(p, n_points)
        assert m[0] == min(n_points, N) == len(want)                                   # n_points > N gives N picks
        assert np.array_equal(idx[0, : m[0]], want) and (idx[0, m[0]:] == -1).all(), (N, n_points)
        assert len(set(want.tolist())) == len(want)
        idx, m = ts.emul_fps(p[None], [N], n_points, use_fps=False)
        assert np.array_equal(idx[0, : m[0]], ts.ref_stride(N, n_points))


def test_sampling_ties_go_to_the_lowest_index():
    g = np.arange(6, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)          # integer coordinates: every distance exact, many ties
    doubled = np.concatenate([lattice[:50], lattice[:50], lattice[:50]])                 # every point three times
    for p in (lattice, doubled):
        idx, m = ts.emul_fps(p[None], [len(p)], 64)
        want = ts.ref_fps(p, 64)
        assert np.array_equal(idx[0, : m[0]], want)
    # by hand: from corner 0 the farthest lattice point is the opposite corner; all duplicates of one point -> the lowest index again and again
    assert ts.emul_fps(lattice[None], [216], 2)[0][0].tolist() == [0, 215]
    same = np.zeros((5, 3), np.float32)
    assert ts.emul_fps(same[None], [5], 4)[0][0].tolist() == [0, 0, 0, 0]
    # several rows with their own counts in one launch
    rows = np.stack([_cloud(100, 1), _cloud(100, 2), _cloud(100, 3)])
    idx, m = ts.emul_fps(rows, [100, 0, 37], 50)
    assert m.tolist() == [50, 0, 37] and (idx[1] == -1).all()
    assert np.array_equal(idx[2, :37], ts.ref_fps(rows[2, :37], 50)) and np.array_equal(idx[0], ts.ref_fps(rows[0], 50))


# graph -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ts.SOLVE_CASES)
def test_graph_equals_fp32_restatement_and_float64_outside_the_margin(case):
    src, dst, _, _, inl = ts.correspondences(*case)
    adj = ts.emul_graph(src, dst).astype(bool)
    assert np.array_equal(adj, adj.T) and not adj.diagonal().any()
    assert np.array_equal(adj, ts.ref_graph_f32(src, dst))
    a64, clear = ts.ref_graph_f64(src, dst)
    n_pairs = len(src) * (len(src) - 1)
    unclear = n_pairs - int(clear.sum())
    print(f"{case}: {unclear} of {n_pairs} ordered pairs within {ts.GRAPH_MARGIN} m of the threshold")
    assert unclear <= ts.GRAPH_CAP * n_pairs
    assert np.array_equal(adj[clear], a64[clear])
    assert adj[np.ix_(inl, inl)].sum() == inl.sum() * (inl.sum() - 1)                  # inlier noise of a quarter of the bound: a clique


# cores -----------------------------------------------------------------------------------------------------------------------------------
def _graph(n, edges):
    a = np.zeros((n, n), np.uint8)
    for i, j in edges:
        a[i, j] = a[j, i] = 1
    return a


def _clique(vs):
    return [(i, j) for i in vs for j in vs if i < j]


def _selected(a):
    core, k = ts.emul_cores(a)
    assert np.array_equal(core, ts.ref_cores(a)) and (len(core) == 0 or k == core.max())
    return set(np.where(core == k)[0].tolist()), k


def test_cores_against_a_sequential_peel():
    assert _selected(_graph(30, [])) == (set(range(30)), 0)                                  # empty graph: every vertex has core number 0
    assert _selected(_graph(40, _clique(range(40)))) == (set(range(40)), 39)                  # complete graph
    rng = np.random.RandomState(4)
    noise = [(int(i), int(j)) for i, j in rng.randint(0, 100, size=(150, 2)) if i != j]
    sel, k = _selected(_graph(100, _clique(range(40, 60)) + noise))                           # a 20-clique in sparse noise
    assert set(range(40, 60)) <= sel and k >= 19 and len(sel) <= 24
    sel, k = _selected(_graph(30, _clique(range(10)) + _clique(range(15, 27))))               # cliques of 10 and 12
    assert sel == set(range(15, 27)) and k == 11
    # the documented deviation from the exact maximum clique: a 4-clique (core number 3) beside K5,5 (core number 5, largest clique 2)
    k55 = [(4 + i, 9 + j) for i in range(5) for j in range(5)]
    sel, k = _selected(_graph(14, _clique(range(4)) + k55))
    assert sel == set(range(4, 14)) and k == 5
    for seed in range(5):                                                                      # random graphs, sparse to dense
        a = np.triu(np.random.RandomState(seed).rand(70, 70) < 0.05 + 0.2 * seed, 1).astype(np.uint8)
        _selected(a + a.T)


# registration ----------------------------------------------------------------------------------------------------------------------------
def _bounds(src):
    """what inlier noise within a quarter of the bound allows: the centre within half the bound, the angle within half the bound over the
    cloud's rms radius"""
    c = src.astype(np.float64).mean(0)
    radius = float(np.sqrt(((src - c) ** 2).sum(1).mean()))
    return c, ts.NOISE_BOUND / 2 / radius, ts.NOISE_BOUND / 2


@pytest.mark.parametrize("graph", ("chain", "complete"))
@pytest.mark.parametrize("case", ts.SOLVE_CASES)
def test_known_transform_is_recovered(case, graph):
    src, dst, R, t, inl = ts.correspondences(*case)
    out = ts.emul_solve(src[None], dst[None], [len(src)], rotation_tim_graph=graph)
    c, ang_max, pos_max = _bounds(src)
    ang, pos = ts.pose_error(out["Rt"][0], R, t, c)
    n, M, m, its, n_in = out["info"][0]
    print(f"{case} {graph}: angle {ang:.2e} rad (bound {ang_max:.2e}), centre {pos:.2e} m (bound {pos_max:.2e}), selected {m}, iterations {its}, inliers {n_in}")
    assert n == M == len(src) and ang <= ang_max and pos <= pos_max
    assert n_in >= inl.sum() - 1 and out["selected"][0][inl].all()
    # all-points least squares on the same data
    s, d = src.astype(np.float64), dst.astype(np.float64)
    Rk = ts.kabsch(s - s.mean(0), d - d.mean(0))
    k_ang, k_pos = ts.pose_error(np.concatenate([Rk, (d.mean(0) - Rk @ s.mean(0))[:, None]], 1), R, t, c)
    if case[1] == 0.6:
        assert k_pos > 10 * pos_max
    if case[1] == 0.0:
        assert k_pos <= pos_max


def test_registration_tolerance_is_the_measured_one():
    """every selection and graph on every correspondence fixture (selection "none" is where the GNC loop has outliers to reject: 23 to 29
    iterations at 30 and 60 %), and every launch from depth frames of the two test files"""
    worst, most = 0.0, 0
    for case in ts.SOLVE_CASES:
        src, dst, _, _, _ = ts.correspondences(*case)
        for graph in ("chain", "complete"):
            for sel in ("kcore", "none"):
                out = ts.emul_solve(src[None], dst[None], [len(src)], inlier_selection=sel, rotation_tim_graph=graph)
                ref = ts.ref_solve(src, dst, inlier_selection=sel, rotation_tim_graph=graph)
                assert np.array_equal(out["selected"][0] == 1, ref["selected"]) and np.array_equal(out["core"][0], ref["core"])
                assert out["info"][0].tolist()[2:] == [ref["n_selected"], ref["gnc_iterations"], ref["num_inliers"]], (case, graph, sel)
                worst = max(worst, float(np.abs(out["Rt"][0] - ref["Rt"]).max()))
                most = max(most, ref["gnc_iterations"])
    assert most >= 20
    for name in ts.FRAME_CASES:
        for variant in range(len(ts.FRAME_VARIANTS)):
            rows = (0,) if (name, variant) == ("big", 2) else None      # (all pairs of 1000 samples in numpy: one row of the three)
            worst = max(worst, _frames_against_the_restatement(name, variant, rows))
    print(f"largest |emulation - float64 restatement| over [R t]: {worst:.3e}; RT_TOL = {ts.RT_TOL:.3e}")
    assert worst <= ts.RT_TOL and worst >= ts.RT_TOL / 40     # (the constant is this measurement times 4: neither exceeded nor stale)


def test_accept_rule_at_its_threshold_and_too_few_selected():
    src, dst, _, _, inl = ts.correspondences(120, 0.3, 1203)
    n_in = int(ts.emul_solve(src[None], dst[None], [120])["info"][0, 4])
    assert 80 <= n_in <= 120
    for min_inl, want in ((n_in - 1, 0), (n_in, 0), (n_in + 1, -1)):
        out = ts.emul_solve(src[None], dst[None], [120], min_num_inliers=min_inl)
        assert out["retval"][0] == want and out["info"][0, 4] == n_in
        assert ts.ref_solve(src, dst, min_num_inliers=min_inl)["retval"] == want
    # fewer than 3 selected: two correspondences, and three of which only two are consistent
    src, dst = src[inl], dst[inl]
    far = dst[:3].copy()
    far[2] += np.float32(1.0)                      # vertex 2 is consistent with nobody: core number 0 under the pair's 1
    for s, d, cnt, m in ((src[:2], dst[:2], 2, 2), (src[:3], far, 3, 2), (src[:3], dst[:3], 0, 0)):
        out = ts.emul_solve(s[None], d[None], [cnt])
        assert out["retval"][0] == -1 and out["info"][0].tolist() == [cnt, cnt, m, 0, 0]
        assert np.array_equal(out["Rt"][0], np.eye(3, 4))


def test_rows_of_one_launch_equal_single_launches():
    """several rows, their own counts, a failed row between good ones"""
    stride = 200
    rows, counts = [], []
    for n, o, seed in ((200, 0.3, 20003), (2, 0.0, 7), (50, 0.6, 5006), (120, 0.0, 12000)):
        src, dst, _, _, _ = ts.correspondences(n, o, seed)
        pad = np.full((stride - n, 3), np.nan, np.float32)            # past the count: never read
        rows.append((np.concatenate([src, pad]), np.concatenate([dst, pad])))
        counts.append(n)
    S, D = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    both = ts.emul_solve(S, D, counts, min_num_inliers=10)
    assert both["retval"].tolist() == [0, -1, 0, 0]
    for r in range(4):
        one = ts.emul_solve(S[r: r + 1], D[r: r + 1], counts[r: r + 1], min_num_inliers=10)
        for key in both:
            assert np.array_equal(both[key][r], one[key][0]), (r, key)
        assert (both["degree"][r, counts[r]:] == -1).all() and (both["selected"][r, counts[r]:] == -1).all()


# the chain from depth frames ----------------------------------------------------------------------------------------------------------------
def _frames_against_the_restatement(name, variant, rows=None):
    """one launch of the emulation against the restatement row by row: counts, samples, decisions; -> the largest |difference| of [R t]"""
    frames, kw = ts.FRAME_CASES[name]
    kw = dict(kw, **ts.FRAME_VARIANTS[variant])
    meas, im_ids, rend, K, TCO = ts.frame_case(*frames)
    out = ts.emul_frames(name, variant)
    worst = 0.0
    for r in (range(len(TCO)) if rows is None else rows):
        ref = ts.ref_refine_row(meas[im_ids[r]], rend[r], K[r], **kw)
        assert ref["N"] == out["info"][r, 0] and ref["retval"] == out["retval"][r], (name, variant, r)
        assert out["info"][r, 1:3].tolist() == [0 if ref["sample_idx"] is None else len(ref["sample_idx"]), ref["n_selected"]], (name, variant, r)
        if ref["sample_idx"] is not None:
            assert np.array_equal(out["sample_idx"][r, : len(ref["sample_idx"])], ref["sample_idx"])
        if frames[3][r] == "noise":      # outliers only: there is no transform to agree on; both sides reject the row
            assert out["retval"][r] == -1
            continue
        assert out["info"][r, 3:].tolist() == [ref["gnc_iterations"], ref["num_inliers"]], (name, variant, r)
        if ref["Rt"] is not None:
            worst = max(worst, float(np.abs(out["Rt"][r] - ref["Rt"]).max()))
        if out["retval"][r] == 0:
            pose = (np.vstack([out["Rt"][r], [0, 0, 0, 1]]) @ TCO[r].astype(np.float64)).astype(np.float32)
            assert np.array_equal(out["TCO"][r], pose)
        else:
            assert np.array_equal(out["TCO"][r], TCO[r])                                    # a failed row keeps its pose
    return worst


def test_refine_from_frames():
    """what the rows of the "small" and "tiny" launches are there for"""
    simple, thresh = ts.emul_frames("small", 0), ts.emul_frames("small", 1)
    assert simple["info"][:, 0].tolist() == [700, 64, 0, 150 + 150, 500] and thresh["info"][:, 0].tolist()[:4] == [700, 64, 0, 150]
    assert thresh["info"][4, 0] < 500                                                       # random depths: most are beyond the threshold
    assert simple["info"][:, 1].tolist() == [100, 0, 0, 100, 100]                           # a row under n_min_points takes no samples
    assert simple["retval"].tolist() == [0, -1, -1, -1, -1] and thresh["retval"].tolist()[:4] == [0, -1, -1, 0]
    tiny = ts.emul_frames("tiny", 0)
    assert tiny["info"][:, :2].tolist() == [[1, 1], [63, 63], [64, 64], [65, 64], [0, 0]] and tiny["retval"].tolist() == [-1, 0, 0, 0, -1]
    strided = ts.emul_frames("big", 4)
    assert np.array_equal(strided["sample_idx"][1], (np.arange(1000) * 19200) // 1000)


def test_limits():
    lim = ts.limits()
    assert lim == dict(threads=1024, max_points=1024, fps_resident=ts.FPS_RESIDENT, gnc_max_iter=100, info=5)
