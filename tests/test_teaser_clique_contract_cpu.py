"""CPU: the rule of the exact maximum-clique inlier selection (megapose6d_amd/csrc/teaser_clique_core.h) on the host emulation
(tests/teaser_clique_emul.cpp) against an independent Bron-Kerbosch in plain Python (tests/support/teaser_clique.py): the result is a
maximum clique -- the only one where it is unique --, the shortcut, the counter-example of the k-core rule, the step budget, the
registration in that mode, and the public names.  The GPU test (tests/test_gpu_teaser_clique.py) holds the kernel to this emulation
bit for bit."""
import numpy as np
import pytest

from support import teaser as ts
from support import teaser_clique as tc


@pytest.mark.parametrize("n", (1, 2, 3, 14, 31, 32, 33, 40))
def test_result_is_a_maximum_clique(n):
    unique = 0
    for p in (0.1, 0.3, 0.5, 0.7, 0.9):
        for seed in range(4):
            a = tc.gnp(n, p, 1000 * n + seed)
            omega, cliques = tc.bron_kerbosch(a)
            members, info = tc.emul_max_clique(a)
            got = tc.members_of(members[0])
            size, upper, exact, steps = info[0].tolist()
            assert tc.is_clique(a, got) and size == len(got) == omega and exact == 1, (n, p, seed, got, omega)
            assert tuple(got) in cliques and omega <= upper <= n and steps >= 0
            assert steps > 0 or size == upper                       # no search only where the greedy clique meets the bound
            if len(cliques) == 1:
                unique += 1
                assert tuple(got) == cliques[0]
    print(f"n = {n}: {unique} of 20 graphs have one maximum clique")


def test_brute_force_on_graphs_known_by_hand():
    assert tc.bron_kerbosch(np.zeros((5, 5))) == (1, [(0,), (1,), (2,), (3,), (4,)])
    assert tc.bron_kerbosch(1 - np.eye(6)) == (6, [(0, 1, 2, 3, 4, 5)])
    assert tc.bron_kerbosch(tc.counter_example()) == (4, [(0, 1, 2, 3)])
    ring = np.zeros((5, 5), np.uint8)
    for i in range(5):
        ring[i, (i + 1) % 5] = 1                                    # one side only: the brute force symmetrises too
    assert tc.bron_kerbosch(ring) == (2, [(0, 1), (0, 4), (1, 2), (2, 3), (3, 4)])


def test_counter_example_of_the_kcore_rule():
    a = tc.counter_example()
    members, info = tc.emul_max_clique(a)
    assert tc.members_of(members[0]) == [0, 1, 2, 3] and info[0].tolist() == [4, 6, 1, 20]
    core, k = ts.emul_cores(a)
    assert set(np.where(core == k)[0].tolist()) == set(range(4, 14)) and k == 5          # the k-core rule still selects the bipartite part
    assert tc.bron_kerbosch(a[4:, 4:])[0] == 2


def test_planted_clique_takes_the_shortcut():
    a, who = tc.planted(100, 20, 1.0, 0.03, 0)
    members, info = tc.emul_max_clique(a, max_steps=0)                                    # no search: no budget needed
    assert tc.members_of(members[0]) == who.tolist() and info[0].tolist() == [20, 20, 1, 0]


def test_asymmetric_input_loops_and_counts():
    a, counts = tc.stride70_rows()
    members, info = tc.emul_rows("stride70")
    assert info[:, 2].all()
    for r, n in enumerate(counts):
        sub = a[r, :n, :n] * (1 - np.eye(n, dtype=np.uint8))
        got = tc.members_of(members[r])
        assert tc.is_clique(sub, got) and max(got) < n
        if n <= 33:
            assert len(got) == tc.bron_kerbosch(sub)[0]
    assert tc.members_of(members[2]) == [0, 1, 2, 3] and info[2].tolist() == [4, 6, 1, 20]
    # a row alone, without the counts argument, equals the row of the launch
    one, one_info = tc.emul_max_clique(a[8])
    assert np.array_equal(one[0], members[8]) and np.array_equal(one_info[0], info[8])
    m0, i0 = tc.emul_max_clique(a[:2], [0, -3])
    assert (m0 == -1).all() and i0.tolist() == [[0, 0, 1, 0]] * 2


def test_step_budget():
    n = tc.BUDGET_GRAPH[0]
    a = tc.gnp(*tc.BUDGET_GRAPH)
    full_m, full = tc.emul_max_clique(a)
    greedy_m, greedy = tc.emul_max_clique(a, max_steps=0)
    small_m, small = tc.emul_max_clique(a, max_steps=tc.SMALL_BUDGET)
    print("full", full[0].tolist(), "budget", tc.SMALL_BUDGET, small[0].tolist(), "greedy", greedy[0].tolist())
    assert full[0, 2] == 1 and full[0, 3] > 20 * tc.SMALL_BUDGET and tc.is_clique(a, tc.members_of(full_m[0]))
    assert not any(tc.is_clique(a, tc.members_of(full_m[0]) + [v]) for v in range(n) if v not in full_m[0])
    assert small[0, 2] == 0 and tc.SMALL_BUDGET < small[0, 3] <= tc.SMALL_BUDGET + n
    assert greedy[0, 2] == 0 and 0 < greedy[0, 3] <= n
    assert tc.is_clique(a, tc.members_of(small_m[0])) and tc.is_clique(a, tc.members_of(greedy_m[0]))
    assert greedy[0, 0] <= small[0, 0] <= full[0, 0]
    last = 0
    for budget in (0, 100, 1000, 5000, 20000, int(full[0, 3]) - 1, int(full[0, 3]), tc.FULL_BUDGET):   # a larger budget never returns a smaller clique
        m, info = tc.emul_max_clique(a, max_steps=budget)
        assert info[0, 0] >= last and tc.is_clique(a, tc.members_of(m[0])) and info[0, 2] == (1 if budget >= full[0, 3] else 0)
        last = int(info[0, 0])
    assert last == full[0, 0]


def _bounds(src):
    """as tests/test_teaser_contract_cpu.py: the centre within half the bound, the angle within half the bound over the rms radius"""
    c = src.astype(np.float64).mean(0)
    radius = float(np.sqrt(((src - c) ** 2).sum(1).mean()))
    return c, ts.NOISE_BOUND / 2 / radius, ts.NOISE_BOUND / 2


@pytest.mark.parametrize("graph", ("chain", "complete"))
@pytest.mark.parametrize("case", ts.SOLVE_CASES)
def test_known_transform_is_recovered_in_the_new_mode(case, graph):
    src, dst, R, t, inl = ts.correspondences(*case)
    out = tc.emul_solve(src[None], dst[None], [len(src)], inlier_selection="max_clique", rotation_tim_graph=graph)
    c, ang_max, pos_max = _bounds(src)
    ang, pos = ts.pose_error(out["Rt"][0], R, t, c)
    n, M, m, its, n_in = out["info"][0]
    print(f"{case} {graph}: angle {ang:.2e} rad (bound {ang_max:.2e}), centre {pos:.2e} m (bound {pos_max:.2e}), selected {m}, clique {out['clique'][0].tolist()}")
    assert n == M == len(src) and ang <= ang_max and pos <= pos_max
    assert n_in >= inl.sum() - 1 and out["selected"][0][inl].all() and out["clique"][0, 2] == 1
    sel = np.where(out["selected"][0] == 1)[0]
    assert m == out["clique"][0, 0] == len(sel) and tc.is_clique(ts.emul_graph(src, dst), sel)
    # the other modes go through the same wrapper unchanged
    for mode in ("kcore", "none"):
        a, b = tc.emul_solve(src[None], dst[None], [len(src)], inlier_selection=mode), ts.emul_solve(src[None], dst[None], [len(src)], inlier_selection=mode)
        assert all(np.array_equal(a[k], b[k]) for k in b) and "clique" not in a


def test_rejected_rows_and_frames_in_the_new_mode():
    src, dst, _, _, inl = ts.correspondences(120, 0.3, 1203)
    out = tc.emul_solve(src[inl][None, :2], dst[inl][None, :2], [2], inlier_selection="max_clique")
    assert out["retval"][0] == -1 and out["info"][0].tolist() == [2, 2, 2, 0, 0] and out["clique"][0].tolist() == [2, 2, 1, 0]
    assert np.array_equal(out["Rt"][0], np.eye(3, 4))
    frames, kw = ts.FRAME_CASES["tiny"]
    got = tc.emul_refine(*ts.frame_case(*frames), **kw)
    want = ts.emul_frames("tiny", 0)
    # near-rigid rows: the largest core is the inlier clique, so the two selections agree on these frames
    assert np.array_equal(got["retval"], want["retval"]) and np.array_equal(got["sample_idx"], want["sample_idx"])
    assert got["clique"][:, 2].all() and np.array_equal(got["clique"][:, 0], got["info"][:, 2])


def test_public_names():
    from megapose6d_amd import TeaserppRefiner
    from megapose6d_amd import engine as eng

    refiner = TeaserppRefiner(None, None, inlier_selection="max_clique")
    assert refiner.inlier_selection == "max_clique" and refiner.max_clique_steps is None
    with pytest.raises(ValueError):
        TeaserppRefiner(None, None, inlier_selection="clique")
    default = TeaserppRefiner(None, None)
    assert default.inlier_selection == "kcore" and default.rotation_tim_graph == "chain" and default.max_clique_steps is None
    assert eng.TEASER_SELECTIONS == {"kcore": 0, "none": 1, "max_clique": 2}
    assert eng.TEASER_CLIQUE_INFO == tc.CLIQUE_INFO == ("size", "upper_bound", "exact", "steps")
    lim = tc.limits()
    assert lim["info"] == 4 and lim["selection"] == eng.TEASER_SELECTIONS["max_clique"] and lim["step_ceiling"] == 16 * lim["default_steps"]
    assert lim["default_steps"] & (lim["default_steps"] - 1) == 0 and tc.FULL_BUDGET <= lim["step_ceiling"]
    assert eng.max_clique_step_limits() == (lim["default_steps"], lim["step_ceiling"])


def test_emulation_under_the_sanitizers(tmp_path):
    """the emulation as a stand-alone program (tests/teaser_clique_asan_main.cpp) under the address and undefined-behaviour sanitizers, on
    the fixtures above: search stacks are where off-by-ones live.  The program compares every case with what the plain build returned."""
    import subprocess

    cases = [(tc.counter_example(), None, tc.FULL_BUDGET), (tc.planted(100, 20, 1.0, 0.03, 0)[0], None, 0), (np.zeros((1, 1), np.uint8), None, 5)]
    cases += [(tc.gnp(*tc.BUDGET_GRAPH), None, b) for b in (0, tc.SMALL_BUDGET, tc.FULL_BUDGET)]
    cases += [(tc.gnp(n, p, 7 * n), None, tc.FULL_BUDGET) for n in (2, 3, 31, 32, 33, 40) for p in (0.1, 0.5, 0.9)]
    rows, counts = tc.stride70_rows()
    cases += [(rows[r], int(counts[r]), tc.FULL_BUDGET) for r in range(len(counts))] + [(rows[0], 0, 10), (rows[0], -7, 10), (rows[8], 500, 10)]
    with open(tmp_path / "cases.bin", "wb") as f:
        for a, count, budget in cases:
            members, info = tc.emul_max_clique(a, None if count is None else [count], budget)
            f.write(np.asarray([len(a), -2 ** 31 if count is None else count, budget], np.int32).tobytes())
            f.write(np.ascontiguousarray(a, np.uint8).tobytes() + members[0].tobytes() + info[0].tobytes())
    exe = tmp_path / "clique_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    str(tc.CSRC), "-I", str(tc.TESTS), "-o", str(exe), str(tc.TESTS / "teaser_clique_asan_main.cpp")], check=True)
    run = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip() == f"{len(cases)} cases, 0 bad", (run.stdout, run.stderr[-2000:])
