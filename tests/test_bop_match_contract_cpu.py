"""CPU: the contract of BOP's greedy matching (csrc/bop_match_core.h).  The host emulation (tests/bop_match_emul.cpp: the lines the
kernel compiles) against an independent numpy restatement written from the contract's text, against what the REFERENCE's match_poses /
get_top_n_ids / add_valid_gt returned on seeded tables (tests/golden/bop_match.npz, written by scripts/make_bop_match_golden.py) on
every recorded problem, and on hand-written cases that pin what the reference leaves open (ties) and every edge of the contract.  Then
the host side of `evaluation`: the candidate table, the index, the threshold tables and the recall arithmetic.  Every comparison is
exact integer (or bit) equality."""
import numpy as np
import pandas as pd
import pytest

from support import bop_match as bm


def _ev():
    from megapose6d_amd import evaluation as ev

    return ev


def _both(c, n_top=None):
    a = bm.emul(c["pred_id"], c["gt_id"], c["group_id"], c["errs"], c["scores"], c["thr"], n_top)
    b = bm.restated(c["pred_id"], c["gt_id"], c["group_id"], c["errs"], c["scores"], c["thr"], n_top)
    assert a.dtype == np.int32 and np.array_equal(a, b)
    return a


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("E,n_theta,n_groups", [(1, 1, 40), (3, 4, 120), (12, 10, 25), (16, 16, 6)])
def test_emulation_matches_the_restatement_on_ragged_groups(E, n_theta, n_groups, ties):
    sizes = bm.ragged_sizes(100 + E, n_groups)
    c = bm.case(7 * E + n_theta, sizes, E, n_theta, ties=ties)
    rng = np.random.RandomState(E)
    full = _both(c)
    cut = _both(c, rng.randint(0, 4, size=n_groups))
    assert (full >= 0).any() and (cut >= 0).sum() <= (full >= 0).sum()
    # a ground truth is given once per problem, and only to an estimate of its own group
    for e in range(E):
        for k in range(n_theta):
            got = full[:, e, k][full[:, e, k] >= 0]
            assert len(set(got.tolist())) == len(got)
    if ties:
        assert len(set(c["scores"].tolist())) < len(c["scores"])


def test_emulation_on_one_large_group_past_a_64_bit_mask():
    c = bm.case(3, [(7, 70), (2, 3)], 2, 3, nan_share=0.0)
    m = _both(c)
    assert (m[:, 0, 2] >= 0).sum() >= 7


@pytest.fixture(scope="module")
def golden():
    fx = dict(np.load(bm.GOLDEN))
    keys = ["scene_id", "view_id", "label"]
    pred = pd.DataFrame({k: fx[f"pred_{k}"] for k in keys})
    gt = pd.DataFrame({k: fx[f"gt_{k}"] for k in keys})
    cand = _ev().bop_candidates(pred, gt, valid=fx["gt_valid"], keys=keys)
    return fx, pred, gt, cand


def test_candidates_and_valid_mask_against_the_reference(golden):
    fx, pred, gt, cand = golden
    assert np.array_equal(fx["gt_visib_fract"] >= 0.1, fx["gt_valid"])                       # add_valid_gt(visib_gt_min=0.1)
    assert list(cand.columns) == ["pred_id", "gt_id", "group_id"] and len(cand) == len(fx["cand_pred_id"]) > 300
    assert np.array_equal(cand["pred_id"].to_numpy(), fx["cand_pred_id"]) and np.array_equal(cand["gt_id"].to_numpy(), fx["cand_gt_id"])
    assert fx["gt_valid"][cand["gt_id"].to_numpy()].all()
    # a group is one value of the keys, numbered in order of first appearance
    grp = cand["group_id"].to_numpy()
    first = [tuple(pred.iloc[p]) for p in cand["pred_id"].to_numpy()]
    seen = {}
    for key, g in zip(first, grp):
        assert seen.setdefault(key, len(seen)) == g
    assert all(tuple(pred.iloc[p]) == tuple(gt.iloc[g]) for p, g in zip(cand["pred_id"], cand["gt_id"]))
    # Series masks are aligned by index; every valid pair is there
    again = _ev().bop_candidates(pred, gt, valid=pd.Series(fx["gt_valid"][::-1], index=gt.index[::-1]), keys=["scene_id", "view_id", "label"])
    assert again.equals(cand)
    for bad in (fx["gt_valid"].astype(np.int64), fx["gt_valid"][:-1], np.ones((len(gt), 1), bool)):
        with pytest.raises(ValueError):
            _ev().bop_candidates(pred, gt, valid=bad, keys=["scene_id", "view_id", "label"])
    assert len(_ev().bop_candidates(pred, gt, keys=["scene_id", "view_id", "label"])) > len(cand)   # default: every ground truth


def test_emulation_against_the_reference_on_every_recorded_problem(golden):
    fx, pred, gt, cand = golden
    n_groups = int(cand["group_id"].max()) + 1
    E, K = fx["thetas"].shape
    thr = np.broadcast_to(fx["thetas"][None], (n_groups, E, K)).copy()
    args = (cand["pred_id"].to_numpy(), cand["gt_id"].to_numpy(), cand["group_id"].to_numpy(), fx["errs"], fx["pred_score"], thr)
    got = bm.emul(*args)
    assert got.shape == fx["match_all"].shape
    for e in range(E):
        for k in range(K):
            assert np.array_equal(got[:, e, k], fx["match_all"][:, e, k]), (e, k)
    assert (got >= 0).sum() > 1000 and np.array_equal(got, bm.restated(*args))
    # get_top_n_ids(targets=...): n_top = the group's number of valid ground truths
    n_top = _ev().bop_n_top("targets", cand.groupby("group_id")["gt_id"].nunique().to_numpy())
    top = bm.emul(*args, n_top)
    assert np.array_equal(top, fx["match_top"]) and np.array_equal(top, bm.restated(*args, n_top))
    cut = np.setdiff1d(np.arange(len(pred)), fx["top_keep"])
    assert len(cut) > 20 and (top[cut] == -1).all() and not np.array_equal(top, got)


# hand-written cases: (pred, gt, err) triples of ONE group unless `group` is given; one error column, one threshold -------------------------
def _hand(triples, scores, thr, n_top=None, group=None):
    pid, gid, err = (np.asarray([t[i] for t in triples]) for i in range(3))
    grp = np.zeros(len(triples), np.int64) if group is None else np.asarray(group)
    n_groups = int(grp.max()) + 1 if len(grp) else 1
    c = dict(pred_id=pid.astype(np.int64), gt_id=gid.astype(np.int64), group_id=grp, errs=np.asarray(err, np.float32).reshape(-1, 1),
             scores=np.asarray(scores, np.float64), thr=np.full((n_groups, 1, 1), thr, np.float64))
    return _both(c, None if n_top is None else np.full(n_groups, n_top, np.int32))[:, 0, 0].tolist()


def test_two_estimates_compete_for_one_ground_truth_the_higher_score_wins():
    assert _hand([(0, 0, 0.1), (1, 0, 0.2)], [0.9, 0.5], 0.5) == [0, -1]
    assert _hand([(0, 0, 0.1), (1, 0, 0.2)], [0.5, 0.9], 0.5) == [-1, 0]                       # even with the larger error


def test_an_estimate_falls_back_to_its_second_best_when_its_best_is_taken():
    assert _hand([(0, 0, 0.10), (0, 1, 0.30), (1, 0, 0.05), (1, 1, 0.20)], [0.9, 0.5], 0.5) == [0, 1]


def test_an_estimate_gets_nothing_when_its_only_admissible_ground_truth_is_taken():
    assert _hand([(0, 0, 0.10), (0, 1, 0.30), (1, 0, 0.05), (1, 1, 0.70)], [0.9, 0.5], 0.5) == [0, -1]


def test_error_tie_the_lower_gt_row_wins_and_score_tie_the_lower_pred_row_goes_first():
    assert _hand([(0, 5, 0.25), (0, 2, 0.25), (0, 7, 0.25)], [1.0], 0.5) == [2]
    assert _hand([(1, 0, 0.2), (0, 0, 0.3)], [0.5, 0.5], 0.5) == [0, -1]                       # pred row 0 first, whatever the errors
    assert _hand([(1, 0, 0.2), (0, 0, 0.3), (1, 1, 0.4)], [0.5, 0.5], 0.5) == [0, 1]


def test_threshold_is_strict_nan_never_matches_and_the_comparison_is_made_in_float64():
    assert _hand([(0, 0, 0.25)], [1.0], 0.25) == [-1]                                          # exactly on the threshold
    assert _hand([(0, 0, 0.25)], [1.0], np.nextafter(0.25, 1.0)) == [0]
    assert _hand([(0, 0, np.nan), (0, 1, 0.4)], [1.0], 0.5) == [1]
    assert _hand([(0, 0, np.nan)], [1.0], np.inf) == [-1]
    assert _hand([(0, 0, np.inf)], [1.0], 0.5) == [-1]
    # float32(0.35) = 0.3499999940... < 0.35 as float64; rounded to float32 the two would be equal and the match lost
    assert float(np.float32(0.35)) < 0.35 and np.float32(0.35) == np.float32(np.float64(0.35))
    assert _hand([(0, 0, np.float32(0.35))], [1.0], 0.35) == [0]
    # float32(0.3) = 0.30000001192... > 0.3: no match, though float32(0.3) < float32 would also say so -- and one ulp below matches
    assert float(np.float32(0.3)) > 0.3
    assert _hand([(0, 0, np.float32(0.3))], [1.0], 0.3) == [-1]
    assert _hand([(0, 0, np.nextafter(np.float32(0.3), np.float32(0)))], [1.0], 0.3) == [0]


def test_n_top_cuts_the_one_estimate_that_would_have_matched():
    triples = [(0, 0, 0.9), (1, 0, 0.1)]
    assert _hand(triples, [0.9, 0.5], 0.5) == [-1, 0]
    assert _hand(triples, [0.9, 0.5], 0.5, n_top=1) == [-1, -1]
    assert _hand(triples, [0.9, 0.5], 0.5, n_top=2) == [-1, 0] and _hand(triples, [0.9, 0.5], 0.5, n_top=7) == [-1, 0]


def test_groups_without_valid_ground_truth_estimates_without_ground_truth_and_no_candidates():
    ev = _ev()
    pred = pd.DataFrame(dict(batch_im_id=[0, 0, 1, 2], label=["a", "a", "a", "b"]))
    gt = pd.DataFrame(dict(batch_im_id=[0, 1, 1, 3], label=["a", "a", "a", "b"]))
    valid = np.array([False, True, True, True])
    cand = ev.bop_candidates(pred, gt, valid=valid)
    # image 0: its only ground truth is not valid; image 2 / label b: no ground truth at all; image 3: no estimate
    assert cand.to_dict("list") == dict(pred_id=[2, 2], gt_id=[1, 2], group_id=[0, 0])
    m = _both(dict(pred_id=cand["pred_id"], gt_id=cand["gt_id"], group_id=cand["group_id"], errs=np.float32([[0.3], [0.2]]), scores=np.ones(4),
                   thr=np.full((1, 1, 1), 0.5)))
    assert m[:, 0, 0].tolist() == [-1, -1, 2, -1]
    none = ev.bop_candidates(pred, gt, valid=np.zeros(4, bool))
    assert len(none) == 0 and list(none.columns) == ["pred_id", "gt_id", "group_id"]
    z = np.zeros(0, np.int64)
    m = _both(dict(pred_id=z, gt_id=z, group_id=z, errs=np.zeros((0, 2), np.float32), scores=np.ones(3), thr=np.zeros((0, 2, 3))))   # C = 0
    assert m.shape == (3, 2, 3) and (m == -1).all()
    m = _both(dict(pred_id=z, gt_id=z, group_id=z, errs=np.zeros((0, 2), np.float32), scores=np.ones(0), thr=np.zeros((0, 2, 3))))   # P = 0
    assert m.shape == (0, 2, 3)


def test_index_layout_and_what_it_refuses():
    ev = _ev()
    ix = ev.bop_match_index([0, 0, 1, 1, 2], [4, 9, 9, 4, 7], [0, 0, 0, 0, 1], [0.1, 0.2, 0.3])
    assert ix["order"].tolist() == [3, 2, 0, 1, 4] and ix["cand_gt"].tolist() == [4, 9, 4, 9, 7] and ix["cand_lgt"].tolist() == [0, 1, 0, 1, 0]
    assert ix["est_row"].tolist() == [1, 0, 2] and ix["est_off"].tolist() == [0, 2, 4, 5] and ix["group_est_off"].tolist() == [0, 2, 3]
    assert ix["group_n_gt"].tolist() == [2, 1] and ix["group_taken_off"].tolist() == [0, 1, 2] and ix["n_taken_words"] == 2
    assert all(ix[k].dtype == np.int32 for k in ix if k not in ("order", "n_taken_words"))
    wide = ev.bop_match_index(np.zeros(70, int), np.arange(70), np.zeros(70, int), [1.0], n_groups=2)   # 70 ground truths: 3 words; group 1 empty
    assert wide["group_taken_off"].tolist() == [0, 3, 3] and wide["group_est_off"].tolist() == [0, 1, 1] and wide["cand_lgt"].tolist() == list(range(70))
    for scores in ([0.1, np.nan, 0.3], [0.1, np.inf, 0.3], [0.1, -np.inf, 0.3]):
        with pytest.raises(ValueError):
            ev.bop_match_index([0], [0], [0], scores)
    for bad in (([0, 0], [1, 2], [0, 1]), ([0, 1], [2, 2], [0, 1]), ([0, 5], [1, 2], [0, 0]), ([0, -1], [1, 2], [0, 0]), ([0, 1], [1, -2], [0, 0]),
                ([0, 1], [1, 2], [0])):
        with pytest.raises(ValueError):
            ev.bop_match_index(*bad, [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        ev.bop_match_index([0], [0], [3], [0.1], n_groups=2)


def test_threshold_tables_and_recall_arithmetic_are_those_of_bop_recall():
    """a one-to-one table: estimate i against ground truth i, each in a group of its own.  The matching then gives row i its ground
    truth exactly where err < thr, so a match tensor stubbed that way must score what bop_recall scores on the error table"""
    ev = _ev()
    rng = np.random.RandomState(5)
    n, n_tau = 37, len(ev.BOP_TAUS)
    names = [f"vsd_{t:.2f}" for t in ev.BOP_TAUS]
    diam = rng.uniform(0.05, 0.4, n)
    df = pd.DataFrame({c: rng.choice([0.0, 0.05, 0.1, 0.15, 0.2, 0.3, 0.35, 0.5, 0.77, 1.0], n).astype(np.float32).astype(np.float64) for c in names})
    df["mssd"] = (rng.uniform(0, 0.6, n) * diam).astype(np.float32).astype(np.float64)
    df["mspd"] = rng.uniform(0, 60, n).astype(np.float32).astype(np.float64)
    df.loc[3, names[0]] = np.nan
    df.loc[4, "mssd"] = np.nan
    df.loc[5, "mspd"] = 5.0 * 800 / 640                                                   # exactly on a threshold at width 800
    df["diameter"] = diam
    valid = rng.uniform(size=n) < 0.8
    for width in (640, 800):
        thr = ev.bop_thresholds(diam, n_tau, image_width=width)
        assert thr.shape == (n, n_tau + 2, 10) and thr.dtype == np.float64
        thetas = np.asarray(ev.BOP_THRESHOLDS, np.float64)
        assert np.array_equal(thr[:, :n_tau], np.broadcast_to(thetas, (n, n_tau, 10)))
        assert np.array_equal(thr[:, n_tau], thetas[None, :] * diam[:, None])
        assert np.array_equal(thr[:, n_tau + 1], np.broadcast_to(np.arange(5, 51, 5).astype(np.float64) * (float(width) / 640.0), (n, 10)))
        errs = df[names + ["mssd", "mspd"]].to_numpy(np.float64)
        match = np.where(errs[:, :, None] < thr, np.arange(n)[:, None, None], -1).astype(np.int32)
        match[~valid] = -1                                                                 # a row that is no target has no candidate
        got = ev.bop_match_recall(match, int(valid.sum()))
        assert got == ev.bop_recall(df, image_width=width, valid=valid)
        assert 0.2 < got["ar"] < 0.9
    # targets without any candidate count in the denominator
    half = ev.bop_match_recall(match, 2 * int(valid.sum()))
    assert half["ar_mssd"] == float((match[:, n_tau] >= 0).sum() / (2 * int(valid.sum()) * 10)) and 0 < half["ar_mssd"] < got["ar_mssd"]
    with pytest.raises(ValueError):
        ev.bop_match_recall(match, 0)
    with pytest.raises(ValueError):
        ev.bop_match_recall(match[:, :2], 5)


def test_the_three_forms_of_n_top():
    ev = _ev()
    n_gt = np.array([2, 1, 5], np.int32)
    assert ev.bop_n_top("targets", n_gt).tolist() == [2, 1, 5] and ev.bop_n_top(3, n_gt).tolist() == [3, 3, 3]
    assert ev.bop_n_top(None, n_gt).tolist() == [0, 0, 0] and ev.bop_n_top(0, n_gt).tolist() == [0, 0, 0]
    assert ev.bop_n_top("targets", n_gt).dtype == np.int32
    for bad in ("all", -1, 1.5, True):
        with pytest.raises(ValueError):
            ev.bop_n_top(bad, n_gt)


def test_limits_are_stated_once():
    from megapose6d_amd import engine as eng

    assert bm.limits() == dict(max_errors=eng.BOP_MATCH_MAX_ERRORS, max_thetas=eng.BOP_MATCH_MAX_THETAS, mask_bits=eng.BOP_MATCH_MASK_BITS,
                               stage_floats=eng.BOP_MATCH_STAGE_FLOATS)
