"""TEST SUPPORT: ctypes wrapper of the host emulation of the BOP matching kernel (tests/bop_match_emul.cpp), built on first use; an
independent numpy restatement of the contract, written from its text and not from the rules header (it works on the raw candidate
table: no index, no sorted copy, sets of taken ground truths); and the seeded cases the CPU contract test and the GPU test share."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np

from .emul import CSRC, TESTS, _p, build

GOLDEN = TESTS / "golden" / "bop_match.npz"


def load():
    lib = build("bop_match_emul", [TESTS / "bop_match_emul.cpp", CSRC / "bop_match_core.h"], fma=False)
    lib.bop_match_emul.restype = C.c_int
    lib.bop_match_emul_limits.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_int * 4)()
    load().bop_match_emul_limits(v)
    return dict(zip(("max_errors", "max_thetas", "mask_bits", "stage_floats"), (int(x) for x in v)))


def emul_index(errs_sorted, index, thr, n_pred, n_top=None) -> np.ndarray:
    """the emulation on the arguments of the C ABI: errs_sorted [C,E] in the index's order, index = `evaluation.bop_match_index`"""
    errs_sorted = np.ascontiguousarray(errs_sorted, np.float32)
    thr = np.ascontiguousarray(thr, np.float64)
    n_groups, E, n_theta = thr.shape
    assert errs_sorted.ndim == 2 and errs_sorted.shape == (len(index["cand_gt"]), E) and len(index["group_n_gt"]) == n_groups
    n_top = None if n_top is None else np.ascontiguousarray(n_top, np.int32)
    match = np.empty((n_pred, E, n_theta), np.int32)
    rc = load().bop_match_emul(_p(errs_sorted), _p(index["cand_gt"]), _p(index["cand_lgt"]), _p(index["est_row"]), _p(index["est_off"]),
                               _p(index["group_est_off"]), _p(index["group_n_gt"]), _p(n_top), _p(thr), C.c_int(n_pred), C.c_int(n_groups), C.c_int(E),
                               C.c_int(n_theta), _p(match))
    assert rc == 0
    return match


def emul(pred_id, gt_id, group_id, errs, scores, thr, n_top=None) -> np.ndarray:
    """the emulation on a raw candidate table, through the product's index builder -> match [P,E,n_theta]"""
    from megapose6d_amd import evaluation as ev

    thr = np.asarray(thr, np.float64)
    index = ev.bop_match_index(pred_id, gt_id, group_id, scores, thr.shape[0])
    errs = np.asarray(errs, np.float32).reshape(len(index["order"]), thr.shape[1])
    return emul_index(errs[index["order"]], index, thr, len(scores), n_top)


def restated(pred_id, gt_id, group_id, errs, scores, thr, n_top=None) -> np.ndarray:
    """The contract, from its text: per group, per (e, k), the estimates by decreasing score (ties: ascending pred row), cut to the
    first n_top; each takes, among its candidates in ascending gt row whose ground truth is free and whose error as float64 is below
    the threshold, the smallest error (the first on a tie) -> match [P,E,n_theta] int32, -1 where there is none."""
    pred_id, gt_id, group_id = (np.asarray(a, np.int64) for a in (pred_id, gt_id, group_id))
    scores, thr = np.asarray(scores, np.float64), np.asarray(thr, np.float64)
    n_groups, E, n_theta = thr.shape
    errs = np.asarray(errs, np.float32).reshape(len(pred_id), E).astype(np.float64)
    match = np.full((len(scores), E, n_theta), -1, np.int32)
    for g in range(n_groups):
        rows = np.flatnonzero(group_id == g)
        ests = sorted(set(pred_id[rows].tolist()), key=lambda r: (-scores[r], r))
        if n_top is not None and n_top[g] > 0:
            ests = ests[:int(n_top[g])]
        per_est = {r: sorted(rows[pred_id[rows] == r].tolist(), key=lambda c: gt_id[c]) for r in ests}
        for e in range(E):
            for k in range(n_theta):
                taken = set()
                for r in ests:
                    best = None
                    for c in per_est[r]:
                        if gt_id[c] in taken or not errs[c, e] < thr[g, e, k]:
                            continue
                        if best is None or errs[c, e] < errs[best, e]:
                            best = c
                    if best is not None:
                        taken.add(int(gt_id[best]))
                        match[r, e, k] = gt_id[best]
    return match


# seeded cases shared by the CPU contract test and the GPU test --------------------------------------------------------------------
def case(seed, sizes, E, n_theta, ties=False, nan_share=0.02, permute=True):
    """sizes = [(n_est, n_gt)] per group: full cross products, rows shuffled.  Errors in [0, 1), thresholds in (0, 1) rising with k,
    a share of NaN errors; with `ties`, errors and scores are drawn from a few values so that both kinds of tie are frequent.
    -> dict(pred_id, gt_id, group_id, errs [C,E], scores [P], thr [n_groups,E,n_theta], n_pred, n_gt)"""
    rng = np.random.RandomState(seed)
    n_groups = len(sizes)
    P, G = sum(s[0] for s in sizes), sum(s[1] for s in sizes)
    pred_rows, gt_rows = (rng.permutation(P), rng.permutation(G)) if permute else (np.arange(P), np.arange(G))
    pid, gid, grp = [], [], []
    p0 = g0 = 0
    for g, (ne, ng) in enumerate(sizes):
        for a in range(ne):
            for b in range(ng):
                pid.append(pred_rows[p0 + a])
                gid.append(gt_rows[g0 + b])
                grp.append(g)
        p0, g0 = p0 + ne, g0 + ng
    pid, gid, grp = (np.asarray(a, np.int64) for a in (pid, gid, grp))
    c = len(pid)
    shuffle = rng.permutation(c)
    pid, gid, grp = pid[shuffle], gid[shuffle], grp[shuffle]
    if ties:
        errs = rng.randint(0, 6, size=(c, E)).astype(np.float32) / np.float32(8)
        scores = rng.randint(0, 3, size=P).astype(np.float64)
    else:
        errs = rng.uniform(0, 1, size=(c, E)).astype(np.float32)
        scores = rng.permutation(P).astype(np.float64) / max(P, 1)
    errs[rng.uniform(size=(c, E)) < nan_share] = np.nan
    thr = np.sort(rng.uniform(0.05, 0.95, size=(n_groups, E, n_theta)), axis=2)
    if ties:
        thr = np.round(thr * 8) / 8                                  # thresholds that errors hit exactly
    return dict(pred_id=pid, gt_id=gid, group_id=grp, errs=errs, scores=scores, thr=thr, n_pred=P, n_gt=G)


def ragged_sizes(seed, n_groups, max_est=6, max_gt=5):
    rng = np.random.RandomState(seed)
    return [(int(rng.randint(0, max_est + 1)), int(rng.randint(0, max_gt + 1))) for _ in range(n_groups)]


def pairs(match_col) -> set:
    """one problem's column of a match table -> {(pred row, gt row)}"""
    rows = np.flatnonzero(np.asarray(match_col) >= 0)
    return {(int(r), int(match_col[r])) for r in rows}
