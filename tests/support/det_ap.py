"""TEST SUPPORT: ctypes wrapper of the host emulation of the detection matching kernel (tests/det_ap_emul.cpp), built on first use; an
independent numpy restatement of the contract of csrc/det_ap_core.h and of COCO's accumulate, written from the contract's text and not
from the header or from `evaluation` (it works on the raw candidate table: no index, no sorted copy, sets of taken ground truths, plain
per-pixel `!= 0` masks); and the seeded and hand-written cases the CPU contract test and the GPU test share."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np

from .emul import CSRC, TESTS, _p, build

IOU_THRS = np.linspace(0.5, 0.95, 10)


def load():
    lib = build("det_ap_emul", [TESTS / "det_ap_emul.cpp", CSRC / "det_ap_core.h", CSRC / "bop_match_core.h"], fma=False)
    lib.det_match_emul.restype = C.c_int
    lib.mask_pair_counts_emul.restype = None
    lib.det_ap_emul_limits.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_int * 2)()
    load().det_ap_emul_limits(v)
    return dict(max_thetas=int(v[0]), max_pairs=int(v[1]))


def emul_index(iou_sorted, index, gt_ignore, thr, n_pred, n_top=None) -> np.ndarray:
    """the emulation on the arguments of the C ABI: iou_sorted [C] in the index's order, index = `evaluation.bop_match_index`"""
    iou_sorted = np.ascontiguousarray(iou_sorted, np.float64)
    thr = np.ascontiguousarray(thr, np.float64)
    ign = np.ascontiguousarray(gt_ignore, np.uint8)
    n_groups = len(index["group_n_gt"])
    assert iou_sorted.shape == (len(index["cand_gt"]),) and thr.ndim == 1
    n_top = None if n_top is None else np.ascontiguousarray(n_top, np.int32)
    match = np.empty((n_pred, len(thr)), np.int32)
    rc = load().det_match_emul(_p(iou_sorted), _p(index["cand_gt"]), _p(index["cand_lgt"]), _p(index["est_row"]), _p(index["est_off"]),
                               _p(index["group_est_off"]), _p(index["group_n_gt"]), _p(n_top), _p(ign), _p(thr), C.c_int(n_pred), C.c_int(n_groups),
                               C.c_int(len(thr)), _p(match))
    assert rc == 0
    return match


def emul(pred_id, gt_id, group_id, iou, scores, gt_ignore, thr=IOU_THRS, n_top=None) -> np.ndarray:
    """the emulation on a raw candidate table, through the product's index builder -> match [P,T]; n_top an int (every group) or None"""
    from megapose6d_amd import evaluation as ev

    index = ev.bop_match_index(pred_id, gt_id, group_id, scores)
    iou = np.asarray(iou, np.float64)
    cut = None if n_top is None else np.full(len(index["group_n_gt"]), int(n_top), np.int32)
    return emul_index(iou[index["order"]], index, gt_ignore, thr, len(scores), cut)


def emul_pair_counts(a, b) -> np.ndarray:
    a, b = np.ascontiguousarray(a).view(np.uint8).ravel(), np.ascontiguousarray(b).view(np.uint8).ravel()
    out = np.empty(3, np.int32)
    load().mask_pair_counts_emul(_p(a), _p(b), C.c_longlong(a.size), _p(out))
    return out


# the restatement --------------------------------------------------------------------------------------------------------------------
def restated_match(pred_id, gt_id, group_id, iou, scores, gt_ignore, thr=IOU_THRS, n_top=None, stats=None) -> np.ndarray:
    """The contract, from its text: per group and threshold, the estimates by decreasing score (ties: ascending pred row), cut to the
    first n_top; each looks at its ground truths that nobody took, first those not ignored, then (only if none of those is admissible)
    the ignored ones; within the class at hand it takes the largest IoU that is >= min(t, 1 - 1e-10), the last in gt row order on a tie.
    stats (a dict) counts what happened: ties, matches to ignored ground truths, estimates cut."""
    pred_id, gt_id, group_id = (np.asarray(a, np.int64) for a in (pred_id, gt_id, group_id))
    iou, scores, thr = np.asarray(iou, np.float64), np.asarray(scores, np.float64), np.asarray(thr, np.float64)
    ign = np.asarray(gt_ignore).astype(bool)
    match = np.full((len(scores), len(thr)), -1, np.int32)
    stats = {} if stats is None else stats
    for key in ("ties", "to_ignored", "cut"):
        stats.setdefault(key, 0)
    for g in (np.unique(group_id) if len(group_id) else []):
        rows = np.flatnonzero(group_id == g)
        ests = sorted(set(pred_id[rows].tolist()), key=lambda r: (-scores[r], r))
        if n_top:
            stats["cut"] += max(0, len(ests) - int(n_top))
            ests = ests[:int(n_top)]
        for k, t in enumerate(thr):
            bar = min(t, 1 - 1e-10)
            taken = set()
            for r in ests:
                free = [c for c in rows[pred_id[rows] == r] if gt_id[c] not in taken and iou[c] >= bar]
                for wanted in (False, True):
                    pool = [c for c in free if bool(ign[gt_id[c]]) == wanted]
                    if pool:
                        top = max(iou[c] for c in pool)
                        tied = [c for c in pool if iou[c] == top]
                        stats["ties"] += len(tied) > 1
                        stats["to_ignored"] += wanted
                        pick = max(tied, key=lambda c: gt_id[c])
                        taken.add(int(gt_id[pick]))
                        match[r, k] = gt_id[pick]
                        break
    return match


def restated_kept(pred_group, scores, n_top) -> np.ndarray:
    """pred_group [P]: any hashable per detection naming its (image, label) -> whether it is among the first n_top of it"""
    scores = np.asarray(scores, np.float64)
    kept = np.ones(len(scores), bool)
    if not n_top:
        return kept
    by_group = {}
    for r, g in enumerate(pred_group):
        by_group.setdefault(g, []).append(r)
    for rows in by_group.values():
        for r in sorted(rows, key=lambda r: (-scores[r], r))[int(n_top):]:
            kept[r] = False
    return kept


def restated_accumulate(match, scores, pred_labels, gt_labels, gt_ignore, kept, thr=IOU_THRS) -> Dict[str, object]:
    """COCO's accumulate and summarize from the issue's text, one detection at a time: precision [T,101,K], recall [T,K] over the labels
    with a ground truth that is not ignored, by ascending label; AP, AP50, AP75, AR, AP_per_label as np.mean over those arrays."""
    match, scores = np.asarray(match), np.asarray(scores, np.float64)
    pred_labels, gt_labels, ign, kept = np.asarray(pred_labels), np.asarray(gt_labels), np.asarray(gt_ignore).astype(bool), np.asarray(kept).astype(bool)
    labels = sorted(l for l in set(gt_labels.tolist()) if any(not ign[i] for i in range(len(ign)) if gt_labels[i] == l))
    rec_thrs = np.linspace(0, 1, 101)
    T = len(thr)
    precision, recall = np.zeros((T, 101, len(labels))), np.zeros((T, len(labels)))
    for k, label in enumerate(labels):
        npig = sum(1 for i in range(len(ign)) if gt_labels[i] == label and not ign[i])
        dets = sorted((r for r in range(len(scores)) if pred_labels[r] == label and kept[r]), key=lambda r: (-scores[r], r))
        for t in range(T):
            tp = fp = 0
            rc, pr = [], []
            for r in dets:
                m = match[r, t]
                if m < 0:
                    fp += 1
                elif not ign[m]:
                    tp += 1
                rc.append(np.float64(tp) / npig)
                pr.append(np.float64(tp) / (np.float64(fp) + np.float64(tp) + np.spacing(1)))
            recall[t, k] = rc[-1] if dets else 0.0
            for i in range(len(pr) - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            for ri, want in enumerate(rec_thrs):
                at = next((i for i, v in enumerate(rc) if v >= want), None)            # searchsorted(side="left")
                precision[t, ri, k] = pr[at] if at is not None else 0.0
    if not labels:
        return dict(AP=-1.0, AP50=-1.0, AP75=-1.0, AR=-1.0, AP_per_label={}, labels=[])

    def at_thr(value):
        hit = [t for t in range(T) if abs(thr[t] - value) < 1e-9]
        return float(np.mean(precision[hit[0]])) if hit else -1.0

    return dict(AP=float(np.mean(precision)), AP50=at_thr(0.5), AP75=at_thr(0.75), AR=float(np.mean(recall)),
                AP_per_label={l: float(np.mean(precision[:, :, k])) for k, l in enumerate(labels)}, labels=labels)


def restated_pair_counts(pred_masks, gt_masks, cand_pred, cand_gt) -> np.ndarray:
    a, b = np.asarray(pred_masks) != 0, np.asarray(gt_masks) != 0
    out = np.empty((len(cand_pred), 3), np.int32)
    for c, (i, j) in enumerate(zip(cand_pred, cand_gt)):
        out[c] = [(a[i] & b[j]).sum(), a[i].sum(), b[j].sum()]
    return out


def restated_mask_iou(counts) -> np.ndarray:
    counts = np.asarray(counts, np.float64)
    union = counts[:, 1] + counts[:, 2] - counts[:, 0]
    return np.where(union > 0, counts[:, 0] / np.where(union > 0, union, 1.0), 0.0)


def restated_box_iou(pred_boxes, gt_boxes, cand_pred, cand_gt) -> np.ndarray:
    """the expression order of `evaluation.box_iou`'s docstring, in numpy float64"""
    p, g = np.asarray(pred_boxes, np.float64)[cand_pred], np.asarray(gt_boxes, np.float64)[cand_gt]
    iw = np.maximum(np.minimum(p[:, 2], g[:, 2]) - np.maximum(p[:, 0], g[:, 0]), 0)
    ih = np.maximum(np.minimum(p[:, 3], g[:, 3]) - np.maximum(p[:, 1], g[:, 1]), 0)
    inter = iw * ih
    union = ((p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]) + (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])) - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)


# seeded cases shared by the CPU contract test and the GPU test --------------------------------------------------------------------
def case(seed, sizes, ties=True, nan_share=0.02, ignore_share=0.3):
    """sizes = [(n_est, n_gt)] per group: full cross products with shuffled rows.  With `ties`, IoUs and scores are drawn from a few
    values (eighths, so that thresholds are hit exactly) and both kinds of tie are frequent; a share of NaN IoUs and of ignored ground
    truths.  -> dict(pred_id, gt_id, group_id, iou [C], scores [P], gt_ignore [G], n_pred, n_gt)"""
    rng = np.random.RandomState(seed)
    P, G = sum(s[0] for s in sizes), sum(s[1] for s in sizes)
    pred_rows, gt_rows = rng.permutation(P), rng.permutation(G)
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
    # group ids must be dense over the groups that have a candidate
    grp = np.unique(grp, return_inverse=True)[1].astype(np.int64) if len(grp) else grp
    c = len(pid)
    shuffle = rng.permutation(c)
    pid, gid, grp = pid[shuffle], gid[shuffle], grp[shuffle]
    if ties:
        iou = rng.randint(2, 9, size=c).astype(np.float64) / 8.0
        scores = rng.randint(0, 3, size=P).astype(np.float64)
    else:
        iou = rng.uniform(0.2, 1.0, size=c)
        scores = rng.permutation(P).astype(np.float64) / max(P, 1)
    iou[rng.uniform(size=c) < nan_share] = np.nan
    return dict(pred_id=pid, gt_id=gid, group_id=grp, iou=iou, scores=scores, gt_ignore=rng.uniform(size=G) < ignore_share, n_pred=P, n_gt=G)


def ragged_sizes(seed, n_groups, max_est=6, max_gt=5):
    rng = np.random.RandomState(seed)
    return [(int(rng.randint(0, max_est + 1)), int(rng.randint(0, max_gt + 1))) for _ in range(n_groups)]


SEEDED = dict(seed=11, n_groups=150, n_top=3)          # the seeded table of both test files; its cut is n_top per group


def seeded():
    return case(SEEDED["seed"], ragged_sizes(SEEDED["seed"] + 1, SEEDED["n_groups"]))


def hand(triples, scores, gt_ignore, group=None) -> dict:
    """(pred, gt, iou) triples of ONE group unless `group` is given -> a case"""
    pid, gid = (np.asarray([t[i] for t in triples], np.int64) for i in range(2))
    iou = np.asarray([t[2] for t in triples], np.float64)
    grp = np.zeros(len(triples), np.int64) if group is None else np.asarray(group, np.int64)
    return dict(pred_id=pid, gt_id=gid, group_id=grp, iou=iou, scores=np.asarray(scores, np.float64), gt_ignore=np.asarray(gt_ignore, bool))


def hand_cases():
    """name -> (case, thresholds, n_top, expected match table as lists): the hand-written cases of the contract, shared with the GPU test"""
    t5 = np.array([0.5])
    big = hand([(0, g, 0.5 + 0.005 * g) for g in range(70)] + [(1, g, 0.6 if g == 69 else 0.9 - 0.005 * g) for g in range(70)], [0.9, 0.8],
               [False] * 70)
    return {
        # intersection 1, union 2 is exactly 0.5: it matches at 0.5 and not above
        "iou exactly at a threshold": (hand([(0, 0, 1 / 2)], [1.0], [False]), np.array([0.5, np.nextafter(0.5, 1)]), None, [[0, -1]]),
        # the bar of threshold 1.0 is 1 - 1e-10: IoU 1.0 passes it, the largest double below the bar does not
        "iou 1.0 against the capped bar": (hand([(0, 0, 1.0), (1, 1, np.nextafter(1 - 1e-10, 0))], [1.0, 0.9], [False, False]), np.array([1.0]), None,
                                           [[0], [-1]]),
        "two ground truths tied in iou: the last": (hand([(0, 3, 0.75), (0, 1, 0.75), (0, 2, 0.5)], [1.0], [False] * 4), t5, None, [[3]]),
        "an ignored ground truth with the higher iou loses": (hand([(0, 0, 0.9), (0, 1, 0.6)], [1.0], [True, False]), t5, None, [[1]]),
        # estimate 0 reaches only the ignored ground truth 0 and takes it; estimate 1 then finds it taken
        "only an ignored ground truth, then taken": (hand([(0, 0, 0.8), (0, 1, 0.3), (1, 0, 0.9)], [0.9, 0.5], [True, False]), t5, None, [[0], [-1]]),
        "score ties are broken by pred row": (hand([(1, 0, 0.9), (0, 0, 0.6)], [0.5, 0.5], [False]), t5, None, [[0], [-1]]),
        "the n_top cut": (hand([(0, 0, 0.2), (1, 0, 0.9)], [0.9, 0.5], [False]), t5, 1, [[-1], [-1]]),
        "without the cut": (hand([(0, 0, 0.2), (1, 0, 0.9)], [0.9, 0.5], [False]), t5, None, [[-1], [0]]),
        # 70 ground truths: estimate 0 takes the last (largest IoU), estimate 1 then its best free one (gt 0), not gt 69
        "a group with more than 64 ground truths": (big, t5, None, [[69], [0]]),
        "an estimate without candidates": (hand([(0, 0, 0.9)], [0.5, 0.9, 0.7], [False]), t5, None, [[0], [-1], [-1]]),
        "nan iou never matches": (hand([(0, 0, np.nan), (0, 1, 0.6), (1, 0, np.nan)], [0.9, 0.5], [False, False]), np.array([0.5, 0.0]), None,
                                  [[1, 1], [-1, -1]]),
    }
