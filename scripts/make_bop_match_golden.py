#!/usr/bin/env python3
"""Write tests/golden/bop_match.npz: what the REFERENCE's own matching (evaluation/meters/utils.py: add_valid_gt,
get_candidate_matches, get_top_n_ids, match_poses -- loaded from the reference checkout as a file: it needs numpy and pandas only)
returns on seeded tables of a few hundred estimates and ground truths.  Needs the reference checkout, so it runs where that exists;
the tests read the fixture only.

Recorded, for E error columns and K thresholds per column:
  * add_valid_gt's mask for visib_gt_min = 0.1, and the candidate table of get_candidate_matches(only_valids=True);
  * for every (column, theta) the pairs match_poses(cand[cand.error < theta]) returns, as a table match_all [P,E,K] of gt rows (-1: none);
  * the same after get_top_n_ids(pred, targets=...) has cut the estimates of each group to the targets' inst_count (= the group's
    number of valid ground truths): match_top, with the rows it kept.

The reference is indeterminate on ties (`sort_values` is not stable, `<` keeps an arbitrary first candidate), so the tables have
pairwise distinct scores within a group and pairwise distinct errors per estimate and column; that is asserted before recording.

Usage: python scripts/make_bop_match_golden.py
"""
from __future__ import annotations

import importlib.util
import sys
import warnings
from pathlib import Path

import numpy as np
import pandas as pd

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import ref_import  # noqa: E402

OUT = ROOT / "tests" / "golden" / "bop_match.npz"
KEYS = ["scene_id", "view_id", "label"]
E, K = 3, 6


def load_reference_utils():
    path = ref_import.REFERENCE_SRC / "megapose" / "evaluation" / "meters" / "utils.py"
    spec = importlib.util.spec_from_file_location("reference_meters_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tables(rng):
    """120 (scene, view, label) groups with 0-5 estimates and 0-4 ground truths each, rows shuffled"""
    pred, gt = [], []
    for g in range(120):
        key = dict(scene_id=g // 30, view_id=(g // 5) % 6, label=f"obj_{g % 5:06d}")
        n_est, n_gt = int(rng.randint(0, 6)), int(rng.randint(0, 5))
        pred += [dict(key) for _ in range(n_est)]
        gt += [dict(key, visib_fract=float(rng.choice([0.0, 0.05, 0.3, 0.8, 1.0]))) for _ in range(n_gt)]
    pred, gt = pd.DataFrame(pred), pd.DataFrame(gt)
    pred["score"] = rng.permutation(len(pred)).astype(np.float64) / len(pred)        # pairwise distinct
    pred = pred.iloc[rng.permutation(len(pred))].reset_index(drop=True)
    gt = gt.iloc[rng.permutation(len(gt))].reset_index(drop=True)
    return pred, gt


def match_table(ru, cand, errs, thetas, n_pred, orig_pred):
    out = np.full((n_pred, E, K), -1, np.int32)
    for e in range(E):
        for k in range(K):
            c = cand.copy()
            c["error"] = errs[:, e].astype(np.float64)
            c = c[c["error"] < thetas[e, k]]
            m = ru.match_poses(c, group_keys=KEYS)
            if len(m) == 0:
                continue
            rows = orig_pred[m["pred_id"].to_numpy().astype(np.int64)]
            assert len(set(rows.tolist())) == len(rows)
            out[rows, e, k] = m["gt_id"].to_numpy().astype(np.int32)
    return out


def main() -> int:
    warnings.simplefilter("ignore")
    ru = load_reference_utils()
    rng = np.random.RandomState(11)
    pred, gt = tables(rng)
    n_pred = len(pred)
    gt = ru.add_valid_gt(gt, group_keys=KEYS, visib_gt_min=0.1)
    valid = gt["valid"].to_numpy().astype(np.bool_)
    cand = ru.get_candidate_matches(pred.copy(), gt.copy(), group_keys=KEYS, only_valids=True)
    cand_pred, cand_gt = cand["pred_id"].to_numpy().astype(np.int64), cand["gt_id"].to_numpy().astype(np.int64)
    # errors: float32 values, pairwise distinct per estimate and column (distinct over the whole column, in fact)
    errs = np.stack([(rng.permutation(len(cand)).astype(np.float64) + rng.uniform(0.1, 0.9, len(cand))) / len(cand) for _ in range(E)], axis=1)
    errs = errs.astype(np.float32)
    thetas = np.stack([np.linspace(0.15, 0.9, K) * s for s in (1.0, 0.8, 1.1)]).astype(np.float64)
    for e in range(E):
        assert len(np.unique(errs[:, e])) == len(cand), "errors must be pairwise distinct"
    for _, rows in pred.groupby(KEYS).groups.items():
        assert len(set(pred.loc[rows, "score"])) == len(rows), "scores must be pairwise distinct within a group"
    match_all = match_table(ru, cand, errs, thetas, n_pred, np.arange(n_pred))
    # the cut: targets = one row per group that has a valid ground truth, inst_count = their number
    targets = gt[gt["valid"]].groupby(KEYS).size().reset_index(name="inst_count")
    keep = np.sort(np.asarray(ru.get_top_n_ids(pred.copy(), group_keys=KEYS, top_key="score", targets=targets)).astype(np.int64))
    pred_top = pred.iloc[keep].reset_index(drop=True)
    cand_top = ru.get_candidate_matches(pred_top.copy(), gt.copy(), group_keys=KEYS, only_valids=True)
    pair_err = {(int(p), int(g)): errs[i] for i, (p, g) in enumerate(zip(cand_pred, cand_gt))}
    errs_top = np.stack([pair_err[(int(keep[p]), int(g))] for p, g in zip(cand_top["pred_id"], cand_top["gt_id"])])
    match_top = match_table(ru, cand_top, errs_top, thetas, n_pred, keep)
    out = dict(pred_scene_id=pred["scene_id"].to_numpy().astype(np.int64), pred_view_id=pred["view_id"].to_numpy().astype(np.int64),
               pred_label=pred["label"].to_numpy().astype(str), pred_score=pred["score"].to_numpy().astype(np.float64),
               gt_scene_id=gt["scene_id"].to_numpy().astype(np.int64), gt_view_id=gt["view_id"].to_numpy().astype(np.int64),
               gt_label=gt["label"].to_numpy().astype(str), gt_visib_fract=gt["visib_fract"].to_numpy().astype(np.float64), gt_valid=valid,
               cand_pred_id=cand_pred, cand_gt_id=cand_gt, errs=errs, thetas=thetas, match_all=match_all, match_top=match_top, top_keep=keep)
    out["notes"] = np.array("the reference's evaluation/meters/utils.py on seeded tables (keys scene_id, view_id, label): gt_valid = add_valid_gt("
                            "visib_gt_min=0.1); cand_* = get_candidate_matches(only_valids=True); match_all[p,e,k] = the gt_id match_poses(cand["
                            "cand.error < thetas[e,k]]) pairs with pred_id p under error column e (-1: none); match_top = the same on the rows "
                            "top_keep = get_top_n_ids(pred, top_key='score', targets=...) keeps, targets' inst_count = the group's number of valid "
                            "ground truths; errors are float32 values compared as float64; scores distinct within a group, errors distinct")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes): {n_pred} estimates, {len(gt)} ground truths ({int(valid.sum())} valid), {len(cand)} candidates, "
          f"{int((match_all >= 0).sum())} / {int((match_top >= 0).sum())} matches over {E * K} problems")
    return 0


if __name__ == "__main__":
    sys.exit(main())
