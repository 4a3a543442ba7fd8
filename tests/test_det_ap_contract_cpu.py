"""CPU: the contract of BOP's detection / segmentation scores (csrc/det_ap_core.h: COCO's greedy matching; `evaluation.coco_accumulate`:
COCO's accumulate).  The host emulation (tests/det_ap_emul.cpp: the lines the kernel compiles) against an independent numpy
restatement written from the contract's text, on seeded tables and on hand-written cases that pin every edge; the host arithmetic of
`evaluation` against the restatement bit for bit and against answers worked out by hand.  pycocotools and bop_toolkit are absent: the
scores are unpinned against them.  Matches compare exactly; known answers within 1e-12."""
import numpy as np
import pandas as pd
import pytest
import torch

from support import det_ap as da


def _ev():
    from megapose6d_amd import evaluation as ev

    return ev


def _both(c, thr=da.IOU_THRS, n_top=None, stats=None):
    args = (c["pred_id"], c["gt_id"], c["group_id"], c["iou"], c["scores"], c["gt_ignore"], thr, n_top)
    a, b = da.emul(*args), da.restated_match(*args, stats=stats)
    assert a.dtype == np.int32 and a.shape == (len(c["scores"]), len(thr)) and np.array_equal(a, b)
    return a


def test_emulation_matches_the_restatement_on_the_seeded_table():
    c = da.seeded()
    # what the seed was picked for, counted by the restatement: ties, matches to ignored ground truths, estimates cut
    stats = {}
    da.restated_match(c["pred_id"], c["gt_id"], c["group_id"], c["iou"], c["scores"], c["gt_ignore"], da.IOU_THRS, da.SEEDED["n_top"], stats=stats)
    assert stats["ties"] >= 1 and stats["to_ignored"] >= 1 and stats["cut"] >= 1, stats
    assert np.isnan(c["iou"]).any() and len(set(c["scores"].tolist())) < len(c["scores"])
    full = _both(c)
    cut = _both(c, n_top=da.SEEDED["n_top"])
    assert (full >= 0).any() and 0 < (cut >= 0).sum() < (full >= 0).sum()
    # a ground truth is given once per threshold; the matches thin out as the threshold rises
    for k in range(full.shape[1]):
        got = full[:, k][full[:, k] >= 0]
        assert len(set(got.tolist())) == len(got)
    assert (full[:, 0] >= 0).sum() > (full[:, -1] >= 0).sum()


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n_theta,n_groups", [(1, 60), (10, 80), (16, 30)])
def test_emulation_matches_the_restatement_on_ragged_groups(n_theta, n_groups, ties):
    c = da.case(3 * n_theta + ties, da.ragged_sizes(50 + n_theta, n_groups), ties=ties)
    thr = np.linspace(0.25, 1.0, n_theta) if n_theta > 1 else np.array([0.5])
    full = _both(c, thr)
    cut = _both(c, thr, n_top=2)
    assert (full >= 0).any() and (cut >= 0).sum() <= (full >= 0).sum()


@pytest.mark.parametrize("name", list(da.hand_cases()))
def test_hand_written_cases(name):
    c, thr, n_top, want = da.hand_cases()[name]
    assert _both(c, thr, n_top).tolist() == want


def test_the_word_test_of_the_pair_counts_marks_exactly_the_non_zero_bytes():
    rng = np.random.RandomState(0)
    for n in (1, 7, 8, 9, 91, 2145, 4096):
        a = rng.choice(np.array([0, 0, 1, 2, 127, 128, 129, 254, 255], np.uint8), size=n)
        b = rng.choice(np.array([0, 1, 255, 0x80, 0x7f], np.uint8), size=n)
        assert da.emul_pair_counts(a, b).tolist() == [int(((a != 0) & (b != 0)).sum()), int((a != 0).sum()), int((b != 0).sum())]
    every = np.arange(256, dtype=np.uint8)
    assert da.emul_pair_counts(every, every[::-1].copy()).tolist() == [254, 255, 255]


# the host side of evaluation ------------------------------------------------------------------------------------------------------------
def _labelled(c, seed, n_labels=4):
    """labels for the estimates and ground truths of a case: a group's members share one; some estimates belong to no group"""
    rng = np.random.RandomState(seed)
    group_label = rng.randint(0, n_labels, size=int(c["group_id"].max()) + 1)
    pred_labels, gt_labels = rng.randint(0, n_labels, size=c["n_pred"]), rng.randint(0, n_labels, size=c["n_gt"])
    pred_labels[c["pred_id"]] = group_label[c["group_id"]]
    gt_labels[c["gt_id"]] = group_label[c["group_id"]]
    names = np.array(["obj_%02d" % i for i in range(n_labels)])
    pred_group = np.full(c["n_pred"], -1, np.int64)
    pred_group[c["pred_id"]] = c["group_id"]
    lone = np.flatnonzero(pred_group < 0)
    pred_group[lone] = 10_000 + np.arange(len(lone)) // 2          # estimates without ground truth: two per (image, label)
    pred_labels[lone] = pred_labels[lone[(np.arange(len(lone)) // 2) * 2]]
    return names[pred_labels], names[gt_labels], pred_group


@pytest.mark.parametrize("n_top", [None, 2])
def test_coco_accumulate_equals_the_restatement_bit_for_bit(n_top):
    ev = _ev()
    c = da.seeded()
    pred_labels, gt_labels, pred_group = _labelled(c, 4)
    match = da.restated_match(c["pred_id"], c["gt_id"], c["group_id"], c["iou"], c["scores"], c["gt_ignore"], da.IOU_THRS, n_top)
    kept = da.restated_kept(pred_group.tolist(), c["scores"], n_top)
    infos = pd.DataFrame(dict(batch_im_id=pred_group, label=pred_labels))
    assert np.array_equal(ev.coco_kept(infos, c["scores"], n_top=n_top), kept) and (n_top is None or not kept.all())
    assert ((match >= 0).any(axis=1) <= kept).all()                                  # a cut estimate has no match
    got = ev.coco_accumulate(match, c["scores"], pred_labels, gt_labels, c["gt_ignore"], kept)
    want = da.restated_accumulate(match, c["scores"], pred_labels, gt_labels, c["gt_ignore"], kept)
    assert got == want and list(got) == ["AP", "AP50", "AP75", "AR", "AP_per_label", "labels"]
    assert 0.05 < got["AP"] < got["AP50"] < 0.95 and got["AP75"] < got["AP50"] and 0 < got["AR"] < 1 and len(got["labels"]) == 4
    assert np.array_equal(ev.COCO_IOU_THRS, da.IOU_THRS)


def _table(gt_labels, gt_ignore, dets):
    """dets = [(label, score, matched gt row or -1)]: the same match at every threshold"""
    match = np.repeat(np.asarray([d[2] for d in dets], np.int32).reshape(-1, 1), 10, axis=1)
    return _ev().coco_accumulate(match, [d[1] for d in dets], np.asarray([d[0] for d in dets], dtype=object).astype(str), np.asarray(gt_labels),
                                 np.asarray(gt_ignore, bool), np.ones(len(dets), bool))


def test_known_answers():
    gt_labels = ["a", "a", "b", "c", "c"]
    ign = [False, False, False, True, True]                                          # label c has only ignored ground truths
    perfect = _table(gt_labels, ign, [("a", 0.9, 0), ("a", 0.8, 1), ("b", 0.7, 2), ("c", 0.6, 3), ("a", 0.1, -1)])
    for key in ("AP", "AP50", "AP75", "AR"):
        assert abs(perfect[key] - 1.0) < 1e-12, key                                  # the false positive ranks last: it costs nothing
    assert perfect["labels"] == ["a", "b"] and set(perfect["AP_per_label"]) == {"a", "b"}
    none = _ev().coco_accumulate(np.zeros((0, 10), np.int32), [], np.zeros(0, str), np.asarray(gt_labels), np.asarray(ign), np.zeros(0, bool))
    assert none["AP"] == none["AR"] == none["AP50"] == 0.0 and none["labels"] == ["a", "b"]
    only_ignored = _table(["c"], [True], [("c", 0.9, 0)])
    assert only_ignored["AP"] == -1.0 and only_ignored["labels"] == []
    # one extra unmatched detection ranked first on label a (2 ground truths, both then detected): tp = 0 1 2, fp = 1 1 1, recall = 0 .5
    # 1, precision = 0 1/2 2/3 -> envelope 2/3 everywhere: AP(a) = 2/3 at every threshold, AP(b) = 1; AR stays 1
    extra = _table(gt_labels, ign, [("a", 0.95, -1), ("a", 0.9, 0), ("a", 0.8, 1), ("b", 0.7, 2)])
    assert abs(extra["AP_per_label"]["a"] - 2 / 3) < 1e-12 and abs(extra["AP_per_label"]["b"] - 1.0) < 1e-12
    assert abs(extra["AP"] - (2 / 3 + 1) / 2) < 1e-12 and abs(extra["AP50"] - 5 / 6) < 1e-12 and abs(extra["AR"] - 1.0) < 1e-12
    # a detection matched to an ignored ground truth is neither: it does not lower the precision
    with_ignored = _table(["a", "a"], [False, True], [("a", 0.9, 1), ("a", 0.8, 0)])
    assert abs(with_ignored["AP"] - 1.0) < 1e-12
    # an estimate cut by n_top is dropped: the false positive no longer counts
    match = np.repeat(np.int32([[-1], [0]]), 10, axis=1)
    cut = _ev().coco_accumulate(match, [0.9, 0.8], np.array(["a", "a"]), np.array(["a"]), np.zeros(1, bool), np.array([False, True]))
    assert abs(cut["AP"] - 1.0) < 1e-12
    for bad in (dict(match=match[:, :3]), dict(kept=np.ones(2, np.int32)), dict(ign=np.zeros(1, np.int32)), dict(match=match + 1)):
        with pytest.raises(ValueError):
            _ev().coco_accumulate(bad.get("match", match), [0.9, 0.8], np.array(["a", "a"]), np.array(["a"]), bad.get("ign", np.zeros(1, bool)),
                                  bad.get("kept", np.ones(2, bool)))


def test_box_iou_follows_the_expression_order_of_its_docstring():
    ev = _ev()
    rng = np.random.RandomState(2)
    n = 400
    xy = rng.uniform(-20, 600, size=(2, n, 2))
    wh = rng.uniform(0, 200, size=(2, n, 2)) * (rng.uniform(size=(2, n, 1)) > 0.05)      # a few empty boxes
    boxes = np.concatenate([xy, xy + wh], axis=2).astype(np.float32)
    boxes[1, :40] = boxes[0, :40]                                                          # identical boxes: IoU 1 (0 for the empty ones)
    boxes[1, 40] = [-1, -1, -1, -1]                                                        # gt_info's blank box
    pid, gid = rng.randint(0, n, size=3000), rng.randint(0, n, size=3000)
    pid[:41], gid[:41] = np.arange(41), np.arange(41)
    got = ev.box_iou(torch.from_numpy(boxes[0]), torch.from_numpy(boxes[1]), (pid, gid))
    want = da.restated_box_iou(boxes[0], boxes[1], pid, gid)
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want)
    area = (boxes[0, :40, 2] - boxes[0, :40, 0]) * (boxes[0, :40, 3] - boxes[0, :40, 1])
    assert np.array_equal(want[:40], (area > 0).astype(np.float64)) and want[40] == 0.0 and 0 < (want > 0).mean() < 1
    cand = pd.DataFrame(dict(pred_id=pid, gt_id=gid))
    assert torch.equal(ev.box_iou(torch.from_numpy(boxes[0]), torch.from_numpy(boxes[1]), cand), got)
    # a box with a one-pixel side: w = x2 - x1 with no +1
    one = ev.box_iou(torch.tensor([[0.0, 0.0, 2.0, 2.0]]), torch.tensor([[1.0, 0.0, 3.0, 2.0]]), ([0], [0]))
    assert one.tolist() == [2.0 / 6.0]


def test_limits_are_stated_once():
    from megapose6d_amd import engine as eng

    assert da.limits() == dict(max_thetas=eng.DET_MATCH_MAX_THETAS, max_pairs=eng.MASK_PAIR_MAX_PAIRS)
