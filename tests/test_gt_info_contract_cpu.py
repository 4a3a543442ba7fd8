"""CPU: the contract of the ground-truth-info arithmetic (megapose6d_amd/csrc/gt_info_core.h) through the host emulation
(tests/gt_info_emul.cpp), against hand-written counts and boxes and against an independent float64 restatement of the definition
(tests/support/gt_info.py), and the host logic on top (`evaluation.gt_info_table`, `detections_from_gt_info`, `bop_recall(valid=)`).
Reads nothing outside the tree.

THE BORDERLINE BAND.  Of the four counts and two boxes only px_count_visib and bbox_visib depend on rounded arithmetic, through the one
compared quantity dist_gt - dist_test - delta, which is VSD's: the derivation in tests/test_vsd_contract_cpu.py gives 12 roundings' worth on
the difference, the band is 16 * 2^-24 * D_max.  obj (depth_gt > 0), the observed test (dist_test > 0: a positive depth times r >= 1), the
other three counts, bbox_obj and the mask are exact on both sides and must be EQUAL.  px_count_visib may differ by at most the number of
borderline pixels; a bound of bbox_visib may differ only where a borderline pixel is the unique extreme of the box, i.e. it must lie
between the box of the visible pixels without any borderline pixel and the box with every one of them.  visib_fract is one division of
the emulation's own counts.

THE GUARD.  On the seeded scenes of 48 x 64 and larger px_count_visib >= 1000 and the borderline pixels are at most 1 % of px_count_visib,
measured from the float64 restatement alone (observed: printed by the tests, recorded in DESIGN 3.9), so the rule cannot hide a wrong count.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from support import gt_info as gi
from support import vsd as vs

_K = vs.intrinsics


def _both(gt, test, K, canvas, **kw):
    """emulation and float64 on hand-made inputs that have no borderline pixel: the two must agree exactly"""
    a = gi.gt_info(gt, test, K, canvas, **kw)
    r = gi.f64_gt_info(gt, test, K, canvas, **kw)
    assert np.all(r["borderline"] == 0)
    assert np.array_equal(a["counts"], r["counts"]) and np.array_equal(a["boxes"], r["boxes"])
    assert np.array_equal(a["mask"] == 255, r["mask"]) and np.array_equal(a["mask_visib"] == 255, r["mask_visib"])
    assert np.all((a["mask"] == 0) | (a["mask"] == 255)) and np.all((a["mask_visib"] == 0) | (a["mask_visib"] == 255))
    assert np.array_equal(np.isnan(a["visib_fract"]), np.isnan(r["visib_fract"]))
    ok = ~np.isnan(r["visib_fract"])
    assert np.array_equal(a["visib_fract"][ok], r["visib_fract"][ok].astype(np.float32))
    return a


K3 = _K(100.0, 1.5, 1.5)[None]


def test_three_by_three_map_with_known_counts_and_boxes():
    gt = np.zeros((1, 1, 3, 3), np.float32)
    gt[0, 0, 0:2, 1:3] = 1.0                                   # 4 object pixels: x 1..2, y 0..1
    test = np.zeros((1, 3, 3), np.float32)
    test[0, 0, 1] = 0.5                                        # an occluder 0.5 m nearer over (1, 0)
    test[0, 1, 2] = 1.0                                        # the surface itself over (2, 1)
    out = _both(gt, test, K3, 1)
    assert list(out["counts"][0]) == [4, 4, 2, 3] and out["visib_fract"][0] == np.float32(0.75)
    assert list(out["boxes"][0]) == [1, 0, 2, 1, 1, 0, 2, 1]    # (1, 1) and (2, 0) are unobserved: visible, and they span the box
    assert out["mask"][0].tolist() == [[0, 255, 255], [0, 255, 255], [0, 0, 0]]
    assert out["mask_visib"][0].tolist() == [[0, 0, 255], [0, 255, 255], [0, 0, 0]]
    # the same object on the centre tile of a 3 x 3 canvas, a two-pixel piece of it in the tile above and one in the tile to the right
    big = np.zeros((1, 9, 3, 3), np.float32)
    big[0, 4] = gt[0, 0]
    big[0, 1, 2, 1:3] = 1.0                                    # tile (0, 1): image y = 2 - 3 = -1, x 1..2
    big[0, 5, 0, 0] = 1.0                                      # tile (1, 2): image x = 0 + 3 = 3, y 0
    out = _both(big, test, K3, 3)
    assert list(out["counts"][0]) == [7, 4, 2, 3] and out["visib_fract"][0] == np.float32(3) / np.float32(7)
    assert list(out["boxes"][0]) == [1, -1, 3, 1, 1, 0, 2, 1]


def test_an_object_only_in_an_outer_tile():
    gt = np.zeros((1, 9, 4, 5), np.float32)
    gt[0, 3, 1:3, 2:4] = 0.8                                   # tile (1, 0): image x = 2 - 5 .. 3 - 5 = -3 .. -2, y 1..2
    out = _both(gt, np.full((1, 4, 5), 1.0, np.float32), _K(50.0, 2.5, 2.0)[None], 3)
    assert list(out["counts"][0]) == [4, 0, 0, 0] and out["visib_fract"][0] == 0
    assert list(out["boxes"][0]) == [-3, 1, -2, 2, -1, -1, -1, -1]
    assert not out["mask"].any() and not out["mask_visib"].any()
    # nothing anywhere: px_count_all == 0 gives visib_fract 0 and two blank boxes
    out = _both(np.zeros_like(gt), np.zeros((1, 4, 5), np.float32), _K(50.0, 2.5, 2.0)[None], 3)
    assert list(out["counts"][0]) == [0, 0, 0, 0] and out["visib_fract"][0] == 0 and list(out["boxes"][0]) == [-1] * 8


def test_nan_negative_and_zero_observed_depths_count_as_unobserved():
    gt = np.zeros((1, 1, 4, 4), np.float32)
    gt[0, 0, 1:3, 1:3] = 1.0
    for bad in (np.nan, -1.0, 0.0, np.inf, -np.inf):
        out = _both(gt, np.full((1, 4, 4), bad, np.float32), _K(80.0, 2.0, 2.0)[None], 1)
        assert list(out["counts"][0]) == [4, 4, 0, 4]             # visible, not valid
        assert list(out["boxes"][0]) == [1, 1, 2, 2, 1, 1, 2, 2] and out["visib_fract"][0] == 1
    out = _both(gt, np.full((1, 4, 4), 0.5, np.float32), _K(80.0, 2.0, 2.0)[None], 1)
    assert list(out["counts"][0]) == [4, 4, 4, 0] and list(out["boxes"][0]) == [1, 1, 2, 2, -1, -1, -1, -1]   # each box blank on its own


def test_exact_hit_on_delta():
    K1 = _K(50.0, 0.5, 0.5)[None]                               # a 1 x 1 map whose ray is the optical axis: r = 1 exactly
    one = lambda z: np.full((1, 1, 1), z, np.float32)           # noqa: E731
    out = gi.gt_info(one(1.0)[None], one(0.75), K1, 1, delta=0.25)
    assert list(out["counts"][0]) == [1, 1, 1, 1] and list(out["boxes"][0]) == [0] * 8
    out = gi.gt_info(one(1.0)[None], one(np.float32(0.75) - np.float32(2.0 ** -24)), K1, 1, delta=0.25)
    assert list(out["counts"][0]) == [1, 1, 1, 0] and list(out["boxes"][0]) == [0, 0, 0, 0, -1, -1, -1, -1]


def test_a_non_finite_k_gives_minus_one_nan_and_zero_masks():
    c = gi.case(3, 4, 12, 16, 3)
    c["K"][1, 0, 0] = np.nan
    c["K"][2, 2, 1] = np.inf
    out = _both(c["gt"], c["test"], c["K"], 3)
    for i in (1, 2):
        assert np.all(out["counts"][i] == -1) and np.all(out["boxes"][i] == -1) and np.isnan(out["visib_fract"][i])
        assert not out["mask"][i].any() and not out["mask_visib"][i].any()
    assert out["counts"][0, 1] > 0 and out["counts"][3, 1] > 0


# --------------------------------------------------------------------------------------------------------------------------------
def check_against_f64(c, got, guard=True):
    r = gi.f64_gt_info(c["gt"], c["test"], c["K"], c["canvas"], gt_ids=c["gt_ids"], im_ids=c["im_ids"])
    n_vis = r["counts"][:, 3]
    share = 100.0 * r["borderline"] / np.maximum(1, n_vis)
    diff = np.abs(got["counts"].astype(np.int64) - r["counts"])
    print(f"px_count_visib {n_vis.min()} .. {n_vis.max()}; borderline pixels {int(r['borderline'].sum())} (per row {share.min():.4f} .. {share.max():.4f} % of "
          f"px_count_visib); counts differ from float64 at {int(diff.sum())} pixels")
    assert np.array_equal(got["counts"][:, :3], r["counts"][:, :3]) and np.all(diff[:, 3] <= r["borderline"])
    assert np.array_equal(got["boxes"][:, :4], r["boxes"][:, :4]) and np.array_equal(got["mask"] == 255, r["mask"])
    flips = (got["mask_visib"] == 255) != r["mask_visib"]
    assert not np.any(flips & ~r["near"])                       # only a borderline pixel may fall the other way
    for i in range(len(n_vis)):
        inner, outer = gi.visib_box_range(r, i)
        box = got["boxes"][i, 4:]
        if inner == outer:
            assert list(box) == inner
        elif inner != [-1] * 4 and list(box) != [-1] * 4:
            assert outer[0] <= box[0] <= inner[0] and outer[1] <= box[1] <= inner[1] and inner[2] <= box[2] <= outer[2] and inner[3] <= box[3] <= outer[3]
    if guard:
        assert np.all(n_vis >= 1000), n_vis.min()
        assert np.all(r["borderline"] <= 0.01 * n_vis)
    want = np.where(got["counts"][:, 0] == 0, 0.0, got["counts"][:, 3].astype(np.float64) / np.maximum(got["counts"][:, 0], 1)).astype(np.float32)
    assert np.array_equal(got["visib_fract"], want)
    return r


def _emul(c):
    return gi.gt_info(c["gt"], c["test"], c["K"], c["canvas"], gt_ids=c["gt_ids"], im_ids=c["im_ids"])


@pytest.mark.parametrize("seed,b,h,w,canvas,share,variant", [(21, 3, 48, 64, 3, False, None), (22, 5, 48, 64, 3, True, None), (23, 2, 96, 128, 1, False, None),
                                                            (24, 3, 120, 160, 3, False, "seam"), (25, 2, 240, 320, 3, False, None)])
def test_emulation_against_float64_on_seeded_maps(seed, b, h, w, canvas, share, variant):
    c = gi.case(seed, b, h, w, canvas, n_gt=2 if share else None, n_im=2 if share else None, share=share, variant=variant)
    got = _emul(c)
    r = check_against_f64(c, got)
    assert np.all(got["counts"][:, 3] < got["counts"][:, 1])    # the occluder hides something
    if canvas == 3:
        assert np.all(got["counts"][:, 0] > got["counts"][:, 1]) and np.all(got["boxes"][:, 0] < 0)
    if variant == "seam":
        assert np.all(r["boxes"][:, 0] <= -3) and np.all(got["mask"][:, h // 2, 0] == 255)   # one box over the seam at image x = -1 | 0


def test_small_scalar_shapes_and_an_empty_centre_tile_against_float64():
    for args in ((31, 3, 5, 7, 3), (32, 1, 1, 1, 1), (33, 2, 4, 260, 3)):
        c = gi.case(*args)
        check_against_f64(c, _emul(c), guard=False)
    c = gi.case(34, 2, 48, 64, 3, variant="empty_centre")
    got = _emul(c)
    check_against_f64(c, got, guard=False)
    assert np.all(got["counts"][:, 0] > 0) and np.all(got["counts"][:, 1:] == 0) and np.all(got["visib_fract"] == 0)
    assert np.all(got["boxes"][:, 4:] == -1) and not got["mask"].any()


def test_the_float64_restatement_alone_keeps_the_borderline_share_small():
    """the guard's premise, measured before it is relied on: borderline pixels are a tiny share of the visible ones"""
    c = gi.case(77, 3, 240, 320, 3)
    r = gi.f64_gt_info(c["gt"], c["test"], c["K"], 3)
    share = r["borderline"] / r["counts"][:, 3]
    print("borderline share of px_count_visib per row:", share)
    assert np.all(r["counts"][:, 3] >= 1000) and np.all(share <= 0.01)


# --------------------------------------------------------------------------------------------------------------------------------
# host logic
# --------------------------------------------------------------------------------------------------------------------------------
def _table():
    from megapose6d_amd import evaluation as ev

    counts = np.array([[100, 60, 50, 40], [30, 0, 0, 0], [9, 9, 9, 0], [-1, -1, -1, -1], [1, 1, 0, 1], [50, 50, 50, 2]])
    boxes = np.array([[-20, 5, 30, 44, 3, 6, 30, 40], [-9, 2, -3, 7, -1, -1, -1, -1], [4, 4, 6, 6, -1, -1, -1, -1], [-1] * 8,
                      [-1, -1, -1, -1, -1, -1, -1, -1], [0, 0, 9, 9, 2, 3, 3, 3]])
    fract = np.array([0.4, 0.0, 0.0, np.nan, 1.0, 0.04])
    return ev, ev.gt_info_table(counts, boxes, fract, index=np.arange(6) + 10)


def test_the_box_conversions():
    ev, df = _table()
    assert list(df.columns) == ["px_count_all", "px_count_image", "px_count_valid", "px_count_visib", "visib_fract", "bbox_obj", "bbox_visib",
                                "bbox_amodal", "bbox_modal"] and list(df.index) == list(range(10, 16))
    assert df["bbox_amodal"].iloc[0] == [-20, 5, 30, 44] and df["bbox_obj"].iloc[0] == [-20, 5, 50, 39]      # w = xmax - xmin
    assert df["bbox_modal"].iloc[0] == [3, 6, 30, 40] and df["bbox_visib"].iloc[0] == [3, 6, 27, 34]
    assert df["bbox_obj"].iloc[1] == [-9, 2, 6, 5] and df["bbox_visib"].iloc[1] == [-1] * 4 and df["bbox_modal"].iloc[1] == [-1] * 4
    assert df["bbox_obj"].iloc[3] == [-1] * 4 and df["bbox_amodal"].iloc[3] == [-1] * 4 and np.isnan(df["visib_fract"].iloc[3])
    # one pixel at image pixel (-1, -1) is a box, not the blank: its count says so
    assert df["bbox_obj"].iloc[4] == [-1, -1, 0, 0] and df["bbox_amodal"].iloc[4] == [-1, -1, -1, -1] and df["px_count_all"].iloc[4] == 1
    K = torch.tensor([[[500.0, 0, 320.5], [0, 510.0, 239.25], [0, 0, 1]]])
    Kt = ev.tile_intrinsics(K, 3, (480, 640))
    assert Kt.shape == (1, 9, 3, 3) and torch.equal(Kt[0, 4], K[0])
    assert Kt[0, 0, 0, 2] == 320.5 + 640 and Kt[0, 0, 1, 2] == 239.25 + 480 and Kt[0, 5, 0, 2] == 320.5 - 640 and Kt[0, 5, 1, 2] == 239.25
    assert torch.equal(Kt[0, :, 0, 0], torch.full((9,), 500.0)) and torch.equal(ev.tile_intrinsics(K, 1, (480, 640))[:, 0], K)
    with pytest.raises(ValueError):
        ev.tile_intrinsics(K, 2, (480, 640))


def test_detections_from_gt_info_drop_invisible_rows():
    from megapose6d_amd.tcoll import PandasTensorCollection

    ev, df = _table()
    infos = pd.DataFrame(dict(label=list("abcdef"), batch_im_id=[0, 0, 1, 1, 2, 2]), index=np.arange(6) + 10)
    gt = PandasTensorCollection(infos, poses=torch.eye(4).repeat(6, 1, 1))
    det = ev.detections_from_gt_info(gt, df)
    assert list(det.infos["label"]) == ["a", "e", "f"] and list(det.infos["batch_im_id"]) == [0, 2, 2] and list(det.infos["instance_id"]) == [0, 4, 5]
    assert det.bboxes.dtype == torch.float32 and det.bboxes.tolist() == [[3, 6, 30, 40], [-1, -1, -1, -1], [2, 3, 3, 3]]
    det = ev.detections_from_gt_info(gt, df, visib_gt_min=0.1)                               # BOP's threshold
    assert list(det.infos["label"]) == ["a", "e"] and det.bboxes.shape == (2, 4)
    gt.infos["instance_id"] = [7, 7, 7, 8, 8, 9]
    assert list(ev.detections_from_gt_info(gt, df).infos["instance_id"]) == [7, 8, 9]
    none = ev.detections_from_gt_info(gt, df, visib_gt_min=2.0)
    assert len(none.infos) == 0 and none.bboxes.shape == (0, 4)
    from megapose6d_amd.types import assert_detections_valid                                   # what the pose estimator asks of detections

    assert_detections_valid(det)


def test_bop_recall_on_the_valid_rows_only():
    from megapose6d_amd import evaluation as ev

    def table(vsd, mssd, mspd, diameter):
        d = {c: np.asarray(vsd, np.float64)[:, k] for k, c in enumerate(ev._vsd_names(ev.BOP_TAUS))}
        d.update(mssd=np.asarray(mssd, np.float64), mspd=np.asarray(mspd, np.float64), diameter=np.asarray(diameter, np.float64))
        return pd.DataFrame(d)

    vsd = np.array([[0.0] * 10, [1.0] * 10, [0.22] * 10, [np.nan] * 10])
    t = table(vsd, [0.0, 1.0, 0.031, np.nan], [0.0, 500.0, 12.0, np.nan], [0.1] * 4)
    valid = np.array([True, False, True, False])
    assert ev.bop_recall(t, valid=valid) == ev.bop_recall(t[valid])
    assert ev.bop_recall(t, valid=pd.Series(valid[::-1], index=t.index[::-1])) == ev.bop_recall(t[valid])
    assert ev.bop_recall(t, valid=None) == ev.bop_recall(t) and ev.bop_recall(t, valid=np.ones(4, bool)) == ev.bop_recall(t)
    assert ev.bop_recall(t)["ar_vsd"] == pytest.approx(0.4) and ev.bop_recall(t, valid=valid)["ar_vsd"] == pytest.approx(0.8)
    for bad in (np.array([1, 0, 1, 0]), valid[:3]):
        with pytest.raises(ValueError):
            ev.bop_recall(t, valid=bad)
    with pytest.raises(ValueError):
        ev.bop_recall(t, valid=np.zeros(4, bool))
