"""GPU: the device side of BOP's detection / segmentation scores (csrc/det_ap.hip) through the C ABI and the wrappers.  The pair counts
against plain numpy `!= 0` masks, exactly, at sizes that take the 16-byte path, the byte path, unaligned mask starts and several slices
per mask; the match table against the host emulation built from the same rules header (tests/det_ap_emul.cpp), exactly, on the seeded
and hand-written cases of the contract test; `evaluation.bop_detection_scores` end to end on a rendered scene against the numpy
restatement run on the same tables copied to the host.  Bad arguments are refused before any launch.  Reads nothing outside the tree."""
import numpy as np
import pandas as pd
import pytest
import torch

from support import det_ap as da

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _masks(rng, n, h, w, values, share=0.4):
    m = rng.choice(np.asarray(values, np.uint8), size=(n, h, w))
    m[rng.uniform(size=(n, h, w)) > share] = 0
    return m


# --------------------------------------------------------------------------------------------------------------------------------
# pair counts
# --------------------------------------------------------------------------------------------------------------------------------
# 1 x 1, 7 x 13 and 33 x 65 are no multiple of 16 (byte path, masks start at unaligned offsets); 64 x 64 takes the 16-byte path
@pytest.mark.parametrize("h,w", [(1, 1), (7, 13), (33, 65), (64, 64)])
def test_pair_counts_match_numpy_at_small_and_odd_sizes(h, w):
    from megapose6d_amd import engine as eng

    rng = np.random.RandomState(h * w)
    pred, gt = _masks(rng, 5, h, w, [1, 255, 2, 128, 77], share=0.6), _masks(rng, 4, h, w, [255], share=0.5)
    pid, gid = rng.randint(0, 5, size=23).astype(np.int32), rng.randint(0, 4, size=23).astype(np.int32)
    want = da.restated_pair_counts(pred, gt, pid, gid)
    for split in (0, 1, 3, 7):                                          # integer sums: any number of slices gives the same bits
        got = eng.mask_pair_counts(_dev(pred), _dev(gt), _dev(pid), _dev(gid), split=split)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), split
    assert want[:, 0].max() > 0 or h * w == 1
    # the pred tensor on a base that is not 16-byte aligned: the byte path, the same counts
    flat = torch.zeros(pred.size + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = _dev(pred).flatten()
    assert np.array_equal(eng.mask_pair_counts(flat[1:].view(5, h, w), _dev(gt), _dev(pid), _dev(gid)).cpu().numpy(), want)
    assert np.array_equal(da.emul_pair_counts(pred[pid[0]], gt[gid[0]]), want[0])


def test_pair_counts_at_480_x_640_mixed_bytes_bool_views_shared_masks_and_no_candidates():
    from megapose6d_amd import engine as eng
    from megapose6d_amd import evaluation as ev

    rng = np.random.RandomState(1)
    h, w = 480, 640
    pred = _masks(rng, 3, h, w, [1, 255, 3, 0x80, 0x7f, 200])
    gt = _masks(rng, 3, h, w, [255, 1])
    pred[2] = 0                                                          # an all-zero mask ...
    gt[2] = 0                                                            # ... against an all-zero mask: union 0
    pid = np.int32([0, 0, 0, 1, 1, 2, 2, 0])                            # several pairs share prediction 0 and ground truth 1
    gid = np.int32([0, 1, 2, 1, 0, 2, 1, 1])
    want = da.restated_pair_counts(pred, gt, pid, gid)
    got = eng.mask_pair_counts(_dev(pred), _dev(gt), _dev(pid), _dev(gid))
    assert np.array_equal(got.cpu().numpy(), want) and want[5].tolist() == [0, 0, 0] and want[1, 0] > 10000
    assert np.array_equal(eng.mask_pair_counts(_dev(pred), _dev(gt), _dev(pid), _dev(gid), split=5).cpu().numpy(), want)
    # a bool tensor goes through a uint8 view (no copy): the counts of its 0 / 1 bytes
    pred_bool = _dev(pred != 0)
    assert pred_bool.dtype == torch.bool
    assert np.array_equal(eng.mask_pair_counts(pred_bool, _dev(gt), _dev(pid), _dev(gid)).cpu().numpy(), want)
    # mask_iou: one float64 division, 0 where the union is 0
    iou = ev.mask_iou(pred_bool, _dev(gt), (pid, gid))
    assert iou.dtype == torch.float64 and iou.is_cuda and np.array_equal(iou.cpu().numpy(), da.restated_mask_iou(want)) and iou[5] == 0
    # C = 0; an index out of range reads nothing and gives -1 (NaN IoU)
    empty = eng.mask_pair_counts(pred_bool, _dev(gt), _dev(pid[:0]), _dev(gid[:0]))
    assert tuple(empty.shape) == (0, 3)
    out = eng.mask_pair_counts(pred_bool, _dev(gt), _dev(np.int32([0, 3, -1, 1])), _dev(np.int32([1, 0, 0, 3])), split=2).cpu().numpy()
    assert np.array_equal(out[0], want[1]) and (out[1:] == -1).all()
    assert torch.isnan(ev.mask_iou(pred_bool, _dev(gt), ([3], [0]))).all()


def test_pair_counts_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    lib = _lib.load()
    m = torch.ones(2, 4, 8, dtype=torch.uint8, device="cuda")
    ids = torch.zeros(3, dtype=torch.int32, device="cuda")
    counts = torch.full((3, 3), 7, dtype=torch.int32, device="cuda")

    def call(a=m.data_ptr(), b=m.data_ptr(), p=ids.data_ptr(), g=ids.data_ptr(), P=2, G=2, C=3, H=4, W=8, split=0, out=counts.data_ptr()):
        return lib.mp_mask_pair_counts(a, b, p, g, P, G, C, H, W, split, out, None)

    for bad in (dict(a=None), dict(b=None), dict(p=None), dict(g=None), dict(out=None), dict(P=-1), dict(G=-1), dict(C=-1), dict(split=-1), dict(H=0),
                dict(W=0), dict(H=-4), dict(H=65536, W=32768), dict(P=0), dict(C=eng.MASK_PAIR_MAX_PAIRS + 1)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()
    assert (counts == 7).all()                                           # nothing was written
    assert call(C=0, a=None, b=None, p=None, g=None, out=None) == 0
    assert call(H=1, W=2 ** 31 - 1, C=0) == 0                            # the largest H * W is accepted
    assert call() == 0
    torch.cuda.synchronize()
    assert (counts == 32).all()
    for args in ((m.float(), m, ids, ids), (m, m[:, :2], ids, ids), (m, m, ids, ids[:2]), (m.cpu(), m, ids, ids)):
        with pytest.raises(eng.EngineError):
            eng.mask_pair_counts(*args)


# --------------------------------------------------------------------------------------------------------------------------------
# the match table
# --------------------------------------------------------------------------------------------------------------------------------
def _check(c, thr=da.IOU_THRS, n_top=None):
    """the kernel (through evaluation.coco_match) and the emulation on one case -> the table"""
    from megapose6d_amd import evaluation as ev

    cand = pd.DataFrame(dict(pred_id=c["pred_id"], gt_id=c["gt_id"], group_id=c["group_id"]))
    got = ev.coco_match(cand, _dev(c["iou"]), c["scores"], c["gt_ignore"], iou_thrs=thr, n_top=n_top)
    assert got.is_cuda and got.dtype == torch.int32
    ref = da.emul(c["pred_id"], c["gt_id"], c["group_id"], c["iou"], c["scores"], c["gt_ignore"], thr, n_top)
    assert np.array_equal(got.cpu().numpy(), ref)
    return ref


@pytest.mark.parametrize("n_theta", [1, 10, 16])
def test_match_table_equals_the_emulation_on_the_seeded_table(n_theta):
    c = da.seeded()
    thr = {1: np.array([0.5]), 10: da.IOU_THRS, 16: np.linspace(0.25, 1.0, 16)}[n_theta]
    full = _check(c, thr)
    cut = _check(c, thr, n_top=da.SEEDED["n_top"])
    assert 0 < (cut >= 0).sum() < (full >= 0).sum()
    # more groups than one workgroup holds, and a last workgroup that is not full
    many = da.case(5, da.ragged_sizes(6, 300) + [(3, 70)], ties=n_theta != 10)
    assert (_check(many, thr) >= 0).sum() > 100


@pytest.mark.parametrize("name", list(da.hand_cases()))
def test_match_table_equals_the_emulation_on_the_hand_written_cases(name):
    c, thr, n_top, want = da.hand_cases()[name]
    assert _check(c, thr, n_top).tolist() == want


def test_match_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng
    from megapose6d_amd import evaluation as ev

    lib = _lib.load()
    c = da.case(1, [(2, 2), (1, 3)], nan_share=0.0)
    index = ev.bop_match_index(c["pred_id"], c["gt_id"], c["group_id"], c["scores"])
    t = {k: _dev(index[k]) for k in eng.BOP_MATCH_INDEX}
    iou, thr, ign = _dev(c["iou"][index["order"]]), _dev(da.IOU_THRS), _dev(c["gt_ignore"].astype(np.uint8))
    P, C = 3, 7
    match = torch.full((P, 10), 7, dtype=torch.int32, device="cuda")
    need = int(lib.mp_det_match_workspace_bytes(index["n_taken_words"], 10))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def call(iou_p=iou.data_ptr(), gt_p=t["cand_gt"].data_ptr(), off_p=t["est_off"].data_ptr(), ign_p=ign.data_ptr(), thr_p=thr.data_ptr(),
             m_p=match.data_ptr(), ws_p=ws.data_ptr(), ws_bytes=need, P=P, C=C, n_est=3, n_groups=2, words=index["n_taken_words"], n_theta=10):
        return lib.mp_det_match(iou_p, gt_p, t["cand_lgt"].data_ptr(), t["est_row"].data_ptr(), off_p, t["group_est_off"].data_ptr(),
                                t["group_n_gt"].data_ptr(), t["group_taken_off"].data_ptr(), None, ign_p, thr_p, P, C, n_est, n_groups, words, n_theta,
                                m_p, ws_p, ws_bytes, None)

    for bad in (dict(iou_p=None), dict(gt_p=None), dict(off_p=None), dict(ign_p=None), dict(thr_p=None), dict(m_p=None), dict(ws_p=None),
                dict(ws_bytes=need - 1), dict(P=-1), dict(C=-1), dict(n_est=-1), dict(n_groups=-1), dict(words=-1), dict(n_theta=0),
                dict(n_theta=eng.DET_MATCH_MAX_THETAS + 1), dict(n_est=C + 1)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()
    assert (match == 7).all()                                            # nothing was written
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(match.cpu().numpy(), da.emul_index(c["iou"][index["order"]], index, c["gt_ignore"], da.IOU_THRS, P))
    match.fill_(7)
    assert call(C=0, n_est=0, n_groups=0, iou_p=None, gt_p=None, off_p=None, ign_p=None, thr_p=None, ws_p=None, ws_bytes=0) == 0
    torch.cuda.synchronize()
    assert (match == -1).all()
    assert call(P=0, m_p=None) == 0
    assert lib.mp_det_match_workspace_bytes(-1, 3) == 0 and lib.mp_det_match_workspace_bytes(4, 0) == 0 and lib.mp_det_match_workspace_bytes(4, 17) == 0
    # the wrapper
    cand = pd.DataFrame(dict(pred_id=c["pred_id"], gt_id=c["gt_id"], group_id=c["group_id"]))
    d_iou = _dev(c["iou"])
    empty = ev.coco_match(cand.iloc[:0], d_iou[:0], c["scores"], c["gt_ignore"])
    assert tuple(empty.shape) == (3, 10) and (empty == -1).all()
    for kw in (dict(iou=d_iou.float()), dict(iou=d_iou[:-1]), dict(iou=d_iou.cpu()), dict(scores=[0.1, np.nan, 0.2]), dict(gt_ignore=c["gt_ignore"][:2]),
               dict(gt_ignore=c["gt_ignore"].astype(np.int32)), dict(iou_thrs=np.zeros(17)), dict(iou_thrs=np.zeros(0)), dict(n_top=-1), dict(n_top=1.5)):
        args = dict(dict(cand=cand, iou=d_iou, scores=c["scores"], gt_ignore=c["gt_ignore"]), **kw)
        with pytest.raises(ValueError):
            ev.coco_match(**args)


def test_smallest_index_and_the_misfits_the_wrapper_refuses_itself():
    """2 groups, 3 candidates, 2 estimates, n_theta = 2: the table of the emulation; an est_off one element short and an n_top of
    [n_groups + 1] are refused by the wrapper with its own texts (not the library's "mp_engine error"), i.e. before any launch."""
    from megapose6d_amd import engine as eng
    from megapose6d_amd import evaluation as ev

    c = da.case(6, [(1, 2), (1, 1)], nan_share=0.0)
    thr2 = np.array([0.5, 0.75])
    assert len(c["pred_id"]) == 3 and len(c["scores"]) == 2
    ref = _check(c, thr2)
    assert ref.shape == (2, 2) and (ref >= 0).any() and (ref < 0).any()
    index = ev.bop_match_index(c["pred_id"], c["gt_id"], c["group_id"], c["scores"])
    t = dict({k: _dev(index[k]) for k in eng.BOP_MATCH_INDEX}, n_taken_words=index["n_taken_words"])
    iou, thr, ign = _dev(c["iou"][index["order"]]), _dev(thr2), _dev(c["gt_ignore"].astype(np.uint8))
    assert np.array_equal(eng.det_match(iou, t, ign, thr, 2, n_top=_dev(np.ones(2, np.int32))).cpu().numpy(),
                          da.emul_index(c["iou"][index["order"]], index, c["gt_ignore"], thr2, 2, [1, 1]))
    with pytest.raises(eng.EngineError) as short:
        eng.det_match(iou, dict(t, est_off=t["est_off"][:-1]), ign, thr, 2)
    assert str(short.value) == "the index does not fit iou [C]"
    with pytest.raises(eng.EngineError) as top:
        eng.det_match(iou, t, ign, thr, 2, n_top=_dev(np.ones(3, np.int32)))
    assert str(top.value) == "n_top must be [n_groups], got (3,)"


# --------------------------------------------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------------------------------------------
def test_bop_detection_scores_end_to_end_on_a_rendered_scene(object_dataset):
    from megapose6d_amd import Panda3dSceneRenderer
    from megapose6d_amd import evaluation as ev
    from megapose6d_amd.renderer import Panda3dBatchRenderer
    from megapose6d_amd.tcoll import PandasTensorCollection
    from megapose6d_amd.types import make_scene_lights
    from support import pose_error as pes
    from tests.support import synthetic as syn

    H, W = 96, 128
    rng = np.random.RandomState(3)
    labels = [o.label for o in object_dataset.list_objects]
    assert len(labels) == 3
    K_im = np.repeat((np.diag([0.2, 0.2, 1.0]) @ syn.K_EXAMPLE)[None], 2, axis=0).astype(np.float32)
    # image 0: the three objects side by side and a second instance of object 0 right behind the first (mostly hidden); image 1: two
    obj, im = np.array([0, 1, 2, 0, 0, 1]), np.array([0, 0, 0, 0, 1, 1])
    xyz = [(-0.1, 0.0, 0.5), (0.0, 0.01, 0.55), (0.1, -0.01, 0.5), (-0.095, 0.005, 0.75), (-0.05, 0.0, 0.5), (0.06, 0.0, 0.55)]
    T_gt = np.stack([pes.pose(pes.random_rotation(rng), list(p)) for p in xyz]).astype(np.float32)
    n_gt = len(obj)
    gt = PandasTensorCollection(pd.DataFrame(dict(label=[labels[o] for o in obj], batch_im_id=im)), poses=torch.from_numpy(T_gt).cuda())
    K = torch.from_numpy(K_im).cuda()
    scene = Panda3dSceneRenderer(object_dataset, msaa=1)
    renderer = Panda3dBatchRenderer(object_dataset, n_workers=1)
    try:
        frames = scene.render_scenes(list(gt.infos["label"]), gt.poses, K[torch.from_numpy(im).cuda()], im.tolist(), (H, W), make_scene_lights(),
                                     render_depth=True).depths[:, 0].contiguous()
        info, _, mask_visib = ev.gt_info(gt, renderer, frames, K, return_masks=True)
    finally:
        scene.close()
        renderer.stop()
    fract = info["visib_fract"].to_numpy()
    levels = np.unique(fract)
    assert len(levels) >= 2 and (info["px_count_visib"].to_numpy() > 0).sum() >= 4
    visib_gt_min = 0.5 * float(levels[0] + levels[1])                    # the least visible instance is the ignored ground truth
    # detections: every ground truth itself, a copy of each shifted by (3, 2) pixels with a lower score, a second far-shifted copy of
    # some, and one detection of a label that image 1 does not show (no ground truth, no candidate: a false positive)
    gt_boxes = np.asarray(list(info["bbox_modal"]), np.float32)
    shift = lambda m, dx, dy: torch.roll(m, shifts=(dy, dx), dims=(1, 2))  # noqa: E731
    masks = torch.cat([mask_visib > 0, shift(mask_visib, 3, 2) > 0, shift(mask_visib[:3], 40, 0) > 0, mask_visib[2:3] > 0])
    boxes = np.concatenate([gt_boxes, gt_boxes + np.float32([3, 2, 3, 2]), gt_boxes[:3] + np.float32([40, 0, 40, 0]), gt_boxes[2:3]])
    p_obj, p_im = np.concatenate([obj, obj, obj[:3], [2]]), np.concatenate([im, im, im[:3], [1]])
    scores = np.concatenate([[0.9, 0.5, 0.8, 0.7, 0.6, 0.95], [0.95, 0.4, 0.3, 0.2, 0.9, 0.1], [0.97, 0.45, 0.1], [0.99]])
    infos = pd.DataFrame(dict(label=[labels[o] for o in p_obj], batch_im_id=p_im, score=scores), index=np.arange(len(scores)) + 20)
    pred = PandasTensorCollection(infos, bboxes=torch.from_numpy(boxes).cuda(), masks=masks)
    assert masks.dtype == torch.bool and mask_visib.dtype == torch.uint8 and int(mask_visib.max()) == 255

    cand = ev.bop_candidates(pred.infos, gt.infos)
    pid, gid, grp = (cand[k].to_numpy() for k in ("pred_id", "gt_id", "group_id"))
    assert len(cand) == 5 * 2 + 3 + 3 + 2 + 2 and 15 not in pid                  # group (image 0, object 0): 5 detections x 2 ground truths
    ign = (fract < visib_gt_min) | (info["px_count_visib"].to_numpy() == 0)
    assert 1 <= ign.sum() < n_gt
    masks_h, gt_masks_h = masks.cpu().numpy(), mask_visib.cpu().numpy()
    ious = dict(segm=da.restated_mask_iou(da.restated_pair_counts(masks_h, gt_masks_h, pid, gid)), bbox=da.restated_box_iou(boxes, gt_boxes, pid, gid))
    pred_group = list(zip(p_im.tolist(), p_obj.tolist()))
    results = {}
    for iou_type in ("bbox", "segm"):
        for n_top in (100, 2):
            got = ev.bop_detection_scores(pred, gt, info, iou_type=iou_type, gt_masks=mask_visib, visib_gt_min=visib_gt_min, n_top=n_top)
            match = da.restated_match(pid, gid, grp, ious[iou_type], scores, ign, da.IOU_THRS, n_top)
            kept = da.restated_kept(pred_group, scores, n_top)
            want = da.restated_accumulate(match, scores, infos["label"].to_numpy(), gt.infos["label"].to_numpy(), ign, kept)
            print(f"bop_detection_scores {iou_type}, n_top {n_top}: {got}")
            assert got == want, (iou_type, n_top)
            assert 0 < got["AP"] < 1                                     # exact copies are found; the detection without ground truth ranks first
            results[iou_type, n_top] = got
    assert results["segm", 100] != results["segm", 2]                     # the cut drops detections of the crowded group
    # the device IoUs themselves, against the restatement: masks exactly, boxes exactly
    assert np.array_equal(ev.mask_iou(masks, mask_visib, cand).cpu().numpy(), ious["segm"])
    assert np.array_equal(ev.box_iou(pred.bboxes, torch.from_numpy(gt_boxes), cand).cpu().numpy(), ious["bbox"])
    with pytest.raises(ValueError):
        ev.bop_detection_scores(pred, gt, info, iou_type="keypoints")
    with pytest.raises(ValueError):
        ev.bop_detection_scores(pred, gt, info, iou_type="segm")
    with pytest.raises(ValueError):
        ev.bop_detection_scores(pred, gt, info.iloc[:-1])
