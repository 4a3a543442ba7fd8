"""GPU: the BOP matching kernel (csrc/bop_match.hip) through the C ABI against the host emulation built from the same rules header
(tests/bop_match_emul.cpp): every entry of the match table, exactly, on both paths of the kernel and just past each limit of the fast
one; invariance under the order of the rows; `evaluation.bop_scores` end to end on the synthetic objects against `bop_recall` of
`bop_errors` and against the emulation fed `bop_candidate_errors`' own output.  Bad arguments are refused before any launch.  Reads
nothing outside the tree."""
import numpy as np
import pandas as pd
import pytest
import torch

from support import bop_match as bm
from support import pose_error as pes

pytestmark = pytest.mark.gpu

from megapose6d_amd.engine import BOP_MATCH_MASK_BITS, BOP_MATCH_MAX_ERRORS, BOP_MATCH_MAX_THETAS, BOP_MATCH_STAGE_FLOATS  # noqa: E402


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _gpu(c, n_top=None):
    """the kernel and the emulation on one index -> (match of the kernel, match of the emulation)"""
    from megapose6d_amd import engine as eng
    from megapose6d_amd import evaluation as ev

    index = ev.bop_match_index(c["pred_id"], c["gt_id"], c["group_id"], c["scores"], c["thr"].shape[0])
    errs = np.ascontiguousarray(c["errs"][index["order"]], np.float32)
    on_dev = {k: _dev(index[k]) for k in eng.BOP_MATCH_INDEX}
    on_dev["n_taken_words"] = index["n_taken_words"]
    got = eng.bop_match(_dev(errs), on_dev, _dev(c["thr"]), len(c["scores"]), n_top=_dev(None if n_top is None else np.asarray(n_top, np.int32)))
    torch.cuda.synchronize()
    return got.cpu().numpy(), bm.emul_index(errs, index, c["thr"], len(c["scores"]), n_top)


def _check(c, n_top=None):
    got, ref = _gpu(c, n_top)
    assert got.dtype == np.int32 and got.shape == ref.shape and np.array_equal(got, ref)
    return ref


def test_limits_of_the_library_are_the_named_constants():
    from megapose6d_amd import engine as eng

    assert eng.bop_match_limits() == bm.limits() == dict(max_errors=BOP_MATCH_MAX_ERRORS, max_thetas=BOP_MATCH_MAX_THETAS,
                                                         mask_bits=BOP_MATCH_MASK_BITS, stage_floats=BOP_MATCH_STAGE_FLOATS)


# (E, n_theta): the smallest, BOP's, the largest the entry point accepts
@pytest.mark.parametrize("E,n_theta", [(1, 1), (12, 10), (BOP_MATCH_MAX_ERRORS, BOP_MATCH_MAX_THETAS), (5, 13)])
@pytest.mark.parametrize("ties", [False, True])
def test_kernel_matches_the_emulation_on_ragged_groups(E, n_theta, ties):
    ref = _check(bm.case(1, [(1, 1)], E, n_theta, ties=ties, nan_share=0.0))                 # one group of 1 x 1
    assert ref.shape == (1, E, n_theta)
    n_groups = 300
    c = bm.case(20 + E, bm.ragged_sizes(E + n_theta, n_groups), E, n_theta, ties=ties)       # 0-6 estimates x 0-5 ground truths
    full = _check(c)
    cut = _check(c, np.random.RandomState(E).randint(0, 4, size=n_groups))
    assert 0.1 < (full >= 0).mean() < 0.9 and (cut >= 0).sum() < (full >= 0).sum()
    print(f"bop_match ({E} x {n_theta}, ties {ties}): {len(c['pred_id'])} candidates, {int((full >= 0).sum())} matches, {int((cut >= 0).sum())} after the cut")


def _limit_cases():
    m, s = BOP_MATCH_MASK_BITS, BOP_MATCH_STAGE_FLOATS
    cases = [("mask+1", 2, 3, [(3, m + 1)]), ("mask", 2, 3, [(3, m)]), ("mask+1 among small", 12, 10, [(2, 3), (3, m + 1), (4, 2), (1, 2 * m + 5)])]
    for E in (1, 12, BOP_MATCH_MAX_ERRORS):
        at = s // E                                                      # candidates that still fit the staging
        n_gt = max(d for d in range(1, m + 1) if at % d == 0)            # at = n_est * n_gt with n_gt <= 64: the fast path, full
        cases.append((f"stage E={E}", E, 2, [(at // n_gt, n_gt), (2, 2)]))
        past = at + 1
        n_gt = max(d for d in range(1, m + 1) if past % d == 0)
        cases.append((f"stage+1 E={E}", E, 2, [(2, 2), (past // n_gt, n_gt)]))
    return cases


@pytest.mark.parametrize("name,E,n_theta,sizes", _limit_cases(), ids=[c[0] for c in _limit_cases()])
def test_kernel_matches_the_emulation_at_and_past_each_limit_of_the_fast_path(name, E, n_theta, sizes):
    c = bm.case(len(name), sizes, E, n_theta, nan_share=0.01)
    n_cand = [ne * ng for ne, ng in sizes]
    fast = [ng <= BOP_MATCH_MASK_BITS and nc * E <= BOP_MATCH_STAGE_FLOATS for (ne, ng), nc in zip(sizes, n_cand)]
    assert fast.count(False) == (0 if name in ("mask",) or (name.startswith("stage E")) else (2 if "among" in name else 1)), (name, fast)
    full = _check(c)
    assert (full >= 0).sum() > 0
    # a cut that brings the walked candidates of the large group back under the staging limit: the other path, the same rules
    _check(c, [1] * len(sizes))
    _check(c, [2] * len(sizes))
    # the same group handled by either path gives the same matches: thresholds and errors of the large group alone, as a small E = 1 problem
    if E > 1:
        one = dict(c, errs=c["errs"][:, :1].copy(), thr=c["thr"][:, :1].copy())
        assert np.array_equal(_check(one)[:, 0], full[:, 0])


def test_invariance_under_the_order_of_the_rows():
    c = bm.case(9, bm.ragged_sizes(4, 200) + [(3, BOP_MATCH_MASK_BITS + 6)], 4, 5, permute=False)
    assert len(set(c["scores"].tolist())) == len(c["scores"])
    base = _check(c)
    rng = np.random.RandomState(2)
    new_pred, new_gt = rng.permutation(c["n_pred"]), rng.permutation(c["n_gt"])          # old row -> new row
    scores = np.empty_like(c["scores"])
    scores[new_pred] = c["scores"]
    shuffle = rng.permutation(len(c["pred_id"]))
    moved = dict(c, pred_id=new_pred[c["pred_id"]][shuffle], gt_id=new_gt[c["gt_id"]][shuffle], group_id=c["group_id"][shuffle],
                 errs=c["errs"][shuffle], scores=scores)
    got = _check(moved)
    back = np.full_like(base, -1)
    old_gt = np.argsort(new_gt)
    back[:] = np.where(got[new_pred] >= 0, old_gt[np.clip(got[new_pred], 0, None)], -1)
    # with distinct scores the walk is the same; an error tie may pick another ground truth only if gt rows order differently, and the
    # seeded errors are continuous: no ties
    assert np.array_equal(back, base)
    for e in range(base.shape[1]):
        for k in range(base.shape[2]):
            assert {(p, int(old_gt[g])) for p, g in bm.pairs(got[new_pred][:, e, k])} == bm.pairs(base[:, e, k])


def test_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng
    from megapose6d_amd import evaluation as ev

    lib = _lib.load()
    c = bm.case(1, [(2, 2), (1, 3)], 2, 3)
    index = ev.bop_match_index(c["pred_id"], c["gt_id"], c["group_id"], c["scores"], 2)
    t = {k: _dev(index[k]) for k in eng.BOP_MATCH_INDEX}
    errs, thr = _dev(np.ascontiguousarray(c["errs"][index["order"]])), _dev(c["thr"])
    P, C = 3, 7
    match = torch.full((P, 2, 3), 7, dtype=torch.int32, device="cuda")
    need = int(lib.mp_bop_match_workspace_bytes(index["n_taken_words"], 2, 3))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def call(errs_p=errs.data_ptr(), gt_p=t["cand_gt"].data_ptr(), off_p=t["est_off"].data_ptr(), thr_p=thr.data_ptr(), m_p=match.data_ptr(),
             ws_p=ws.data_ptr(), ws_bytes=need, P=P, C=C, n_est=3, n_groups=2, words=index["n_taken_words"], E=2, n_theta=3):
        return lib.mp_bop_match(errs_p, gt_p, t["cand_lgt"].data_ptr(), t["est_row"].data_ptr(), off_p, t["group_est_off"].data_ptr(),
                                t["group_n_gt"].data_ptr(), t["group_taken_off"].data_ptr(), None, thr_p, P, C, n_est, n_groups, words, E, n_theta, m_p,
                                ws_p, ws_bytes, None)

    for bad in (dict(errs_p=None), dict(gt_p=None), dict(off_p=None), dict(thr_p=None), dict(m_p=None), dict(ws_p=None), dict(ws_bytes=need - 1),
                dict(P=-1), dict(C=-1), dict(n_est=-1), dict(n_groups=-1), dict(words=-1), dict(E=0), dict(E=BOP_MATCH_MAX_ERRORS + 1), dict(n_theta=0),
                dict(n_theta=BOP_MATCH_MAX_THETAS + 1), dict(n_est=C + 1)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()
    assert (match == 7).all()                                                # nothing was written
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(match.cpu().numpy(), bm.emul_index(c["errs"][index["order"]], index, c["thr"], P))
    # no candidate: -1 everywhere, whatever the other pointers; no estimate: nothing
    match.fill_(7)
    assert call(C=0, n_est=0, n_groups=0, errs_p=None, gt_p=None, off_p=None, thr_p=None, ws_p=None, ws_bytes=0) == 0
    torch.cuda.synchronize()
    assert (match == -1).all()
    assert call(P=0, m_p=None) == 0
    assert lib.mp_bop_match_workspace_bytes(-1, 2, 3) == 0 and lib.mp_bop_match_workspace_bytes(4, 0, 3) == 0 and lib.mp_bop_match_workspace_bytes(4, 2, 17) == 0
    # the wrappers
    cand = pd.DataFrame(dict(pred_id=c["pred_id"], gt_id=c["gt_id"], group_id=c["group_id"]))
    d_errs = _dev(c["errs"])
    ok = ev.bop_match(cand, d_errs, c["scores"], c["thr"])
    assert np.array_equal(ok.cpu().numpy(), bm.emul(c["pred_id"], c["gt_id"], c["group_id"], c["errs"], c["scores"], c["thr"]))
    empty = ev.bop_match(cand.iloc[:0], d_errs[:0], c["scores"], c["thr"][:0])
    assert tuple(empty.shape) == (3, 2, 3) and (empty == -1).all()
    for kw in (dict(scores=[0.1, np.nan, 0.2]), dict(scores=[0.1, np.inf, 0.2]), dict(thresholds=c["thr"].astype(np.float32)), dict(thresholds=c["thr"][:, :1]),
               dict(thresholds=c["thr"][:1]), dict(errs=d_errs[:-1]), dict(errs=d_errs.cpu()), dict(n_top=-1), dict(n_top=[1, 2, 3]), dict(n_top=1.5)):
        args = dict(dict(cand=cand, errs=d_errs, scores=c["scores"], thresholds=c["thr"]), **kw)
        with pytest.raises(ValueError):
            ev.bop_match(**args)
    with pytest.raises(eng.EngineError):
        eng.bop_match(errs, dict(t, n_taken_words=index["n_taken_words"]), _dev(np.zeros((2, 2, 17))), P)
    with pytest.raises(eng.EngineError):
        eng.bop_match(errs, dict(t, n_taken_words=index["n_taken_words"], est_off=t["est_off"][:-1]), thr, P)


def test_smallest_index_and_the_misfits_the_wrapper_refuses_itself():
    """2 groups, 3 candidates, 2 estimates, E = 1, n_theta = 2: the table of the emulation; an est_off one element short and an n_top of
    [n_groups + 1] are refused by the wrapper with its own texts (not the library's "mp_engine error"), i.e. before any launch."""
    from megapose6d_amd import engine as eng
    from megapose6d_amd import evaluation as ev

    c = bm.case(4, [(1, 2), (1, 1)], 1, 2, nan_share=0.0)
    assert len(c["pred_id"]) == 3 and len(c["scores"]) == 2 and c["thr"].shape == (2, 1, 2)
    ref = _check(c)
    assert ref.shape == (2, 1, 2) and (ref >= 0).any() and (ref < 0).any()
    index = ev.bop_match_index(c["pred_id"], c["gt_id"], c["group_id"], c["scores"], 2)
    t = dict({k: _dev(index[k]) for k in eng.BOP_MATCH_INDEX}, n_taken_words=index["n_taken_words"])
    errs, thr = _dev(np.ascontiguousarray(c["errs"][index["order"]], np.float32)), _dev(c["thr"])
    assert np.array_equal(eng.bop_match(errs, t, thr, 2, n_top=_dev(np.ones(2, np.int32))).cpu().numpy(),
                          bm.emul_index(c["errs"][index["order"]], index, c["thr"], 2, [1, 1]))
    with pytest.raises(eng.EngineError) as short:
        eng.bop_match(errs, dict(t, est_off=t["est_off"][:-1]), thr, 2)
    assert str(short.value) == "the index does not fit errs [C,E] and thr [n_groups,E,n_theta]"
    with pytest.raises(eng.EngineError) as top:
        eng.bop_match(errs, t, thr, 2, n_top=_dev(np.ones(3, np.int32)))
    assert str(top.value) == "n_top must be [n_groups], got (3,)"


# --------------------------------------------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------------------------------------------
def test_bop_scores_end_to_end_on_the_synthetic_objects(object_dataset, engine_meshes):
    from megapose6d_amd import evaluation as ev
    from megapose6d_amd.mesh_db import MeshDataBase
    from megapose6d_amd.renderer import Panda3dBatchRenderer
    from megapose6d_amd.tcoll import PandasTensorCollection
    from tests.support import synthetic as syn

    H, W, n_im = 60, 80, 4
    rng = np.random.RandomState(8)
    labels = [o.label for o in object_dataset.list_objects]
    assert len(labels) == 3
    K_im = np.repeat((np.diag([0.125, 0.125, 1.0]) @ syn.K_EXAMPLE)[None], n_im, axis=0).astype(np.float32)
    K_im[1:, 0, 2] += np.float32([1.5, -2.0, 0.5])
    # a one-to-one table: every (image, label) has one ground truth and one estimate, row-aligned
    n = 3 * n_im
    obj, im = np.arange(n) % 3, np.arange(n) // 3
    T_gt = np.stack([pes.pose(pes.random_rotation(rng), [(-0.1, 0.0, 0.1)[o], rng.uniform(-0.03, 0.03), rng.uniform(0.45, 0.6)]) for o in obj]).astype(np.float32)
    T_est = np.stack([pes.perturbed(rng, T_gt[i][None], (1.0, 4.0, 10.0, 25.0)[i % 4], (0.002, 0.006, 0.015, 0.04)[i % 4])[0] for i in range(n)])
    T_est[4] = T_gt[4]
    T_est[7, 0, 3] = np.nan
    valid = np.ones(n, np.bool_)
    valid[2] = False
    gt_infos = pd.DataFrame(dict(label=[labels[o] for o in obj], batch_im_id=im))
    infos = pd.DataFrame(dict(label=[labels[o] for o in obj], batch_im_id=im, score=rng.permutation(n) / n + 1.0), index=np.arange(n) + 50)
    gt = PandasTensorCollection(gt_infos, poses=torch.from_numpy(T_gt).cuda())
    pred = PandasTensorCollection(infos, poses=torch.from_numpy(T_est).cuda())
    meshes = MeshDataBase.from_object_ds(object_dataset).batched(n_sym=4).cuda()
    renderer = Panda3dBatchRenderer(object_dataset, n_workers=1)
    K = torch.from_numpy(K_im).cuda()
    d_gt = renderer.render_depth(list(gt_infos["label"]), gt.poses, K[torch.from_numpy(im).cuda()], (H, W))
    assert all(int((d > 0).sum()) > 60 for d in d_gt)
    frames = torch.full((n_im, H, W), 1.5, device="cuda")
    for i in range(n):
        f = frames[im[i]]
        take = (d_gt[i] > 0) & (d_gt[i] < f)
        f[take] = d_gt[i][take]
    frames = frames + torch.from_numpy((rng.randn(n_im, H, W) * 0.002).astype(np.float32)).cuda()

    df = ev.bop_errors(pred, gt, meshes, renderer, frames, K)
    want = ev.bop_recall(df, image_width=W, valid=valid)
    got = ev.bop_scores(pred, gt, meshes, renderer, frames, K, valid=valid, image_width=W)
    assert got == dict(want, n_targets=n - 1) and 0.1 < got["ar"] < 0.9 and 0 < got["ar_vsd"] < 1
    assert ev.bop_scores(pred, gt, meshes, renderer, frames, K, valid=valid, image_width=W, n_top=None) == got
    assert ev.bop_scores(pred, gt, meshes, renderer, frames, K, valid=pd.Series(valid, index=gt_infos.index), image_width=W, n_top=1) == got

    # the candidates' errors are the rows of bop_errors, bit for bit; every distinct estimate and ground truth is rendered once
    cand = ev.bop_candidates(pred.infos, gt.infos, valid=valid)
    assert cand["pred_id"].tolist() == cand["gt_id"].tolist() == [i for i in range(n) if valid[i]]
    rendered, real = [], renderer.render_depth
    renderer.render_depth = lambda lab, *a, **k: (rendered.append(len(lab)), real(lab, *a, **k))[1]
    errs = ev.bop_candidate_errors(pred, gt, cand, meshes, renderer, frames, K)
    renderer.render_depth = real
    assert sum(rendered) == 2 * (n - 1) and errs.is_cuda and errs.dtype == torch.float32 and tuple(errs.shape) == (n - 1, 12)
    names = [f"vsd_{t:.2f}" for t in ev.BOP_TAUS] + ["mssd", "mspd"]
    assert np.array_equal(errs.cpu().numpy().view(np.uint32), df[names].to_numpy()[valid].astype(np.float32).view(np.uint32))
    assert torch.isnan(errs[cand["pred_id"].tolist().index(7)]).all()

    # duplicates: a second, lower-scored estimate for every (image, label) -- better than the first for every fourth row
    T_dup = np.stack([pes.perturbed(rng, T_gt[i][None], 2.0, 0.003)[0] if i % 4 == 3 else pes.perturbed(rng, T_est[i if i != 7 else 0][None], 3.0, 0.01)[0]
                      for i in range(n)])
    infos2 = pd.concat([infos, infos.assign(score=infos["score"] - 1.0)], ignore_index=True)
    pred2 = PandasTensorCollection(infos2, poses=torch.from_numpy(np.concatenate([T_est, T_dup])).cuda())
    assert ev.bop_scores(pred2, gt, meshes, renderer, frames, K, valid=valid, image_width=W, n_top="targets") == got
    more, pairs = ev.bop_scores(pred2, gt, meshes, renderer, frames, K, valid=valid, image_width=W, n_top=None, return_matches=True,
                                matches_at=("mssd", 3))
    assert more["ar"] > got["ar"] and all(more[k] >= got[k] for k in ("ar_vsd", "ar_mssd", "ar_mspd"))
    # ... against the emulation fed bop_candidate_errors' own output
    cand2 = ev.bop_candidates(pred2.infos, gt.infos, valid=valid)
    errs2 = ev.bop_candidate_errors(pred2, gt, cand2, meshes, renderer, frames, K)
    grp = cand2["group_id"].to_numpy()
    assert len(cand2) == 2 * (n - 1) and grp.max() == n - 2
    group_label = [infos2["label"].iloc[cand2["pred_id"].to_numpy()[np.flatnonzero(grp == g)[0]]] for g in range(n - 1)]
    diam = dict(zip(pred.infos["label"], df["diameter"]))
    thr = ev.bop_thresholds([diam[l] for l in group_label], 10, image_width=W)
    scores2 = infos2["score"].to_numpy()
    for n_top, expect in ((None, more), (np.ones(n - 1, np.int32), got)):
        ref = bm.emul(cand2["pred_id"].to_numpy(), cand2["gt_id"].to_numpy(), grp, errs2.cpu().numpy(), scores2, thr, n_top)
        dev = ev.bop_match(cand2, errs2, scores2, thr, n_top=n_top).cpu().numpy()
        assert np.array_equal(dev, ref)
        assert dict(ev.bop_match_recall(ref, n - 1), n_targets=n - 1) == expect
        if n_top is None:
            # the duplicates can only fill targets the first estimate missed: the first estimates keep their matches
            first = bm.emul(cand2["pred_id"].to_numpy(), cand2["gt_id"].to_numpy(), grp, errs2.cpu().numpy(), scores2, thr, np.ones(n - 1, np.int32))
            assert np.array_equal(ref[:n], first[:n]) and (first[n:] == -1).all()
            assert ((ref[n:] >= 0) <= (ref[:n] == -1)).all() and (ref[n:] >= 0).any()
            col = ref[:, 10, 3]
            assert pairs.to_dict("list") == dict(pred_id=np.flatnonzero(col >= 0).tolist(), gt_id=col[col >= 0].tolist())
    with pytest.raises(ValueError):
        ev.bop_scores(pred, gt, meshes, renderer, frames, K, valid=np.zeros(n, np.bool_))
    with pytest.raises(ValueError):
        ev.bop_scores(pred, gt, meshes, renderer, frames, K, n_top="all")
    with pytest.raises(ValueError):
        ev.bop_scores(pred, gt, meshes, renderer, frames, K, valid=valid.astype(np.int32))
    with pytest.raises(ValueError):
        ev.bop_scores(pred.__class__(infos.assign(score=np.nan), poses=pred.poses), gt, meshes, renderer, frames, K)
