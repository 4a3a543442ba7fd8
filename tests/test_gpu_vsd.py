"""GPU: the VSD kernels (csrc/vsd.hip) and the projected symmetry-set kernel (MSPD, csrc/pose_error.hip) through the C ABI against the
host emulation built from the same arithmetic headers (tests/vsd_emul.cpp): VSD counts integer-equal and errors bit for bit, for every
forced split; MSPD errs / err / idx / T_gt_sym bit for bit (a maximum has no order).  Then `evaluation.bop_errors` end to end on the
synthetic objects, the emulation fed the ORACLE rasteriser's depths.  Bad arguments are refused before any launch.  Reads nothing
outside the tree."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

from support import pose_error as pes
from support import vsd as vs

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _gpu_vsd(c, taus, split=0, delta=0.015, normalized=True):
    from megapose6d_amd import engine as eng

    out = eng.vsd(_dev(c["est"]), _dev(c["gt"]), _dev(c["test"]), _dev(c["K"]), _dev(c["diam"]), delta=delta, taus=taus,
                  normalized_by_diameter=normalized, est_ids=_dev(c.get("est_ids")), gt_ids=_dev(c.get("gt_ids")), im_ids=_dev(c.get("im_ids")),
                  split=split)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _emul(c, taus, delta=0.015, normalized=True):
    return vs.vsd(c["est"], c["gt"], c["test"], c["K"], c["diam"], delta=delta, taus=taus, normalized=normalized, est_ids=c.get("est_ids"),
                  gt_ids=c.get("gt_ids"), im_ids=c.get("im_ids"))


def _check(c, taus, splits=(0, 1, 3, 1000), **kw):
    ref = _emul(c, taus, **kw)
    for split in splits:
        got = _gpu_vsd(c, taus, split=split, **kw)
        assert np.array_equal(got["counts"], ref["counts"]), (split, np.abs(got["counts"] - ref["counts"]).max())
        assert np.array_equal(_bits(got["errs"]), _bits(ref["errs"])), split
    return ref


# (b, h, w, n_tau, shared ids, distinct estimate maps)
CASES = [(1, 1, 1, 10, False, None), (7, 37, 53, 16, False, None), (7, 37, 53, 1, True, None), (1, 37, 53, 10, False, None),
         (7, 480, 640, 10, False, None), (1, 480, 640, 16, False, None), (576, 480, 640, 10, True, 48), (1, 1024, 1024, 10, False, None),
         (3, 1024, 1024, 1, True, None), (7, 50, 1022, 10, False, None)]


@pytest.mark.parametrize("b,h,w,n_tau,share,n_est", CASES)
def test_vsd_kernel_matches_the_emulation_bit_for_bit(b, h, w, n_tau, share, n_est):
    c = vs.scene(1000 + b + h + n_tau, b, h, w, n_im=(2 if share else None), n_gt=(min(b, 4) if share else None), share=share, n_est=n_est)
    ref = _check(c, vs.taus_of(n_tau))
    if h * w > 1:
        assert ref["counts"][:, 1].min() > 0 and np.any(ref["errs"] > 0) and np.any(ref["errs"] < 1)
    print(f"vsd ({b},{h}x{w},{n_tau}): n_inter {ref['counts'][:, 1].min()} .. {ref['counts'][:, 1].max()}")


def test_vsd_on_maps_whose_base_is_not_16_byte_aligned():
    """w % 4 == 0 but the maps start 4 bytes off a 16-byte boundary: the scalar path, the same counts"""
    from megapose6d_amd import engine as eng

    c = vs.scene(5, 3, 40, 64)
    ref = _emul(c, vs.DEFAULT_TAUS)
    pad = lambda a: torch.cat([torch.zeros(1), torch.from_numpy(a).flatten()]).cuda()[1:].view(a.shape)   # noqa: E731
    est, gt, test = pad(c["est"]), pad(c["gt"]), pad(c["test"])
    assert est.data_ptr() % 16 == 4 and est.is_contiguous()
    out = eng.vsd(est, gt, test, _dev(c["K"]), _dev(c["diam"]))
    assert np.array_equal(out["counts"].cpu().numpy(), ref["counts"]) and np.array_equal(_bits(out["errs"].cpu().numpy()), _bits(ref["errs"]))


def test_vsd_exact_hits_invalid_rows_and_invalid_observed_depths():
    K1 = vs.intrinsics(50.0, 0.5, 0.5)[None]                # the ray is the optical axis: r = 1 exactly
    one = lambda z: np.full((1, 1, 1), z, np.float32)        # noqa: E731
    d = np.array([0.5], np.float32)
    below, above = np.float32(0.75) - np.float32(2.0 ** -24), np.float32(0.75) + np.float32(2.0 ** -24)
    for est, test, delta, want in ((1.0, 0.75, 0.25, [1, 1, 0]), (1.0, below, 0.25, [0, 0, 0]), (0.75, 0.0, 0.015, [1, 1, 1]), (above, 0.0, 0.015, [1, 1, 0])):
        c = dict(est=one(est), gt=one(1.0), test=one(test), K=K1, diam=d)
        ref = _check(c, [0.5], delta=delta)
        assert list(ref["counts"][0]) == want
    # rows with a non-finite K or a diameter that is not positive and finite; NaN, negative and infinite observed depths
    c = vs.scene(6, 6, 37, 53)
    c["K"][1, 0, 0] = np.nan
    c["K"][2, 2, 1] = np.inf
    c["diam"][3:] = [0.0, -0.1, np.inf]
    c["test"][0, 5:9, :] = [[np.nan], [-1.0], [np.inf], [-np.inf]]
    ref = _check(c, vs.DEFAULT_TAUS)
    assert np.all(ref["counts"][1:] == -1) and np.all(np.isnan(ref["errs"][1:])) and ref["counts"][0, 1] > 0
    c2 = dict(c, test=c["test"].copy())
    c2["test"][0, 5:9, :] = 0.0
    assert np.array_equal(_gpu_vsd(c2, vs.DEFAULT_TAUS)["counts"][0], ref["counts"][0])
    # not normalised by the diameter
    c = vs.scene(7, 2, 37, 53)
    _check(c, [0.01, 0.03, 0.08], normalized=False, splits=(0,))


def test_vsd_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    z = lambda *s: torch.zeros(*s, device="cuda")             # noqa: E731
    K, d = torch.eye(3, device="cuda").repeat(2, 1, 1), torch.ones(2, device="cuda")
    with pytest.raises(eng.EngineError):
        eng.vsd(z(2, 4, 1025), z(2, 4, 1025), z(2, 4, 1025), K, d)
    with pytest.raises(eng.EngineError):
        eng.vsd(z(2, 1025, 4), z(2, 1025, 4), z(2, 1025, 4), K, d)
    with pytest.raises(eng.EngineError):
        eng.vsd(z(2, 4, 4), z(2, 4, 4), z(2, 4, 4), K, d, taus=[0.1] * 17)
    with pytest.raises(eng.EngineError):
        eng.vsd(z(2, 4, 4), z(2, 4, 4), z(2, 4, 4), K, d, taus=[])
    with pytest.raises(eng.EngineError):
        eng.vsd(z(2, 4, 4), z(1, 4, 4), z(2, 4, 4), K, d)                   # one ground-truth map, two rows, no ids
    with pytest.raises(eng.EngineError):
        eng.vsd(z(2, 4, 4), z(2, 4, 5), z(2, 4, 4), K, d)
    with pytest.raises(eng.EngineError):
        eng.vsd(z(2, 4, 4), z(2, 4, 4), z(2, 4, 4), K[:1], d)
    with pytest.raises(eng.EngineError):
        eng.vsd(z(2, 4, 4), z(2, 4, 4), z(2, 4, 4), K, d, split=-1)
    # the C ABI itself
    lib = _lib.load()
    maps, errs, ws = z(2, 4, 4), z(2, 10), torch.zeros(4096, dtype=torch.uint8, device="cuda")
    taus = (C.c_float * 10)(*vs.DEFAULT_TAUS)
    tp = C.cast(taus, C.c_void_p)

    def call(est=maps.data_ptr(), b=2, h=4, w=4, n_tau=10, taus_p=tp, ws_bytes=4096, errs_p=errs.data_ptr(), kp=K.data_ptr()):
        return lib.mp_vsd(est, None, maps.data_ptr(), None, maps.data_ptr(), None, 2, 2, 2, kp, d.data_ptr(), b, h, w, 0.015, taus_p, n_tau, 1, 0,
                          errs_p, None, ws.data_ptr(), ws_bytes, None)

    assert call() == 0
    assert call(b=0) == 0 and call(b=0, est=None, errs_p=None) == 0            # b == 0: a successful no-op
    for bad in (dict(b=-1), dict(h=0), dict(w=0), dict(h=1025), dict(w=1025), dict(n_tau=0), dict(n_tau=17), dict(taus_p=None), dict(est=None),
                dict(errs_p=None), dict(kp=None), dict(ws_bytes=0), dict(ws_bytes=int(lib.mp_vsd_workspace_bytes(2, 10)) - 1), dict(b=3)):
        assert call(**bad) != 0, bad
    assert lib.mp_vsd_workspace_bytes(2, 0) == 0 and lib.mp_vsd_workspace_bytes(-1, 10) == 0 and lib.mp_vsd_workspace_bytes(2, 17) == 0
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------------------------
# MSPD
# --------------------------------------------------------------------------------------------------------------------------------
MSPD_SHAPES = [(1, 1, 1, 1, False), (3, 7, 1, 1, False), (5, 63, 2, 1, False), (2, 10007, 64, 3, True), (576, 2000, 8, 1, False), (2, 300, 512, 1, False)]


@pytest.mark.parametrize("b,N,S,n_mesh,ragged", MSPD_SHAPES)
def test_mspd_kernel_matches_the_emulation_bit_for_bit(b, N, S, n_mesh, ragged):
    from megapose6d_amd import engine as eng

    c = vs.mspd_case(b, N, S, seed=400 + N, n_mesh=n_mesh, ragged=ragged)
    ref = vs.mspd(c["T_pred"], c["T_gt"], c["syms"], c["n_sym"], c["pts"], c["K"], c["ids"], c["n_points"])

    def run(split, **kw):
        out = eng.pose_error_mspd(_dev(c["T_pred"]), _dev(c["T_gt"]), _dev(c["syms"]), _dev(c["n_sym"]), _dev(c["pts"]), _dev(c["K"]), _dev(c["ids"]),
                                  _dev(c["n_points"]), split=split, with_alt=True, **kw)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    for split in (0, 1, 7):
        got = run(split)
        for k in ("errs", "err", "idx", "T_gt_sym"):
            assert np.array_equal(_bits(got[k]), _bits(ref[k])), (k, split)
    # the mean form (order of the sum is the kernel's own): against the emulation's double sum, and its minimum in err_alt
    mean = vs.mspd(c["T_pred"], c["T_gt"], c["syms"], c["n_sym"], c["pts"], c["K"], c["ids"], c["n_points"], reduce_max=False)
    tol = 64 * vs.ULP * np.maximum(1.0, mean["err"])
    assert np.all(np.abs(got["err_alt"] - mean["err"]) <= tol)
    gm = run(0, reduce=eng.POSE_ERROR_MEAN)
    assert np.all(np.abs(gm["err"] - mean["err"]) <= tol) and np.array_equal(_bits(gm["err_alt"]), _bits(ref["err"]))


def test_mspd_non_finite_poses_ties_explicit_candidates_and_bad_arguments():
    from megapose6d_amd import engine as eng

    c = vs.mspd_case(4, 200, 4, seed=9)
    c["syms"][0, 2] = c["syms"][0, 1]
    c["T_pred"] = np.stack([(c["T_gt"][i].astype(np.float64) @ c["syms"][0, 1].astype(np.float64)).astype(np.float32) for i in range(4)])
    c["T_pred"][1, 0, 3] = np.nan
    c["T_gt"][2, 1, 1] = np.inf
    ref = vs.mspd(c["T_pred"], c["T_gt"], c["syms"], c["n_sym"], c["pts"], c["K"], c["ids"], c["n_points"])
    args = (_dev(c["T_pred"]), _dev(c["T_gt"]), _dev(c["syms"]), _dev(c["n_sym"]), _dev(c["pts"]), _dev(c["K"]), _dev(c["ids"]), _dev(c["n_points"]))
    got = {k: v.cpu().numpy() for k, v in eng.pose_error_mspd(*args).items()}
    assert list(got["idx"]) == [1, -1, -1, 1] and np.all(np.isnan(got["err"][1:3]))
    for k in ("errs", "err", "idx", "T_gt_sym"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    # explicit candidates = the composed form
    c = vs.mspd_case(3, 500, 6, seed=10)
    args = (_dev(c["T_pred"]), _dev(c["T_gt"]), _dev(c["syms"]), _dev(c["n_sym"]), _dev(c["pts"]), _dev(c["K"]), _dev(c["ids"]), _dev(c["n_points"]))
    comp = eng.pose_error_mspd(*args)
    cand = np.stack([vs.mspd(c["T_pred"], c["T_gt"], c["syms"][:, s:s + 1], None, c["pts"], c["K"], c["ids"], c["n_points"])["T_gt_sym"] for s in range(6)], axis=1)
    expl = eng.pose_error_mspd(args[0], _dev(cand), None, None, *args[4:])
    for k in ("errs", "err", "idx", "T_gt_sym"):
        assert torch.equal(comp[k], expl[k]), k
    with pytest.raises(eng.EngineError):
        eng.pose_error_mspd(args[0], args[1], _dev(np.tile(np.eye(4, dtype=np.float32), (1, 513, 1, 1))), None, *args[4:])
    with pytest.raises(eng.EngineError):
        eng.pose_error_mspd(*args[:5], args[5][:2], *args[6:])
    with pytest.raises(eng.EngineError):
        eng.pose_error_mspd(*args, split=-1)


# --------------------------------------------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------------------------------------------
def test_bop_errors_end_to_end_against_the_emulation_on_oracle_renders(object_dataset, engine_meshes, oracle_meshes):
    from megapose6d_amd import evaluation as ev
    from megapose6d_amd.mesh_db import MeshDataBase
    from megapose6d_amd.renderer import Panda3dBatchRenderer
    from megapose6d_amd.tcoll import PandasTensorCollection
    from oracle import raster as orr
    from tests.support import synthetic as syn

    H, W = 240, 320
    rng = np.random.RandomState(3)
    labels = [o.label for o in object_dataset.list_objects]
    assert len(labels) == 3 and len(oracle_meshes) == 3 and len(engine_meshes) == 3
    K_im = np.stack([np.diag([0.5, 0.5, 1.0]) @ syn.K_EXAMPLE, np.diag([0.5, 0.5, 1.0]) @ syn.K_EXAMPLE + [[4.0, 0, 3.0], [0, -3.0, 2.0], [0, 0, 0]]]).astype(np.float32)
    gt_obj, gt_im = [0, 1, 2], [0, 0, 1]
    T_gt = np.stack([pes.pose(pes.random_rotation(rng), t) for t in ([-0.09, 0.0, 0.5], [0.1, 0.01, 0.55], [0.0, 0.0, 0.45])]).astype(np.float32)
    render = lambda o, T, im: orr.render(oracle_meshes[o], T[None], K_im[im][None], H, W, orr.FLAG_DEPTH)[2][0]   # noqa: E731  one sample per pixel
    d_gt = np.stack([render(gt_obj[g], T_gt[g], gt_im[g]) for g in range(3)])
    assert all((d > 0).sum() > 1500 for d in d_gt)
    # observed frames: the ground-truth objects of the frame, a nearer occluder over part of object 0, a region of zeros
    frames = np.zeros((2, H, W), np.float32)
    for g in range(3):
        f = frames[gt_im[g]]
        take = (d_gt[g] > 0) & ((f == 0) | (d_gt[g] < f))
        f[take] = d_gt[g][take]
    frames = np.where(frames > 0, frames + (rng.randn(2, H, W) * 0.002).astype(np.float32), np.float32(1.5)).astype(np.float32)
    ys, xs = np.nonzero(d_gt[0] > 0)
    frames[0, ys.min():(ys.min() + ys.max()) // 2, xs.min():xs.max() + 1] -= 0.1
    frames[1, H // 2:H // 2 + 30, :] = 0.0
    # four estimates per ground truth, interleaved (gt_index is no identity), one with a NaN pose
    n = 12
    gt_index = np.arange(n) % 3
    T_est = np.stack([pes.perturbed(rng, T_gt[g][None], 6.0, 0.006)[0] for g in gt_index])
    T_est[3] = T_gt[0]                                   # one exact estimate
    T_est[5, 1, 2] = np.nan
    infos = pd.DataFrame(dict(label=[labels[gt_obj[g]] for g in gt_index], batch_im_id=[gt_im[g] for g in gt_index], instance_id=np.arange(n)),
                         index=np.arange(n) + 100)
    gt_infos = pd.DataFrame(dict(label=[labels[o] for o in gt_obj], batch_im_id=gt_im))
    pred = PandasTensorCollection(infos, poses=torch.from_numpy(T_est).cuda())
    gt = PandasTensorCollection(gt_infos, poses=torch.from_numpy(T_gt).cuda())
    meshes = MeshDataBase.from_object_ds(object_dataset).batched(n_sym=4).cuda()
    renderer = Panda3dBatchRenderer(object_dataset, n_workers=1)
    rendered = []
    real = renderer.render_depth
    renderer.render_depth = lambda lab, *a, **k: (rendered.append(len(lab)), real(lab, *a, **k))[1]
    df = ev.bop_errors(pred, gt, meshes, renderer, torch.from_numpy(frames).cuda(), torch.from_numpy(K_im).cuda(), gt_index=gt_index)
    renderer.render_depth = real
    assert sum(rendered) == 3 + n                         # every distinct ground truth once, every estimate once
    names = [f"vsd_{t:.2f}" for t in vs.DEFAULT_TAUS]
    assert list(df.columns) == names + ["mssd", "mspd", "sym_id_mssd", "sym_id_mspd", "diameter"] and df.index.equals(pred.infos.index)
    # emulation on the oracle's renders
    ok = np.array([i != 5 for i in range(n)])
    d_est = np.stack([render(gt_obj[gt_index[i]], T_est[i], gt_im[gt_index[i]]) if ok[i] else np.zeros((H, W), np.float32) for i in range(n)])
    K_rows = K_im[[gt_im[g] for g in gt_index]]
    diam = df["diameter"].to_numpy().astype(np.float32)
    ref = vs.vsd(d_est, d_gt, frames, K_rows, diam, gt_ids=gt_index, im_ids=[gt_im[g] for g in gt_index])
    got = df[names].to_numpy()
    assert np.all(np.isnan(got[5])) and np.isnan(df["mssd"].iloc[5]) and np.isnan(df["mspd"].iloc[5]) and df["sym_id_mssd"].iloc[5] == -1
    assert np.array_equal(got[ok].astype(np.float32).view(np.uint32), ref["errs"][ok].view(np.uint32))
    assert np.all(got[3] == 0) and np.any((got[ok] > 0) & (got[ok] < 1))
    assert ref["counts"][0, 0] > ref["counts"][0, 1]     # the occluder hides part of object 0 ...
    # ... and the counts, from the engine's own renders through evaluation.vsd
    e_est = renderer.render_depth(list(infos["label"][ok]), torch.from_numpy(T_est[ok]).cuda(), torch.from_numpy(K_rows[ok]).cuda(), (H, W))
    e_gt = renderer.render_depth(list(gt_infos["label"]), torch.from_numpy(T_gt).cuda(), torch.from_numpy(K_im[gt_im]).cuda(), (H, W))
    out = ev.vsd(e_est, e_gt, torch.from_numpy(frames).cuda(), torch.from_numpy(K_rows[ok]).cuda(), torch.from_numpy(diam[ok]).cuda(),
                 gt_ids=torch.from_numpy(gt_index[ok]).cuda(), im_ids=torch.tensor([gt_im[g] for g in gt_index[ok]]).cuda())
    assert np.array_equal(out["counts"].cpu().numpy(), ref["counts"][ok])
    # MSSD / MSPD columns: the emulations on the engine's mesh tables
    ids = np.array([meshes.label_to_id[l] for l in infos["label"]], np.int32)
    n_points = np.array([meshes.infos[l]["n_points"] for l in meshes.labels], np.int32)
    n_sym = np.array([meshes.infos[l]["n_sym"] for l in meshes.labels], np.int32)
    pts, syms = meshes.points.cpu().numpy(), meshes.symmetries.cpu().numpy()
    m3 = pes.sym(T_est, T_gt[gt_index], syms, n_sym, pts, ids, n_points, reduce_max=True, with_diffs=False)
    m2 = vs.mspd(T_est, T_gt[gt_index], syms, n_sym, pts, K_rows, ids, n_points)
    assert np.array_equal(df["mssd"].to_numpy()[ok].astype(np.float32).view(np.uint32), m3["err"][ok].view(np.uint32))
    assert np.array_equal(df["mspd"].to_numpy()[ok].astype(np.float32).view(np.uint32), m2["err"][ok].view(np.uint32))
    assert np.array_equal(df["sym_id_mssd"].to_numpy(), m3["idx"]) and np.array_equal(df["sym_id_mspd"].to_numpy(), m2["idx"])
    rec = ev.bop_recall(df, image_width=W)
    assert 0 < rec["ar"] < 1 and rec["ar"] == pytest.approx((rec["ar_vsd"] + rec["ar_mssd"] + rec["ar_mspd"]) / 3)
    # evaluation.mspd: the shape of evaluation.mssd
    one = ev.mspd(torch.from_numpy(T_est[:3]).cuda(), torch.from_numpy(T_gt).cuda(), meshes.points[0, : n_points[0]], meshes.symmetries[0],
                  torch.from_numpy(K_rows[:3]).cuda())
    assert one["errs"].shape == (3, meshes.symmetries.shape[1]) and one["sym"].shape == (3, 4, 4) and one["idx"].dtype == torch.int64
    assert one["err"][0].item() == np.float32(df["mspd"].iloc[0])
