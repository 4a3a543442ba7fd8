"""GPU: the pose-error kernels (csrc/pose_error.hip) through the C ABI against the host emulation built from the same arithmetic header
(tests/pose_error_emul.cpp): bit for bit for every per-point vector, assignment, symmetry index and T_gt_sym; per-row scalars within
beta(sigma) = 64 * 2^-24 * sigma (maxima bit for bit) and bit-identical between launches and between the one-workgroup and split-row
forms.  Then the Python layer (megapose6d_amd.distances / .evaluation) on a synthetic three-object dataset.  Reads nothing outside
the tree."""
import numpy as np
import pandas as pd
import pytest
import torch

from support import pose_error as pes

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _np(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _object_points(rng, n, n_valid):
    pts = (rng.uniform(-1, 1, size=(n, 3)) * np.array([0.04, 0.06, 0.1])).astype(np.float32)
    if n_valid < n:
        pts[n_valid:] = pts[rng.choice(n_valid, size=n - n_valid)]
    return pts


def _case(b, N, S, seed, n_mesh=1, ragged=False):
    """meshes with n_valid <= N points (padded with re-drawn points when ragged) and n_sym <= S symmetries about z (identity-padded)"""
    rng = np.random.RandomState(seed)
    n_points = np.array([N if (not ragged or m == 0) else N - 1 - 997 * m for m in range(n_mesh)], np.int32)
    n_sym = np.array([S if (not ragged or m == 0) else max(1, S // (3 * m)) for m in range(n_mesh)], np.int32)
    pts = np.stack([_object_points(rng, N, int(n_points[m])) for m in range(n_mesh)])
    syms = np.tile(np.eye(4, dtype=np.float32), (n_mesh, S, 1, 1))
    for m in range(n_mesh):
        for s in range(n_sym[m]):
            syms[m, s] = pes.pose(pes.axis_rotation(2, 2 * np.pi * s / n_sym[m]), [0.0, 0.0, 0.002 * (s % 2)])
    ids = ((np.arange(b) + n_mesh - 1) % n_mesh).astype(np.int32)
    T_gt = pes.random_poses(rng, b)
    T_pred = np.stack([pes.perturbed(rng, (T_gt[i].astype(np.float64) @ syms[ids[i], (3 * i + 1) % n_sym[ids[i]]].astype(np.float64))[None], 1.5, 0.003)[0]
                       for i in range(b)])
    return dict(T_pred=T_pred, T_gt=T_gt, syms=syms, n_sym=n_sym, pts=pts, ids=ids, n_points=n_points)


def _betas(c):
    return np.array([pes.beta(c["T_pred"][i], c["T_gt"][i], points=c["pts"][c["ids"][i]], symmetries=c["syms"][c["ids"][i]]) for i in range(len(c["ids"]))])


def _gpu_sym(c, reduce, split, explicit=None):
    from megapose6d_amd import engine as eng

    if explicit is not None:
        out = eng.pose_error_sym(_dev(c["T_pred"]), _dev(explicit), None, None, _dev(c["pts"]), _dev(c["ids"]), _dev(c["n_points"]), reduce=reduce,
                                 split=split, with_diffs=True, with_alt=True)
    else:
        out = eng.pose_error_sym(_dev(c["T_pred"]), _dev(c["T_gt"]), _dev(c["syms"]), _dev(c["n_sym"]), _dev(c["pts"]), _dev(c["ids"]),
                                 _dev(c["n_points"]), reduce=reduce, split=split, with_diffs=True, with_alt=True)
    return _np(out)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32) if np.asarray(a).dtype == np.float32 else a, np.asarray(b).view(np.uint32) if np.asarray(b).dtype == np.float32 else b)


SHAPES = [(1, 1, 1, 1, False), (3, 7, 1, 1, False), (5, 63, 2, 1, False), (2, 10007, 64, 3, True), (576, 2000, 8, 1, False)]


@pytest.mark.parametrize("b,N,S,n_mesh,ragged", SHAPES)
def test_symmetry_set_kernels_match_the_emulation(b, N, S, n_mesh, ragged):
    c = _case(b, N, S, seed=100 + N, n_mesh=n_mesh, ragged=ragged)
    betas = _betas(c)
    worst = 0.0
    for reduce_max in (0, 1):
        ref = pes.sym(c["T_pred"], c["T_gt"], c["syms"], c["n_sym"], c["pts"], c["ids"], c["n_points"], reduce_max=bool(reduce_max))
        got = _gpu_sym(c, reduce_max, 0)
        # deterministic: a second launch, one workgroup per row, and a forced split give the same bits
        for other in (_gpu_sym(c, reduce_max, 0), _gpu_sym(c, reduce_max, 1), _gpu_sym(c, reduce_max, 7)):
            for k in got:
                assert _same_bits(got[k], other[k]), k
        # errs of every symmetry: within beta of the emulation's (the max form: bit for bit)
        fin = np.isfinite(ref["errs"])
        assert np.array_equal(fin, np.isfinite(got["errs"])) and np.array_equal(np.isposinf(ref["errs"]), np.isposinf(got["errs"]))
        dev = np.abs(np.where(fin, got["errs"], 0) - np.where(fin, ref["errs"], 0)).max(1)
        worst = max(worst, float((dev / betas).max()) * 64)
        assert np.all(dev <= betas)
        if reduce_max:
            assert _same_bits(got["errs"], ref["errs"]) and _same_bits(got["err"], ref["err"])
        else:
            assert _same_bits(got["err_alt"], ref["err_alt"])          # the minimum of the max form
        assert np.all(np.abs(got["err_alt"] - ref["err_alt"]) <= betas)
        # symmetry index: bit for bit where the emulation's best and second best differ by more than 2 beta, else by the float64 rule
        srt = np.sort(ref["errs"], axis=1)
        clear = (srt[:, 1] - srt[:, 0] > 2 * betas) if S > 1 else np.ones(b, bool)
        assert clear.mean() >= 0.9, clear.mean()
        assert np.array_equal(got["idx"][clear], ref["idx"][clear])
        for i in np.flatnonzero(~clear):
            m = c["ids"][i]
            G = c["T_gt"][i].astype(np.float64) @ c["syms"][m, : c["n_sym"][m]].astype(np.float64)
            P = c["pts"][m, : c["n_points"][m]]
            norms = np.linalg.norm(pes.f64_transform(G, P) - pes.f64_transform(c["T_pred"][i], P)[None], axis=-1)
            e64 = norms.max(1) if reduce_max else norms.mean(1)
            assert 0 <= got["idx"][i] < c["n_sym"][m] and e64[got["idx"][i]] - e64.min() <= betas[i]
        same = got["idx"] == ref["idx"]
        assert _same_bits(got["T_gt_sym"][same], ref["T_gt_sym"][same]) and _same_bits(got["diffs"][same], ref["diffs"][same])
        assert np.all(np.abs(got["err"] - ref["err"])[same] <= betas[same])
        # the explicit-candidate form on the same sets = the composed form (every symmetry slot composed, identity padding included)
        if not ragged:
            from megapose6d_amd import engine as eng

            cand = np.stack([_np(eng.pose_error_sym(_dev(c["T_pred"]), _dev(c["T_gt"]), _dev(c["syms"][:, s:s + 1]), None, _dev(c["pts"]), _dev(c["ids"]),
                                                    _dev(c["n_points"])))["T_gt_sym"] for s in range(S)], axis=1)
            expl = _gpu_sym(c, reduce_max, 0, explicit=cand)
            for k in got:
                assert _same_bits(got[k], expl[k]), k
    print(f"sym ({b},{N},{S}): largest deviation of a mean from the emulation {worst:.2f} x 2^-24 sigma")


NN_SHAPES = [(1, 1, 1, False), (3, 7, 1, False), (5, 63, 1, False), (2, 10007, 3, True), (576, 2000, 1, False), (1, 20011, 1, False)]


@pytest.mark.parametrize("b,N,n_mesh,ragged", NN_SHAPES)
def test_nearest_neighbour_kernels_match_the_emulation(b, N, n_mesh, ragged):
    from megapose6d_amd import engine as eng

    c = _case(b, N, 1, seed=200 + N, n_mesh=n_mesh, ragged=ragged)
    c["T_pred"] = pes.perturbed(np.random.RandomState(N), c["T_gt"], 20.0, 0.02)
    betas = _betas(c)
    ref = pes.nn(c["T_pred"], c["T_gt"], c["pts"], c["ids"], c["n_points"])
    run = lambda split: _np(eng.pose_error_nn(_dev(c["T_pred"]), _dev(c["T_gt"]), _dev(c["pts"]), _dev(c["ids"]), _dev(c["n_points"]), split=split))  # noqa: E731
    got = run(0)
    for other in (run(0), run(1), run(5)):
        for k in got:
            assert _same_bits(got[k], other[k]), k
    assert np.array_equal(got["assign"], ref["assign"])
    assert _same_bits(got["diffs"], ref["diffs"])
    assert _same_bits(got["max"], ref["max"])
    dev = np.abs(got["mean"] - ref["mean"])
    assert np.all(dev <= betas)
    print(f"nn ({b},{N}): largest deviation of a mean from the emulation {float((dev / betas).max()) * 64:.2f} x 2^-24 sigma")


def test_nearest_neighbour_on_a_row_of_identical_points_and_on_duplicates():
    from megapose6d_amd import engine as eng

    rng = np.random.RandomState(4)
    base = _object_points(rng, 1500, 1500)
    pts = np.stack([np.repeat(base[:1], 1500, axis=0), np.concatenate([base[:700], base[rng.choice(700, size=800)]])])
    T_gt = pes.random_poses(rng, 2)
    T_pred = np.stack([pes.perturbed(rng, T_gt[:1], 10.0, 0.02)[0], T_gt[1]])
    ref = pes.nn(T_pred, T_gt, pts)
    got = _np(eng.pose_error_nn(_dev(T_pred), _dev(T_gt), _dev(pts)))
    assert np.all(got["assign"][0] == 0)
    first = np.array([int(np.flatnonzero((pts[1] == p).all(1))[0]) for p in pts[1]])
    assert np.array_equal(got["assign"][1], first) and got["mean"][1] == 0 and got["max"][1] == 0
    for k in ("assign", "diffs", "max"):
        assert _same_bits(got[k], ref[k]), k


def test_rigid_and_projection_errors_match_the_emulation():
    from megapose6d_amd import engine as eng

    c = _case(64, 3001, 1, seed=5, n_mesh=3, ragged=True)
    c["n_points"][:] = [3001, 2500, 1]
    K = np.tile(np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1.0]], np.float32), (64, 1, 1))
    ref = pes.rigid(c["T_gt"], c["T_pred"], K, c["pts"], c["ids"], c["n_points"])
    run = lambda: _np(eng.pose_error_rigid(_dev(c["T_gt"]), _dev(c["T_pred"]), _dev(K), _dev(c["pts"]), _dev(c["ids"]), _dev(c["n_points"])))  # noqa: E731
    got, again = run(), run()
    for k in got:
        assert _same_bits(got[k], again[k]), k
    betas = _betas(c)
    assert _same_bits(got["trans_err"], ref["trans_err"])
    assert np.all(np.abs(got["rot_err_deg"] - ref["rot_err_deg"]) <= 1e-4)      # atan2f is the device library's: the contract test's bound
    assert np.all(np.abs(got["proj_error"] - ref["proj_error"]) <= betas), np.abs(got["proj_error"] - ref["proj_error"]).max()
    only = _np(eng.pose_error_rigid(_dev(c["T_gt"]), _dev(c["T_pred"])))
    assert _same_bits(only["trans_err"], got["trans_err"]) and _same_bits(only["rot_err_deg"], got["rot_err_deg"])
    # rotation error at the angles of the contract test, against float64 atan2
    rng = np.random.RandomState(0)
    Ta, Tb = [], []
    for angle in (0.0, 1e-3, 5.0, 90.0, 179.999, 180.0):
        A = pes.random_poses(rng, 1)[0].astype(np.float64)
        Ta.append(A)
        Tb.append(pes.pose(pes.axis_rotation(1, np.deg2rad(angle)) @ A[:3, :3], A[:3, 3]))
    Ta, Tb = np.stack(Ta).astype(np.float32), np.stack(Tb).astype(np.float32)
    rot = _np(eng.pose_error_rigid(_dev(Ta), _dev(Tb)))["rot_err_deg"]
    for i in range(len(Ta)):
        assert abs(rot[i] - pes.f64_rot_err_deg(Ta[i], Tb[i])) <= 1e-4


def test_non_finite_poses_and_bad_arguments():
    from megapose6d_amd import engine as eng

    c = _case(4, 300, 4, seed=8)
    c["T_pred"][1, 2, 3] = np.nan
    c["T_gt"][2, 0, 0] = np.inf
    got = _gpu_sym(c, 0, 0)
    assert list(got["idx"][1:3]) == [-1, -1] and np.all(np.isnan(got["err"][1:3])) and np.all(np.isnan(got["errs"][1:3])) and got["idx"][0] >= 0 and got["idx"][3] >= 0
    nn = _np(eng.pose_error_nn(_dev(c["T_pred"]), _dev(c["T_gt"]), _dev(c["pts"]), _dev(c["ids"]), _dev(c["n_points"])))
    assert np.all(nn["assign"][1:3] == -1) and np.all(np.isnan(nn["mean"][1:3])) and np.all(nn["assign"][[0, 3]] >= 0)
    ref = pes.nn(c["T_pred"], c["T_gt"], c["pts"], c["ids"], c["n_points"])
    assert np.array_equal(nn["assign"], ref["assign"])
    with pytest.raises(eng.EngineError):
        eng.pose_error_sym(_dev(c["T_pred"]), _dev(c["T_gt"]), _dev(np.tile(np.eye(4, dtype=np.float32), (1, 513, 1, 1))), None, _dev(c["pts"]), _dev(c["ids"]))
    with pytest.raises(eng.EngineError):
        eng.pose_error_nn(_dev(c["T_pred"]), _dev(c["T_gt"]), torch.zeros(1, 0, 3).cuda(), _dev(c["ids"]))


# --------------------------------------------------------------------------------------------------------------------------------
# Python layer
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sym_dataset(tmp_path_factory):
    from megapose6d_amd.mesh_db import MeshDataBase
    from megapose6d_amd.object_dataset import RigidObject
    from megapose6d_amd.symmetries import ContinuousSymmetry, DiscreteSymmetry
    from tests.support import synthetic as syn

    base = syn.make_object_dataset(tmp_path_factory.mktemp("sym_meshes"), n_objects=3, seed=3, n_theta=36, n_z=30)
    o = base.list_objects
    half = pes.pose(pes.axis_rotation(2, np.pi), [0.0, 0.0, 0.0])
    objs = [RigidObject(o[0].label, o[0].mesh_path, mesh_units="mm", symmetries_continuous=[ContinuousSymmetry(offset=np.zeros(3), axis=np.array([0, 0, 1]))]),
            RigidObject(o[1].label, o[1].mesh_path, mesh_units="mm", symmetries_discrete=[DiscreteSymmetry(pose=half)]),
            RigidObject(o[2].label, o[2].mesh_path, mesh_units="mm")]
    meshes = MeshDataBase(objs).batched(n_sym=16).cuda()
    return objs, meshes


def _tables(meshes, rng, n_rows):
    from megapose6d_amd.tcoll import PandasTensorCollection

    labels = [meshes.labels[i % 3] for i in range(n_rows)]
    sym_ids = []
    T_gt = pes.random_poses(rng, n_rows)
    T_pred = []
    for i, l in enumerate(labels):
        m = meshes.label_to_id[l]
        k = (5 * i + 3) % meshes.infos[l]["n_sym"]
        sym_ids.append(k)
        T_pred.append((T_gt[i].astype(np.float64) @ meshes.symmetries[m, k].cpu().numpy().astype(np.float64)).astype(np.float32))
    infos = pd.DataFrame(dict(label=labels, scene_id=np.arange(n_rows) // 3, view_id=0, instance_id=np.arange(n_rows)), index=np.arange(n_rows)[::-1])
    return (PandasTensorCollection(infos.copy(), poses=torch.from_numpy(np.stack(T_pred)).cuda()),
            PandasTensorCollection(infos.copy(), poses=torch.from_numpy(T_gt).cuda()), np.array(sym_ids))


def test_pose_errors_table_on_symmetric_objects(sym_dataset):
    from megapose6d_amd import evaluation as ev

    objs, meshes = sym_dataset
    assert meshes.n_sym_mapping == {objs[0].label: 16, objs[1].label: 2, objs[2].label: 1}
    rng = np.random.RandomState(0)
    pred, gt, sym_ids = _tables(meshes, rng, 12)
    K = torch.tensor([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1.0]]).repeat(12, 1, 1).cuda()
    df = ev.pose_errors(pred, gt, meshes, K=K)
    assert list(df.columns) == ["add", "add_sym", "mssd", "adds", "sym_id", "trans_err", "rot_err_deg", "proj_error", "diameter"]
    assert df.index.equals(pred.infos.index) and df["sym_id"].dtype == np.int64 and all(df[c].dtype == np.float64 for c in df.columns if c != "sym_id")
    pts = meshes.points.cpu().numpy()
    for r in range(12):
        l = pred.infos["label"].iloc[r]
        m = meshes.label_to_id[l]
        beta = pes.beta(pred.poses[r].cpu().numpy(), gt.poses[r].cpu().numpy(), points=pts[m], symmetries=meshes.symmetries[m].cpu().numpy())
        row = df.iloc[r]
        # the prediction is the ground truth times a declared symmetry: zero against the symmetry set, that symmetry picked
        assert row["add_sym"] <= beta and row["mssd"] <= beta and row["trans_err"] <= beta and row["sym_id"] == sym_ids[r]
        assert row["rot_err_deg"] <= 1e-4 + np.rad2deg(8 * 2.0 ** -24) * 4     # two fp32 rotation matrices equal to a few roundings per entry
        if sym_ids[r] != 0:
            assert row["add"] > 1e-3                                        # ... while the plain ADD sees the rotation
        else:
            assert row["add"] == row["add_sym"]
        assert row["adds"] <= row["add"]
        assert abs(row["diameter"] - objs[m].diameter_meters) <= 1e-6
    asym = (pred.infos["label"] == objs[2].label).to_numpy()
    assert np.array_equal(df["add_sym"].to_numpy()[asym], df["add"].to_numpy()[asym])      # exactly
    # a generic prediction: adds <= add row by row, add_sym <= add, and the summary is the pandas one-liner
    pred2 = pred.clone()
    pred2.poses = torch.from_numpy(pes.perturbed(rng, gt.poses.cpu().numpy(), 8.0, 0.03)).cuda()
    df2 = ev.pose_errors(pred2, gt, meshes, K=K)
    assert np.all(df2["adds"] <= df2["add"]) and np.all(df2["add_sym"] <= df2["add"]) and np.all(df2["add_sym"] <= df2["mssd"])
    s = ev.summary(df2)
    assert s == {"add0.1d": float((df2["add"] < 0.1 * df2["diameter"]).mean()), "5deg_5cm": float(((df2["trans_err"] < 0.05) & (df2["rot_err_deg"] < 5)).mean()),
                 "proj2d_5px": float((df2["proj_error"] < 5).mean())}
    assert 0 < s["5deg_5cm"] < 1 or 0 < s["add0.1d"] < 1 or 0 < s["proj2d_5px"] < 1
    no_nn = ev.pose_errors(pred2, gt, meshes, nearest=False)
    assert list(no_nn.columns) == ["add", "add_sym", "mssd", "sym_id", "trans_err", "rot_err_deg", "diameter"]
    assert np.array_equal(no_nn["add_sym"].to_numpy(), df2["add_sym"].to_numpy())


def test_compute_errors_on_a_prediction_runner_dict(sym_dataset):
    from megapose6d_amd import evaluation as ev

    objs, meshes = sym_dataset
    rng = np.random.RandomState(1)
    pred, gt, _ = _tables(meshes, rng, 9)
    method = "gt_detections+coarse"

    def table(angle):
        p = gt.clone()
        p.poses = torch.from_numpy(pes.perturbed(rng, pred.poses.cpu().numpy(), angle, angle * 1e-3)).cuda()
        return p

    preds = {f"{method}/ground_truth": gt, f"{method}/refiner/init": table(8.0), f"{method}/refiner/iteration=1": table(3.0),
             f"{method}/refiner/iteration=2": table(1.0), f"{method}/refiner/final": table(1.0), f"{method}/coarse": table(8.0),
             "other/refiner/init": table(5.0)}
    before = {k: list(p.infos.columns) for k, p in preds.items()}
    out = ev.compute_errors(preds, method, meshes)
    assert out is preds
    for k, p in preds.items():
        new = [c for c in p.infos.columns if c not in before[k]]
        if k == f"{method}/refiner/init":
            assert new == ["trans_err", "rot_err_deg"]
        elif "iteration=" in k and k.startswith(method):
            assert new == ["trans_err", "rot_err_deg", "trans_err_init", "rot_err_deg_init"]
            assert np.array_equal(p.infos["rot_err_deg_init"].to_numpy(), preds[f"{method}/refiner/init"].infos["rot_err_deg"].to_numpy())
        else:
            assert new == []
    # errors are measured against the CLOSEST symmetric ground truth: the 8 / 3 / 1 degree perturbations show, not the symmetry
    assert preds[f"{method}/refiner/init"].infos["rot_err_deg"].max() <= 8.001
    assert preds[f"{method}/refiner/iteration=2"].infos["rot_err_deg"].max() <= 1.001
    ref = ev.compute_pose_error(gt.poses, preds[f"{method}/refiner/iteration=2"].poses)
    asym = (gt.infos["label"] == objs[2].label).to_numpy()
    assert np.allclose(ref["roterr_deg"].cpu().numpy()[asym], preds[f"{method}/refiner/iteration=2"].infos["rot_err_deg"].to_numpy()[asym], atol=1e-4)


def test_distances_module_has_the_reference_shapes(sym_dataset):
    from megapose6d_amd import distances as dist
    from megapose6d_amd import evaluation as ev

    _, meshes = sym_dataset
    rng = np.random.RandomState(2)
    b = 5
    n = meshes.infos[meshes.labels[2]]["n_points"]
    pts = meshes.points[2, :n].unsqueeze(0).repeat(b, 1, 1).contiguous()
    T_gt = torch.from_numpy(pes.random_poses(rng, b)).cuda()
    T_pred = torch.from_numpy(pes.perturbed(rng, T_gt.cpu().numpy(), 10.0, 0.01)).cuda()
    syms = meshes.symmetries[0]
    cand = T_gt.unsqueeze(1) @ syms.unsqueeze(0)
    d_add, d_syms = dist.dists_add(T_pred, T_gt, pts), dist.dists_add_symmetries(T_pred, cand, pts)
    d_nn, assign = dist.dists_add_symmetric(T_pred, T_gt, pts, return_assign=True)
    assert d_add.shape == d_syms.shape == d_nn.shape == (b, n, 3) and assign.shape == (b, n) and assign.dtype == torch.int64
    ref = pes.sym(T_pred.cpu().numpy(), T_gt.cpu().numpy()[:, None], None, None, pts.cpu().numpy())
    assert np.array_equal(d_add.cpu().numpy(), ref["diffs"])
    refn = pes.nn(T_pred.cpu().numpy(), T_gt.cpu().numpy(), pts.cpu().numpy())
    assert np.array_equal(assign.cpu().numpy(), refn["assign"]) and np.array_equal(d_nn.cpu().numpy(), refn["diffs"])
    assert torch.all(d_nn.norm(dim=-1).mean(-1) <= d_add.norm(dim=-1).mean(-1))
    out = ev.mssd(T_pred, T_gt, pts[0], syms)
    assert out["errs"].shape == (b, 16) and out["sym"].shape == (b, 4, 4) and out["idx"].dtype == torch.int64
    refm = pes.sym(T_pred.cpu().numpy(), T_gt.cpu().numpy(), syms.cpu().numpy()[None], None, pts[:1].cpu().numpy(), np.zeros(b, np.int32))
    assert np.array_equal(out["idx"].cpu().numpy(), refm["idx"]) and np.array_equal(out["T_gt_sym"].cpu().numpy(), refm["T_gt_sym"])
    assert torch.equal(d_syms.norm(dim=-1).mean(-1) <= d_add.norm(dim=-1).mean(-1) + 1e-7, torch.ones(b, dtype=torch.bool).cuda())
