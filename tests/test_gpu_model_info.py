"""GPU: the model-info kernels (csrc/model_info.hip) through the C ABI against the host emulation built from the same rules header
(tests/model_info_emul.cpp): d2 bit for bit, the pair exactly, the bounds bit for bit against numpy, on every point set of
tests/support/model_info.py at every tile (0 = the library's choice, one job per 8192 j points; 64, 128, 256 = several jobs and
several stages at a few hundred points); several objects in one launch, with padding rows 100 m away and with a NaN object;
`evaluation.model_info` on a mesh database against a float64 brute force; and `diameters="exact"` against the default in `pose_errors`
and `bop_scores`.  Bad arguments are refused before any launch.  Tile culling is not built, so there is nothing to switch."""
import numpy as np
import pandas as pd
import pytest
import torch

from support import model_info as mi
from support import pose_error as pes

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gpu(points, n_points, tile):
    from megapose6d_amd import engine as eng

    d2, pair, bounds = eng.model_info(torch.from_numpy(np.ascontiguousarray(points)).cuda(), np.asarray(n_points, np.int32), tile=tile)
    assert d2.dtype == torch.float32 and pair.dtype == torch.int32 and bounds.dtype == torch.float32
    return d2.cpu().numpy(), pair.cpu().numpy(), bounds.cpu().numpy()


@pytest.mark.parametrize("tile", mi.TILES)
def test_kernel_matches_the_emulation_on_every_point_set(tile):
    for name, c in mi.cases().items():
        p = c["points"]
        want_d2, want_pair, want_bounds = mi.emul_case(name, tile)
        d2, pair, bounds = _gpu(p[None], [len(p)], tile)
        assert d2.shape == (1,) and pair.shape == (1, 2) and bounds.shape == (1, 6)
        assert _bits(d2)[0] == _bits(want_d2) and tuple(pair[0]) == want_pair, (name, tile, d2, pair, want_d2, want_pair)
        assert np.array_equal(_bits(bounds[0]), _bits(mi.numpy_bounds(p))) and np.array_equal(_bits(bounds[0]), _bits(want_bounds)), (name, tile)
        if c["pair"] is not None:
            assert tuple(pair[0]) == c["pair"]


@pytest.mark.parametrize("tile", mi.TILES)
def test_three_objects_in_one_launch(tile):
    points, n = mi.three_objects()
    singles = [_gpu(points[o:o + 1], n[o:o + 1], tile) for o in range(3)]
    d2, pair, bounds = _gpu(points, n, tile)
    want = mi.emul(points, n, tile)
    assert np.array_equal(_bits(d2), _bits(want[0])) and np.array_equal(pair, want[1]) and np.array_equal(_bits(bounds), _bits(want[2]))
    for o in range(3):
        assert _bits(d2)[o] == _bits(singles[o][0])[0] and np.array_equal(pair[o], singles[o][1][0])
        assert np.array_equal(_bits(bounds[o]), _bits(singles[o][2][0]))
        assert np.array_equal(_bits(bounds[o]), _bits(mi.numpy_bounds(points[o, :n[o]])))
    assert (d2 < 50.0).all() and (pair < n[:, None]).all()          # the padding 100 m away never wins
    bad, _ = mi.three_objects(with_nan=True)
    b_d2, b_pair, b_bounds = _gpu(bad, n, tile)
    assert np.isnan(b_d2[1]) and tuple(b_pair[1]) == (-1, -1) and np.isnan(b_bounds[1]).all()
    for o in (0, 2):
        assert _bits(b_d2)[o] == _bits(d2)[o] and np.array_equal(b_pair[o], pair[o]) and np.array_equal(_bits(b_bounds[o]), _bits(bounds[o]))


def test_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import engine as eng

    p = torch.zeros(2, 10, 3, device="cuda")
    for n_points, tile in (([10, 11], 0), ([0, 3], 0), ([3], 0), ([3, 3], 32), ([3, 3], 96), ([3, 3], 2048)):
        with pytest.raises(eng.EngineError):
            eng.model_info(p, np.asarray(n_points, np.int32), tile=tile)
    with pytest.raises(eng.EngineError):
        eng.model_info(torch.zeros(2, 10, 2, device="cuda"), [3, 3])
    lib = eng._lib.load()
    h = np.asarray([3, 3], np.int32)
    assert lib.mp_model_info_scratch_bytes(2, h.ctypes.data, 0) > 0 and lib.mp_model_info_scratch_bytes(2, h.ctypes.data, 65) == 0
    assert lib.mp_model_info_scratch_bytes(0, h.ctypes.data, 0) == 0


@pytest.fixture(scope="module")
def two_objects(tmp_path_factory):
    from megapose6d_amd.mesh_db import MeshDataBase
    from tests.support import synthetic as syn

    ds = syn.make_object_dataset(tmp_path_factory.mktemp("model_info_meshes"), n_objects=2, seed=3, n_theta=24, n_z=21)
    return ds, MeshDataBase.from_object_ds(ds).batched(n_sym=4).cuda()


def test_evaluation_model_info_on_a_mesh_database(two_objects):
    from megapose6d_amd import evaluation as ev

    ds, meshes = two_objects
    info = ev.model_info(meshes)
    assert list(info.index) == list(meshes.labels) and list(info.columns) == list(ev.MODEL_INFO_COLUMNS)
    assert ev.model_info(meshes, tile=64).equals(info)
    pts = meshes.points.cpu().numpy()
    box = ev._diameters(meshes)
    for o, label in enumerate(meshes.labels):
        n = meshes.infos[label]["n_points"]
        p, row = pts[o, :n], info.loc[label]
        assert 0 <= row["pt_i"] <= row["pt_j"] < n                                        # real rows, not padding
        want = mi.brute_force(p)
        print(f"{label}: n {n}, brute force {want!r}, model_info {row['diameter']!r}, box diagonal {box[label]!r}")
        assert abs(row["diameter"] - want) <= mi.REL_BOUND * want
        assert row["diameter"] == mi.pair_distance(p, (row["pt_i"], row["pt_j"])) and row["diameter"] < box[label]
        assert np.array_equal(_bits(row[list(ev.MODEL_INFO_COLUMNS[1:7])].to_numpy()), _bits(mi.numpy_bounds(p)))
    exact = ev.resolve_diameters(meshes, "exact", list(meshes.labels))
    assert exact == info["diameter"].to_dict() and ev.resolve_diameters(meshes, None, list(meshes.labels)) is box


def test_exact_diameter_turns_a_correct_estimate_wrong(two_objects):
    """One cylinder-like object (a bottle of revolution), one estimate shifted so that its MSSD lies between theta * d_exact and
    theta * d_box for theta = BOP_THRESHOLDS[K_THETA]: correct under the default diameter, wrong under BOP's."""
    from megapose6d_amd import evaluation as ev
    from megapose6d_amd.renderer import Panda3dBatchRenderer
    from megapose6d_amd.tcoll import PandasTensorCollection
    from tests.support import synthetic as syn

    K_THETA = 1
    ds, meshes = two_objects
    label = str(meshes.labels[0])
    theta = ev.BOP_THRESHOLDS[K_THETA]
    d_box = ev.resolve_diameters(meshes, None, [label])[label]
    d_exact = ev.resolve_diameters(meshes, "exact", [label])[label]
    assert d_exact < 0.97 * d_box
    H, W = 60, 80
    K = torch.from_numpy((np.diag([0.125, 0.125, 1.0]) @ syn.K_EXAMPLE)[None].astype(np.float32)).cuda()
    T_gt = pes.pose(pes.random_rotation(np.random.RandomState(4)), [0.0, 0.0, 0.5]).astype(np.float32)[None]
    T_est = T_gt.copy()
    T_est[0, 0, 3] += theta * 0.5 * (d_exact + d_box)           # a pure shift: every model point moves by it, so MSSD is its length
    gt = PandasTensorCollection(pd.DataFrame(dict(label=[label], batch_im_id=[0])), poses=torch.from_numpy(T_gt).cuda())
    pred = PandasTensorCollection(pd.DataFrame(dict(label=[label], batch_im_id=[0], score=[1.0])), poses=torch.from_numpy(T_est).cuda())
    renderer = Panda3dBatchRenderer(ds, n_workers=1)
    frames = renderer.render_depth([label], gt.poses, K, (H, W))
    frames = torch.where(frames > 0, frames, torch.full_like(frames, 1.5))

    given = {label: 0.123}
    dfs = {k: ev.bop_errors(pred, gt, meshes, renderer, frames, K, diameters=v) for k, v in (("box", None), ("exact", "exact"), ("given", given))}
    assert dfs["box"]["diameter"].tolist() == [d_box] and dfs["exact"]["diameter"].tolist() == [d_exact] and dfs["given"]["diameter"].tolist() == [0.123]
    assert ev.bop_errors(pred, gt, meshes, renderer, frames, K).equals(dfs["box"])
    mssd = float(dfs["box"]["mssd"].iloc[0])
    assert mssd == float(dfs["exact"]["mssd"].iloc[0])
    assert theta * d_exact < mssd < theta * d_box, (theta * d_exact, mssd, theta * d_box)      # the placement this test is about
    pe = {k: ev.pose_errors(pred, gt, meshes, nearest=False, diameters=v) for k, v in (("box", None), ("exact", "exact"), ("given", given))}
    assert pe["box"]["diameter"].tolist() == [d_box] and pe["exact"]["diameter"].tolist() == [d_exact] and pe["given"]["diameter"].tolist() == [0.123]
    assert ev.pose_errors(pred, gt, meshes, nearest=False).equals(pe["box"])
    with pytest.raises(KeyError):
        ev.pose_errors(pred, gt, meshes, nearest=False, diameters={"another": 0.1})
    with pytest.raises(ValueError):
        ev.bop_errors(pred, gt, meshes, renderer, frames, K, diameters={label: 0.0})

    at = ("mssd", K_THETA)
    s_box, m_box = ev.bop_scores(pred, gt, meshes, renderer, frames, K, image_width=W, return_matches=True, matches_at=at)
    s_def, m_def = ev.bop_scores(pred, gt, meshes, renderer, frames, K, image_width=W, return_matches=True, matches_at=at, diameters=None)
    s_exact, m_exact = ev.bop_scores(pred, gt, meshes, renderer, frames, K, image_width=W, return_matches=True, matches_at=at, diameters="exact")
    assert s_def == s_box and m_def.equals(m_box)
    assert m_box.values.tolist() == [[0, 0]] and len(m_exact) == 0                              # correct under None, wrong under "exact"
    assert s_exact["ar_mssd"] == pytest.approx(s_box["ar_mssd"] - 0.1, abs=1e-12) and s_exact["ar_mspd"] == s_box["ar_mspd"]     # one theta of ten
    s_given = ev.bop_scores(pred, gt, meshes, renderer, frames, K, image_width=W, diameters={label: d_exact})
    assert s_given == s_exact
