"""GPU: the symmetry kernels (csrc/symmetry.hip) through the C ABI against the host emulation built from the same rules header
(tests/symmetry_emul.cpp): the accept flags of both modes, and dev2 and the worst point bit for bit (mode 1: every candidate; mode 0:
the accepted ones), on the fixtures batched as one call and at the smallest shapes where the kernel can go wrong; then
`evaluation.find_symmetries` end to end on a mesh database, and its result in `pose_errors`."""
import numpy as np
import pandas as pd
import pytest
import torch

from support import pose_error as pes
from support import symmetry as sy

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gpu(args, mode, tile=0):
    from megapose6d_amd import engine as eng

    v, f, t, R, c, vo, fo, to, co, tol = args
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()   # noqa: E731
    accept, dev2, worst = eng.symmetry_check(dev(v), np.asarray(f, np.int32), dev(t), dev(R).reshape(-1, 3, 3), dev(c), vo, fo, to, co, tol, mode=mode,
                                             tile=tile)
    assert accept.dtype == torch.uint8 and dev2.dtype == torch.float32 and worst.dtype == torch.int32
    return accept.cpu().numpy(), dev2.cpu().numpy(), worst.cpu().numpy()


def _check(args, tile=0):
    """both modes on the device against the emulation -> the emulation's mode-1 (accept, dev2, worst)"""
    n_cand = int(np.asarray(args[8])[-1])
    rc, acc1, dev1, worst1 = sy.emul(*args, mode=1, tile=tile)
    assert rc == 0
    got = _gpu(args, 1, tile)
    np.testing.assert_array_equal(got[0][:n_cand], acc1)
    np.testing.assert_array_equal(_bits(got[1][:n_cand]), _bits(dev1))
    np.testing.assert_array_equal(got[2][:n_cand], worst1)
    rc, acc0, dev0, worst0 = sy.emul(*args, mode=0, tile=tile)
    assert rc == 0
    np.testing.assert_array_equal(acc0, acc1)                     # the screen decides as the measurement does
    got = _gpu(args, 0, tile)
    np.testing.assert_array_equal(got[0][:n_cand], acc0)
    np.testing.assert_array_equal(_bits(got[1][:n_cand]), _bits(dev0))        # NaN bits for the rejected, dev2 bits for the accepted
    np.testing.assert_array_equal(got[2][:n_cand], worst0)
    keep = acc1 > 0
    np.testing.assert_array_equal(_bits(got[1][:n_cand][keep]), _bits(dev1[keep]))
    assert np.isnan(got[1][:n_cand][~keep]).all() and (got[2][:n_cand][~keep] == -1).all()
    return acc1, dev1, worst1


def _args_of(named, n_samples, tile=0):
    """the arguments `find_symmetries` hands to symmetry_check for these meshes (test points sampled by the emulation)"""
    from megapose6d_amd import evaluation as ev

    ms = sy.MeshSet(named)
    backend = sy.EmulBackend()
    table = ev.find_symmetries(ms, rel_tol=sy.REL_TOL, n_samples=n_samples, diameters=ms.diameters(), device="cpu", tile=tile, backend=backend)
    return table, backend.calls[0]["args"]


def test_fixtures_in_one_call_match_the_emulation():
    table, backend = sy.found()
    acc, _, _ = _check(backend.calls[0]["args"])
    assert 0 < acc.sum() < len(acc)


@pytest.mark.parametrize("n_tests", (255, 256, 257, 513))
def test_test_point_counts_around_a_block(n_tests):
    v, f = sy.meshes()["hex_prism"]
    table, args = _args_of({"hex_prism": (v, f)}, n_tests - len(v))
    assert args[7][-1] == n_tests and table.loc["hex_prism", "n_symmetries"] == 12
    _check(args)


@pytest.mark.parametrize("n_tri", (63, 64, 65))
def test_triangle_counts_around_a_tile(n_tri):
    tile = sy.limits()["tile_step"]
    table, args = _args_of({"cone": sy.cone(n_tri, 0.08, 0.2, closed=False)}, 40, tile=tile)
    assert args[6][-1] == n_tri == tile + (n_tri - 64) and table.loc["cone", "n_symmetries"] == n_tri
    _check(args, tile=tile)


def test_single_triangle():
    a = 2.0 * np.pi / 3.0
    tri = (np.asarray([[0.1 * np.cos(k * a), 0.1 * np.sin(k * a), 0.02] for k in range(3)], np.float32), np.asarray([[0, 1, 2]], np.int32))
    table, args = _args_of({"triangle": tri}, 30)
    assert table.loc["triangle", "n_symmetries"] == 6             # three turns about the normal, three flips
    _check(args)


def test_rejected_in_the_first_block_and_in_the_last():
    """three copies of the cube with its 24 candidates: one point 5 cm off the surface as the LAST test point (every candidate is
    rejected only after the last block), as the FIRST (rejected in the first block), and not at all (accepted after the last block)"""
    _, args = _args_of({"cube": sy.meshes()["cube"]}, 520)      # 528 test points: three blocks with the added one
    v, f, t, R, c, vo, fo, to, co, tol = args
    off =np.asarray([[0.15, 0.0, 0.0]], np.float32)
    tests = [np.concatenate([t, off]), np.concatenate([off, t]), t]
    three = (np.concatenate([v] * 3), np.concatenate([f] * 3), np.concatenate(tests), np.concatenate([R] * 3), np.concatenate([c] * 3),
             np.arange(4) * len(v), np.arange(4) * len(f), np.concatenate([[0], np.cumsum([len(x) for x in tests])]), np.arange(4) * len(R),
             np.concatenate([tol] * 3))
    acc, dev2, worst = _check(three)
    n = len(R)
    assert len(t) + 1 > 2 * sy.limits()["block"] and not acc[:2 * n].any() and acc[2 * n:].all()
    # the identity keeps the point where it is: it is the worst point, at 5 cm
    ident = int(np.argmin(np.abs(R.reshape(-1, 9) - np.eye(3).ravel()).max(1)))
    assert worst[ident] == len(t) and worst[n + ident] == 0 and abs(np.sqrt(dev2[ident]) - 0.05) < 1e-6


def test_two_objects_with_poisoned_padding():
    """objects of different sizes in one call; rows past the last prefix entry hold NaN (faces: an index far outside), and the last block
    of every object ends within rows that belong to the next: nothing of that may be read"""
    _, args = _args_of({"cylinder_32": sy.meshes()["cylinder_32"], "tetrahedron": sy.meshes()["tetrahedron"]}, 200)
    want = _check(args)
    v, f, t, R, c, vo, fo, to, co, tol = args
    nan = lambda n, w: np.full((n, w), np.nan, np.float32)   # noqa: E731
    padded = (np.concatenate([v, nan(300, 3)]), np.concatenate([f, np.full((70, 3), 1 << 30, np.int32)]), np.concatenate([t, nan(300, 3)]),
              np.concatenate([R.reshape(-1, 9), nan(5, 9)]), c, vo, fo, to, co, tol)
    for mode in (0, 1):
        acc, dev2, worst = _gpu(padded, mode)
        n = int(co[-1])
        np.testing.assert_array_equal(acc[:n], want[0])
        keep = want[0] > 0 if mode == 0 else np.ones(n, bool)
        np.testing.assert_array_equal(_bits(dev2[:n][keep]), _bits(want[1][keep]))
        np.testing.assert_array_equal(worst[:n][keep], want[2][keep])
        assert not acc[n:].any() and np.isnan(dev2[n:]).all() and (worst[n:] == -1).all()     # rows of no candidate are left alone


def test_bad_arguments_are_refused():
    from megapose6d_amd import engine as eng

    _, args = _args_of({"cube": sy.meshes()["cube"]}, 8)
    v, f, t, R, c, vo, fo, to, co, tol = args
    bad_face = f.copy()
    bad_face[3, 2] = len(v)
    for change in (dict(f=bad_face), dict(tol=[np.nan]), dict(tol=[np.inf]), dict(tol=[-1.0]), dict(fo=[0, 0]), dict(vo=[0, 0]), dict(to=[0, 0]),
                   dict(tile=96), dict(tile=1024), dict(mode=2)):
        a = dict(v=v, f=f, t=t, R=R, c=c, vo=vo, fo=fo, to=to, co=co, tol=tol, mode=0, tile=0)
        a.update(change)
        with pytest.raises(eng.EngineError):
            _gpu(tuple(a[k] for k in ("v", "f", "t", "R", "c", "vo", "fo", "to", "co", "tol")), a["mode"], a["tile"])
    too_many = np.zeros((sy.limits()["max_candidates"] + 1, 9), np.float32)
    with pytest.raises(eng.EngineError):
        _gpu((v, f, t, too_many, c, vo, fo, to, [0, len(too_many)], tol), 0)


@pytest.fixture(scope="module")
def found_on_device(tmp_path_factory):
    from megapose6d_amd import evaluation as ev

    db = sy.mesh_database({n: sy.meshes()[n] for n in sy.ORDERS}, tmp_path_factory.mktemp("symmetry_meshes"))
    return db, ev.find_symmetries(db, rel_tol=sy.REL_TOL, n_samples=sy.N_SAMPLES)


def test_find_symmetries_end_to_end(found_on_device):
    from megapose6d_amd import evaluation as ev

    _, table = found_on_device
    assert table["n_symmetries"].to_dict() == sy.ORDERS and (table["status"] == "ok").all()
    want, _ = sy.found()
    assert table["n_candidates"].to_dict() == want["n_candidates"].to_dict()
    cyl = table.loc["cylinder_32"]
    assert len(cyl["symmetries_continuous"]) == 1 and len(cyl["symmetries_discrete"]) == 1
    np.testing.assert_allclose(cyl["symmetries_continuous"][0]["axis"], [0.0, 0.0, 1.0], atol=1e-6)
    np.testing.assert_allclose(cyl["symmetries_continuous"][0]["offset"], 0.0, atol=1e-9)
    T = cyl["symmetries_discrete"][0]
    assert abs(np.trace(T[:3, :3]) + 1.0) < 1e-6 and abs(ev._axis_angle(T[:3, :3])[0][2]) < 1e-6
    assert table.loc["cone_32", "symmetries_discrete"] == [] and len(table.loc["cone_32", "symmetries_continuous"]) == 1
    assert len(table.loc["hex_prism", "symmetries_discrete"]) == 11 and table.loc["hex_prism", "symmetries_continuous"] == []
    assert (table["deviation"] < 1e-5).all()


def test_quarter_turn_of_the_cube_is_correct_under_the_found_set(found_on_device):
    from megapose6d_amd import evaluation as ev
    from megapose6d_amd.mesh_db import with_symmetries
    from megapose6d_amd.tcoll import PandasTensorCollection

    db, table = found_on_device
    plain = db.batched().cuda()
    assert plain.infos["cube"]["n_sym"] == 1
    found = with_symmetries(plain, {l: ev.symmetry_poses(table.loc[l]) for l in ("cube", "hex_prism")})
    assert found.infos["cube"]["n_sym"] == 24 and found.infos["hex_prism"]["n_sym"] == 12 and found.infos["cone_32"]["n_sym"] == 1
    assert found.symmetries.is_cuda and found.symmetries.shape[:2] == (len(sy.ORDERS), 24)
    T_gt = pes.pose(pes.random_rotation(np.random.RandomState(4)), [0.05, -0.1, 0.8])
    T_pred = T_gt @ pes.pose(pes.axis_rotation(2, np.pi / 2), [0.0, 0.0, 0.0])
    infos = pd.DataFrame(dict(label=["cube"], scene_id=0, view_id=0, instance_id=0))
    pred = PandasTensorCollection(infos.copy(), poses=torch.from_numpy(T_pred[None].astype(np.float32)).cuda())
    gt = PandasTensorCollection(infos.copy(), poses=torch.from_numpy(T_gt[None].astype(np.float32)).cuda())
    with_set, without = ev.pose_errors(pred, gt, found), ev.pose_errors(pred, gt, plain)
    beta = pes.beta(T_pred, T_gt, points=sy.meshes()["cube"][0], symmetries=found.symmetries.cpu().numpy())
    assert with_set["mssd"][0] <= beta and with_set["add_sym"][0] <= beta and with_set["sym_id"][0] > 0
    assert 0.19 <= without["mssd"][0] <= 0.21 and without["sym_id"][0] == 0
