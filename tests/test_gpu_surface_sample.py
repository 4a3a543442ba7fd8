"""GPU: the surface-sampling kernels (csrc/surface_sample.hip) through the C ABI against the host emulation built from the same rules
header (tests/surface_sample_emul.cpp): points bit for bit and faces exactly, on every mesh of tests/support/surface_sample.py at
every count and every block (0 = the library's choice, one job per 2048 faces; 64, 128, 256 = several blocks at a few hundred faces,
so both levels of the search), one object per launch and several, failed objects included; bad arguments are refused before any launch;
`MeshDataBase.batched_surface` (shape, seed, on the surface, the point-cloud branch, a failed object); `pose_errors`, `summary` and
`model_info` on its result; and on a unit cube what the feature is for: ADD on the surface against ADD on the eight vertices."""
import numpy as np
import pandas as pd
import pytest
import torch

from support import pose_error as pes
from support import surface_sample as ss

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gpu(packed, u, block):
    from megapose6d_amd import engine as eng

    v, f, vo, fo = packed
    points, face = eng.surface_sample(torch.tensor(v, dtype=torch.float32).cuda(), torch.tensor(f, dtype=torch.int32).cuda(), vo, fo,
                                      torch.tensor(u, dtype=torch.float32).cuda(), block=block)
    assert points.dtype == torch.float32 and face.dtype == torch.int32
    return points.cpu().numpy(), face.cpu().numpy()


@pytest.mark.parametrize("block", ss.BLOCKS)
def test_kernel_matches_the_emulation_on_every_mesh(block):
    for name, mesh in ss.meshes().items():
        for count in ss.COUNTS:
            want_points, want_face = ss.emul_case(name, count, block)
            points, face = _gpu(ss.pack([mesh]), ss.case_uniforms(name, count)[None], block)
            assert points.shape == (1, count, 3) and face.shape == (1, count)
            assert np.array_equal(face[0], want_face), (name, count, block, int((face[0] != want_face).sum()))
            assert np.array_equal(_bits(points[0]), _bits(want_points)), (name, count, block)
            if name in ss.FAILED:
                assert np.isnan(points).all() and (face == -1).all()


@pytest.mark.parametrize("block", ss.BLOCKS)
def test_several_objects_in_one_launch(block):
    for count in ss.COUNTS:
        packed, u, (want_points, want_face) = ss.multi_case(count, block)
        points, face = _gpu(packed, u, block)
        assert np.array_equal(face, want_face) and np.array_equal(_bits(points), _bits(want_points)), (count, block)
        for o, name in enumerate(ss.MULTI):
            assert np.isnan(points[o]).all() == (name in ss.FAILED) and (face[o] == -1).all() == (name in ss.FAILED)


def test_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import engine as eng

    v, f = (torch.tensor(a).cuda() for a in ss.meshes()["cube"])
    u = torch.zeros(1, 4, 3, device="cuda")
    for vert_off, face_off, block in (([0, 8], [0, 12], 32), ([0, 8], [0, 12], 96), ([0, 8], [0, 12], 4096), ([0, 8], [0, 11], 0), ([0, 7], [0, 12], 0),
                                      ([1, 8], [0, 12], 0), ([0, 8], [0, 12, 12], 0), ([0, 8], [12, 12], 0)):
        with pytest.raises(eng.EngineError):
            eng.surface_sample(v, f, vert_off, face_off, u, block=block)
    two = torch.zeros(2, 4, 3, device="cuda")
    for vert_off, face_off in (([0, 8, 8], [0, 12, 12]), ([0, 9, 8], [0, 6, 12]), ([0, 4, 8], [0, 6])):
        with pytest.raises(eng.EngineError):
            eng.surface_sample(v, f, vert_off, face_off, two)
    for bad_u in (torch.zeros(1, 0, 3, device="cuda"), torch.zeros(1, 4, 2, device="cuda"), torch.zeros(4, 3, device="cuda")):
        with pytest.raises(eng.EngineError):
            eng.surface_sample(v, f, [0, 8], [0, 12], bad_u)
    lib = eng._lib.load()
    h = np.asarray([0, 12, 24], np.int32)
    assert lib.mp_surface_sample_scratch_bytes(2, h.ctypes.data, 1, 0) > 0
    for n_obj, off, count, block in ((0, h, 1, 0), (2, h, 0, 0), (2, h, 1, 65), (2, np.asarray([0, 12, 12], np.int32), 1, 0),
                                     (1, np.asarray([0, (1 << 22) + 1], np.int32), 1, 0), (1, np.asarray([0, 64 * 2048 + 1], np.int32), 1, 64)):
        assert lib.mp_surface_sample_scratch_bytes(n_obj, off.ctypes.data, count, block) == 0
    # the C entry itself: offsets that descend, an empty object and a bad block return an error code, nothing is launched
    points, face = torch.empty(2, 4, 3, device="cuda"), torch.empty(2, 4, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    d = torch.zeros(3, dtype=torch.int32, device="cuda")
    for vo, fo, count, block in (([0, 8, 4], [0, 6, 12], 4, 0), ([0, 8, 8], [0, 12, 12], 4, 0), ([0, 8, 8], [0, 6, 12], 4, 100), ([0, 8, 8], [0, 6, 12], 0, 0)):
        hv, hf = np.asarray(vo, np.int32), np.asarray(fo, np.int32)
        rc = lib.mp_surface_sample(v.data_ptr(), f.data_ptr(), d.data_ptr(), d.data_ptr(), hv.ctypes.data, hf.ctypes.data, 2, two.data_ptr(), count, block,
                                   ws.data_ptr(), points.data_ptr(), face.data_ptr(), eng._stream())
        assert rc != 0, (vo, fo, count, block)


# the mesh database ----------------------------------------------------------------------------------------------------------------------
def _write_cloud(path, vertices):
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(vertices)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        for v in vertices:
            f.write(f"{float(v[0])!r} {float(v[1])!r} {float(v[2])!r}\n")


@pytest.fixture(scope="module")
def database(tmp_path_factory):
    """two lathe meshes and one point cloud between them"""
    from megapose6d_amd.mesh_db import MeshDataBase
    from megapose6d_amd.object_dataset import RigidObject
    from tests.support import synthetic as syn

    d = tmp_path_factory.mktemp("surface_meshes")
    ds = syn.make_object_dataset(d, n_objects=2, seed=3, n_theta=24, n_z=21)
    _write_cloud(d / "cloud.ply", np.random.RandomState(1).uniform(-40, 40, size=(700, 3)))
    objs = [ds[0], RigidObject("cloud", d / "cloud.ply", mesh_units="mm"), ds[1]]
    return d, MeshDataBase(objs)


def test_batched_surface(database):
    from megapose6d_amd import engine as eng
    from megapose6d_amd.mesh_db import MeshDataBase, deterministic_point_ids
    from megapose6d_amd.object_dataset import RigidObject
    from tests.support import synthetic as syn

    d, db = database
    n = 500
    got = db.batched_surface(n, n_sym=4)
    assert got.points.shape == (3, n, 3) and got.points.dtype == torch.float32 and not got.points.is_cuda
    assert list(got.labels) == db.labels and all(got.infos[l]["n_points"] == n for l in db.labels)
    assert torch.equal(got.symmetries, db.batched(n_sym=4).symmetries)
    again, other = db.batched_surface(n, n_sym=4), db.batched_surface(n, n_sym=4, seed=1)
    assert torch.equal(again.points, got.points)
    assert not torch.equal(other.points[0], got.points[0]) and not torch.equal(other.points[2], got.points[2])
    cloud = db.engine_meshes["cloud"]["points"]
    assert np.array_equal(got.points[1].numpy(), cloud[deterministic_point_ids(len(cloud), n)]) and torch.equal(other.points[1], got.points[1])
    # on the surface: the same uniforms through engine.surface_sample name the faces
    meshed = [l for l in db.labels if l != "cloud"]
    u = torch.rand(2, n, 3, generator=torch.Generator().manual_seed(0))
    packed = ss.pack([(db.engine_meshes[l]["points"], db.engine_meshes[l]["faces"]) for l in meshed])
    points, face = _gpu(packed, u.numpy(), 0)
    for k, l in enumerate(meshed):
        v, f = db.engine_meshes[l]["points"], db.engine_meshes[l]["faces"]
        assert np.array_equal(_bits(points[k]), _bits(got.points[db.labels.index(l)].numpy()))
        _, _, dist, beyond = ss.on_face(v, f, points[k], face[k])
        print(f"{l}: plane distance / extent {dist / ss.extent(v):.3e}, beyond an edge / extent {beyond / ss.extent(v):.3e}")
        assert dist <= ss.ON_FACE * ss.extent(v) and beyond <= ss.ON_FACE * ss.extent(v)
        assert len(np.unique(face[k])) > 200                                       # spread over the mesh, not a few faces
    with pytest.raises(AssertionError):
        db.batched_surface(701)                                                    # the cloud has 700 vertices
    # a failed object raises and is named
    v, f, c = syn.make_lathe_mesh(5, n_theta=12, n_z=9)
    v = v.astype(np.float32).copy()
    v[17, 2] = np.nan
    syn.write_ply(d / "broken.ply", v, f, c)
    broken = MeshDataBase([db.obj_list[0], RigidObject("broken", d / "broken.ply", mesh_units="mm")])
    with pytest.raises(ValueError, match="broken"):
        broken.batched_surface(64)


def _collections(labels, T_pred, T_gt):
    from megapose6d_amd.tcoll import PandasTensorCollection

    infos = pd.DataFrame(dict(label=list(labels), batch_im_id=list(range(len(labels)))))
    return (PandasTensorCollection(infos.assign(score=1.0), poses=torch.from_numpy(T_pred.astype(np.float32)).cuda()),
            PandasTensorCollection(infos.copy(), poses=torch.from_numpy(T_gt.astype(np.float32)).cuda()))


def test_pose_errors_summary_and_model_info_run_on_a_surface_database(database):
    from megapose6d_amd import evaluation as ev
    from tests.support import synthetic as syn

    _, db = database
    meshes = db.batched_surface(300, n_sym=4).cuda()
    rng = np.random.RandomState(2)
    labels = [db.labels[k % 3] for k in range(6)]
    T_gt = np.stack([pes.pose(pes.random_rotation(rng), [0.0, 0.0, 0.6]) for _ in labels])
    T_pred = T_gt.copy()
    T_pred[:, :3, 3] += rng.uniform(-0.004, 0.004, size=(6, 3))
    pred, gt = _collections(labels, T_pred, T_gt)
    K = torch.from_numpy(np.repeat(syn.K_EXAMPLE[None], 6, 0).astype(np.float32)).cuda()
    df = ev.pose_errors(pred, gt, meshes, K=K)
    assert len(df) == 6 and np.isfinite(df[["add", "add_sym", "mssd", "adds", "proj_error", "diameter"]].to_numpy()).all()
    shift = np.linalg.norm(T_pred[:, :3, 3] - T_gt[:, :3, 3], axis=1)
    assert np.abs(df["add"].to_numpy() - shift).max() <= 1e-6 and (df["adds"].to_numpy() <= df["add"].to_numpy() + 1e-7).all()
    s = ev.summary(df)
    assert set(s) == {"add0.1d", "5deg_5cm", "proj2d_5px"} and s["add0.1d"] == 1.0
    info = ev.model_info(meshes)
    pts = meshes.points.cpu().numpy().astype(np.float64)
    for o, label in enumerate(meshes.labels):
        assert 0 <= info.loc[label, "pt_i"] <= info.loc[label, "pt_j"] < 300
        want = max(float(np.linalg.norm(pts[o, r] - pts[o], axis=1).max()) for r in range(300))
        assert abs(info.loc[label, "diameter"] - want) <= 1e-6 * want


def test_add_on_a_unit_cube_surface_against_its_vertices(tmp_path):
    """The eight vertices of a cube sit at its extremes; its surface does not.  A pure translation moves every point alike, so both
    databases give its length; a rotation about a diagonal moves the vertices further than the surface, so the vertex ADD is the
    larger: an error of the tessellation, which the surface database does not have."""
    from megapose6d_amd import evaluation as ev
    from megapose6d_amd.mesh_db import MeshDataBase
    from megapose6d_amd.object_dataset import RigidObject
    from tests.support import synthetic as syn

    v, f = ss.meshes()["cube"]
    syn.write_ply(tmp_path / "cube.ply", v, f)
    db = MeshDataBase([RigidObject("cube", tmp_path / "cube.ply", mesh_units="m")])
    by_vertex, by_surface = db.batched().cuda(), db.batched_surface(4096).cuda()
    assert by_vertex.points.shape == (1, 8, 3) and by_surface.points.shape == (1, 4096, 3)
    p = by_surface.points[0].cpu().numpy()
    assert p.min() >= 0.0 and p.max() <= 1.0 and (np.isin(p, (0.0, 1.0)).sum(1) >= 1).all()      # every point on one of the six sides
    rng = np.random.RandomState(6)
    T_gt = pes.pose(pes.random_rotation(rng), [0.05, -0.02, 1.5])
    t = np.asarray([0.03, -0.04, 0.12])
    moved = T_gt.copy()
    moved[:3, 3] += t
    angle, axis = np.deg2rad(20.0), np.ones(3) / np.sqrt(3.0)
    Kx = np.asarray([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    turn = np.eye(4)
    turn[:3, :3] = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx          # about the diagonal through vertex 0 and vertex 7
    turned = T_gt @ turn
    pred, gt = _collections(["cube", "cube"], np.stack([moved, turned]), np.stack([T_gt, T_gt]))
    add = {k: ev.pose_errors(pred, gt, m, nearest=False)["add"].to_numpy() for k, m in (("vertex", by_vertex), ("surface", by_surface))}
    print("add:", add)
    for k, m in (("vertex", by_vertex), ("surface", by_surface)):
        assert abs(add[k][0] - np.linalg.norm(t)) <= 1e-6
        x = m.points[0].cpu().numpy().astype(np.float64)
        want = np.linalg.norm(x @ (turned[:3, :3] - T_gt[:3, :3]).T + (turned[:3, 3] - T_gt[:3, 3]), axis=1).mean()
        assert abs(add[k][1] - want) <= 1e-6
    # vertices: six of eight at sqrt(2/3) from the axis, two on it -> 2 sin(10 deg) * 0.75 * sqrt(2/3) = 0.2127; the surface is closer
    assert abs(add["vertex"][1] - 2.0 * np.sin(angle / 2.0) * 0.75 * np.sqrt(2.0 / 3.0)) <= 1e-6
    assert add["vertex"][1] > 1.1 * add["surface"][1]
