"""CPU: the host logic of MeshDataBase.batched_aabb and of the point-cloud branch of MeshDataBase.batched_surface (neither needs the
library), and batched() itself, which keeps refusing the reference's two keywords."""
import numpy as np
import pytest
import torch

from megapose6d_amd.mesh_db import MeshDataBase, deterministic_point_ids
from megapose6d_amd.object_dataset import RigidObject
from megapose6d_amd.symmetries import ContinuousSymmetry


def _write_ply(path, vertices, faces=()):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\n")
        f.write(f"element vertex {len(vertices)}\nproperty float x\nproperty float y\nproperty float z\n")
        f.write(f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
        for v in vertices:
            f.write(f"{float(v[0])!r} {float(v[1])!r} {float(v[2])!r}\n")
        for t in faces:
            f.write(f"3 {t[0]} {t[1]} {t[2]}\n")


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    d = tmp_path_factory.mktemp("surface_db")
    rng = np.random.RandomState(0)
    clouds = {"cloud_a": rng.uniform(-50, 50, size=(40, 3)), "cloud_b": rng.uniform(-20, 90, size=(25, 3))}
    objs = []
    for label, v in clouds.items():
        _write_ply(d / f"{label}.ply", v)
        sym = [ContinuousSymmetry(offset=np.zeros(3), axis=np.array([0, 0, 1]))] if label == "cloud_b" else []
        objs.append(RigidObject(label, d / f"{label}.ply", mesh_units="mm", symmetries_continuous=sym))
    return MeshDataBase(objs)


def test_batched_aabb_corner_order_and_values(db):
    boxes = db.batched_aabb(n_sym=4)
    assert boxes.points.shape == (2, 8, 3) and boxes.points.dtype == torch.float32 and not boxes.points.is_cuda
    assert list(boxes.labels) == db.labels and boxes.infos == {"cloud_a": {"n_points": 8, "n_sym": 1}, "cloud_b": {"n_points": 8, "n_sym": 4}}
    plain = db.batched(n_sym=4)
    assert torch.equal(boxes.symmetries, plain.symmetries) and boxes.n_sym_mapping == plain.n_sym_mapping
    for n, label in enumerate(db.labels):
        p = db.engine_meshes[label]["points"]
        assert p.dtype == np.float32
        (x0, y0, z0), (x1, y1, z1) = p.min(0), p.max(0)
        # lib3d/mesh_ops.py get_meshes_bounding_boxes: v0 = (xmin, ymax, zmax) ... v7 = (xmin, ymin, zmin)
        want = np.asarray([[x0, y1, z1], [x1, y1, z1], [x1, y0, z1], [x0, y0, z1], [x0, y1, z0], [x1, y1, z0], [x1, y0, z0], [x0, y0, z0]], np.float32)
        assert np.array_equal(boxes.points[n].numpy(), want)
        assert np.array_equal(boxes.points[n].numpy().min(0), p.min(0)) and np.array_equal(boxes.points[n].numpy().max(0), p.max(0))


def test_point_clouds_keep_the_deterministic_subset(db):
    got = db.batched_surface(20, n_sym=4)           # no object has faces: no launch, no library
    assert got.points.shape == (2, 20, 3) and got.points.dtype == torch.float32 and not got.points.is_cuda
    assert got.infos == {"cloud_a": {"n_points": 20, "n_sym": 1}, "cloud_b": {"n_points": 20, "n_sym": 4}}
    assert torch.equal(got.symmetries, db.batched(n_sym=4).symmetries)
    for n, label in enumerate(db.labels):
        p = db.engine_meshes[label]["points"]
        assert np.array_equal(got.points[n].numpy(), p[deterministic_point_ids(len(p), 20)])
    assert torch.equal(db.batched_surface(20, n_sym=4, seed=5).points, got.points)     # nothing is drawn for a point cloud
    with pytest.raises(AssertionError):
        db.batched_surface(26)                      # cloud_b has 25 vertices
    with pytest.raises(ValueError):
        db.batched_surface(0)


def test_batched_still_refuses_both_keywords(db):
    with pytest.raises(NotImplementedError):
        db.batched(aabb=True)
    with pytest.raises(NotImplementedError):
        db.batched(resample_n_points=100)
    assert db.batched().points.shape == (2, 40, 3)
