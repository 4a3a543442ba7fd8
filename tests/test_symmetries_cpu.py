"""CPU: object symmetry sets (megapose6d_amd.symmetries, RigidObject.make_symmetry_poses, MeshDataBase.batched) against the reference's
own make_symmetries_poses, recorded in tests/golden/pose_errors.npz by scripts/make_pose_error_golden.py (float64 on both sides, the
same formulas: agreement <= 1e-12)."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from megapose6d_amd.mesh_db import MeshDataBase
from megapose6d_amd.object_dataset import RigidObject
from megapose6d_amd.symmetries import ContinuousSymmetry, DiscreteSymmetry, make_symmetries_poses

GOLDEN = Path(__file__).resolve().parent / "golden" / "pose_errors.npz"
TOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _cases(golden):
    return json.loads(str(golden["meta"]))


def _inputs(golden, name):
    disc = [DiscreteSymmetry(pose=np.array(M)) for M in golden[f"sym_{name}_discrete"]]
    cont = [ContinuousSymmetry(offset=np.zeros(3), axis=np.array(a)) for a in golden[f"sym_{name}_continuous"]]
    return disc, cont


def test_the_fixture_covers_the_cases_and_holds_data_only(golden):
    names = set(_cases(golden))
    assert {"none", "discrete_mm", "discrete_m", "discrete_scale", "continuous_x_1", "continuous_y_8", "continuous_z_64", "both_z_4"} <= names
    assert "euler2quat" in str(golden["notes"])
    assert GOLDEN.stat().st_size < 1 << 20
    assert golden["dist_points"].shape[0] <= 8 and golden["dist_points"].shape[1] <= 512 and golden["dist_T_gt_possible"].shape[1] <= 16


@pytest.mark.parametrize("name", ["none", "discrete_mm", "discrete_m", "discrete_scale", "continuous_x_1", "continuous_y_8", "continuous_z_64",
                                  "continuous_x_8", "both_z_4", "both_scale"])
def test_make_symmetries_poses_matches_the_reference(golden, name):
    meta = _cases(golden)[name]
    disc, cont = _inputs(golden, name)
    before = [d.pose.copy() for d in disc]
    got = make_symmetries_poses(disc, cont, n_symmetries_continuous=meta["n"], units=meta["units"], scale=meta["scale"])
    want = golden[f"sym_{name}"]
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.abs(got - want).max() <= TOL
    assert np.array_equal(got[0], np.eye(4))   # identity first
    # the reference scales the discrete poses in place, so its second call differs; this one returns the first answer again
    again = make_symmetries_poses(disc, cont, n_symmetries_continuous=meta["n"], units=meta["units"], scale=meta["scale"])
    assert np.array_equal(again, got)
    assert all(np.array_equal(d.pose, b) for d, b in zip(disc, before))


def test_order_of_the_product_is_continuous_inside_discrete(golden):
    meta = _cases(golden)["both_z_4"]
    disc, cont = _inputs(golden, "both_z_4")
    got = make_symmetries_poses(disc, cont, n_symmetries_continuous=meta["n"], units=meta["units"], scale=meta["scale"])
    n = meta["n"]
    assert got.shape[0] == (1 + len(disc)) * n
    only_c = make_symmetries_poses([], cont, n_symmetries_continuous=n)
    only_d = make_symmetries_poses(disc, [], units=meta["units"])
    for d in range(1 + len(disc)):
        for c in range(n):
            assert np.abs(got[d * n + c] - only_c[c] @ only_d[d]).max() <= TOL


def test_asserts_and_unsupported_axes():
    with pytest.raises(AssertionError):
        make_symmetries_poses([], [ContinuousSymmetry(offset=np.array([0.0, 0.0, 1.0]), axis=np.array([0, 0, 1]))])
    with pytest.raises(AssertionError):
        make_symmetries_poses([], [ContinuousSymmetry(offset=np.zeros(3), axis=np.array([0, 0, 2]))])
    with pytest.raises(NotImplementedError):
        make_symmetries_poses([], [ContinuousSymmetry(offset=np.zeros(3), axis=np.array([0.5, 0.5, 0.0]))])
    with pytest.raises(KeyError):
        make_symmetries_poses([], [], units="cm")


def _write_ply(path, vertices):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\n")
        f.write(f"element vertex {len(vertices)}\nproperty float x\nproperty float y\nproperty float z\n")
        f.write("element face 1\nproperty list uchar int vertex_indices\nend_header\n")
        for v in vertices:
            f.write(f"{v[0]} {v[1]} {v[2]}\n")
        f.write("3 0 1 2\n")


def test_rigid_object_and_batched_carry_the_symmetry_sets(golden, tmp_path):
    rng = np.random.RandomState(0)
    specs = {"plain": ("none", 5), "half": ("discrete_mm", 9), "lathe": ("continuous_z_64", 7), "mixed": ("both_z_4", 4)}
    objs = []
    for label, (case, n_v) in specs.items():
        path = tmp_path / f"{label}.ply"
        _write_ply(path, rng.uniform(-50, 50, size=(n_v, 3)))
        disc, cont = _inputs(golden, case)
        objs.append(RigidObject(label, path, mesh_units="mm", symmetries_discrete=disc, symmetries_continuous=cont))
    # RigidObject.make_symmetry_poses = make_symmetries_poses(..., scale=self.scale); mm -> the golden of the "mm" cases
    for o, (case, _) in zip(objs, specs.values()):
        n = _cases(golden)[case]["n"]
        got = o.make_symmetry_poses(n_symmetries_continuous=n)
        assert np.abs(got - golden[f"sym_{case}"]).max() <= TOL
    assert objs[0].make_symmetry_poses().shape == (1, 4, 4) and not objs[0].is_symmetric
    assert objs[2].make_symmetry_poses().shape == (64, 4, 4)   # default n_symmetries_continuous = 64

    db = MeshDataBase(objs)
    meshes = db.batched(n_sym=4)
    want = {"plain": golden["sym_none"], "half": golden["sym_discrete_mm"], "mixed": golden["sym_both_z_4"]}
    assert meshes.n_sym_mapping == {"plain": 1, "half": 2, "lathe": 4, "mixed": 12}
    assert meshes.symmetries.shape == (4, 12, 4, 4) and meshes.symmetries.dtype == torch.float32
    for label, w in want.items():
        i = meshes.label_to_id[label]
        assert meshes.infos[label]["n_sym"] == len(w)
        assert torch.equal(meshes.symmetries[i, : len(w)], torch.as_tensor(w).float())
        assert torch.equal(meshes.symmetries[i, len(w):], torch.eye(4).expand(12 - len(w), 4, 4))   # identity padding
    assert meshes.points.shape == (4, 9, 3) and meshes.infos["plain"]["n_points"] == 5
    sel = meshes.select(["mixed", "plain"])
    assert sel.symmetries.shape == (2, 12, 4, 4)
    with pytest.raises(NotImplementedError):
        db.batched(aabb=True)
    with pytest.raises(NotImplementedError):
        db.batched(resample_n_points=100)

    # objects without symmetries: what batched() gave before
    plain = MeshDataBase([objs[0]]).batched()
    assert plain.symmetries.shape == (1, 1, 4, 4) and torch.equal(plain.symmetries[0, 0], torch.eye(4)) and plain.infos["plain"]["n_sym"] == 1
