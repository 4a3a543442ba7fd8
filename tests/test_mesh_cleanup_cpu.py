"""megapose6d_amd.mesh_cleanup without a device: grid_for, the dict plumbing (on the host emulation as the backend), simplify_object
refusing a textured mesh, and the PLY round trip of a simplified mesh."""
from __future__ import annotations

import numpy as np
import pytest

from megapose6d_amd import RigidObject, mesh_io
from megapose6d_amd import mesh_cleanup as mc
from tests.support import mesh_cleanup as sm

F32 = np.float32


def test_grid_for():
    m = sm.mesh([[0.0, 0.0, 0.0], [1.0, 0.5, 0.25], [np.nan, 7.0, 7.0], [0.5, np.inf, 0.1]], [[0, 1, 2]])
    be = sm.EmulBackend()
    origin, cell, dims = mc.grid_for(m, 4, backend=be)                  # the two vertices with a non-finite coordinate do not count
    assert origin == (0.0, 0.0, 0.0) and cell == 0.25 and dims == (5, 3, 2)        # floor(extent / cell) + 1: the farthest vertex included
    assert mc.grid_for(m, 1, backend=be) == ((0.0, 0.0, 0.0), 1.0, (2, 1, 1))
    assert mc.grid_for(m, 1024, backend=be)[2] == (512, 512, 257)       # 1025 and 513 clipped to the limit
    s = sm.sphere()
    for cells in (1, 7, 100, 511):
        origin, cell, dims = mc.grid_for(s, cells, backend=be)
        lo, hi = s["vertices"].min(0), s["vertices"].max(0)
        assert origin == tuple(float(v) for v in lo) and cell == float(F32((hi - lo).max()) / F32(cells))
        assert max(dims) in (cells, cells + 1) and max(dims) <= 512
        rc, totals = sm.emul_cluster_count(s, origin, cell, dims)
        assert rc == 0 and totals[2] == 0                               # no vertex falls outside the grid
    with pytest.raises(ValueError, match="at least 1"):
        mc.grid_for(m, 0, backend=be)
    with pytest.raises(ValueError, match="no vertex with finite"):
        mc.grid_for(sm.mesh([[np.nan, 0, 0]], np.zeros((0, 3))), 4, backend=be)
    with pytest.raises(ValueError, match="span no length"):
        mc.grid_for(sm.mesh([[1, 2, 3], [1, 2, 3]], np.zeros((0, 3))), 4, backend=be)


def test_dict_plumbing():
    m = sm.scene()
    be = sm.EmulBackend()
    as_lists = dict(vertices=m["vertices"].astype(np.float64).tolist(), faces=m["faces"].tolist(), colors=None, normals="ignored")
    out = mc.keep_components(as_lists, backend=be)
    assert set(out) == {"vertices", "faces", "colors"} and out["colors"] is None
    assert out["vertices"].dtype == F32 and out["faces"].dtype == np.int32 and len(out["faces"]) == sm.sphere().F
    with pytest.raises(ValueError, match="nothing to do"):
        mc.keep_components(m, largest=False, backend=be)
    both = mc.keep_components(m, largest=True, min_faces=sm.sphere().F + 1, backend=be)      # the largest is not large enough
    assert len(both["faces"]) == 0 and len(both["vertices"]) == 0
    assert mc.clean_mesh(m, keep_largest=False, max_faces=None, backend=be) is m
    host = mc.to_host(mc.clean_mesh(m, max_faces=3000, backend=be))
    assert set(host) == {"vertices", "faces", "colors", "normals"} and 0 < len(host["faces"]) <= 3000
    assert host["normals"].dtype == F32 and np.allclose(np.linalg.norm(host["normals"], axis=1), 1.0, atol=1e-5)
    centre = host["vertices"].mean(0)
    assert (np.einsum("ij,ij->i", host["normals"], host["vertices"] - centre) > 0).mean() > 0.99     # still wound outwards
    with pytest.raises(ValueError, match="cell_size"):
        mc.simplify(m, cell_size=-1.0, backend=be)
    with pytest.raises(ValueError, match="at most 512 a side"):
        mc.simplify(m, cell_size=1e-5, backend=be)
    with pytest.raises(ValueError, match="max_faces 0 must be"):
        mc.simplify(m, max_faces=0, backend=be)


def test_simplify_object_and_the_ply_round_trip(tmp_path):
    s = sm.sphere()
    normals = mesh_io.vertex_normals(s["vertices"], s["faces"])
    path = mesh_io.write_ply(tmp_path / "scan.ply", s["vertices"] * 1000.0, s["faces"], colors=s["colors"], normals=normals)
    obj = RigidObject("scan", path, mesh_units="mm", symmetries_discrete=[np.eye(4).tolist()], ypr_offset_deg=(10.0, 0.0, 0.0))
    light = mc.simplify_object(obj, 2000, tmp_path / "light", backend=sm.EmulBackend())
    assert light.label == "scan" and str(light.mesh_path).endswith("light/scan.ply") and light.mesh_units == "mm" and light.scale == obj.scale
    assert light.symmetries_discrete == obj.symmetries_discrete and tuple(light.ypr_offset_deg) == (10.0, 0.0, 0.0)
    back = mesh_io.read_ply(light.mesh_path)
    raw = mesh_io.read_ply(path)
    want = mc.to_host(mc.simplify(dict(vertices=raw["vertices"], faces=raw["faces"], colors=raw["colors"]), max_faces=2000, backend=sm.EmulBackend()))
    assert 0 < len(back["faces"]) <= 2000
    assert np.array_equal(back["vertices"].astype(F32), want["vertices"]) and np.array_equal(back["faces"], want["faces"])
    assert np.array_equal(back["normals"].astype(F32), want["normals"])
    assert np.abs(back["colors"] - want["colors"]).max() <= 0.5 / 255 + 1e-6
    rep = sm.edge_balance(back["faces"], len(back["vertices"]))
    assert rep["balanced"] and rep["unreferenced"] == 0
    loaded = mesh_io.load_rigid_object(light)                           # what the renderer and MeshDataBase read
    assert loaded["vertices"].shape == (len(back["vertices"]), 3) and np.abs(loaded["points"]).max() < 0.06
    with pytest.raises(ValueError, match=r"simplify_object\('scan'\): simplify: no face is left"):
        mc.simplify_object(obj, 3, tmp_path / "light", backend=sm.EmulBackend())


def test_simplify_object_refuses_a_textured_mesh(tmp_path):
    (tmp_path / "tex.mtl").write_text("newmtl m\nmap_Kd tex.png\n")
    (tmp_path / "tex.obj").write_text("mtllib tex.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl m\nf 1/1 2/2 3/3\n")
    assert mesh_io.load_mesh_file(tmp_path / "tex.obj")["uvs"] is not None
    with pytest.raises(ValueError, match="texture coordinates"):
        mc.simplify_object(RigidObject("tex", tmp_path / "tex.obj"), 100, tmp_path / "out", backend=sm.EmulBackend())
    assert not (tmp_path / "out").exists()
