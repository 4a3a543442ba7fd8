"""The contract of the mesh clean-up kernels (csrc/mesh_cleanup_core.h) on the CPU: the host emulation against an independent numpy
restatement bit for bit, literal worked examples, the properties that hold by theorem (a simplicial map keeps a closed mesh closed),
accuracy on the analytic sphere, the face-budget search of mesh_cleanup.simplify through the emulation, refusals, and the emulation as a
stand-alone program under the sanitizers."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from megapose6d_amd import mesh_cleanup as mc

from tests.support import mesh_cleanup as sm
from tests.support import tsdf as st

F32 = np.float32
SETTINGS = [(c, s) for c in sm.CELLS_VOXELS for s in sm.SHIFTS]


def same_bits(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_mesh(got, want):
    for k, name in enumerate(("vertices", "faces", "colors")):
        assert same_bits(got[k], want[k]), name
    assert got[3] == want[3]


def fixture(name) -> sm.Mesh:
    if name.startswith("chain_"):
        return sm.chain(name[6:])
    return getattr(sm, name)()


COMPONENT_FIXTURES = ("sphere", "torus", "scene", "chain_forward", "chain_reverse", "chain_bitrev", "star", "large")


def test_fixture_sizes():
    assert (sm.sphere().V, sm.sphere().F) == (7754, 15504) and (sm.torus().V, sm.torus().F) == (6054, 12108)
    lim = sm.limits()
    assert lim == dict(max_count=1 << 29, max_dim=512, max_cells=1 << 27)
    assert (mc.MAX_DIM, mc.MAX_CELLS) == (lim["max_dim"], lim["max_cells"])
    # the large fixture: more workgroups of the face rank pass than one round of the scan over their totals takes
    assert -(-sm.large().F // sm.RANK_SPAN) > sm.SCAN_ROUND


@pytest.mark.parametrize("name", COMPONENT_FIXTURES)
def test_components_emulation_is_the_restatement(name):
    m = fixture(name)
    got, want = sm.emul_components(m.V, m["faces"]), sm.restated_components(m.V, m["faces"])
    for g, w, what in zip(got, want, ("labels", "face_labels", "face_count", "totals")):
        assert same_bits(g, w), what


def test_components_of_the_scene():
    m = sm.scene()
    labels, flabels, fcount, totals = sm.emul_components(m.V, m["faces"])
    assert totals.tolist() == [3, sm.scene_sphere_label(), 2, 0]          # sphere, torus, tetrahedron; the largest is the sphere
    assert len(np.unique(labels)) == 3 + 3                                 # + the three vertices on no face
    for l in np.unique(labels):
        assert l == np.nonzero(labels == l)[0].min()                       # every label is its component's minimum
    assert fcount.sum() == m.F - 2 and fcount[totals[1]] == sm.sphere().F
    assert (flabels == -1).sum() == 2
    assert sorted(fcount[fcount > 0].tolist()) == [4, sm.torus().F, sm.sphere().F]


@pytest.mark.parametrize("name", ("sphere", "scene"))
@pytest.mark.parametrize("variant", ("all", "none", "third", "largest"))
def test_select_emulation_is_the_restatement(name, variant):
    m = fixture(name)
    keep = sm.keep_variants(m)[variant]
    got = sm.emul_select(m, keep)
    assert_same_mesh(got, sm.restated_select(m, keep))
    if variant == "none":
        assert len(got[0]) == 0 and len(got[1]) == 0
    if variant == "largest" and name == "scene":
        assert (len(got[0]), len(got[1])) == (sm.sphere().V, sm.sphere().F)
        rep = sm.edge_balance(got[1], len(got[0]))
        assert rep["balanced"] and rep["unreferenced"] == 0
    no_colors = sm.mesh(m["vertices"], m["faces"])
    assert_same_mesh(sm.emul_select(no_colors, keep), sm.restated_select(no_colors, keep))


@pytest.mark.parametrize("name", ("sphere", "torus", "scene"))
@pytest.mark.parametrize("cell_voxels,shift", SETTINGS)
def test_cluster_emulation_is_the_restatement(name, cell_voxels, shift):
    m = fixture(name)
    grid = sm.grid_of(m, cell_voxels, shift)
    assert_same_mesh(sm.emul_cluster(m, *grid), sm.restated_cluster(m, *grid))
    no_colors = sm.mesh(m["vertices"], m["faces"])
    assert_same_mesh(sm.emul_cluster(no_colors, *grid), sm.restated_cluster(no_colors, *grid))


def test_cluster_with_vertices_outside_the_grid():
    """a grid that holds half of the scene: vertices outside are bad, their faces are dropped and counted"""
    m = sm.scene()
    origin, cell, dims = sm.grid_of(m, 2.0, 0.37)
    dims = (dims[0] // 2, dims[1], dims[2])                          # the cut runs through the sphere
    got = sm.emul_cluster(m, origin, cell, dims)
    assert_same_mesh(got, sm.restated_cluster(m, origin, cell, dims))
    assert got[3] > 2 and len(got[1]) > 0


# literal worked examples ------------------------------------------------------------------------------------------------------------------
TETRA_FACES = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]
OCTA = np.array([[1.5, 1.5, 0.5], [1.5, 0.5, 1.5], [0.5, 1.5, 1.5], [2.5, 1.5, 1.5], [1.5, 2.5, 1.5], [1.5, 1.5, 2.5]], F32)   # cells 4 10 12 14 16 22
OCTA_FACES = np.array([[5, 3, 4], [5, 4, 2], [5, 2, 1], [5, 1, 3], [0, 4, 3], [0, 2, 4], [0, 1, 2], [0, 3, 1]], np.int32)


def test_tetrahedron_inside_one_cell_vanishes():
    m = sm.mesh([[0.1, 0.1, 0.1], [0.9, 0.1, 0.1], [0.1, 0.9, 0.1], [0.1, 0.1, 0.9]], TETRA_FACES)
    v, f, c, dropped = sm.emul_cluster(m, (0, 0, 0), 1.0, (1, 1, 1))
    assert len(v) == 0 and len(f) == 0 and c is None and dropped == 0


def test_octahedron_with_one_vertex_per_cell_is_itself():
    order = np.array([3, 5, 0, 1, 4, 2])          # input vertex of each cell-ordered output vertex: a shuffled input
    new_of_old = np.argsort(order)
    m = sm.mesh(OCTA[order], new_of_old[OCTA_FACES], colors=np.linspace(0, 1, 18).reshape(6, 3)[order])
    v, f, c, dropped = sm.emul_cluster(m, (0, 0, 0), 1.0, (3, 3, 3))
    assert dropped == 0 and np.array_equal(v, OCTA) and np.array_equal(f, OCTA_FACES)       # renumbered in cell order, corners in order
    assert np.abs(c - np.linspace(0, 1, 18).reshape(6, 3)).max() <= 0.5 / 65535 + 1e-7
    assert sm.edge_balance(f, 6)["balanced"]


def test_a_vertex_on_a_cell_boundary_goes_to_the_upper_cell():
    m = sm.mesh([[1.0, 0.25, 0.25], [0.5, 0.5, 0.5], [0.25, 1.0, 0.25]], [[0, 1, 2]])
    v, f, _, _ = sm.emul_cluster(m, (0, 0, 0), 1.0, (2, 2, 1))
    assert np.array_equal(v, [[0.5, 0.5, 0.5], [1.0, 0.25, 0.25], [0.25, 1.0, 0.25]]) and f.tolist() == [[1, 0, 2]]      # cells 0, 1, 2
    # ... and one exactly on the far side of the grid is outside it
    v, f, _, dropped = sm.emul_cluster(m, (0, 0, 0), 1.0, (1, 2, 1))
    assert len(f) == 0 and dropped == 1


def test_a_nan_vertex_drops_its_faces_and_moves_no_mean():
    base = sm.mesh(np.concatenate([OCTA, [[1.25, 1.25, 0.25]]]), OCTA_FACES)                          # a 7th vertex in cell 4, on no face
    with_nan = sm.mesh(np.concatenate([OCTA, [[1.25, 1.25, 0.25], [np.nan, 1.5, 0.5], [1.5, np.inf, 0.5]]]),
                       np.concatenate([OCTA_FACES, [[7, 3, 4], [0, 8, 2]]]))
    a, b = sm.emul_cluster(base, (0, 0, 0), 1.0, (3, 3, 3)), sm.emul_cluster(with_nan, (0, 0, 0), 1.0, (3, 3, 3))
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and (a[3], b[3]) == (0, 2)
    assert np.array_equal(a[0][0], [1.375, 1.375, 0.375])                                               # the mean takes the vertex on no face


# theorem-level properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("sphere", "torus"))
@pytest.mark.parametrize("cell_voxels,shift", SETTINGS)
def test_clustering_keeps_a_closed_mesh_closed(name, cell_voxels, shift):
    m = fixture(name)
    assert sm.edge_balance(m["faces"], m.V)["balanced"]
    v, f, c, dropped = sm.emul_cluster(m, *sm.grid_of(m, cell_voxels, shift))
    rep = sm.edge_balance(f, len(v))
    assert dropped == 0 and len(f) > 0
    assert rep["index_ok"] and rep["unreferenced"] == 0 and rep["no_loop"] and rep["balanced"], rep
    assert np.isfinite(v).all() and np.isfinite(c).all() and c.min() >= 0 and c.max() <= 1


@pytest.mark.parametrize("shift", sm.SHIFTS)
def test_accuracy_on_the_analytic_sphere(shift):
    """every output vertex within 1 voxel of the sphere, the signed volume within 5 % of the input's (cells of 2 voxels).
    Measured: aligned 609 vertices, 1218 faces, 0.5706 voxel, volume ratio 0.98498; shifted by 0.37 voxel 553 vertices, 1118 faces,
    0.5706 voxel, 0.98123."""
    m = sm.sphere()
    v, f, _, _ = sm.emul_cluster(m, *sm.grid_of(m, 2.0, shift))
    dist = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - st.SPHERE_R).max() / sm.SPHERE_VOXEL
    ratio = sm.signed_volume(v, f) / sm.signed_volume(m["vertices"], m["faces"])
    print(f"shift {shift}: {len(v)} vertices, {len(f)} faces, max distance {dist:.4f} voxel, volume ratio {ratio:.5f}")
    assert dist <= 1.0
    assert abs(ratio - 1.0) <= 0.05


# mesh_cleanup.simplify / keep_components through the emulation ------------------------------------------------------------------------------
def test_simplify_max_faces_replays_the_stated_bisection():
    m = sm.sphere()
    be = sm.EmulBackend()
    out = mc.simplify(m, max_faces=1500, backend=be)
    assert 0 < len(out["faces"]) <= 1500
    lo, hi, tested = 1, 512, []
    while hi - lo > 1:
        mid = (lo + hi) // 2
        grid = mc.grid_for(m, mid, backend=sm.EmulBackend())
        rc, totals = sm.emul_cluster_count(m, *grid)
        assert rc == 0
        tested.append((*grid, int(totals[1])))
        lo, hi = (mid, hi) if totals[1] <= 1500 else (lo, mid)
    assert len(tested) <= 9 and be.count_calls == tested
    want = sm.emul_cluster(m, *mc.grid_for(m, lo, backend=sm.EmulBackend()))
    assert same_bits(out["vertices"], want[0]) and same_bits(out["faces"], want[1]) and same_bits(out["colors"], want[2])
    # one more cell along the longest side would exceed the budget
    assert sm.emul_cluster_count(m, *mc.grid_for(m, lo + 1, backend=sm.EmulBackend()))[1][1] > 1500


def test_simplify_within_budget_and_without_a_face_left():
    m = sm.sphere()
    assert mc.simplify(m, max_faces=m.F, backend=sm.EmulBackend()) is m
    with pytest.raises(ValueError, match="no face is left at max_faces 3"):
        mc.simplify(m, max_faces=3, backend=sm.EmulBackend())              # one cell along the longest side holds the whole sphere
    with pytest.raises(ValueError, match="no face is left at cell_size 1.0"):
        mc.simplify(m, cell_size=1.0, backend=sm.EmulBackend())            # the whole sphere in one cell
    with pytest.raises(ValueError, match="exactly one"):
        mc.simplify(m, backend=sm.EmulBackend())
    by_cell = mc.simplify(m, cell_size=2 * sm.SPHERE_VOXEL, backend=sm.EmulBackend())
    want = sm.emul_cluster(m, *sm.grid_of(m, 2.0, 0.0))
    assert same_bits(by_cell["vertices"], want[0]) and same_bits(by_cell["faces"], want[1])


def test_keep_components_and_clean_mesh_through_the_emulation():
    m = sm.scene()
    out = mc.keep_components(m, backend=sm.EmulBackend())
    assert (len(out["vertices"]), len(out["faces"])) == (sm.sphere().V, sm.sphere().F)
    out = mc.keep_components(m, largest=False, min_faces=5, backend=sm.EmulBackend())
    assert len(out["faces"]) == sm.sphere().F + sm.torus().F
    cc = mc.connected_components(m, backend=sm.EmulBackend())
    assert (cc["n_components"], cc["largest"], cc["n_bad_faces"]) == (3, sm.scene_sphere_label(), 2)
    out = mc.clean_mesh(m, keep_largest=True, max_faces=2000, backend=sm.EmulBackend())
    assert 0 < len(out["faces"]) <= 2000
    assert sm.emul_components(len(out["vertices"]), out["faces"])[3][0] == 1


# refusals and limits ----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_limits():
    m = sm.mesh(OCTA, OCTA_FACES)
    ok = ((0, 0, 0), 1.0, (3, 3, 3))
    assert sm.emul_cluster_count(m, *ok)[0] == 0
    for dims in ((0, 3, 3), (3, 513, 3), (3, 3, -1), (512, 512, 513), (512, 512, 512 + 1)):
        rc, totals = sm.emul_cluster_count(m, ok[0], ok[1], dims)
        assert rc != 0 and (totals == sm.SENTINEL).all(), dims
    assert sm.emul_cluster_count(m, ok[0], ok[1], (512, 512, 512))[0] == 0                      # exactly 2^27 cells
    for cell in (0.0, -1.0, np.inf, np.nan):
        rc, totals = sm.emul_cluster_count(m, ok[0], cell, ok[2])
        assert rc != 0 and (totals == sm.SENTINEL).all(), cell
    assert sm.emul_cluster_count(m, (np.nan, 0, 0), 1.0, ok[2])[0] != 0
    # capacities below the totals
    assert sm.emul_cluster(m, *ok, caps=(5, 8)) != 0 and sm.emul_cluster(m, *ok, caps=(6, 7)) != 0 and sm.emul_cluster(m, *ok, caps=(6, 8)) == 0
    keep = np.ones(8, np.uint8)
    assert sm.emul_select(m, keep, caps=(5, 8)) != 0 and sm.emul_select(m, keep, caps=(6, 7)) != 0 and sm.emul_select(m, keep, caps=(7, 9)) == 0
    # empty inputs succeed with zero totals
    empty_f = sm.mesh(OCTA, np.zeros((0, 3), np.int32))
    empty_v = sm.mesh(np.zeros((0, 3), F32), OCTA_FACES)
    for e in (empty_f, empty_v):
        assert sm.emul_cluster(e, *ok)[3] == 0 and len(sm.emul_cluster(e, *ok)[0]) == 0
        assert sm.emul_select(e, np.ones(e.F, np.uint8))[3] == 0
        labels, flabels, fcount, totals = sm.emul_components(e.V, e["faces"])
        assert totals.tolist() == [0, -1, 0, 0] and labels.tolist() == list(range(e.V)) and (flabels == -1).all() and (fcount == 0).all()


# sanitizers -------------------------------------------------------------------------------------------------------------------------------
def test_emulation_under_the_sanitizers(tmp_path):
    """the emulation as a stand-alone program (tests/mesh_cleanup_asan_main.cpp) under the address and undefined-behaviour sanitizers, on
    arrays of exactly the call's sizes: a bad index used as an address, a vertex past the counted ones, a cell outside the grid would be
    caught here.  The program compares every call with what the plain build returned."""
    n_calls = 0

    def write(fh, op, m, grid, keep, results, nv, nf):
        nonlocal n_calls
        origin, cell, dims = grid
        fh.write(np.array([op, m.V, m.F, m["colors"] is not None, *dims, nv, nf], np.int32).tobytes())
        fh.write(np.array([*origin, cell], np.float32).tobytes())
        for a in (m["vertices"], m["colors"], m["faces"], keep, *results):
            if a is not None:
                fh.write(np.ascontiguousarray(a).tobytes())
        n_calls += 1

    none = ((0, 0, 0), 1.0, (1, 1, 1))
    with open(tmp_path / "calls.bin", "wb") as fh:
        for name in ("scene", "chain_bitrev", "star"):
            m = fixture(name)
            write(fh, 0, m, none, None, sm.emul_components(m.V, m["faces"]), 0, 0)
        m = sm.scene()
        for variant, keep in sm.keep_variants(m).items():
            v, f, c, bad = sm.emul_select(m, keep)
            write(fh, 1, m, none, keep, (sm.emul_select_count(m.V, m["faces"], keep)[1], v, c, f), len(v), len(f))
        for mm in (m, sm.mesh(m["vertices"], m["faces"]), sm.sphere()):
            for cell_voxels, shift in ((1.5, 0.37), (4.0, 0.0)):
                grid = sm.grid_of(mm, cell_voxels, shift)
                v, f, c, dropped = sm.emul_cluster(mm, *grid)
                write(fh, 2, mm, grid, None, (sm.emul_cluster_count(mm, *grid)[1], v, c, f), len(v), len(f))
        origin, cell, dims = sm.grid_of(m, 2.0, 0.37)
        grid = (origin, cell, (dims[0] // 2, dims[1], dims[2]))                               # vertices outside the grid
        v, f, c, dropped = sm.emul_cluster(m, *grid)
        write(fh, 2, m, grid, None, (sm.emul_cluster_count(m, *grid)[1], v, c, f), len(v), len(f))
    exe = tmp_path / "mesh_cleanup_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    str(sm.CSRC), "-I", str(sm.TESTS), "-o", str(exe), str(sm.TESTS / "mesh_cleanup_asan_main.cpp")], check=True)
    run = subprocess.run([str(exe), str(tmp_path / "calls.bin")], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip() == f"{n_calls} calls, 0 bad", (run.stdout, run.stderr[-2000:])
