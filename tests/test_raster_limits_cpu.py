"""CPU: the inputs of tests/test_gpu_raster_limits.py reach the code paths they are meant for (regime guards, from the host count of
raster_bin's lists in tests/raster_emul.cpp), and on every one of them the host emulation of the kernels equals the independent oracle
(oracle/raster.c) bit for bit -- so a mismatch of the GPU tests points at the device glue (wave broadcasts, LDS hand-offs, atomics), not
at the arithmetic of raster_core.h."""
import numpy as np
import pytest

from tests.support import raster_limits as rl

H, W = rl.H, rl.W


@pytest.fixture(scope="module")
def views(engine_meshes):
    return rl.single_views(engine_meshes)


def _counts(view, ns):
    mesh, T, K = view
    return rl.bin_counts(mesh, T, K, H, W, ns), rl.bin_layout(len(mesh["faces"]), H, W)


@pytest.mark.parametrize("ns", [1, 4])
def test_regime_list_overflow(views, ns):
    """A near: the binned records exceed cap_list by at least 10 %, no large entry; A far fits"""
    c, lay = _counts(views["A_near"], ns)
    assert lay["cap_list"] == 3 * 864 + 2048 and lay["cap_large"] == 4 * 864 + 4096
    assert c["n_binned"][0] >= 1.1 * lay["cap_list"] and c["n_large"][0] == 0, (c["n_binned"], c["n_large"])
    c, _ = _counts(views["A_far"], ns)
    assert 0 < c["n_binned"][0] <= lay["cap_list"] and c["n_large"][0] <= lay["cap_large"]


@pytest.mark.parametrize("ns", [1, 4])
def test_regime_large_overflow(views, ns):
    """B: the large-list entries exceed cap_large by at least 10 % while the binned total fits; B tilted through the near plane: the
    same cause, with clipped pieces and second pieces (ids >= F)"""
    for name in ("B", "B_clip"):
        c, lay = _counts(views[name], ns)
        assert lay["cap_large"] == 4 * 320 + 4096
        assert c["n_large"][0] >= 1.1 * lay["cap_large"] and c["n_binned"][0] <= lay["cap_list"], (name, c["n_binned"], c["n_large"])
    assert _counts(views["B"], ns)[0]["n_binned"][0] == 0
    st = _counts(views["B_clip"], ns)[0]["stats"][0]
    assert st[3] >= 100 and st[0] > 320 + 40, st   # clipped pieces; more pieces than triangles that survive: second pieces exist
    c, lay = _counts(views["A_clip"], ns)   # (mesh A through the near plane: clipped pieces, but it cannot overflow -- see rl.A_CLIP_VIEW)
    assert c["stats"][0][3] >= 100 and c["n_binned"][0] <= lay["cap_list"] and c["n_large"][0] <= lay["cap_large"]


@pytest.mark.parametrize("name", ["D_52x76", "A_92x124"])
def test_regime_ragged_frames(name):
    """the frames of the output-form test: the O view overflows by the stated cause with 10 % to spare, the F view fits; and the emulation
    equals the oracle on both"""
    from oracle import raster as orr

    mesh, h, w, K, z_over, z_fit, cause = rl.ragged_configs()[name]
    lay = rl.bin_layout(len(mesh["faces"]), h, w)
    T = np.stack([rl.pose_z(z_over), rl.pose_z(z_fit)])
    Kn = np.repeat(K[None], 2, 0)
    for ns in (1, 4):
        c = rl.bin_counts(mesh, T, Kn, h, w, ns)
        if cause == "list":
            assert c["n_binned"][0] >= 1.1 * lay["cap_list"] and c["n_large"][0] <= lay["cap_large"]
        else:
            assert c["n_large"][0] >= 1.1 * lay["cap_large"] and c["n_binned"][0] <= lay["cap_list"]
        assert 0 < c["n_binned"][1] <= lay["cap_list"] and c["n_large"][1] <= lay["cap_large"]
    ref = orr.render(mesh, T, Kn, h, w, 19)
    for g, r in zip(rl.emul_render(mesh, T, Kn, h, w, 19, cap_list=1), ref):
        assert np.array_equal(g, r)


def test_regime_record_slots_beyond_510(views):
    """C at 4x MSAA fits, and its fullest tile holds more than 511 records (at one sample per pixel most of its 0.45-pixel triangles
    contain no sample and are never binned: 142 in the fullest tile)"""
    c, lay = _counts(views["C"], 4)
    assert c["n_binned"][0] <= lay["cap_list"] and c["n_large"][0] == 0
    assert c["binned"].max() > rl.SLOT_NONE + 100, c["binned"].max()
    c1, _ = _counts(views["C"], 1)
    assert c1["n_binned"][0] <= lay["cap_list"] and c1["binned"].max() < rl.SLOT_NONE


@pytest.mark.parametrize("ns", [1, 4])
def test_regime_guard_band(views, ns):
    """the table view: pieces with |X| > 2^21 sub-pixel units (8192 px), triangles rejected by GUARD, pieces clipped at the near plane"""
    c, _ = _counts(views["table"], ns)
    n_pieces, n_wide, n_guard, n_clipped = c["stats"][0]
    assert n_wide >= 3 and n_guard >= 1 and n_clipped >= 3, c["stats"]
    assert c["n_large"][0] > 0 and c["n_binned"][0] > 0


def test_regime_far_plane(views):
    """the far-plane views: at half the scale (same picture, every depth halved, nothing out of range) the visible surface has samples on
    both sides of what corresponds to 10 m, in the views from 10.5 m on; and the picture at full scale is cut there"""
    from oracle import raster as orr

    mesh, T, K = views["far_plane"]
    dep = orr.render(mesh, T, K, H, W, 2)[2]
    mh, Th = rl.half_scale(mesh, T)
    d2 = 2.0 * orr.render(mh, Th, K, H, W, 2)[2]
    for i, z in enumerate(rl.FAR_ZS):
        beyond, within = int((d2[i] > rl.Z_FAR + 0.01).sum()), int(((d2[i] > 0) & (d2[i] < rl.Z_FAR - 0.01)).sum())
        assert within > 200, (z, within)
        assert (beyond > 200) == (z >= 10.5), (z, beyond)
        assert dep[i].max() <= rl.Z_FAR and (dep[i] > 0).sum() >= within and (dep[i] > 0).sum() <= within + 200


@pytest.mark.parametrize("msaa", [1, 4])
@pytest.mark.parametrize("name", ["A_near", "A_far", "A_clip", "B", "B_clip", "C", "table", "far_plane"])
def test_emulation_equals_oracle(views, name, msaa):
    """the emulation's capacities are the device's for this mesh (3 F + 2048 records, 4 F + 4096 large entries): A near, B and B_clip take
    the fallback (every tile walks all 2F piece indices), the others their lists"""
    from oracle import raster as orr

    mesh, T, K = views[name]
    flags = 3 | (16 if msaa == 4 else 0)
    ref = orr.render(mesh, T, K, H, W, flags)
    got = rl.emul_render(mesh, T, K, H, W, flags)
    for g, r, what in zip(got, ref, ("rgb", "normals", "depth")):
        assert np.array_equal(g, r), (name, what, (g != r).mean())
    assert (ref[2] > 0).any()


@pytest.mark.parametrize("msaa", [1, 4])
def test_emulation_fallback_equals_oracle_on_large_pieces(views, msaa):
    """B and B tilted with cap_list = 1 (B itself bins no record, so it is its large list that sends it to the fallback either way; the
    tilted view bins a few), and every other view with cap_list = 1 wherever that forces the fallback"""
    from oracle import raster as orr

    flags = 3 | (16 if msaa == 4 else 0)
    for name in ("B", "B_clip", "A_far", "A_clip", "C", "table"):
        mesh, T, K = views[name]
        ref = orr.render(mesh, T, K, H, W, flags)
        got = rl.emul_render(mesh, T, K, H, W, flags, cap_list=1)
        for g, r in zip(got, ref):
            assert np.array_equal(g, r), name


@pytest.mark.parametrize("msaa", [1, 4])
def test_scene_emulation_on_the_overflow_scene(msaa):
    """the scene of the GPU test: its first camera's near object overflows (regime guard), and the single-object camera of the scene
    emulation equals the oracle"""
    from oracle import raster as orr
    from tests.support import raster_scene as rsc

    meshes, obj_off, mesh_ids, T, K, radius = rl.overflow_scene()
    ns = 4 if msaa == 4 else 1
    lay = rl.bin_layout(max(len(m["faces"]) for m in meshes), H, W)
    c = rl.bin_counts(meshes[0], T[:2], K[[0, 0]], H, W, ns)
    assert c["n_binned"][0] >= 1.1 * lay["cap_list"] and 0 < c["n_binned"][1] <= lay["cap_list"]
    cb = rl.bin_counts(meshes[1], T[3:4], K[1:2], H, W, ns)
    assert cb["n_large"][0] >= 1.1 * lay["cap_large"]   # B overflows the capacity the database's largest mesh (A) sets
    flags = 3 | (16 if msaa == 4 else 0)
    cc = rl.bin_counts(meshes[1], T[3:4], K[1:2], H, W, ns)
    lay_c = rl.bin_layout(3200, H, W)   # with mesh C in the database, nothing of this scene overflows on the device
    assert c["n_binned"][0] <= lay_c["cap_list"] and cc["n_large"][0] <= lay_c["cap_large"]
    rigs = [orr.lights_struct() for _ in mesh_ids]
    rgb, nrm, dep, ins = rsc.render(meshes, obj_off, mesh_ids, T, K, radius, rigs, H, W, flags)
    assert set(np.unique(ins[0]).tolist()) == {-1, 0, 1, 2}   # every object of camera 0 is seen
    far = orr.render(meshes[0], T[1:2], K[:1], H, W, flags)[2][0] > 0
    assert (far & (ins[0] == 0)).sum() > 100 and (far & (ins[0] == 1)).sum() > 100   # A far: partly behind A near, partly visible
    ref = orr.render(meshes[1], T[3:4], K[1:2], H, W, flags)
    assert np.array_equal(rgb[1], ref[0][0]) and np.array_equal(nrm[1], ref[1][0]) and np.array_equal(dep[1], ref[2][0])


def test_bin_layout_restatement_by_hand():
    """bin_layout / workspace_bytes for mesh A at 96 x 128, worked out by hand from the layout comment of raster_bin.h (the GPU tier compares
    them with mp_raster_workspace_bytes)"""
    lay = rl.bin_layout(864, H, W)
    assert lay["cap_list"] == 4640 and lay["cap_large"] == 7552 and lay["n_tiles"] == 192
    assert lay["off_tl"] == 200 and lay["off_large"] == 396 and lay["off_list"] == 396 + 7552 and lay["view_ints"] == 396 + 7552 + 8 * 4640
    assert rl.workspace_bytes(lay, 2) == (2 * lay["view_ints"] + 4 + 384) * 4 + 2 * 384
