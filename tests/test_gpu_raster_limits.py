"""-m gpu: the rasteriser (raster_bin, raster_classify, raster_tiles*, raster_scene_tiles) at its overflow, size and range limits, on the
device -- the paths the lathe meshes at ordinary distances never take and the host emulation cannot cover (wave broadcasts, LDS hand-offs,
atomics).  Inputs and their regimes: tests/support/raster_limits.py, re-checked on the CPU by tests/test_raster_limits_cpu.py.

Every pixel comparison is bit for bit against oracle.raster.render (the scene renderer: against its host emulation, and against the oracle
where one object is alone); the sole exception is point-lit RGB, with the allowance of test_raster_bit_exact_vs_oracle (1 LSB of the 8-bit
quantisation on fewer than 1e-3 of the pixels).  What raster_bin wrote (per-view header, tile offsets) is read back from the workspace and
compared with the host count of tests/raster_emul.cpp: that is how these tests know the overflow branch ran."""
import numpy as np
import pytest
import torch

from tests.support import raster_limits as rl

pytestmark = pytest.mark.gpu

H, W = rl.H, rl.W
SENT = -3.0


@pytest.fixture(scope="module")
def eng():
    from megapose6d_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert engine.device_info()[2].startswith("gfx950")
    return engine


@pytest.fixture(scope="module")
def views(engine_meshes):
    return rl.single_views(engine_meshes)


_oracle_cache = {}


def _oracle(key, mesh, T, K, h, w, flags, lights=None):
    """oracle.raster.render, computed once per (key, frame, flags) and shared between the tests (never modified)"""
    from oracle import raster as orr

    k = (key, h, w, flags, lights is not None)
    if k not in _oracle_cache:
        _oracle_cache[k] = orr.render(mesh, T, K, h, w, flags, lights)
    return _oracle_cache[k]


def _render(eng, db, T, K, h, w, flags, lights=None, mesh_ids=None):
    """n single views into a sentinel-poisoned [n, h, w, 8] tensor: rgb 0..2, normals 3..5, depth 6; channel 7 must stay untouched"""
    n = len(T)
    ids = torch.zeros(n, dtype=torch.int32, device="cuda") if mesh_ids is None else torch.as_tensor(mesh_ids, dtype=torch.int32).cuda()
    out = torch.full((n, h, w, 8), SENT, device="cuda")
    eng.raster_render(db, ids, torch.from_numpy(np.ascontiguousarray(T, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(K, np.float32)).cuda(),
                      h, w, flags, lights if lights is not None else eng.make_lights(), out, h * w * 8, w * 8, 8, 0, 3, 6)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[..., 7] == SENT).all(), "the unwritten channel was touched"
    return got


def _assert_equals_oracle(got, ref, flags, what, lit=False):
    rgb, nrm, dep = ref
    if lit:   # point lights use sqrt / div chains: 1 LSB of the uint8 quantisation on a few pixels (test_raster_bit_exact_vs_oracle)
        d = np.abs(got[..., 0:3] - rgb)
        assert d.max() <= 1.0 / 255 + 1e-7 and (d > 0).mean() < 1e-3, (what, d.max(), (d > 0).mean())
    else:
        assert np.array_equal(got[..., 0:3], rgb), (what, "rgb", (got[..., 0:3] != rgb).mean())
    if flags & 1:
        assert np.array_equal(got[..., 3:6], nrm), (what, "normals", (got[..., 3:6] != nrm).mean())
    if flags & 2:
        assert np.array_equal(got[..., 6], dep), (what, "depth", (got[..., 6] != dep).mean())


def _check_headers(db, mesh, T, K, h, w, ns, what):
    """the headers and tile offsets of the LAST launch on db (views of `mesh`, the database's largest) == the host count -> hdr, tile_off"""
    got = rl.view_headers(db, len(T), h, w)
    lay = got["layout"]
    assert lay == rl.bin_layout(len(mesh["faces"]), h, w), "the workspace is not sized for this mesh as the database's largest"
    counts = rl.bin_counts(mesh, T, K, h, w, ns)
    hdr, off, off_l = rl.expected_headers(counts, lay)
    assert np.array_equal(got["hdr"][:, :3], hdr), (what, got["hdr"].tolist(), hdr.tolist())
    assert set(got["hdr"][:, 3].tolist()) <= {0, 1}
    for v in range(len(T)):
        if not hdr[v, 2]:
            assert np.array_equal(got["tile_off"][v], off[v]), (what, v, "tile offsets of the binned records")
            assert np.array_equal(got["tile_off_l"][v], off_l[v]), (what, v, "tile offsets of the large list")
    return got["hdr"], got["tile_off"]


# ---- 1. what raster_bin writes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msaa", [1, 4])
def test_bin_pass_headers_and_tile_offsets_equal_the_host_count(eng, engine_meshes, views, msaa):
    """hdr[0] (large entries), hdr[1] (binned entries), hdr[2] (overflow) of every view == the host count; without overflow both
    tile-offset arrays == the prefix sums of the host's per-tile counts.  Views: A near (list overflow), A far, A through the near plane, a
    non-finite pose (one launch of four views); B and B through the near plane (large-list overflow); C; a lathe mesh."""
    flags = 3 | (16 if msaa == 4 else 0)
    A = views["A_near"][0]
    T = np.stack([views["A_near"][1][0], views["A_far"][1][0], views["A_clip"][1][0], views["A_far"][1][0]])
    T[3, 0, 3] = np.nan
    K = np.repeat(rl.K_SMALL[None], 4, 0)
    db = eng.MeshDB([A])
    _render(eng, db, T, K, H, W, flags)
    hdr, _ = _check_headers(db, A, T, K, H, W, msaa, "A")
    assert hdr[:, 2].tolist() == [1, 0, 0, 0] and hdr[0, 0] == 0 and hdr[3, :2].tolist() == [0, 0]
    B = views["B"][0]
    T = np.stack([views["B"][1][0], views["B_clip"][1][0]])
    db = eng.MeshDB([B])
    _render(eng, db, T, K[:2], H, W, flags)
    hdr, _ = _check_headers(db, B, T, K[:2], H, W, msaa, "B")
    assert hdr[:, 2].tolist() == [1, 1] and hdr[0, 1] == 0
    Cm, T, Kc = views["C"]
    db = eng.MeshDB([Cm])
    _render(eng, db, T, Kc, H, W, flags)
    hdr, _ = _check_headers(db, Cm, T, Kc, H, W, msaa, "C")
    assert hdr[0, 2] == 0
    lathe = max(engine_meshes, key=lambda m: len(m["faces"]))   # (the largest of its database: the capacities are its own)
    from tests.support import synthetic as syn
    T = np.stack([syn.random_pose(np.random.RandomState(3), z_range=(0.3, 0.4)) for _ in range(2)]).astype(np.float32)
    db = eng.MeshDB(engine_meshes)
    ids = [engine_meshes.index(lathe)] * 2
    _render(eng, db, T, K[:2], H, W, flags, mesh_ids=ids)
    hdr, _ = _check_headers(db, lathe, T, K[:2], H, W, msaa, "lathe")
    assert hdr[:, 2].tolist() == [0, 0] and (hdr[:, 1] > 0).all()


def test_workspace_layout_restatement_equals_the_library(eng, engine_meshes, views):
    from megapose6d_amd import _lib

    lib = _lib.load()
    for meshes in ([views["A_near"][0]], [views["B"][0]], [views["C"][0], views["B"][0]], engine_meshes):
        db = eng.MeshDB(meshes)
        F = max(len(m["faces"]) for m in meshes)
        for h, w in ((96, 128), (52, 76)):
            assert rl.db_max_faces(db, h, w) == F
            for n_views in (1, 2, 5):
                assert rl.workspace_bytes(rl.bin_layout(F, h, w), n_views) == lib.mp_raster_workspace_bytes(db.handle, n_views, h, w)


# ---- 2. overflowed views against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msaa", [1, 4])
@pytest.mark.parametrize("cause", ["list", "large", "large_clipped"])
def test_overflowed_view_equals_oracle(eng, views, cause, msaa):
    """A view whose lists do not fit: raster_tiles walks all 2F piece indices through the 64-bit sweep, no record, no record prefetch.
    Causes: the binned records (A), the large list (B), the large list of a mesh crossing the near plane (B tilted: clipped pieces, second
    pieces with ids >= F).  RGB, normals, depth; at 4x MSAA also with six point lights.  The header says overflow == 1.
    (Mesh A through the near plane cannot overflow, see rl.A_CLIP_VIEW: it is compared here as well, as a view that fits.)"""
    from oracle import raster as orr

    name = {"list": "A_near", "large": "B", "large_clipped": "B_clip"}[cause]
    mesh, T, K = views[name]
    flags = 3 | (16 if msaa == 4 else 0)
    db = eng.MeshDB([mesh])
    got = _render(eng, db, T, K, H, W, flags)
    hdr = rl.view_headers(db, 1, H, W)["hdr"]
    assert hdr[0, 2] == 1, hdr
    assert (hdr[0, 1] > hdr[0, 0]) == (cause == "list")
    ref = _oracle(name, mesh, T, K, H, W, flags)
    assert (ref[2] > 0).mean() > 0.2
    _assert_equals_oracle(got, ref, flags, name)
    if msaa == 4:
        dirs, cols, offs = orr.POINT_DIRS, [(0.4, 0.4, 0.4)] * 6, [(0.0, 0.0, 0.01 * k) for k in range(6)]
        L, Lo = eng.make_lights((0.1, 0.1, 0.1), dirs, cols, offs), orr.lights_struct((0.1, 0.1, 0.1), dirs, cols, offs)
        got = _render(eng, db, T, K, H, W, flags, L)
        assert rl.view_headers(db, 1, H, W)["hdr"][0, 2] == 1
        _assert_equals_oracle(got, _oracle(name, mesh, T, K, H, W, flags, Lo), flags, name + " lit", lit=True)
    if cause == "list":
        mesh, T, K = views["A_clip"]
        got = _render(eng, db, T, K, H, W, flags)
        assert rl.view_headers(db, 1, H, W)["hdr"][0, 2] == 0
        _assert_equals_oracle(got, _oracle("A_clip", mesh, T, K, H, W, flags), flags, "A_clip")


# ---- 3. items of four views with an overflowed view in any position --------------------------------------------------------------------------
PATTERNS = ["OFOF", "FOFF", "FFFO", "OOOO", "EEOE"]


def _item_poses(pattern, z_over, z_fit):
    T = np.stack([rl.pose_z(z_over if c == "O" else z_fit) for c in pattern])
    for v, c in enumerate(pattern):
        if c == "E":
            T[v, 0, 3] = np.nan
    return T


@pytest.mark.parametrize("msaa", [1, 4])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_item_of_four_views_with_overflowed_views(eng, views, monkeypatch, pattern, msaa):
    """views_per_item = 4 (a wave walks the four views of its item; the first records of view r + 1 are requested while view r is
    processed, which must skip an overflowed view), mesh A: O = near (overflow), F = far (fits), E = non-finite pose (empty).  Each view ==
    the oracle; the direct form (MP_RASTER_COMPACT=0) == the compacted form; three runs are equal; for E E O E every tile of the item is
    marked as reached (an overflowed view reaches every tile)."""
    mesh = views["A_near"][0]
    V, Cp, flags = 4, 32, 3 | (16 if msaa == 4 else 0)
    Tn = _item_poses(pattern, rl.Z_NEAR_VIEW, rl.Z_FAR_VIEW)
    Kn = np.repeat(rl.K_SMALL[None], V, 0)
    T, K = torch.from_numpy(Tn).cuda(), torch.from_numpy(Kn).cuda()
    ids = torch.zeros(V, dtype=torch.int32, device="cuda")
    db = eng.MeshDB([mesh])
    ref = {"O": _oracle("A_near", *views["A_near"], H, W, flags), "F": _oracle("A_far", *views["A_far"], H, W, flags)}
    outs = []
    for compact in ("0", "1", "1", "1"):
        monkeypatch.setenv("MP_RASTER_COMPACT", compact)
        x = torch.full((1, H, W, Cp), SENT, device="cuda")
        eng.raster_render(db, ids, T, K, H, W, flags, eng.make_lights(), x, H * W * Cp, W * Cp, Cp, 0, 3, 6, views_per_item=V, stride_view=7)
        torch.cuda.synchronize()
        outs.append(x.cpu().numpy())
    hdr = rl.view_headers(db, V, H, W)["hdr"]
    assert hdr[:, 2].tolist() == [1 if c == "O" else 0 for c in pattern], hdr
    if pattern == "EEOE":   # the job flags of the last (compacted) launch: inside the workspace, behind the view blocks
        n_tiles = rl.bin_layout(len(mesh["faces"]), H, W)["n_tiles"]
        ws = db.workspace(V, H, W, rl.launch_device())
        addr = eng.raster_job_flags(db, V, H, W, rl.launch_device())
        assert addr != 0, "the compacted launch left no job flags"
        off = addr - ws.data_ptr()
        assert 0 < off and off + n_tiles <= ws.numel()
        assert (ws[off:off + n_tiles].cpu().numpy() == 1).all(), "a tile of an item with an overflowed view counts as not reached"
    got = outs[0][0]
    assert (got[..., 7 * V:] == SENT).all(), "a padding channel was written"
    for v, c in enumerate(pattern):
        g = got[..., 7 * v:7 * v + 7]
        if c == "E":
            assert (g == 0).all(), f"view {v} (non-finite pose) is not empty"
        else:
            rgb, nrm, dep = ref[c]
            assert np.array_equal(g[..., 0:3], rgb[0]), f"view {v} ({c}): rgb differs from the oracle"
            assert np.array_equal(g[..., 3:6], nrm[0]), f"view {v} ({c}): normals differ from the oracle"
            assert np.array_equal(g[..., 6], dep[0]), f"view {v} ({c}): depth differs from the oracle"
    assert np.array_equal(outs[0], outs[1]), "the compacted form differs from the direct form"
    assert np.array_equal(outs[1], outs[2]) and np.array_equal(outs[1], outs[3]), "two runs differ"


# ---- 4. output forms under overflow ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["D_52x76", "A_92x124"])
def test_output_forms_of_an_item_with_overflowed_views(eng, monkeypatch, config):
    """Item O F O F written as fp32 with the fused crop, as binary16 and as RGB stem records, in a sentinel-poisoned tensor with a margin and
    padding channels, at frames whose last tile column and row are cut (the ragged store): binary16 == fp32.half(); the decoded records ==
    fp32 (decoding of test_raster_ragged_tiles_every_output_form); the sentinel survives outside; the fp32 views == the oracle.  52 x 76 runs
    mesh D (large-list overflow), 92 x 124 mesh A (list overflow): see rl.ragged_configs."""
    mesh, h, w, K1, z_over, z_fit, cause = rl.ragged_configs()[config]
    V, Cp, flags = 4, 32, 1 | 16
    Tn = _item_poses("OFOF", z_over, z_fit)
    Kn = np.repeat(K1[None], V, 0)
    T, K = torch.from_numpy(Tn).cuda(), torch.from_numpy(Kn).cuda()
    ids = torch.zeros(V, dtype=torch.int32, device="cuda")
    db = eng.MeshDB([mesh])
    g = torch.Generator().manual_seed(5)
    obs = eng.PackedObservation(torch.rand(1, 3, 480, 640, generator=g).cuda())
    im_ids = torch.tensor([0], dtype=torch.int32).cuda()
    boxes = torch.tensor([[100.0, 80, 400, 305]]).cuda()
    HP, WP = h + 4, w + 4
    n_written = 3 + 6 * V
    monkeypatch.setenv("MP_RASTER_COMPACT", "1")
    out = {}
    for mode in ("fp32_crop", "f16_crop", "records_rgb"):
        if mode == "records_rgb":
            R = eng.xrec_elements(3, 6 * V)
            x = torch.full((1, HP, WP, R), SENT, device="cuda", dtype=torch.bfloat16)
            eng.raster_render(db, ids, T, K, h, w, flags, eng.make_lights(), x, HP * WP * R, WP * R, R, 3, 6, -1, views_per_item=V, stride_view=6,
                              crop=(obs, im_ids, boxes, 0))
            n_ch = R
        else:
            x = torch.full((1, HP, WP, Cp), SENT, device="cuda", dtype=torch.float16 if mode == "f16_crop" else torch.float32)
            eng.raster_render(db, ids, T, K, h, w, flags, eng.make_lights(), x, HP * WP * Cp, WP * Cp, Cp, 3, 6, -1, views_per_item=V, stride_view=6,
                              crop=(obs, im_ids, boxes, 0))
            n_ch = n_written
        torch.cuda.synchronize()
        hdr = rl.view_headers(db, V, h, w)["hdr"]
        assert hdr[:, 2].tolist() == [1, 0, 1, 0], (mode, hdr)
        assert (hdr[0, 1] > hdr[0, 0]) == (cause == "list")
        x = x.float()
        assert (x[:, :h, :w, :n_ch] != SENT).all(), f"{mode}: a pixel of a written channel was not written"
        assert (x[:, h:] == SENT).all() and (x[:, :, w:] == SENT).all(), f"{mode}: written below / right of the image"
        assert (x[:, :h, :w, n_ch:] == SENT).all(), f"{mode}: a padding channel was written"
        out[mode] = x[:, :h, :w].cpu()
    ref = out["fp32_crop"][..., :n_written]
    for v, c in enumerate("OFOF"):
        rgb, nrm, _ = _oracle((config, c), mesh, Tn[v:v + 1], Kn[v:v + 1], h, w, flags | 2)
        got = ref[0, :, :, 3 + 6 * v:9 + 6 * v].numpy()
        assert np.array_equal(got[..., :3], rgb[0]), f"view {v}: rgb differs from the oracle"
        assert np.array_equal(got[..., 3:], nrm[0]), f"view {v}: normals differ from the oracle"
        assert (rgb[0] > 0).any(-1)[h - 4:].any() or c == "F", "the overflowed view should reach the ragged last tile row"
    assert torch.equal(out["f16_crop"][..., :n_written], ref.half().float())
    rec = out["records_rgb"]
    crop_dec = torch.stack([(rec[..., 3 * c] + rec[..., 3 * c + 1]) + rec[..., 3 * c + 2] for c in range(3)], dim=-1)
    k = rec[..., 9:9 + 6 * V]
    assert torch.equal(k, k.round()) and (k >= 0).all() and (k <= 255).all()
    assert torch.equal(torch.cat([crop_dec, k / 255.0], dim=-1), ref)
    assert (rec[..., 9 + 6 * V:] == 0).all()   # the record's zero padding


# ---- 5. scene renderer ---------------------------------------------------------------------------------------------------------------------------
def _render_scene(eng, db, obj_off, mesh_ids, T, K, radius, rigs, h, w, flags):
    n_cams = len(obj_off) - 1
    dev = torch.device("cuda")
    out = torch.full((n_cams, h, w, 8), SENT, device=dev)
    inst = torch.full((n_cams, h, w), -7, dtype=torch.int32, device=dev)
    eng.raster_render_scene(db, obj_off, torch.tensor(mesh_ids, dtype=torch.int32, device=dev), torch.from_numpy(np.ascontiguousarray(T, np.float32)).to(dev),
                            torch.from_numpy(np.ascontiguousarray(K, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(radius, np.float32)).to(dev),
                            eng.lights_array(rigs, dev), h, w, flags, out, h * w * 8, w * 8, 8, 0, 3, 6, inst)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[..., 7] == SENT).all()
    return o, inst.cpu().numpy()


@pytest.mark.parametrize("msaa", [1, 4])
@pytest.mark.parametrize("database", ["A_largest", "C_largest"])
def test_scene_with_overflowed_objects_equals_emulation_and_oracle(eng, database, msaa):
    """raster_scene_tiles has its own copy of the overflow walk.  Camera 0: A near (list overflow), A far partly behind it, the pyramid of
    test_raster_large_triangles_and_close_camera; camera 1: B alone (large-list overflow).  The scene emulation decides overflow per object
    mesh, the device per database maximum: with A the database's largest mesh both sides overflow; with mesh C appended to the database
    only the emulation does (rl.overflow_scene, counted in tests/test_raster_limits_cpu.py), and the pixels must agree whichever side
    overflowed.  Kernel == emulation in RGB, normals, depth and instance ids; the single-object camera == the oracle."""
    from oracle import raster as orr
    from tests.support import raster_scene as rsc

    meshes, obj_off, mesh_ids, T, K, radius = rl.overflow_scene(with_c=database == "C_largest")
    flags = 3 | (16 if msaa == 4 else 0)
    rigs = [eng.make_lights() for _ in mesh_ids]
    db = eng.MeshDB(meshes)
    o, inst = _render_scene(eng, db, obj_off, mesh_ids, T, K, radius, rigs, H, W, flags)
    if ("scene", flags) not in _oracle_cache:   # (the emulation does not see the database: one reference for both)
        _oracle_cache[("scene", flags)] = rsc.render(meshes[:3], obj_off, mesh_ids, T, K, radius, rigs, H, W, flags)
    rgb, nrm, dep, ins = _oracle_cache[("scene", flags)]
    assert np.array_equal(o[..., 0:3], rgb), ("rgb", (o[..., 0:3] != rgb).mean())
    assert np.array_equal(o[..., 3:6], nrm), ("normals", (o[..., 3:6] != nrm).mean())
    assert np.array_equal(o[..., 6], dep) and np.array_equal(inst, ins)
    assert set(np.unique(ins[0]).tolist()) == {-1, 0, 1, 2}
    ref = orr.render(meshes[1], T[3:4], K[1:2], H, W, flags)
    _assert_equals_oracle(o[1:2], ref, flags, "B alone in a scene")
    assert (ref[2] > 0).mean() > 0.2


# ---- 6. record slots beyond 510 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msaa", [1, 4])
def test_tile_with_more_than_511_records_equals_oracle(eng, views, msaa):
    """The depth key has 9 slot bits; a record at position >= 511 of its tile's list carries SLOT_NONE and shading re-derives the piece
    from the mesh.  C is one layer of 0.45-pixel triangles with nothing hidden, so records at such positions win samples in whatever order
    the list was filled.  At 4x MSAA the fullest tile holds 648 records (from the device's own tile offsets); at one sample per pixel most of
    these triangles contain no sample and are not binned (fullest tile: 142), that run keeps the comparison only."""
    mesh, T, K = views["C"]
    flags = 3 | (16 if msaa == 4 else 0)
    db = eng.MeshDB([mesh])
    got = _render(eng, db, T, K, H, W, flags)
    hdr, tile_off = _check_headers(db, mesh, T, K, H, W, msaa, "C")
    assert hdr[0, 2] == 0
    fullest = int(np.diff(tile_off[0]).max())
    print("fullest tile:", fullest, "records")
    if msaa == 4:
        assert fullest > rl.SLOT_NONE
    ref = _oracle("C", mesh, T, K, H, W, flags)
    assert (ref[0][0] > 0).any(-1).sum() > 150
    _assert_equals_oracle(got, ref, flags, "C")


# ---- 7. guard band and far plane ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msaa", [1, 4])
def test_table_seen_from_close_up_equals_oracle(eng, views, msaa):
    """A 4 m table top with a lathe mesh on it, camera 0.3 m above it at a grazing angle: triangles cross the near plane, others reach
    beyond 8192 px (edge values of the 64-bit sweep up to ~2^46), some are dropped by the guard band (by contract, oracle/raster.c).  As a
    batch-renderer view and as a one-object scene."""
    mesh, T, K = views["table"]
    flags = 3 | (16 if msaa == 4 else 0)
    ref = _oracle("table", mesh, T, K, H, W, flags)
    assert (ref[2] > 0).mean() > 0.1
    db = eng.MeshDB([mesh])
    got = _render(eng, db, T, K, H, W, flags)
    _check_headers(db, mesh, T, K, H, W, msaa, "table")
    _assert_equals_oracle(got, ref, flags, "table, batch renderer")
    o, inst = _render_scene(eng, db, [0, 1], [0], T, K, np.array([2.9], np.float32), [eng.make_lights()], H, W, flags)
    _assert_equals_oracle(o, ref, flags, "table, scene renderer")
    assert np.array_equal(inst[0] >= 0, ref[2][0] > 0)


@pytest.mark.parametrize("msaa", [1, 4])
def test_far_plane_cuts_the_picture_like_the_oracle(eng, views, msaa):
    """A lathe mesh scaled x20 at 9 .. 11 m: the per-sample depth range ends at Z_FAR = 10 m, from 10.5 m on part of the visible surface lies
    beyond it.  At 12 m nothing is left."""
    mesh, T, K = views["far_plane"]
    T = np.concatenate([T, rl.tilted(90.0, 12.0)[None]])
    K = np.repeat(rl.K_SMALL[None], len(T), 0)
    flags = 3 | (16 if msaa == 4 else 0)
    ref = _oracle("far_plane+12", mesh, T, K, H, W, flags)
    db = eng.MeshDB([mesh])
    got = _render(eng, db, T, K, H, W, flags)
    _assert_equals_oracle(got, ref, flags, "far plane")
    dep = got[..., 6]
    assert dep.max() <= rl.Z_FAR
    assert all((dep[i] > 0).sum() > 200 for i in range(len(rl.FAR_ZS))) and dep[2].max() > rl.Z_FAR - 0.01
    assert (got[-1, ..., :7] == 0).all()
    o, _ = _render_scene(eng, db, [0, 1, 2], [0, 0], T[[2, 4]], K[:2], np.array([1.8, 1.8], np.float32), [eng.make_lights()] * 2, H, W, flags)
    _assert_equals_oracle(o, tuple(r[[2, 4]] for r in ref), flags, "far plane, scene renderer")


# ---- 8. frame limits -------------------------------------------------------------------------------------------------------------------------------
def _frame_K(h, w):
    K = rl.K_TABLE.copy()
    K[0, 2], K[1, 2] = 0.5 * w, 0.5 * h
    return K[None]


def test_largest_frame_equals_oracle(eng, views):
    """1024 x 1024, the limit the entries state: raster_bin needs 2 x 16384 tile counters = exactly the 128 KB of dynamic LDS
    raster_bin_launch asks for, next to its static arrays.  The table view's mesh (table top + lathe mesh), 4x MSAA."""
    mesh, T, _ = views["table"]
    h = w = 1024
    K, flags = _frame_K(h, w), 19
    ref = _oracle("table", mesh, T, K, h, w, flags)
    assert 0.3 < (ref[2] > 0).mean() < 0.9
    db = eng.MeshDB([mesh])
    got = _render(eng, db, T, K, h, w, flags)
    _check_headers(db, mesh, T, K, h, w, 4, "1024 x 1024")
    _assert_equals_oracle(got, ref, flags, "1024 x 1024")
    o, _ = _render_scene(eng, db, [0, 1], [0], T, K, np.array([2.9], np.float32), [eng.make_lights()], h, w, flags)
    _assert_equals_oracle(o, ref, flags, "1024 x 1024, scene renderer")


@pytest.mark.parametrize("h,w", [(1, 1), (8, 1024), (1024, 8)])
def test_thin_frames_equal_oracle(eng, views, h, w):
    mesh, T, _ = views["table"]
    K = _frame_K(h, w)
    db = eng.MeshDB([mesh])
    for flags in (3, 19):
        ref = _oracle("table", mesh, T, K, h, w, flags)
        assert (ref[2] > 0).any()
        _assert_equals_oracle(_render(eng, db, T, K, h, w, flags), ref, flags, f"{h} x {w}")
        o, _ = _render_scene(eng, db, [0, 1], [0], T, K, np.array([2.9], np.float32), [eng.make_lights()], h, w, flags)
        _assert_equals_oracle(o, ref, flags, f"{h} x {w}, scene renderer")


@pytest.mark.parametrize("h,w", [(1025, 8), (8, 1025)])
def test_frames_beyond_the_limit_are_refused_and_nothing_is_written(eng, views, h, w):
    mesh, T, _ = views["table"]
    db = eng.MeshDB([mesh])
    out = torch.full((1, h, w, 8), SENT, device="cuda")
    with pytest.raises(eng.EngineError, match="bad size"):
        eng.raster_render(db, torch.zeros(1, dtype=torch.int32, device="cuda"), torch.from_numpy(T).cuda(), torch.from_numpy(_frame_K(h, w)).cuda(), h, w,
                          3, eng.make_lights(), out, h * w * 8, w * 8, 8, 0, 3, 6)
    inst = torch.full((1, h, w), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(eng.EngineError, match="bad size"):
        eng.raster_render_scene(db, [0, 1], torch.zeros(1, dtype=torch.int32, device="cuda"), torch.from_numpy(T).cuda(),
                                torch.from_numpy(_frame_K(h, w)).cuda(), torch.tensor([2.9], device="cuda"), eng.lights_array([eng.make_lights()], "cuda"),
                                h, w, 3, out, h * w * 8, w * 8, 8, 0, 3, 6, inst)
    torch.cuda.synchronize()
    assert (out == SENT).all() and (inst == -7).all()
