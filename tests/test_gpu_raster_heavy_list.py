"""-m gpu: the packed launch form of raster_tiles (MP_RASTER_HEAVY_LIST = W waves per workgroup: raster_classify packs the reached
(item, tile) pairs into a list, wave j of the grid renders pair j) against the two forms it must equal BIT FOR BIT, on every output byte and on
the job flags: the direct form (MP_RASTER_COMPACT=0) and the compacted strip form (MP_RASTER_HEAVY_LIST=0).

Shapes: frames 40 x 72 (5 x 9 tiles: tiles_x no multiple of 4, 135 pairs = one block of raster_classify) and 64 x 96 (288 pairs = two blocks),
three items of 1 or 4 views, MSAA 1 and 4, W = 1, 2, 4, the output forms fp32, binary16, stem records and stem records with a depth channel
(all with the fused crop).  Meshes: a 384-triangle lathe (synthetic.make_lathe_mesh), a 144-triangle plate and mesh D of
tests/support/raster_limits.py (640 triangles, the database's largest: it sets the list capacities).  Scenes:
  mixed     item 0 the lathe at about 1 m (a silhouette: reached and unreached tiles in one strip), item 1 reached by no view (off-screen poses
            and non-finite poses), item 2 a plate so close that every tile is reached; the lathe's shift is chosen, by the host count of
            tests/raster_emul.cpp, so that the reached-pair count is ODD (no multiple of W = 2 or 4) -- and the device count must equal it
  overflow  item 1 = views O F E F of mesh D, the overflowed view (64 x 96: its large list overflows; 40 x 72: its binned records do) shifted
            so that it does not cover the frame: every tile of the item must still be in the heavy list
  none      no item is reached by any view: a heavy count of zero for the whole launch
  full      every tile of every item is reached: the heavy list fills the shared array (with one view per item that is the whole pair list of
            the workspace) and the light list is empty
and launches of different n_views, one after the other on one workspace (stale counts and stale list entries).
The bookkeeping is read back from the workspace (layout: raster_bin.h, restated in raster_limits.workspace_bytes): heavy + light = pairs, the
two lists partition the pairs, heavy = {job flag != 0}, and the heavy pairs of one classify block are contiguous and in pair order."""
import numpy as np
import pytest
import torch

from tests.support import raster_limits as rl
from tests.support import synthetic as syn

pytestmark = pytest.mark.gpu

SENT = -3.0   # exact in binary16 and bfloat16, never a value
N_ITEMS = 3
WS = ("1", "2", "4")
FORMS = ("fp32", "f16", "records", "records_depth")
CLASSIFY_BLOCK = 256
LATHE, PLATE, MESH_D = 0, 1, 2


@pytest.fixture(scope="module")
def eng():
    from megapose6d_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert engine.device_info()[2].startswith("gfx950")
    return engine


def _small_lathe():
    v, f, c = syn.make_lathe_mesh(seed=1, n_theta=16, n_z=12)
    v = (v / 1000.0).astype(np.float32)
    n = v * np.array([1.0, 1.0, 0.3], np.float32)
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-6)
    return {"vertices": v, "normals": n.astype(np.float32), "colors": (c / 255.0).astype(np.float32), "faces": f.astype(np.int32)}


@pytest.fixture(scope="module")
def meshes():
    m = [_small_lathe(), rl.layered_grid(6, 2, 0.4, 0.002, 0.15, 7), rl.layered_grid(**rl.CASE_D)]
    assert [len(x["faces"]) for x in m] == [384, 144, 640]
    return m


@pytest.fixture(scope="module")
def dbs(eng, meshes):
    """two databases of the same meshes = two workspaces: the launches under test and the reference launches do not disturb each other"""
    return eng.MeshDB(meshes), eng.MeshDB(meshes)


def _K(h, w):
    return np.array([[2.4 * w, 0, w / 2], [0, 2.4 * w, h / 2], [0, 0, 1]], np.float32)


def _lathe_views(V, dx):
    T = np.stack([rl.tilted(70.0 + 10 * i, z) for i, z in enumerate((1.0, 0.8, 1.1, 0.9)[:V])])
    T[:, 0, 3] += np.float32(dx) + np.float32(0.01) * np.arange(V, dtype=np.float32)
    return T


def _nan_pose():
    T = rl.pose_z(0.5)
    T[0, 3] = np.nan
    return T


def _unreached_views(V):
    """off-screen and non-finite poses in turn (one view: off-screen)"""
    return np.stack([rl.pose_z(0.5, x=3.0) if v % 2 == 0 else _nan_pose() for v in range(V)])


def _host_reach(mesh, T, K1, h, w, ns):
    """[n_views, n_tiles] bool: the view has a binned or a large piece in the tile (host count of tests/raster_emul.cpp)"""
    c = rl.bin_counts(mesh, T, np.repeat(K1[None], len(T), 0), h, w, ns)
    return (c["binned"] + c["large"]) > 0, c


def _scene(name, meshes, h, w, V, ns, n_items=N_ITEMS):
    """-> dict(ids [n_items * V], T, K, expect: per item None | 0 | 1 (job flags all 0 / all 1), n_heavy: the host's count or None)"""
    K1 = _K(h, w)
    n_tiles = rl.bin_layout(0, h, w)["n_tiles"]
    n_heavy = None
    if name == "mixed":
        # the lathe's shift: the first candidate whose host count makes the launch's reached-pair count odd
        for dx in (0.0, 0.02, 0.04, 0.06, 0.08, 0.1):
            reach, _ = _host_reach(meshes[LATHE], _lathe_views(V, dx), K1, h, w, ns)
            n_heavy = int(reach.any(0).sum()) + (n_tiles if n_items == 3 else 0)
            if n_heavy % 2 == 1:
                break
        assert n_heavy % 2 == 1, "no candidate shift gives an odd reached-pair count"
        items = [(LATHE, _lathe_views(V, dx), None), (PLATE, _unreached_views(V), 0), (PLATE, np.stack([rl.pose_z(0.5)] * V), 1)]
    elif name == "overflow":
        # host counts.  64 x 96, z = 0.3: 7473 (MSAA 1) / 7677 (MSAA 4) large entries of 6656, 88 of the 96 tiles reached (large-list overflow);
        # 40 x 72, z = 0.7: 4331 / 4392 binned records of 3968, 30 / 31 of the 45 tiles reached (list overflow)
        over = rl.pose_z(0.3 if (h, w) == (64, 96) else 0.7, x=0.09)
        reach, c = _host_reach(meshes[MESH_D], over[None], K1, h, w, ns)
        lay = rl.bin_layout(len(meshes[MESH_D]["faces"]), h, w)
        if (h, w) == (64, 96):
            assert c["n_large"][0] > lay["cap_large"] + 200, "the view's large list should overflow"
        else:
            assert c["n_binned"][0] > lay["cap_list"] + 200, "the view's binned records should overflow"
        assert reach.sum() < n_tiles, "the overflowed view should not cover the frame"
        pat = [over, rl.pose_z(3.0), _nan_pose(), rl.pose_z(3.0)][:V]
        items = [(LATHE, _lathe_views(V, 0.0), None), (MESH_D, np.stack(pat), 1), (PLATE, _unreached_views(V), 0)]
    elif name == "none":
        items = [(LATHE, np.stack([_nan_pose()] * V), 0), (PLATE, _unreached_views(V), 0), (MESH_D, np.stack([rl.pose_z(0.5, x=5.0)] * V), 0)]
        n_heavy = 0
    elif name == "full":
        items = [(PLATE, np.stack([rl.pose_z(z)] * V), 1) for z in (0.5, 0.45, 0.4)]
        n_heavy = n_items * n_tiles
    items = items[:n_items]
    return dict(ids=np.repeat([i[0] for i in items], V).astype(np.int32), T=np.concatenate([i[1] for i in items]).astype(np.float32),
                K=np.repeat(K1[None], len(items) * V, 0), expect=[i[2] for i in items], n_heavy=n_heavy, n_items=len(items))


_crop_cache = {}


def _crop_inputs(eng):
    if not _crop_cache:
        g = torch.Generator().manual_seed(11)
        images = torch.rand(2, 4, 120, 160, generator=g).cuda()
        images[:, 3] = torch.where(images[:, 3] < 0.1, torch.zeros_like(images[:, 3]), 0.3 + images[:, 3])
        _crop_cache.update(obs3=eng.PackedObservation(images[:, :3].contiguous()), obs4=eng.PackedObservation(images),
                           im_ids=torch.tensor([1, 0, 1], dtype=torch.int32).cuda(),
                           boxes=torch.tensor([[20.0, 10, 120, 85], [-10.0, -8, 80, 60], [60.0, 40, 170, 130]]).cuda(),
                           tCR=torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 0.5], [0.1, 0.0, 0.5]]).cuda())
    return _crop_cache


def _launch(eng, db, sc, h, w, V, msaa, form):
    """one launch into a sentinel-poisoned tensor with a margin of 4 pixels and padding channels -> the tensor's bytes (on the host)"""
    ci = _crop_inputs(eng)
    n = sc["n_items"]
    ids, T, K = torch.from_numpy(sc["ids"]).cuda(), torch.from_numpy(sc["T"]).cuda(), torch.from_numpy(sc["K"]).cuda()
    flags = 1 | (16 if msaa == 4 else 0)
    HP, WP = h + 4, w + 4
    if form.startswith("records"):
        depth = form == "records_depth"
        C, nper = (4, 7) if depth else (3, 6)
        mask = (1 << C) - 1
        if depth:
            for v in range(V):
                mask |= 1 << (C + 6 + nper * v)
        n_f32 = bin(mask).count("1")
        R = eng.xrec_elements(n_f32, C + nper * V - n_f32)
        x = torch.full((n, HP, WP, R), SENT, device="cuda", dtype=torch.bfloat16)
        eng.raster_render(db, ids, T, K, h, w, flags | (2 if depth else 0), eng.make_lights(), x, HP * WP * R, WP * R, R, C, C + 3, C + 6 if depth else -1,
                          views_per_item=V, stride_view=nper, crop=(ci["obs4"] if depth else ci["obs3"], ci["im_ids"][:n], ci["boxes"][:n], 0),
                          xrec=(mask, ci["tCR"][:n], 2) if depth else None)
    else:
        Cp = 32
        x = torch.full((n, HP, WP, Cp), SENT, device="cuda", dtype=torch.float16 if form == "f16" else torch.float32)
        eng.raster_render(db, ids, T, K, h, w, flags, eng.make_lights(), x, HP * WP * Cp, WP * Cp, Cp, 3, 6, -1, views_per_item=V, stride_view=6,
                          crop=(ci["obs3"], ci["im_ids"][:n], ci["boxes"][:n], 0))
    torch.cuda.synchronize()
    assert (x[:, h:] == SENT).all() and (x[:, :, w:] == SENT).all(), f"{form}: written below / right of the image"
    assert not (x[:, :h, :w] == SENT).all(dim=-1).any(), f"{form}: a pixel was not written"
    return x.contiguous().view(torch.uint8).cpu()


def _bookkeeping(eng, db, n_items, V, h, w):
    """what raster_classify left in the workspace of the last (compacted) launch on db -> job flags [n_items, n_tiles], light list, heavy list
    in the order the waves take it (entry j = pair of wave j)"""
    n_views = n_items * V
    n_tiles = rl.bin_layout(0, h, w)["n_tiles"]
    ws = db.workspace(n_views, h, w, rl.launch_device())
    addr = eng.raster_job_flags(db, n_views, h, w, rl.launch_device())
    assert addr != 0, "the launch left no job flags"
    off_flags = addr - ws.data_ptr()
    off_list = off_flags - 4 * n_views * n_tiles          # [4 counters][pair list: one int per (view, tile)][job flags]
    assert off_list >= 16 and off_flags + n_items * n_tiles <= ws.numel()
    total = n_items * n_tiles
    flags = ws[off_flags:off_flags + total].cpu().numpy().reshape(n_items, n_tiles)
    counters = ws[off_list - 16:off_list].view(torch.int32).cpu().numpy()
    pairs = ws[off_list:off_list + 4 * total].view(torch.int32).cpu().numpy()
    n_light, n_heavy = int(counters[0]), int(counters[1])
    assert 0 <= n_light and 0 <= n_heavy and n_light + n_heavy == total, (counters.tolist(), total)   # the lists meet without overlap
    return flags, pairs[:n_light], pairs[total - n_heavy:][::-1]


def _check_bookkeeping(flags, light, heavy, sc):
    total = flags.size
    assert np.array_equal(np.sort(np.concatenate([light, heavy])), np.arange(total)), "the two lists do not partition the pairs"
    assert np.array_equal(np.sort(heavy), np.flatnonzero(flags.ravel())), "the heavy pairs are not the pairs whose job flag is set"
    assert set(np.unique(flags).tolist()) <= {0, 1}
    # a classify block's heavy pairs: contiguous, in pair order (neighbouring tiles stay neighbours); the blocks in any order
    blocks = heavy // CLASSIFY_BLOCK
    starts = np.flatnonzero(np.diff(blocks)) + 1
    for seg in np.split(heavy, starts):
        assert (np.diff(seg) > 0).all(), "a block's heavy pairs are not in pair order"
    assert len(np.unique(blocks)) == len(starts) + (1 if len(heavy) else 0), "a block's heavy pairs are not contiguous in the list"
    for item, e in enumerate(sc["expect"]):
        if e is not None:
            assert (flags[item] == e).all(), f"item {item}: expected every job flag {e}"
    if sc["n_heavy"] is not None:
        assert len(heavy) == sc["n_heavy"], (len(heavy), sc["n_heavy"])


def _run_forms(eng, monkeypatch, db, db_ref, sc, h, w, V, msaa, form, ws=WS):
    """direct form and strip form on db_ref, every W on db; all equal bit for bit, the job flags too; the bookkeeping of every W holds"""
    monkeypatch.setenv("MP_RASTER_COMPACT", "0")
    monkeypatch.delenv("MP_RASTER_HEAVY_LIST", raising=False)
    direct = _launch(eng, db_ref, sc, h, w, V, msaa, form)
    monkeypatch.setenv("MP_RASTER_COMPACT", "1")
    monkeypatch.setenv("MP_RASTER_HEAVY_LIST", "0")
    strips = _launch(eng, db_ref, sc, h, w, V, msaa, form)
    flags0, light0, heavy0 = _bookkeeping(eng, db_ref, sc["n_items"], V, h, w)
    _check_bookkeeping(flags0, light0, heavy0, sc)
    assert torch.equal(direct, strips), f"{form}: the strip form differs from the direct form"
    for W in ws:
        monkeypatch.setenv("MP_RASTER_HEAVY_LIST", W)
        got = _launch(eng, db, sc, h, w, V, msaa, form)
        flags, light, heavy = _bookkeeping(eng, db, sc["n_items"], V, h, w)
        assert torch.equal(got, direct), f"{form}, W = {W}: the packed form differs from the direct form"
        assert torch.equal(got, strips), f"{form}, W = {W}: the packed form differs from the strip form"
        assert np.array_equal(flags, flags0), f"{form}, W = {W}: the job flags differ from the strip form's"
        _check_bookkeeping(flags, light, heavy, sc)
    return flags0


CASES = [(s, h, w, V, m) for s in ("mixed", "overflow", "none", "full") for (h, w) in ((40, 72), (64, 96)) for V in (1, 4) for m in (1, 4)]


@pytest.mark.parametrize("scene,h,w,V,msaa", CASES)
def test_packed_form_equals_direct_and_strip_forms(eng, meshes, dbs, monkeypatch, scene, h, w, V, msaa):
    """every output form x every W, bit for bit against the direct and the strip form, and the bookkeeping (module docstring)"""
    db, db_ref = dbs
    sc = _scene(scene, meshes, h, w, V, msaa)
    n_tiles = rl.bin_layout(0, h, w)["n_tiles"]
    for form in FORMS:
        flags = _run_forms(eng, monkeypatch, db, db_ref, sc, h, w, V, msaa, form)
        if scene == "mixed":   # a silhouette: the lathe's item has reached and unreached tiles, some of them in one strip of four
            f0 = flags[0].reshape(-1, (w + 7) // 8)
            pad = np.zeros((f0.shape[0], (-f0.shape[1]) % 4), f0.dtype)
            per_strip = np.concatenate([f0, pad], 1).reshape(f0.shape[0], -1, 4).sum(-1)
            assert ((per_strip > 0) & (per_strip < 4)).any() and 0 < flags[0].sum() < n_tiles
            assert flags.sum() % 2 == 1, "the reached-pair count should be no multiple of W = 2, 4"
        if scene == "overflow":
            hdr = rl.view_headers(db, N_ITEMS * V, h, w)["hdr"]
            assert hdr[V, 2] == 1 and hdr[:V, 2].sum() == 0 and hdr[V + 1:, 2].sum() == 0, hdr[:, 2]
        if scene == "full" and V == 1:   # items = views: the heavy list is the whole pair list of the workspace
            assert flags.sum() == N_ITEMS * V * n_tiles


@pytest.mark.parametrize("W", WS)
def test_launches_of_different_n_views_on_one_workspace(eng, meshes, dbs, monkeypatch, W):
    """full (3 items) -> mixed (2 items) -> none (3 items) -> mixed (3 items) -> full (2 items), back to back on one workspace: each launch's
    counts and lists are its own (nothing of the launch before is taken for a pair), outputs and flags == the direct and the strip form"""
    db, db_ref = dbs
    h, w, V, msaa = 40, 72, 4, 4
    for scene, n_items in (("full", 3), ("mixed", 2), ("none", 3), ("mixed", 3), ("full", 2)):
        sc = _scene(scene, meshes, h, w, V, msaa, n_items)
        _run_forms(eng, monkeypatch, db, db_ref, sc, h, w, V, msaa, "records", ws=(W,))


@pytest.mark.parametrize("value", ["3", "abc", "x1", "1x", "01", " 1", "-1", "8"])
def test_switch_values_other_than_0_1_2_4_are_refused(eng, meshes, dbs, monkeypatch, value):
    """the switch is exactly one of 0 1 2 4: nothing else selects a form silently, in the compacted and in the direct form alike"""
    sc = _scene("none", meshes, 40, 72, 1, 1)
    monkeypatch.setenv("MP_RASTER_HEAVY_LIST", value)
    for compact in ("1", "0"):
        monkeypatch.setenv("MP_RASTER_COMPACT", compact)
        with pytest.raises(Exception, match="MP_RASTER_HEAVY_LIST"):
            _launch(eng, dbs[0], sc, 40, 72, 1, 1, "fp32")


def test_unset_switch_equals_every_form(eng, meshes, dbs, monkeypatch):
    """the default (switch unset: packed where the instance has no scratch, strips elsewhere) at MSAA 4 and 1 == the strip form"""
    db, db_ref = dbs
    for msaa in (4, 1):
        sc = _scene("mixed", meshes, 40, 72, 4, msaa)
        monkeypatch.setenv("MP_RASTER_COMPACT", "1")
        monkeypatch.setenv("MP_RASTER_HEAVY_LIST", "0")
        strips = _launch(eng, db_ref, sc, 40, 72, 4, msaa, "records")
        monkeypatch.delenv("MP_RASTER_HEAVY_LIST")
        got = _launch(eng, db, sc, 40, 72, 4, msaa, "records")
        assert torch.equal(got, strips)
        _check_bookkeeping(*_bookkeeping(eng, db, sc["n_items"], 4, 40, 72), sc)
