"""GPU: the TSDF kernels (csrc/tsdf.hip) through the C ABI and the wrappers.  mp_tsdf_integrate, mp_tsdf_extract_count and
mp_tsdf_extract against the host emulation built from the same rules header (tests/tsdf_emul.cpp), bit for bit, on the fixtures of the
contract test (tensors of exactly the stated sizes; one call, two calls, view by view; with and without masks, colours and carving;
TCO rows of 12 and 16 floats; 40 different views in one call, more than the 32 the integrate kernel stages at a time, into 48^3 nodes =
432 workgroups, more than the 256 the scan over the workgroups takes at a time; eight nodes, fewer than a wave); the empty, all-inside and all-unobserved volumes; the argument rules (refused before any launch); and an
object reconstructed from rendered depth that the renderer, MeshDataBase, batched_surface and bop_models_info take like any other.
Reads nothing outside the tree."""
import functools

import numpy as np
import pytest
import torch

from tests.support import tsdf as st

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(None)
def _emul(name, carve=True, drop=(), color=True):
    """the emulation's volume and meshes (min_views 1 and 2) of a fixture, computed once"""
    g, views = st.fixture(name)
    vol = st.new_volume(g.dims, color)
    assert st.emul_integrate(vol, g, st.without(views, *drop), carve=carve) == 0
    return vol, {mv: st.emul_extract(vol, g, mv) for mv in (1, 2)}


def _abi_integrate(vol_t, g, views, sel, carve=True, tco_floats=16, mu=None):
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    depth, masks, rgb, K, TCO = st.view_arrays(views, sel)
    TCO = np.ascontiguousarray(TCO[:, :tco_floats])
    n, h, w = depth.shape
    nx, ny, nz = g.dims
    t = [_dev(a) for a in (depth, masks, rgb, K, TCO)]
    ptr = [None if a is None or a.numel() == 0 else a.data_ptr() for a in t]
    rc = _lib.load().mp_tsdf_integrate(vol_t.data_ptr(), nx, ny, nz, int(vol_t.shape[0] == 6), *g.origin, g.voxel, *ptr, tco_floats, n, h, w,
                                       float(g.mu3 if mu is None else mu), st.Z_MIN, int(carve), eng._stream())
    torch.cuda.synchronize()
    return rc


def _abi_extract(vol_t, g, min_views=1):
    """the two entry points on tensors of exactly the counted sizes -> numpy vertices, colors, faces"""
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    lib = _lib.load()
    nx, ny, nz = g.dims
    color = int(vol_t.shape[0] == 6)
    ws = torch.empty(lib.mp_tsdf_extract_workspace_bytes(nx, ny, nz), dtype=torch.uint8, device="cuda")
    totals = torch.full((2,), -5, dtype=torch.int32, device="cuda")
    _lib.check(lib.mp_tsdf_extract_count(vol_t.data_ptr(), nx, ny, nz, color, min_views, totals.data_ptr(), ws.data_ptr(), ws.numel(), eng._stream()))
    nv, nt = totals.tolist()
    v = torch.full((nv, 3), -7.0, dtype=torch.float32, device="cuda")
    c = torch.full((nv, 3), -7.0, dtype=torch.float32, device="cuda")
    f = torch.full((nt, 3), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.mp_tsdf_extract(vol_t.data_ptr(), nx, ny, nz, color, *g.origin, g.voxel, nv, nt, v.data_ptr() if nv else None,
                                   c.data_ptr() if nv else None, f.data_ptr() if nt else None, nv, nt, ws.data_ptr(), ws.numel(), eng._stream()))
    return v.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy()


def _same_bits(a, b, what):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


def _same_mesh(got, want, what):
    for a, b, name in zip(got, want, ("vertices", "colors", "faces")):
        _same_bits(a, b, (what, name))


@pytest.mark.parametrize("name", st.FIXTURES)
def test_entry_points_equal_the_emulation_split_and_unsplit(name):
    g, views = st.fixture(name)
    n = len(views["depth"])
    want_vol, want_mesh = _emul(name)
    for splits in ([slice(0, n)], [slice(0, n // 2), slice(n // 2, n)], [slice(v, v + 1) for v in range(n)]):
        vol = _dev(st.new_volume(g.dims, True))
        for sel in splits:
            assert _abi_integrate(vol, g, views, sel) == 0
        _same_bits(vol, want_vol, (name, len(splits), "volume"))
    for min_views in (1, 2):
        _same_mesh(_abi_extract(vol, g, min_views), want_mesh[min_views], (name, min_views))
    assert len(want_mesh[1][2]) > 0


def test_the_second_rounds_of_the_view_and_scan_loops_are_what_is_tested():
    """the sizes that make `many` and `tiny` worth their names, stated against the kernels' constants (csrc/tsdf_views.h: kViewChunk = 32,
    csrc/tsdf.hip: kTsdfBlock = 256): a partial last round of views, a non-finite view in it, vertices owned by nodes past the first round of the scan"""
    g, views = st.fixture("many")
    n, nodes = len(views["depth"]), int(np.prod(g.dims))
    assert 32 < n < 64 and n % 32 != 0 and not np.isfinite(views["K"][35]).all() and -(-nodes // 256) > 256
    vol, mesh = _emul("many")
    assert len({views["TCO"][v].tobytes() for v in range(n)}) == n                       # no two views alike
    later = st.new_volume(g.dims, True)
    assert st.emul_integrate(later, g, views, slice(32, n)) == 0 and st.counts_of(later).max() > 0   # the second round contributes
    v, _, f = mesh[1]
    first_round_top = g.origin[2] + g.voxel * (256 * 256 // (g.dims[0] * g.dims[1]))     # z of the last node of the scan's first round
    assert (v[:, 2] > first_round_top + g.voxel).sum() > 1000 and len(f) > 10000
    assert int(np.prod(st.fixture("tiny")[0].dims)) < 64


@pytest.mark.parametrize("name", ["sphere", "awkward"])
def test_variants_of_the_inputs(name):
    from megapose6d_amd import engine as eng

    g, views = st.fixture(name)
    for var in (dict(carve=False), dict(drop=("masks",)), dict(drop=("rgb",)), dict(drop=("masks", "rgb"), carve=False), dict(color=False)):
        want_vol, want_mesh = _emul(name, **{k: (tuple(v) if k == "drop" else v) for k, v in var.items()})
        vv = st.without(views, *var.get("drop", ()))
        vol = _dev(st.new_volume(g.dims, var.get("color", True)))
        assert _abi_integrate(vol, g, vv, slice(None), carve=var.get("carve", True), tco_floats=12) == 0         # rows of 12 floats
        _same_bits(vol, want_vol, (name, var))
        _same_mesh(_abi_extract(vol, g), want_mesh[1], (name, var))
        # the wrappers: bool masks, [n,4,4] poses
        vol2 = eng.tsdf_volume(g.dims, var.get("color", True), "cuda")
        eng.tsdf_integrate(vol2, g.origin, g.voxel, _dev(vv["depth"]), _dev(vv["K"]), _dev(vv["TCO"]), None if vv["masks"] is None else _dev(vv["masks"]) != 0,
                           _dev(vv["rgb"]), carve=var.get("carve", True), z_min=st.Z_MIN)
        _same_bits(vol2, want_vol, (name, var, "wrapper"))
        _same_mesh(eng.tsdf_extract(vol2, g.origin, g.voxel, 2), want_mesh[2], (name, var, "wrapper"))


def test_a_field_set_directly_and_the_worked_example():
    for color in (True, False):
        vol = st.plane_volume(color=color)
        for min_views in (1, 2, 3):
            _same_mesh(_abi_extract(_dev(vol), st.ODD_GRID, min_views), st.emul_extract(vol, st.ODD_GRID, min_views), (color, min_views))
    vol, g = st.corner_volume()
    v, c, f = _abi_extract(_dev(vol), g)
    assert v.tolist() == st.CORNER_VERTICES and f.tolist() == st.CORNER_FACES and (c == 1).all()


def test_empty_all_inside_and_all_unobserved_volumes():
    from megapose6d_amd.onboarding import TsdfVolume

    g = st.ODD_GRID
    empty = _dev(st.new_volume(g.dims, True))
    assert [len(a) for a in _abi_extract(empty, g)] == [0, 0, 0]
    assert _abi_integrate(empty, g, st.sphere_views(), slice(0, 0)) == 0 and not bool(empty.view(torch.int32).any())
    inside = st.new_volume(g.dims, False)
    inside[0], inside[1] = -1.0, np.ones(inside[1].shape, np.int32).view(np.float32)
    assert [len(a) for a in _abi_extract(_dev(inside), g)] == [0, 0, 0]
    assert [len(a) for a in _abi_extract(_dev(inside), g, min_views=2)] == [0, 0, 0]          # now all unobserved
    inside[0, 4, 8, 16] = 1.0                                                                 # one outside node: its 14 edges, 24 triangles
    got = _abi_extract(_dev(inside), g)
    _same_mesh(got, st.emul_extract(inside, g), "one node")
    assert len(got[0]) == 14 and len(got[2]) == 24
    tv = TsdfVolume(g.origin, g.voxel, g.dims, color=False)
    assert int(tv.counts.sum()) == 0 and bool(torch.isnan(tv.field).all()) and len(tv.extract()["faces"]) == 0
    views = st.sphere_views()
    tv.integrate(views["depth"], views["K"], views["TCO"], masks=views["masks"])
    _same_bits(tv.volume, _emul("odd", color=False)[0], "TsdfVolume")
    mesh = tv.extract()
    _same_bits(mesh["vertices"], _emul("odd", color=False)[1][1][0], "TsdfVolume.extract")
    assert mesh["normals"].shape == mesh["vertices"].shape and mesh["normals"].dtype == np.float32
    tv.reset()
    assert int(tv.counts.sum()) == 0 and not bool(tv.volume.view(torch.int32).any())


def test_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    lib = _lib.load()
    g, views = st.fixture("sphere")
    depth, masks, rgb, K, TCO = (_dev(a) for a in st.view_arrays(views, slice(0, 2)))
    vol = torch.zeros(6, 8, 8, 8, dtype=torch.float32, device="cuda")
    s = eng._stream()
    nan, inf = float("nan"), float("inf")

    def integrate(vol=vol.data_ptr(), dims=(8, 8, 8), origin=(-0.04, -0.04, -0.04), voxel=0.01, depth=depth.data_ptr(), K=K.data_ptr(),
                  TCO=TCO.data_ptr(), tco=16, n=2, h=st.H, w=st.W, mu=0.03, z_min=0.0):
        return lib.mp_tsdf_integrate(vol, *dims, 1, *origin, voxel, depth, masks.data_ptr(), rgb.data_ptr(), K, TCO, tco, n, h, w, mu, z_min, 1, s)

    for bad in (dict(dims=(1, 8, 8)), dict(dims=(8, 513, 8)), dict(dims=(512, 512, 513)), dict(voxel=0.0), dict(voxel=nan), dict(voxel=inf),
                dict(voxel=-0.01), dict(origin=(0.0, nan, 0.0)), dict(mu=0.0), dict(mu=-1.0), dict(mu=inf), dict(mu=nan), dict(z_min=-1.0),
                dict(z_min=nan), dict(n=-1), dict(tco=9), dict(h=0), dict(w=8193), dict(vol=None), dict(depth=None), dict(K=None), dict(TCO=None)):
        assert integrate(**bad) != 0, bad
    assert b"null pointer" in lib.mp_last_error()
    torch.cuda.synchronize()
    assert not bool(vol.view(torch.int32).any())
    assert lib.mp_tsdf_volume_bytes(8, 8, 8, 1) == 6 * 512 * 4 and lib.mp_tsdf_volume_bytes(8, 8, 8, 0) == 2 * 512 * 4
    assert lib.mp_tsdf_volume_bytes(1, 8, 8, 0) == 0 and lib.mp_tsdf_volume_bytes(512, 512, 513, 0) == 0 and lib.mp_tsdf_volume_bytes(512, 512, 512, 0) == 2 ** 30
    assert lib.mp_tsdf_extract_workspace_bytes(8, 1, 8) == 0 and lib.mp_tsdf_extract_workspace_bytes(8, 8, 8) > 0
    assert integrate(n=0) == 0 and integrate(n=0, vol=None, depth=None, K=None, TCO=None) == 0                          # n = 0: a no-op
    assert integrate() == 0
    torch.cuda.synchronize()
    assert bool(vol.view(torch.int32).any())
    # extraction, on the worked example
    cvol, cg = st.corner_volume()
    cvol = _dev(cvol)
    need = lib.mp_tsdf_extract_workspace_bytes(2, 2, 2)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    totals = torch.full((2,), -5, dtype=torch.int32, device="cuda")

    def count(vol=cvol.data_ptr(), dims=(2, 2, 2), min_views=1, t=totals.data_ptr(), wsp=ws.data_ptr(), wsn=need):
        return lib.mp_tsdf_extract_count(vol, *dims, 0, min_views, t, wsp, wsn, s)

    assert count(vol=None) != 0 and count(t=None) != 0 and count(wsp=None) != 0 and count(dims=(2, 1, 2)) != 0 and count(min_views=0) != 0
    assert count(wsn=need - 1) != 0 and b"needed" in lib.mp_last_error()
    assert count(wsp=ws.data_ptr() + 4, wsn=need + 12) != 0 and b"aligned" in lib.mp_last_error()                        # large enough, misaligned
    torch.cuda.synchronize()
    assert totals.tolist() == [-5, -5] and not bool(ws.any())
    assert count() == 0 and totals.tolist() == [7, 6]
    v = torch.full((7, 3), -7.0, device="cuda")
    c = torch.full((7, 3), -7.0, device="cuda")
    f = torch.full((6, 3), -7, dtype=torch.int32, device="cuda")

    def extract(vol=cvol.data_ptr(), dims=(2, 2, 2), voxel=1.0, nv=7, nt=6, vp=v.data_ptr(), cp=c.data_ptr(), fp=f.data_ptr(), cap_v=7, cap_t=6,
                wsp=ws.data_ptr(), wsn=need):
        return lib.mp_tsdf_extract(vol, *dims, 0, 0.0, 0.0, 0.0, voxel, nv, nt, vp, cp, fp, cap_v, cap_t, wsp, wsn, s)

    assert extract(vol=None) != 0 and extract(vp=None) != 0 and extract(cp=None) != 0 and extract(fp=None) != 0 and extract(wsp=None) != 0
    assert extract(cap_v=6) != 0 and b"capacity" in lib.mp_last_error()
    assert extract(cap_t=5) != 0 and extract(nv=-1) != 0 and extract(nt=-1) != 0 and extract(voxel=0.0) != 0 and extract(voxel=nan) != 0
    assert extract(dims=(2, 2, 1)) != 0 and extract(wsn=need - 1) != 0 and extract(wsp=ws.data_ptr() + 4, wsn=need + 12) != 0
    torch.cuda.synchronize()
    assert bool((v == -7).all()) and bool((c == -7).all()) and bool((f == -7).all())
    assert extract(nv=0, nt=0, vp=None, cp=None, fp=None, cap_v=0, cap_t=0) == 0                                         # nothing to write: a no-op
    assert extract() == 0
    assert v.tolist() == st.CORNER_VERTICES and f.tolist() == st.CORNER_FACES and bool((c == 1).all())
    with pytest.raises(eng.EngineError):
        eng.tsdf_volume((1, 8, 8), True, "cuda")
    with pytest.raises(eng.EngineError):
        eng.tsdf_integrate(vol, (0, 0, 0), 0.01, depth, K, TCO, masks=masks[:, :5])
    with pytest.raises(eng.EngineError):
        eng.tsdf_extract(vol.double(), (0, 0, 0), 0.01)


def test_reconstructed_object_end_to_end(tmp_path):
    """depth of an icosphere rendered from the eight fixture cameras -> reconstruct_object at 32 nodes -> both objects rendered from a
    ninth camera.  The median |dz| over the pixels hit in both is at most 1 voxel: it follows from the vertex condition of the contract
    test (every vertex within 0.6 voxel of the sphere along the normal; half of a disc's pixels have normals within 45 degrees of the
    view axis, where that becomes at most 0.85 voxel along z; faceting adds about 0.01 voxel)."""
    from megapose6d_amd import RigidObject, RigidObjectDataset, mesh_io, onboarding
    from megapose6d_amd import evaluation as ev
    from megapose6d_amd.mesh_db import MeshDataBase
    from megapose6d_amd.renderer import Panda3dBatchRenderer

    v, f = st.icosphere()
    original = RigidObject("ico", mesh_io.write_ply(tmp_path / "ico.ply", v, f), mesh_units="m")
    renderer = Panda3dBatchRenderer(RigidObjectDataset([original]))
    views = st.sphere_views()
    K, TCO = _dev(views["K"]), _dev(views["TCO"])
    depth = renderer.render_depth(["ico"] * 8, TCO, K, (st.H, st.W))
    assert depth.shape == (8, st.H, st.W) and bool((depth > 0).any())
    masks = depth > 0
    rec = onboarding.reconstruct_object("ico_rec", depth, K, TCO, masks=masks, resolution=32, out_dir=tmp_path / "rec")
    assert rec.label == "ico_rec" and str(rec.mesh_path).endswith("rec/ico_rec.ply") and rec.scale == 1.0
    _, voxel, dims = onboarding.volume_for_views(depth, K, TCO, masks, resolution=32)
    assert max(dims) == 32
    mesh = mesh_io.read_ply(rec.mesh_path)
    rep = st.mesh_report(mesh["vertices"], mesh["faces"])
    assert rep["directed_once"] and rep["reverse_present"] and rep["euler"] == 2 and rep["volume"] > 0 and mesh["colors"] is not None
    ds = RigidObjectDataset([original, rec])
    both = Panda3dBatchRenderer(ds)
    held_out = _dev(st.look_at((0.1, -0.3, 0.2)).astype(np.float32)[None].repeat(2, 0))
    d = both.render_depth(["ico", "ico_rec"], held_out, K[:2], (st.H, st.W))
    hit = (d[0] > 0) & (d[1] > 0)
    assert bool((d[0] > 0).any()) and bool((d[1] > 0).any()) and int(hit.sum()) > 100
    dz = (d[0] - d[1]).abs()[hit]
    print(f"voxel {voxel * 1e3:.3f} mm, {int(hit.sum())} pixels hit in both, median |dz| {float(dz.median()) / voxel:.3f} voxel, max {float(dz.max()) / voxel:.3f} voxel")
    assert float(dz.median()) <= voxel
    mesh_db = MeshDataBase.from_object_ds(ds)
    info = ev.bop_models_info(ev.model_info(mesh_db.batched(n_sym=4).cuda()), scale=1.0)
    print("diameters", info["ico"]["diameter"], info["ico_rec"]["diameter"])
    assert abs(info["ico_rec"]["diameter"] - 0.1) <= 2 * voxel and abs(info["ico"]["diameter"] - 0.1) <= 1e-3
    surf = mesh_db.batched_surface(256)
    assert surf.points.shape == (2, 256, 3) and bool(torch.isfinite(surf.points).all())
    r = surf.points[1].norm(dim=1)
    assert float((r - st.SPHERE_R).abs().max()) <= voxel                                     # the vertex condition again, on surface samples
    with pytest.raises(ValueError, match="surface is empty"):
        onboarding.reconstruct_object("nothing", depth, K, TCO, masks=masks, resolution=32, out_dir=tmp_path / "rec", min_views=9)
