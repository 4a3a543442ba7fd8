"""CPU: the arithmetic the HIP rasteriser is built from (megapose6d_amd/csrc/raster_core.h, executed by tests/raster_emul.cpp in the
kernels' own order: tile binning, lane coverage incl. the 32-bit path, shading tasks, 8-bit multisample resolve) against the
independent oracle (oracle/raster.c) -- bit for bit, on crop-like views, MSAA 1 / 4, near-plane clipping, textures with per-pixel
LOD, point lights, large triangles, the list-overflow fallback and arbitrary list order."""
import ctypes as C

import numpy as np
import pytest

from support.emul import CSRC, TESTS, build


@pytest.fixture(scope="module")
def emul():
    lib = build("raster_emul", [TESTS / "raster_emul.cpp", CSRC / "raster_core.h"])
    lib.raster_emul_render.restype = None
    return lib


def _emul_render(lib, mesh, T, K, h, w, flags, lights, cap_list=0, reverse=0):
    from oracle import raster as orr

    v = np.ascontiguousarray(mesh["vertices"], np.float32)
    n = np.ascontiguousarray(mesh["normals"], np.float32)
    c = np.ascontiguousarray(mesh["colors"], np.float32)
    f = np.ascontiguousarray(mesh["faces"], np.int32)
    T = np.ascontiguousarray(T, np.float32).reshape(-1, 16)
    K = np.ascontiguousarray(K, np.float32).reshape(-1, 9)
    nv = T.shape[0]
    out = np.full((nv, h, w, 8), -7.0, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    uv_p, tex_p, tw, th, nl = C.c_void_p(None), C.c_void_p(None), 0, 0, 0
    keep = []
    if mesh.get("uvs") is not None and mesh.get("texture_mips") is not None:
        uv = np.ascontiguousarray(mesh["uvs"], np.float32)
        mips = mesh["texture_mips"]
        flat = np.ascontiguousarray(np.concatenate([lv.reshape(-1) for lv in mips]).astype(np.uint32))
        th, tw = mips[0].shape[:2]
        uv_p, tex_p, nl = p(uv), p(flat), len(mips)
        keep += [uv, flat]
    LL = C.c_longlong
    lib.raster_emul_render(p(v), p(n), p(c), p(f), C.c_int(v.shape[0]), C.c_int(f.shape[0]), C.c_float(orr.mesh_radius(v)), uv_p, tex_p,
                           C.c_int(tw), C.c_int(th), C.c_int(nl), p(T), p(K), C.c_int(nv), C.c_int(h), C.c_int(w), C.c_uint32(flags),
                           C.byref(lights), p(out), LL(h * w * 8), C.c_int(1), LL(0), LL(w * 8), LL(8), C.c_int(0), C.c_int(3), C.c_int(6),
                           C.c_int(cap_list), C.c_int(reverse))
    return out[..., 0:3], out[..., 3:6], out[..., 6], out[..., 7]


def _compare(lib, mesh, T, K, h, w, flags, lights=None, **kw):
    from oracle import raster as orr

    L = lights if lights is not None else orr.lights_struct()
    rgb_o, nrm_o, dep_o = orr.render(mesh, T, K, h, w, flags, L)
    rgb_e, nrm_e, dep_e, pad = _emul_render(lib, mesh, T, K, h, w, flags, L, **kw)
    assert (pad == -7.0).all()                       # the unwritten channel stays untouched
    assert np.array_equal(rgb_e, rgb_o), ("rgb", np.abs(rgb_e - rgb_o).max(), (rgb_e != rgb_o).mean())
    if flags & 1:
        assert np.array_equal(nrm_e, nrm_o), ("normals", (nrm_e != nrm_o).mean())
    if flags & 2:
        assert np.array_equal(dep_e, dep_o), ("depth", np.abs(dep_e - dep_o).max())
    return rgb_o, nrm_o, dep_o


def _poses(n, seed, z=(0.35, 0.7), xy=0.12):
    from tests.support import synthetic as syn

    rng = np.random.RandomState(seed)
    return np.stack([syn.random_pose(rng, z_range=z, xy_frac=xy) for _ in range(n)])


K_FULL = np.array([[605.95, 0, 319.03], [0, 605.0, 249.68], [0, 0, 1]], np.float32)
K_CROP = np.array([[1500.0, 0, 160], [0, 1500.0, 120], [0, 0, 1]], np.float32)


@pytest.mark.parametrize("msaa", [1, 4])
def test_crop_like_views_match_oracle(emul, engine_meshes, msaa):
    T = _poses(3, 1, z=(0.4, 0.6), xy=0.02)
    K = np.repeat(K_CROP[None], 3, 0)
    rgb, nrm, dep = _compare(emul, engine_meshes[0], T, K, 240, 320, 3 | (16 if msaa == 4 else 0))
    assert (dep > 0).mean() > 0.2 and rgb.max() > 0.5
    if msaa == 4:   # silhouette pixels are blended: values that are not multiples of what a single sample could produce exist
        cov_partial = ((rgb > 0).any(-1) & (dep == 0)).mean()
        assert cov_partial > 0, "no partially covered pixel found"


def test_full_frame_view_with_point_lights_and_reverse_list_order(emul, engine_meshes):
    from oracle import raster as orr

    T = _poses(2, 2)
    K = np.repeat(K_FULL[None], 2, 0)
    L = orr.lights_struct((0.1, 0.1, 0.1), orr.POINT_DIRS, [(0.4, 0.4, 0.4)] * 6, [(0.0, 0.01, 0.0)] * 6)
    _compare(emul, engine_meshes[1], T, K, 480, 640, 16, L)
    _compare(emul, engine_meshes[1], T[:1], K[:1], 480, 640, 16 | 1, L, reverse=1)


def test_near_plane_clipping_matches_oracle(emul, engine_meshes):
    """the camera sits so close that the object crosses z = 0.1 m: triangles are clipped (1 and 2 pieces), not dropped"""
    T = _poses(2, 3, z=(0.07, 0.11), xy=0.05)
    K = np.repeat(K_FULL[None], 2, 0)
    for flags in (3, 16 | 3):
        rgb, nrm, dep = _compare(emul, engine_meshes[0], T, K, 240, 320, flags, reverse=1)
        assert (dep > 0).mean() > 0.3
        assert dep[dep > 0].min() >= 0.1 - 1e-6   # nothing nearer than the near plane survives
    # and the clip really happened: some vertices are behind the near plane
    v = engine_meshes[0]["vertices"]
    z = (T[0, :3, :3] @ v.T + T[0, :3, 3:4])[2]
    assert (z < 0.1).any() and (z > 0.1).any()


def test_large_triangles_and_list_overflow_fallback(emul):
    """a 12-triangle box filling the frame: every triangle goes to the per-view 'large' list; then the same with a list capacity of
    zero entries on a dense mesh (overflow -> every tile walks all pieces)"""
    v = np.array([[x, y, z] for x in (-0.1, 0.1) for y in (-0.07, 0.07) for z in (-0.05, 0.05)], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    nrm = v / np.linalg.norm(v, axis=1, keepdims=True)
    col = (v - v.min(0)) / (v.max(0) - v.min(0))
    box = dict(vertices=v, normals=nrm.astype(np.float32), colors=col.astype(np.float32), faces=f)
    T = _poses(2, 5, z=(0.3, 0.45), xy=0.05)
    K = np.repeat(K_FULL[None], 2, 0)
    rgb, _, dep = _compare(emul, box, T, K, 240, 320, 16 | 3)
    assert (dep > 0).mean() > 0.05


def test_overflow_fallback_dense_mesh(emul, engine_meshes):
    T = _poses(1, 6, z=(0.4, 0.5), xy=0.02)
    _compare(emul, engine_meshes[2], T, K_CROP[None], 120, 160, 16 | 3, cap_list=1)


@pytest.mark.parametrize("msaa", [1, 4])
def test_textured_mesh_trilinear_lod_matches_oracle(emul, tmp_path, msaa):
    from megapose6d_amd import mesh_io
    from tests.support import synthetic as syn

    obj = syn.make_textured_object(tmp_path, fmt="obj")
    mesh = mesh_io.load_rigid_object(obj)
    assert mesh.get("uvs") is not None and len(mesh["texture_mips"]) > 3
    T = np.concatenate([_poses(1, 7, z=(0.3, 0.35), xy=0.02), _poses(1, 8, z=(1.2, 1.5), xy=0.05)])   # magnified and minified
    K = np.repeat(K_FULL[None], 2, 0)
    rgb, _, dep = _compare(emul, mesh, T, K, 240, 320, 3 | (16 if msaa == 4 else 0))
    assert (dep[0] > 0).mean() > 0.1 and (dep[1] > 0).mean() > 0.002


def test_anisotropic_filter_is_exercised_and_sharper_than_trilinear_at_grazing_angles(emul, tmp_path):
    """Contract v2.1 (round 6): degree-16 anisotropic filtering (reference panda3d_scene_renderer.py:72) by the EXT_texture_filter_anisotropic
    formula.  A textured object seen at a grazing angle: (i) engine contract == oracle bit for bit (as every textured case), (ii) the
    oracle's isotropic rendering (test hook oracle_set_max_aniso(1) = contract v2) differs on a good share of the covered pixels, and
    (iii) the anisotropic picture keeps more texture contrast (the isotropic level of detail follows the LONG axis of the footprint and
    blurs along the short one)."""
    from megapose6d_amd import mesh_io
    from oracle import raster as orr
    from tests.support import synthetic as syn

    obj = syn.make_textured_object(tmp_path, fmt="obj")
    mesh = mesh_io.load_rigid_object(obj)
    T = _poses(1, 7, z=(0.55, 0.6), xy=0.01)
    a = np.deg2rad(78.0)   # tilt the object's axis towards the camera: its side walls are seen at a grazing angle
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]], np.float32)
    T[0, :3, :3] = Rx @ T[0, :3, :3]
    K = K_FULL[None]
    rgb, _, dep = _compare(emul, mesh, T, K, 240, 320, 3)           # (i)
    lib = orr.lib()
    lib.oracle_set_max_aniso(1)
    try:
        iso, _, _ = orr.render(mesh, T, K, 240, 320, 3)
    finally:
        lib.oracle_set_max_aniso(16)
    cov = dep[0] > 0
    assert cov.mean() > 0.01
    changed = (np.abs(rgb[0] - iso[0]).max(-1) > 0.5 / 255) & cov
    assert changed.sum() > 0.05 * cov.sum(), (changed.sum(), cov.sum())   # (ii)
    gx = lambda im: np.abs(np.diff(im.mean(-1), axis=1))[cov[:, 1:] & cov[:, :-1]].mean()   # noqa: E731
    assert gx(rgb[0]) > gx(iso[0]), (gx(rgb[0]), gx(iso[0]))               # (iii)


def test_non_finite_pose_renders_zeros(emul, engine_meshes):
    T = _poses(2, 9)
    T[1, 0, 0] = np.nan
    K = np.array([[150.0, 0, 48], [0, 150.0, 32], [0, 0, 1]], np.float32)
    rgb, nrm, dep = _compare(emul, engine_meshes[0], T, np.repeat(K[None], 2, 0), 64, 96, 16 | 3)
    assert rgb[1].max() == 0 and dep[1].max() == 0 and rgb[0].max() > 0


def test_msaa_resolve_properties(engine_meshes):
    """interior pixels are identical with and without multisampling; silhouette pixels are blends; depth is sample 0's"""
    from oracle import raster as orr

    T = _poses(1, 10, z=(0.4, 0.5), xy=0.02)
    r1, n1, d1 = orr.render(engine_meshes[0], T, K_CROP[None], 240, 320, 3)
    r4, n4, d4 = orr.render(engine_meshes[0], T, K_CROP[None], 240, 320, 16 | 3)
    q = np.round(r4 * 255)
    assert np.abs(r4 * 255 - q).max() < 1e-3          # still 8-bit values
    same = (r1 == r4).all(-1)
    assert same.mean() > 0.5                          # background + many interior pixels
    cov1, cov4 = (r1 > 0).any(-1), (r4 > 0).any(-1)
    assert cov4.sum() >= cov1.sum()                   # partially covered pixels appear
    edge = cov4 & ~cov1
    assert edge.sum() > 0 and (r4[edge].max(-1) <= r1.max() + 1e-6).all()
