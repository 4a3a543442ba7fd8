"""GPU: the texture-atlas kernels (csrc/texture_bake.hip) through the C ABI and the wrappers.  mp_texture_atlas_uvs and mp_texture_bake
against the host emulation built from the same rules header (tests/texture_bake_emul.cpp), every byte, with canary words around both
outputs: the icosphere under the sphere's views in both modes, with and without masks and vertex colours, at B = 8 and 16; one and
two triangles (B = 64), 7 (B = 32) and 400 (B = 4: 32 triangles a workgroup); 40 views (two staging rounds, the last one partial,
a non-finite K in it); awkward views; 1 x 1 frames; no view at all; a mesh with a zero-area triangle, non-finite vertices and face
indices out of range.  The argument rules (refused before any launch), determinism, and the point of it all: a reconstructed object
with a baked texture renders closer to the truth than the same object with vertex colours.  Reads nothing outside the tree."""
import functools

import numpy as np
import pytest
import torch

from tests.support import texture_bake as tb

pytestmark = pytest.mark.gpu

CANARY = 0x5C
PAD = 256


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(None)
def _case(name):
    """-> vertices, faces, colours, views, S of a named case"""
    v, f, c = tb.ico_mesh()
    if name in ("ico256", "ico512"):
        return v, f, c, tb.sphere_views(), int(name[3:])
    if name in ("t1", "t2", "t7", "t400"):
        vv, ff, cc = tb.single_triangles(int(name[1:]))
        return vv, ff, cc, tb.sphere_views(), 64
    if name == "many":
        return v, f, c, tb.many_views(), 256
    if name == "awkward":
        return v, f, c, tb.awkward_views(), 256
    if name == "pixel":
        return v, f, c, tb.one_pixel_views(), 256
    if name == "broken":
        bv, bf, bc, _ = tb.broken_mesh()
        return bv, bf, bc, tb.sphere_views(), 256
    raise ValueError(name)


@functools.lru_cache(None)
def _emul(name, masks=True, colors=True, best_view=False, n=None):
    v, f, c, views, S = _case(name)
    return tb.emul_bake(v, f, views, S, colors=c if colors else None, masks=masks, best_view=best_view, sel=slice(0, n))


def _abi_bake(name, masks=True, colors=True, best_view=False, n=None, tco_floats=16):
    """mp_texture_bake on outputs with PAD canary bytes on either side -> rc, texels, seen (numpy), canaries intact"""
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    v, f, c, views, S = _case(name)
    v, f, c, depth, m, rgb, K, TCO = tb.bake_arrays(v, f, views, c if colors else None, slice(0, n), masks)
    TCO = np.ascontiguousarray(TCO[:, :tco_floats])
    nv, h, w = depth.shape
    t = [_dev(a) for a in (v, f, c, depth, m, rgb, K, TCO)]
    ptr = [None if a is None or a.numel() == 0 else a.data_ptr() for a in t]
    buf_t = torch.full((PAD + S * S * 4 + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    buf_s = torch.full((PAD + S * S + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    rc = _lib.load().mp_texture_bake(ptr[0], len(v), ptr[1], len(f), ptr[2], ptr[3], ptr[4], ptr[5], ptr[6], ptr[7], tco_floats, nv, h, w, S,
                                     tb.DEPTH_TOL, tb.COS_MIN, tb.Z_MIN, int(best_view), buf_t.data_ptr() + PAD, buf_s.data_ptr() + PAD, eng._stream())
    torch.cuda.synchronize()
    bt, bs = buf_t.cpu().numpy(), buf_s.cpu().numpy()
    intact = all((edge == CANARY).all() for edge in (bt[:PAD], bt[-PAD:], bs[:PAD], bs[-PAD:]))
    return rc, bt[PAD:-PAD].reshape(S, S, 4), bs[PAD:-PAD].reshape(S, S), intact


def _same(got, want, what):
    rc, texels, seen, intact = got
    assert rc == 0 and intact, what
    assert np.array_equal(seen, want[1]), (what, "seen", int((seen != want[1]).sum()))
    assert np.array_equal(texels, want[0]), (what, "texels", int((texels != want[0]).any(-1).sum()))


@pytest.mark.parametrize("name", ["ico256", "ico512"])
def test_bake_equals_the_emulation_in_every_mode(name):
    for best_view in (False, True):
        for masks in (True, False):
            for colors in (True, False):
                kw = dict(masks=masks, colors=colors, best_view=best_view)
                _same(_abi_bake(name, **kw), _emul(name, **kw), (name, kw))
    texels, seen = _emul(name)
    assert seen.max() >= 2 and (seen == 0).any() and not np.array_equal(texels, _emul(name, best_view=True)[0])


@pytest.mark.parametrize("name,T,B", [("t1", 1, 64), ("t2", 2, 64), ("t7", 7, 32), ("t400", 400, 4)])
def test_block_sizes_and_the_last_block(name, T, B):
    from megapose6d_amd import engine as eng

    v, f, c, views, S = _case(name)
    assert len(f) == T and eng.texture_atlas_block(T, S) == B == tb.emul_block(T, S)
    want = _emul(name)
    _same(_abi_bake(name), want, name)
    _same(_abi_bake(name, tco_floats=12), want, (name, "rows of 12 floats"))
    texels, seen = want
    assert (seen > 0).any()                                            # the triangles face camera 0: something is baked from a view
    t, _, _ = tb.chart_coordinates(T, S)
    assert (texels[t < 0] == 0).all() and (seen[t < 0] == 0).all() and (texels[t >= 0][:, 3] == 255).all()
    if T % 2:                                                          # the upper half of the last block holds no triangle
        last = (T // 2 % (S // B)) * B, (T // 2 // (S // B)) * B
        assert (t[last[1]:last[1] + B, last[0]:last[0] + B] < 0).sum() == B * (B - 1) // 2
    uvs = eng.texture_atlas_uvs(T, S)
    torch.cuda.synchronize()
    assert uvs.dtype == torch.float32 and np.array_equal(uvs.cpu().numpy(), tb.emul_uvs(T, S))


def test_uvs_equal_the_emulation_with_canaries():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    for T, S in ((1280, 256), (1280, 512), (3, 64), (512, 64)):
        buf = torch.full((64 + T * 6 + 64,), -7.0, dtype=torch.float32, device="cuda")
        assert _lib.load().mp_texture_atlas_uvs(T, S, buf.data_ptr() + 256, eng._stream()) == 0
        got = buf.cpu().numpy()
        assert (got[:64] == -7).all() and (got[-64:] == -7).all()
        assert np.array_equal(got[64:-64].reshape(T, 3, 2), tb.emul_uvs(T, S)), (T, S)


def test_more_views_than_a_staging_round():
    """40 views against the kernel's 32 a round (csrc/tsdf_views.h: kViewChunk): a partial last round with a non-finite K in it;
    the views past the first round contribute, so a round dropped or read twice shows"""
    v, f, c, views, S = _case("many")
    n = len(views["depth"])
    assert 32 < n < 64 and n % 32 != 0 and not np.isfinite(views["K"][35]).all()
    want = _emul("many")
    assert not np.array_equal(want[1], _emul("many", n=32)[1])
    _same(_abi_bake("many"), want, "many")
    _same(_abi_bake("many", best_view=True), _emul("many", best_view=True), "many, best view")
    _same(_abi_bake("many", n=32), _emul("many", n=32), "exactly one round")
    _same(_abi_bake("many", n=33), _emul("many", n=33), "one view in the second round")


@pytest.mark.parametrize("name", ["awkward", "pixel"])
def test_awkward_views_and_one_pixel_frames(name):
    for masks in (True, False):
        want = _emul(name, masks=masks)
        _same(_abi_bake(name, masks=masks), want, (name, masks))
    assert (_emul(name)[1] > 0).any() and (_emul(name)[1] == 0).any()


def test_no_view_is_all_fallback():
    from megapose6d_amd import engine as eng

    v, f, c, views, S = _case("ico256")
    for colors in (True, False):
        want = _emul("ico256", colors=colors, n=0)
        _same(_abi_bake("ico256", colors=colors, n=0), want, ("n = 0", colors))
        assert (want[1] == 0).all()
    white = _emul("ico256", colors=False, n=0)[0]
    assert (white[white[..., 3] == 255] == 255).all()
    empty = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device="cuda")   # noqa: E731
    texels, seen = eng.texture_bake(_dev(v), _dev(f), empty(0, 4, 6), empty(0, 3, 3), empty(0, 4, 4), None, empty(0, 4, 6, 3, dt=torch.uint8), S,
                                    colors=_dev(c))
    assert np.array_equal(texels.cpu().numpy(), _emul("ico256", n=0)[0]) and not bool(seen.any())


def test_broken_faces_bake_unseen_and_touch_nothing():
    v, f, c, unseen = tb.broken_mesh()
    S = 256
    got = _abi_bake("broken")
    _same(got, _emul("broken"), "broken")
    t, _, _ = tb.chart_coordinates(len(f), S)
    seen = got[2]
    assert len(unseen) >= 6 and all((seen[t == k] == 0).all() for k in unseen)
    assert (seen[(t >= 0) & ~np.isin(t, unseen)] > 0).mean() > 0.9
    for k in (30, 31, 32):                                             # an index out of range: white, its colours are not addressed either
        assert (got[1][t == k] == 255).all()
    _same(_abi_bake("broken", colors=False, best_view=True), _emul("broken", colors=False, best_view=True), "broken, best view")


def test_wrapper_takes_bool_masks_and_4x4_poses():
    from megapose6d_amd import engine as eng

    v, f, c, views, S = _case("ico256")
    texels, seen = eng.texture_bake(_dev(v), _dev(f), _dev(views["depth"]), _dev(views["K"]), _dev(views["TCO"]), _dev(views["masks"]) != 0,
                                    _dev(views["rgb"]), S, colors=_dev(c), depth_tol=tb.DEPTH_TOL, cos_min=tb.COS_MIN, z_min=tb.Z_MIN)
    want = _emul("ico256")
    assert texels.shape == (S, S, 4) and texels.dtype == torch.uint8 and seen.shape == (S, S) and seen.dtype == torch.uint8
    assert np.array_equal(texels.cpu().numpy(), want[0]) and np.array_equal(seen.cpu().numpy(), want[1])
    with pytest.raises(eng.EngineError):
        eng.texture_bake(_dev(v), _dev(f), _dev(views["depth"]), _dev(views["K"]), _dev(views["TCO"]), None, _dev(views["rgb"])[:, :5], S)
    with pytest.raises(eng.EngineError):
        eng.texture_bake(_dev(v), _dev(f), _dev(views["depth"]), _dev(views["K"]), _dev(views["TCO"]), None, None, S)
    with pytest.raises(eng.EngineError):
        eng.texture_bake(_dev(v), _dev(f), _dev(views["depth"]), _dev(views["K"]), _dev(views["TCO"]), None, _dev(views["rgb"]), 64)   # do not fit
    with pytest.raises(eng.EngineError):
        eng.texture_atlas_uvs(0, 64)


def test_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    lib = _lib.load()
    v, f, c, views, _ = _case("ico256")
    S = 256
    v, f, c, depth, m, rgb, K, TCO = (_dev(a) for a in tb.bake_arrays(v, f, views, c))
    n, h, w = depth.shape
    texels = torch.full((S, S, 4), CANARY, dtype=torch.uint8, device="cuda")
    seen = torch.full((S, S), CANARY, dtype=torch.uint8, device="cuda")
    uvs = torch.full((len(f), 3, 2), -7.0, device="cuda")
    s = eng._stream()
    nan, inf = float("nan"), float("inf")

    def bake(vp=v.data_ptr(), V=len(v), fp=f.data_ptr(), T=len(f), cp=c.data_ptr(), dp=depth.data_ptr(), mp=m.data_ptr(), rp=rgb.data_ptr(),
             kp=K.data_ptr(), tp=TCO.data_ptr(), tco=16, n=n, h=h, w=w, size=S, tol=tb.DEPTH_TOL, cos_min=0.2, z_min=1e-3, out=texels.data_ptr(),
             sn=seen.data_ptr()):
        return lib.mp_texture_bake(vp, V, fp, T, cp, dp, mp, rp, kp, tp, tco, n, h, w, size, tol, cos_min, z_min, 0, out, sn, s)

    for bad in (dict(T=0), dict(T=-1), dict(V=-1), dict(size=0), dict(size=32), dict(size=96), dict(size=255), dict(size=16384), dict(size=-256),
                dict(size=64), dict(tol=0.0), dict(tol=-1.0), dict(tol=nan), dict(tol=inf), dict(cos_min=-0.1), dict(cos_min=1.0), dict(cos_min=nan),
                dict(z_min=-1.0), dict(z_min=nan), dict(z_min=inf), dict(n=-1), dict(tco=9), dict(h=0), dict(w=8193), dict(vp=None), dict(fp=None),
                dict(dp=None), dict(rp=None), dict(kp=None), dict(tp=None), dict(out=None), dict(sn=None), dict(out=texels.data_ptr() + 2),
                dict(vp=v.data_ptr() + 1), dict(dp=depth.data_ptr() + 2)):
        assert bake(**bad) != 0, bad
    assert b"aligned" in lib.mp_last_error()
    assert bake(size=64) != 0 and b"do not fit" in lib.mp_last_error()            # 1 280 triangles want 640 blocks, 64 / 4 squared is 256
    for bad in ((0, S, uvs.data_ptr()), (-1, S, uvs.data_ptr()), (len(f), 100, uvs.data_ptr()), (len(f), 64, uvs.data_ptr()), (len(f), S, None),
                (len(f), S, uvs.data_ptr() + 1), (len(f), 0, uvs.data_ptr()), (len(f), 16384, uvs.data_ptr())):
        assert lib.mp_texture_atlas_uvs(bad[0], bad[1], bad[2], s) != 0, bad
    assert lib.mp_texture_atlas_block(0, S) == 0 and lib.mp_texture_atlas_block(2, 100) == 0 and lib.mp_texture_atlas_block(513, 64) == 0
    assert lib.mp_texture_atlas_block(512, 64) == 4 and lib.mp_texture_atlas_block(1, 8192) == 64
    torch.cuda.synchronize()
    assert bool((texels == CANARY).all()) and bool((seen == CANARY).all()) and bool((uvs == -7).all())
    assert bake(mp=None) == 0 and bake(cp=None) == 0 and bake(n=0, dp=None, rp=None, kp=None, tp=None, mp=None, h=0, w=0) == 0
    assert bake() == 0 and lib.mp_texture_atlas_uvs(len(f), S, uvs.data_ptr(), s) == 0
    torch.cuda.synchronize()
    want = _emul("ico256")
    assert np.array_equal(texels.cpu().numpy(), want[0]) and np.array_equal(seen.cpu().numpy(), want[1])
    assert np.array_equal(uvs.cpu().numpy(), tb.emul_uvs(len(f), S))


def test_two_calls_and_dirty_outputs_give_the_same_bytes():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    v, f, c, views, S = _case("many")
    args = [_dev(a) for a in tb.bake_arrays(v, f, views, c)]
    n, h, w = args[3].shape
    results = []
    torch.manual_seed(0)
    for fill in ("zeros", "dirty", "dirty"):
        big = torch.zeros(3, S + 8, S * 4 + 64, dtype=torch.uint8, device="cuda") if fill == "zeros" else \
            torch.randint(0, 256, (3, S + 8, S * 4 + 64), dtype=torch.uint8, device="cuda")
        flat = big.reshape(-1)
        texels = flat[1028:1028 + S * S * 4]                                # 4-byte aligned, not 256
        seen = flat[1028 + S * S * 4 + 7:1028 + S * S * 4 + 7 + S * S]      # not aligned at all
        before = flat.clone()
        assert _lib.load().mp_texture_bake(args[0].data_ptr(), len(v), args[1].data_ptr(), len(f), *(a.data_ptr() for a in args[2:]), 16, n, h, w, S,
                                           tb.DEPTH_TOL, tb.COS_MIN, tb.Z_MIN, 0, texels.data_ptr(), seen.data_ptr(), eng._stream()) == 0
        torch.cuda.synchronize()
        results.append((texels.clone(), seen.clone()))
        touched = flat != before
        touched[1028:1028 + S * S * 4] = False
        touched[1028 + S * S * 4 + 7:1028 + S * S * 4 + 7 + S * S] = False
        assert not bool(touched.any())
    for texels, seen in results[1:]:
        assert torch.equal(texels, results[0][0]) and torch.equal(seen, results[0][1])
    want = _emul("many")
    assert np.array_equal(results[0][0].cpu().numpy().reshape(S, S, 4), want[0]) and np.array_equal(results[0][1].cpu().numpy().reshape(S, S), want[1])


def test_a_baked_texture_brings_a_light_mesh_closer_to_the_truth(tmp_path):
    """The point of the feature.  A sphere whose colour is a 3-D checker of 8 mm period (cells of 4 mm), seen by 24 analytic views of
    120 x 160 at f = 200, reconstructed at 48 nodes and decimated to at most 1 500 faces (edges of about 7 mm: the vertex colours
    cannot carry the pattern), once with texture_size = 512 and once without.  Both are rendered under ambient light at a held-out
    pose; the mean absolute RGB difference to the analytic image over the pixels both cover must be lower for the textured one.
    Rehearsed on the CPU with the emulations and the oracle's rasteriser: 46.8 levels vertex-coloured, 31.5 textured (the checker
    itself as the texture of this mesh scores 25.2: the cells are 2.7 pixels wide, so most of what is left is how a binary pattern is filtered).
    MEASURED on the MI355X: 3 282 pixels covered by both, 46.78 levels vertex-coloured, 31.51 textured."""
    from megapose6d_amd import RigidObjectDataset, mesh_io, onboarding
    from megapose6d_amd.renderer import Panda3dBatchRenderer
    from megapose6d_amd.types import Panda3dLightData
    from tests.support import tsdf as st

    views = tb.checker_views(tb.checker_cameras(24))
    depth, K, TCO, masks, rgb = (_dev(views[k]) for k in ("depth", "K", "TCO", "masks", "rgb"))
    kw = dict(masks=masks, rgb=rgb, resolution=48, keep_largest=True, max_faces=1500)
    plain = onboarding.reconstruct_object("checker_plain", depth, K, TCO, out_dir=tmp_path / "plain", **kw)
    textured = onboarding.reconstruct_object("checker_tex", depth, K, TCO, out_dir=tmp_path / "tex", texture_size=512, **kw)
    assert (tmp_path / "tex" / "checker_tex.ply").is_file() and (tmp_path / "tex" / "checker_tex.png").is_file()
    assert not (tmp_path / "plain" / "checker_plain.png").exists()
    head = (tmp_path / "tex" / "checker_tex.ply").read_bytes().split(b"end_header\n")[0].decode("ascii").splitlines()
    assert "comment TextureFile checker_tex.png" in head and "property list uchar float texcoord" in head and "property float nx" in head
    assert not any(line.split()[-1] in ("red", "green", "blue") for line in head if line.startswith("property"))
    loaded = mesh_io.load_rigid_object(textured)
    raw_plain = mesh_io.read_ply(plain.mesh_path)
    assert loaded["uvs"].shape == (len(loaded["faces"]), 3, 2) and loaded["texture_mips"][0].shape == (512, 512) and (loaded["colors"] == 1).all()
    assert len(loaded["faces"]) <= 1500 and np.array_equal(loaded["faces"], raw_plain["faces"]) and raw_plain["colors"] is not None
    assert np.array_equal(loaded["uvs"], tb.emul_uvs(len(loaded["faces"]), 512))
    with pytest.raises(ValueError, match="needs rgb"):
        onboarding.reconstruct_object("no_rgb", depth, K, TCO, masks=masks, resolution=48, out_dir=tmp_path / "no", texture_size=512)
    assert not (tmp_path / "no").exists()
    held = st.look_at((0.12, -0.25, 0.14))[None]
    truth = tb.checker_views(held, supersample=4)
    renderer = Panda3dBatchRenderer(RigidObjectDataset([plain, textured]))
    pose = _dev(held.astype(np.float32).repeat(2, 0))
    out = renderer.render(["checker_plain", "checker_tex"], pose, _dev(truth["K"].repeat(2, 0)), [[Panda3dLightData("ambient")]] * 2,
                          (tb.CHECK_H, tb.CHECK_W), render_depth=True)
    img = (out.rgbs * 255).permute(0, 2, 3, 1).cpu().numpy().astype(np.float64)
    d = out.depths[:, 0].cpu().numpy()
    both = (d[0] > 0) & (d[1] > 0) & (truth["depth"][0] > 0)
    want = truth["rgb"][0].astype(np.float64)
    err_plain, err_tex = float(np.abs(img[0] - want)[both].mean()), float(np.abs(img[1] - want)[both].mean())
    print(f"{int(both.sum())} pixels covered by both; mean |RGB difference| to the analytic image: vertex colours {err_plain:.2f}, texture {err_tex:.2f}")
    assert int(both.sum()) > 2500
    assert err_tex < err_plain
    # bake_texture on a host mesh, with its default tolerance: the covered share comes back, the mesh keeps its entries
    mesh = dict(vertices=loaded["vertices"], faces=loaded["faces"], note="kept")
    baked, coverage = onboarding.bake_texture(mesh, depth, K, TCO, masks=masks, rgb=rgb, texture_size=512, best_view=True)
    assert baked["note"] == "kept" and baked["texture"].shape == (512, 512, 3) and baked["texture"].dtype == torch.uint8 and baked["texture"].is_cuda
    assert baked["seen"].shape == (512, 512) and baked["uvs"].shape == (len(loaded["faces"]), 3, 2) and 0.95 <= coverage <= 1.0
    with pytest.raises(ValueError, match="rgb"):
        onboarding.bake_texture(mesh, depth, K, TCO)
    with pytest.raises(ValueError, match="do not fit"):
        onboarding.bake_texture(mesh, depth, K, TCO, rgb=rgb, texture_size=64)
