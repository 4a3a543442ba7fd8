"""GPU: the camera-tracking kernels (csrc/tsdf_track.hip) through the C ABI and the wrappers.  mp_tsdf_track against the host emulation
built from the same rules header (tests/tsdf_track_emul.cpp), bit for bit, on the fixtures of the contract test (tensors of exactly the
stated sizes; the records after one iteration, pose, status, used and rms after 1 and 10; a batch against single calls; with and without
masks; min_views 1 and 2); the partial sums as a typed output on dirty memory between canaries; the argument rules (refused before any
launch, outputs untouched); `TsdfVolume.track`, `track_views` with a blank frame in the sequence, and an object reconstructed from
rendered depth without poses.  Reads nothing outside the tree."""
import functools

import numpy as np
import pytest
import torch

from tests.support import tsdf as st
from tests.support import tsdf_track as tt

pytestmark = pytest.mark.gpu
CANARY, GUARD = 0xA5, 256


def _dev(a):
    return None if a is None else torch.as_tensor(np.array(a)).cuda()          # (a writable, contiguous copy: the fixtures are read-only)


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


@functools.lru_cache(None)
def _emul(name, iters, no_masks=False, min_views=1, min_pixels=tt.MIN_PIXELS):
    g, vol, fr = tt.fixture(name)
    got = tt.emul_track(vol, g, fr["depth"], None if no_masks else fr["masks"], fr["K"], fr["TCO"], iters=iters, min_views=min_views, min_pixels=min_pixels)
    assert got.rc == 0
    return got


def _abi_track(name, iters, sel=slice(None), no_masks=False, min_views=1, min_pixels=tt.MIN_PIXELS, fill="sevens", short=0) -> tt.Tracked:
    """mp_tsdf_track on tensors of exactly the stated sizes; the partials between two canaries of 256 bytes, pre-filled as `fill` says"""
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    g, vol, fr = tt.fixture(name)
    depth, masks, K, TCO = (_dev(fr[k][sel]) for k in ("depth", "masks", "K", "TCO"))
    n, h, w = depth.shape
    groups = _lib.load().mp_tsdf_track_groups(h, w)
    assert groups == tt.groups(h, w)
    out = tt.Tracked(TCO=torch.full((n, 16), -7.0, device="cuda"), status=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                     used=torch.full((n,), -7, dtype=torch.int32, device="cuda"), rms=torch.full((n,), -7.0, device="cuda"))
    n_rec = n * groups - short
    arena = torch.full((GUARD + n_rec * tt.RECORD * 8 + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    body = arena[GUARD:GUARD + n_rec * tt.RECORD * 8]
    if fill == "ff":
        body.fill_(0xFF)
    else:
        body.view(torch.float64).fill_(float("nan") if fill == "nan" else -7.0)
    before = body.clone()
    nx, ny, nz = g.dims
    vol_t = _dev(vol)
    out["rc"] = _lib.load().mp_tsdf_track(vol_t.data_ptr(), nx, ny, nz, 0, *g.origin, g.voxel, depth.data_ptr(), None if no_masks else masks.data_ptr(),
                                          K.data_ptr(), TCO.data_ptr(), n, h, w, float(g.mu3), min_views, min_pixels, iters, tt.EPS_ROT, tt.eps_trans(g),
                                          out["TCO"].data_ptr(), out["status"].data_ptr(), out["used"].data_ptr(), out["rms"].data_ptr(),
                                          body.data_ptr(), n_rec, eng._stream())
    torch.cuda.synchronize()
    assert bool((arena[:GUARD] == CANARY).all()) and bool((arena[GUARD + body.numel():] == CANARY).all()), "a canary around the partials is damaged"
    res = tt.Tracked({k: out[k].cpu().numpy() for k in ("TCO", "status", "used", "rms")}, rc=out["rc"])
    res["untouched"] = bool(torch.equal(body, before))
    if not short:
        res["records"] = body.view(torch.float64).view(n, groups, tt.RECORD).cpu().numpy()
    return res


def _same(got, want, what, sel=slice(None), records=True):
    assert got.rc == 0, what
    for k in ("status", "used", "TCO", "rms"):
        assert np.array_equal(_bits(got[k]), _bits(want[k][sel])), (what, k, got[k], want[k][sel])
    if records:
        ran = want.status[sel] != -2                         # the records of a frame that never ran keep what they held
        assert np.array_equal(_bits(got.records[ran]), _bits(want.records[sel][ran])), (what, "records")


@pytest.mark.parametrize("name", tt.FIXTURES)
def test_entry_point_equals_the_emulation(name):
    _same(_abi_track(name, 1), _emul(name, 1), (name, 1))
    _same(_abi_track(name, 10), _emul(name, 10), (name, 10), records=False)


def test_the_groups_and_the_partial_group_are_what_is_tested():
    """the sizes that make the fixtures worth their names, stated against the kernel's constants (csrc/tsdf_track_core.h: kTrackGroupPixels =
    1024, kTrackBlock = 256): more than one group, every wave of a group at work, a partial last group, one pixel"""
    from megapose6d_amd import engine as eng

    assert tt.limits()["group_pixels"] == 1024 and tt.limits()["block"] == 256 and eng.TSDF_TRACK_RECORD == tt.limits()["record"] == 32
    assert eng.tsdf_track_groups(48, 64) == 3 and 48 * 64 == 3 * 1024 and eng.tsdf_track_groups(37, 53) == 2 and 37 * 53 - 1024 < 1024
    assert eng.tsdf_track_groups(1, 1) == 1 and eng.tsdf_track_groups(0, 4) == 0 and eng.tsdf_track_groups(8193, 4) == 0
    trio, cropped = _emul("trio", 1), _emul("cropped", 1)
    assert (trio.records[:, :, 28] > 0).sum(1).min() >= 2 and (cropped.records[:, 1, 28] > 0).all()      # the partial group contributes
    assert set(_emul("awkward", 10).status.tolist()) == {1, -1, -2} and tt.fixture("pixel")[2]["depth"].shape[1:] == (1, 1)


@pytest.mark.parametrize("name", ["trio", "awkward"])
def test_a_batch_of_three_equals_three_single_calls(name):
    want = _emul(name, 3)
    _same(_abi_track(name, 3, sel=slice(1, 4)), want, (name, "batch"), sel=slice(1, 4))
    for v in (1, 2, 3):
        _same(_abi_track(name, 3, sel=slice(v, v + 1)), want, (name, v), sel=slice(v, v + 1))


@pytest.mark.parametrize("name", ["trio", "awkward"])
def test_without_masks_and_with_two_views_a_node(name):
    for kw in (dict(no_masks=True), dict(min_views=2), dict(no_masks=True, min_views=2, min_pixels=2000)):
        _same(_abi_track(name, 2, **kw), _emul(name, 2, **kw), (name, kw))


def test_the_partial_sums_on_dirty_memory_between_canaries():
    """the partials are a typed output, not a workspace: every entry of a running frame's records is written by a plain store, whatever the
    buffer held (0xFF bytes, NaN), nothing around it is touched (the canaries are checked in every call of this module), and a capacity
    one record short is refused before any launch"""
    for name in ("trio", "cropped", "awkward"):
        want = _emul(name, 1)
        for fill in ("ff", "nan"):
            _same(_abi_track(name, 1, fill=fill), want, (name, fill))
        _same(_abi_track(name, 10, fill="nan"), _emul(name, 10), (name, "nan", 10), records=False)
    from megapose6d_amd import _lib

    short = _abi_track("trio", 1, short=1)
    assert short.rc != 0 and b"records" in _lib.load().mp_last_error() and short.untouched
    assert (short.TCO == -7).all() and (short.status == -7).all() and (short.used == -7).all() and (short.rms == -7).all()


def test_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    lib = _lib.load()
    g, vol, fr = tt.fixture("trio")
    depth, masks, K, TCO = (_dev(fr[k][:2]) for k in ("depth", "masks", "K", "TCO"))
    vol_t = _dev(vol)
    out = torch.full((2, 16), -7.0, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    used = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    rms = torch.full((2,), -7.0, device="cuda")
    part = torch.full((2, 3, 32), -7.0, dtype=torch.float64, device="cuda")
    s = eng._stream()
    nan, inf = float("nan"), float("inf")

    def track(vol=vol_t.data_ptr(), dims=g.dims, origin=g.origin, voxel=g.voxel, depth=depth.data_ptr(), K=K.data_ptr(), T=TCO.data_ptr(), n=2, h=48,
              w=64, mu=float(g.mu3), min_views=1, min_pixels=64, iters=2, eps_rot=1e-5, eps_trans=1e-6, To=out.data_ptr(), st_=status.data_ptr(),
              us=used.data_ptr(), rm=rms.data_ptr(), pp=part.data_ptr(), cap=6):
        return lib.mp_tsdf_track(vol, *dims, 0, *origin, voxel, depth, masks.data_ptr(), K, T, n, h, w, mu, min_views, min_pixels, iters, eps_rot, eps_trans,
                                 To, st_, us, rm, pp, cap, s)

    for bad in (dict(dims=(1, 32, 32)), dict(dims=(32, 513, 32)), dict(dims=(512, 512, 513)), dict(voxel=0.0), dict(voxel=nan), dict(voxel=inf),
                dict(voxel=-0.01), dict(origin=(0.0, nan, 0.0)), dict(mu=0.0), dict(mu=-1.0), dict(mu=inf), dict(mu=nan), dict(min_views=0),
                dict(min_pixels=0), dict(iters=0), dict(iters=65), dict(eps_rot=-1.0), dict(eps_rot=nan), dict(eps_trans=-1.0), dict(eps_trans=inf),
                dict(n=-1), dict(n=65536), dict(h=0), dict(w=8193), dict(vol=None), dict(depth=None), dict(K=None), dict(T=None), dict(To=None),
                dict(st_=None), dict(us=None), dict(rm=None), dict(pp=None), dict(To=TCO.data_ptr()), dict(cap=5), dict(pp=part.data_ptr() + 4),
                dict(vol=vol_t.data_ptr() + 2)):
        assert track(**bad) != 0, bad
    assert b"aligned" in lib.mp_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((status == -7).all()) and bool((used == -7).all()) and bool((rms == -7).all()) and bool((part == -7).all())
    assert track(n=0) == 0 and track(n=0, vol=None, depth=None, K=None, T=None, To=None, st_=None, us=None, rm=None, pp=None, cap=0) == 0   # a no-op
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((status == -7).all()) and bool((part == -7).all())
    assert track() == 0
    torch.cuda.synchronize()
    want = _emul("trio", 2)
    assert np.array_equal(_bits(out), _bits(want.TCO[:2])) and status.tolist() == want.status[:2].tolist()
    with pytest.raises(eng.EngineError):
        eng.tsdf_track(vol_t, g.origin, g.voxel, depth, K.view(2, 3, 3), TCO.view(2, 4, 4), masks=masks[:, :5])
    with pytest.raises(eng.EngineError):
        eng.tsdf_track(vol_t, g.origin, g.voxel, depth, K.view(2, 3, 3), TCO.view(2, 4, 4), iters=0)
    empty = eng.tsdf_track(vol_t, g.origin, g.voxel, depth[:0], K[:0].view(0, 3, 3), TCO[:0].view(0, 4, 4))
    assert [tuple(t.shape) for t in empty] == [(0, 4, 4), (0,), (0,), (0,)]


def test_the_wrappers_equal_the_emulation():
    from megapose6d_amd import engine as eng
    from megapose6d_amd.onboarding import TsdfVolume

    for name in ("trio", "awkward"):
        g, vol, fr = tt.fixture(name)
        want = _emul(name, 10)
        n = len(fr["depth"])
        part = torch.full((n, 3, 32), float("nan"), dtype=torch.float64, device="cuda")
        got = eng.tsdf_track(_dev(vol), g.origin, g.voxel, _dev(fr["depth"]), _dev(fr["K"]).view(n, 3, 3), _dev(fr["TCO"]).view(n, 4, 4),
                             _dev(fr["masks"]) != 0, partials=part)                                  # bool masks, [n,4,4] poses, the defaults
        for a, k in zip(got, ("TCO", "status", "used", "rms")):
            assert np.array_equal(_bits(a.reshape(want[k].shape)), _bits(want[k])), (name, k)
        assert bool(torch.isfinite(part[torch.as_tensor(want.status != -2).cuda()]).all())
    g, vol, fr = tt.fixture("trio")
    tv = TsdfVolume(g.origin, g.voxel, g.dims, color=False)
    views = tt.trio_views()
    tv.integrate(views["depth"], views["K"], views["TCO"], masks=views["masks"])
    assert np.array_equal(_bits(tv.volume), _bits(vol))
    got = tv.track(np.array(fr["depth"]), np.array(fr["K"]).reshape(-1, 3, 3), np.array(fr["TCO"]).reshape(-1, 4, 4),
                   masks=np.array(fr["masks"]))                                                      # host arrays; the volume's own mu
    want = _emul("trio", 10)
    for a, k in zip(got, ("TCO", "status", "used", "rms")):
        assert np.array_equal(_bits(a.reshape(want[k].shape)), _bits(want[k])), k


def _relative_truth(first):
    """the true poses of the orbit in the object frame that `first` (frame 0's pose) fixes"""
    true = tt.orbit_cameras()
    return np.stack([T @ np.linalg.inv(true[0]) @ first for T in true])


def test_track_views_on_trio_and_a_blank_frame_in_the_sequence():
    """24 views in steps of 15 degrees, nothing known but the frames: every frame tracks, and the points of the 0.05 m sphere move by at
    most 1.5 voxels (of the tracking volume) between the true and the tracked pose -- the condition of the contract test's sequence.  Then
    the same sequence with a blank frame after frame 11: it is flagged and not integrated, it keeps the pose before it, and the frames
    after it track to the same poses bit for bit.  Measured: 0.780 voxel of 4.94 mm at most."""
    from megapose6d_amd import onboarding

    fr = tt.fixture("trio")[2]
    depth, masks, K = np.array(fr["depth"]), np.array(fr["masks"]), np.array(fr["K"]).reshape(-1, 3, 3)         # (writable copies)
    poses, tracked, info = onboarding.track_views(depth, K, masks=masks, resolution=32)
    assert poses.shape == (24, 4, 4) and poses.is_cuda and tracked.dtype == torch.bool and bool(tracked.all()) and (info["status"] >= 0).all()
    first = poses[0].double().cpu().numpy()
    pts = onboarding._first_view_points(torch.as_tensor(depth[0]), torch.as_tensor(K[0]), torch.as_tensor(masks[0]))
    assert np.array_equal(first[:3, :3], np.eye(3)) and np.allclose(first[:3, 3], pts.mean(0).numpy(), atol=1e-6)
    vol = info["volume"]
    assert vol.dims == (32, 32, 32) and int(vol.counts.max()) > 12
    want = _relative_truth(first)
    disp = [tt.displacement(want[k], poses[k].cpu().numpy()) / vol.voxel_size for k in range(24)]
    print(f"track_views: voxel {vol.voxel_size * 1e3:.3f} mm, max displacement {max(disp):.3f} voxel at frame {int(np.argmax(disp))}, "
          f"status {info['status'].tolist()}, rms {info['rms'].max() * 1e3:.3f} mm at most")
    assert max(disp) <= 1.5
    ins = lambda a, blank: np.concatenate([a[:12], blank[None], a[12:]])   # noqa: E731
    poses2, tracked2, info2 = onboarding.track_views(ins(depth, np.zeros_like(depth[0])), ins(K, K[0]), masks=ins(masks, np.zeros_like(masks[0])),
                                                     resolution=32)
    assert tracked2.tolist() == [True] * 12 + [False] + [True] * 12 and info2["status"][12] == -1 and info2["used"][12] == 0
    assert torch.equal(poses2[12], poses2[11]) and torch.equal(torch.cat([poses2[:12], poses2[13:]]), poses)
    assert torch.equal(info2["volume"].volume, vol.volume)                                           # the blank frame carved nothing
    strict = onboarding.track_views(depth[:4], K[:4], masks=masks[:4], resolution=32, rms_max=1e-9)  # no frame meets such a residual
    assert strict[1].tolist() == [True, False, False, False] and torch.equal(strict[0][3], strict[0][0])
    with pytest.raises(ValueError, match="no measured pixel"):
        onboarding.track_views(np.zeros_like(depth[:2]), K[:2], masks=masks[:2], resolution=32)


def test_object_reconstructed_without_poses_end_to_end(tmp_path):
    """depth of three overlapping icospheres (the trio's centres and radii) rendered from the 24 orbit cameras -> reconstruct_object_unposed
    at 32 nodes -> the original and the reconstruction rendered from a 25th camera, the reconstruction placed with the object frame that
    TCO_first fixes.  Every frame tracks, and the median |dz| over the pixels hit in both is at most 1 voxel of the second pass's volume:
    the condition of the posed end-to-end test (tests/test_gpu_tsdf.py).  The measured figures rest on the GPU run alone: every frame
    tracked, 0.638 voxel of displacement at most, median |dz| 0.166 voxel of 3.81 mm over 1189 pixels."""
    from megapose6d_amd import RigidObject, RigidObjectDataset, mesh_io, onboarding
    from megapose6d_amd.renderer import Panda3dBatchRenderer

    vs, fs = [], []
    for c, r in zip(tt.TRIO_CENTRES, tt.TRIO_RADII):
        v, f = st.icosphere(r, 3)
        fs.append(f + sum(len(q) for q in vs))
        vs.append(v + c)
    original = RigidObject("trio", mesh_io.write_ply(tmp_path / "trio.ply", np.concatenate(vs), np.concatenate(fs)), mesh_units="m")
    renderer = Panda3dBatchRenderer(RigidObjectDataset([original]))
    cams = tt.orbit_cameras()
    K = _dev(np.repeat(st.intrinsics()[None], 24, 0).astype(np.float32))
    depth = renderer.render_depth(["trio"] * 24, _dev(cams.astype(np.float32)), K, (st.H, st.W))
    masks = depth > 0
    assert depth.shape == (24, st.H, st.W) and int(masks[0].sum()) > 800
    first = np.eye(4)
    first[2, 3] = 0.4                                          # camera 0 looks at the origin from 0.4 m: the object's frame with the camera's axes
    poses, tracked, info = onboarding.track_views(depth, K, masks=masks, TCO_first=first, resolution=32)
    want = _relative_truth(first)
    disp = [tt.displacement(want[k], poses[k].cpu().numpy()) / info["volume"].voxel_size for k in range(24)]
    assert bool(tracked.all()), info["status"]
    rec = onboarding.reconstruct_object_unposed("trio_rec", depth, K, masks=masks, TCO_first=first, resolution=32, out_dir=tmp_path / "rec")
    assert rec.label == "trio_rec" and str(rec.mesh_path).endswith("rec/trio_rec.ply")
    _, voxel, dims = onboarding.volume_for_views(depth, K, _dev(want.astype(np.float32)), masks, resolution=32)
    both = Panda3dBatchRenderer(RigidObjectDataset([original, rec]))
    T25 = st.look_at((0.1, -0.3, 0.2))
    held = np.stack([T25, T25 @ np.linalg.inv(cams[0]) @ first]).astype(np.float32)
    d = both.render_depth(["trio", "trio_rec"], _dev(held), K[:2], (st.H, st.W))
    hit = (d[0] > 0) & (d[1] > 0)
    assert bool((d[0] > 0).any()) and bool((d[1] > 0).any()) and int(hit.sum()) > 100
    dz = (d[0] - d[1]).abs()[hit]
    print(f"unposed: tracking voxel {info['volume'].voxel_size * 1e3:.3f} mm, max displacement {max(disp):.3f} voxel, second-pass voxel {voxel * 1e3:.3f} mm, "
          f"{int(hit.sum())} pixels hit in both, median |dz| {float(dz.median()) / voxel:.3f} voxel, max {float(dz.max()) / voxel:.3f} voxel")
    assert float(dz.median()) <= voxel
    with pytest.raises(ValueError, match="1 of 3 frames tracked"):
        blank = torch.zeros_like(depth[:3])
        blank[0] = depth[0]
        onboarding.reconstruct_object_unposed("nothing", blank, K[:3], masks=blank > 0, resolution=32, out_dir=tmp_path / "rec")
