"""CPU: the contract of tracking the camera against the TSDF as csrc/tsdf_track_core.h states it -- the host emulation of the kernels
(tests/tsdf_track_emul.cpp, built on the header) against an independent numpy restatement written from the contract's text
(tests/support/tsdf_track.py), bit for bit: the per-pixel terms, the records, the poses after 1 and 10 iterations; a batch against single
calls; convergence against the analytic poses (relocalisation, a sequence that integrates its own tracked poses, the sphere); a pose
at the optimum; refusals and limits; and the emulation as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.support import tsdf as st
from tests.support import tsdf_track as tt

F = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same(got: tt.Tracked, want: tt.Tracked, what, records=True):
    assert got.rc == 0 and want.rc == 0, what
    for k in ("status", "used", "TCO", "rms"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k, got[k], want[k])
    if records:
        ran = want.status != -2                              # the records of a frame that never ran keep what they held
        assert np.array_equal(_bits(got.records[ran]), _bits(want.records[ran])), (what, "records")


def _track(name, iters, fn=tt.emul_track, sel=slice(None), **kw):
    g, vol, fr = tt.fixture(name)
    return fn(vol, g, fr["depth"][sel], None if kw.pop("no_masks", False) else fr["masks"][sel], fr["K"][sel], fr["TCO"][sel], iters=iters, **kw)


@pytest.mark.parametrize("name", tt.FIXTURES)
def test_emulation_equals_the_restatement(name):
    g, vol, fr = tt.fixture(name)
    n_used = 0
    for v in range(len(fr["depth"])):
        got = tt.emul_rows(vol, g, fr["depth"][v], fr["masks"][v], fr["K"][v], fr["TCO"][v])
        if got is None:
            assert not (np.isfinite(fr["K"][v]).all() and np.isfinite(fr["TCO"][v, :12]).all())
            continue
        used, rows = tt.restated_rows(vol, g, fr["depth"][v], fr["masks"][v], fr["K"][v], fr["TCO"][v])
        assert np.array_equal(got[0], used) and np.array_equal(_bits(got[1]), _bits(rows)), (name, v)
        n_used += int(used.sum())
    assert n_used > 0
    _same(_track(name, 1), _track(name, 1, tt.restated_track), (name, 1))                      # the records of the one iteration too
    _same(_track(name, 10), _track(name, 10, tt.restated_track), (name, 10), records=False)
    if name in ("trio", "awkward"):
        for kw in (dict(no_masks=True), dict(min_views=2), dict(min_pixels=2000)):
            _same(_track(name, 2, **kw), _track(name, 2, tt.restated_track, **kw), (name, kw))


def test_the_fixtures_are_what_their_names_say():
    lim = tt.limits()
    assert lim == dict(group_pixels=tt.GROUP, block=tt.BLOCK, sums=tt.SUMS, record=tt.RECORD, max_iters=64, max_frames=65535)
    assert tt.groups(48, 64) == 3 and 48 * 64 == 3 * tt.GROUP                                   # exactly three groups
    assert tt.fixture("cropped")[2]["depth"].shape[1:] == (37, 53) and tt.groups(37, 53) == 2 and 37 * 53 % tt.GROUP != 0   # a partial group
    assert tt.groups(1, 1) == 1 and tt.groups(8192, 8192) == 65536 and tt.groups(0, 5) == 0 and tt.groups(5, 8193) == 0
    trio, leaving, awkward = _track("trio", 10), _track("leaving", 1), _track("awkward", 10)
    masked = tt.fixture("trio")[2]["masks"].reshape(24, -1).sum(1)
    assert (trio.used >= 0.99 * masked).all() and leaving.used.sum() < 0.5 * masked.sum() and (leaving.used > 0).all()
    assert (trio.records[:, :, 28] > 0).sum(1).min() >= 2                                       # more than one group contributes
    assert awkward.status.tolist() == [1, -1, -2, -2, -1, 1] and awkward.used.tolist()[1:5] == [0, 0, 0, 0]
    fr = tt.fixture("awkward")[2]
    for v in (1, 2, 3, 4):                                                                       # lost or refused: the input pose bit for bit
        assert np.array_equal(_bits(awkward.TCO[v]), _bits(fr["TCO"][v]))
    assert 0 < awkward.used[0] < np.isfinite(fr["depth"][0]).sum()
    pixel = _track("pixel", 3)
    assert pixel.status.tolist() == [-1, -1, -1] and pixel.used.tolist() == [1, 1, 1]           # one pixel is fewer than min_pixels
    one = _track("pixel", 3, min_pixels=1)                                                       # a rank-1 system: the damping keeps it solvable
    assert (one.status >= 0).all() and np.isfinite(one.TCO).all()
    sphere = _track("sphere", 10)
    assert (sphere.status >= 0).all() and np.isfinite(sphere.TCO).all() and np.isfinite(sphere.rms).all()


@pytest.mark.parametrize("name", ["trio", "awkward"])
def test_n_frames_in_one_call_equal_n_calls_of_one(name):
    whole = _track(name, 4)
    for v in range(6):
        one = _track(name, 4, sel=slice(v, v + 1))
        for k in ("TCO", "status", "used", "rms"):
            assert np.array_equal(_bits(one[k][0]), _bits(whole[k][v])), (name, v, k)
        if whole.status[v] != -2:
            assert np.array_equal(_bits(one.records[0]), _bits(whole.records[v]))


def test_relocalisation_on_trio():
    """every view restarted from a seeded perturbation of 5 degrees / 5 mm of its true pose, against the volume fused from the 24 true
    poses at 32^3: the points of the 0.05 m sphere move by at most 1 voxel between the true and the tracked pose (the bound of the sphere
    accuracy test of the fusion, for its reason: the field is sampled once per voxel).  Measured: 0.351 voxel at most, 0.21 in the mean."""
    g, vol, fr = tt.fixture("trio")
    start = [tt.displacement(fr["TCO_true"][v], fr["TCO"][v]) / g.voxel for v in range(24)]
    got = _track("trio", 10)
    disp = [tt.displacement(fr["TCO_true"][v], got.TCO[v]) / g.voxel for v in range(24)]
    masked = fr["masks"].reshape(24, -1).sum(1)
    print(f"relocalisation: start {min(start):.2f} .. {max(start):.2f} voxel, tracked max {max(disp):.3f} mean {np.mean(disp):.3f} voxel, "
          f"used {float((got.used / masked).min()):.4f} of the masked pixels at least, status {got.status.tolist()}")
    assert min(start) > 1.0                                                                      # the perturbation is worth the name
    assert (got.status >= 0).all() and max(disp) <= 1.0


def test_sequence_on_trio_integrating_the_tracked_poses():
    """24 views in steps of 15 degrees: frame 0 integrated at its true pose, every later frame tracked from the previous estimate and
    integrated (with carving) at the tracked pose.  Every frame tracks, and the drift stays within 1.5 voxels, half the truncation band:
    past the band the next frame would start outside the basin.  Measured: 0.655 voxel at most over the loop."""
    g, _, fr = tt.fixture("trio")
    vol = tt.new_volume(g.dims, False)
    views = dict(depth=fr["depth"], masks=fr["masks"], K=fr["K"], TCO=fr["TCO_true"].copy(), rgb=None)
    assert tt.emul_integrate(vol, g, views, slice(0, 1)) == 0
    pose, disp, status = fr["TCO_true"][0], [0.0], [1]
    for k in range(1, 24):
        got = tt.emul_track(vol, g, fr["depth"][k:k + 1], fr["masks"][k:k + 1], fr["K"][k:k + 1], pose[None], iters=10)
        status.append(int(got.status[0]))
        assert got.rc == 0 and got.status[0] >= 0, (k, got.status, got.used)
        pose = got.TCO[0]
        views["TCO"][k] = pose
        assert tt.emul_integrate(vol, g, views, slice(k, k + 1)) == 0
        disp.append(tt.displacement(fr["TCO_true"][k], pose) / g.voxel)
    print(f"sequence: max displacement {max(disp):.3f} voxel at frame {int(np.argmax(disp))}, last {disp[-1]:.3f}, status {status}")
    assert max(disp) <= 1.5


def test_sphere_translation_from_a_5_mm_offset():
    """rotation about the sphere's centre is unobservable: the damping keeps the solve finite, and the centre comes back within 1 voxel"""
    g, _, fr = tt.fixture("sphere")
    got = _track("sphere", 10)
    start = np.linalg.norm(fr["TCO"].reshape(-1, 4, 4)[:, :3, 3] - fr["TCO_true"].reshape(-1, 4, 4)[:, :3, 3], axis=1)
    err = np.linalg.norm(got.TCO.reshape(-1, 4, 4)[:, :3, 3].astype(np.float64) - fr["TCO_true"].reshape(-1, 4, 4)[:, :3, 3], axis=1)
    print(f"sphere: start {start.max() * 1e3:.2f} mm = {start.max() / g.voxel:.2f} voxel, tracked centre within {err.max() / g.voxel:.3f} voxel")
    assert start.min() > g.voxel and (got.status >= 0).all() and err.max() <= g.voxel


def test_a_pose_at_the_optimum_converges_and_stays():
    g, vol, fr = tt.fixture("trio")
    first = _track("trio", 10, sel=slice(0, 6))
    conv = first.status == 1
    assert conv.sum() >= 3
    again = {it: tt.emul_track(vol, g, fr["depth"][:6], fr["masks"][:6], fr["K"][:6], first.TCO, iters=it) for it in (1, 2, 10)}
    assert (again[1].status[conv] == 1).all()
    for it in (2, 10):                                                                           # later iterations leave a converged frame alone
        for k in ("TCO", "status", "used", "rms"):
            assert np.array_equal(_bits(again[it][k][conv]), _bits(again[1][k][conv])), (it, k)
        assert np.array_equal(_bits(again[it].records[conv]), _bits(again[1].records[conv]))
    moved = np.abs(again[1].TCO[conv].astype(np.float64) - first.TCO[conv]).max()
    assert moved < 1e-3 * g.voxel


def test_emulation_refuses_bad_arguments():
    g, vol, fr = tt.fixture("trio")
    sel = slice(0, 2)
    nan, inf = float("nan"), float("inf")

    def track(out=None, **kw):
        gg = tt.Grid(kw.pop("origin", g.origin), kw.pop("voxel", g.voxel), kw.pop("dims", g.dims))
        return tt.emul_track(vol, gg, kw.pop("depth", fr["depth"][sel]), fr["masks"][sel], fr["K"][sel], fr["TCO"][sel], out=out, **kw)

    for bad in (dict(dims=(1, 32, 32)), dict(dims=(32, 513, 32)), dict(voxel=0.0), dict(voxel=nan), dict(voxel=-1.0), dict(origin=(0.0, inf, 0.0)),
                dict(mu=0.0), dict(mu=nan), dict(mu=inf), dict(min_views=0), dict(min_pixels=0), dict(iters=0), dict(iters=65), dict(eps_rot=-1.0),
                dict(eps_rot=nan), dict(eps_tr=-1.0), dict(eps_tr=inf)):
        got = track(**bad)
        assert got.rc != 0, bad
        assert (got.TCO == -7).all() and (got.status == -7).all() and (got.used == -7).all() and (got.rms == -7).all() and (got.records == -7).all(), bad
    short = tt.new_outputs(2, 48, 64)
    short["records"] = short["records"].reshape(-1, tt.RECORD)[:5].reshape(1, 5, tt.RECORD).copy()      # one record short
    assert track(out=short).rc != 0 and (short.records == -7).all() and (short.status == -7).all()
    assert track(iters=64).rc == 0 and track(iters=1, eps_rot=0.0, eps_tr=0.0).rc == 0
    lib = tt.load()
    z = C.c_int(0)
    args = [None, C.c_int(8), C.c_int(8), C.c_int(8), z, C.c_float(0), C.c_float(0), C.c_float(0), C.c_float(0.01), None, None, None, None, z, z, z,
            C.c_float(0.03), C.c_int(1), C.c_int(1), C.c_int(1), C.c_float(0), C.c_float(0), None, None, None, None, None, C.c_longlong(0)]
    assert lib.tsdf_track_emul(*args) == 0                                                       # n = 0: a no-op, whatever the pointers
    args[13] = C.c_int(-1)
    assert lib.tsdf_track_emul(*args) != 0
    args[13] = C.c_int(65536)
    assert lib.tsdf_track_emul(*args) != 0


def test_emulation_under_the_sanitizers(tmp_path):
    """the emulation as a stand-alone program (tests/tsdf_track_asan_main.cpp) under the address and undefined-behaviour sanitizers, on
    arrays of exactly the call's sizes: a corner outside the volume, a pixel outside a frame, a record past the stated ones would be
    caught here.  The program compares every call with what the plain build returned."""
    n_calls = 0
    with open(tmp_path / "calls.bin", "wb") as fh:
        for name, kw in (("trio", dict(iters=3)), ("cropped", dict(iters=2)), ("leaving", dict(iters=3)), ("awkward", dict(iters=3)),
                         ("awkward", dict(iters=2, no_masks=True, min_views=2)), ("sphere", dict(iters=2)), ("pixel", dict(iters=2, min_pixels=1))):
            g, vol, fr = tt.fixture(name)
            no_masks = kw.get("no_masks", False)
            got = _track(name, **kw)
            assert got.rc == 0
            n, h, w = fr["depth"].shape
            rec = got.records.copy()
            rec[got.status == -2] = 0.0                                                          # (never written: the program starts from these)
            fh.write(np.array([*g.dims, n, h, w, not no_masks, kw.get("min_views", 1), kw.get("min_pixels", tt.MIN_PIXELS), kw["iters"]], np.int32).tobytes())
            fh.write(np.array([*g.origin, g.voxel, g.mu3, tt.EPS_ROT, tt.eps_trans(g)], F).tobytes())
            for a in (vol[:2], fr["depth"], None if no_masks else fr["masks"], fr["K"], fr["TCO"], got.TCO, got.status, got.used, got.rms, rec):
                if a is not None:
                    fh.write(np.ascontiguousarray(a).tobytes())
            n_calls += 1
    exe = tmp_path / "tsdf_track_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    str(st.CSRC), "-I", str(st.TESTS), "-o", str(exe), str(st.TESTS / "tsdf_track_asan_main.cpp")], check=True)
    run = subprocess.run([str(exe), str(tmp_path / "calls.bin")], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip() == f"{n_calls} calls, 0 bad", (run.stdout, run.stderr[-2000:])
