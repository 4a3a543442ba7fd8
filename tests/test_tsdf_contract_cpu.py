"""CPU: the contract of TSDF fusion and marching tetrahedra as csrc/tsdf_core.h states it -- the host emulation of the kernels
(tests/tsdf_emul.cpp, built on the header) against an independent numpy restatement written from the contract's text
(tests/support/tsdf.py), bit for bit; split calls; the topology of the sphere and the torus; the accuracy on the analytic sphere; the
worked 2 x 2 x 2 example as literal values; refusals and limits; and the emulation under the sanitizers."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.support import tsdf as st

VARIANTS = [dict(), dict(carve=False), dict(drop=("masks",)), dict(drop=("rgb",)), dict(drop=("masks", "rgb"), carve=False), dict(color=False)]


def _fused(name, carve=True, drop=(), color=True, integrate=st.emul_integrate, splits=None):
    g, views = st.fixture(name)
    views = st.without(views, *drop)
    vol = st.new_volume(g.dims, color)
    n = len(views["depth"])
    for sel in (splits or [slice(0, n)]):
        rc = integrate(vol, g, views, sel, carve=carve)
        assert rc in (0, None)
    return g, vol


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


@pytest.mark.parametrize("name", st.FIXTURES)
def test_emulation_equals_restatement_on_every_fixture(name):
    for var in VARIANTS:
        g, vol = _fused(name, **var)
        _, want = _fused(name, integrate=st.restated_integrate, **var)
        _same_bits(vol, want, (name, var, "volume"))
        assert st.counts_of(vol).max() > 0
        for min_views in (1, 2):
            got, exp = st.emul_extract(vol, g, min_views), st.restated_extract(vol, g, min_views)
            for a, b, what in zip(got, exp, ("vertices", "colors", "faces")):
                _same_bits(a, b, (name, var, min_views, what))
    assert len(got[0]) > 0 and len(got[2]) > 0


def test_a_field_set_directly_extracts_as_restated():
    for color in (True, False):
        vol = st.plane_volume(color=color)
        for min_views in (1, 2, 3):
            got, exp = st.emul_extract(vol, st.ODD_GRID, min_views), st.restated_extract(vol, st.ODD_GRID, min_views)
            for a, b, what in zip(got, exp, ("vertices", "colors", "faces")):
                _same_bits(a, b, (color, min_views, what))
    v, c, f = st.emul_extract(st.plane_volume(), st.ODD_GRID, 1)
    assert len(f) > 100 and st.mesh_report(v, f)["index_ok"]
    # zeros exactly on nodes: zero-area triangles are kept
    p = v.astype(np.float64)
    area = np.linalg.norm(np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]), axis=1)
    assert (area == 0).any() and (area > 0).any()
    # every triangle of positive area faces positive f: the field grows along (0.25, 0.5, -2)
    n = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])[area > 0]
    assert (n @ np.array([0.25, 0.5, -2.0]) > 0).all()
    assert c.min() >= 0 and c.max() <= 1 and (c == 1).any() and (c < 1).any()


@pytest.mark.parametrize("name", ["sphere", "awkward"])
def test_split_calls_leave_the_same_bits(name):
    g, whole = _fused(name)
    n = len(st.fixture(name)[1]["depth"])
    _, halves = _fused(name, splits=[slice(0, n // 2), slice(n // 2, n)])
    _, singles = _fused(name, splits=[slice(v, v + 1) for v in range(n)])
    _same_bits(whole, halves, "two calls")
    _same_bits(whole, singles, "view by view")
    _, empty = _fused(name, splits=[slice(0, 0)])
    assert not empty.view(np.uint32).any()


@pytest.mark.parametrize("name,euler", [("sphere", 2), ("torus", 0)])
def test_topology(name, euler):
    g, vol = _fused(name)
    v, c, f = st.emul_extract(vol, g)
    rep = st.mesh_report(v, f)
    print(name, len(v), len(f), rep)
    assert rep["index_ok"] and rep["no_loop"] and rep["directed_once"] and rep["reverse_present"]
    assert rep["euler"] == euler and rep["volume"] > 0 and rep["unreferenced"] == 0
    exact = 4 / 3 * np.pi * st.SPHERE_R ** 3 if name == "sphere" else 2 * np.pi ** 2 * st.TORUS_R * st.TORUS_r ** 2
    assert 0.7 * exact < rep["volume"] < 1.3 * exact


@pytest.mark.parametrize("carve", [True, False])
def test_accuracy_on_the_analytic_sphere(carve):
    """every vertex within 1 voxel of the sphere, within 0.25 voxel on average (float64).  The distance is truncated at 3 voxels and
    sampled once per voxel, so the zero crossing of a linear interpolation lies well inside one voxel; measured: 0.58 and 0.12 voxel with
    carving, 0.50 and 0.10 without."""
    g, vol = _fused("sphere", carve=carve)
    v, _, f = st.emul_extract(vol, g)
    err = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - st.SPHERE_R) / g.voxel
    print(f"carve {carve}: {len(v)} vertices, max {err.max():.3f} voxel, mean {err.mean():.3f} voxel")
    assert len(v) > 500 and err.max() <= 1.0 and err.mean() <= 0.25


def test_worked_example_and_limits():
    vol, g = st.corner_volume()
    v, c, f = st.emul_extract(vol, g)
    assert v.tolist() == st.CORNER_VERTICES and f.tolist() == st.CORNER_FACES and (c == 1).all()
    r = st.restated_extract(vol, g)
    assert r[0].tolist() == st.CORNER_VERTICES and r[2].tolist() == st.CORNER_FACES
    # every normal points away from the inside corner
    p = v.astype(np.float64)
    n = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    assert (np.einsum("ij,ij->i", n, p[f].mean(1)) > 0).all()
    # the complement: the same vertices, every triangle reversed in place (second and third corner swapped)
    vol[0] = -vol[0]
    v2, _, f2 = st.emul_extract(vol, g)
    assert v2.tolist() == st.CORNER_VERTICES and f2.tolist() == [[a, c_, b] for a, b, c_ in st.CORNER_FACES]
    # one unobserved corner: no complete cell, no surface; all inside / all outside: none either
    vol[1, 1, 1, 1] = 0
    assert [len(a) for a in st.emul_extract(vol, g)] == [0, 0, 0]
    for value in (1.0, -1.0):
        vol, g = st.corner_volume()
        vol[0] = value
        assert [len(a) for a in st.emul_extract(vol, g)] == [0, 0, 0]
    assert st.limits() == dict(min_dim=2, max_dim=512, max_nodes=2 ** 27, max_side=8192, edge_kinds=7, tets=6)


def test_emulation_refuses_bad_arguments():
    lib = st.load()
    g, views = st.fixture("sphere")
    depth, masks, rgb, K, TCO = st.view_arrays(views, slice(0, 2))
    vol = st.new_volume((4, 4, 4), True)

    def integrate(vol=vol, dims=(4, 4, 4), origin=(0.0, 0.0, 0.0), voxel=0.01, depth=depth, K=K, TCO=TCO, tco=16, n=2, h=st.H, w=st.W, mu=0.03,
                  z_min=0.0):
        return lib.tsdf_integrate_emul(st._p(vol), *(C.c_int(d) for d in dims), C.c_int(1), *(C.c_float(o) for o in origin), C.c_float(voxel),
                                       st._p(depth), st._p(masks), st._p(rgb), st._p(K), st._p(TCO), C.c_int(tco), C.c_int(n), C.c_int(h), C.c_int(w),
                                       C.c_float(mu), C.c_float(z_min), C.c_int(1))

    for bad in (dict(dims=(1, 4, 4)), dict(dims=(4, 513, 4)), dict(dims=(512, 512, 513)), dict(voxel=0.0), dict(voxel=float("nan")),
                dict(voxel=float("inf")), dict(origin=(0.0, float("nan"), 0.0)), dict(mu=0.0), dict(mu=-1.0), dict(mu=float("inf")),
                dict(z_min=-1.0), dict(z_min=float("nan")), dict(n=-1), dict(tco=9), dict(h=0), dict(w=8193), dict(vol=None), dict(depth=None),
                dict(K=None), dict(TCO=None)):
        assert integrate(**bad) != 0, bad
    assert not vol.view(np.uint32).any()
    assert integrate(n=0, vol=None, depth=None, K=None, TCO=None) == 0 and integrate() == 0
    totals = np.zeros(2, np.int32)
    assert lib.tsdf_extract_count_emul(st._p(vol), C.c_int(4), C.c_int(4), C.c_int(4), C.c_int(1), C.c_int(0), st._p(totals)) != 0       # min_views 0
    assert lib.tsdf_extract_count_emul(st._p(vol), C.c_int(4), C.c_int(1), C.c_int(4), C.c_int(1), C.c_int(1), st._p(totals)) != 0
    v = np.zeros((8, 3), np.float32)
    f = np.zeros((8, 3), np.int32)

    def extract(nv=7, nt=6, cap_v=8, cap_t=8, voxel=1.0):
        vol, _ = st.corner_volume()
        return lib.tsdf_extract_emul(st._p(vol), C.c_int(2), C.c_int(2), C.c_int(2), C.c_int(0), C.c_float(0), C.c_float(0), C.c_float(0),
                                     C.c_float(voxel), C.c_int(1), C.c_int(nv), C.c_int(nt), st._p(v), st._p(v.copy()), st._p(f), C.c_longlong(cap_v),
                                     C.c_longlong(cap_t))

    assert extract(cap_v=6) != 0 and extract(cap_t=5) != 0 and extract(nv=-1) != 0 and extract(voxel=0.0) != 0
    assert not v.any() and not f.any()
    assert extract() == 0 and f[:6].tolist() == st.CORNER_FACES


def test_emulation_under_the_sanitizers(tmp_path):
    """the emulation as a stand-alone program (tests/tsdf_asan_main.cpp) under the address and undefined-behaviour sanitizers, on arrays of
    exactly the call's sizes: a pixel outside a frame, a corner outside the volume, a vertex past the counted ones would be caught
    here.  The program compares every call with what the plain build returned."""
    n_calls = 0
    with open(tmp_path / "calls.bin", "wb") as fh:
        for name, var, min_views in (("sphere", dict(), 1), ("odd", dict(), 1), ("awkward", dict(), 1), ("awkward", dict(carve=False, drop=("masks",)), 2),
                                     ("torus", dict(drop=("rgb",)), 1), ("odd", dict(color=False), 2), ("tiny", dict(), 1)):
            g, views = st.fixture(name)
            views = st.without(views, *var.get("drop", ()))
            color, carve = var.get("color", True), var.get("carve", True)
            depth, masks, rgb, K, TCO = st.view_arrays(views)
            n, h, w = depth.shape
            vol = st.new_volume(g.dims, color)
            for sel in (slice(0, n // 2), slice(n // 2, n)):
                assert st.emul_integrate(vol, g, views, sel, carve=carve) == 0
            v, c, f = st.emul_extract(vol, g, min_views)
            fh.write(np.array([*g.dims, int(color), n, h, w, TCO.shape[1], int(carve), masks is not None, rgb is not None, min_views, len(v), len(f)],
                              np.int32).tobytes())
            fh.write(np.array([*g.origin, g.voxel, g.mu3, st.Z_MIN], np.float32).tobytes())
            for a in (depth, masks, rgb, K, TCO, vol, v, c, f):
                if a is not None:
                    fh.write(np.ascontiguousarray(a).tobytes())
            n_calls += 1
    exe = tmp_path / "tsdf_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    str(st.CSRC), "-I", str(st.TESTS), "-o", str(exe), str(st.TESTS / "tsdf_asan_main.cpp")], check=True)
    run = subprocess.run([str(exe), str(tmp_path / "calls.bin")], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip() == f"{n_calls} calls, 0 bad", (run.stdout, run.stderr[-2000:])
