"""GPU: the mesh clean-up kernels (csrc/mesh_cleanup.hip) through the C ABI and the wrappers.  The eight entry points against the host
emulation built from the same rules header (tests/mesh_cleanup_emul.cpp), bit for bit, on the fixtures of the contract test, on tensors
of exactly the stated sizes pre-filled with a sentinel (the chain, star and large fixtures for the union-find; the large fixture for the
second round of the scan over the workgroup totals); determinism under repetition and under permutations of the faces and vertices;
empty and degenerate inputs; the argument rules (refused before any launch); the wrappers of megapose6d_amd.mesh_cleanup; and an object
reconstructed from rendered depth with a loose fragment, cleaned and decimated on the way.  Reads nothing outside the tree."""
import functools

import numpy as np
import pytest
import torch

from tests.support import mesh_cleanup as sm
from tests.support import tsdf as st

pytestmark = pytest.mark.gpu

SENT = sm.SENTINEL
SETTINGS = [(c, s) for c in sm.CELLS_VOXELS for s in sm.SHIFTS]


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _same_bits(a, b, what):
    a = _np(a) if isinstance(a, torch.Tensor) else a
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def _same_mesh(got, want, what):
    for a, b, name in zip(got[:3], want[:3], ("vertices", "faces", "colors")):
        _same_bits(a, b, (what, name))
    assert got[3] == want[3], (what, "dropped", got[3], want[3])


def fixture(name) -> sm.Mesh:
    if name.startswith("chain_"):
        return sm.chain(name[6:])
    return getattr(sm, name)()


@functools.lru_cache(None)
def _on_device(name, colors=True):
    m = fixture(name)
    return _dev(m["vertices"]), _dev(m["faces"]), _dev(m["colors"]) if colors else None


def _lib_and_stream():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    return _lib.load(), eng._stream()


def abi_components(V, faces_t):
    lib, s = _lib_and_stream()
    F = int(faces_t.shape[0])
    labels, fcount = torch.full((V,), SENT, dtype=torch.int32, device="cuda"), torch.full((V,), SENT, dtype=torch.int32, device="cuda")
    flabels, totals = torch.full((F,), SENT, dtype=torch.int32, device="cuda"), torch.full((4,), SENT, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.mp_mesh_components_workspace_bytes(V, F), dtype=torch.uint8, device="cuda")
    rc = lib.mp_mesh_components(V, _ptr(faces_t), F, _ptr(labels), _ptr(flabels), _ptr(fcount), totals.data_ptr(), ws.data_ptr(), ws.numel(), s)
    assert rc == 0, lib.mp_last_error()
    torch.cuda.synchronize()
    return _np(labels), _np(flabels), _np(fcount), _np(totals)


def abi_select(v_t, f_t, keep_t, c_t=None):
    """the two entry points on tensors of exactly the counted sizes -> numpy vertices, faces, colors, n_bad"""
    lib, s = _lib_and_stream()
    V, F = int(v_t.shape[0]), int(f_t.shape[0])
    ws = torch.empty(lib.mp_mesh_select_workspace_bytes(V, F), dtype=torch.uint8, device="cuda")
    totals = torch.full((3,), SENT, dtype=torch.int32, device="cuda")
    rc = lib.mp_mesh_select_count(V, _ptr(f_t), F, _ptr(keep_t), totals.data_ptr(), ws.data_ptr(), ws.numel(), s)
    assert rc == 0, lib.mp_last_error()
    nv, nf, bad = totals.tolist()
    ov, of = torch.full((nv, 3), float(SENT), device="cuda"), torch.full((nf, 3), SENT, dtype=torch.int32, device="cuda")
    oc = None if c_t is None else torch.full((nv, 3), float(SENT), device="cuda")
    rc = lib.mp_mesh_select(_ptr(v_t), _ptr(c_t), V, _ptr(f_t), F, nv, nf, _ptr(ov), _ptr(oc), _ptr(of), nv, nf, ws.data_ptr(), ws.numel(), s)
    assert rc == 0, lib.mp_last_error()
    torch.cuda.synchronize()
    return _np(ov), _np(of), _np(oc), bad


def abi_cluster_count(v_t, f_t, grid):
    lib, s = _lib_and_stream()
    origin, cell, dims = grid
    V, F = int(v_t.shape[0]), int(f_t.shape[0])
    ws = torch.empty(lib.mp_mesh_cluster_workspace_bytes(V, F, *dims), dtype=torch.uint8, device="cuda")
    totals = torch.full((3,), SENT, dtype=torch.int32, device="cuda")
    rc = lib.mp_mesh_cluster_count(_ptr(v_t), V, _ptr(f_t), F, *origin, cell, *dims, totals.data_ptr(), ws.data_ptr(), ws.numel(), s)
    assert rc == 0, lib.mp_last_error()
    return totals.tolist(), ws


def abi_cluster(v_t, f_t, grid, c_t=None):
    lib, s = _lib_and_stream()
    origin, cell, dims = grid
    V, F = int(v_t.shape[0]), int(f_t.shape[0])
    (nv, nf, dropped), ws = abi_cluster_count(v_t, f_t, grid)
    ov, of = torch.full((nv, 3), float(SENT), device="cuda"), torch.full((nf, 3), SENT, dtype=torch.int32, device="cuda")
    oc = None if c_t is None else torch.full((nv, 3), float(SENT), device="cuda")
    rc = lib.mp_mesh_cluster(_ptr(v_t), _ptr(c_t), V, _ptr(f_t), F, *origin, cell, *dims, nv, nf, _ptr(ov), _ptr(oc), _ptr(of), nv, nf, ws.data_ptr(),
                             ws.numel(), s)
    assert rc == 0, lib.mp_last_error()
    torch.cuda.synchronize()
    return _np(ov), _np(of), _np(oc), dropped


# against the emulation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("sphere", "torus", "scene", "chain_forward", "chain_reverse", "chain_bitrev", "star", "large"))
def test_components_equal_the_emulation(name):
    m = fixture(name)
    _, f_t, _ = _on_device(name)
    want = sm.emul_components(m.V, m["faces"])
    for run in range(2):                                            # the same call twice: the arrival order of the hooks must not show
        got = abi_components(m.V, f_t)
        for g, w, what in zip(got, want, ("labels", "face_labels", "face_count", "totals")):
            _same_bits(g, w, (name, run, what))
    assert want[3][3] == 0


def test_the_large_fixture_reaches_the_second_round_of_the_scan():
    """stated against the kernels' constants (csrc/mesh_cleanup.hip: kRankSpan = 256 * 16 bytes a workgroup, kMcBlock = 256 totals a round)"""
    m = sm.large()
    assert -(-m.F // sm.RANK_SPAN) > sm.SCAN_ROUND
    keep = np.ones(m.F, np.uint8)
    keep[::5] = 0
    v_t, f_t, c_t = _on_device("large")
    got = abi_select(v_t, f_t, _dev(keep), c_t)
    _same_mesh(got, sm.emul_select(m, keep), "large select")
    assert keep[sm.RANK_SPAN * sm.SCAN_ROUND:].sum() > 100            # kept faces whose rank starts from a base of the second round
    grid = sm.grid_of(m, 8.0, 0.37)
    assert max(grid[2]) <= 512
    _same_mesh(abi_cluster(v_t, f_t, grid, c_t), sm.emul_cluster(m, *grid), "large cluster")


@pytest.mark.parametrize("name", ("sphere", "scene"))
def test_select_equals_the_emulation(name):
    m = fixture(name)
    v_t, f_t, c_t = _on_device(name)
    for variant, keep in sm.keep_variants(m).items():
        for colors in (c_t, None):
            mm = m if colors is not None else sm.mesh(m["vertices"], m["faces"])
            _same_mesh(abi_select(v_t, f_t, _dev(keep), colors), sm.emul_select(mm, keep), (name, variant, colors is not None))


@pytest.mark.parametrize("name", ("sphere", "torus", "scene"))
def test_cluster_equals_the_emulation(name):
    m = fixture(name)
    v_t, f_t, c_t = _on_device(name)
    plain = sm.mesh(m["vertices"], m["faces"])
    for cell_voxels, shift in SETTINGS:
        grid = sm.grid_of(m, cell_voxels, shift)
        want = sm.emul_cluster(m, *grid)
        _same_mesh(abi_cluster(v_t, f_t, grid, c_t), want, (name, cell_voxels, shift))
        _same_mesh(abi_cluster(v_t, f_t, grid, None), sm.emul_cluster(plain, *grid), (name, cell_voxels, shift, "no colours"))
        assert len(want[1]) > 0
    origin, cell, dims = sm.grid_of(m, 2.0, 0.37)
    grid = (origin, cell, (dims[0] // 2, dims[1], dims[2]))          # vertices outside the grid
    _same_mesh(abi_cluster(v_t, f_t, grid, c_t), sm.emul_cluster(m, *grid), (name, "cut"))


# determinism --------------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_order_of_faces_or_vertices():
    m = sm.scene()
    rng = np.random.default_rng(7)
    grid = sm.grid_of(m, 2.0, 0.37)
    keep = sm.keep_variants(m)["third"]
    v_t, f_t, c_t = _on_device("scene")
    base_c, base_s = abi_cluster(v_t, f_t, grid, c_t), abi_select(v_t, f_t, _dev(keep), c_t)
    _same_mesh(abi_cluster(v_t, f_t, grid, c_t), base_c, "again")
    # the faces permuted: the vertices are bit-identical, the faces are the same rows in the permuted order (the emulation's, which
    # hands out indices face by face)
    fp = rng.permutation(m.F)
    permuted = sm.mesh(m["vertices"], m["faces"][fp], m["colors"])
    rows = lambda a: a[np.lexsort(a.T[::-1])]                                      # noqa: E731
    got = abi_cluster(v_t, _dev(permuted["faces"]), grid, c_t)
    _same_mesh(got, sm.emul_cluster(permuted, *grid), "cluster under a face permutation")
    _same_bits(got[0], base_c[0], "vertices under a face permutation")
    _same_bits(got[2], base_c[2], "colours under a face permutation")
    _same_bits(rows(got[1]), rows(base_c[1]), "the same faces under a face permutation")
    got = abi_select(v_t, _dev(permuted["faces"]), _dev(keep[fp]), c_t)
    _same_mesh(got, sm.emul_select(permuted, keep[fp]), "select under a face permutation")
    _same_bits(got[0], base_s[0], "selected vertices under a face permutation")
    _same_bits(rows(got[1]), rows(base_s[1]), "the same selected faces under a face permutation")
    # the vertices' arrival order changed: the same mesh with its vertices renumbered gives the same means, cell by cell
    vp = rng.permutation(m.V)                                        # new index of old vertex
    v2, c2 = np.empty_like(m["vertices"]), np.empty_like(m["colors"])
    v2[vp], c2[vp] = m["vertices"], m["colors"]
    good = ((m["faces"] >= 0) & (m["faces"] < m.V)).all(1)
    f2 = np.where(good[:, None], vp[np.where(good[:, None], m["faces"], 0)], m["faces"]).astype(np.int32)
    got = abi_cluster(_dev(v2), _dev(f2), grid, _dev(c2))
    _same_mesh(got, base_c, "vertices renumbered")


# empty and degenerate inputs --------------------------------------------------------------------------------------------------------------------
def test_empty_and_degenerate_inputs():
    octa = sm.mesh([[1.5, 1.5, 0.5], [1.5, 0.5, 1.5], [0.5, 1.5, 1.5], [2.5, 1.5, 1.5], [1.5, 2.5, 1.5], [1.5, 1.5, 2.5]],
                   [[5, 3, 4], [5, 4, 2], [5, 2, 1], [5, 1, 3], [0, 4, 3], [0, 2, 4], [0, 1, 2], [0, 3, 1]],
                   colors=np.linspace(0, 1, 18).reshape(6, 3))
    grid = ((0.0, 0.0, 0.0), 1.0, (3, 3, 3))
    cases = dict(fewer_than_a_wave=octa,
                 no_faces=sm.mesh(octa["vertices"], np.zeros((0, 3), np.int32), octa["colors"]),
                 no_vertices=sm.mesh(np.zeros((0, 3), np.float32), octa["faces"], np.zeros((0, 3), np.float32)),
                 all_bad=sm.mesh(octa["vertices"], [[0, 1, 6], [-1, 2, 3], [2 ** 31 - 1, 0, 1], [-2 ** 31, 4, 5]], octa["colors"]),
                 all_degenerate=sm.mesh(octa["vertices"], [[0, 0, 1], [2, 3, 3], [4, 4, 4], [5, 1, 5]], octa["colors"]))
    for name, m in cases.items():
        v_t, f_t, c_t = _dev(m["vertices"]), _dev(m["faces"]), _dev(m["colors"])
        for g, w, what in zip(abi_components(m.V, f_t), sm.emul_components(m.V, m["faces"]), ("labels", "face_labels", "face_count", "totals")):
            _same_bits(g, w, (name, what))
        keep = np.ones(m.F, np.uint8)
        _same_mesh(abi_select(v_t, f_t, _dev(keep), c_t), sm.emul_select(m, keep), (name, "select"))
        for gr in (grid, ((0.0, 0.0, 0.0), 4.0, (1, 1, 1))):       # one vertex per cell; one cell for everything
            _same_mesh(abi_cluster(v_t, f_t, gr, c_t), sm.emul_cluster(m, *gr), (name, "cluster", gr[2]))
    got = abi_cluster(_dev(octa["vertices"]), _dev(octa["faces"]), grid, _dev(octa["colors"]))
    assert np.array_equal(got[0], octa["vertices"]) and np.array_equal(got[1], octa["faces"])
    assert [len(a) for a in abi_cluster(_dev(octa["vertices"]), _dev(octa["faces"]), ((0.0, 0.0, 0.0), 4.0, (1, 1, 1)))[:2]] == [0, 0]
    m = cases["all_degenerate"]                                       # degenerate faces still join their vertices
    assert abi_components(m.V, _dev(m["faces"]))[3].tolist() == [3, 0, 0, 0]    # {0, 1, 5}, {2, 3}, {4}


# the argument rules -----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import engine as eng

    lib, s = _lib_and_stream()
    m = sm.mesh([[1.5, 1.5, 0.5], [1.5, 0.5, 1.5], [0.5, 1.5, 1.5], [2.5, 1.5, 1.5], [1.5, 2.5, 1.5], [1.5, 1.5, 2.5]],
                [[5, 3, 4], [5, 4, 2], [5, 2, 1], [5, 1, 3], [0, 4, 3], [0, 2, 4], [0, 1, 2], [0, 3, 1]], colors=np.full((6, 3), 0.5))
    v, f, c = _dev(m["vertices"]), _dev(m["faces"]), _dev(m["colors"])
    keep = torch.ones(8, dtype=torch.uint8, device="cuda")
    nan, inf = float("nan"), float("inf")
    big = 2 ** 29 + 1
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    totals = torch.full((4,), SENT, dtype=torch.int32, device="cuda")
    labels, flabels, fcount = (torch.full((n,), SENT, dtype=torch.int32, device="cuda") for n in (6, 8, 6))
    ov, oc, of = torch.full((6, 3), float(SENT), device="cuda"), torch.full((6, 3), float(SENT), device="cuda"), torch.full((8, 3), SENT, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == SENT).all()) for t in (totals, labels, flabels, fcount, ov, oc, of)) and not bool(ws.any())

    def components(V=6, fp=f.data_ptr(), F=8, lp=labels.data_ptr(), flp=flabels.data_ptr(), fcp=fcount.data_ptr(), tp=totals.data_ptr(), wsp=ws.data_ptr(),
                   wsn=ws.numel()):
        return lib.mp_mesh_components(V, fp, F, lp, flp, fcp, tp, wsp, wsn, s)

    for bad in (dict(V=-1), dict(F=-1), dict(V=big), dict(F=big), dict(fp=None), dict(lp=None), dict(flp=None), dict(fcp=None), dict(tp=None),
                dict(wsp=None), dict(wsn=8), dict(wsp=ws.data_ptr() + 4)):
        assert components(**bad) != 0, bad
    assert b"aligned" in lib.mp_last_error()
    assert lib.mp_mesh_components_workspace_bytes(-1, 8) == 0 and lib.mp_mesh_components_workspace_bytes(6, big) == 0

    need = lib.mp_mesh_select_workspace_bytes(6, 8)
    assert need > 0 and lib.mp_mesh_select_workspace_bytes(big, 8) == 0

    def select_count(V=6, fp=f.data_ptr(), F=8, kp=keep.data_ptr(), tp=totals.data_ptr(), wsp=ws.data_ptr(), wsn=need):
        return lib.mp_mesh_select_count(V, fp, F, kp, tp, wsp, wsn, s)

    for bad in (dict(V=-1), dict(F=big), dict(fp=None), dict(kp=None), dict(tp=None), dict(wsp=None), dict(wsn=need - 1), dict(wsp=ws.data_ptr() + 8)):
        assert select_count(**bad) != 0, bad

    def select(vp=v.data_ptr(), V=6, fp=f.data_ptr(), F=8, nv=6, nf=8, ovp=ov.data_ptr(), ocp=oc.data_ptr(), ofp=of.data_ptr(), cap_v=6, cap_f=8,
               wsp=ws.data_ptr(), wsn=need):
        return lib.mp_mesh_select(vp, c.data_ptr(), V, fp, F, nv, nf, ovp, ocp, ofp, cap_v, cap_f, wsp, wsn, s)

    for bad in (dict(V=-1), dict(F=big), dict(nv=-1), dict(nf=-1), dict(cap_v=5), dict(cap_f=7), dict(vp=None), dict(fp=None), dict(ovp=None),
                dict(ocp=None), dict(ofp=None), dict(wsp=None), dict(wsn=need - 1)):
        assert select(**bad) != 0, bad
    assert select(cap_v=5) != 0 and b"capacity" in lib.mp_last_error()

    grid_ok = dict(o=(0.0, 0.0, 0.0), cell=1.0, dims=(3, 3, 3))
    cneed = lib.mp_mesh_cluster_workspace_bytes(6, 8, 3, 3, 3)
    assert cneed > 0 and lib.mp_mesh_cluster_workspace_bytes(6, 8, 0, 3, 3) == 0 and lib.mp_mesh_cluster_workspace_bytes(6, 8, 3, 513, 3) == 0
    assert lib.mp_mesh_cluster_workspace_bytes(6, 8, 512, 512, 512) > 2 ** 27 and lib.mp_mesh_cluster_workspace_bytes(6, big, 3, 3, 3) == 0

    def cluster_count(vp=v.data_ptr(), V=6, fp=f.data_ptr(), F=8, o=grid_ok["o"], cell=1.0, dims=(3, 3, 3), tp=totals.data_ptr(), wsp=ws.data_ptr(),
                      wsn=cneed):
        return lib.mp_mesh_cluster_count(vp, V, fp, F, *o, cell, *dims, tp, wsp, wsn, s)

    bad_grids = (dict(dims=(0, 3, 3)), dict(dims=(3, 513, 3)), dict(dims=(3, 3, -1)), dict(dims=(512, 512, 513)), dict(cell=0.0), dict(cell=-1.0),
                 dict(cell=inf), dict(cell=nan), dict(o=(0.0, nan, 0.0)), dict(o=(inf, 0.0, 0.0)))
    for bad in bad_grids + (dict(V=-1), dict(F=big), dict(vp=None), dict(fp=None), dict(tp=None), dict(wsp=None), dict(wsn=cneed - 1)):
        assert cluster_count(**bad) != 0, bad

    def cluster(vp=v.data_ptr(), V=6, fp=f.data_ptr(), F=8, o=grid_ok["o"], cell=1.0, dims=(3, 3, 3), nv=6, nf=8, ovp=ov.data_ptr(), ocp=oc.data_ptr(),
                ofp=of.data_ptr(), cap_v=6, cap_f=8, wsp=ws.data_ptr(), wsn=cneed):
        return lib.mp_mesh_cluster(vp, c.data_ptr(), V, fp, F, *o, cell, *dims, nv, nf, ovp, ocp, ofp, cap_v, cap_f, wsp, wsn, s)

    for bad in bad_grids + (dict(V=-1), dict(F=big), dict(nv=-1), dict(nf=-1), dict(nv=7, cap_v=7), dict(cap_v=5), dict(cap_f=7), dict(vp=None),
                            dict(fp=None), dict(ovp=None), dict(ocp=None), dict(ofp=None), dict(wsp=None), dict(wsn=cneed - 1)):
        assert cluster(**bad) != 0, bad
    assert untouched()
    # ... and the same calls with everything in order
    assert components() == 0 and select_count() == 0 and totals[:3].tolist() == [6, 8, 0] and select() == 0
    torch.cuda.synchronize()
    assert np.array_equal(_np(ov), m["vertices"]) and np.array_equal(_np(of), m["faces"]) and bool((oc == 0.5).all())
    ov.fill_(float(SENT)), of.fill_(SENT)
    assert cluster_count() == 0 and totals[:3].tolist() == [6, 8, 0] and cluster() == 0
    torch.cuda.synchronize()
    assert np.array_equal(_np(ov), m["vertices"]) and np.array_equal(_np(of), m["faces"])
    assert cluster(nv=0, nf=0, ovp=None, ocp=None, ofp=None, cap_v=0, cap_f=0) == 0                  # nothing to write: a no-op
    with pytest.raises(eng.EngineError):
        eng.mesh_cluster(v, f, (0, 0, 0), 1.0, (0, 3, 3))
    with pytest.raises(eng.EngineError):
        eng.mesh_select(v, f, keep[:5])
    with pytest.raises(eng.EngineError):
        eng.mesh_components(6, f[:, :2])


# the wrappers ---------------------------------------------------------------------------------------------------------------------------------
def test_the_wrappers_equal_the_emulation():
    from megapose6d_amd import engine as eng
    from megapose6d_amd import mesh_cleanup as mc

    m = sm.scene()
    v_t, f_t, c_t = _on_device("scene")
    labels, flabels, fcount, totals = eng.mesh_components(v_t, f_t)
    for g, w in zip((labels, flabels, fcount, totals), sm.emul_components(m.V, m["faces"])):
        _same_bits(g, w, "engine.mesh_components")
    cc = mc.connected_components(m)
    assert (cc["n_components"], cc["largest"], cc["n_bad_faces"]) == (3, sm.scene_sphere_label(), 2) and cc["labels"].is_cuda
    for kw in (dict(), dict(largest=False, min_faces=5)):
        got, want = mc.keep_components(dict(vertices=v_t, faces=f_t, colors=c_t), **kw), mc.keep_components(m, backend=sm.EmulBackend(), **kw)
        assert got["vertices"].is_cuda
        for k in ("vertices", "faces", "colors"):
            _same_bits(got[k], want[k], ("keep_components", kw, k))
    assert got["faces"].shape[0] == sm.sphere().F + sm.torus().F
    grid = sm.grid_of(m, 2.0, 0.37)
    assert list(eng.mesh_cluster_count(v_t, f_t, *grid)) == sm.emul_cluster_count(m, *grid)[1].tolist()
    ov, of, oc, dropped = eng.mesh_cluster(v_t, f_t, *grid, colors=c_t)
    _same_mesh((ov, of, oc, dropped), sm.emul_cluster(m, *grid), "engine.mesh_cluster")
    assert mc.grid_for(m, 37) == mc.grid_for(m, 37, backend=sm.EmulBackend())
    sphere = sm.sphere()
    for kw in (dict(max_faces=1500), dict(cell_size=2.5 * sm.SPHERE_VOXEL)):
        got, want = mc.simplify(sphere, **kw), mc.simplify(sphere, backend=sm.EmulBackend(), **kw)
        for k in ("vertices", "faces", "colors"):
            _same_bits(got[k], want[k], ("simplify", kw, k))
    assert mc.simplify(sphere, max_faces=sphere.F) is sphere
    with pytest.raises(ValueError, match="no face is left"):
        mc.simplify(sphere, cell_size=1.0)
    got, want = mc.clean_mesh(m, keep_largest=True, max_faces=2000), mc.clean_mesh(m, keep_largest=True, max_faces=2000, backend=sm.EmulBackend())
    for k in ("vertices", "faces", "colors"):
        _same_bits(got[k], want[k], ("clean_mesh", k))
    host = mc.to_host(got)
    assert 0 < len(host["faces"]) <= 2000 and host["normals"].shape == host["vertices"].shape and host["normals"].dtype == np.float32
    assert sm.edge_balance(host["faces"], len(host["vertices"]))["balanced"]


# end to end -----------------------------------------------------------------------------------------------------------------------------------
def test_reconstructed_object_is_cleaned_and_decimated_end_to_end(tmp_path):
    """the scenario of the TSDF test with a loose fragment: an icosphere and a second small one placed apart from it, both inside every
    mask, rendered from the eight fixture cameras -> reconstruct_object(resolution=32, keep_largest=True, max_faces=1500): one component
    within the budget that the renderer, MeshDataBase, batched_surface and bop_models_info take; original and result rendered from a
    ninth camera agree to a median |dz| of at most 1 voxel (vertex means of points within 0.58 voxel of a convex surface stay in that
    band outwards and move inwards by less than the sagitta of a cell diagonal, about 0.13 voxel)."""
    from megapose6d_amd import RigidObject, RigidObjectDataset, mesh_io, onboarding
    from megapose6d_amd import evaluation as ev
    from megapose6d_amd import mesh_cleanup as mc
    from megapose6d_amd.mesh_db import MeshDataBase
    from megapose6d_amd.renderer import Panda3dBatchRenderer

    v, f = st.icosphere()
    vs, fs = st.icosphere(radius=0.015, subdivisions=2)
    original = RigidObject("ico", mesh_io.write_ply(tmp_path / "ico.ply", v, f), mesh_units="m")
    small = RigidObject("small", mesh_io.write_ply(tmp_path / "small.ply", vs, fs), mesh_units="m")
    renderer = Panda3dBatchRenderer(RigidObjectDataset([original, small]))
    views = st.sphere_views()
    K = _dev(np.repeat(st.intrinsics(f=120.0)[None], 8, 0).astype(np.float32))      # wide enough for both objects in every frame
    TCO = _dev(views["TCO"])
    apart = torch.eye(4, device="cuda")
    apart[0, 3] = 0.095                                               # 3 cm of air between the two surfaces
    d_big = renderer.render_depth(["ico"] * 8, TCO, K, (st.H, st.W))
    d_small = renderer.render_depth(["small"] * 8, TCO @ apart, K, (st.H, st.W))
    far = torch.full_like(d_big, float("inf"))
    depth = torch.minimum(torch.where(d_big > 0, d_big, far), torch.where(d_small > 0, d_small, far))
    depth = torch.where(torch.isfinite(depth), depth, torch.zeros_like(depth))
    masks = depth > 0
    assert bool(((d_small > 0) & (d_big == 0)).flatten(1).any(1).all())          # the fragment shows next to the sphere in every view
    kw = dict(masks=masks, resolution=32, out_dir=tmp_path / "rec")
    raw = onboarding.reconstruct_object("raw", depth, K, TCO, **kw)
    rec = onboarding.reconstruct_object("clean", depth, K, TCO, keep_largest=True, max_faces=1500, **kw)
    origin, voxel, dims = onboarding.volume_for_views(depth, K, TCO, masks, resolution=32)
    # without the two keywords: the parent's mesh, bit for bit
    vol = onboarding.TsdfVolume(origin, voxel, dims, color=False)
    vol.integrate(depth, K, TCO, masks=masks)
    parent = vol.extract()
    parent_path = mesh_io.write_ply(tmp_path / "parent.ply", parent["vertices"], parent["faces"], colors=parent["colors"], normals=parent["normals"])
    assert parent_path.read_bytes() == raw.mesh_path.read_bytes()
    raw_mesh, mesh = mesh_io.read_ply(raw.mesh_path), mesh_io.read_ply(rec.mesh_path)
    assert mc.connected_components(raw_mesh)["n_components"] >= 2                 # the fragment is in the raw mesh ...
    assert np.asarray(raw_mesh["vertices"])[:, 0].max() > 0.08
    cc = mc.connected_components(mesh)
    assert cc["n_components"] == 1 and cc["n_bad_faces"] == 0 and 0 < len(mesh["faces"]) <= 1500 < len(raw_mesh["faces"])
    rep = sm.edge_balance(mesh["faces"], len(mesh["vertices"]))
    assert rep["balanced"] and rep["unreferenced"] == 0 and rep["index_ok"] and mesh["colors"] is not None
    assert np.asarray(mesh["vertices"])[:, 0].max() < 0.06                         # ... and not in the clean one
    ds = RigidObjectDataset([original, rec])
    both = Panda3dBatchRenderer(ds)
    held_out = _dev(st.look_at((0.1, -0.3, 0.2)).astype(np.float32)[None].repeat(2, 0))
    d = both.render_depth(["ico", "clean"], held_out, K[:2], (st.H, st.W))
    hit = (d[0] > 0) & (d[1] > 0)
    assert int(hit.sum()) > 100
    dz = (d[0] - d[1]).abs()[hit]
    print(f"voxel {voxel * 1e3:.3f} mm, {len(raw_mesh['faces'])} -> {len(mesh['faces'])} faces, {int(hit.sum())} pixels hit in both, "
          f"median |dz| {float(dz.median()) / voxel:.3f} voxel, max {float(dz.max()) / voxel:.3f} voxel")
    assert float(dz.median()) <= voxel
    mesh_db = MeshDataBase.from_object_ds(ds)
    info = ev.bop_models_info(ev.model_info(mesh_db.batched(n_sym=4).cuda()), scale=1.0)
    print("diameters", info["ico"]["diameter"], info["clean"]["diameter"])
    assert abs(info["clean"]["diameter"] - 0.1) <= 2 * voxel
    surf = mesh_db.batched_surface(256)
    assert surf.points.shape == (2, 256, 3) and bool(torch.isfinite(surf.points).all())
    with pytest.raises(TypeError):
        onboarding.reconstruct_object("x", depth, K, TCO, max_face=10, **kw)
