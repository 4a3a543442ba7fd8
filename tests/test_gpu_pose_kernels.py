"""GPU tier of the pose / camera-geometry kernel tests: every kernel of megapose6d_amd/csrc/pose.hip through megapose6d_amd.engine against
the float64 reference tests/support/pose_ref.py, over the case families of tests/support/pose_cases.py (per-row intrinsics with skew, close /
far / off-screen poses, batches across a block boundary and at the pipeline's row counts, point counts around a wave and a block in a
buffer wider than the used prefix, portrait / square shapes, every view list).  No row and no element is left out of a comparison.

Bounds are an error model, not constants: |got - ref64| <= k * 2^-24 * S with S per row from the float64 reference (pose_ref.prepare_units,
update_scales, init_poses_scales, init_extents_scale) and k = 4 x the fp32 oracle's own worst error in the same units (the floor, measured
on the CPU by tests/test_pose_ref_cpu.py::test_bounds_follow_from_the_oracle_floor), rounded up to a power of two, at least 8.

Worst case per family in units of 2^-24 * S, as "fp32-oracle floor (CPU) -> k | kernel, measured on the MI355X":
  output         mid                     mid_offaxis             close                   far                     offscreen
  TCO_n          2.86 -> 16 | 3.33       2.48 -> 16 | 3.07       1.9 -> 8 | 2.31         2 -> 8 | 2.4            3.3 -> 16 | 2.76
  tCR            0 -> 8 | 0              0 -> 8 | 0              0 -> 8 | 0              0 -> 8 | 0              0 -> 8 | 0
  TCV_O          8.25 -> 64 | 5.44       7 -> 32 | 12.24         6.53 -> 32 | 4.64       6.21 -> 32 | 3.99       7.3 -> 32 | 3.66
  boxes_rend     3.21 -> 16 | 3.21       3.16 -> 16 | 3.68       2.73 -> 16 | 2.73       2.52 -> 16 | 2.52       3.12 -> 16 | 3.12
  boxes_crop     4.79 -> 32 | 4.79       4.56 -> 32 | 4.56       3.59 -> 16 | 3.59       5.02 -> 32 | 5.02       4.69 -> 32 | 4.69
  K_main         782.2 -> 4096 | 782.2   377.4 -> 2048 | 377.4   7.21 -> 32 | 7.58       94.6 -> 512 | 94.6      208.9 -> 1024 | 208.9
  K_main.focal   9.82 -> 64 | 9.82       7.6 -> 32 | 8.66        7.21 -> 32 | 7.58       8.87 -> 64 | 8.87       7.56 -> 32 | 7.56
  K_main.pp      5.55 -> 32 | 5.55       5.43 -> 32 | 6.15       4.53 -> 32 | 4.06       8.37 -> 64 | 8.37       7.03 -> 32 | 7.03
  KV_crop        782.2 -> 4096 | 782.2   91.8 -> 512 | 299.7     14.02 -> 64 | 10.74     94.6 -> 512 | 94.6      18.49 -> 128 | 17.76
  KV_crop.focal  12.72 -> 64 | 10.41     12.74 -> 64 | 11.81     11.45 -> 64 | 10.74     9.16 -> 64 | 9.83       7.57 -> 32 | 7.36
  KV_crop.pp     17.45 -> 128 | 12.05    31.82 -> 128 | 17.75    14.02 -> 64 | 8.52      23.95 -> 128 | 14.42    18.49 -> 128 | 17.76
  pose_update 3.32 -> 16 | 3.06    init_poses 17.87 -> 128 | 3.21    init_extents 4.94 -> 32 | 4.94    normalize_T 3.27 -> 16 | 3.21
The kernel follows the reference's operation order without contraction, so on most outputs it lands on the oracle's own figure.  The
one place it is above the floor by more than a rounding is mid_offaxis (the 26 sphere views): TCV_O 12.2 against 7.0 and KV_crop 300
against 92.  Those are the cameras straight above and below the object, whose look-at divides by |y x up| ~ 0.15: the oracle builds
them in float64 and rounds once, the kernel in fp32, and 12.2 is what 1 / 0.15 makes of ~2 units; both are within k.
The large floors of K_main / KV_crop are the principal point where its two terms cancel ((out - 1) / 2 + scale * (c - box centre); one
row of 4608 has cy = 0.79 from 119.5 - 118.7), which the scale max(1, |value|) * |box| / width cannot see.  That check is kept as it is;
the focal lengths alone (.focal, same scale) and the principal point against the scale of its terms (.pp, pose_ref._pp_scale) are checked
besides, with the far lower floors and bounds of their own.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests.support import pose_cases as pc
from tests.support import pose_ref as pr

pytestmark = pytest.mark.gpu

WORST = {}


def _note(family: str, name: str, value: float) -> None:
    WORST[(family, name)] = max(WORST.get((family, name), 0.0), float(value))


@pytest.fixture(scope="module")
def eng():
    from megapose6d_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert engine.device_info()[2].startswith("gfx950")
    yield engine
    print("\nkernel worst case per (family, output), units of 2^-24 * S:")
    for (f, n), v in sorted(WORST.items()):
        print(f"  {f:12s} {n:14s} {v:8.2f}")


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t) -> np.ndarray:
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(a).view(np.int32)


def _check(family: str, name: str, u: np.ndarray) -> None:
    """print the figure, then assert it: every element within k * 2^-24 * S"""
    k = pc.K_BOUND[family][name]
    worst = float(u.max())
    _note(family, name, worst)
    print(f"  {family} {name}: worst {worst:.2f} of k = {k}")
    assert worst <= k, (family, name, worst, k, np.unravel_index(u.argmax(), u.shape))


@functools.lru_cache(maxsize=None)
def _case_data(i: int):
    case = pc.PREPARE_CASES[i]
    inp = case.inputs()
    return case, inp, case.reference(inp)


def run_prepare(eng, case, inp, rows=slice(None)):
    out = eng.pose_prepare(_cu(inp["TCO_in"][rows]), _cu(inp["K"][rows]), _cu(inp["mesh_ids"][rows]), _cu(inp["points"]), case.n_main,
                           case.n_views, case.V, case.code, case.im_hw, case.out_hw, case.lamb, with_K_main=True)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in zip(pr.PREPARE_OUTPUTS, out)}


# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("i", range(len(pc.PREPARE_CASES)), ids=[c.name for c in pc.PREPARE_CASES])
def test_pose_prepare_vs_float64(eng, i):
    case, inp, ref = _case_data(i)
    got = run_prepare(eng, case, inp)
    for n, u in pr.prepare_units(got, ref, case.out_hw).items():
        _check(case.family, n, u)
    K = inp["K"]
    # what is copied is copied exactly: the anchor, the unscaled entries of the intrinsics, the TCO view
    assert (_bits(got["tCR"]) == _bits(got["TCO_n"][:, :3, 3])).all()
    for Kc, Kin in ((got["K_main"], K), (got["KV_crop"], np.broadcast_to(K[:, None], got["KV_crop"].shape))):
        for r, c in ((0, 1), (1, 0), (2, 0), (2, 1), (2, 2)):
            assert (_bits(Kc[..., r, c]) == _bits(Kin[..., r, c])).all(), (r, c)
    # KV_crop[:, 0]: crop_inputs' K_crop when the TCO view is rendered, the view's own crop from n_pts_views points when it is removed
    # (models/pose_rigid.py:550-552)
    if not case.remove:
        assert (_bits(got["KV_crop"][:, 0]) == _bits(got["K_main"])).all() and (_bits(got["TCV_O"][:, 0]) == _bits(got["TCO_n"])).all()
    elif case.n_views < case.n_main:
        # (value parity with the n_pts_views crop is part of the check of KV_crop above)
        assert (np.abs(ref["KV_crop"][:, 0] - ref["K_main"]).max(axis=(1, 2)) > 1e-3).mean() > 0.5
        assert (np.abs(got["KV_crop"][:, 0] - got["K_main"]).max(axis=(1, 2)) > 1e-3).mean() > 0.5


@pytest.mark.parametrize("b", pc.BATCHES)
def test_normalize_T_vs_float64(eng, b):
    T = pc.normalize_T_inputs(b)
    ref = pr.normalize_T(T)
    got = eng.normalize_T(_cu(T)).cpu().numpy()
    _check("normalize", "T", pr.units(got, ref, pr._T_scale(ref)))
    assert (_bits(got[:, :3, 3]) == _bits(T[:, :3, 3])).all()


@pytest.mark.parametrize("b", pc.BATCHES)
def test_pose_update_vs_float64(eng, b):
    inp = pc.update_inputs(b)
    K = inp["KV_crop"][:, 0]
    ref = pr.pose_update(inp["TCO"], K, inp["out9"], inp["tCR"])
    got = eng.pose_update(_cu(inp["TCO"]), _cu(K), _cu(inp["out9"]), _cu(inp["tCR"])).cpu().numpy()
    _check("update", "TCO_out", pr.units(got, ref, pr.update_scales(ref, inp["out9"], inp["tCR"])))


def test_pose_update_reads_K_in_place(eng):
    """k_stride_floats: K read from KV_crop[:, 0] of a [b, V, 3, 3] tensor (stride 9 V) whose other views hold other intrinsics"""
    b, V = 577, 4
    inp = pc.update_inputs(b, seed=1, V=V)
    KV = _cu(inp["KV_crop"])
    args = (_cu(inp["TCO"]),), (_cu(inp["out9"]), _cu(inp["tCR"]))
    in_place = eng.pose_update(*args[0], KV, *args[1], k_stride_floats=9 * V).cpu().numpy()
    copied = eng.pose_update(*args[0], KV[:, 0].contiguous(), *args[1], k_stride_floats=9).cpu().numpy()
    assert (_bits(in_place) == _bits(copied)).all()
    ref = pr.pose_update(inp["TCO"], inp["KV_crop"][:, 0], inp["out9"], inp["tCR"])
    _check("update", "TCO_out", pr.units(in_place, ref, pr.update_scales(ref, inp["out9"], inp["tCR"])))
    wrong = pr.pose_update(inp["TCO"], inp["KV_crop"].reshape(-1, 3, 3)[:b], inp["out9"], inp["tCR"])      # what stride 9 would read
    assert np.abs(wrong - ref).max() > 1e-3


@pytest.mark.parametrize("grid,n_pts", pc.EXTENT_CASES)
def test_init_extents_vs_float64(eng, grid, n_pts):
    pts, R = pc.make_points(n_pts, n_pts), pc.so3_grid(grid)
    got = eng.init_extents(_cu(pts), _cu(R)).cpu().numpy()
    _check("init", "extents", pr.units(got, pr.init_extents(pts, R), pr.init_extents_scale(pts, R)[..., None] * np.ones(2)))


@pytest.mark.parametrize("b,grid,n_pts", [(1, 72, 2000), (127, 576, 2000), (128, 4608, 2000), (129, 72, 255), (576, 576, 65), (4608, 4608, 2000)])
def test_init_poses_from_boxes_vs_float64(eng, b, grid, n_pts):
    """the pair init_extents + init_poses end to end, from points"""
    inp = pc.init_inputs(b, grid, n_pts)
    R = _cu(inp["R"])
    ext = eng.init_extents(_cu(inp["points"]), R)
    got = eng.init_poses_from_boxes(_cu(inp["boxes"]), _cu(inp["K"]), _cu(inp["mesh_ids"]), _cu(inp["rot_ids"]), R, ext).cpu().numpy()
    Rrow = inp["R"][inp["rot_ids"]]
    ref = pr.init_poses_from_boxes(inp["boxes"], inp["K"], inp["points"][inp["mesh_ids"]], Rrow)
    _check("init", "TCO_init", pr.units(got, ref, pr.init_poses_scales(ref, inp["boxes"], inp["K"])))
    assert (_bits(got[:, :3, :3]) == _bits(Rrow)).all()


# --------------------------------------------------------------------------- #
BIG = next(i for i, c in enumerate(pc.PREPARE_CASES) if c.name == "batch-4608")
ROWS = (0, 1, 127, 128, 129, 2303, 4606, 4607)


def test_row_independence_and_determinism(eng):
    """row i of a 4608-row call is bit-identical to the same row computed alone, and two identical calls give identical bits"""
    case, inp, _ = _case_data(BIG)
    full, again = run_prepare(eng, case, inp), run_prepare(eng, case, inp)
    for n in pr.PREPARE_OUTPUTS:
        assert (_bits(full[n]) == _bits(again[n])).all(), n
    for r in ROWS:
        alone = run_prepare(eng, case, inp, slice(r, r + 1))
        for n in pr.PREPARE_OUTPUTS:
            assert (_bits(alone[n][0]) == _bits(full[n][r])).all(), (n, r)
    b = 4608
    T = pc.normalize_T_inputs(b)
    u = pc.update_inputs(b)
    ini = pc.init_inputs(b, 4608)
    R = _cu(ini["R"])
    ext = eng.init_extents(_cu(ini["points"]), R)
    calls = {
        "normalize_T": lambda s: eng.normalize_T(_cu(T[s])),
        "pose_update": lambda s: eng.pose_update(_cu(u["TCO"][s]), _cu(u["KV_crop"][s, 0]), _cu(u["out9"][s]), _cu(u["tCR"][s])),
        "init_poses": lambda s: eng.init_poses_from_boxes(_cu(ini["boxes"][s]), _cu(ini["K"][s]), _cu(ini["mesh_ids"][s]), _cu(ini["rot_ids"][s]), R, ext),
    }
    for name, f in calls.items():
        full, again = f(slice(None)).cpu().numpy(), f(slice(None)).cpu().numpy()
        assert (_bits(full) == _bits(again)).all(), name
        for r in ROWS:
            assert (_bits(f(slice(r, r + 1)).cpu().numpy()[0]) == _bits(full[r])).all(), (name, r)
    assert (_bits(ext) == _bits(eng.init_extents(_cu(ini["points"]), R))).all()


# --------------------------------------------------------------------------- #
GUARD, PATTERN = 64, 0x7FC0BEEF      # a quiet NaN with a payload


class Guarded:
    """an output buffer pre-filled with a NaN pattern, with a guard band on either side"""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.raw = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.int32, device="cuda")

    @property
    def ptr(self) -> int:
        return self.raw.data_ptr() + 4 * GUARD

    def payload(self) -> np.ndarray:
        return self.raw[GUARD:GUARD + self.n].view(torch.float32).cpu().numpy().reshape(self.shape)

    def check(self, name, written=True):
        raw = self.raw.cpu().numpy()
        assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + self.n:] == PATTERN).all(), f"{name}: guard band written"
        if written:
            assert np.isfinite(self.payload()).all() and (raw[GUARD:GUARD + self.n] != PATTERN).all(), f"{name}: elements not written"
        else:
            assert (raw[GUARD:GUARD + self.n] == PATTERN).all(), f"{name}: written although the call was refused"


def _prepare_raw(eng, case, inp, **over):
    """mp_pose_prepare_ex through the C entry on guarded buffers -> (rc, buffers)"""
    from megapose6d_amd import _lib

    b, V = case.b, over.pop("V", case.V)
    bufs = dict(TCO_n=Guarded(b, 4, 4), tCR=Guarded(b, 3), TCV_O=Guarded(b, V, 4, 4), KV_crop=Guarded(b, V, 3, 3), boxes_rend=Guarded(b, 4),
                boxes_crop=Guarded(b, 4), K_main=Guarded(b, 3, 3))
    a = dict(stride=inp["points"].shape[1], n_main=case.n_main, n_views=case.n_views, code=case.code)
    a.update(over)
    keep = [_cu(inp[n]) for n in ("TCO_in", "K", "mesh_ids", "points")]
    rc = _lib.load().mp_pose_prepare_ex(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), a["stride"], a["n_main"],
                                        a["n_views"], b, V, a["code"], case.im_hw[0], case.im_hw[1], case.out_hw[0], case.out_hw[1], case.lamb,
                                        *[bufs[n].ptr for n in pr.PREPARE_OUTPUTS], eng._stream())
    torch.cuda.synchronize()
    return rc, bufs


WRITE_CASES = [i for i, c in enumerate(pc.PREPARE_CASES) if c.name in ("views-m0", "views-m0-rm", "views-m1", "views-m1-rm", "views-m2-rm",
                                                                        "views-m3-rm-inplane", "pose-close", "batch-129", "points-1-1")]


@pytest.mark.parametrize("i", WRITE_CASES, ids=[pc.PREPARE_CASES[i].name for i in WRITE_CASES])
def test_pose_prepare_writes_every_element_and_nothing_else(eng, i):
    """in particular TCO_n / tCR / boxes / K_main when remove_TCO_rendering moves the main unit to blockIdx.y == V"""
    case, inp, ref = _case_data(i)
    rc, bufs = _prepare_raw(eng, case, inp)
    assert rc == 0
    for n, g in bufs.items():
        g.check(n)
    via_engine = run_prepare(eng, case, inp)
    for n, g in bufs.items():
        assert (_bits(g.payload()) == _bits(via_engine[n])).all(), n


def test_small_kernels_write_every_element_and_nothing_else(eng):
    from megapose6d_amd import _lib

    lib, b = _lib.load(), 129
    T, u, ini = _cu(pc.normalize_T_inputs(b)), {k: _cu(v) for k, v in pc.update_inputs(b).items()}, {k: _cu(v) for k, v in pc.init_inputs(b, 72, 65).items()}
    out = Guarded(b, 4, 4)
    assert lib.mp_normalize_T(T.data_ptr(), b, out.ptr, eng._stream()) == 0
    out.check("normalize_T")
    out = Guarded(b, 4, 4)
    K = u["KV_crop"][:, 0].contiguous()
    assert lib.mp_pose_update(u["TCO"].data_ptr(), K.data_ptr(), 9, u["out9"].data_ptr(), u["tCR"].data_ptr(), b, out.ptr, eng._stream()) == 0
    out.check("pose_update")
    ext = Guarded(pc.N_MESH, 72, 2)
    assert lib.mp_init_extents(ini["points"].data_ptr(), pc.N_MESH, 65, ini["R"].data_ptr(), 72, ext.ptr, eng._stream()) == 0
    ext.check("init_extents")
    ext_t = eng.init_extents(ini["points"], ini["R"])
    out = Guarded(b, 4, 4)
    assert lib.mp_init_poses_from_boxes(ini["boxes"].data_ptr(), ini["K"].data_ptr(), ini["mesh_ids"].data_ptr(), ini["rot_ids"].data_ptr(),
                                        ini["R"].data_ptr(), 72, ext_t.data_ptr(), b, out.ptr, eng._stream()) == 0
    out.check("init_poses_from_boxes")


def test_argument_checks_refuse_instead_of_launching(eng):
    from megapose6d_amd import _lib

    i = next(i for i, c in enumerate(pc.PREPARE_CASES) if c.name == "views-m1-rm")
    case, inp, _ = _case_data(i)
    plain = pc.PREPARE_CASES[next(i for i, c in enumerate(pc.PREPARE_CASES) if c.name == "views-m1")]
    single = pc.PREPARE_CASES[next(i for i, c in enumerate(pc.PREPARE_CASES) if c.name == "views-m0")]
    refused = [
        ("V not matching the code", case, dict(V=case.V + 1)),
        ("V not matching the code", case, dict(V=1)),
        ("in-plane copies without remove_TCO_rendering", plain, dict(code=plain.code | pc.MV_INPLANE, V=16)),
        ("unknown mode", case, dict(code=7)),
        ("unknown flag", case, dict(code=case.code | 1024)),
        ("n_pts_main > n_pts_stride", case, dict(n_main=inp["points"].shape[1] + 1)),
        ("n_pts_views > n_pts_stride", case, dict(n_views=inp["points"].shape[1] + 1)),
        ("n_pts_main = 0", case, dict(n_main=0)),
        ("n_pts_views = 0 with the TCO view removed", case, dict(n_views=0)),
        ("n_pts_views = 0 with V > 1", plain, dict(n_views=0)),
        ("n_pts_views < 0 with V > 1", plain, dict(n_views=-5)),
        ("n_pts_views = 0, one view, TCO removed", single, dict(n_views=0, code=pc.MV_REMOVE_TCO)),
    ]
    for why, c, over in refused:
        rc, bufs = _prepare_raw(eng, c, c.inputs(), **over)
        assert rc != 0, why
        assert _lib.load().mp_last_error()
        for n, g in bufs.items():
            g.check(f"{why}: {n}", written=False)
    # one view that is the main unit never reads n_pts_views
    rc, bufs = _prepare_raw(eng, single, single.inputs(), n_views=0)
    assert rc == 0
    for n, g in bufs.items():
        g.check(n)
    with pytest.raises(_lib.EngineError):
        eng.pose_prepare(_cu(inp["TCO_in"]), _cu(inp["K"]), _cu(inp["mesh_ids"]), _cu(inp["points"]), case.n_main, 0, case.V, case.code, case.im_hw, case.out_hw)
    u = {k: _cu(v) for k, v in pc.update_inputs(16).items()}
    out = Guarded(16, 4, 4)
    for stride in (8, 0, -9):
        assert _lib.load().mp_pose_update(u["TCO"].data_ptr(), u["KV_crop"].data_ptr(), stride, u["out9"].data_ptr(), u["tCR"].data_ptr(), 16, out.ptr,
                                          eng._stream()) != 0
    torch.cuda.synchronize()
    out.check("pose_update with k_stride_floats < 9", written=False)
    with pytest.raises(_lib.EngineError):
        eng.pose_update(u["TCO"], u["KV_crop"], u["out9"], u["tCR"], k_stride_floats=8)
