"""CPU: the contract of BOP's model info (csrc/model_info_core.h).  The host emulation (tests/model_info_emul.cpp: the lines the kernel
compiles) against a float64 brute force on seeded point sets and on sets that pin the tie-break; its invariance under the tile and
under the order of the jobs, bit for bit; the prefix array of job counts against a count of the (i-block, j-chunk) pairs; the
models_info.json round trip; and the `diameters=` keyword.  bop_toolkit is absent: the result is unpinned against calc_pts_diameter.

The bound on the emulated pair's float64 distance against the brute-force maximum is 1e-6 relative (support.model_info.REL_BOUND): each
fp32 difference is exact to 2^-24 relative and the three-term sum adds at most 3 ulp, so a pair whose fp32 d2 wins can be short of the
true maximum by about 4 * 2^-24 = 2.4e-7; 1e-6 is that figure with a factor 4 of margin."""
import json
import math
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch

from support import model_info as mi

GOLDEN = Path(__file__).resolve().parent / "golden"


def _ev():
    from megapose6d_amd import evaluation as ev

    return ev


@pytest.mark.parametrize("name", sorted(mi.cases()))
def test_emulation_against_float64_brute_force(name):
    c = mi.cases()[name]
    p = c["points"]
    d2, pair, bounds = mi.emul_case(name, 0)
    assert 0 <= pair[0] <= pair[1] < len(p)
    want, got = mi.brute_force(p), mi.pair_distance(p, pair)
    print(f"{name}: n {len(p)}, brute force {want!r}, emulated pair {pair} at {got!r}, relative gap {abs(got - want) / max(want, 1e-300):.3e}")
    assert abs(got - want) <= mi.REL_BOUND * want
    assert abs(float(d2) - got * got) <= mi.REL_BOUND * got * got          # the fp32 d2 is that pair's
    assert np.array_equal(bounds.view(np.uint32), mi.numpy_bounds(p).view(np.uint32))
    if c["pair"] is not None:
        assert pair == c["pair"]


def test_one_point_and_the_cylinder():
    d2, pair, _ = mi.emul_case("random_1", 0)
    assert float(d2) == 0.0 and pair == (0, 0)
    p = mi.cases()["cylinder"]["points"]
    assert len(p) == 300
    _, pair, bounds = mi.emul_case("cylinder", 0)
    exact, box = mi.pair_distance(p, pair), float(np.linalg.norm(bounds[3:].astype(np.float64)))
    assert abs(exact - math.sqrt(4 * mi.CYL_R ** 2 + mi.CYL_H ** 2)) <= 1e-6 * exact
    assert abs(box - math.sqrt(8 * mi.CYL_R ** 2 + mi.CYL_H ** 2)) <= 1e-6 * box and exact < box


def test_emulation_is_invariant_under_tile_and_job_order():
    rng = np.random.RandomState(0)
    for name, c in mi.cases().items():
        p = c["points"]
        ref = mi.emul_case(name, 0)
        for tile in (64, 128, 256):
            got = mi.emul_case(name, tile)
            assert np.float32(got[0]).view(np.uint32) == np.float32(ref[0]).view(np.uint32) and got[1] == ref[1], (name, tile)
            assert np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32))
            n_jobs = int(mi.prefix([len(p)], tile)[-1])
            d2, pair, _ = mi.emul(p[None], [len(p)], tile, job_order=rng.permutation(n_jobs))
            assert d2.view(np.uint32)[0] == np.float32(ref[0]).view(np.uint32) and tuple(pair[0]) == ref[1], (name, tile)
    # the forced tiles split 1025 points into several jobs, the default does not: both sides of that were compared
    assert mi.prefix([1025], 64)[-1] > 1 and mi.prefix([1025], 0)[-1] == 5


def test_three_objects_padding_and_nan():
    points, n = mi.three_objects()
    singles = [mi.emul_case(k, 64) for k in ("duplicates", "extremes_first_last", "random_65")]
    for tile in mi.TILES:
        d2, pair, bounds = mi.emul(points, n, tile)
        for o, s in enumerate(singles):
            assert d2.view(np.uint32)[o] == np.float32(s[0]).view(np.uint32) and tuple(pair[o]) == s[1]
            assert np.array_equal(bounds[o].view(np.uint32), s[2].view(np.uint32))
        assert (bounds[:, :3] + bounds[:, 3:] < 50).all()           # the padding 100 m away was never a point
    bad, _ = mi.three_objects(with_nan=True)
    d2, pair, bounds = mi.emul(bad, n, 128)
    assert np.isnan(d2[1]) and tuple(pair[1]) == (-1, -1) and np.isnan(bounds[1]).all()
    for o in (0, 2):
        assert d2.view(np.uint32)[o] == np.float32(singles[o][0]).view(np.uint32) and tuple(pair[o]) == singles[o][1]
        assert np.array_equal(bounds[o].view(np.uint32), singles[o][2].view(np.uint32))


def _count_jobs(n, block, chunk):
    """the (i-block, j-chunk) pairs whose chunk does not end before the block starts, counted one by one"""
    n_blocks, n_chunks = -(-n // block), -(-n // chunk)
    return sum(1 for b in range(n_blocks) for c in range(n_chunks) if (c + 1) * chunk > b * block)


@pytest.mark.parametrize("tile", [0, 64, 128, 256, 512, 1024])
def test_prefix_array_of_job_counts(tile):
    lim = mi.limits()
    chunk = lim["default_chunk"] if tile == 0 else -(-tile // lim["block"]) * lim["block"]
    for n in (1, 256, 257, 1025, 20000):
        off = mi.prefix([n], tile)
        assert off.shape == (2,) and off[0] == 0 and off[1] == _count_jobs(n, lim["block"], chunk), (n, tile)
        # every job decodes to its own (block, chunk), with a j range that is not empty, starts at or after the block and ends inside
        seen = set()
        for k in range(int(off[1])):
            b, c, j0, j1 = mi.decode(k, tile, n)
            assert (c + 1) * chunk > b * lim["block"] and b * lim["block"] < n and max(c * chunk, b * lim["block"]) == j0 < j1 <= min(n, (c + 1) * chunk)
            seen.add((b, c))
        assert len(seen) == off[1]
    two = mi.prefix([1025, 257], tile)
    assert two.shape == (3,) and two.dtype == np.int32            # n_obj + 1 entries, whatever the objects' sizes
    assert two[1] == _count_jobs(1025, lim["block"], chunk) and two[2] - two[1] == _count_jobs(257, lim["block"], chunk)
    assert mi.prefix([10 ** 6], 0).shape == (2,) and mi.prefix([10 ** 6], 0)[-1] < 2 ** 18


def test_bad_arguments_give_no_prefix():
    assert mi.prefix([5, 0], 0) is None and mi.prefix([5], 32) is None and mi.prefix([5], 96) is None and mi.prefix([5], 2048) is None
    assert mi.prefix([2 ** 31 - 1], 64) is None                    # more jobs than a launch has


# models_info.json --------------------------------------------------------------------------------------------------------------------
def _table():
    ev = _ev()
    names = ["obj_000003", "obj_000011", "mug"]
    keys = ("cylinder", "cube", "random_65")
    res = [mi.emul_case(k, 0) for k in keys]
    pts = [mi.cases()[k]["points"] for k in keys]
    return ev.model_info_table(names, [r[1] for r in res], [r[2] for r in res], [p[r[1][0]] for p, r in zip(pts, res)],
                               [p[r[1][1]] for p, r in zip(pts, res)]), pts, res


def test_model_info_table_and_the_models_info_round_trip(tmp_path):
    ev = _ev()
    info, pts, res = _table()
    assert list(info.columns) == list(ev.MODEL_INFO_COLUMNS) and list(info.index) == ["obj_000003", "obj_000011", "mug"]
    for k in range(3):
        assert info["diameter"].iloc[k] == mi.pair_distance(pts[k], res[k][1])        # float64 of the two fp32 points, not sqrt(d2)
        assert (info["pt_i"].iloc[k], info["pt_j"].iloc[k]) == res[k][1]
    assert info.loc["obj_000011", "diameter"] == math.sqrt(3.0) and info.loc["obj_000011", ["size_x", "size_y", "size_z"]].tolist() == [1.0] * 3
    bop = ev.bop_models_info(info)
    assert list(bop) == [3, 11, "mug"] and set(bop[3]) == {"diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z"}
    assert bop[11]["diameter"] == math.sqrt(3.0) * 1000.0 and bop[11]["size_y"] == 1000.0
    path = tmp_path / "models_info.json"
    ev.save_models_info(path, info)
    assert set(json.loads(path.read_text())) == {"3", "11", "mug"}
    back = ev.load_models_info(path)
    assert set(back) == set(info.index)
    for label in info.index:
        assert back[label] == info.loc[label, "diameter"] * 1000.0 * 0.001           # float64 equality after the mm scale
    ev.save_models_info(path, bop)                                                       # a dict that is already BOP's
    assert ev.load_models_info(path) == back
    with pytest.raises(ValueError):
        ev.bop_models_info(info.rename(index={"mug": "11"}))


def test_golden_models_info_loads_with_its_symmetry_fields():
    ev = _ev()
    diam, infos = ev.load_models_info(GOLDEN / "models_info_small.json", return_info=True)
    assert diam == {"obj_000001": 172.063 * 0.001, "obj_000012": 223.606797749979 * 0.001}
    assert "symmetries_discrete" not in infos["obj_000001"]
    assert len(infos["obj_000012"]["symmetries_discrete"][0]) == 16 and infos["obj_000012"]["symmetries_continuous"][0]["axis"] == [0, 0, 1]
    assert ev.load_models_info(GOLDEN / "models_info_small.json", scale=1.0, label_format="{}") == {"1": 172.063, "12": 223.606797749979}


# the diameters= keyword ---------------------------------------------------------------------------------------------------------------
def _meshes():
    pts = [mi.cases()["cylinder"]["points"], mi.cases()["random_65"]["points"]]
    labels = ["can", "blob"]
    points = np.full((2, 320, 3), 100.0, np.float32)
    for o, p in enumerate(pts):
        points[o, :len(p)] = p
    infos = {l: {"n_points": len(p), "n_sym": 1} for l, p in zip(labels, pts)}
    return SimpleNamespace(labels=np.asarray(labels), infos=infos, points=torch.from_numpy(points)), pts


def test_diameters_keyword():
    ev = _ev()
    meshes, pts = _meshes()
    box = ev._diameters(meshes)
    for l, p in zip(meshes.labels, pts):
        assert box[l] == float(np.linalg.norm((p.max(0) - p.min(0)).astype(np.float64)))
    assert ev.resolve_diameters(meshes, None, ["can", "blob", "can"]) is box                # None: today's table itself
    given = {"can": 0.2, "blob": 0.31, "other": float("nan")}
    assert ev.resolve_diameters(meshes, given, ["blob", "can", "blob"]) == {"blob": 0.31, "can": 0.2}
    with pytest.raises(KeyError):
        ev.resolve_diameters(meshes, {"can": 0.2}, ["can", "blob"])
    for bad in (0.0, float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError):
            ev.resolve_diameters(meshes, {"can": bad, "blob": 0.3}, ["can"])
    with pytest.raises(ValueError):
        ev.resolve_diameters(meshes, "bop", ["can"])
    # "exact" reads the table of `model_info` kept on the meshes: here the emulation's, through the host half of `model_info`
    res = [mi.emul(p[None], [len(p)])[1:] for p in pts]
    table = ev.model_info_table(meshes.labels, [r[0][0] for r in res], [r[1][0] for r in res], [p[r[0][0, 0]] for p, r in zip(pts, res)],
                                [p[r[0][0, 1]] for p, r in zip(pts, res)])
    object.__setattr__(meshes, "_model_info", table)
    exact = ev.resolve_diameters(meshes, "exact", ["can", "blob"])
    assert exact["can"] < box["can"] and abs(exact["can"] - math.sqrt(4 * mi.CYL_R ** 2 + mi.CYL_H ** 2)) <= 1e-6 * exact["can"]
    assert abs(box["can"] - math.sqrt(8 * mi.CYL_R ** 2 + mi.CYL_H ** 2)) <= 1e-6 * box["can"]
    assert exact["blob"] <= box["blob"] and abs(exact["blob"] - mi.brute_force(pts[1])) <= mi.REL_BOUND * exact["blob"]
    assert ev.resolve_diameters(meshes, None, ["can"]) is box                               # the default is untouched by the exact table
    # the thresholds follow: MSSD's theta * d
    thr_box, thr_exact = ev.bop_thresholds([box["can"]]), ev.bop_thresholds([exact["can"]])
    assert (thr_exact[0, -2] < thr_box[0, -2]).all() and np.array_equal(thr_exact[0, :-2], thr_box[0, :-2])
