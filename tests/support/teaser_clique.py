"""TEST SUPPORT: ctypes wrapper of the host emulation of the exact maximum-clique inlier selection (tests/teaser_clique_emul.cpp, the rule
of megapose6d_amd/csrc/teaser_clique_core.h), built on first use; an independent plain-Python Bron-Kerbosch that lists every maximum
clique; and the seeded graphs the CPU contract test and the GPU test share."""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import teaser as ts
from .emul import CSRC, TESTS, _f32, _i32, _p, build

CLIQUE_INFO = ("size", "upper_bound", "exact", "steps")
FULL_BUDGET = 1 << 20      # steps: above every fixture of the two test files (the largest needs about 8e4), under the entry points' ceiling


def load():
    lib = build("teaser_clique_emul", [TESTS / "teaser_clique_emul.cpp", TESTS / "teaser_emul.cpp", CSRC / "teaser_clique_core.h", CSRC / "teaser_core.h"])
    for name in ("teaser_clique_emul_max_clique", "teaser_clique_emul_solve", "teaser_clique_emul_refine"):
        getattr(lib, name).restype = C.c_int
    lib.teaser_clique_emul_limits.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_int * 4)()
    load().teaser_clique_emul_limits(v)
    return dict(info=int(v[0]), default_steps=int(v[1]), step_ceiling=int(v[2]), selection=int(v[3]))


# the emulation ---------------------------------------------------------------------------------------------------------------------------
def emul_max_clique(adjacency, counts=None, max_steps: int = FULL_BUDGET) -> Tuple[np.ndarray, np.ndarray]:
    """adjacency [n,stride,stride] (or one [stride,stride]) -> members [n,stride] int32 (-1 past the size), info [n,4] = CLIQUE_INFO"""
    a = np.ascontiguousarray(adjacency, np.uint8)
    a = a[None] if a.ndim == 2 else a
    n, stride = a.shape[0], a.shape[1]
    assert a.shape == (n, stride, stride)
    c = None if counts is None else _i32(counts)
    members, info = np.empty((n, stride), np.int32), np.empty((n, 4), np.int32)
    rc = load().teaser_clique_emul_max_clique(_p(a), _p(c), C.c_int(n), C.c_int(stride), C.c_int(max_steps), _p(members), _p(info))
    assert rc == 0
    return members, info


def emul_solve(src, dst, counts, noise_bound: float = ts.NOISE_BOUND, min_num_inliers: int = 0, inlier_selection: str = "kcore",
               rotation_tim_graph: str = "chain", max_steps: int = FULL_BUDGET):
    """support.teaser.emul_solve with the selection "max_clique" beside its own; in that mode the dict also holds clique [n,4]"""
    if inlier_selection != "max_clique":
        return ts.emul_solve(src, dst, counts, noise_bound, min_num_inliers, inlier_selection, rotation_tim_graph)
    s, d, c = _f32(src), _f32(dst), _i32(counts)
    n, stride = s.shape[0], s.shape[1]
    out = dict(Rt=np.empty((n, 3, 4), np.float64), retval=np.empty(n, np.int32), degree=np.empty((n, stride), np.int32),
               core=np.empty((n, stride), np.int32), selected=np.empty((n, stride), np.int32), info=np.empty((n, 5), np.int32),
               clique=np.empty((n, 4), np.int32))
    rc = load().teaser_clique_emul_solve(_p(s), _p(d), _p(c), C.c_int(n), C.c_int(stride), C.c_float(noise_bound), C.c_int(ts.TIM_GRAPHS[rotation_tim_graph]),
                                         C.c_int(min_num_inliers), C.c_int(max_steps), _p(out["Rt"]), _p(out["retval"]), _p(out["degree"]), _p(out["core"]),
                                         _p(out["selected"]), _p(out["info"]), _p(out["clique"]))
    assert rc == 0
    return out


def emul_refine(depth_meas, im_ids, depth_rend, K_rows, TCO, mask_type="simple", depth_delta_thresh=0.1, n_min_points=100, n_points=1000,
                noise_bound=ts.NOISE_BOUND, min_num_inliers=50, use_farthest_point_sampling=True, rotation_tim_graph="chain", max_steps: int = FULL_BUDGET):
    """support.teaser.emul_refine in the selection "max_clique"; the dict also holds clique [n,4]"""
    dm, dr, K, T, ids = _f32(depth_meas), _f32(depth_rend), _f32(K_rows), _f32(TCO), _i32(im_ids)
    n, (B, H, W) = len(T), dm.shape
    assert dr.shape == (n, H, W) and K.shape == (n, 3, 3) and T.shape == (n, 4, 4)
    out = dict(TCO=np.empty((n, 4, 4), np.float32), retval=np.empty(n, np.int32), Rt=np.empty((n, 3, 4), np.float64),
               sample_idx=np.empty((n, n_points), np.int32), degree=np.empty((n, n_points), np.int32), core=np.empty((n, n_points), np.int32),
               selected=np.empty((n, n_points), np.int32), info=np.empty((n, 5), np.int32), clique=np.empty((n, 4), np.int32))
    rc = load().teaser_clique_emul_refine(_p(dm), C.c_int(B), _p(ids), _p(dr), _p(K), _p(T), C.c_int(n), C.c_int(H), C.c_int(W), C.c_int(ts.MASK_TYPES[mask_type]),
                                          C.c_float(depth_delta_thresh), C.c_int(n_min_points), C.c_int(n_points), C.c_float(noise_bound),
                                          C.c_int(min_num_inliers), C.c_int(int(use_farthest_point_sampling)), C.c_int(ts.TIM_GRAPHS[rotation_tim_graph]),
                                          C.c_int(max_steps), _p(out["TCO"]), _p(out["retval"]), _p(out["Rt"]), _p(out["sample_idx"]), _p(out["degree"]),
                                          _p(out["core"]), _p(out["selected"]), _p(out["info"]), _p(out["clique"]))
    assert rc == 0
    return out


# the brute force --------------------------------------------------------------------------------------------------------------------------
def bron_kerbosch(adj) -> Tuple[int, List[Tuple[int, ...]]]:
    """-> (the clique number, every maximum clique as an ascending tuple, sorted).  Bron-Kerbosch with a pivot on Python integers as
    vertex sets; a branch is left only when it cannot reach the largest size seen so far."""
    a = np.asarray(adj).astype(bool)
    a = a | a.T
    n = len(a)
    nb = [sum(1 << j for j in range(n) if a[i, j] and i != j) for i in range(n)]
    best = [0]
    found: List[Tuple[int, ...]] = []

    def bits(s):
        while s:
            low = s & -s
            yield low.bit_length() - 1
            s ^= low

    def go(R, P, X):
        if not P and not X:
            if len(R) > best[0]:
                best[0] = len(R)
                found.clear()
            if len(R) == best[0]:
                found.append(tuple(sorted(R)))
            return
        if len(R) + bin(P).count("1") < best[0]:
            return
        pivot = max(bits(P | X), key=lambda u: bin(P & nb[u]).count("1"))
        for v in bits(P & ~nb[pivot]):
            go(R + [v], P & nb[v], X & nb[v])
            P &= ~(1 << v)
            X |= 1 << v

    go([], (1 << n) - 1, 0)
    return best[0], sorted(found)


def is_clique(adj, members) -> bool:
    a = np.asarray(adj).astype(bool)
    a = a | a.T
    m = list(members)
    return len(set(m)) == len(m) and all(a[i, j] for i in m for j in m if i != j)


def members_of(row) -> List[int]:
    """one row of a members array -> the list before the -1 fill (which must be all that follows)"""
    row = np.asarray(row)
    k = int((row >= 0).sum())
    assert (row[:k] >= 0).all() and (row[k:] == -1).all() and (np.diff(row[:k]) > 0).all()
    return row[:k].tolist()


# graphs -------------------------------------------------------------------------------------------------------------------------------------
def gnp(n: int, p: float, seed: int) -> np.ndarray:
    """G(n, p), symmetric uint8 [n,n]"""
    a = np.triu(np.random.RandomState(seed).rand(n, n) < p, 1).astype(np.uint8)
    return a + a.T


def planted(n: int, k: int, p_in: float, p_bg: float, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """G(n, p_bg) with edge probability p_in among k seeded vertices -> (adjacency, the planted vertices ascending)"""
    rng = np.random.RandomState(seed)
    who = np.sort(rng.permutation(n)[:k])
    p = np.full((n, n), p_bg)
    p[np.ix_(who, who)] = p_in
    a = np.triu(rng.rand(n, n) < p, 1).astype(np.uint8)
    return a + a.T, who


def counter_example() -> np.ndarray:
    """a 4-clique (core number 3) beside K5,5 (core number 5, largest clique 2): the k-core rule selects the bipartite part"""
    a = np.zeros((14, 14), np.uint8)
    for i in range(4):
        for j in range(4):
            a[i, j] = i != j
    for i in range(5):
        for j in range(5):
            a[4 + i, 9 + j] = a[9 + j, 4 + i] = 1
    return a


BUDGET_GRAPH = (70, 0.85, 0)      # gnp arguments: about 8e4 steps, a clique of 20
SMALL_BUDGET = 1000


@lru_cache(maxsize=None)
def stride70_rows() -> Tuple[np.ndarray, np.ndarray]:
    """one launch at stride 70: rows of 1, 2, 14 (the counter-example), 31, 32, 33, 64, 65, 70 vertices -- the word and the wave edges --
    embedded in [9,70,70] with asymmetric junk and a diagonal past nothing: an entry set on one side only is still an edge, the diagonal
    never is, and what lies past a row's count is not read.  -> (adjacency, counts); read-only"""
    counts = np.asarray([1, 2, 14, 31, 32, 33, 64, 65, 70], np.int32)
    a = np.zeros((len(counts), 70, 70), np.uint8)
    for r, n in enumerate(counts):
        g = counter_example() if n == 14 else gnp(int(n), 0.3 + 0.06 * r, 50 + r)
        a[r, :n, :n] = np.triu(g)            # one side only: the packing makes it symmetric
        a[r, np.arange(n), np.arange(n)] = 1    # loops are no edges
        a[r, n:, :] = 1                      # past the count
        a[r, :, n:] = 1
    a.setflags(write=False)
    counts.setflags(write=False)
    return a, counts


@lru_cache(maxsize=None)
def stride1024_rows() -> Tuple[np.ndarray, np.ndarray]:
    """one launch at stride 1024 (bits above 992, the full LDS footprint): 300 planted in background 0.05 (the shortcut), 40 planted in
    background 0.05 (about 2e3 steps), G(1024, 0.1) (about 8e4 steps).  -> (adjacency [3,1024,1024], counts); read-only"""
    a = np.stack([planted(1024, 300, 1.0, 0.05, 1)[0], planted(1024, 40, 1.0, 0.05, 2)[0], gnp(1024, 0.1, 3)])
    counts = np.asarray([1024, 1024, 1024], np.int32)
    a.setflags(write=False)
    counts.setflags(write=False)
    return a, counts


@lru_cache(maxsize=None)
def emul_rows(which: str, max_steps: int = FULL_BUDGET):
    """the emulation's result of one of the two launches above, computed once"""
    a, counts = stride70_rows() if which == "stride70" else stride1024_rows()
    out = emul_max_clique(a, counts, max_steps)
    for x in out:
        x.setflags(write=False)
    return out


def exhausting_row(seed: int = 0) -> np.ndarray:
    """the row of the step-cost benchmark: 300 planted vertices with internal edge probability 0.98 among 1024, background 0.05"""
    return planted(1024, 300, 0.98, 0.05, seed)[0]
