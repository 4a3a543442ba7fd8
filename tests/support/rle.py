"""TEST SUPPORT: ctypes wrapper of the host emulation of the run-length kernels (tests/rle_emul.cpp), built on first use; an independent
numpy restatement of the format written from the contract's text and not from csrc/rle_core.h (`ravel(order="F")`, `flatnonzero`, `diff`,
`repeat`; the compressed string digit by digit); and the shapes, mask kinds and malformed lists the CPU contract test and the GPU test
share."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .emul import CSRC, TESTS, _p, build

SHAPES = [(1, 1), (1, 67), (67, 1), (3, 5), (63, 65), (64, 64), (65, 257)]
KINDS = ("empty", "full", "checker_set", "checker_unset", "noise", "rectangle", "first_pixel", "last_pixel", "run_across_columns",
         "transition_at_column")
SET_VALUES = np.array([1, 2, 128, 255], np.uint8)
STATUS_EMPTY, STATUS_NEGATIVE, STATUS_SUM = 1, 2, 4


def load():
    lib = build("rle_emul", [TESTS / "rle_emul.cpp", CSRC / "rle_core.h", CSRC / "det_ap_core.h", CSRC / "bop_match_core.h"], fma=False)
    for name in ("rle_count_emul", "rle_encode_emul", "rle_decode_emul"):
        getattr(lib, name).restype = C.c_int
    lib.rle_emul_limits.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_longlong * 3)()
    load().rle_emul_limits(v)
    return dict(max_pixels=int(v[0]), default_rows=int(v[1]), unit=int(v[2]))


def _masks_u8(masks) -> np.ndarray:
    masks = np.asarray(masks)
    masks = masks.view(np.uint8) if masks.dtype == np.bool_ else masks
    assert masks.dtype == np.uint8 and masks.ndim == 3
    return np.ascontiguousarray(masks)


def emul_count(masks, rows_per_segment=0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    masks = _masks_u8(masks)
    n, h, w = masks.shape
    n_counts, areas, boxes = np.empty(n, np.int32), np.empty(n, np.int32), np.empty((n, 4), np.int32)
    rc = load().rle_count_emul(_p(masks), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(rows_per_segment), _p(n_counts), _p(areas), _p(boxes))
    assert rc == 0
    return n_counts, areas, boxes


def emul_encode(masks, rows_per_segment=0) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """-> counts [total] int32, offsets [n + 1] int64, areas, boxes: what `engine.rle_encode` returns"""
    masks = _masks_u8(masks)
    n, h, w = masks.shape
    n_counts, areas, boxes = emul_count(masks, rows_per_segment)
    offsets = np.concatenate([[0], np.cumsum(n_counts, dtype=np.int64)]).astype(np.int64)
    counts = np.full(int(offsets[-1]), -7, np.int32)
    rc = load().rle_encode_emul(_p(masks), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(rows_per_segment), _p(offsets), _p(counts),
                                C.c_longlong(len(counts)))
    assert rc == 0
    return counts, offsets, areas, boxes


def emul_decode(counts, offsets, h, w) -> Tuple[np.ndarray, np.ndarray]:
    counts, offsets = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(offsets, np.int64)
    n = len(offsets) - 1
    masks, status = np.full((n, h, w), 9, np.uint8), np.full(n, -1, np.int32)
    rc = load().rle_decode_emul(_p(counts), _p(offsets), C.c_longlong(len(counts)), C.c_int(n), C.c_int(h), C.c_int(w), _p(masks), _p(status))
    assert rc == 0
    return masks, status


# the restatement ----------------------------------------------------------------------------------------------------------------------
def restated_counts(mask) -> List[int]:
    """One mask [h,w] -> its list: the set pixels in column-major order with v[-1] := 0, the positions where the value changes, the
    differences of 0, the positions and h * w."""
    v = (np.asarray(mask) != 0).ravel(order="F").astype(np.int8)
    pos = np.flatnonzero(np.diff(np.concatenate([[0], v])))
    return np.diff(np.concatenate([[0], pos, [v.size]])).astype(np.int64).tolist()


def restated_mask(counts: Sequence[int], h: int, w: int) -> Tuple[np.ndarray, int]:
    """A list -> (mask [h,w] uint8 0 / 1, status): malformed (no entries, a negative one, a sum that is not h * w) gives zeros."""
    c = np.asarray(counts, np.int64).reshape(-1)
    status = (STATUS_EMPTY if c.size == 0 else 0) | (STATUS_NEGATIVE if (c < 0).any() else 0) | (STATUS_SUM if int(c.sum()) != h * w else 0)
    if status:
        return np.zeros((h, w), np.uint8), status
    v = np.repeat(np.arange(c.size) % 2, c).astype(np.uint8)
    return np.ascontiguousarray(v.reshape((h, w), order="F")), 0


def restated_area_box(mask) -> Tuple[int, List[int]]:
    ys, xs = np.nonzero(np.asarray(mask) != 0)
    if len(ys) == 0:
        return 0, [0, 0, -1, -1]
    return int(len(ys)), [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def restated_encode(masks) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    lists = [restated_counts(m) for m in masks]
    offsets = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    stats = [restated_area_box(m) for m in masks]
    return (np.asarray([c for l in lists for c in l], np.int32), offsets, np.asarray([s[0] for s in stats], np.int32),
            np.asarray([s[1] for s in stats], np.int32).reshape(-1, 4))


def restated_to_string(counts: Sequence[int]) -> str:
    """pycocotools' rleToString from the contract's text: from the fourth entry on the difference to the entry two before; then five bits
    at a time, lowest first, bit 0x20 = more follow, a digit is chr(48 + bits); the number ends when what is left is all sign."""
    out = []
    for i, x in enumerate(int(c) for c in counts):
        if i > 2:
            x -= int(counts[i - 2])
        while True:
            c = x & 0x1F
            x >>= 5                      # (Python's >> on a negative int is arithmetic, as in C on the int the packages use)
            more = (x != -1) if (c & 0x10) else (x != 0)
            out.append(chr((c | 0x20 if more else c) + 48))
            if not more:
                break
    return "".join(out)


def restated_from_string(s: str) -> List[int]:
    counts: List[int] = []
    i = 0
    while i < len(s):
        x, k = 0, 0
        while True:
            c = ord(s[i]) - 48
            i += 1
            x |= (c & 0x1F) << (5 * k)
            k += 1
            if not (c & 0x20):
                if c & 0x10:
                    x |= -1 << (5 * k)
                break
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


# masks ----------------------------------------------------------------------------------------------------------------------------------
def make_mask(kind: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    """[h,w] uint8.  The set bytes of "noise" are drawn from {1, 2, 128, 255}; the others are 1 or 255."""
    m = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "empty":
        pass
    elif kind == "full":
        m[:] = 255
    elif kind == "checker_set":          # pixel (0, 0) set: on 3 x 5 every pixel is a run, h * w + 1 counts
        m[(yy + xx) % 2 == 0] = 1
    elif kind == "checker_unset":
        m[(yy + xx) % 2 == 1] = 1
    elif kind == "noise":
        rng = np.random.RandomState(1000 + 31 * seed + 7 * h + w)
        m = np.where(rng.uniform(size=(h, w)) < 0.5, SET_VALUES[rng.randint(0, 4, size=(h, w))], 0).astype(np.uint8)
    elif kind == "rectangle":
        m[h // 4:max(h // 4 + 1, (3 * h) // 4), w // 3:max(w // 3 + 1, (2 * w) // 3)] = 255
    elif kind == "first_pixel":
        m[0, 0] = 2
    elif kind == "last_pixel":
        m[h - 1, w - 1] = 128
    elif kind == "run_across_columns":   # the bottom of column x and the top of column x + 1 both set: one run
        x = (w - 1) // 2
        m[h - 1, x] = 1
        m[0, min(x + 1, w - 1)] = 1
    elif kind == "transition_at_column":  # the whole of one column set: its run starts and ends exactly at column boundaries
        m[:, w // 2] = 255
    else:
        raise ValueError(kind)
    return m


def batch(kinds: Sequence[str], h: int, w: int, seed: int = 0) -> np.ndarray:
    return np.stack([make_mask(k, h, w, seed + i) for i, k in enumerate(kinds)])


def blobs(n: int, h: int, w: int, seed: int = 0, share: float = 0.1) -> np.ndarray:
    """n masks of one ellipse each covering about `share` of the frame, bytes 0 / 1"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        ratio = rng.uniform(0.5, 2.0)
        ry = np.sqrt(share * h * w / np.pi * ratio)
        rx = share * h * w / np.pi / ry
        cy, cx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w
        out[i] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0).astype(np.uint8)
    return out


def malformed(h: int, w: int) -> Dict[str, Tuple[Optional[List[int]], int]]:
    """name -> (list, expected status) for an h x w mask with h * w >= 4"""
    hw = h * w
    return {
        "negative entry": ([3, -1, hw - 2], STATUS_NEGATIVE),
        "short sum": ([1, 2], STATUS_SUM) if hw != 3 else ([1, 1], STATUS_SUM),
        "long sum": ([1, hw], STATUS_SUM),
        "no entries": ([], STATUS_EMPTY | STATUS_SUM),
        "negative and wrong sum": ([-2, 1], STATUS_NEGATIVE | STATUS_SUM),
    }


def zero_run_lists(h: int, w: int) -> List[List[int]]:
    """well-formed lists (no negative entry, sum h * w, for h * w >= 15) with runs of length zero inside: no encoder writes them, a
    file may hold them, and the pixel after one belongs to a run further on"""
    hw = h * w
    return [[0, 0, hw], [2, 0, 0, 3, 0, hw - 5], [0, 1, 0, 0, 0, 1, hw - 2], [hw, 0, 0], [hw - 7, 0, 0, 0, 0, 0, 7],
            [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, hw - 4], [0] * 40 + [hw // 2, 0, 0, 0, hw - hw // 2]]


def ragged(lists: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    offsets = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return np.asarray([c for l in lists for c in l], np.int32), offsets
