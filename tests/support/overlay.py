"""TEST SUPPORT: the prediction overlays (megapose6d_amd/csrc/overlay.hip).  An independent numpy restatement of the contract, written
literally on whole images (per label: OpenCV's Canny on the 0 / 255 mask with its real thresholds, k rounds of a 3x3 dilation, labels
painted in ascending order; numpy's evaluation of the blend; boxes painted in ascending order); the ctypes wrapper of the host emulation
(tests/overlay_emul.cpp), built on first use; and the seeded cases the CPU contract test and the GPU test share."""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .emul import CSRC, TESTS, _p, build

SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (13, 17), (48, 64))     # (h, w)
DILATIONS = (0, 1, 2, 8)
LABEL_POOL = (0, 1, 2, 3, 7, 12, 25)            # with 5 colours: labels above n_colors, and two labels (2, 7, 12) of one colour
COLORS = np.asarray([[255, 0, 0], [0, 255, 0], [10, 20, 250], [1, 2, 3], [200, 200, 0]], np.uint8)
OUTPUTS = ("contour", "canny", "mask", "mesh")


def load():
    lib = build("overlay_emul", [TESTS / "overlay_emul.cpp", CSRC / "overlay_core.h"])
    lib.overlay_emul.restype = C.c_int
    lib.overlay_emul_boxes.restype = C.c_int
    lib.overlay_emul_tables.restype = None
    lib.overlay_emul_limits.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_int * 5)()
    load().overlay_emul_limits(v)
    return dict(tile_w=int(v[0]), tile_h=int(v[1]), max_dilate=int(v[2]), max_thickness=int(v[3]), max_side=int(v[4]))


def emul_tables() -> Tuple[np.ndarray, np.ndarray]:
    obj, bg = np.empty(256, np.uint8), np.empty(256, np.uint8)
    load().overlay_emul_tables(_p(obj), _p(bg))
    return obj, bg


def _u8(a):
    return None if a is None else np.ascontiguousarray(a, np.uint8)


def emul(images, render=None, labels=None, colors=COLORS, k: int = 1, tile: Optional[Tuple[int, int]] = None,
         outputs: Sequence[str] = OUTPUTS, rc_only: bool = False):
    """the emulation on the arguments of the C ABI: images [n,h,w,3] uint8, render the same or None, labels [n,h,w] int32 or None;
    tile = (tile_w, tile_h), default the kernel's -> dict of the requested outputs (an output not asked for is passed as NULL)"""
    images = _u8(images)
    n, h, w = images.shape[:3]
    render, colors = _u8(render), _u8(colors)
    labels = None if labels is None else np.ascontiguousarray(labels, np.int32)
    lim = limits()
    tw, th = tile or (lim["tile_w"], lim["tile_h"])
    out = {name: np.full((n, h, w, 3) if name in ("contour", "mesh") else (n, h, w), 0xA5, np.uint8) for name in outputs}
    rc = load().overlay_emul(_p(images), _p(render), _p(labels), _p(colors), C.c_int(len(colors)), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(k),
                             C.c_int(tw), C.c_int(th), *[_p(out.get(name)) for name in OUTPUTS])
    if rc_only:
        return rc
    assert rc == 0
    return out


def emul_boxes(images, boxes, image_ids, colors=COLORS, t: int = 2) -> np.ndarray:
    images, colors = _u8(images), _u8(colors)
    n, h, w = images.shape[:3]
    boxes, ids = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4), np.ascontiguousarray(image_ids, np.int32)
    out = np.full_like(images, 0xA5)
    rc = load().overlay_emul_boxes(_p(images), _p(boxes), _p(ids), C.c_int(len(ids)), _p(colors), C.c_int(len(colors)), C.c_int(n), C.c_int(h),
                                   C.c_int(w), C.c_int(t), _p(out))
    assert rc == 0
    return out


# the restatement ------------------------------------------------------------------------------------------------------------------------
def canny_of_mask(mask: np.ndarray) -> np.ndarray:
    """bool [h,w] -> bool [h,w]: cv2.Canny(255 * mask, 30, 100) (L1 norm, aperture 3) on the whole image.  Sobel with a replicated border,
    magnitudes zero outside the image, OpenCV's suppression rule with its mix of > and >=; a survivor above the high threshold is an
    edge, one between the two needs a neighbour that is one -- which cannot happen here, and is asserted."""
    h, w = mask.shape
    p = np.pad(mask.astype(np.int64) * 255, 1, mode="edge")
    gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    mag = np.abs(gx) + np.abs(gy)
    mz = np.pad(mag, 1)

    def at(dx, dy):
        return mz[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    ax, ay = np.abs(gx), np.abs(gy) << 15
    t = ax * 13573
    horizontal = ay < t
    vertical = ~horizontal & (ay > t + (ax << 16))
    keep_h = (mag > at(-1, 0)) & (mag >= at(1, 0))
    keep_v = (mag > at(0, -1)) & (mag >= at(0, 1))
    keep_same = (mag > at(-1, -1)) & (mag > at(1, 1))        # gx and gy of one sign
    keep_opp = (mag > at(1, -1)) & (mag > at(-1, 1))
    keep = np.where(horizontal, keep_h, np.where(vertical, keep_v, np.where((gx ^ gy) < 0, keep_opp, keep_same)))
    survivors = keep & (mag > 30)
    assert not (survivors & (mag <= 100)).any()
    return survivors & (mag > 100)


def dilate3(a: np.ndarray, k: int) -> np.ndarray:
    """k rounds of a 3x3 dilation of a bool image; nothing enters from outside the image"""
    h, w = a.shape
    for _ in range(k):
        p = np.pad(a, 1)
        a = np.zeros_like(a)
        for dy in range(3):
            for dx in range(3):
                a = a | p[dy:dy + h, dx:dx + w]
    return a


def labels_of_render(render: np.ndarray) -> np.ndarray:
    return (render > 0).any(-1).astype(np.int32) - 1


def blend(image: np.ndarray, render: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """the mesh blend of one image as the contract states it: per channel render * 0.8 + 255 * 0.2 on the mask, image * 0.6 + 255 * 0.4
    off it; a uint8 array times a Python float is float64 in numpy, the result is rounded to float32 and truncated"""
    on, off = render * 0.8 + 255 * 0.2, image * 0.6 + 255 * 0.4
    assert on.dtype == np.float64 and off.dtype == np.float64
    return np.where(mask[..., None], on, off).astype(np.float32).astype(np.uint8)


def restate(images, render=None, labels=None, colors=COLORS, k: int = 1) -> Dict[str, np.ndarray]:
    images = np.asarray(images, np.uint8)
    n, h, w = images.shape[:3]
    if labels is None:
        labels = np.stack([labels_of_render(r) for r in render]) if n else np.zeros((0, h, w), np.int32)
    contour, canny = images.copy(), np.zeros((n, h, w), np.uint8)
    mask = np.where(labels >= 0, 255, 0).astype(np.uint8)
    for i in range(n):
        for l in sorted(int(v) for v in np.unique(labels[i]) if v >= 0):
            fat = dilate3(canny_of_mask(labels[i] == l), k)
            contour[i][fat] = colors[l % len(colors)]
            canny[i][fat] = 255
    out = dict(contour=contour, canny=canny, mask=mask)
    if render is not None:
        out["mesh"] = np.stack([blend(images[i], render[i], labels[i] >= 0) for i in range(n)]) if n else images.copy()
    return out


def restate_boxes(images, boxes, image_ids, colors=COLORS, t: int = 2) -> np.ndarray:
    out = np.asarray(images, np.uint8).copy()
    n, h, w = out.shape[:3]
    ys, xs = np.mgrid[0:h, 0:w]
    g, s = t // 2, (t + 1) // 2
    for j, (box, i) in enumerate(zip(np.asarray(boxes, np.float32).reshape(-1, 4), image_ids)):
        if not 0 <= i < n or np.isnan(box).any():
            continue
        x1, y1, x2, y2 = (int(v) for v in box.astype(np.int64))
        grown = (xs >= x1 - g) & (xs <= x2 + g) & (ys >= y1 - g) & (ys <= y2 + g)
        shrunk = (xs >= x1 + s) & (xs <= x2 - s) & (ys >= y1 + s) & (ys <= y2 - s)
        out[i][grown & ~shrunk] = colors[j % len(colors)]
    return out


# the cases ------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def blob_labels(h: int, w: int, seed: int, cover: bool = False) -> np.ndarray:
    """a label map [h,w] int32 of random ellipses with labels from LABEL_POOL, painted over one another (so instances touch with no
    background between them), some centred at the image border; cover: every pixel takes the label of the nearest of a few seeds instead
    (no background at all).  Images of fewer than 16 pixels draw every pixel from the pool and -1."""
    rng = np.random.RandomState(1000 * seed + 31 * h + w)
    if h * w < 16:
        lab = rng.choice((-1,) + LABEL_POOL[:3], size=(h, w)).astype(np.int32)
    elif cover:
        pts = rng.uniform(0, 1, size=(6, 2)) * (h, w)
        ys, xs = np.mgrid[0:h, 0:w]
        lab = np.asarray(LABEL_POOL, np.int32)[((ys[..., None] - pts[:, 0]) ** 2 + (xs[..., None] - pts[:, 1]) ** 2).argmin(-1)]
    else:
        lab = np.full((h, w), -1, np.int32)
        ys, xs = np.mgrid[0:h, 0:w]
        for b in range(7):
            cy, cx = (rng.uniform(0, h), rng.uniform(0, w)) if b % 3 else (rng.choice((0.0, h - 1.0)), rng.uniform(0, w))
            ry, rx = rng.uniform(1.0, 0.3 * h + 1.5), rng.uniform(1.0, 0.3 * w + 1.5)
            lab[((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0] = LABEL_POOL[rng.randint(len(LABEL_POOL))]
    lab.setflags(write=False)
    return lab


@lru_cache(maxsize=None)
def scene(n: int, h: int, w: int, seed: int):
    """images, render [n,h,w,3] uint8 and labels [n,h,w] int32: the render is non-zero exactly where the label is >= 0 (one channel may be
    zero there), and both images hold every byte value when they have 256 bytes"""
    rng = np.random.RandomState(seed + 7 * n + 13 * h + 17 * w)
    labels = np.stack([blob_labels(h, w, seed + i, cover=(i % 3 == 2)) for i in range(n)])
    images = rng.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    render = rng.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    if images.size >= 256:
        images.reshape(-1)[:256] = np.arange(256)
        render.reshape(-1)[-256:] = np.arange(256)[::-1]
    render[..., 1] |= 1          # somewhere non-zero on the objects ...
    render[..., 0][rng.uniform(size=(n, h, w)) < 0.3] = 0
    render[labels < 0] = 0       # ... and black on the background
    for a in (images, render, labels):
        a.setflags(write=False)
    return images, render, labels


@lru_cache(maxsize=None)
def batch3():
    """n = 3 at 48 x 64, the middle image entirely background"""
    images, render, labels = (a.copy() for a in scene(3, 48, 64, 5))
    labels[1] = -1
    render[1] = 0
    for a in (images, render, labels):
        a.setflags(write=False)
    return images, render, labels


@lru_cache(maxsize=None)
def box_case():
    """two images of 20 x 24 and the boxes of the contract test: inside, partly and wholly outside, degenerate, overlapping (a later box
    over an earlier one), fractional and negative corners, an image id outside the batch, a NaN corner"""
    rng = np.random.RandomState(3)
    images = rng.randint(0, 256, size=(2, 20, 24, 3)).astype(np.uint8)
    boxes = np.asarray([[3.7, 2.2, 15.9, 12.5], [8.0, 6.0, 20.0, 17.0], [-5.5, -4.5, 6.5, 5.5], [18.0, 14.0, 40.0, 30.0], [100.0, 100.0, 120.0, 130.0],
                        [-30.0, -30.0, -10.0, -12.0], [11.0, 1.0, 11.0, 18.0], [2.0, 9.0, 21.0, 9.0], [5.0, 5.0, 5.0, 5.0], [4.0, 4.0, 16.0, 14.0],
                        [1.0, 1.0, 22.0, 18.0], [6.0, 6.0, 12.0, 12.0], [0.0, 0.0, 23.0, 19.0], [2.0, 2.0, np.nan, 9.0], [-0.9, -0.9, 3.9, 3.9]], np.float32)
    ids = np.asarray([0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 1, 0, 1], np.int32)
    for a in (images, boxes, ids):
        a.setflags(write=False)
    return images, boxes, ids
