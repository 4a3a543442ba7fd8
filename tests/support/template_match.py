"""TEST SUPPORT: the training-free detector's three launches (megapose6d_amd/csrc/template_match.hip).  An independent numpy restatement
of the contract, written literally on whole images (no tiles, no linearised layout: it produces r_o(x, y) and re-indexes at the end; the
irrational bin boundaries through floor(sqrt(2) a), not through squares); the ctypes wrapper of the host emulation
(tests/template_match_emul.cpp), built on first use; and the seeded cases the CPU contract test and the GPU test share."""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from typing import Dict, Optional, Tuple

import numpy as np

from .emul import CSRC, TESTS, _p, build

SHAPES = ((1, 1), (1, 7), (7, 1), (3, 3), (8, 8), (13, 17), (48, 64))     # (h, w)
SPREADS = (1, 2, 5, 8)                                                    # T
WEAK = 30                                                                 # weak_threshold of the cases
TEMPLATE_COUNTS = (1, 2, 65, 257)
N_OBJECTS = 3                                                             # of the random tables; object 2 never has a template


def load():
    lib = build("template_match_emul", [TESTS / "template_match_emul.cpp", CSRC / "template_match_core.h"])
    for name in ("tm_emul_quantize", "tm_emul_response", "tm_emul_match", "tm_emul_bin", "tm_emul_better", "tm_emul_resp_tile_w"):
        getattr(lib, name).restype = C.c_int
    lib.tm_emul_limits.restype = None
    return lib


def limits() -> Dict[str, int]:
    v = (C.c_int * 10)()
    load().tm_emul_limits(v)
    names = ("quant_tile_w", "quant_tile_h", "resp_tile_h", "loc_w", "loc_h", "max_t", "max_features", "max_box", "max_weak", "max_side")
    return {k: int(x) for k, x in zip(names, v)}


def resp_tile(T: int) -> Tuple[int, int]:
    return int(load().tm_emul_resp_tile_w(C.c_int(T))), limits()["resp_tile_h"]


def grid(h: int, w: int, T: int) -> Tuple[int, int]:
    return -(-h // T), -(-w // T)


# the emulation ----------------------------------------------------------------------------------------------------------------------------
def emul_quantize(images, blur: bool = True, weak: int = WEAK, tile: Optional[Tuple[int, int]] = None, want_mag2: bool = True, rc_only: bool = False):
    """images uint8 [n,h,w,3]; tile = (tile_w, tile_h), default the kernel's -> ori uint8 [n,h,w], mag2 int32 [n,h,w] (or None)"""
    images = np.ascontiguousarray(images, np.uint8)
    n, h, w = images.shape[:3]
    lim = limits()
    tw, th = tile or (lim["quant_tile_w"], lim["quant_tile_h"])
    ori = np.full((n, h, w), 0xA5, np.uint8)
    mag2 = np.full((n, h, w), -1515870811, np.int32) if want_mag2 else None
    rc = load().tm_emul_quantize(_p(images), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(int(blur)), C.c_int(weak), C.c_int(tw), C.c_int(th), _p(ori),
                                 _p(mag2))
    if rc_only:
        return rc
    assert rc == 0
    return ori, mag2


def emul_response(ori, T: int, tile: Optional[Tuple[int, int]] = None, rc_only: bool = False):
    """ori uint8 [n,h,w] -> resp uint8 [n,8,T,T,gh,gw]"""
    ori = np.ascontiguousarray(ori, np.uint8)
    n, h, w = ori.shape
    if rc_only and not 1 <= T <= 8:
        return load().tm_emul_response(_p(ori), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(T), C.c_int(1), C.c_int(1), _p(np.zeros(1, np.uint8)))
    tw, th = tile or resp_tile(T)
    gh, gw = grid(h, w, T)
    resp = np.full((n, 8, T, T, gh, gw), 0xA5, np.uint8)
    rc = load().tm_emul_response(_p(ori), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(T), C.c_int(tw), C.c_int(th), _p(resp))
    if rc_only:
        return rc
    assert rc == 0
    return resp


def emul_match(resp, h: int, w: int, T: int, templates, features, n_objects: int, tile: Optional[Tuple[int, int]] = None, rc_only: bool = False):
    """resp uint8 [n,8,T,T,gh,gw]; templates int32 [n_templates,5]; features uint8 [n_features,4] -> best_score, best_f uint8 and
    best_template int32, each [n,n_objects,gh,gw]"""
    resp = np.ascontiguousarray(resp, np.uint8)
    templates = np.ascontiguousarray(templates, np.int32).reshape(-1, 5)
    features = np.ascontiguousarray(features, np.uint8).reshape(-1, 4)
    n = resp.shape[0]
    lim = limits()
    tw, th = tile or (lim["loc_w"], lim["loc_h"])
    gh, gw = grid(h, w, T)
    shape = (n, max(n_objects, 0), gh, gw)
    score, f, best = np.full(shape, 0xA5, np.uint8), np.full(shape, 0xA5, np.uint8), np.full(shape, -1515870811, np.int32)
    rc = load().tm_emul_match(_p(resp), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(T), _p(templates), _p(features), C.c_int(len(templates)),
                              C.c_int(len(features)), C.c_int(n_objects), C.c_int(tw), C.c_int(th), _p(score), _p(f), _p(best))
    if rc_only:
        return rc
    assert rc == 0
    return score, f, best


def emul_bin(gx: int, gy: int) -> int:
    return int(load().tm_emul_bin(C.c_int(gx), C.c_int(gy)))


def emul_better(a, b) -> bool:
    return bool(load().tm_emul_better(*[C.c_int(int(v)) for v in (*a, *b)]))


# the restatement --------------------------------------------------------------------------------------------------------------------------
def restate_bin(gx: np.ndarray, gy: np.ndarray) -> np.ndarray:
    """the bin of the angle of (gx, gy) modulo 180 degrees, [k 22.5, (k + 1) 22.5) half open; integers [..] -> int [..] (4 for gx = gy = 0,
    which is never a candidate).  tan 22.5 = sqrt2 - 1 and tan 67.5 = sqrt2 + 1; sqrt2 a is irrational for a > 0, so b < sqrt2 a - a is
    b <= floor(sqrt2 a) - a."""
    gx, gy = np.asarray(gx, np.int64), np.asarray(gy, np.int64)
    flip = (gy < 0) | ((gy == 0) & (gx < 0))
    gx, gy = np.where(flip, -gx, gx), np.where(flip, -gy, gy)
    a, b = np.abs(gx), gy
    root = np.floor(np.sqrt((2 * a * a).astype(np.float64))).astype(np.int64)          # floor(sqrt2 a)
    assert ((root * root <= 2 * a * a) & ((root + 1) * (root + 1) > 2 * a * a)).all()
    under_22, under_45, under_67 = b <= root - a, b < a, b <= root + a                   # the first-quadrant angle of (a, b) under 22.5, 45, 67.5
    first = np.where(under_22, 0, np.where(under_45, 1, np.where(under_67, 2, 3)))      # theta = that angle
    # gx < 0: theta = 180 - phi; theta in [k 22.5, (k + 1) 22.5) <=> phi in (180 - (k + 1) 22.5, 180 - k 22.5]
    second = np.where(under_22 & (a > 0), 7, np.where(b <= a, 6, np.where(under_67, 5, 4)))
    return np.where(gx > 0, first, np.where(gx == 0, 4, second))


def restate_quantize(images, blur: bool = True, weak: int = WEAK):
    images = np.asarray(images, np.uint8)
    n, h, w = images.shape[:3]
    ori, mag2 = np.zeros((n, h, w), np.uint8), np.zeros((n, h, w), np.int32)
    k = np.asarray([1, 4, 6, 4, 1], np.int64)
    for i in range(n):
        a = images[i].astype(np.int64)
        if blur:
            p = np.pad(a, ((2, 2), (2, 2), (0, 0)), mode="edge")
            s = np.zeros_like(a)
            for dy in range(5):
                for dx in range(5):
                    s += k[dy] * k[dx] * p[dy:dy + h, dx:dx + w]
            a = (s + 128) >> 8
            assert a.min() >= 0 and a.max() <= 255
        p = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode="edge")
        gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
        gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
        m = gx * gx + gy * gy                                  # [h,w,3]
        ch = m.argmax(-1)[..., None]                           # the first of equal maxima: the lowest channel
        m1 = np.take_along_axis(m, ch, -1)[..., 0]
        b = restate_bin(np.take_along_axis(gx, ch, -1)[..., 0], np.take_along_axis(gy, ch, -1)[..., 0])
        cand = (m1 >= weak * weak) & (m1 > 0)
        for o in range(8):
            votes = np.pad((cand & (b == o)).astype(np.int64), 1)
            count = sum(votes[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
            ori[i] |= np.where(count >= 5, 1 << o, 0).astype(np.uint8)
        mag2[i] = m1
    return ori, mag2


def restate_maps(ori: np.ndarray, T: int) -> np.ndarray:
    """ori uint8 [h,w] -> r_o(x, y) uint8 [8,h,w]"""
    h, w = ori.shape
    p = np.pad(ori, ((0, T - 1), (0, T - 1)))
    s = np.zeros((h, w), np.uint8)
    for dy in range(T):
        for dx in range(T):
            s |= p[dy:dy + h, dx:dx + w]
    r = np.zeros((8, h, w), np.uint8)
    for o in range(8):
        same = (s >> o) & 1
        near = ((s >> ((o + 1) % 8)) | (s >> ((o - 1) % 8))) & 1
        r[o] = np.where(same == 1, 4, np.where(near == 1, 1, 0))
    return r


def restate_response(ori, T: int) -> np.ndarray:
    ori = np.asarray(ori, np.uint8)
    n, h, w = ori.shape
    gh, gw = grid(h, w, T)
    resp = np.zeros((n, 8, T, T, gh, gw), np.uint8)
    for i in range(n):
        r = restate_maps(ori[i], T)
        for py in range(T):
            for px in range(T):
                part = r[:, py::T, px::T]
                resp[i, :, py, px, :part.shape[1], :part.shape[2]] = part
    return resp


def restate_match(ori, T: int, templates, features, n_objects: int):
    """from the orientation bytes [n,h,w] (through r_o(x, y), not the linearised maps) -> best_score, best_f, best_template"""
    ori = np.asarray(ori, np.uint8)
    n, h, w = ori.shape
    gh, gw = grid(h, w, T)
    templates, features = np.asarray(templates, np.int64).reshape(-1, 5), np.asarray(features, np.int64).reshape(-1, 4)
    score, fbest = np.zeros((n, n_objects, gh, gw), np.int64), np.zeros((n, n_objects, gh, gw), np.int64)
    best = np.full((n, n_objects, gh, gw), -1, np.int64)
    for i in range(n):
        r = restate_maps(ori[i], T).astype(np.int64)
        for t, (obj, first, f, width, height) in enumerate(templates):
            if width > w or height > h:
                continue
            ny, nx = (h - height) // T + 1, (w - width) // T + 1                 # the valid locations: gy T + height <= h
            sc = np.zeros((ny, nx), np.int64)
            for dx, dy, o, _ in features[first:first + f]:
                sc += r[o, dy:dy + (ny - 1) * T + 1:T, dx:dx + (nx - 1) * T + 1:T]
            s0, f0, b0 = score[i, obj, :ny, :nx], fbest[i, obj, :ny, :nx], best[i, obj, :ny, :nx]
            wins = (b0 < 0) | (sc * f0 > s0 * f)                                  # sc / (4 f) > s0 / (4 f0), exactly; ties keep the lower index
            s0[wins], f0[wins], b0[wins] = sc[wins], f, t
    return score.astype(np.uint8), fbest.astype(np.uint8), best.astype(np.int32)


# the cases --------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def image_case(n: int, h: int, w: int, seed: int) -> np.ndarray:
    """images uint8 [n,h,w,3]: coloured ellipses and bars over a gradient, some centred on the border, with a little noise (so that
    majorities survive and every bin occurs); the last image of three or more is black; tiny images are random bytes"""
    rng = np.random.RandomState(1000 * seed + 31 * h + w + 7 * n)
    if h * w < 16:
        out = rng.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
        out[0, :, :w // 2] = (10, 20, 30)                 # the first is a vertical step: a 3 x 3 image keeps a bit at its centre
        out[0, :, w // 2:] = (200, 90, 30)
    else:
        ys, xs = np.mgrid[0:h, 0:w]
        out = np.zeros((n, h, w, 3), np.uint8)
        for i in range(n):
            img = np.stack([xs * 255.0 / max(w - 1, 1), ys * 255.0 / max(h - 1, 1), np.full((h, w), 128.0)], -1) * rng.uniform(0.2, 0.6)
            for b in range(8):
                cy, cx = (rng.uniform(0, h), rng.uniform(0, w)) if b % 3 else (rng.choice((0.0, h - 1.0)), rng.uniform(0, w))
                ry, rx = rng.uniform(1.5, 0.3 * h + 2), rng.uniform(1.5, 0.3 * w + 2)
                ang = rng.uniform(0, np.pi)
                u, v = (xs - cx) * np.cos(ang) + (ys - cy) * np.sin(ang), -(xs - cx) * np.sin(ang) + (ys - cy) * np.cos(ang)
                inside = (u / rx) ** 2 + (v / ry) ** 2 <= 1.0 if b % 2 else (np.abs(u) <= rx) & (np.abs(v) <= ry)
                img[inside] = rng.uniform(0, 255, size=3)
            out[i] = np.clip(img + rng.normal(0, 3.0, size=img.shape), 0, 255).astype(np.uint8)
    if n >= 3:
        out[-1] = 0
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def table_case(h: int, w: int, n_templates: int, seed: int, n_objects: int = N_OBJECTS):
    """templates int32 [n_templates,5], features uint8 [n_features,4]: random boxes up to one pixel larger than the image (those have no
    valid location), random features inside them, f from 1 to 63 with both ends present when there is room, first-feature offsets that
    are not multiples of anything (a few unused features sit between templates), objects 0 and 1 only (the last object has none)"""
    rng = np.random.RandomState(77 * seed + 5 * h + 3 * w + n_templates)
    rows, feats = [], []
    for t in range(n_templates):
        f = (1, 63)[t] if t < 2 and n_templates >= 2 else int(rng.randint(1, 64))
        width, height = int(rng.randint(1, min(w + 1, 256) + 1)), int(rng.randint(1, min(h + 1, 256) + 1))
        if t % 7 == 3:
            width, height = min(w, 256), min(h, 256)                    # exactly the image: one valid location
        feats += [(0, 0, 0, 0)] * int(rng.randint(0, 3))               # unused
        rows.append((int(rng.randint(0, max(n_objects - 1, 1))), len(feats), f, width, height))
        feats += [(int(rng.randint(0, width)), int(rng.randint(0, height)), int(rng.randint(0, 8)), 0) for _ in range(f)]
    templates, features = np.asarray(rows, np.int32).reshape(-1, 5), np.asarray(feats, np.uint8).reshape(-1, 4)
    templates.setflags(write=False)
    features.setflags(write=False)
    return templates, features


def cut_template(ori: np.ndarray, x0: int, y0: int, width: int, height: int, max_f: int = 63):
    """the features of a template cut from an orientation map [h,w] at (x0, y0): up to max_f pixels of the box with a bit set ->
    features uint8 [f,4] (dx, dy, index, 0)"""
    ys, xs = np.nonzero(ori[y0:y0 + height, x0:x0 + width])
    keep = np.linspace(0, len(ys) - 1, min(max_f, len(ys))).astype(int) if len(ys) else np.zeros(0, int)
    ys, xs = ys[keep], xs[keep]
    idx = np.log2(ori[y0 + ys, x0 + xs].astype(np.float64)).astype(np.uint8)
    return np.stack([xs.astype(np.uint8), ys.astype(np.uint8), idx, np.zeros(len(ys), np.uint8)], 1).reshape(-1, 4)


def limit_cases():
    """(name, images, T, templates, features, n_objects) of the limits the contract test states: f = 1 and f = 63; a template exactly the
    image's size and one a pixel larger; 1, 2, 65 and 257 templates; objects without a template; n = 3 with one black image"""
    out = []
    for count in TEMPLATE_COUNTS:
        for T in (1, 5):
            templates, features = table_case(13, 17, count, 1)
            out.append((f"{count} templates T={T}", image_case(2, 13, 17, 2), T, templates, features, N_OBJECTS))
    images = image_case(3, 48, 64, 3)
    templates, features = table_case(48, 64, 65, 2)
    out.append(("n=3 with a black image T=8", images, 8, templates, features, N_OBJECTS))
    out.append(("n=3 with a black image T=2", images, 2, templates, features, N_OBJECTS))
    exact = np.asarray([[0, 0, 1, 17, 13], [1, 1, 1, 18, 13], [1, 2, 2, 17, 14]], np.int32)
    feats = np.asarray([[16, 12, 3, 0], [17, 12, 0, 0], [0, 13, 1, 0], [5, 5, 2, 0]], np.uint8)
    for T in (1, 8):
        out.append((f"exactly the image and one pixel larger T={T}", image_case(1, 13, 17, 4), T, exact, feats, 2))
    out.append(("no template at all", image_case(1, 13, 17, 4), 5, np.zeros((0, 5), np.int32), np.zeros((0, 4), np.uint8), 2))
    return out


# the detection scenes of the end-to-end tests (CPU: oracle rasteriser + emulation; GPU: the engine's renderer + kernels) ---------------------
DET_HW = (120, 160)
DET_K = np.asarray([[150.0, 0.0, 80.0], [0.0, 150.0, 60.0], [0.0, 0.0, 1.0]], np.float32)
DET_GRID = 72                                    # rotations of the templates: the 72-rotation SO(3) grid
DET_DISTANCES = (0.45, 0.6)                      # of the templates, metres
DET_QUERY_DISTANCE = 0.525                       # of the planted objects: between the two
# per scene: the background seed and per object (grid rotation the pose is near, pixel offset of the paste: not a multiple of T = 8)
DET_SCENES = ((2, {0: (17, (29, 19)), 1: (63, (-41, -9))}), (3, {0: (33, (-3, -5)), 1: (12, (45, 22))}))


def rotation(axis, degrees: float) -> np.ndarray:
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    k = np.asarray([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)


@lru_cache(maxsize=None)
def det_background(seed: int) -> np.ndarray:
    """uint8 [h,w,3]: low waves, six rectangles of up to +-30 grey levels (their edges are above the weak threshold) and a little noise"""
    h, w = DET_HW
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(6):
            fx, fy = rng.uniform(-0.03, 0.03, 2)
            ph = rng.uniform(0, 6.28)
            img[..., c] += rng.uniform(2, 6) * np.sin(fx * xs * 6.28 + fy * ys * 6.28 + ph)
    for _ in range(6):
        x, y, ww, hh = rng.randint(0, w), rng.randint(0, h), rng.randint(8, 50), rng.randint(8, 50)
        img[y:y + hh, x:x + ww] += rng.uniform(-1, 1, 3) * 30
    img += 110 + rng.normal(0, 2.0, size=img.shape)
    out = np.clip(img, 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def det_query_poses(grid_R: np.ndarray, seed: int, plant) -> Dict[int, np.ndarray]:
    """object -> TCO [4,4] on the optical axis: its grid rotation turned by 5 .. 8 degrees about a random axis, at the query distance"""
    rng = np.random.RandomState(seed)
    poses = {}
    for o, (v, _) in plant.items():
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = rotation(rng.normal(size=3), rng.uniform(5, 8)) @ grid_R[v]
        T[2, 3] = DET_QUERY_DISTANCE
        poses[o] = T
    return poses


def det_compose(seed: int, plant, renders: Dict[int, np.ndarray], masks: Dict[int, np.ndarray]):
    """paste the render uint8 [h,w,3] of every object (silhouette bool [h,w]) at its offset over the background -> the query image
    uint8 [h,w,3] and object -> the box (x1, y1, x2, y2, inclusive) of its pasted silhouette"""
    img = det_background(seed).copy()
    boxes = {}
    for o, (_, (dx, dy)) in plant.items():
        ys, xs = np.nonzero(masks[o])
        img[ys + dy, xs + dx] = renders[o][ys, xs]
        boxes[o] = (int(xs.min()) + dx, int(ys.min()) + dy, int(xs.max()) + dx, int(ys.max()) + dy)
    return img, boxes


def box_iou(a, b) -> float:
    iw = max(min(a[2], b[2]) - max(a[0], b[0]) + 1, 0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]) + 1, 0)
    area = lambda r: (r[2] - r[0] + 1) * (r[3] - r[1] + 1)   # noqa: E731
    return iw * ih / float(area(a) + area(b) - iw * ih)
