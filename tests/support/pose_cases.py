"""Seeded case generators for the pose / camera-geometry kernel tests.  TEST INFRASTRUCTURE ONLY.

Everything returned is fp32 (ids int32) and depends only on the arguments: the CPU tier (tests/test_pose_ref_cpu.py) and the GPU tier
(tests/test_gpu_pose_kernels.py) build the same cases.  Ill-conditioned rows are kept out by construction, never masked; the CPU tier
asserts the conditions on the float64 reference.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np

from tests.support import pose_ref as pr
from tests.support.synthetic import K_EXAMPLE

N_MESH = 5
MESH_RADIUS = 0.08            # metres: the largest distance of a used point from the mesh origin
DATA_DIR = Path(__file__).resolve().parents[2] / "megapose6d_amd" / "data"
MV_REMOVE_TCO, MV_INPLANE = 256, 512     # include/mp_engine.h


def _rng(*key) -> np.random.RandomState:
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def random_rotations(rng, n: int) -> np.ndarray:
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


# --------------------------------------------------------------------------- #
def make_points(n_used: int, stride: int, seed: int = 0) -> np.ndarray:
    """[N_MESH, stride, 3]: each mesh an ellipsoid-like cloud of its own shape inside MESH_RADIUS.  Mesh 0 has its farthest point at
    index 0, mesh 1 at index n_used - 1 (a loop that skips either end changes every extent).  Past the first n_used points the buffer
    holds points three times as far out: reading them, or addressing a mesh by the wrong stride, changes every box."""
    rng = _rng("points", n_used, stride, seed)
    out = np.empty((N_MESH, stride, 3))
    for m in range(N_MESH):
        d = rng.normal(size=(stride, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        axes = rng.uniform(0.35, 0.8, size=3)
        p = d * axes * rng.uniform(0.6, 1.0, size=(stride, 1)) * MESH_RADIUS
        if m < 2 and n_used > 1:
            e = rng.normal(size=3)
            p[0 if m == 0 else n_used - 1] = e / np.linalg.norm(e) * MESH_RADIUS
        p[n_used:] = d[n_used:] * 3 * MESH_RADIUS
        out[m] = p
    return out.astype(np.float32)


def make_mesh_ids(b: int, seed: int = 0) -> np.ndarray:
    """non-monotonic, every mesh used once the batch is large enough"""
    ids = (np.arange(b) * 3 + 2) % N_MESH
    return _rng("ids", b, seed).permutation(ids).astype(np.int32)


def make_K(b: int, im_hw, seed: int = 0) -> np.ndarray:
    """per-row fx != fy in 300..1200, principal point off centre, non-zero K[0,1] and K[1,0]; one row is K_EXAMPLE"""
    rng = _rng("K", b, tuple(im_hw), seed)
    h, w = im_hw
    K = np.zeros((b, 3, 3))
    K[:, 0, 0] = rng.uniform(300, 1200, b)
    K[:, 1, 1] = rng.uniform(300, 1200, b)
    K[:, 0, 2] = w / 2 + rng.uniform(-0.2, 0.2, b) * w
    K[:, 1, 2] = h / 2 + rng.uniform(-0.2, 0.2, b) * h
    K[:, 0, 1] = rng.uniform(0.5, 2.0, b) * rng.choice([-1, 1], b)
    K[:, 1, 0] = rng.uniform(0.25, 1.0, b) * rng.choice([-1, 1], b)
    K[:, 2, 2] = 1.0
    K[min(3, b - 1)] = K_EXAMPLE
    return K.astype(np.float32)


POSE_KINDS = ("mid", "mid_offaxis", "close", "far", "offscreen")


def make_poses(kind: str, b: int, K: np.ndarray, im_hw, seed: int = 0, orthonormal: bool = False) -> np.ndarray:
    """TCO_in [b, 4, 4].
    mid         object 0.35..0.7 m away, within 15 % of the optical axis: nothing is clamped
    mid_offaxis the same, 15..30 % above or below the axis: what the sphere views need (the camera straight above the object looks
                along the up vector when the object is at the height of the optical axis; |y x up| of that look-at is |t_y| / |t|)
    close       rows in turn: some points behind z = 0.1, the object centre behind it with points in front, everything behind the camera
    far         far away; PrepareCase.inputs then moves each row along its ray until the crop is 13..27 px wide
    offscreen   the centre projects more than a frame outside the image
    Unless `orthonormal`, the rotation block is not orthonormal (1 % noise), and in two rows of four its first two columns are scaled by
    1e-3 and 1e3 (normalize_T is scale-free)."""
    rng = _rng("poses", kind, b, seed)
    R = random_rotations(rng, b)
    K = K.astype(np.float64)
    fx, fy = K[:, 0, 0], K[:, 1, 1]
    ang = rng.uniform(0, 2 * np.pi, b)
    if kind in ("mid", "mid_offaxis"):
        z = rng.uniform(0.35, 0.7, b)
        if kind == "mid":
            rad = rng.uniform(0.0, 0.15, b)
            t = np.stack([rad * np.cos(ang) * z, rad * np.sin(ang) * z, z], axis=1)
        else:
            t = np.stack([rng.uniform(-0.2, 0.2, b) * z, rng.uniform(0.15, 0.3, b) * rng.choice([-1, 1], b) * z, z], axis=1)
    elif kind == "close":
        i = np.arange(b) % 3
        z = np.where(i == 0, rng.uniform(0.105, 0.12, b), np.where(i == 1, rng.uniform(0.088, 0.098, b), rng.uniform(-0.4, -0.15, b)))
        t = np.stack([rng.uniform(-0.02, 0.02, b), rng.uniform(-0.02, 0.02, b), z], axis=1)
    elif kind == "far":
        z = 2 * 1.4 * np.minimum(fx, fy) * MESH_RADIUS / rng.uniform(17, 22, b)
        t = np.stack([rng.uniform(-0.1, 0.1, b) * z, rng.uniform(-0.1, 0.1, b) * z, z], axis=1)
    elif kind == "offscreen":
        z = rng.uniform(0.5, 0.9, b)
        horizontal = rng.uniform(size=b) < 0.5
        frames = rng.uniform(1.2, 1.6, b) * rng.choice([-1, 1], b)
        dx = np.where(horizontal, frames * im_hw[1] / fx, rng.uniform(-0.1, 0.1, b))
        dy = np.where(horizontal, rng.uniform(-0.1, 0.1, b), frames * im_hw[0] / fy)
        t = np.stack([dx * z, dy * z, z], axis=1)
    else:
        raise ValueError(kind)
    T = np.tile(np.eye(4), (b, 1, 1))
    T[:, :3, :3] = R
    T[:, :3, 3] = t
    if not orthonormal:
        T[:, :3, :3] += 0.01 * rng.normal(size=(b, 3, 3))
        T[1::4, :3, 0] *= 1e-3
        T[1::4, :3, 1] *= 1e3
        T[2::4, :3, 0] *= 1e3
        T[2::4, :3, 1] *= 1e-3
    return T.astype(np.float32)


# --------------------------------------------------------------------------- #
@dataclass(frozen=True)
class PrepareCase:
    """one call of engine.pose_prepare; `family` is the group its bound k belongs to (the pose kind sets the conditioning)"""
    name: str
    pose: str = "mid"
    b: int = 16
    mode: int = 1
    remove: bool = False
    inplane: bool = False
    n_main: int = 2000
    n_views: int = 200
    stride: int = 2000
    im_hw: Tuple[int, int] = (480, 640)
    out_hw: Tuple[int, int] = (240, 320)
    lamb: float = 1.4
    seed: int = 0

    @property
    def family(self) -> str:
        return self.pose

    @property
    def code(self) -> int:
        return self.mode | (MV_REMOVE_TCO if self.remove else 0) | (MV_INPLANE if self.inplane else 0)

    @property
    def V(self) -> int:
        return pr.n_views(self.mode, self.remove, self.inplane)

    def inputs(self) -> Dict[str, np.ndarray]:
        K = make_K(self.b, self.im_hw, self.seed)
        inp = dict(TCO_in=make_poses(self.pose, self.b, K, self.im_hw, self.seed), K=K, mesh_ids=make_mesh_ids(self.b, self.seed),
                   points=make_points(max(self.n_main, self.n_views), self.stride, self.seed))
        if self.pose == "far":      # the crop width goes as 1 / distance: scale each translation to a width drawn from 13..27 px
            bc = pr.pose_prepare_detail(inp["TCO_in"], K, inp["mesh_ids"], inp["points"], self.n_main, self.n_views, 0, False, False,
                                        self.im_hw, self.out_hw, self.lamb)["boxes_crop"]
            target = _rng("far", self.b, self.seed).uniform(13, 27, self.b)
            inp["TCO_in"][:, :3, 3] *= ((bc[:, 2] - bc[:, 0]) / target)[:, None].astype(np.float32)
        return inp

    def reference(self, inp=None) -> Dict[str, np.ndarray]:
        inp = inp or self.inputs()
        return pr.pose_prepare_detail(inp["TCO_in"], inp["K"], inp["mesh_ids"], inp["points"], self.n_main, self.n_views, self.mode,
                                      self.remove, self.inplane, self.im_hw, self.out_hw, self.lamb)


def _prepare_cases() -> List[PrepareCase]:
    C = PrepareCase
    cases = []
    # views: every accepted code; the sphere modes take the off-axis poses
    for mode in (0, 1, 2, 3):
        for remove, inplane in ((False, False), (True, False), (True, True)):
            if mode == 0 and inplane:
                continue
            cases.append(C(f"views-m{mode}{'-rm' if remove else ''}{'-inplane' if inplane else ''}", pose="mid_offaxis" if mode == 3 else "mid",
                           b=12, mode=mode, remove=remove, inplane=inplane, seed=mode))
    # poses x (TCO kept, TCO removed)
    for pose in ("close", "far", "offscreen"):
        cases.append(C(f"pose-{pose}", pose=pose, b=129, mode=1))
        cases.append(C(f"pose-{pose}-rm", pose=pose, b=48, mode=1, remove=True, seed=1))
    # batch sizes: the pipeline's row counts
    cases += [C("batch-1", b=1, mode=1), C("batch-129", b=129, mode=2), C("batch-576-sphere", pose="mid_offaxis", b=576, mode=3, remove=True, inplane=True),
              C("batch-4608", b=4608, mode=1)]
    # point counts around a wave and a block, in a buffer wider than the used prefix
    for n_main in (1, 63, 64, 65, 255, 256, 257, 2000):
        n_views = {1: 1, 63: 1, 64: 64, 65: 64, 255: 200, 256: 200, 257: 64, 2000: 200}[n_main]
        cases.append(C(f"points-{n_main}-{n_views}", b=10, mode=1, remove=n_main % 2 == 1, n_main=n_main, n_views=min(n_views, n_main), stride=2048, seed=n_main))
    # image / output shapes and lamb (a readable cross, not the product)
    shapes = [((640, 480), (240, 320), 1.4), ((512, 512), (224, 224), 1.4), ((480, 640), (320, 240), 2.0), ((640, 480), (320, 240), 1.0),
              ((480, 640), (224, 224), 1.0), ((512, 512), (240, 320), 2.0)]
    for i, (im, out, lamb) in enumerate(shapes):
        cases.append(C(f"shape-{im[0]}x{im[1]}-{out[0]}x{out[1]}-l{lamb}", b=10, mode=1, remove=i % 2 == 1, im_hw=im, out_hw=out, lamb=lamb, seed=i))
    cases.append(C("shape-far-portrait", pose="far", b=32, mode=1, im_hw=(640, 480), out_hw=(320, 240)))
    return cases


PREPARE_CASES = _prepare_cases()
BATCHES = (1, 127, 128, 129, 576, 4608)


# --------------------------------------------------------------------------- #
def normalize_T_inputs(b: int, seed: int = 0) -> np.ndarray:
    """every pose kind in one batch, non-orthonormal and scaled rotation blocks included"""
    K = make_K(b, (480, 640), seed)
    T = np.concatenate([make_poses(kind, b, K, (480, 640), seed)[i::len(POSE_KINDS)] for i, kind in enumerate(POSE_KINDS)])
    return T[_rng("nT", b, seed).permutation(b)]


def update_inputs(b: int, seed: int = 0, V: int = 1) -> Dict[str, np.ndarray]:
    """network output with 6D vectors of unequal length (0.3..3) and up to 60 degrees from orthogonal, pixel offsets up to 30 px, vz in
    0.5..2, K_crop per row inside a [b, V, 3, 3] tensor whose other views hold other intrinsics; tCR is TCO's translation in half of the
    rows and 2 cm off it in the others."""
    rng = _rng("update", b, seed)
    K0 = make_K(b, (480, 640), seed)
    TCO = make_poses("mid", b, K0, (480, 640), seed, orthonormal=True)
    tCR = TCO[:, :3, 3].astype(np.float64)
    tCR = tCR + np.where(np.arange(b)[:, None] % 2 == 1, rng.uniform(-0.02, 0.02, (b, 3)), 0.0)
    R = random_rotations(rng, b)
    a = R[:, :, 0]
    dev = np.deg2rad(rng.uniform(-60, 60, b))[:, None]
    c = np.cos(dev) * R[:, :, 1] + np.sin(dev) * a          # 90 deg - dev from a
    out9 = np.concatenate([a * rng.uniform(0.3, 3.0, (b, 1)), c * rng.uniform(0.3, 3.0, (b, 1)), rng.uniform(-30, 30, (b, 2)), rng.uniform(0.5, 2.0, (b, 1))], axis=1)
    KV = np.zeros((b, V, 3, 3))
    KV[..., 0, 0] = rng.uniform(500, 3000, (b, V))
    KV[..., 1, 1] = rng.uniform(500, 3000, (b, V))
    KV[..., 0, 2] = rng.uniform(100, 220, (b, V))
    KV[..., 1, 2] = rng.uniform(80, 160, (b, V))
    KV[..., 0, 1] = rng.uniform(0.5, 2.0, (b, V))
    KV[..., 2, 2] = 1.0
    return dict(TCO=TCO, KV_crop=KV.astype(np.float32), out9=out9.astype(np.float32), tCR=tCR.astype(np.float32))


def so3_grid(n: int) -> np.ndarray:
    """rotations [n, 3, 3] (fp32) of a shipped SO(3) grid of unit quaternions (file order x y z w)"""
    q = np.load(DATA_DIR / f"so3_grid_{n}_xyzw.npy").astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    return R.astype(np.float32)


EXTENT_CASES = [(72, 1), (72, 63), (72, 255), (512, 64), (576, 257), (576, 2000), (4608, 256), (4608, 65)]   # (grid, points per mesh)


def init_inputs(b: int, grid: int, n_pts: int = 2000, seed: int = 0) -> Dict[str, np.ndarray]:
    """detection boxes in turn inside the frame, partly outside it and one pixel wide (x2 == x1), per-row K, rotations drawn from a
    shipped grid"""
    rng = _rng("init", b, grid, n_pts, seed)
    K = make_K(b, (480, 640), seed)
    u0, v0 = rng.uniform(60, 500, b), rng.uniform(60, 360, b)
    w, h = rng.uniform(20, 200, b), rng.uniform(20, 200, b)
    i = np.arange(b) % 3
    u0 = np.where(i == 1, rng.uniform(-150, -5, b), u0)
    v0 = np.where(i == 1, rng.uniform(465, 475, b), v0)
    w = np.where(i == 2, 0.0, w)
    boxes = np.stack([u0, v0, u0 + w, v0 + h], axis=1).astype(np.float32)
    return dict(boxes=boxes, K=K, mesh_ids=make_mesh_ids(b, seed), rot_ids=rng.randint(0, grid, b).astype(np.int32), R=so3_grid(grid),
                points=make_points(n_pts, n_pts, seed))


# Bounds of the GPU tier: |got - ref64| <= k * 2^-24 * S (S: tests/support/pose_ref.py).  Not tuned: every k is pose_ref.k_from_floor of the
# fp32 oracle's own worst error on the family's cases (4 x floor, next power of two, at least 8), which
# tests/test_pose_ref_cpu.py::test_bounds_follow_from_the_oracle_floor measures and compares with this table; the floors are in the
# docstring of tests/test_gpu_pose_kernels.py.  Families of pose_prepare are the pose kinds.
_K = lambda *v: dict(zip(pr.PREPARE_CHECKS, v))   # noqa: E731
#                        TCO_n tCR TCV_O KV_crop b_rend b_crop K_main K_main.focal K_main.pp KV_crop.focal KV_crop.pp
K_BOUND = {
    "mid":         _K(16, 8, 64, 4096, 16, 32, 4096, 64, 32, 64, 128),
    "mid_offaxis": _K(16, 8, 32, 512, 16, 32, 2048, 32, 32, 64, 128),
    "close":       _K(8, 8, 32, 64, 16, 16, 32, 32, 32, 64, 64),
    "far":         _K(8, 8, 32, 512, 16, 32, 512, 64, 64, 64, 128),
    "offscreen":   _K(16, 8, 32, 128, 16, 32, 1024, 32, 32, 32, 128),
    "update": {"TCO_out": 16},
    "init": {"TCO_init": 128, "extents": 32},
    "normalize": {"T": 16},
}
