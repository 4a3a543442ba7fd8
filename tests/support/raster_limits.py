"""TEST SUPPORT: inputs that take the rasteriser to its limits (list overflow by either cause, record slots beyond 510, the guard band,
the far plane), a Python restatement of the workspace layout raster_bin fills, a reader of what it wrote, and the ctypes wrappers of
tests/raster_emul.cpp these tests use (the emulated render and the host count of raster_bin's lists).

The three layered meshes reach their regime at a 96 x 128 frame, fx = fy = 300, cx = 64, cy = 48, identity rotation, z = 0.5 m, with the
capacities of a database whose LARGEST mesh they are (cap_list = 3 F + 2048 records, cap_large = 4 F + 4096 entries):
  A  6 x 6 quads x 12 layers, 0.2 m   F =  864   the binned records exceed cap_list, no large piece        (fits at z = 1.5 m)
  B  2 x 2 quads x 40 layers, 0.24 m  F =  320   nothing binned, the large-list entries exceed cap_large
  C  40 x 40 quads, 1 layer, 0.03 m   F = 3200   no overflow, the fullest tile holds more than 511 records
tests/test_raster_limits_cpu.py re-checks these statements with margins, so the GPU tests cannot silently leave their code paths."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np

from .emul import CSRC, TESTS, _f32, _i32, _p, build

H, W = 96, 128
K_SMALL = np.array([[300.0, 0, 64], [0, 300.0, 48], [0, 0, 1]], np.float32)
CASE_A = dict(G=6, L=12, size=0.2, dz=0.002, jitter=0.15, seed=1)
CASE_B = dict(G=2, L=40, size=0.24, dz=0.002, jitter=0.15, seed=2)
CASE_C = dict(G=40, L=1, size=0.03, dz=0.002, jitter=0.15, seed=3)
Z_NEAR_VIEW, Z_FAR_VIEW, Z_CLIP_VIEW = 0.5, 1.5, 0.1   # the case's regime | A fits | A crosses the near plane (clipped second pieces)
HDR_INTS, TILE, REC_INTS, SLOT_NONE = 4, 8, 8, 511
GUARD_PX, Z_FAR = 16384.0, 10.0


def layered_grid(G: int, L: int, size: float, dz: float, jitter: float, seed: int) -> Dict[str, np.ndarray]:
    """L layers of G x G quads (2 triangles each) spanning size x size metres around the origin, dz apart along z; every vertex moved in
    x and y by up to +-jitter cells; random unit normals and colours.  F = 2 G^2 L."""
    rs = np.random.RandomState(seed)
    cell = size / G
    g = np.arange(G + 1) * cell - 0.5 * size
    gx, gy = np.meshgrid(g, g)
    verts, faces = [], []
    for layer in range(L):
        xy = np.stack([gx.ravel(), gy.ravel()], 1) + rs.uniform(-jitter, jitter, ((G + 1) ** 2, 2)) * cell
        verts.append(np.concatenate([xy, np.full((len(xy), 1), (layer - 0.5 * (L - 1)) * dz)], 1))
        base = layer * (G + 1) ** 2
        for r in range(G):
            for c in range(G):
                a = base + r * (G + 1) + c
                faces += [[a, a + 1, a + G + 2], [a, a + G + 2, a + G + 1]]
    v = np.concatenate(verts).astype(np.float32)
    n = rs.randn(*v.shape)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return {"vertices": v, "normals": n.astype(np.float32), "colors": rs.rand(len(v), 3).astype(np.float32), "faces": np.asarray(faces, np.int32)}


def pose_z(z: float, x: float = 0.0, y: float = 0.0) -> np.ndarray:
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (x, y, z)
    return T


def tilted(deg: float, z: float) -> np.ndarray:
    """the mesh turned about the camera's x axis by deg, its centre on the optical axis at depth z: the layers cross planes of constant z"""
    a = np.deg2rad(deg)
    T = pose_z(z)
    T[1, 1], T[1, 2], T[2, 1], T[2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return T


# Mesh A cannot overflow while it crosses the near plane: at z = 0.1 m the 96 x 128 frame sees about one of its 33 mm cells, every piece is
# large, and 12 layers x 192 tiles stay far below cap_large (host count: 55 binned, 1735 large entries of 7552).  Mesh B can: tilted by
# 45 degrees at z = 0.15 m it has 400 pieces, 240 of them clipped and 80 second pieces (ids >= F), and 9605 large entries of 5376.
A_CLIP_VIEW = (30.0, 0.1)
B_CLIP_VIEW = (45.0, 0.15)


# Frames whose last tile column and row are cut to 4 pixels (the ragged store).  At 52 x 76 neither A nor B can overflow (the frame sees
# too little of A; B's 40 layers give at most ~4200 large entries of 5376), so that frame gets mesh D: B's shape with 80 layers, F = 640,
# about 8000 large entries of 6656 at z = 0.4 m.  Mesh A keeps its list overflow at 92 x 124.
CASE_D = dict(G=2, L=80, size=0.24, dz=0.001, jitter=0.15, seed=5)


def ragged_configs() -> Dict[str, tuple]:
    """name -> (mesh, h, w, K, z of the overflowed view, z of the view that fits, cause of the overflow)"""
    k = lambda cx, cy: np.array([[300.0, 0, cx], [0, 300.0, cy], [0, 0, 1]], np.float32)   # noqa: E731
    return {"D_52x76": (layered_grid(**CASE_D), 52, 76, k(38, 26), 0.4, 3.0, "large"),
            "A_92x124": (layered_grid(**CASE_A), 92, 124, k(62, 46), Z_NEAR_VIEW, Z_FAR_VIEW, "list")}


def pyramid_mesh()-> Dict[str, np.ndarray]:
    """the 6-triangle pyramid of test_raster_large_triangles_and_close_camera (0.2 m base)"""
    v = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [0, 0, 0.5]], np.float32) * 0.1
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], np.int32)
    nrm = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-6)
    return {"vertices": v, "normals": nrm.astype(np.float32), "colors": np.random.RandomState(0).rand(5, 3).astype(np.float32), "faces": f}


def overflow_scene(with_c: bool = False):
    """Two cameras over the database [A, B, pyramid] (largest mesh: A).  Camera 0: A near (its lists overflow), A far partly behind it
    and partly beside it, the pyramid in front of A near's left part.  Camera 1: B alone (its large list overflows, also at the capacity
    A sets).  The scene emulation sizes the lists per OBJECT mesh, the device by the database's largest: with mesh C appended to the
    database (with_c; no object uses it) nothing overflows on the device, while the emulation still takes its fallback for A near and B.
    -> meshes, obj_off, mesh_ids, TCO [4,4,4], K [2,3,3], radius [2]"""
    meshes = [layered_grid(**CASE_A), layered_grid(**CASE_B), pyramid_mesh()] + ([layered_grid(**CASE_C)] if with_c else [])
    T = np.stack([pose_z(Z_NEAR_VIEW, x=-0.03), pose_z(Z_FAR_VIEW, x=0.27), pose_z(0.4, x=-0.12, y=0.01), pose_z(Z_NEAR_VIEW)])
    return meshes, [0, 3, 4], [0, 0, 2, 1], T, np.repeat(K_SMALL[None], 2, 0), np.array([0.3, 0.2], np.float32)


def merge_meshes(*meshes: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """vertex-coloured meshes as one (faces re-based)"""
    off = np.cumsum([0] + [len(m["vertices"]) for m in meshes[:-1]])
    out = {k: np.ascontiguousarray(np.concatenate([np.asarray(m[k], np.float32) for m in meshes])) for k in ("vertices", "normals", "colors")}
    out["faces"] = np.ascontiguousarray(np.concatenate([np.asarray(m["faces"], np.int32) + o for m, o in zip(meshes, off)]).astype(np.int32))
    return out


def plain_mesh(m: Dict[str, np.ndarray], scale: float = 1.0, shift=(0.0, 0.0, 0.0)) -> Dict[str, np.ndarray]:
    """the vertex-coloured part of a loaded mesh (no texture), scaled and moved"""
    v = np.asarray(m["vertices"], np.float32) * np.float32(scale) + np.asarray(shift, np.float32)
    return {"vertices": np.ascontiguousarray(v, np.float32), "normals": np.ascontiguousarray(m["normals"], np.float32),
            "colors": np.ascontiguousarray(m["colors"], np.float32), "faces": np.ascontiguousarray(m["faces"], np.int32)}


def table_mesh(seed: int = 4) -> Dict[str, np.ndarray]:
    """a 4 m x 4 m table top in the plane z = 0, 4 x 4 quads of 1 m (32 triangles)"""
    return layered_grid(4, 1, 4.0, 0.0, 0.0, seed)


def standing_on_table(m: Dict[str, np.ndarray], at=(0.64, 0.0)) -> Dict[str, np.ndarray]:
    """the loaded mesh with its lowest point on the table top, at table position `at`"""
    v = np.asarray(m["vertices"], np.float32)
    c = 0.5 * (v.min(0) + v.max(0))
    return plain_mesh(m, 1.0, (at[0] - c[0], at[1] - c[1], -v[:, 2].min()))


K_TABLE = np.array([[1200.0, 0, 64], [0, 1200.0, 48], [0, 0, 1]], np.float32)


def table_pose(pitch_deg: float = 10.0, eye=(-1.06, 0.0, 0.3)) -> np.ndarray:
    """TCO of a camera 0.3 m above the table top (object frame: z up), looking along +x, pitched down by pitch_deg: the row of table
    vertices at x = -1 lies 6 cm in front of it (just beyond the near plane, 2 m to either side: beyond the guard band under K_TABLE),
    the row at x = -2 behind it (triangles cross the near plane), the far edge 3 m away."""
    p = np.deg2rad(pitch_deg)
    R = np.array([[0.0, -1.0, 0.0], [-np.sin(p), 0.0, -np.cos(p)], [np.cos(p), 0.0, -np.sin(p)]])   # rows: right, down, forward
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ np.asarray(eye, np.float64)
    return T.astype(np.float32)


def centred(m: Dict[str, np.ndarray], scale: float) -> Dict[str, np.ndarray]:
    v = np.asarray(m["vertices"], np.float32)
    c = 0.5 * (v.min(0) + v.max(0))
    return plain_mesh(m, scale, -c * np.float32(scale))


FAR_ZS = (9.0, 10.0, 10.5, 11.0)


def far_plane_views(lathe: Dict[str, np.ndarray], zs=FAR_ZS):
    """the lathe mesh scaled x20 (2.8 m tall), its axis upright in the picture, centred at depth z: from z = 10.5 m on, the part of its
    front surface near the silhouette lies beyond Z_FAR = 10 m.  -> mesh, TCO, K"""
    T = np.stack([tilted(90.0, z) for z in zs])
    return centred(lathe, 20.0), T, np.repeat(K_SMALL[None], len(zs), 0)


def half_scale(mesh: Dict[str, np.ndarray], T: np.ndarray):
    """the same picture at half the distance (mesh and translations x 0.5): every depth halves, so nothing leaves the depth range"""
    Th = np.array(T, np.float32)
    Th[:, :3, 3] *= np.float32(0.5)
    return plain_mesh(mesh, 0.5), Th


def table_view(lathe: Dict[str, np.ndarray]):
    """the table top with the lathe mesh standing on it, as ONE mesh, from the grazing camera.  -> mesh, TCO [1,4,4], K [1,3,3]"""
    return merge_meshes(table_mesh(), standing_on_table(lathe)), table_pose()[None], K_TABLE[None]


def single_views(lathe_meshes) -> Dict[str, tuple]:
    """name -> (mesh, TCO [n,4,4], K [n,3,3]) of every single-object view of these tests at the H x W frame"""
    k = lambda n: np.repeat(K_SMALL[None], n, 0)   # noqa: E731
    A, B, Cm = layered_grid(**CASE_A), layered_grid(**CASE_B), layered_grid(**CASE_C)
    return {
        "A_near": (A, pose_z(Z_NEAR_VIEW)[None], k(1)),
        "A_far": (A, pose_z(Z_FAR_VIEW)[None], k(1)),
        "A_clip": (A, tilted(*A_CLIP_VIEW)[None], k(1)),
        "B": (B, pose_z(Z_NEAR_VIEW)[None], k(1)),
        "B_clip": (B, tilted(*B_CLIP_VIEW)[None], k(1)),
        "C": (Cm, pose_z(Z_NEAR_VIEW)[None], k(1)),
        "table": table_view(lathe_meshes[0]),
        "far_plane": far_plane_views(lathe_meshes[1]),
    }


# ---- the workspace of raster_bin -------------------------------------------------------------------------------------------------
def bin_layout(max_faces: int, h: int, w: int) -> Dict[str, int]:
    """raster_bin_layout (megapose6d_amd/csrc/raster_db.hip) restated; offsets in ints from the start of a view's block"""
    tiles_x, tiles_y = -(-w // TILE), -(-h // TILE)
    n_tiles = tiles_x * tiles_y
    cap_list, cap_large = 3 * max_faces + 2048, 4 * max_faces + 4096
    off_tl = (HDR_INTS + n_tiles + 1 + 3) & ~3
    off_large = (off_tl + n_tiles + 1 + 3) & ~3
    off_list = (off_large + cap_large + 3) & ~3
    return dict(tiles_x=tiles_x, tiles_y=tiles_y, n_tiles=n_tiles, cap_list=cap_list, cap_large=cap_large, off_tl=off_tl, off_large=off_large,
                off_list=off_list, view_ints=off_list + cap_list * REC_INTS)


def workspace_bytes(lay: Dict[str, int], n_views: int) -> int:
    """mp_raster_workspace_bytes restated: the view blocks, then 4 counters, the light-job list (one int per (view, tile)), the job flags
    and the per-view tile flags (one byte per (view, tile) each, padded to 16)"""
    pairs = n_views * lay["n_tiles"]
    tail = (n_views * lay["view_ints"] + 3) & ~3
    return (tail + 4 + pairs) * 4 + 2 * ((pairs + 15) & ~15)


def db_max_faces(db, h: int, w: int) -> int:
    """the face count of the database's largest mesh, from the size of a one-view workspace (the layout is linear in it: 4 F + 4096
    large-list ints + 8 ints for each of the 3 F + 2048 records)"""
    from megapose6d_amd import _lib

    lay0 = bin_layout(0, h, w)
    extra = int(_lib.load().mp_raster_workspace_bytes(db.handle, 1, h, w)) - workspace_bytes(lay0, 1)
    assert extra >= 0 and extra % (4 * 28) == 0, extra
    return extra // (4 * 28)


def launch_device():
    """the device of a launch's output tensor, as MeshDB.workspace compares it (an index-less "cuda" would make it allocate a new one)"""
    import torch

    return torch.device("cuda", torch.cuda.current_device())


def view_headers(db, n_views: int, h: int, w: int) -> Dict[str, np.ndarray]:
    """What raster_bin wrote for the n_views views of the LAST launch on this database's workspace (valid until the next launch on that
    slot): hdr [n_views, 4] = (large entries, binned entries, overflow, orientation hint), tile_off / tile_off_l [n_views, n_tiles + 1]."""
    import torch

    lay = bin_layout(db_max_faces(db, h, w), h, w)
    held = db._ws.get(0)
    ws = db.workspace(n_views, h, w, launch_device())
    assert held is not None and ws.data_ptr() == held.data_ptr(), "not the workspace of the last launch"
    torch.cuda.synchronize()
    ints = ws[: n_views * lay["view_ints"] * 4].view(torch.int32).reshape(n_views, lay["view_ints"])
    n = lay["n_tiles"] + 1
    return dict(hdr=ints[:, :HDR_INTS].cpu().numpy(), tile_off=ints[:, HDR_INTS:HDR_INTS + n].cpu().numpy(),
                tile_off_l=ints[:, lay["off_tl"]:lay["off_tl"] + n].cpu().numpy(), layout=lay)


# ---- tests/raster_emul.cpp -----------------------------------------------------------------------------------------------------------
def emul_lib():
    lib = build("raster_emul", [TESTS / "raster_emul.cpp", CSRC / "raster_core.h"])
    lib.raster_emul_render.restype = None
    lib.raster_emul_bin_counts.restype = None
    return lib


def bin_counts(mesh: Dict[str, np.ndarray], T: np.ndarray, K: np.ndarray, h: int, w: int, ns: int) -> Dict[str, np.ndarray]:
    """raster_emul_bin_counts: per view the binned records per tile, the large-list entries per tile and
    stats = (pieces, pieces with a coordinate beyond 2^21 sub-pixel units, unclipped triangles dropped by GUARD, clipped pieces)"""
    v, f = _f32(mesh["vertices"]), _i32(mesh["faces"])
    T = _f32(np.asarray(T).reshape(-1, 16))
    K = _f32(np.asarray(K).reshape(-1, 9))
    assert T.shape[0] == K.shape[0]
    n_views, n_tiles = T.shape[0], (-(-h // TILE)) * (-(-w // TILE))
    binned = np.full((n_views, n_tiles), -1, np.int32)
    large = np.full((n_views, n_tiles), -1, np.int32)
    stats = np.full((n_views, 4), -1, np.int32)
    emul_lib().raster_emul_bin_counts(_p(v), _p(f), C.c_int(v.shape[0]), C.c_int(f.shape[0]), _p(T), _p(K), C.c_int(n_views), C.c_int(h), C.c_int(w),
                                      C.c_int(ns), _p(binned), _p(large), _p(stats))
    return dict(binned=binned, large=large, stats=stats, n_binned=binned.sum(1), n_large=large.sum(1), n_pieces=stats[:, 0])


def expected_headers(counts: Dict[str, np.ndarray], lay: Dict[str, int]):
    """-> (hdr[:, :3] as raster_bin must write it, tile_off, tile_off_l) from the host count"""
    overflow = (counts["n_binned"] > lay["cap_list"]) | (counts["n_large"] > lay["cap_large"])
    hdr = np.stack([counts["n_large"], counts["n_binned"], overflow.astype(np.int64)], 1).astype(np.int32)
    z = np.zeros((len(hdr), 1), np.int64)
    off = np.concatenate([z, np.cumsum(counts["binned"], 1)], 1).astype(np.int32)
    off_l = np.concatenate([z, np.cumsum(counts["large"], 1)], 1).astype(np.int32)
    return hdr, off, off_l


def emul_render(mesh: Dict[str, np.ndarray], T: np.ndarray, K: np.ndarray, h: int, w: int, flags: int, lights=None, cap_list: int = 0,
                reverse: int = 0):
    """raster_emul_render of a vertex-coloured mesh -> rgb [n,h,w,3], normals [n,h,w,3], depth [n,h,w]; cap_list = 0: the device's rule
    (3 F + 2048) for this mesh"""
    from oracle import raster as orr

    v, n, c, f = _f32(mesh["vertices"]), _f32(mesh["normals"]), _f32(mesh["colors"]), _i32(mesh["faces"])
    T = _f32(np.asarray(T).reshape(-1, 16))
    K = _f32(np.asarray(K).reshape(-1, 9))
    nv = T.shape[0]
    out = np.full((nv, h, w, 8), -7.0, np.float32)
    L = lights if lights is not None else orr.lights_struct()
    LL = C.c_longlong
    emul_lib().raster_emul_render(_p(v), _p(n), _p(c), _p(f), C.c_int(v.shape[0]), C.c_int(f.shape[0]), C.c_float(orr.mesh_radius(v)), None, None,
                                  C.c_int(0), C.c_int(0), C.c_int(0), _p(T), _p(K), C.c_int(nv), C.c_int(h), C.c_int(w), C.c_uint32(flags),
                                  C.byref(L), _p(out), LL(h * w * 8), C.c_int(1), LL(0), LL(w * 8), LL(8), C.c_int(0), C.c_int(3), C.c_int(6),
                                  C.c_int(cap_list), C.c_int(reverse))
    assert (out[..., 7] == -7.0).all()
    return out[..., 0:3], out[..., 3:6], out[..., 6]
