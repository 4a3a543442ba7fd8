"""TEST SUPPORT: ctypes wrapper of the host emulation of the scene rasteriser (tests/raster_scene_emul.cpp), built on first use."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence

import numpy as np

from .emul import CSRC, TESTS, build


def load():
    lib = build("raster_scene_emul", [TESTS / "raster_scene_emul.cpp", TESTS / "raster_emul.cpp", CSRC / "raster_core.h",
                                      CSRC / "raster_scene_core.h"])
    lib.raster_scene_emul_render.restype = None
    return lib


def render(meshes: Sequence[Dict[str, np.ndarray]], obj_off: Sequence[int], mesh_ids: Sequence[int], TCO: np.ndarray, K: np.ndarray,
           radius: Sequence[float], rigs: Sequence, h: int, w: int, flags: int, cap_list: int = 0, reverse: int = 0):
    """rigs: one light struct per object (megapose6d_amd._lib.Lights or oracle.raster._Lights: the same layout).
    -> rgb [n_cams,h,w,3], normals [n_cams,h,w,3], depth [n_cams,h,w], instance ids [n_cams,h,w] (channels not asked for stay 0)"""
    lib = load()
    nm = len(meshes)
    keep: List[np.ndarray] = []

    def arr(key, dtype):
        out = (C.c_void_p * nm)()
        for i, m in enumerate(meshes):
            a = np.ascontiguousarray(m[key], dtype)
            keep.append(a)
            out[i] = a.ctypes.data
        return out

    uvs, tex = (C.c_void_p * nm)(), (C.c_void_p * nm)()
    tw, th, tl = (C.c_int * nm)(), (C.c_int * nm)(), (C.c_int * nm)()
    for i, m in enumerate(meshes):
        if m.get("uvs") is not None and m.get("texture_mips") is not None:
            uv = np.ascontiguousarray(m["uvs"], np.float32)
            mips = m["texture_mips"]
            flat = np.ascontiguousarray(np.concatenate([lv.reshape(-1) for lv in mips]).astype(np.uint32))
            keep += [uv, flat]
            uvs[i], tex[i] = uv.ctypes.data, flat.ctypes.data
            th[i], tw[i] = mips[0].shape[:2]
            tl[i] = len(mips)
    nv = (C.c_int * nm)(*[int(np.asarray(m["vertices"]).shape[0]) for m in meshes])
    nf = (C.c_int * nm)(*[int(np.asarray(m["faces"]).shape[0]) for m in meshes])
    n_cams = len(obj_off) - 1
    off = np.ascontiguousarray(obj_off, np.int32)
    ids = np.ascontiguousarray(mesh_ids, np.int32).reshape(-1)
    T = np.ascontiguousarray(TCO, np.float32).reshape(-1, 16)
    Kc = np.ascontiguousarray(K, np.float32).reshape(-1, 9)
    rad = np.ascontiguousarray(radius, np.float32)
    L = (type(rigs[0]) * len(rigs))(*rigs) if len(rigs) else None
    out = np.zeros((n_cams, h, w, 8), np.float32)
    inst = np.full((n_cams, h, w), -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    LL = C.c_longlong
    lib.raster_scene_emul_render(C.c_int(nm), arr("vertices", np.float32), arr("normals", np.float32), arr("colors", np.float32),
                                 arr("faces", np.int32), nv, nf, uvs, tex, tw, th, tl, C.c_int(n_cams), p(off), p(ids), p(T), p(Kc), p(rad),
                                 L, C.c_int(h), C.c_int(w), C.c_uint32(flags), p(out), LL(h * w * 8), LL(w * 8), LL(8), C.c_int(0), C.c_int(3),
                                 C.c_int(6), p(inst), C.c_int(cap_list), C.c_int(reverse))
    return out[..., 0:3], out[..., 3:6], out[..., 6], inst
