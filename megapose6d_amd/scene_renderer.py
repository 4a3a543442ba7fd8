"""Panda3dSceneRenderer: drop-in for the reference's multi-object scene renderer, backed by the on-device HIP scene rasteriser
(mp_raster_render_scene, csrc/raster_scene.hip).

Same constructor and `render_scene(...)` signature as
the reference's src/megapose/panda3d_renderer/panda3d_scene_renderer.py:139-358: several objects per camera image, depth-tested
against each other, RGB / normals / depth / binary mask per camera as host arrays.  `render_scenes` is the tensor-level form (device
tensors in and out, plus a per-pixel instance map) that `render_scene` wraps.

Host rules (float64, rounded to float32 once):
  - TCO = inv(TWC) . TWO per (camera, object).
  - Scene radius: every object contributes its mesh bounding sphere (object-frame AABB centre, radius mp_mesh_db_radius) moved by TWO;
    the scene sphere is the fold, in list order, of "the smallest sphere enclosing both".  One object: the mesh radius, bit for bit.
  - Light rig: a point light sits at p_world = a * radius + b (resolve_light_position of its positioning_function); per object it is
    passed in the object's frame as dir = R_WO^T a / 10, offset = R_WO^T (b - t_WO), the engine's position dir * 10 * radius + offset.
Known deviation: the reference sets `binary_mask` only on the last rendering (a loop variable leaks, :329-335); here every camera gets
its own mask.
"""
from __future__ import annotations

import time
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np
import torch

from . import engine as eng
from . import mesh_io
from .renderer import _point_light
from .types import (CameraRenderingData, Panda3dCameraData, Panda3dLightData, Panda3dObjectData, Resolution,  # noqa: F401
                    pose_matrix)

MAX_POINT_LIGHTS = 8
MAX_OBJECTS_PER_CAMERA = 256


@dataclass
class Panda3dDebugData:
    timings: Dict[str, float] = field(default_factory=dict)


@dataclass
class SceneRenderOutput:
    """rgbs [n,3,h,w], normals [n,3,h,w] | None, depths [n,1,h,w] | None (device tensors, values as BatchRenderOutput);
    instance_ids [n,h,w] int32 | None: index, among the scene's rows in input order, of the object that owns sample 0; -1 = background."""
    rgbs: torch.Tensor
    normals: Optional[torch.Tensor]
    depths: Optional[torch.Tensor]
    instance_ids: Optional[torch.Tensor]


# --------------------------------------------------------------------------- host rules
def aabb_centre(vertices: np.ndarray) -> np.ndarray:
    """object-frame AABB centre of a mesh, in float32 exactly as the mesh database computes it for the bounding radius"""
    v = np.asarray(vertices, np.float32)
    return (np.float32(0.5) * (v.min(0) + v.max(0))).astype(np.float32)


def enclose_spheres(c1, r1: float, c2, r2: float) -> Tuple[np.ndarray, float]:
    """the smallest sphere enclosing the spheres (c1, r1) and (c2, r2), float64"""
    c1, c2 = np.asarray(c1, np.float64), np.asarray(c2, np.float64)
    d = float(np.linalg.norm(c2 - c1))
    if d + r2 <= r1:
        return c1, float(r1)
    if d + r1 <= r2:
        return c2, float(r2)
    r = 0.5 * (d + r1 + r2)
    return c1 + (c2 - c1) * ((r - r1) / d), r


def scene_sphere(centres: Sequence[np.ndarray], radii: Sequence[float]) -> Tuple[np.ndarray, float]:
    """fold of enclose_spheres over the (world-frame) object spheres, in list order; no sphere -> radius 0"""
    if len(radii) == 0:
        return np.zeros(3), 0.0
    c, r = np.asarray(centres[0], np.float64), float(radii[0])
    for c2, r2 in zip(centres[1:], radii[1:]):
        c, r = enclose_spheres(c, r, c2, float(r2))
    return c, r


def scene_tco(TWC: np.ndarray, TWO: np.ndarray) -> np.ndarray:
    """camera-from-object pose inv(TWC) . TWO, float64"""
    return np.linalg.inv(np.asarray(TWC, np.float64)) @ np.asarray(TWO, np.float64)


def object_light_rig(dirs: Sequence, offsets: Sequence, TWO: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """world-frame point-light rig (position = dir * 10 * radius + offset) -> the same lights in the object's frame, float64 [n, 3] each"""
    R, t = np.asarray(TWO, np.float64)[:3, :3], np.asarray(TWO, np.float64)[:3, 3]
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    o = np.asarray(offsets, np.float64).reshape(-1, 3)
    return d @ R, (o - t) @ R   # row-wise R^T x


def parse_scene_lights(light_datas: Sequence[Panda3dLightData]):
    """-> (ambient (3,), point colours [(r, g, b)], world-frame dirs [n,3], offsets [n,3]); NotImplementedError for what the contract
    does not render (directional lights, more than 8 point lights)"""
    amb = np.zeros(3, np.float64)
    cols, dirs, offs = [], [], []
    for ld in light_datas:
        if ld.light_type == "ambient":
            amb += np.asarray(ld.color[:3], np.float64)
        elif ld.light_type == "point":
            d, o = _point_light(ld, len(dirs))
            dirs.append(d)
            offs.append(o)
            cols.append(tuple(float(c) for c in ld.color[:3]))
        else:
            raise NotImplementedError(f"light type {ld.light_type!r} (the scene renderer draws ambient and point lights)")
    if len(dirs) > MAX_POINT_LIGHTS:
        raise NotImplementedError(f"at most {MAX_POINT_LIGHTS} point lights per scene, got {len(dirs)}")
    return amb, cols, np.asarray(dirs, np.float64).reshape(-1, 3), np.asarray(offs, np.float64).reshape(-1, 3)


def _check_object(od: Panda3dObjectData) -> None:
    if od.color is not None or od.material is not None:
        raise NotImplementedError("object colour / material overrides are not rendered")
    if od.scale != 1:
        raise NotImplementedError("object scale != 1 is not rendered")
    if od.positioning_function is not None:
        raise NotImplementedError("object positioning_function is not supported")


def _check_camera(cd: Panda3dCameraData) -> None:
    if cd.positioning_function is not None:
        raise NotImplementedError("camera positioning_function is not supported")
    if cd.z_near != 0.1 or cd.z_far != 10:
        raise NotImplementedError("the rasteriser's clip range is z_near = 0.1, z_far = 10")


# --------------------------------------------------------------------------- renderer
class Panda3dSceneRenderer:
    def __init__(self, asset_dataset, preload_labels: Set[str] = set(), debug: bool = False, verbose: bool = False, msaa: int = 4):
        """`msaa` (engine extension, trailing keyword) = samples per pixel: 4 = the reference's configuration
        (panda3d_scene_renderer.py:73-74), 1 = one sample at the pixel centre."""
        if msaa not in (1, 4):
            raise ValueError("msaa must be 1 or 4")
        assert isinstance(preload_labels, set)
        self._asset_dataset = asset_dataset
        self.verbose = verbose
        self.debug = debug
        self.msaa = msaa
        self.debug_data = Panda3dDebugData(timings=dict())
        self._labels = [obj.label for obj in asset_dataset.list_objects]
        self._label_to_id: Dict[str, int] = {l: i for i, l in enumerate(self._labels)}
        self._db: Optional[eng.MeshDB] = None
        self._centres: Optional[np.ndarray] = None
        self._radii: Optional[np.ndarray] = None
        for label in preload_labels:
            self._label_to_id[label]   # KeyError for an unknown label, as get_object_node
        if preload_labels:
            self._ensure_db()

    def _ensure_db(self) -> eng.MeshDB:
        if self._db is None:
            meshes = [mesh_io.load_rigid_object(o) for o in self._asset_dataset.list_objects]
            self._db = eng.MeshDB(meshes)
            self._centres = np.stack([aabb_centre(m["vertices"]) for m in meshes]).astype(np.float64)
            self._radii = np.array([self._db.radius(i) for i in range(len(meshes))], np.float64)
        return self._db

    def _render(self, mesh_ids: Sequence[int], TWO: np.ndarray, scene_of_row: np.ndarray, TWC: np.ndarray, K: np.ndarray, resolution: Resolution,
                light_datas: Sequence[Panda3dLightData], render_depth: bool, render_normals: bool, with_instance_ids: bool,
                device) -> SceneRenderOutput:
        """rows (mesh id, world-from-object TWO [n,4,4] float64) drawn into scene scene_of_row[i]; per scene TWC [s,4,4], K [s,3,3]"""
        db = self._ensure_db()
        amb, cols, dirs_w, offs_w = parse_scene_lights(light_datas)
        n_scenes = TWC.shape[0]
        h, w = (int(v) for v in resolution)
        scene_of_row = np.asarray(scene_of_row, np.int64)
        order = np.argsort(scene_of_row, kind="stable")   # rows grouped per scene, list order kept inside a scene (the tie rule)
        counts = np.bincount(scene_of_row, minlength=n_scenes) if len(order) else np.zeros(n_scenes, np.int64)
        if counts.size and counts.max() > MAX_OBJECTS_PER_CAMERA:
            raise ValueError(f"at most {MAX_OBJECTS_PER_CAMERA} objects per camera, got {int(counts.max())}")
        obj_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        radius = np.zeros(n_scenes, np.float64)
        for s in range(n_scenes):
            rows = order[obj_off[s]:obj_off[s + 1]]
            ok = [i for i in rows if np.isfinite(TWO[i]).all()]   # a non-finite pose contributes nothing
            centres = [TWO[i, :3, :3] @ self._centres[mesh_ids[i]] + TWO[i, :3, 3] for i in ok]
            radius[s] = scene_sphere(centres, [self._radii[mesh_ids[i]] for i in ok])[1]
        TCO = np.zeros((len(order), 4, 4), np.float64)
        rigs = []
        for k, i in enumerate(order):
            s = scene_of_row[i]
            TCO[k] = scene_tco(TWC[s], TWO[i])
            d_o, o_o = object_light_rig(dirs_w, offs_w, TWO[i])
            rigs.append(eng.make_lights(tuple(float(a) for a in amb), [tuple(float(x) for x in v) for v in d_o], cols,
                                        [tuple(float(x) for x in v) for v in o_o]))
        flags = (eng.RASTER_MSAA4 if self.msaa == 4 else 0) | (eng.RASTER_NORMALS if render_normals else 0) | (eng.RASTER_DEPTH if render_depth else 0)
        C = 8   # rgb 0..2, normals 3..5, depth 6
        out = torch.empty(n_scenes, h, w, C, dtype=torch.float32, device=device)
        inst = torch.empty(n_scenes, h, w, dtype=torch.int32, device=device) if with_instance_ids else None
        if n_scenes:
            eng.raster_render_scene(db, [int(v) for v in obj_off], torch.as_tensor(np.asarray(mesh_ids, np.int64)[order], dtype=torch.int32, device=device),
                                    torch.from_numpy(TCO.astype(np.float32)).to(device), torch.from_numpy(np.asarray(K, np.float32).reshape(-1, 3, 3)).to(device),
                                    torch.from_numpy(radius.astype(np.float32)).to(device), eng.lights_array(rigs, device), h, w, flags, out,
                                    h * w * C, w * C, C, 0, 3 if render_normals else -1, 6 if render_depth else -1, inst)
        nchw = out.permute(0, 3, 1, 2)
        return SceneRenderOutput(rgbs=nchw[:, 0:3], normals=nchw[:, 3:6] if render_normals else None,
                                 depths=nchw[:, 6:7] if render_depth else None, instance_ids=inst)

    # -- tensor-level API ------------------------------------------------------------------------------
    def render_scenes(self, labels: List[str], TCO: torch.Tensor, K: torch.Tensor, scene_ids, resolution: Resolution,
                      light_datas: List[Panda3dLightData], render_depth: bool = False, render_normals: bool = False,
                      with_instance_ids: bool = True) -> SceneRenderOutput:
        """Render every row (label, camera-from-object TCO [n,4,4]) into the image of its scene scene_ids[i] (0 .. n_scenes - 1, e.g. the
        batch_im_id of a PoseEstimatesType; n_scenes = max + 1).  The camera sits at the world origin, so the light rig is placed around
        it; K [n,3,3]: a scene takes the K of its first row.  Returns device tensors, one image per scene."""
        n = len(labels)
        TCO = torch.as_tensor(TCO)
        assert TCO.shape == (n, 4, 4) and tuple(torch.as_tensor(K).shape) == (n, 3, 3)
        mesh_ids = [self._label_to_id[l] for l in labels]   # KeyError for an unknown label
        sid = torch.as_tensor(scene_ids).detach().cpu().numpy().astype(np.int64).reshape(-1)
        assert sid.shape == (n,) and (sid >= 0).all()
        n_scenes = int(sid.max()) + 1 if n else 0
        device = TCO.device if TCO.is_cuda else torch.device("cuda")
        T64 = TCO.detach().cpu().double().numpy()
        Kn = torch.as_tensor(K).detach().cpu().double().numpy()
        Ks = np.zeros((n_scenes, 3, 3), np.float64)
        for s in range(n_scenes):
            rows = np.nonzero(sid == s)[0]
            if len(rows):
                Ks[s] = Kn[rows[0]]
        TWC = np.repeat(np.eye(4)[None], n_scenes, 0)
        return self._render(mesh_ids, T64, sid, TWC, Ks, resolution, light_datas, render_depth, render_normals, with_instance_ids, device)

    # -- reference API ---------------------------------------------------------------------------------
    def render_scene(self, object_datas: List[Panda3dObjectData], camera_datas: List[Panda3dCameraData], light_datas: List[Panda3dLightData],
                     render_depth: bool = False, copy_arrays: bool = True, render_binary_mask: bool = False, render_normals: bool = False,
                     clear: bool = True) -> List[CameraRenderingData]:
        """One CameraRenderingData per camera (reference host types).  `copy_arrays` and `clear` are accepted: the arrays are always
        fresh, and there is no scene graph to clear."""
        start = time.time()
        for od in object_datas:
            _check_object(od)
        for cd in camera_datas:
            _check_camera(cd)
        parse_scene_lights(light_datas)   # NotImplementedError before any work
        if render_binary_mask:
            assert render_depth, "render_binary_mask needs render_depth (panda3d_scene_renderer.py:331)"
        mesh_ids = [self._label_to_id[od.label] for od in object_datas]   # KeyError for an unknown label
        TWO = np.stack([pose_matrix(od.TWO) for od in object_datas]) if object_datas else np.zeros((0, 4, 4))
        groups: "OrderedDict[Tuple[int, int], List[int]]" = OrderedDict()   # one launch per resolution (the reference's camera pools, :178-193)
        for i, cd in enumerate(camera_datas):
            groups.setdefault(tuple(int(v) for v in cd.resolution), []).append(i)
        self._ensure_db()
        setup_time = time.time() - start

        start = time.time()
        device = torch.device("cuda")
        renderings: List[Optional[CameraRenderingData]] = [None] * len(camera_datas)
        n_obj = len(object_datas)
        for res, cams in groups.items():
            TWC = np.stack([pose_matrix(camera_datas[c].TWC) for c in cams])
            K = np.stack([np.asarray(camera_datas[c].K, np.float64).reshape(3, 3) for c in cams])
            rows_TWO = np.concatenate([TWO] * len(cams)) if n_obj else np.zeros((0, 4, 4))
            scene_of_row = np.repeat(np.arange(len(cams)), n_obj)
            r = self._render(mesh_ids * len(cams), rows_TWO, scene_of_row, TWC, K, res, light_datas, render_depth, render_normals, False, device)
            rgb = torch.round(r.rgbs * 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
            nrm = torch.round(r.normals * 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy() if render_normals else None
            dep = r.depths.permute(0, 2, 3, 1).contiguous().cpu().numpy() if render_depth else None
            for k, c in enumerate(cams):
                rd = CameraRenderingData(rgb[k].copy())
                if nrm is not None:
                    rd.normals = nrm[k].copy()
                if dep is not None:
                    rd.depth = dep[k].copy()
                if render_binary_mask:
                    rd.binary_mask = rd.depth[..., 0] > 0
                renderings[c] = rd
        render_time = time.time() - start
        self.debug_data.timings["setup_time"] = setup_time
        self.debug_data.timings["render_time"] = render_time
        return renderings

    def close(self) -> None:
        if self._db is not None:
            self._db.close()
            self._db = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass
