"""Mesh database for the pose math: points of every object, padded to a common count, and the deterministic
2000-/200-point subsets the crop logic projects.

Mirrors what the reference builds in src/megapose/lib3d/rigid_mesh_database.py (MeshDataBase :57-88, batched :90-130,
BatchedMeshes.select :146-153, Meshes.sample_points :168-169, pad_stack_tensors :172-200) and
src/megapose/lib3d/mesh_ops.py:77-87 (np.random.RandomState(0).choice without replacement), but samples ONCE per
database on the host (the reference re-draws the same permutation for every batch) and keeps everything resident.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import mesh_io
from .tcoll import TensorCollection


def _pad_points(point_sets: Sequence[torch.Tensor]) -> torch.Tensor:
    """Pad every point set to the longest one with randomly re-drawn points of the same object (seeded; duplicates
    do not change any min/max the pipeline computes)."""
    longest = max(p.shape[0] for p in point_sets)
    draw = np.random.RandomState(0)
    padded = []
    for p in point_sets:
        missing = longest - p.shape[0]
        if missing > 0:
            p = torch.cat((p, p[draw.choice(np.arange(p.shape[0]), size=missing)]), dim=0)
        padded.append(p)
    return torch.stack(padded)


def deterministic_point_ids(n_available: int, n_points: int) -> np.ndarray:
    if n_points > n_available:
        raise AssertionError(f"need at least {n_points} mesh points, got {n_available} (lib3d/mesh_ops.py:79)")
    return np.random.RandomState(0).choice(n_available, size=n_points, replace=False)


class Meshes(TensorCollection):
    def __init__(self, infos, labels, points, symmetries):
        super().__init__(points=points, symmetries=symmetries)
        self.infos = infos
        self.labels = np.asarray(labels)

    def sample_points(self, n_points: int, deterministic: bool = False) -> torch.Tensor:
        n_total = self.points.shape[1]
        if deterministic:
            ids = deterministic_point_ids(n_total, n_points)
        else:
            ids = np.random.choice(n_total, size=n_points, replace=False)
        return torch.index_select(self.points, 1, torch.as_tensor(ids, device=self.points.device))


class BatchedMeshes(TensorCollection):
    """points [n_obj, N_max, 3] (metres, float32) + label bookkeeping; `.select(labels)` gathers rows."""

    def __init__(self, infos, labels, points, symmetries):
        super().__init__(points=points, symmetries=symmetries)
        self.infos = infos
        self.labels = np.asarray(labels)
        self.label_to_id = {label: n for n, label in enumerate(labels)}
        self._sampled: Dict[int, torch.Tensor] = {}

    @property
    def n_sym_mapping(self) -> Dict[str, int]:
        return {label: obj["n_sym"] for label, obj in self.infos.items()}

    def ids(self, labels: Sequence[str]) -> List[int]:
        return [self.label_to_id[l] for l in labels]  # KeyError for unknown labels, like the reference

    def select(self, labels: Sequence[str]) -> Meshes:
        ids = self.ids(labels)
        return Meshes([self.infos[l] for l in labels], self.labels[ids], self.points[ids], self.symmetries[ids])

    def sampled_points(self, n_points: int = 2000) -> torch.Tensor:
        """[n_obj, n_points, 3]: the deterministic subset; its first 200 rows are the 200-point subset
        (RandomState.choice(replace=False) = permutation prefix)."""
        if n_points not in self._sampled:
            ids = torch.as_tensor(deterministic_point_ids(self.points.shape[1], n_points), device=self.points.device)
            self._sampled[n_points] = torch.index_select(self.points, 1, ids).contiguous()
        return self._sampled[n_points]

    def to(self, target):
        super().to(target)
        self._sampled = {}
        return self


def with_symmetries(meshes: BatchedMeshes, poses: Dict[str, object]) -> BatchedMeshes:
    """`meshes` with the symmetry sets of the objects named in `poses` replaced: {label: [n,4,4] poses, the identity first} (e.g.
    evaluation.symmetry_poses of a row of evaluation.find_symmetries).  The other objects keep theirs; the table is identity-padded
    to the longest set and n_sym is rewritten, as MeshDataBase builds them.  The points are shared, not copied; `meshes` is left
    alone.  An unknown label raises KeyError."""
    labels = list(meshes.labels)
    sets = {l: meshes.symmetries[n, : meshes.infos[l]["n_sym"]].detach().cpu().double() for n, l in enumerate(labels)}
    for l, p in poses.items():
        if l not in sets:
            raise KeyError(l)
        p = torch.as_tensor(np.asarray(p, np.float64)).reshape(-1, 4, 4)
        if p.shape[0] < 1:
            raise ValueError(f"object {l!r}: a symmetry set holds at least the identity")
        sets[l] = p
    s_max = max(s.shape[0] for s in sets.values())
    sym = torch.eye(4).repeat(len(labels), s_max, 1, 1)
    infos = {l: dict(meshes.infos[l]) for l in labels}
    for n, l in enumerate(labels):
        sym[n, : sets[l].shape[0]] = sets[l].float()
        infos[l]["n_sym"] = int(sets[l].shape[0])
    return BatchedMeshes(infos, labels, meshes.points, sym.to(meshes.points.device))


class MeshDataBase:
    def __init__(self, obj_list):
        self.obj_list = list(obj_list)
        self.obj_dict = {o.label: o for o in self.obj_list}
        self.infos = {o.label: dict() for o in self.obj_list}
        self.engine_meshes = {o.label: mesh_io.load_rigid_object(o) for o in self.obj_list}
        for o in self.obj_list:
            if getattr(o, "diameter_meters", None) is None:
                pts = self.engine_meshes[o.label]["points"].astype(np.float64)
                o.diameter_meters = float(np.linalg.norm(pts.max(0) - pts.min(0)))

    @staticmethod
    def from_object_ds(object_ds) -> "MeshDataBase":
        return MeshDataBase([object_ds[n] for n in range(len(object_ds))])

    @property
    def labels(self) -> List[str]:
        return [o.label for o in self.obj_list]

    def batched(self, aabb: bool = False, resample_n_points: Optional[int] = None, n_sym: int = 64) -> BatchedMeshes:
        if aabb or resample_n_points:
            raise NotImplementedError("only the hot-path configuration (all vertices) is supported")
        pts = [torch.from_numpy(self.engine_meshes[l]["points"]) for l in self.labels]
        infos = {l: {"n_points": int(p.shape[0])} for l, p in zip(self.labels, pts)}
        return BatchedMeshes(infos, self.labels, _pad_points(pts).float(), self._symmetries(n_sym, infos))

    def _symmetries(self, n_sym: int, infos) -> torch.Tensor:
        """the symmetry sets, identity-padded to the longest one (rigid_mesh_database.py:117-129); writes n_sym into infos"""
        syms = [torch.as_tensor(np.asarray(self.obj_dict[l].make_symmetry_poses(n_symmetries_continuous=n_sym))).float() for l in self.labels]
        s_max = max(s.shape[0] for s in syms)
        sym = torch.eye(4).repeat(len(syms), s_max, 1, 1)
        for n, (l, s) in enumerate(zip(self.labels, syms)):
            sym[n, : s.shape[0]] = s
            infos[l]["n_sym"] = int(s.shape[0])
        return sym

    def batched_surface(self, n_points: int, n_sym: int = 64, seed: int = 0, device="cuda") -> BatchedMeshes:
        """What the reference's batched(resample_n_points=n_points) gives (rigid_mesh_database.py:100-104): every object's vertices
        replaced by n_points points drawn uniformly over its surface (trimesh.sample.sample_surface), here by one launch of
        engine.surface_sample on `device` for all objects, on uniforms drawn by a CPU generator seeded with `seed`: the same points on
        every machine.  An object without faces (a point cloud) keeps the deterministic subset of n_points of its vertices, the
        reference's other branch (AssertionError if it has fewer).  An object the sampler fails (a non-finite coordinate, a face
        index outside its vertices, no area) raises ValueError with its label.  CPU float32 tensors like batched(): the caller moves
        them; nothing is padded, infos[label]["n_points"] == n_points for every object."""
        n_points = int(n_points)
        if n_points < 1:
            raise ValueError(f"n_points must be at least 1, got {n_points}")
        labels = self.labels
        meshed = [l for l in labels if len(self.engine_meshes[l]["faces"]) > 0]
        points = torch.empty(len(labels), n_points, 3, dtype=torch.float32)
        for n, l in enumerate(labels):
            if l not in meshed:
                pts = self.engine_meshes[l]["points"]
                points[n] = torch.from_numpy(pts[deterministic_point_ids(len(pts), n_points)])
        if meshed:
            from . import engine as eng

            verts = [self.engine_meshes[l]["points"] for l in meshed]
            faces = [self.engine_meshes[l]["faces"] for l in meshed]
            vert_off = np.concatenate([[0], np.cumsum([len(v) for v in verts])])
            face_off = np.concatenate([[0], np.cumsum([len(f) for f in faces])])
            u = torch.rand(len(meshed), n_points, 3, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)
            sampled, face = eng.surface_sample(torch.from_numpy(np.concatenate(verts).astype(np.float32)).to(device),
                                               torch.from_numpy(np.concatenate(faces).astype(np.int32)).to(device), vert_off, face_off, u.to(device))
            sampled, face = sampled.cpu(), face.cpu()
            for k, l in enumerate(meshed):
                if int(face[k, 0]) < 0:
                    raise ValueError(f"object {l!r} cannot be sampled: a non-finite vertex, a face index outside its vertices, or no area")
                points[labels.index(l)] = sampled[k]
        infos = {l: {"n_points": n_points} for l in labels}
        sym = self._symmetries(n_sym, infos)
        return BatchedMeshes(infos, labels, points, sym)

    def batched_aabb(self, n_sym: int = 64) -> BatchedMeshes:
        """What the reference's batched(aabb=True) gives (rigid_mesh_database.py:96-99): every object's vertices replaced by the eight
        corners of its axis-aligned box, in the order of lib3d/mesh_ops.py get_meshes_bounding_boxes: v0 = (xmin, ymax, zmax),
        v1 = (xmax, ymax, zmax), v2 = (xmax, ymin, zmax), v3 = (xmin, ymin, zmax), v4 .. v7 the same at zmin.  The exact minimum
        and maximum of the metre-scaled vertices, on the host."""
        labels = self.labels
        points = torch.empty(len(labels), 8, 3, dtype=torch.float32)
        for n, l in enumerate(labels):
            pts = self.engine_meshes[l]["points"]
            (x0, y0, z0), (x1, y1, z1) = pts.min(0), pts.max(0)
            points[n] = torch.as_tensor([[x0, y1, z1], [x1, y1, z1], [x1, y0, z1], [x0, y0, z1],
                                         [x0, y1, z0], [x1, y1, z0], [x1, y0, z0], [x0, y0, z0]], dtype=torch.float32)
        infos = {l: {"n_points": 8} for l in labels}
        sym = self._symmetries(n_sym, infos)
        return BatchedMeshes(infos, labels, points, sym)
