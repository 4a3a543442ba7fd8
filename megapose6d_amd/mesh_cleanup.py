"""Cleaning up triangle meshes on the device: the connected components of a mesh, keeping the largest (or the large enough) ones, and
decimation by vertex clustering (Rossignac-Borrel): the vertices that fall into one cell of a regular grid become their mean, triangles
that lose a corner disappear.  Made for what `onboarding.reconstruct_object` extracts from a TSDF -- hundreds of thousands of small
uniform triangles, with loose fragments next to the object on real frames -- and for heavy scans (`simplify_object`).

A mesh is a dict as `TsdfVolume.extract` and `mesh_io` use them: `vertices` [V,3] float32, `faces` [F,3] int32, optionally `colors`
[V,3] float32 in 0 .. 1.  The functions take numpy arrays or tensors, move them to the device once, and return device tensors: a mesh
stays on the device from one step to the next; `to_host` ends the chain (and recomputes the normals).  Other entries of the dict
(normals, texture coordinates) do not survive: a clustered vertex has neither.

The hot path is csrc/mesh_cleanup.hip (contract: csrc/mesh_cleanup_core.h) through `engine.mesh_components`, `mesh_select`,
`mesh_cluster_count` and `mesh_cluster`; the keep bytes of `keep_components`, the grid of `grid_for` and the bisection of
`simplify(max_faces=)` are plain torch / numpy on a few numbers.  `backend` is what runs the four operations: the device by default;
the tests pass the host emulation.

Not here: removal of duplicate triangles, quadric (edge-collapse) decimation, smoothing, hole filling, "largest" by area, carrying an
existing texture over to the clustered mesh (a new one is baked from the views: `onboarding.bake_texture`).
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import mesh_io
from .object_dataset import RigidObject

MAX_DIM = 512            # cells a side (engine.MESH_MAX_DIM)
MAX_CELLS = 1 << 27      # cells of a grid (engine.MESH_MAX_CELLS)
BISECT_HI = 512          # simplify(max_faces=): cells along the longest side are searched in [1, BISECT_HI)


class DeviceBackend:
    """the four operations on device tensors (megapose6d_amd.engine), and the few array operations around them in torch"""

    def __init__(self, device="cuda"):
        self.device = device

    def mesh(self, mesh) -> Dict[str, object]:
        import torch

        dev = self.device
        for t in (mesh["vertices"], mesh["faces"]):
            if torch.is_tensor(t) and t.is_cuda:
                dev = t.device
        out = dict(vertices=torch.as_tensor(mesh["vertices"]).to(dev, torch.float32).reshape(-1, 3).contiguous(),
                   faces=torch.as_tensor(mesh["faces"]).to(dev, torch.int32).reshape(-1, 3).contiguous(), colors=None)
        if mesh.get("colors") is not None:
            out["colors"] = torch.as_tensor(mesh["colors"]).to(dev, torch.float32).reshape(-1, 3).contiguous()
        return out

    def bounds(self, vertices) -> Optional[Tuple[np.ndarray, np.ndarray]]:
        """fp32 minimum and maximum over the vertices whose three coordinates are finite (None without any)"""
        import torch

        ok = torch.isfinite(vertices).all(1)
        if not bool(ok.any()):
            return None
        v = vertices[ok]
        return v.min(0).values.cpu().numpy(), v.max(0).values.cpu().numpy()

    def components(self, n_vertices, faces):
        from . import engine as eng

        labels, face_labels, face_count, totals = eng.mesh_components(n_vertices, faces)
        return labels, face_labels, face_count, [int(v) for v in totals.cpu().tolist()]

    def keep_bytes(self, face_labels, face_count, largest: Optional[int], min_faces: Optional[int]):
        import torch

        keep = face_labels >= 0
        if largest is not None:
            keep = keep & (face_labels == largest)
        if min_faces is not None:
            keep = keep & (face_count[face_labels.clamp(min=0).long()] >= int(min_faces))
        return keep.to(torch.uint8)

    def select(self, vertices, faces, keep, colors):
        from . import engine as eng

        return eng.mesh_select(vertices, faces, keep, colors)

    def cluster_count(self, vertices, faces, origin, cell, dims):
        from . import engine as eng

        return eng.mesh_cluster_count(vertices, faces, origin, cell, dims)

    def cluster(self, vertices, faces, origin, cell, dims, colors):
        from . import engine as eng

        return eng.mesh_cluster(vertices, faces, origin, cell, dims, colors)


def _backend(backend):
    return DeviceBackend() if backend is None else backend


def _mesh_of(vertices, faces, colors) -> Dict[str, object]:
    return dict(vertices=vertices, faces=faces, colors=colors)


def to_host(mesh) -> Dict[str, Optional[np.ndarray]]:
    """-> numpy arrays, with area-weighted vertex normals recomputed (`mesh_io.vertex_normals`)"""
    host = lambda t: None if t is None else (t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t))   # noqa: E731
    v, f, c = host(mesh["vertices"]).astype(np.float32), host(mesh["faces"]).astype(np.int32), host(mesh.get("colors"))
    return dict(vertices=v, faces=f, colors=None if c is None else c.astype(np.float32), normals=mesh_io.vertex_normals(v, f).astype(np.float32))


def connected_components(mesh, backend=None) -> Dict[str, object]:
    """-> labels [V] (the smallest vertex index of each vertex's component), face_labels [F] (-1 for a face with an index outside
    [0, V)), face_count [V] (faces per label), and the integers n_components (those that own a face), largest (the label of the one
    with the most faces, the smaller label on equal counts, -1 without any) and n_bad_faces."""
    be = _backend(backend)
    m = be.mesh(mesh)
    labels, face_labels, face_count, totals = be.components(int(m["vertices"].shape[0]), m["faces"])
    if totals[3] != 0:
        raise RuntimeError(f"connected_components: the union-find ran into its iteration cap (status {totals[3]}): the labels are not usable")
    return dict(labels=labels, face_labels=face_labels, face_count=face_count, n_components=totals[0], largest=totals[1], n_bad_faces=totals[2])


def keep_components(mesh, largest: bool = True, min_faces: Optional[int] = None, backend=None) -> Dict[str, object]:
    """The mesh without its small parts: with `largest` only the component with the most faces, with `min_faces` only components of at
    least that many faces (both: the largest, if it is large enough).  Faces with a bad index go in every case.  Vertices and colours of
    what stays are copied bit for bit, in order."""
    if not largest and min_faces is None:
        raise ValueError("keep_components: nothing to do: give largest=True or min_faces")
    be = _backend(backend)
    m = be.mesh(mesh)
    cc = connected_components(m, backend=be)
    keep = be.keep_bytes(cc["face_labels"], cc["face_count"], cc["largest"] if largest else None, min_faces)
    v, f, c, _ = be.select(m["vertices"], m["faces"], keep, m["colors"])
    return _mesh_of(v, f, c)


def _extent(mesh_vertices, be, what: str):
    b = be.bounds(mesh_vertices)
    if b is None:
        raise ValueError(f"{what}: the mesh has no vertex with finite coordinates")
    lo, hi = np.asarray(b[0], np.float32), np.asarray(b[1], np.float32)
    return lo, hi - lo                       # float32: the subtraction the kernel makes for the farthest vertex


def _dims(extent: np.ndarray, cell: np.float32) -> Tuple[int, int, int]:
    return tuple(int(v) for v in np.floor(extent / cell).astype(np.int64) + 1)


def _grid_from(lo: np.ndarray, extent: np.ndarray, cells: int):
    if cells < 1:
        raise ValueError(f"grid_for: cells {cells} must be at least 1")
    if not extent.max() > 0:
        raise ValueError("grid_for: the finite vertices span no length")
    cell = np.float32(extent.max()) / np.float32(cells)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError(f"grid_for: {cells} cells along {float(extent.max())} give no usable cell size")
    dims = tuple(min(MAX_DIM, d) for d in _dims(extent, cell))
    return tuple(float(v) for v in lo), float(cell), dims


def grid_for(mesh, cells: int, backend=None) -> Tuple[Tuple[float, float, float], float, Tuple[int, int, int]]:
    """The grid with `cells` cells along the mesh's longest side -> (origin, cell, dims): origin = the fp32 minimum of the vertices with
    finite coordinates, cell = the longest extent / cells (fp32), dims = floor(extent / cell) + 1 per axis (the farthest vertex
    included), clipped to 512 a side."""
    be = _backend(backend)
    lo, extent = _extent(be.mesh(mesh)["vertices"], be, "grid_for")
    return _grid_from(lo, extent, int(cells))


def simplify(mesh, cell_size: Optional[float] = None, max_faces: Optional[int] = None, backend=None) -> Dict[str, object]:
    """Decimation by vertex clustering.  With `cell_size` (metres): the grid of that cell size from the minimum of the vertices.  With
    `max_faces`: a mesh within the budget is returned as it is; otherwise the largest number of cells along the longest side whose
    result has at most max_faces faces, by bisection on the integer `cells`: lo = 1, hi = 512; while hi - lo > 1: mid = (lo + hi) // 2,
    lo = mid if the face count of grid_for(mesh, mid) is <= max_faces else hi = mid; the result uses lo (at most 9 counts).  Raises a
    ValueError that names the cause when the result has no face, or when even lo = 1 (never counted by the search) exceeds the budget."""
    if (cell_size is None) == (max_faces is None):
        raise ValueError("simplify: give exactly one of cell_size and max_faces")
    be = _backend(backend)
    if max_faces is not None and int(mesh["faces"].shape[0]) <= int(max_faces):
        return mesh
    m = be.mesh(mesh)
    lo_v, extent = _extent(m["vertices"], be, "simplify")
    if cell_size is not None:
        cell = np.float32(cell_size)
        if not (np.isfinite(cell) and cell > 0):
            raise ValueError(f"simplify: cell_size {cell_size} must be finite and positive")
        dims = _dims(extent, cell)
        if max(dims) > MAX_DIM or dims[0] * dims[1] * dims[2] > MAX_CELLS:
            raise ValueError(f"simplify: cell_size {cell_size} gives a grid of {dims} cells: at most {MAX_DIM} a side and {MAX_CELLS} in all")
        grid = (tuple(float(v) for v in lo_v), float(cell), dims)
        cause = f"cell_size {cell_size}"
    else:
        if int(max_faces) < 1:
            raise ValueError(f"simplify: max_faces {max_faces} must be at least 1")
        lo, hi = 1, BISECT_HI
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if be.cluster_count(m["vertices"], m["faces"], *_grid_from(lo_v, extent, mid))[1] <= int(max_faces):
                lo = mid
            else:
                hi = mid
        grid = _grid_from(lo_v, extent, lo)
        cause = f"max_faces {max_faces} ({lo} cell(s) along the longest side)"
    v, f, c, _ = be.cluster(m["vertices"], m["faces"], *grid, m["colors"])
    if int(f.shape[0]) == 0:
        raise ValueError(f"simplify: no face is left at {cause}: every triangle has two corners in one cell of {grid[1]:.6g} (or an index or a "
                         f"vertex that cannot be used); use a smaller cell or a larger budget")
    if max_faces is not None and int(f.shape[0]) > int(max_faces):
        raise ValueError(f"simplify: max_faces {max_faces} cannot be met: the coarsest grid the search uses (1 cell along the longest side, "
                         f"{grid[2]} cells) still leaves {int(f.shape[0])} faces")
    return _mesh_of(v, f, c)


def clean_mesh(mesh, keep_largest: bool = True, max_faces: Optional[int] = None, backend=None) -> Dict[str, object]:
    """keep_components(largest) and / or simplify(max_faces=), on the device from end to end"""
    be = _backend(backend)
    out = mesh
    if keep_largest:
        out = keep_components(out, largest=True, backend=be)
    if max_faces is not None:
        out = simplify(out, max_faces=max_faces, backend=be)
    return out


def simplify_object(obj: RigidObject, max_faces: int, out_dir, backend=None) -> RigidObject:
    """A heavy scan made light: reads the object's mesh (`mesh_io.load_mesh_file`), simplifies it to at most max_faces faces, writes
    `<out_dir>/<label>.ply` (vertex colours kept, normals recomputed) and returns the RigidObject that names it, with the units, scale,
    symmetries and offsets of `obj`.  A mesh with texture coordinates is refused: clustering would need a texture atlas."""
    raw = mesh_io.load_mesh_file(Path(obj.mesh_path))
    if raw.get("uvs") is not None:
        raise ValueError(f"simplify_object({obj.label!r}): {obj.mesh_path} has texture coordinates; vertex clustering keeps vertex colours "
                         f"only (a texture atlas is not built)")
    mesh = dict(vertices=np.asarray(raw["vertices"], np.float32), faces=np.asarray(raw["faces"], np.int32),
                colors=None if raw.get("colors") is None else np.asarray(raw["colors"], np.float32))
    try:
        out = to_host(simplify(mesh, max_faces=max_faces, backend=backend))
    except ValueError as e:
        raise ValueError(f"simplify_object({obj.label!r}): {e}") from e
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    path = mesh_io.write_ply(out_dir / f"{obj.label}.ply", out["vertices"], out["faces"], colors=out["colors"], normals=out["normals"])
    return RigidObject(obj.label, path, category=obj.category, mesh_units=obj.mesh_units, symmetries_discrete=obj.symmetries_discrete,
                       symmetries_continuous=obj.symmetries_continuous, ypr_offset_deg=obj.ypr_offset_deg, scaling_factor=obj.scaling_factor,
                       scaling_factor_mesh_units_to_meters=obj.scaling_factor_mesh_units_to_meters)
