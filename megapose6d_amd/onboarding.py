"""Onboarding an object without a CAD model: a few dozen depth frames with known camera poses and object masks (a turntable, a robot arm,
BOP's static onboarding sequences) fused into a truncated signed distance field, and its surface written as a coloured PLY that the
renderer, MeshDataBase, bop_models_info, find_symmetries and the pose estimator take like any other mesh.

The hot path is csrc/tsdf.hip (contract: csrc/tsdf_core.h): `TsdfVolume.integrate` is one launch per call, `TsdfVolume.extract` five
launches and one read-back of two integers.  Sizing the volume (`volume_for_views`) is plain torch: it runs once per object.

`reconstruct_object(..., keep_largest=True, max_faces=N)` passes the surface through mesh_cleanup (csrc/mesh_cleanup.hip) before it is
written: only the component with the most faces, decimated by vertex clustering to at most N faces; the mesh stays on the device in between.

`bake_texture` (and `reconstruct_object(..., texture_size=S)`) gives the mesh a texture atlas baked from the same views (csrc/texture_bake.hip,
contract: csrc/texture_bake_core.h): a chart per triangle, two launches; the PLY then carries texture coordinates and names a PNG.

Frames WITHOUT camera poses (a hand-held depth camera, a turntable without encoders: BOP's dynamic onboarding) go through `track_views`
/ `reconstruct_object_unposed`: every frame is tracked against the volume the frames before it built (csrc/tsdf_track.hip, contract:
csrc/tsdf_track_core.h; `TsdfVolume.track` is 1 + 2 * iters launches and reads nothing back), then fused at its tracked pose.

Not here: coarse-to-fine pyramids, robust weights, loop closure, photometric terms or a motion model for the tracking, smoothing, hole filling, quadric decimation, charts sized by area or packed by a parametrisation,
transferring an existing texture, distances along the ray, per-pixel weights.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import engine as eng
from . import mesh_cleanup, mesh_io
from .object_dataset import RigidObject


def _to_device(t, device) -> Optional[torch.Tensor]:
    """`t` as a tensor on `device`; None stays None"""
    return None if t is None else torch.as_tensor(t).to(device)


def _check_views(who: str, depth, K, TCO=None, masks=None, rgb=None):
    """The shapes of a view set: depth [n,h,w] with n >= 1, K [n,3,3] and, where given, TCO [n,4,4], masks [n,h,w], rgb [n,h,w,3] ->
    (depth, K, TCO) as tensors.  A ValueError begins with `who`."""
    depth = torch.as_tensor(depth)
    if depth.dim() != 3 or depth.shape[0] == 0:
        raise ValueError(f"{who}: depth must be [n,h,w] with at least one view, got {tuple(depth.shape)}")
    n, frame = depth.shape[0], tuple(depth.shape)
    K, TCO = torch.as_tensor(K), None if TCO is None else torch.as_tensor(TCO)
    for name, t, shape in (("K", K, (n, 3, 3)), ("TCO", TCO, (n, 4, 4)), ("masks", masks, frame), ("rgb", rgb, frame + (3,))):
        if t is not None and tuple(torch.as_tensor(t).shape) != shape:
            raise ValueError(f"{who}: {name} must be {shape}, got {tuple(torch.as_tensor(t).shape)}")
    return depth, K, TCO


def _frame_points(depth0: torch.Tensor, K0: torch.Tensor, mask0: Optional[torch.Tensor]) -> torch.Tensor:
    """[m,3] float64: one frame's measured pixels (depth finite and > 0) inside the mask, back-projected through their centres into the
    camera's frame"""
    depth0 = torch.as_tensor(depth0).to(torch.float32)
    K0 = torch.as_tensor(K0).to(depth0.device, torch.float64)
    h, w = depth0.shape
    keep = torch.isfinite(depth0) & (depth0 > 0)
    if mask0 is not None:
        keep = keep & (torch.as_tensor(mask0).to(depth0.device) != 0)
    ys, xs = torch.meshgrid(torch.arange(h, device=depth0.device), torch.arange(w, device=depth0.device), indexing="ij")
    z = depth0[keep].to(torch.float64)
    return torch.stack([(xs[keep] + 0.5 - K0[0, 2]) / K0[0, 0] * z, (ys[keep] + 0.5 - K0[1, 2]) / K0[1, 1] * z, z], 1)


class TsdfVolume:
    """A grid of nx x ny x nz nodes, node (i,j,k) at origin + voxel_size * (i,j,k) in the object's frame (metres), holding per node the
    sum of truncated signed distances and the number of views that saw it (and, with `color`, colour sums): calls of `integrate`
    continue each other bit for bit."""

    def __init__(self, origin: Sequence[float], voxel_size: float, dims: Sequence[int], trunc_voxels: float = 3.0, color: bool = True,
                 device="cuda"):
        self.origin = tuple(float(np.float32(v)) for v in origin)
        self.voxel_size = float(np.float32(voxel_size))
        self.dims = tuple(int(v) for v in dims)
        if len(self.origin) != 3 or len(self.dims) != 3:
            raise ValueError("origin and dims have three entries")
        if not (np.isfinite(self.origin).all() and np.isfinite(self.voxel_size) and self.voxel_size > 0):
            raise ValueError(f"origin {origin} must be finite and voxel_size {voxel_size} finite and positive")
        if not (np.isfinite(trunc_voxels) and trunc_voxels > 0):
            raise ValueError(f"trunc_voxels {trunc_voxels} must be finite and positive")
        nx, ny, nz = self.dims
        if min(self.dims) < eng.TSDF_MIN_DIM or max(self.dims) > eng.TSDF_MAX_DIM or nx * ny * nz > eng.TSDF_MAX_NODES:
            raise ValueError(f"dims {self.dims}: each side {eng.TSDF_MIN_DIM} .. {eng.TSDF_MAX_DIM}, at most {eng.TSDF_MAX_NODES} nodes")
        self.trunc_voxels = float(trunc_voxels)
        self.mu = float(np.float32(trunc_voxels) * np.float32(self.voxel_size))
        self.color = bool(color)
        self._volume = eng.tsdf_volume(self.dims, self.color, device)

    @property
    def volume(self) -> torch.Tensor:
        """the planes [2 or 6, nz, ny, nx] as the kernels see them"""
        return self._volume

    @property
    def counts(self) -> torch.Tensor:
        """[nz, ny, nx] int32: the views that contributed to each node (a view of the volume; do not write)"""
        return self._volume[1].view(torch.int32)

    @property
    def field(self) -> torch.Tensor:
        """[nz, ny, nx] float32: sum / count, the mean truncated distance in units of the truncation (NaN where no view contributed)"""
        return self._volume[0] / self.counts.to(torch.float32)

    def integrate(self, depth: torch.Tensor, K: torch.Tensor, TCO: torch.Tensor, masks: Optional[torch.Tensor] = None,
                  rgb: Optional[torch.Tensor] = None, carve: bool = True, z_min: float = 1e-3) -> "TsdfVolume":
        """depth [n,h,w] metres, K [n,3,3], TCO [n,4,4] object to camera, masks [n,h,w] (non-zero: the object), rgb [n,h,w,3] uint8.
        With masks and `carve`, pixels off the object mark the nodes on their rays as free space (the visual hull)."""
        views = (_to_device(t, self._volume.device) for t in (depth, K, TCO, masks, rgb))
        eng.tsdf_integrate(self._volume, self.origin, self.voxel_size, *views, mu=self.mu, z_min=z_min, carve=carve)
        return self

    def extract(self, min_views: int = 1) -> Dict[str, np.ndarray]:
        """-> vertices [V,3] float32, faces [T,3] int32, colors [V,3] float32 in 0 .. 1, normals [V,3] float32 (area-weighted, pointing
        out of the object), as host arrays"""
        v, c, f = (t.cpu().numpy() for t in self.extract_device(min_views))
        return dict(vertices=v, faces=f, colors=c, normals=mesh_io.vertex_normals(v, f).astype(np.float32))

    def extract_device(self, min_views: int = 1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> vertices [V,3] float32, colors [V,3] float32, faces [T,3] int32 as device tensors (what mesh_cleanup continues from)"""
        return eng.tsdf_extract(self._volume, self.origin, self.voxel_size, min_views)

    def track(self, depth: torch.Tensor, K: torch.Tensor, TCO: torch.Tensor, masks: Optional[torch.Tensor] = None,
              **kw) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """The poses of unposed depth frames against what the volume holds, each from its own starting pose TCO [n,4,4]
        (engine.tsdf_track, whose keywords pass through; the volume's truncation distance is given) -> (TCO [n,4,4], status [n], used
        [n], rms [n]) on the device.  Nothing synchronises."""
        kw.setdefault("mu", self.mu)
        views = (_to_device(t, self._volume.device) for t in (depth, K, TCO, masks))
        return eng.tsdf_track(self._volume, self.origin, self.voxel_size, *views, **kw)

    def reset(self) -> None:
        self._volume.zero_()


def volume_for_views(depth: torch.Tensor, K: torch.Tensor, TCO: torch.Tensor, masks: Optional[torch.Tensor], resolution: int = 128,
                     margin_voxels: int = 4) -> Tuple[Tuple[float, float, float], float, Tuple[int, int, int]]:
    """The volume that holds what the views saw: the masked pixels with a measurement (every measured pixel without masks) are
    back-projected through their centres into the object's frame, and their bounding box, grown by margin_voxels on every side, gets
    `resolution` nodes along its longest side -> (origin, voxel_size, dims).  Plain torch on whatever device the tensors live on."""
    depth = torch.as_tensor(depth).to(torch.float32)
    K, TCO = torch.as_tensor(K).to(depth.device, torch.float64), torch.as_tensor(TCO).to(depth.device, torch.float64)
    n, h, w = depth.shape
    if resolution < 2 * margin_voxels + 2 or resolution > eng.TSDF_MAX_DIM or margin_voxels < 0:
        raise ValueError(f"resolution {resolution} must be at least 2 * margin_voxels + 2 and at most {eng.TSDF_MAX_DIM}")
    masks = _to_device(masks, depth.device)
    lo = torch.full((3,), float("inf"), dtype=torch.float64, device=depth.device)
    hi = -lo
    for v in range(n):
        pc = _frame_points(depth[v], K[v], None if masks is None else masks[v])
        if pc.shape[0] == 0:
            continue
        po = (pc - TCO[v, :3, 3]) @ TCO[v, :3, :3]          # R^T (pc - t)
        lo, hi = torch.minimum(lo, po.min(0).values), torch.maximum(hi, po.max(0).values)
    if not bool(torch.isfinite(lo).all() and torch.isfinite(hi).all()):
        raise ValueError("volume_for_views: no view holds a measured pixel of the object (depth finite and > 0 inside the mask)")
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    side = float((hi - lo).max())
    if side <= 0:
        raise ValueError("volume_for_views: the measured pixels span no length")
    voxel = side / (resolution - 1 - 2 * margin_voxels)
    origin = lo - margin_voxels * voxel
    dims = tuple(int(min(resolution, max(eng.TSDF_MIN_DIM, np.ceil((hi[c] - lo[c]) / voxel - 1e-9) + 1 + 2 * margin_voxels))) for c in range(3))
    return tuple(float(v) for v in origin), float(voxel), dims


def mean_edge_length(vertices: torch.Tensor, faces: torch.Tensor) -> float:
    """the mean length of the three edges of the faces whose indices are in range and whose corners are finite (0.0 without any); plain
    torch, one read-back"""
    f = faces.long()
    ok = ((f >= 0) & (f < vertices.shape[0])).all(1)
    if not bool(ok.any()):
        return 0.0
    tri = vertices[f[ok]]                                    # [T,3,3]
    edges = (tri - tri.roll(1, dims=1)).norm(dim=2)
    edges = edges[torch.isfinite(edges)]
    return float(edges.mean()) if edges.numel() else 0.0


def bake_texture(mesh, depth: torch.Tensor, K: torch.Tensor, TCO: torch.Tensor, masks: Optional[torch.Tensor] = None,
                 rgb: Optional[torch.Tensor] = None, texture_size: int = 1024, depth_tol: Optional[float] = None, cos_min: float = 0.2,
                 best_view: bool = False, device="cuda") -> Tuple[Dict[str, object], float]:
    """A texture atlas for `mesh` from the posed views it was reconstructed from, so that its colour resolution no longer equals its
    vertex density: every triangle gets a chart in a texture_size x texture_size atlas (engine.texture_atlas_uvs), every texel of a
    chart the cos^2-weighted mean of the colours of the views that see its surface point (engine.texture_bake; best_view: the colour of
    the view that sees it most squarely).  A texel no view sees takes the mesh's interpolated vertex colours, or white.

    mesh: a dict with `vertices` [V,3], `faces` [T,3] and optionally `colors` [V,3] in 0 .. 1, numpy arrays or tensors; a device mesh (from
    `mesh_cleanup.clean_mesh`) continues on its device.  depth [n,h,w], K [n,3,3], TCO [n,4,4], masks [n,h,w] or None, rgb [n,h,w,3] uint8.
    -> (the mesh with `uvs` [T,3,2] float32, `texture` [S,S,3] uint8 (row 0 is v = 0: what `mesh_io.write_texture` takes) and `seen`
    [S,S] uint8 (views per texel) added, all on the device; the share of the charts' texels that at least one view coloured).

    depth_tol (metres) is how far a texel's surface point may lie from the depth a view measured at its pixel and still count as seen by
    it, not as hidden behind something else.  It has to cover the distance between the mesh and the measured surface.  The surface of a
    mesh decimated by vertex clustering lies within one cell of the measured one (a clustered vertex is the mean of vertices of one
    cell), and its edges join the means of neighbouring cells, so their mean length is about one cell or more: None takes the mean edge
    length of the mesh.  For a mesh as extracted, whose edges are shorter than a voxel, the right value is the truncation distance of
    the volume (the band in which the views' depths were averaged into the surface): `reconstruct_object` passes the larger of the two.

    Every triangle gets the same chart size whatever its area, so a mesh of uniform triangles (a TSDF surface, a clustered one) uses
    the atlas best.  One launch for the coordinates, one for the bake, one read-back for the covered share (and one for the mean edge
    length when depth_tol is None)."""
    if rgb is None:
        raise ValueError("bake_texture: rgb is what the texture is made of: give the views' colour frames")
    dev = device
    for t in (mesh["vertices"], mesh["faces"]):
        if torch.is_tensor(t) and t.is_cuda:
            dev = t.device
    to_dev = lambda t, dt: torch.as_tensor(t).to(dev, dt).contiguous()   # noqa: E731
    v, f = to_dev(mesh["vertices"], torch.float32).reshape(-1, 3), to_dev(mesh["faces"], torch.int32).reshape(-1, 3)
    c = None if mesh.get("colors") is None else to_dev(mesh["colors"], torch.float32).reshape(-1, 3)
    size = int(texture_size)
    if f.shape[0] < 1 or eng.texture_atlas_block(int(f.shape[0]), size) == 0:
        raise ValueError(f"bake_texture: {int(f.shape[0])} faces (at least 1) do not fit a texture of {size} x {size} (a power of two, "
                         f"{eng.TEXTURE_MIN_SIZE} .. {eng.TEXTURE_MAX_SIZE}; two triangles share a block of at least 4 x 4 texels): "
                         f"use a larger texture_size or fewer faces (max_faces)")
    if depth_tol is None:
        depth_tol = mean_edge_length(v, f)
    if not (np.isfinite(depth_tol) and depth_tol > 0):
        raise ValueError(f"bake_texture: depth_tol {depth_tol} must be finite and positive (a mesh without a usable edge has no default)")
    views = (_to_device(t, dev) for t in (depth, K, TCO, masks, rgb))
    texels, seen = eng.texture_bake(v, f, *views, size, colors=c, depth_tol=float(depth_tol), cos_min=cos_min, best_view=best_view)
    chart = texels[..., 3] != 0
    coverage = float(((seen != 0) & chart).sum() / chart.sum().clamp(min=1))
    out = dict(mesh)
    out.update(vertices=v, faces=f, colors=c, uvs=eng.texture_atlas_uvs(int(f.shape[0]), size, device=dev),
               texture=texels[..., :3].contiguous(), seen=seen)
    return out, coverage


def reconstruct_object(label: str, depth: torch.Tensor, K: torch.Tensor, TCO: torch.Tensor, masks: Optional[torch.Tensor] = None,
                       rgb: Optional[torch.Tensor] = None, resolution: int = 128, out_dir=".", trunc_voxels: float = 3.0, min_views: int = 1,
                       carve: bool = True, device="cuda", keep_largest: bool = False, max_faces: Optional[int] = None,
                       texture_size: Optional[int] = None) -> RigidObject:
    """Posed depth views of one object -> `<out_dir>/<label>.ply` (metres, vertex normals, vertex colours: the views' where rgb is
    given, else white) and the RigidObject that names it.  Raises a ValueError that names the cause when there is no surface.
    keep_largest: only the connected component with the most faces is written (loose fragments of noisy depth or leaking masks go);
    max_faces: the surface is decimated by vertex clustering to at most that many faces (mesh_cleanup.simplify).  Both are off by
    default, and the mesh is then the extracted one bit for bit.
    texture_size: after the clean-up the mesh gets a texture atlas of that many texels a side from the views' rgb (`bake_texture`), and
    `<label>.png` is written next to a PLY that names it: no vertex colours (white times the texture, as the loader renders it),
    texture coordinates per face corner, normals.  `mesh_io.load_rigid_object` then yields `uvs` and `texture_mips` with no further
    argument.  Needs rgb.  None (the default): every byte written is what it was without the argument."""
    if texture_size is not None and rgb is None:
        raise ValueError(f"reconstruct_object({label!r}): texture_size {texture_size} needs rgb: a texture is baked from the views' colour frames")
    depth, K, TCO = _check_views(f"reconstruct_object({label!r})", depth, K, TCO, masks, rgb)
    if not bool(torch.isfinite(K).all() and torch.isfinite(TCO).all()):
        raise ValueError(f"reconstruct_object({label!r}): K or TCO holds a value that is not finite")
    try:
        origin, voxel, dims = volume_for_views(depth, K, TCO, masks, resolution=resolution)
    except ValueError as e:
        raise ValueError(f"reconstruct_object({label!r}): {e}") from e
    vol = TsdfVolume(origin, voxel, dims, trunc_voxels=trunc_voxels, color=rgb is not None, device=device)
    vol.integrate(depth, K, TCO, masks=masks, rgb=rgb, carve=carve)
    v, c, f = vol.extract_device(min_views=min_views)
    mesh = dict(vertices=v, faces=f, colors=c)
    if len(mesh["faces"]) > 0 and (keep_largest or max_faces is not None):
        try:
            mesh = mesh_cleanup.clean_mesh(mesh, keep_largest=keep_largest, max_faces=max_faces)
        except ValueError as e:
            raise ValueError(f"reconstruct_object({label!r}): {e}") from e
    baked = None
    if texture_size is not None and len(mesh["faces"]) > 0:
        try:
            baked, _ = bake_texture(mesh, depth, K, TCO, masks=masks, rgb=rgb, texture_size=texture_size,
                                    depth_tol=max(vol.mu, mean_edge_length(mesh["vertices"], mesh["faces"])), device=device)
        except ValueError as e:
            raise ValueError(f"reconstruct_object({label!r}): {e}") from e
    mesh = mesh_cleanup.to_host(mesh)
    if len(mesh["faces"]) == 0:
        seen = int((vol.counts >= min_views).sum())
        raise ValueError(f"reconstruct_object({label!r}): the surface is empty: {seen} of {vol.counts.numel()} nodes were seen by at least "
                         f"{min_views} view(s) and no complete cell holds a change of sign (poses, intrinsics or units that do not fit the depth?)")
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    if baked is not None:
        texture = mesh_io.write_texture(out_dir / f"{label}.png", baked["texture"].cpu().numpy())
        path = mesh_io.write_ply(out_dir / f"{label}.ply", mesh["vertices"], mesh["faces"], normals=mesh["normals"],
                                 uvs=baked["uvs"].cpu().numpy(), texture_file=texture.name)
    else:
        path = mesh_io.write_ply(out_dir / f"{label}.ply", mesh["vertices"], mesh["faces"], colors=mesh["colors"], normals=mesh["normals"])
    return RigidObject(label, path, mesh_units="m")


def _first_view_points(depth0: torch.Tensor, K0: torch.Tensor, mask0: Optional[torch.Tensor], who: str = "_first_view_points") -> torch.Tensor:
    """[m,3] float64: `_frame_points` of frame 0, which must hold a pixel of the object.  A ValueError begins with `who`."""
    pts = _frame_points(depth0, K0, mask0)
    if pts.shape[0] == 0:
        raise ValueError(f"{who}: frame 0 holds no measured pixel of the object (depth finite and > 0 inside the mask)")
    return pts


def volume_for_first_view(depth0: torch.Tensor, K0: torch.Tensor, TCO0: torch.Tensor, mask0: Optional[torch.Tensor], resolution: int = 128,
                          extent: Optional[float] = None) -> Tuple[Tuple[float, float, float], float, Tuple[int, int, int]]:
    """The volume to track a sequence in when only its first frame is known: a cube of `resolution` nodes a side -> (origin,
    voxel_size, dims).  Frame 0's measured pixels inside the mask are taken to the object's frame by TCO0; with L the longest side of
    their bounding box, the cube has the side `extent`, or 2 L when extent is None, and is centred at the box's centre moved L / 2 along
    the viewing direction: frame 0 sees only the near side of the object, the rest lies behind it.  An object that reaches deeper than
    1.5 L behind its nearest visible point (a long object seen end-on) leaves that cube: give `extent`.  Plain torch, one read-back."""
    if not (eng.TSDF_MIN_DIM <= int(resolution) <= eng.TSDF_MAX_DIM):
        raise ValueError(f"resolution {resolution} must be {eng.TSDF_MIN_DIM} .. {eng.TSDF_MAX_DIM}")
    pts = _first_view_points(depth0, K0, mask0, who="volume_for_first_view")
    T = torch.as_tensor(TCO0).to(pts.device, torch.float64)
    po = (pts - T[:3, 3]) @ T[:3, :3]                        # R^T (pc - t)
    box = torch.stack([po.min(0).values, po.max(0).values, T[2, :3]]).cpu().numpy()          # the camera's z axis in the object's frame
    lo, hi, axis = box
    L = float((hi - lo).max())
    side = float(extent) if extent is not None else 2.0 * L
    if not (np.isfinite(side) and side > 0):
        raise ValueError(f"volume_for_first_view: the cube's side {side} must be finite and positive (frame 0's pixels span no length: give extent)")
    centre = 0.5 * (lo + hi) + 0.5 * L * axis
    voxel = side / (int(resolution) - 1)
    return tuple(float(v) for v in centre - 0.5 * side), float(voxel), (int(resolution),) * 3


def track_views(depth: torch.Tensor, K: torch.Tensor, masks: Optional[torch.Tensor] = None, TCO_first: Optional[torch.Tensor] = None,
                resolution: int = 128, extent: Optional[float] = None, trunc_voxels: float = 3.0, iters: int = 10, min_pixels: int = 64,
                rms_max: Optional[float] = None, device="cuda") -> Tuple[torch.Tensor, torch.Tensor, Dict[str, object]]:
    """The camera poses of a sequence of depth frames of one object (a hand-held camera, a turntable without encoders: BOP's dynamic
    onboarding), frame by frame against the volume the frames before it built: frame 0 is integrated at TCO_first, frame k is tracked
    from the last tracked pose (`TsdfVolume.track`) and, when it tracked, integrated with carving at its tracked pose.  depth [n,h,w]
    metres, K [n,3,3], masks [n,h,w] or None -> (TCO [n,4,4] float32 object to camera, tracked [n] bool, info), the first two on the device.

    TCO_first fixes the object's frame; None puts its origin at the centroid of frame 0's points with the camera's axes.  The volume is
    `volume_for_first_view`'s (resolution, extent).  A frame tracked when its status is 0 or 1, and, with rms_max (metres) given, its
    residual is at most rms_max; None does not test the residual.  A lost frame keeps the pose before it, is flagged and is not
    integrated -- a wrong pose would carve the object away -- and the sequence goes on from the last tracked pose.  Consecutive
    frames must overlap within the truncation band (trunc_voxels voxels): there is no motion model beyond "hold the last pose".
    One read-back of (status, used, rms) per frame.  info: `status`, `used`, `rms` as numpy arrays per frame (frame 0: 1, 0, 0), the
    `volume` (a TsdfVolume) as the last frame left it."""
    depth, K, _ = _check_views("track_views", depth, K, masks=masks)
    n = depth.shape[0]
    depth, K = depth.to(device, torch.float32), K.to(device, torch.float32)
    masks = _to_device(masks, device)
    if TCO_first is None:
        pts = _first_view_points(depth[0], K[0], None if masks is None else masks[0], who="track_views")
        first = torch.eye(4, dtype=torch.float64, device=depth.device)
        first[:3, 3] = pts.mean(0)
    else:
        first = torch.as_tensor(TCO_first).to(depth.device, torch.float64)
        if tuple(first.shape) != (4, 4) or not bool(torch.isfinite(first).all()):
            raise ValueError("track_views: TCO_first must be a finite [4,4] pose")
    try:
        origin, voxel, dims = volume_for_first_view(depth[0], K[0], first, None if masks is None else masks[0], resolution=resolution, extent=extent)
    except ValueError as e:
        raise ValueError(f"track_views: {e}") from e
    vol = TsdfVolume(origin, voxel, dims, trunc_voxels=trunc_voxels, color=False, device=device)
    poses = torch.empty(n, 4, 4, dtype=torch.float32, device=depth.device)
    poses[0] = first.to(torch.float32)
    status, used, rms = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    status[0] = 1
    tracked = [True]
    m = lambda k: None if masks is None else masks[k:k + 1]   # noqa: E731
    vol.integrate(depth[:1], K[:1], poses[:1], masks=m(0))
    last = poses[:1]
    for k in range(1, n):
        T, st, us, rm = vol.track(depth[k:k + 1], K[k:k + 1], last, masks=m(k), iters=iters, min_pixels=min_pixels)
        back = torch.cat([st.to(torch.float64), us.to(torch.float64), rm.to(torch.float64)]).cpu().numpy()      # the frame's one read-back
        status[k], used[k], rms[k] = int(back[0]), int(back[1]), back[2]
        ok = status[k] >= 0 and (rms_max is None or float(rms[k]) <= rms_max)
        tracked.append(bool(ok))
        if ok:
            last = T
            vol.integrate(depth[k:k + 1], K[k:k + 1], T, masks=m(k))
        poses[k] = last[0]
    return poses, torch.as_tensor(tracked, device=depth.device), dict(status=status, used=used, rms=rms, volume=vol)


def reconstruct_object_unposed(label: str, depth: torch.Tensor, K: torch.Tensor, masks: Optional[torch.Tensor] = None,
                               rgb: Optional[torch.Tensor] = None, TCO_first: Optional[torch.Tensor] = None, resolution: int = 128,
                               extent: Optional[float] = None, trunc_voxels: float = 3.0, iters: int = 10, min_pixels: int = 64,
                               rms_max: Optional[float] = None, device="cuda", **kw) -> RigidObject:
    """Depth frames of one object WITHOUT camera poses -> `<out_dir>/<label>.ply` and its RigidObject: `track_views` finds the poses,
    `reconstruct_object` then fuses the frames that tracked at their tracked poses into a volume of its own, sized tightly around what
    they saw (the tracking volume is twice as wide as the object and half as fine).  The object's frame is the one TCO_first fixes (see
    `track_views`).  Every keyword of `reconstruct_object` passes through (out_dir, min_views, carve, keep_largest, max_faces,
    texture_size); resolution and trunc_voxels hold for both passes.  Raises a ValueError that names the count when fewer than two
    frames tracked."""
    poses, tracked, info = track_views(depth, K, masks=masks, TCO_first=TCO_first, resolution=resolution, extent=extent, trunc_voxels=trunc_voxels,
                                       iters=iters, min_pixels=min_pixels, rms_max=rms_max, device=device)
    n_tracked = int(tracked.sum())
    if n_tracked < 2:
        raise ValueError(f"reconstruct_object_unposed({label!r}): {n_tracked} of {len(tracked)} frames tracked, at least 2 are needed "
                         f"(status per frame: {info['status'].tolist()}; frames that overlap too little, or an object deeper than the volume: extent?)")
    keep = tracked.to(poses.device)
    pick = lambda t: None if t is None else torch.as_tensor(t).to(poses.device)[keep]   # noqa: E731
    return reconstruct_object(label, pick(depth), pick(K), poses[keep], masks=pick(masks), rgb=pick(rgb), resolution=resolution,
                              trunc_voxels=trunc_voxels, device=device, **kw)
