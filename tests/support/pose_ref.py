"""Float64 reference of the pose / camera-geometry math of megapose6d_amd/csrc/pose.hip.  TEST INFRASTRUCTURE ONLY.

Plain numpy, float64 throughout; nothing is imported from the package or from oracle/.  Inputs are the fp32 arrays a kernel receives,
widened exactly, so each function answers "what is the exact result for these fp32 inputs" and every difference to it is the rounding of
whoever computed the other side.  The functions are written the obvious way (np.linalg.inv, cross products, matrix products), not as the
kernel's closed forms: a second route to the same numbers.  Like oracle/geometry.py each cites the reference lines it follows (paths under
src/megapose/ of the reference project).

The second half (`*_scales`, `units`) is the error model of the kernel tests: per output a scale S, computed per row from this
reference, so that a bound reads |got - ref| <= k * 2^-24 * S.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

EPS24 = 2.0 ** -24
Z_MIN = 0.1                                   # lib3d/camera_geometry.py:40 (z_min of project_points_robust)
MODES = {"TCO": 0, "TCO+front_3views": 1, "TCO+front_1view": 2, "sphere_26views": 3}
MODE_NAMES = {v: k for k, v in MODES.items()}
# OpenCV camera axes (x right, y down, z forward) from the scene-graph camera's (x right, y forward, z up)
CV_FROM_NODE = np.array([[1.0, 0, 0, 0], [0, 0, -1.0, 0], [0, 1.0, 0, 0], [0, 0, 0, 1.0]])


def f64(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64)


def _unit(v: np.ndarray) -> np.ndarray:
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# --------------------------------------------------------------------------- #
# rotations and transforms
def ortho6d_to_R(x_raw, y_raw) -> np.ndarray:
    """lib3d/rotations.py:25-40: Gram-Schmidt of two 3-vectors; the columns of R are (x, y, z)."""
    x = _unit(f64(x_raw))
    z = _unit(np.cross(x, f64(y_raw)))
    y = np.cross(z, x)
    return np.stack([x, y, z], axis=-1)


def ortho6d_sin(x_raw, y_raw) -> np.ndarray:
    """sine of the angle between the two 6D vectors (the conditioning of ortho6d_to_R)"""
    return np.linalg.norm(np.cross(_unit(f64(x_raw)), _unit(f64(y_raw))), axis=-1)


def normalize_T(T) -> np.ndarray:
    """lib3d/transform_ops.py:106-119: re-orthonormalise the rotation from its first two columns, keep the translation."""
    T = f64(T)
    out = np.zeros_like(T)
    out[..., :3, :3] = ortho6d_to_R(T[..., :3, 0], T[..., :3, 1])
    out[..., :3, 3] = T[..., :3, 3]
    out[..., 3, 3] = 1.0
    return out


# --------------------------------------------------------------------------- #
# SO(3)-grid initialisation
def init_extents(points, R) -> np.ndarray:
    """x / y extents of R p over each mesh's points: [n_mesh, n_rot, 2] (the min / max of lib3d/cosypose_ops.py:197-204; a translation
    does not change an extent)."""
    rp = np.einsum("rij,mnj->mrni", f64(R), f64(points))
    return (rp.max(axis=2) - rp.min(axis=2))[..., :2]


def init_extents_scale(points, R) -> np.ndarray:
    """largest |R p| component that enters an extent, per (mesh, rotation)"""
    rp = np.einsum("rij,mnj->mrni", f64(R), f64(points))
    return np.abs(rp[..., :2]).max(axis=(2, 3))


def init_poses_from_boxes(boxes, K, points, R) -> np.ndarray:
    """lib3d/cosypose_ops.py:169-218 (TCO_init_from_boxes_autodepth_with_R).  points [b, n, 3] and R [b, 3, 3] are per row."""
    boxes, K, points, R = f64(boxes), f64(K), f64(points), f64(R)
    b = boxes.shape[0]
    fx, fy, cx, cy = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    rp = np.einsum("bij,bnj->bni", R, points)
    d3 = rp.max(axis=1) - rp.min(axis=1)
    bdx = boxes[:, 2] - boxes[:, 0] + 1.0
    bdy = boxes[:, 3] - boxes[:, 1] + 1.0
    z = (fy * d3[:, 1] / bdy + fx * d3[:, 0] / bdx) / 2.0
    u = (boxes[:, 0] + boxes[:, 2]) / 2.0
    v = (boxes[:, 1] + boxes[:, 3]) / 2.0
    T = np.tile(np.eye(4), (b, 1, 1))
    T[:, :3, :3] = R
    T[:, 0, 3] = (u - cx) * z / fx
    T[:, 1, 3] = (v - cy) * z / fy
    T[:, 2, 3] = z
    return T


# --------------------------------------------------------------------------- #
# multiview cameras
def view_offsets(mode: int) -> np.ndarray:
    """camera offsets of a view list in units of |tCR|, in the look-at frame (x right, y forward, z up): lib3d/multiview.py:95-162"""
    if mode == MODES["TCO+front_1view"]:
        return np.zeros((1, 3))
    if mode == MODES["TCO+front_3views"]:
        return np.array([[0.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0]])
    if mode == MODES["sphere_26views"]:
        return np.array([[x, y, z] for y in (0, 1, 2) for x in (0, -1, 1) for z in (0, 1, -1) if (x, y, z) != (0, 1, 0)], dtype=np.float64)
    raise ValueError(mode)


def n_views(mode: int, remove_TCO: bool, inplane: bool) -> int:
    if mode == MODES["TCO"]:
        return 1
    return ((0 if remove_TCO else 1) + len(view_offsets(mode))) * (4 if inplane else 1)


def look_at(pos, target, up) -> Tuple[np.ndarray, np.ndarray]:
    """Scene-graph look-at, forward exact: y = unit(target - pos), x = unit(y x up), z = x x y.  Returns the node's axes as the columns
    of a rotation, and |y x up| before normalisation (the conditioning of the construction)."""
    y = _unit(target - pos)
    x_raw = np.cross(y, up)
    x = _unit(x_raw)
    z = np.cross(x, y)
    return np.stack([x, y, z], axis=-1), np.linalg.norm(x_raw, axis=-1)


def multiview_cameras(TCO, tCR, mode: int, remove_TCO: bool = False, inplane: bool = False, detail: bool = False):
    """lib3d/multiview.py:165-246 (make_TCO_multiview) with :31-92 (the look-at cameras): -> TCV_O [b, V, 4, 4].
    One view in all: [TCO], whatever the type (:186-193).  Otherwise [TCO unless removed] + one camera per offset of the type, each
    placed in the look-at frame of the camera position and turned to the reference point; with in-plane copies every view appears four
    times, turned by 0 / 90 / 180 / 270 degrees about its optical axis (:236-245)."""
    TCO, tCR = f64(TCO), f64(tCR)
    b = TCO.shape[0]
    V = n_views(mode, remove_TCO, inplane)
    aux = {"cross_norm_min": np.full(b, np.inf)}
    if V == 1:
        views = TCO[:, None].copy()
        return (views, aux) if detail else views
    TOC = np.linalg.inv(TCO)
    p0 = TOC[:, :3, 3]                                       # camera position in the object frame
    up = -TOC[:, :3, 1]                                      # the image's up direction in the object frame
    ref = np.einsum("bij,bj->bi", TOC[:, :3, :3], tCR) + p0  # reference point in the object frame
    radius = np.linalg.norm(tCR, axis=-1)
    L, n0 = look_at(p0, ref, up)
    aux["cross_norm_min"] = np.minimum(aux["cross_norm_min"], n0)
    views = [] if remove_TCO else [TCO]
    for off in view_offsets(mode):
        pn = p0 + np.einsum("bij,j->bi", L, off) * radius[:, None]
        Rn, n1 = look_at(pn, ref, up)
        aux["cross_norm_min"] = np.minimum(aux["cross_norm_min"], n1)
        TO_node = np.tile(np.eye(4), (b, 1, 1))              # the camera node in the object frame
        TO_node[:, :3, :3] = Rn
        TO_node[:, :3, 3] = pn
        TO_CV = TO_node @ np.linalg.inv(CV_FROM_NODE)        # OpenCV camera in the object frame
        views.append(np.linalg.inv(TO_CV))
    views = np.stack(views, axis=1)
    if inplane:
        assert remove_TCO                                    # multiview.py:237
        turned = []
        for q in range(4):
            c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][q]   # exact quarter turns about z
            Rz = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])
            t = Rz @ views
            t[..., :3, 3] = views[..., :3, 3]                # only the rotation block turns
            turned.append(t)
        views = np.stack(turned, axis=2).reshape(b, -1, 4, 4)
    assert views.shape[1] == V
    return (views, aux) if detail else views


# --------------------------------------------------------------------------- #
# projection, crop boxes, crop intrinsics
def project_points(points, K, T) -> Tuple[np.ndarray, np.ndarray]:
    """lib3d/camera_geometry.py:40-53 (project_points_robust): -> (uv [..., n, 2], unclamped depth [..., n])"""
    P = f64(K) @ f64(T)[..., :3, :]
    ph = np.concatenate([f64(points), np.ones(points.shape[:-1] + (1,))], axis=-1)
    suv = np.einsum("...ij,...nj->...ni", P, ph)
    z = suv[..., 2]
    return suv[..., :2] / np.maximum(Z_MIN, z)[..., None], z


def project_boxes(points, K, T) -> np.ndarray:
    """robust projection + lib3d/camera_geometry.py:56-64 (boxes_from_uv): (umin, vmin, umax, vmax) per row"""
    uv, _ = project_points(points, K, T)
    return np.concatenate([uv.min(axis=-2), uv.max(axis=-2)], axis=-1)


def crop_boxes(center_uv, boxes_rend, im_hw, lamb: float = 1.4) -> np.ndarray:
    """lib3d/cropping.py:30-67 (deepim_boxes with the rendered box on both sides, clamp=False): a box centred on the projected reference
    point, wide enough for the rendered box times lamb, with the aspect ratio longer side : shorter side of the image."""
    center_uv, boxes_rend = f64(center_uv), f64(boxes_rend)
    xc, yc = center_uv[..., 0], center_uv[..., 1]
    r = max(im_hw) / min(im_hw)
    xdist = np.maximum(np.abs(boxes_rend[..., 0] - xc), np.abs(boxes_rend[..., 2] - xc))
    ydist = np.maximum(np.abs(boxes_rend[..., 1] - yc), np.abs(boxes_rend[..., 3] - yc))
    width = np.maximum(xdist, ydist * r) * 2 * lamb
    height = np.maximum(xdist / r, ydist) * 2 * lamb
    return np.stack([xc - width / 2, yc - height / 2, xc + width / 2, yc + height / 2], axis=-1)


def K_crop_resize(K, boxes, out_hw) -> np.ndarray:
    """lib3d/camera_geometry.py:67-115 (get_K_crop_resize): intrinsics of the crop `boxes` resized to longer x shorter side of out_hw.
    Shift the principal point into the crop, then scale about the crop's pixel centre; the other entries are kept."""
    K, boxes = f64(K), f64(boxes)
    fw, fh = float(max(out_hw)), float(min(out_hw))
    cw, ch = boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]
    sx, sy = fw / cw, fh / ch
    out = K.copy()
    out[..., 0, 0] = sx * K[..., 0, 0]
    out[..., 1, 1] = sy * K[..., 1, 1]
    # principal point relative to the crop's centre pixel ((cw - 1) / 2 from its corner), scaled, relative to the output's centre pixel
    out[..., 0, 2] = (fw - 1) / 2 + sx * (K[..., 0, 2] - (boxes[..., 0] + boxes[..., 2]) / 2)
    out[..., 1, 2] = (fh - 1) / 2 + sy * (K[..., 1, 2] - (boxes[..., 1] + boxes[..., 3]) / 2)
    return out


def _crop_of(points, K, T, im_hw, lamb):
    """crop_inputs / compute_crops_multiview for one camera per row (models/pose_rigid.py:180-303): the anchor is the camera's own
    translation, i.e. the projection of the object origin."""
    uv, z = project_points(points, K, T)
    brend = np.concatenate([uv.min(axis=-2), uv.max(axis=-2)], axis=-1)
    centre, zc = project_points(np.zeros(points.shape[:-2] + (1, 3)), K, T)
    bcrop = crop_boxes(centre[..., 0, :], brend, im_hw, lamb)
    return brend, bcrop, (z < Z_MIN).mean(axis=-1), zc[..., 0] < Z_MIN


def pose_prepare_detail(TCO_in, K, mesh_ids, points, n_pts_main: int, n_pts_views: int, mode: int, remove_TCO: bool, inplane: bool,
                        im_hw, out_hw, lamb: float = 1.4) -> Dict[str, np.ndarray]:
    """The composition of models/pose_rigid.py:524-552: the seven outputs of engine.pose_prepare(..., with_K_main=True) under their names,
    plus what the error model and the case conditions need (per-view crop boxes, clamp statistics, look-at conditioning)."""
    K, points = f64(K), f64(points)
    ids = np.asarray(mesh_ids).astype(np.int64)
    TCO_n = normalize_T(TCO_in)
    tCR = TCO_n[:, :3, 3].copy()
    TCV_O, aux = multiview_cameras(TCO_n, tCR, mode, remove_TCO, inplane, detail=True)
    V = TCV_O.shape[1]
    P_main, P_views = points[ids, :n_pts_main], points[ids, :n_pts_views]
    brend, bcrop, frac_clamped, centre_clamped = _crop_of(P_main, K, TCO_n, im_hw, lamb)
    K_main = K_crop_resize(K, bcrop, out_hw)
    _, bcrop_v, _, _ = _crop_of(P_views[:, None], K[:, None], TCV_O, im_hw, lamb)
    KV_crop = K_crop_resize(np.broadcast_to(K[:, None], (K.shape[0], V, 3, 3)), bcrop_v, out_hw)
    if not remove_TCO:                                       # models/pose_rigid.py:550-552
        KV_crop[:, 0] = K_main
        bcrop_v[:, 0] = bcrop
    return dict(TCO_n=TCO_n, tCR=tCR, TCV_O=TCV_O, KV_crop=KV_crop, boxes_rend=brend, boxes_crop=bcrop, K_main=K_main,
                boxes_crop_views=bcrop_v, frac_clamped=frac_clamped, centre_clamped=centre_clamped, cross_norm_min=aux["cross_norm_min"])


PREPARE_OUTPUTS = ("TCO_n", "tCR", "TCV_O", "KV_crop", "boxes_rend", "boxes_crop", "K_main")


def pose_prepare(*args, **kw):
    d = pose_prepare_detail(*args, **kw)
    return tuple(d[n] for n in PREPARE_OUTPUTS)


# --------------------------------------------------------------------------- #
def pose_update(TCO, K_crop, out9, tCR) -> np.ndarray:
    """models/pose_rigid.py:305-312 + lib3d/cosypose_ops.py:33-58: rotate about the reference point by the 6D rotation, move the
    reference point by (vx, vy) pixels of the crop camera and scale its depth by vz."""
    TCO, K, o, tCR = f64(TCO), f64(K_crop), f64(out9), f64(tCR)
    dR = ortho6d_to_R(o[:, 0:3], o[:, 3:6])
    z_src = tCR[:, 2]
    z_tgt = o[:, 8] * z_src
    ref_new = np.stack([(o[:, 6] / K[:, 0, 0] + tCR[:, 0] / z_src) * z_tgt, (o[:, 7] / K[:, 1, 1] + tCR[:, 1] / z_src) * z_tgt, z_tgt], axis=-1)
    out = TCO.copy()
    out[:, :3, :3] = dR @ TCO[:, :3, :3]
    out[:, :3, 3] = np.einsum("bij,bj->bi", dR, TCO[:, :3, 3] - tCR) + ref_new
    return out


# --------------------------------------------------------------------------- #
# error model: |got - ref| <= k * 2^-24 * S with S per row from the float64 reference
def _T_scale(T: np.ndarray) -> np.ndarray:
    """S = 1 for the rotation block and the bottom row, |t| of the row for the translation"""
    S = np.ones_like(T)
    S[..., :3, 3] = np.linalg.norm(T[..., :3, 3], axis=-1)[..., None]
    return S


def _K_scale(Kc: np.ndarray, boxes: np.ndarray) -> np.ndarray:
    """max(1, |value|) * (largest |box coordinate| / crop width): x2 - x1 is where the relative error of the crop grows"""
    amp = np.abs(boxes).max(axis=-1) / (boxes[..., 2] - boxes[..., 0])
    return np.maximum(1.0, np.abs(Kc)) * amp[..., None, None]


def _pp_scale(Kc: np.ndarray, boxes: np.ndarray, out_hw) -> np.ndarray:
    """The principal point of a crop is (out - 1) / 2 + scale * (c - box centre): two terms that can cancel (a row of 4608 had
    cy = 0.79 from 119.5 - 118.7), which max(1, |value|) does not see.  Scale of entries [0,2] and [1,2] by the terms instead:
    max(1, |first term| + |second term|) * (largest |box coordinate| / crop width)."""
    a = (np.array([max(out_hw), min(out_hw)], dtype=np.float64) - 1) / 2
    v = Kc[..., :2, 2]
    amp = np.abs(boxes).max(axis=-1) / (boxes[..., 2] - boxes[..., 0])
    return np.maximum(1.0, a + np.abs(v - a)) * amp[..., None]


PREPARE_CHECKS = PREPARE_OUTPUTS + ("K_main.focal", "K_main.pp", "KV_crop.focal", "KV_crop.pp")


def prepare_units(got: Dict[str, np.ndarray], d: Dict[str, np.ndarray], out_hw) -> Dict[str, np.ndarray]:
    """|got - ref| / (2^-24 * S) of every element of the seven outputs.  The crop intrinsics are measured three times: all nine entries
    against max(1, |value|) * amplification, the two focal lengths alone against the same scale (their floor is far lower than the
    principal point's, so their bound is tighter), and the principal point against the scale of its two terms (`_pp_scale`)."""
    one = np.ones(4)
    S = dict(TCO_n=_T_scale(d["TCO_n"]), tCR=np.linalg.norm(d["tCR"], axis=-1)[:, None] * np.ones(3), TCV_O=_T_scale(d["TCV_O"]),
             boxes_rend=np.abs(d["boxes_rend"]).max(axis=-1)[:, None] * one, boxes_crop=np.abs(d["boxes_crop"]).max(axis=-1)[:, None] * one,
             K_main=_K_scale(d["K_main"], d["boxes_crop"]), KV_crop=_K_scale(d["KV_crop"], d["boxes_crop_views"]))
    u = {n: units(got[n], d[n], S[n]) for n in PREPARE_OUTPUTS}
    for n, bx in (("K_main", "boxes_crop"), ("KV_crop", "boxes_crop_views")):
        u[n + ".focal"] = np.stack([u[n][..., 0, 0], u[n][..., 1, 1]], axis=-1)
        u[n + ".pp"] = units(f64(got[n])[..., :2, 2], d[n][..., :2, 2], _pp_scale(d[n], d[bx], out_hw))
    return u


def update_scales(ref: np.ndarray, out9, tCR) -> np.ndarray:
    """rotation entries: 1 / sin(angle of the 6D pair); translation: (|t| + |tCR|) with |t| of the updated pose, times the same 1 / sin
    since the rotation carries t - tCR"""
    inv_sin = 1.0 / ortho6d_sin(f64(out9)[:, 0:3], f64(out9)[:, 3:6])
    S = np.ones_like(ref) * inv_sin[:, None, None]
    S[:, :3, 3] = ((np.linalg.norm(ref[:, :3, 3], axis=-1) + np.linalg.norm(f64(tCR), axis=-1)) * inv_sin)[:, None]
    S[:, 3, :] = 1.0
    return S


def init_poses_scales(ref: np.ndarray, boxes, K) -> np.ndarray:
    """z of the row for z, times 1 + |u - cx| / fx (resp. v, cy, fy) for x and y; the rotation is a copy (S = 1, error 0)"""
    boxes, K = f64(boxes), f64(K)
    z = ref[:, 2, 3]
    S = np.ones_like(ref)
    S[:, 0, 3] = z * (1 + np.abs((boxes[:, 0] + boxes[:, 2]) / 2 - K[:, 0, 2]) / K[:, 0, 0])
    S[:, 1, 3] = z * (1 + np.abs((boxes[:, 1] + boxes[:, 3]) / 2 - K[:, 1, 2]) / K[:, 1, 1])
    S[:, 2, 3] = z
    return S


def units(got, ref: np.ndarray, S: np.ndarray) -> np.ndarray:
    """|got - ref| in units of 2^-24 * S, element by element (no element left out); a non-finite `got` counts as infinitely wrong"""
    got = f64(got)
    assert got.shape == ref.shape == np.broadcast_shapes(ref.shape, np.shape(S)), (got.shape, ref.shape, np.shape(S))
    u = np.abs(got - ref) / (EPS24 * S)
    return np.where(np.isfinite(got), u, np.inf)


def k_from_floor(floor: float) -> int:
    """the bound a kernel gets from the fp32 oracle's own error: 4 x the floor, rounded up to a power of two, at least 8"""
    return int(max(8, 2 ** int(np.ceil(np.log2(max(4.0 * floor, 1e-300))))))
