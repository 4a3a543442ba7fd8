"""Thin torch-tensor front-end over the C-ABI (include/mp_engine.h).

PyTorch is used for device memory and streams only; every computation below is a
call into libmp_engine.so.  All functions enqueue on torch's current HIP stream and
never synchronise.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, EngineError, Lights, MeshDesc, NamedTensor, check

RASTER_NORMALS = 1
RASTER_DEPTH = 2
RASTER_NORMALS_GL = 4
RASTER_MSAA4 = 16   # 4x multisampling = the reference renderer's configuration (panda3d_scene_renderer.py:73-74)
RASTER_F16 = 32     # "fp16 renders": the output tensor holds binary16 elements (set from `out.dtype`, never by hand)
RASTER_XREC = 64

BACKBONE_KINDS = {"vanilla_resnet34": 0, "resnet34": 1, "resnet18": 2}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dev(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """`t` as a contiguous device tensor of `dtype` (itself if it already is one)"""
    if not t.is_cuda:
        raise EngineError("engine tensors must live on the GPU")
    if t.dtype != dtype or not t.is_contiguous():
        t = t.to(dtype).contiguous()
    return t


def _dev_f32(t: torch.Tensor) -> torch.Tensor:
    return _dev(t, torch.float32)


def _dev_i32(t: torch.Tensor) -> torch.Tensor:
    return _dev(t, torch.int32)


def _workspace(n_bytes: int, device) -> torch.Tensor:
    """a launch's scratch of at least n_bytes (never empty: the entries refuse a null workspace)"""
    return torch.empty(max(int(n_bytes), 256), dtype=torch.uint8, device=device)


class _Handle:
    """Owner of one C handle: `_destroy` names the entry that frees it; it runs once, from close() or at collection."""
    _destroy = ""
    handle = None

    def close(self):
        if self.handle:
            getattr(_lib.load(), self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _named_tensors(state_dict: Dict[str, torch.Tensor]):
    """The floating-point tensors of a state dict as the mp_named_tensor array of a create call -> (array, items); the array points
    into the names and host arrays of `items`: keep that referenced until the call has returned."""
    items = [(k.encode(), np.ascontiguousarray(v.detach().cpu().numpy(), dtype=np.float32)) for k, v in state_dict.items()
             if torch.is_tensor(v) and v.dtype.is_floating_point]
    arr = (NamedTensor * len(items))()
    for i, (k, a) in enumerate(items):
        arr[i] = NamedTensor(k, a.ctypes.data, a.size)
    return arr, items


def clock_probe(ms_target: float = 20.0) -> Dict[str, float]:
    """Effective shader clock (MHz) under fp32-MFMA load and the probe loop's own TFLOP/s (synchronises; mp_clock_probe)."""
    mhz, tf = C.c_double(0), C.c_double(0)
    check(_lib.load().mp_clock_probe(float(ms_target), C.byref(mhz), C.byref(tf), _stream()))
    return {"shader_mhz": mhz.value, "mfma_tflops": tf.value}


def conv_clock(reset: bool = True) -> float:
    """Effective shader clock (MHz) inside the convolution kernels since the last reset (synchronises; mp_conv_clock_read)."""
    mhz = C.c_double(0)
    check(_lib.load().mp_conv_clock_read(C.byref(mhz), 1 if reset else 0))
    return mhz.value


def conv_wino_stats(reset: bool = True) -> Tuple[float, float]:
    """(algorithmic = direct-convolution FLOPs, FLOPs actually executed) of the Winograd launches since the last reset"""
    a, b = C.c_double(0), C.c_double(0)
    check(_lib.load().mp_conv_wino_stats(C.byref(a), C.byref(b), 1 if reset else 0))
    return a.value, b.value


_PROFILING = False


def profiling() -> bool:
    """True between profile_begin() and profile_end() (the per-launch event profiler is on: graph capture is then avoided)"""
    return _PROFILING


def profile_begin() -> None:
    global _PROFILING
    check(_lib.load().mp_profile_begin())
    _PROFILING = True


def profile_end() -> Dict[str, Dict[str, float]]:
    """Stop the per-launch event profiler and return {kernel: {launches, ms, flops, bytes, executed, peak_tflops}} (synchronises):
    flops = algorithmic work, executed = FLOPs issued on the matrix pipe whose dense peak is peak_tflops (mp_profile_query_ex)."""
    global _PROFILING
    lib = _lib.load()
    check(lib.mp_profile_end())
    _PROFILING = False
    out: Dict[str, Dict[str, float]] = {}
    i = 0
    while True:
        name = C.create_string_buffer(128)
        n, ms, fl, by, ex, pk = C.c_int64(0), C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0)
        rc = lib.mp_profile_query_ex(i, name, 128, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by), C.byref(ex), C.byref(pk))
        if rc == 1:
            break
        check(rc)
        out[name.value.decode()] = {"launches": n.value, "ms": ms.value, "flops": fl.value, "bytes": by.value, "executed": ex.value,
                                    "peak_tflops": pk.value}
        i += 1
    return out


def device_info() -> Tuple[int, int, str]:
    lib = _lib.load()
    n_cu, lds = C.c_int(0), C.c_int(0)
    name = C.create_string_buffer(64)
    check(lib.mp_device_info(C.byref(n_cu), C.byref(lds), name, 64))
    return n_cu.value, lds.value, name.value.decode()


# --------------------------------------------------------------------------- #
class MeshDB(_Handle):
    """Device-resident meshes (mp_mesh_db).  `meshes`: list of dicts with float32 arrays
    vertices [V,3] (metres), normals [V,3], colors [V,3] in [0,1], int32 faces [T,3]; optionally uvs [T,3,2] and
    texture_mips (list of uint32 [h_l, w_l] RGBA8 levels) for UV-textured objects."""
    _destroy = "mp_mesh_db_destroy"

    def __init__(self, meshes: Sequence[Dict[str, np.ndarray]]):
        lib = _lib.load()
        self._keep = []
        descs = (MeshDesc * len(meshes))()
        for i, m in enumerate(meshes):
            v = np.ascontiguousarray(m["vertices"], dtype=np.float32)
            n = np.ascontiguousarray(m["normals"], dtype=np.float32)
            c = np.ascontiguousarray(m["colors"], dtype=np.float32)
            f = np.ascontiguousarray(m["faces"], dtype=np.int32)
            assert v.shape == n.shape == c.shape and v.shape[1] == 3 and f.shape[1] == 3
            self._keep += [v, n, c, f]
            descs[i] = MeshDesc(v.ctypes.data, n.ctypes.data, c.ctypes.data, f.ctypes.data, v.shape[0], f.shape[0])
        h = C.c_void_p()
        check(lib.mp_mesh_db_create(descs, len(meshes), C.byref(h)))
        self.handle = h
        self.n = len(meshes)
        self.max_vertices = lib.mp_mesh_db_max_vertices(h)
        for i, m in enumerate(meshes):  # optional UV texture: per-corner uvs [T,3,2] + RGBA8 mip chain (mesh_io.build_mip_chain)
            if m.get("uvs") is not None and m.get("texture_mips") is not None:
                uv = np.ascontiguousarray(m["uvs"], dtype=np.float32)
                mips = m["texture_mips"]
                assert uv.shape == (np.asarray(m["faces"]).shape[0], 3, 2)
                th, tw = mips[0].shape[:2]
                flat = np.ascontiguousarray(np.concatenate([lv.reshape(-1) for lv in mips]).astype(np.uint32))
                check(lib.mp_mesh_db_set_texture(h, i, uv.ctypes.data, flat.ctypes.data, tw, th, len(mips)))
        self._keep = []
        self._ws: Dict[int, torch.Tensor] = {}

    def radius(self, i: int) -> float:
        return _lib.load().mp_mesh_db_radius(self.handle, i)

    def workspace(self, n_views: int, h: int, w: int, device, slot: int = 0) -> torch.Tensor:
        """scratch for the per-view tile lists of a launch; one per `slot` (= concurrent HIP stream)"""
        need = _lib.load().mp_raster_workspace_bytes(self.handle, n_views, h, w)
        ws = self._ws.get(slot)
        if ws is None or ws.numel() < need or ws.device != torch.device(device):
            self._ws[slot] = ws = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
        return ws


def make_lights(ambient=(1.0, 1.0, 1.0), point_dirs=(), point_colors=(), point_offsets=None) -> Lights:
    """point light i sits at dir_i * 10 * (bounding radius of the mesh) + offset_i in the object frame"""
    L = Lights()
    L.ambient[:] = ambient
    L.n_point = len(point_dirs)
    for i, (d, c) in enumerate(zip(point_dirs, point_colors)):
        L.point_dir[i][:] = d
        L.point_color[i][:] = c
        L.point_offset[i][:] = point_offsets[i] if point_offsets is not None else (0.0, 0.0, 0.0)
    return L


class PackedObservation:
    """Observation frames repacked [n_im,H,W,4] on the device (mp_pack_observation_nhwc4) for the fused crop of raster_render."""

    def __init__(self, images: torch.Tensor):
        images = _dev_f32(images)
        self.n_im, self.C, self.H, self.W = (int(v) for v in images.shape)
        self.data = torch.empty(self.n_im, self.H, self.W, 4, dtype=torch.float32, device=images.device)
        check(_lib.load().mp_pack_observation_nhwc4(images.data_ptr(), self.n_im, self.C, self.H, self.W, self.data.data_ptr(), _stream()))


def raster_render(db: MeshDB, mesh_ids: torch.Tensor, TCO: torch.Tensor, K: torch.Tensor, h: int, w: int, flags: int,
                  lights: Lights, out: torch.Tensor, stride_v: int, stride_y: int, stride_x: int, c_rgb: int, c_normals: int,
                  c_depth: int, out_offset_floats: int = 0, views_per_item: int = 1, stride_view: int = 0, slot: int = 0,
                  crop=None, xrec=None) -> None:
    """Render n views into `out` (float32 or float16 device tensor) at the given ELEMENT strides / offset; a float16 `out`
    selects MP_RASTER_F16 (values rounded to nearest-even binary16 as they are stored -- the "fp16 renders" mode).
    crop = (images [n_im,C,H,W], im_ids [n_items], boxes [n_items,4], c0): also roi_align-crop every item's observation into channels
    c0.. of its pixels in the same launch (mp_raster_render_crop).  xrec = (f32_mask, tCR, depth_mode) with a bfloat16 `out`: stem records
    of a model WITH depth channels, depth normalised in the launch (mp_raster_render_xrec)."""
    lib = _lib.load()
    n = int(TCO.shape[0])
    mesh_ids = _dev_i32(mesh_ids)
    TCO = _dev_f32(TCO)
    K = _dev_f32(K)
    assert out.dtype in (torch.float32, torch.float16, torch.bfloat16) and out.is_cuda
    es = out.element_size()
    flags = (flags | RASTER_F16) if out.dtype == torch.float16 else (flags & ~RASTER_F16)
    # a bfloat16 `out` = the stem RECORDS of the exact-piece stem convolution (MP_RASTER_XREC; strides / offset in bf16 elements)
    flags = (flags | RASTER_XREC) if out.dtype == torch.bfloat16 else (flags & ~RASTER_XREC)
    ws = db.workspace(n, h, w, out.device, slot)
    # what the three entries share, in call order (args[7] = flags); the crop forms append theirs
    args = [db.handle, mesh_ids.data_ptr(), TCO.data_ptr(), K.data_ptr(), n, h, w, flags, C.byref(lights),
            out.data_ptr() + es * out_offset_floats, stride_v, views_per_item, stride_view, stride_y, stride_x, c_rgb, c_normals, c_depth,
            ws.data_ptr(), ws.numel()]
    if crop is not None:
        images, im_ids, boxes, c0 = crop
        if isinstance(images, PackedObservation):
            nhwc4, n_im, Cc, H, W, images = 1, images.n_im, images.C, images.H, images.W, images.data
        else:
            images = _dev_f32(images)
            nhwc4 = 0
            n_im, Cc, H, W = images.shape
        im_ids, boxes = _dev_i32(im_ids), _dev_f32(boxes)
        assert boxes.shape[0] * views_per_item == n and im_ids.shape[0] == boxes.shape[0]
        args += [images.data_ptr(), nhwc4, n_im, Cc, H, W, im_ids.data_ptr(), boxes.data_ptr()]
        if xrec is not None:   # records with depth channels: (f32_mask, tCR [n_items, 3], depth mode) -> mp_raster_render_xrec
            assert out.dtype == torch.bfloat16 and c0 == 0
            f32_mask, tCR, depth_mode = xrec
            tCR = _dev_f32(tCR) if tCR is not None else None
            args[7] = flags & ~RASTER_XREC   # (the entry sets that flag itself)
            check(lib.mp_raster_render_xrec(*args, int(f32_mask) & 0xFFFFFFFF, _ptr(tCR), int(depth_mode), _stream()))
            return
        check(lib.mp_raster_render_crop(*args, c0, _stream()))
        return
    check(lib.mp_raster_render(*args, _stream()))


def lights_array(rigs: Sequence[Lights], device) -> torch.Tensor:
    """Per-object light rigs as the device array of mp_lights that raster_render_scene reads (raw bytes)."""
    arr = (Lights * max(len(rigs), 1))(*rigs)
    return torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(device)


def raster_render_scene(db: MeshDB, obj_off: Sequence[int], mesh_ids: torch.Tensor, TCO: torch.Tensor, K: torch.Tensor, radius: torch.Tensor,
                        lights: torch.Tensor, h: int, w: int, flags: int, out: Optional[torch.Tensor], stride_v: int, stride_y: int,
                        stride_x: int, c_rgb: int, c_normals: int, c_depth: int, instance: Optional[torch.Tensor] = None) -> None:
    """Render n_cams = len(obj_off) - 1 scenes (mp_raster_render_scene): camera c draws the objects obj_off[c] .. obj_off[c+1] - 1 of
    mesh_ids [n_obj] / TCO [n_obj,4,4] / lights (lights_array of n_obj object-frame rigs), with K [n_cams,3,3] and scene radius
    radius [n_cams], into the float32 `out` at the given element strides; `instance` (int32 [n_cams,h,w]) receives the object slot of
    sample 0 (-1 = background)."""
    lib = _lib.load()
    n_cams = len(obj_off) - 1
    off = (C.c_int32 * len(obj_off))(*[int(v) for v in obj_off])
    dev = K.device
    d_off = torch.tensor([int(v) for v in obj_off], dtype=torch.int32, device=dev)
    mesh_ids, TCO, K, radius = _dev_i32(mesh_ids), _dev_f32(TCO), _dev_f32(K), _dev_f32(radius)
    assert out is None or (out.dtype == torch.float32 and out.is_cuda)
    assert instance is None or (instance.dtype == torch.int32 and instance.is_cuda and instance.is_contiguous() and instance.numel() >= n_cams * h * w)
    n_obj = int(obj_off[-1])
    need = lib.mp_raster_scene_workspace_bytes(db.handle, n_obj, h, w)
    ws = _workspace(need, dev)
    check(lib.mp_raster_render_scene(db.handle, n_cams, off, d_off.data_ptr(), mesh_ids.data_ptr(), TCO.data_ptr(), K.data_ptr(),
                                     radius.data_ptr(), lights.data_ptr(), h, w, flags, _ptr(out), stride_v, stride_y, stride_x, c_rgb,
                                     c_normals, c_depth, _ptr(instance), ws.data_ptr(), ws.numel(), _stream()))


def raster_job_flags(db: MeshDB, n_views: int, h: int, w: int, device, slot: int = 0) -> int:
    """Device address of the job flags the LAST compacted raster launch on this database's workspace (`slot`) wrote: one byte per
    (item, 8x8-pixel tile), 0 = no view of the item reaches the tile (mp_raster_job_flags).  Valid on the same stream until the next
    raster launch on that slot; 0 if unavailable."""
    ws = db.workspace(n_views, h, w, device, slot)
    return int(_lib.load().mp_raster_job_flags(db.handle, ws.data_ptr(), n_views, h, w) or 0)


def crop_roi_align(images: torch.Tensor, im_ids: torch.Tensor, boxes: torch.Tensor, out_h: int, out_w: int, out: torch.Tensor,
                   stride_b: int, stride_y: int, stride_x: int, c0: int, out_offset_floats: int = 0) -> None:
    lib = _lib.load()
    images = _dev_f32(images)
    n_im, Cc, H, W = images.shape
    check(lib.mp_crop_roi_align(images.data_ptr(), n_im, Cc, H, W, _dev_i32(im_ids).data_ptr(), _dev_f32(boxes).data_ptr(),
                                int(boxes.shape[0]), out_h, out_w, out.data_ptr() + 4 * out_offset_floats, stride_b, stride_y,
                                stride_x, c0, _stream()))


def normalize_depth(x: torch.Tensor, b: int, h: int, w: int, border: int, Cp: int, channels: Sequence[int], tCR: torch.Tensor,
                    mode: int) -> None:
    lib = _lib.load()
    ch = (C.c_int32 * len(channels))(*channels)
    fn = lib.mp_normalize_depth_f16 if x.dtype == torch.float16 else lib.mp_normalize_depth
    check(fn(x.data_ptr(), b, h, w, border, Cp, ch, len(channels), _dev_f32(tCR).data_ptr(), mode, _stream()))


DEPTH_NORM_MODES = {None: 0, "none": 0, "tCR_scale": 1, "tCR_scale_clamp_center": 2, "tCR_center_clamp": 3}


# --------------------------------------------------------------------------- #
def padded_nhwc(n: int, h: int, w: int, c: int, border: int, device, slack: Optional[int] = None,
                dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Zero-initialised flat buffer holding a padded-NHWC tensor + read slack: the conv's last 32-float K chunk may run
    past the kernel window into the next padded row (its weights are zero there, the memory only has to be readable).
    dtype float16 = the half-precision CNN input of the "fp16 renders" mode (same element geometry)."""
    if slack is None:
        slack = (w + 2 * border) * c + 64
    return torch.zeros(n * (h + 2 * border) * (w + 2 * border) * c + slack, dtype=dtype, device=device)


def padded_view(buf: torch.Tensor, n: int, h: int, w: int, c: int, border: int) -> torch.Tensor:
    """[n, h, w, c] view of the interior of a padded-NHWC buffer."""
    full = buf[: n * (h + 2 * border) * (w + 2 * border) * c].view(n, h + 2 * border, w + 2 * border, c)
    return full[:, border : border + h, border : border + w, :]


def _pack_weights(entry, w_oihw: np.ndarray, scale: Optional[np.ndarray], n_out: int, dtype, *dims) -> np.ndarray:
    """What the weight packers share: `w_oihw` as a contiguous fp32 array, the optional `scale` as one (None: NULL), a blob of `n_out`
    elements of `dtype` (the size the library states) and the call entry(w, *dims, scale, blob)."""
    w = np.ascontiguousarray(w_oihw, dtype=np.float32)
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    out = np.empty(n_out, dtype=dtype)
    check(entry(w.ctypes.data, *dims, None if sc is None else sc.ctypes.data, out.ctypes.data))
    return out


def _conv_desc(x: Optional[int], N: int, H: int, W: int, Cp: int, in_border: int, Cout: int, K: int, stride: int, pad: int,
               y: Optional[int] = None, out_border: int = 0, bias=None, residual=None, relu: bool = False, y_act=None, act_scale=None,
               act_shift=None) -> ConvDesc:
    """mp_conv_desc with its input, geometry, output and epilogue groups filled (x, y: device addresses or None, the rest optional
    tensors); the weights and every other field stay zero for the caller to set."""
    d = ConvDesc()
    d.d_x, d.N, d.H, d.W, d.C, d.in_border = x, N, H, W, Cp, in_border
    d.d_bias = _ptr(bias)
    d.Cout, d.KH, d.KW, d.stride, d.pad = Cout, K, K, stride, pad
    d.d_y, d.out_border, d.d_residual, d.relu = y, out_border, _ptr(residual), int(relu)
    d.d_y_act, d.d_act_scale, d.d_act_shift = _ptr(y_act), _ptr(act_scale), _ptr(act_shift)
    return d


def conv_pack_weights(w_oihw: np.ndarray, cin_p: int, scale: Optional[np.ndarray] = None) -> np.ndarray:
    lib = _lib.load()
    Cout, Cin, KH, KW = np.shape(w_oihw)
    return _pack_weights(lib.mp_conv_pack_weights, w_oihw, scale, lib.mp_conv_packed_floats(cin_p, Cout, KH, KW), np.float32,
                         Cout, Cin, KH, KW, cin_p)


def conv2d_nhwc(x: torch.Tensor, N: int, H: int, W: int, Cp: int, in_border: int, w_packed: torch.Tensor,
                bias: Optional[torch.Tensor], Cout: int, K: int, stride: int, pad: int, y: Optional[torch.Tensor], out_border: int,
                residual: Optional[torch.Tensor] = None, relu: bool = False, y_act: Optional[torch.Tensor] = None,
                act_scale: Optional[torch.Tensor] = None, act_shift: Optional[torch.Tensor] = None,
                splitk_ws: Optional[torch.Tensor] = None) -> None:
    """`splitk_ws` (fp32 scratch): lets launches whose tile grid cannot fill the chip split the K loop (deterministic two-pass).
    A float16 `x` (same padded-NHWC geometry) selects the half-precision input path (mp_conv_desc.x_f16; Cout <= 64 only)."""
    assert x.dtype in (torch.float32, torch.float16)
    d = _conv_desc(x.data_ptr(), N, H, W, Cp, in_border, Cout, K, stride, pad, _ptr(y), out_border, bias, residual, relu, y_act, act_scale,
                   act_shift)
    d.d_w, d.x_f16 = w_packed.data_ptr(), int(x.dtype == torch.float16)
    if splitk_ws is not None:
        d.d_splitk_ws, d.splitk_ws_floats = splitk_ws.data_ptr(), splitk_ws.numel()
    check(_lib.load().mp_conv2d_nhwc(C.byref(d), _stream()))


def conv_bf16x9_pack_weights(w_oihw: np.ndarray, cin_p: int, scale: Optional[np.ndarray] = None) -> np.ndarray:
    """direct-convolution weights (scale folded as in conv_pack_weights) split into three exact bf16 pieces, MFMA fragment order
    (mp_conv_bf16x9_pack_weights); uint8 blob for conv2d_bf16x9_nhwc"""
    lib = _lib.load()
    Cout, Cin, KH, KW = np.shape(w_oihw)
    return _pack_weights(lib.mp_conv_bf16x9_pack_weights, w_oihw, scale, lib.mp_conv_bf16x9_packed_bytes(cin_p, Cout, KH, KW), np.uint8,
                         Cout, Cin, KH, KW, cin_p)


def conv2d_bf16x9_nhwc(x: torch.Tensor, N: int, H: int, W: int, Cp: int, in_border: int, w_pieces: torch.Tensor,
                       bias: Optional[torch.Tensor], Cout: int, K: int, stride: int, pad: int, y: Optional[torch.Tensor], out_border: int,
                       residual: Optional[torch.Tensor] = None, relu: bool = False, y_act: Optional[torch.Tensor] = None,
                       act_scale: Optional[torch.Tensor] = None, act_shift: Optional[torch.Tensor] = None) -> None:
    """conv2d_nhwc on the bf16 MFMA through exact operand pieces (mp_conv2d_bf16x9_nhwc): always one single-pass launch;
    `w_pieces` = conv_bf16x9_pack_weights(...) on the device.  Needs Cp % 16 == 0 and K * Cp % 32 == 0."""
    d = _conv_desc(x.data_ptr(), N, H, W, Cp, in_border, Cout, K, stride, pad, _ptr(y), out_border, bias, residual, relu, y_act, act_scale,
                   act_shift)
    d.d_w = w_pieces.data_ptr()
    check(_lib.load().mp_conv2d_bf16x9_nhwc(C.byref(d), w_pieces.data_ptr(), _stream()))


def conv_wino_pack_weights(w_oihw: np.ndarray, cin_p: int, scale: Optional[np.ndarray] = None) -> np.ndarray:
    """Winograd-transformed weights U = G g G^T of a 3x3 layer in MFMA fragment order (mp_conv_wino_pack_weights)"""
    lib = _lib.load()
    Cout, Cin, KH, KW = np.shape(w_oihw)
    assert KH == 3 and KW == 3
    return _pack_weights(lib.mp_conv_wino_pack_weights, w_oihw, scale, lib.mp_conv_wino_packed_floats(cin_p, Cout), np.float32,
                         Cout, Cin, cin_p)


def conv3x3_wino_nhwc(x: torch.Tensor, N: int, H: int, W: int, Cp: int, in_border: int, u_packed: torch.Tensor,
                      bias: Optional[torch.Tensor], Cout: int, y: Optional[torch.Tensor], out_border: int,
                      residual: Optional[torch.Tensor] = None, relu: bool = False, y_act: Optional[torch.Tensor] = None,
                      act_scale: Optional[torch.Tensor] = None, act_shift: Optional[torch.Tensor] = None) -> None:
    """Fused Winograd F(2x2, 3x3) form of a 3x3 / stride-1 / pad-1 convolution (mp_conv3x3_wino_nhwc).  `x` must carry
    (W + 2 * in_border + 1) * Cp floats of readable slack behind the tensor when H or W is odd."""
    d = _conv_desc(x.data_ptr(), N, H, W, Cp, in_border, Cout, 3, 1, 1, _ptr(y), out_border, bias, residual, relu, y_act, act_scale,
                   act_shift)   # (d_w stays unset: the transformed weights are an argument of their own)
    if u_packed.dtype == torch.uint8:   # the three-bf16-piece blob: the exact-piece kernel (mp_conv3x3_wino_bf16_nhwc)
        check(_lib.load().mp_conv3x3_wino_bf16_nhwc(C.byref(d), u_packed.data_ptr(), _stream()))
        return
    check(_lib.load().mp_conv3x3_wino_nhwc(C.byref(d), u_packed.data_ptr(), _stream()))


def conv_wino_eligible(N: int, H: int, W: int, Cp: int, in_border: int, Cout: int, out_border: int, n_cu: int) -> bool:
    """True if the backbone would run this 3x3 / stride-1 / pad-1 layer on a Winograd kernel (mp_conv_wino_eligible): channel counts
    that tile, tensors small enough for 32-bit byte offsets, and a grid of at least a quarter of `n_cu` workgroups"""
    d = _conv_desc(None, N, H, W, Cp, in_border, Cout, 3, 1, 1, None, out_border)
    return bool(_lib.load().mp_conv_wino_eligible(C.byref(d), n_cu))


def conv_wino_bf16_pack_weights(w_oihw: np.ndarray, cin_p: int, scale: Optional[np.ndarray] = None) -> np.ndarray:
    """U = G g G^T of a 3x3 layer split into three exact bf16 pieces, MFMA fragment order (mp_conv_wino_bf16_pack_weights); uint8 blob"""
    lib = _lib.load()
    Cout, Cin, KH, KW = np.shape(w_oihw)
    assert KH == 3 and KW == 3
    return _pack_weights(lib.mp_conv_wino_bf16_pack_weights, w_oihw, scale, lib.mp_conv_wino_bf16_packed_bytes(cin_p, Cout), np.uint8,
                         Cout, Cin, cin_p)


def conv_wino_bf16_telemetry(on: bool) -> bool:
    """in-kernel clock telemetry of the bf16 Winograd kernel (every 64th workgroup, six global atomics): off by default; returns the
    previous setting (mp_conv_wino_bf16_telemetry)"""
    return bool(_lib.load().mp_conv_wino_bf16_telemetry(int(bool(on))))


def conv_wino_bf16_stats(reset: bool = True) -> Tuple[float, float]:
    """(algorithmic = direct-convolution FLOPs, executed bf16 FLOPs) of the bf16x9 Winograd launches since the last reset"""
    a, b = C.c_double(0), C.c_double(0)
    check(_lib.load().mp_conv_wino_bf16_stats(C.byref(a), C.byref(b), 1 if reset else 0))
    return a.value, b.value


def conv_wino_bf16_clock(reset: bool = True) -> Tuple[float, float]:
    """(effective shader clock in MHz, shader cycles per 16-channel step) inside the K loops of the bf16x9 Winograd launches"""
    a, b = C.c_double(0), C.c_double(0)
    check(_lib.load().mp_conv_wino_bf16_clock(C.byref(a), C.byref(b), 1 if reset else 0))
    return a.value, b.value


def leading_mask(n_f32: int) -> int:
    """fp32-kind channel mask of a record whose first `n_f32` channels are the fp32-kind ones"""
    return (1 << int(n_f32)) - 1


def conv_stem_pack_weights(w_oihw: np.ndarray, n_f32: int, scale: Optional[np.ndarray] = None, f32_mask: Optional[int] = None) -> np.ndarray:
    """three exact bf16 pieces of every stem weight (BN scale and, for the integer channels, 1/255 folded in) in MFMA fragment order
    (mp_conv_stem_pack_weights_mask); the first `n_f32` input channels -- or, with `f32_mask`, the channels whose bit is set -- are
    fp32-kind, the others 8-bit integers.  Returns a uint8 blob."""
    lib = _lib.load()
    Cout, Cin, KH, KW = np.shape(w_oihw)
    assert KH == KW
    mask = leading_mask(n_f32) if f32_mask is None else int(f32_mask)
    nf = bin(mask).count("1")
    return _pack_weights(lib.mp_conv_stem_pack_weights_mask, w_oihw, scale, lib.mp_conv_stem_packed_bytes(KH, nf, Cin - nf, Cout), np.uint8,
                         Cout, Cin, KH, mask)


def xrec_elements(n_f32: int, n_u8: int) -> int:
    return int(_lib.load().mp_xrec_elements(n_f32, n_u8))


def conv_stem_pack_weights_sparse(w_oihw: np.ndarray, n_f32: int, scale: Optional[np.ndarray] = None) -> Optional[np.ndarray]:
    """the piece blob of the stem's BACKGROUND-TILE walk (only the record chunks that hold fp32-kind pieces; mp_conv_stem_pack_weights_sparse);
    None if this record has no such form (nothing to skip)"""
    lib = _lib.load()
    Cout, Cin, KH, KW = np.shape(w_oihw)
    n = lib.mp_conv_stem_sparse_packed_bytes(KH, n_f32, Cin - n_f32, Cout)
    if n == 0:
        return None
    return _pack_weights(lib.mp_conv_stem_pack_weights_sparse, w_oihw, scale, n, np.uint8, Cout, Cin, KH, n_f32)


def conv_stem_tail_forms(K: int, n_f32: int, n_u8: int) -> int:
    """which walks of this record have a tail-plane form (mp_conv_stem_tail_forms): bit 0 the dense walk, bit 1 the background walk"""
    return int(_lib.load().mp_conv_stem_tail_forms(K, n_f32, n_u8))


def conv_stem_pack_weights_tail(w_oihw: np.ndarray, n_f32: int, scale: Optional[np.ndarray] = None, background: bool = False,
                                f32_mask: Optional[int] = None) -> Optional[np.ndarray]:
    """the piece blob of the stem's tail-plane walk (mp_conv_stem_pack_weights_tail): the dense walk's, or with `background` the
    background-tile walk's; None if this record has no such form"""
    lib = _lib.load()
    Cout, Cin, KH, KW = np.shape(w_oihw)
    mask = leading_mask(n_f32) if f32_mask is None else int(f32_mask)
    nf = bin(mask).count("1")
    n = lib.mp_conv_stem_tail_packed_bytes(KH, nf, Cin - nf, Cout, int(background))
    if n == 0:
        return None
    return _pack_weights(lib.mp_conv_stem_pack_weights_tail, w_oihw, scale, n, np.uint8, Cout, Cin, KH, mask, int(background))


def conv_stem_bg_stats(reset: bool = True) -> Tuple[float, float]:
    """(workgroups that took the background-tile walk, all workgroups of such launches) counted while the event profiler was active"""
    a, b = C.c_double(), C.c_double()
    check(_lib.load().mp_conv_stem_bg_stats(C.byref(a), C.byref(b), int(reset)))
    return a.value, b.value


def conv_stem_xrec(xrec: torch.Tensor, N: int, H: int, W: int, c_real: int, n_f32: int, in_border: int, w_pieces: torch.Tensor,
                   bias: Optional[torch.Tensor], Cout: int, K: int, pad: int, y: Optional[torch.Tensor], out_border: int, relu: bool = False,
                   y_pool: Optional[torch.Tensor] = None, pool_border: int = 1, w_sparse: Optional[torch.Tensor] = None,
                   tile_flags: Optional[torch.Tensor] = None, tail_forms: int = 0) -> None:
    """stride-2 stem convolution of a bfloat16 record tensor (mp_conv_stem_xrec); with `y_pool` the 3x3 / stride-2 / pad-1 max pool of its
    output is written too (mp_conv_stem_xrec_pool; `y` may then be None); with `w_sparse` + `tile_flags` (uint8 [N, ceil(H/8), ceil(W/8)],
    0 = the tile's integer channels are all 0) workgroups over background take the short walk (mp_conv_stem_xrec_sparse); with
    `tail_forms` bit 0 / bit 1 says that `w_pieces` / `w_sparse` is the blob of a tail-plane walk (mp_conv_stem_xrec_tail)"""
    assert xrec.dtype == torch.bfloat16 and w_pieces.dtype == torch.uint8
    d = _conv_desc(xrec.data_ptr(), N, H, W, (c_real + 3) // 4 * 4, in_border, Cout, K, 2, pad, _ptr(y), out_border, bias, relu=relu)
    d.c_real = c_real
    if tail_forms:
        sp = w_sparse is not None and tile_flags is not None
        assert not sp or (tile_flags.dtype == torch.uint8 and tile_flags.is_cuda and w_sparse.dtype == torch.uint8)
        check(_lib.load().mp_conv_stem_xrec_tail(C.byref(d), w_pieces.data_ptr(), w_sparse.data_ptr() if sp else None, n_f32,
                                                 tile_flags.data_ptr() if sp else None, _ptr(y_pool), pool_border, int(tail_forms), _stream()))
        return
    if w_sparse is not None and tile_flags is not None:
        assert tile_flags.dtype == torch.uint8 and tile_flags.is_cuda and w_sparse.dtype == torch.uint8
        check(_lib.load().mp_conv_stem_xrec_sparse(C.byref(d), w_pieces.data_ptr(), w_sparse.data_ptr(), n_f32, tile_flags.data_ptr(),
                                                   _ptr(y_pool), pool_border, _stream()))
        return
    if y_pool is not None:
        check(_lib.load().mp_conv_stem_xrec_pool(C.byref(d), w_pieces.data_ptr(), n_f32, y_pool.data_ptr(), pool_border, _stream()))
        return
    check(_lib.load().mp_conv_stem_xrec(C.byref(d), w_pieces.data_ptr(), n_f32, _stream()))


def conv2d_plan(N: int, H: int, W: int, Cp: int, in_border: int, Cout: int, K: int, stride: int, pad: int, n_cu: int,
                ws_floats: int = 0, x_f16: bool = False) -> Dict[str, int]:
    """How mp_conv2d_nhwc would lay this launch out on `n_cu` CUs (host-only, no GPU work): mode 0 single pass, 1 every tile
    split along K, 2 full rounds + split-K tail (half-precision inputs always run single pass)."""
    dummy = 0x1000  # the planner only tests pointers for NULL
    d = _conv_desc(dummy, N, H, W, Cp, in_border, Cout, K, stride, pad, dummy, 1)
    d.d_w, d.x_f16 = dummy, int(x_f16)
    if ws_floats:
        d.d_splitk_ws, d.splitk_ws_floats = dummy, ws_floats
    out = (C.c_int32 * 5)()
    check(_lib.load().mp_conv2d_plan(C.byref(d), n_cu, out))
    return dict(zip(("mode", "k_split", "chunks_per_split", "n_main", "m_begin"), out))


def maxpool3x3s2(x, N, H, W, Cc, in_border, y, out_border, y_act=None, sc=None, sh=None) -> None:
    check(_lib.load().mp_maxpool3x3s2(x.data_ptr(), N, H, W, Cc, in_border, _ptr(y), out_border, _ptr(y_act), _ptr(sc), _ptr(sh),
                                      _stream()))


def bn_relu_nhwc(x, N, H, W, Cc, border, y_act, sc, sh) -> None:
    """y_act = relu(x * sc[c] + sh[c]) on the interior of a padded NHWC map (mp_bn_relu_nhwc: the WideResNets' first pre-activation
    behind the stem's fused max pool)"""
    check(_lib.load().mp_bn_relu_nhwc(x.data_ptr(), N, H, W, Cc, border, y_act.data_ptr(), sc.data_ptr(), sh.data_ptr(), _stream()))


def pool_fc_heads(x, N, H, W, Cc, in_border, fc_w, fc_b, n_feat, head_w, head_b, n_out, feat, out, sigmoid) -> None:
    check(_lib.load().mp_pool_fc_heads(x.data_ptr(), N, H, W, Cc, in_border, _ptr(fc_w), _ptr(fc_b), n_feat, head_w.data_ptr(),
                                       head_b.data_ptr(), n_out, _ptr(feat), out.data_ptr(), _ptr(sigmoid), _stream()))


class Backbone(_Handle):
    """mp_backbone: whole CNN + head resident on the device, one call per forward."""
    _destroy = "mp_backbone_destroy"

    def __init__(self, kind: str, c_in: int, head: str, n_out: int, state_dict: Dict[str, torch.Tensor]):
        lib = _lib.load()
        width = 1
        if kind.startswith("resnet34_width="):   # training/pose_models_cfg.py:114-116: WideResNet34(width=int(...))
            width, kind = int(kind.split("resnet34_width=")[1]), "resnet34"
        if kind not in BACKBONE_KINDS:
            raise EngineError(f"unknown backbone '{kind}' (pose_models_cfg.py:106-118 supports {list(BACKBONE_KINDS)} and resnet34_width=N)")
        self.width = width
        arr, items = _named_tensors(state_dict)   # (`items` owns what `arr` points into)
        h = C.c_void_p()
        check(lib.mp_backbone_create_wide(BACKBONE_KINDS[kind], width, c_in, 0 if head == "pose" else 1, n_out, arr, len(items), C.byref(h)))
        self.handle = h
        self.kind, self.c_in, self.n_out = kind, c_in, n_out
        self.c_in_p = lib.mp_backbone_input_channels_padded(h)
        self.in_border = lib.mp_backbone_input_border(h)
        self._ws: Dict[int, torch.Tensor] = {}
        self._xrec_len: Dict[int, int] = {}   # fp32-kind channel mask -> record length of the prepared stem blob (0: no exact-piece form)

    def workspace(self, batch: int, h: int, w: int, device, slot: int = 0) -> torch.Tensor:
        need = _lib.load().mp_backbone_workspace_bytes(self.handle, batch, h, w)
        ws = self._ws.get(slot)
        if ws is None or ws.numel() < need or ws.device != torch.device(device):
            self._ws.pop(slot, None)
            self._ws[slot] = ws = torch.empty(need, dtype=torch.uint8, device=device)
            # a NEW allocation: its borders are not zero even if the executor has seen this address before
            check(_lib.load().mp_backbone_workspace_reset(self.handle, ws.data_ptr()))
        return ws

    def flops(self, batch: int, h: int, w: int) -> float:
        return _lib.load().mp_backbone_flops(self.handle, batch, h, w)

    def xrec_elements(self, n_f32: int = 3, f32_mask: Optional[int] = None) -> int:
        """Record length (bf16 elements per pixel) of the exact-piece stem input whose fp32-kind channels are the first `n_f32` (the
        observation crop) or the set bits of `f32_mask` (crop + depth channels of an RGBD model), all other input channels being 8-bit
        integers (renders); 0 = this stem has no such form.  This is also the PREPARE step (mp_backbone_xrec_prepare): the first call for
        a mask packs and uploads the stem's piece blob -- host work and a synchronous copy, so call it outside stream capture; `forward`
        only looks the blob up."""
        mask = leading_mask(n_f32) if f32_mask is None else int(f32_mask)
        if mask >> 32 or (self.c_in < 32 and mask >> self.c_in):
            return 0
        hit = self._xrec_len.get(mask)
        if hit is None:
            hit = self._xrec_len[mask] = int(_lib.load().mp_backbone_xrec_prepare(self.handle, mask))
        return hit

    def forward(self, x: torch.Tensor, batch: int, h: int, w: int, out: torch.Tensor, sigmoid: Optional[torch.Tensor] = None,
                feat: Optional[torch.Tensor] = None, slot: int = 0, n_f32: int = 3, f32_mask: Optional[int] = None,
                tile_flags: int = 0) -> None:
        """x: fp32 padded NHWC | float16 (same geometry, mp_backbone_forward_f16) | bfloat16 stem records whose fp32-kind channels are
        the first `n_f32` / the bits of `f32_mask` (what the rasteriser writes with MP_RASTER_XREC; mp_backbone_forward_xrec_mask).
        `tile_flags` = device address of the job flags of the raster launch that wrote the records (`raster_job_flags`): the stem takes
        the background-tile walk where it applies (mp_backbone_forward_xrec_sparse)."""
        ws = self.workspace(batch, h, w, x.device, slot)
        assert x.dtype in (torch.float32, torch.float16, torch.bfloat16)
        lib = _lib.load()
        if x.dtype == torch.bfloat16:
            mask = leading_mask(n_f32) if f32_mask is None else int(f32_mask)
            self.xrec_elements(f32_mask=mask)   # (prepared on first use; the C forward never allocates)
            if tile_flags:
                check(lib.mp_backbone_forward_xrec_sparse(self.handle, x.data_ptr(), mask & 0xFFFFFFFF, tile_flags, batch, h, w, out.data_ptr(),
                                                          _ptr(sigmoid), _ptr(feat), ws.data_ptr(), ws.numel(), _stream()))
                return
            check(lib.mp_backbone_forward_xrec_mask(self.handle, x.data_ptr(), mask & 0xFFFFFFFF, batch, h, w, out.data_ptr(), _ptr(sigmoid),
                                                    _ptr(feat), ws.data_ptr(), ws.numel(), _stream()))
            return
        fn = lib.mp_backbone_forward_f16 if x.dtype == torch.float16 else lib.mp_backbone_forward
        check(fn(self.handle, x.data_ptr(), batch, h, w, out.data_ptr(), _ptr(sigmoid), _ptr(feat), ws.data_ptr(), ws.numel(), _stream()))

    def debug_buffer(self, what: str, batch: int, h: int, w: int, slot: int = 0):
        """the WHOLE padded buffer behind a tap of the last forward on `slot` (which must have been one of batch x h x w) ->
        (flat float32 tensor, [n, h, w, c] of the interior, border).  A VIEW of the workspace: the next forward overwrites it."""
        ws = self._ws.get(slot)
        if ws is None:
            raise EngineError(f"debug tap '{what}': no forward has run on workspace slot {slot}")
        ptr, shp, border = C.c_void_p(), (C.c_int64 * 4)(), C.c_int32(0)
        check(_lib.load().mp_backbone_debug_tensor(self.handle, what.encode(), ws.data_ptr(), batch, h, w, C.byref(ptr), shp, C.byref(border)))
        n, hh, ww, c = (int(v) for v in shp)
        b = border.value
        off, n_bytes = ptr.value - ws.data_ptr(), 4 * n * (hh + 2 * b) * (ww + 2 * b) * c
        if off < 0 or off + n_bytes > ws.numel():
            raise EngineError(f"debug tap '{what}' lies outside the workspace of the last forward")
        return ws[off : off + n_bytes].view(torch.float32), [n, hh, ww, c], b

    def debug_tensor(self, what: str, batch: int, h: int, w: int, slot: int = 0) -> torch.Tensor:
        """a COPY of the [n, h, w, c] interior of an intermediate of the last forward (parity tests).  Taps: "stem" (not on the record path),
        "layer1".."layer4", "layer1_act".."layer3_act" (pre-activation nets), "layer2_down".."layer4_down" (mp_backbone_debug_tensor in
        include/mp_engine_debug.h)"""
        flat, s, b = self.debug_buffer(what, batch, h, w, slot)
        return flat.view(s[0], s[1] + 2 * b, s[2] + 2 * b, s[3])[:, b : b + s[1], b : b + s[2]].clone()


# --------------------------------------------------------------------------- #
def normalize_T(T: torch.Tensor) -> torch.Tensor:
    T = _dev_f32(T)
    out = torch.empty_like(T)
    check(_lib.load().mp_normalize_T(T.data_ptr(), T.shape[0], out.data_ptr(), _stream()))
    return out


def init_extents(points: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
    points, R = _dev_f32(points), _dev_f32(R)
    n_mesh, n_pts, _ = points.shape
    ext = torch.empty(n_mesh, R.shape[0], 2, dtype=torch.float32, device=points.device)
    check(_lib.load().mp_init_extents(points.data_ptr(), n_mesh, n_pts, R.data_ptr(), R.shape[0], ext.data_ptr(), _stream()))
    return ext


def init_poses_from_boxes(boxes, K, mesh_ids, rot_ids, R, ext) -> torch.Tensor:
    boxes, K, R, ext = _dev_f32(boxes), _dev_f32(K), _dev_f32(R), _dev_f32(ext)
    b = boxes.shape[0]
    TCO = torch.empty(b, 4, 4, dtype=torch.float32, device=boxes.device)
    check(_lib.load().mp_init_poses_from_boxes(boxes.data_ptr(), K.data_ptr(), _dev_i32(mesh_ids).data_ptr(),
                                               _dev_i32(rot_ids).data_ptr(), R.data_ptr(), R.shape[0], ext.data_ptr(), b,
                                               TCO.data_ptr(), _stream()))
    return TCO


MV_MODES = {"TCO": 0, "1view_TCO": 0, "TCO+front_3views": 1, "TCO+front_1view": 2, "sphere_26views": 3}
MV_REMOVE_TCO, MV_INPLANE = 256, 512


def multiview_n_views(multiview: int) -> int:
    return int(_lib.load().mp_pose_multiview_n_views(int(multiview)))


def pose_prepare(TCO_in, K, mesh_ids, points, n_pts_main: int, n_pts_views: int, V: int, multiview: int, im_hw, out_hw,
                 lamb: float = 1.4, with_K_main: bool = False):
    """-> (TCO_n, tCR, TCV_O [b,V,4,4], KV_crop [b,V,3,3], boxes_rend, boxes_crop[, K_main [b,3,3]]); `multiview` = MV_MODES code
    | MV_REMOVE_TCO | MV_INPLANE (mp_pose_prepare_ex)."""
    TCO_in, K, points = _dev_f32(TCO_in), _dev_f32(K), _dev_f32(points)
    b = TCO_in.shape[0]
    dev = TCO_in.device
    f = dict(dtype=torch.float32, device=dev)
    TCO_n = torch.empty(b, 4, 4, **f)
    tCR = torch.empty(b, 3, **f)
    TCV_O = torch.empty(b, V, 4, 4, **f)
    KV = torch.empty(b, V, 3, 3, **f)
    boxes_rend = torch.empty(b, 4, **f)
    boxes_crop = torch.empty(b, 4, **f)
    K_main = torch.empty(b, 3, 3, **f) if with_K_main else None
    check(_lib.load().mp_pose_prepare_ex(TCO_in.data_ptr(), K.data_ptr(), _dev_i32(mesh_ids).data_ptr(), points.data_ptr(),
                                         points.shape[1], n_pts_main, n_pts_views, b, V, multiview, im_hw[0], im_hw[1], out_hw[0],
                                         out_hw[1], lamb, TCO_n.data_ptr(), tCR.data_ptr(), TCV_O.data_ptr(), KV.data_ptr(),
                                         boxes_rend.data_ptr(), boxes_crop.data_ptr(), _ptr(K_main), _stream()))
    if with_K_main:
        return TCO_n, tCR, TCV_O, KV, boxes_rend, boxes_crop, K_main
    return TCO_n, tCR, TCV_O, KV, boxes_rend, boxes_crop


def pose_update(TCO, K_crop, out9, tCR, k_stride_floats: int = 9) -> torch.Tensor:
    TCO, out9, tCR = _dev_f32(TCO), _dev_f32(out9), _dev_f32(tCR)
    assert K_crop.dtype == torch.float32 and K_crop.is_cuda
    out = torch.empty_like(TCO)
    check(_lib.load().mp_pose_update(TCO.data_ptr(), K_crop.data_ptr(), k_stride_floats, out9.data_ptr(), tCR.data_ptr(),
                                     TCO.shape[0], out.data_ptr(), _stream()))
    return out


# --------------------------------------------------------------------------- #
# pose errors (evaluation): csrc/pose_error.hip
POSE_ERROR_MEAN, POSE_ERROR_MAX = 0, 1


def _pose_error_points(points: torch.Tensor, mesh_ids, n_points, b: int):
    points = _dev_f32(points)
    if points.dim() != 3 or points.shape[-1] != 3 or points.shape[1] < 1:
        raise EngineError(f"points must be [n_mesh, n_pts >= 1, 3], got {tuple(points.shape)}")
    if mesh_ids is None:
        if points.shape[0] != b:
            raise EngineError("without mesh ids the points are per row: [b, n_pts, 3]")
        mesh_ids = torch.arange(b, dtype=torch.int32, device=points.device)
    return points, _dev_i32(mesh_ids), (None if n_points is None else _dev_i32(n_points))


def pose_error_workspace(b: int, n_pts: int, S_max: int, device) -> torch.Tensor:
    return _workspace(_lib.load().mp_pose_error_workspace_bytes(b, n_pts, S_max), device)


def _pose_error_sym_set(entry, T_pred, T_gt, symmetries, n_sym, points, mesh_ids, n_points, reduce, split, with_errs, with_alt,
                        K=None, with_diffs=None) -> Dict[str, torch.Tensor]:
    """what mp_pose_error_sym and mp_pose_error_mspd (`entry`) share: checks, outputs, workspace.  K: only the projected entry takes it;
    with_diffs: only the 3D entry has the argument (None = it has not)."""
    T_pred, T_gt = _dev_f32(T_pred), _dev_f32(T_gt)
    b = T_pred.shape[0]
    if K is not None:
        K = _dev_f32(K)
        if K.shape != (b, 3, 3):
            raise EngineError(f"K must be [b,3,3], got {tuple(K.shape)}")
    points, mesh_ids, n_points = _pose_error_points(points, mesh_ids, n_points, b)
    if symmetries is not None:
        symmetries = _dev_f32(symmetries)
        S = symmetries.shape[1]
        if T_gt.shape != (b, 4, 4):
            raise EngineError(f"T_gt must be [b,4,4], got {tuple(T_gt.shape)}")
    else:
        if T_gt.dim() != 4 or T_gt.shape[0] != b:
            raise EngineError(f"candidate poses must be [b,S,4,4], got {tuple(T_gt.shape)}")
        S = T_gt.shape[1]
    n_sym = None if symmetries is None or n_sym is None else _dev_i32(n_sym)
    n_pts = points.shape[1]
    dev = T_pred.device
    f = dict(dtype=torch.float32, device=dev)
    out = dict(err=torch.empty(b, **f), idx=torch.empty(b, dtype=torch.int32, device=dev), T_gt_sym=torch.empty(b, 4, 4, **f))
    if with_errs:
        out["errs"] = torch.empty(b, S, **f)
    if with_diffs:
        out["diffs"] = torch.empty(b, n_pts, 3, **f)
    if with_alt:
        out["err_alt"] = torch.empty(b, **f)
    ws = pose_error_workspace(b, n_pts, S, dev)
    # the two signatures differ in one argument each: K before the outputs, diffs after them
    check(entry(T_pred.data_ptr(), T_gt.data_ptr(), _ptr(symmetries), _ptr(n_sym), S, points.data_ptr(), n_pts, mesh_ids.data_ptr(),
                _ptr(n_points), n_pts, b, int(reduce), int(split), *([] if K is None else [K.data_ptr()]), out["err"].data_ptr(),
                _ptr(out.get("err_alt")), out["idx"].data_ptr(), out["T_gt_sym"].data_ptr(), _ptr(out.get("errs")),
                *([] if with_diffs is None else [_ptr(out.get("diffs"))]), ws.data_ptr(), ws.numel(), _stream()))
    return out


def pose_error_sym(T_pred: torch.Tensor, T_gt: torch.Tensor, symmetries: Optional[torch.Tensor], n_sym: Optional[torch.Tensor],
                   points: torch.Tensor, mesh_ids: Optional[torch.Tensor] = None, n_points: Optional[torch.Tensor] = None,
                   reduce: int = POSE_ERROR_MEAN, split: int = 0, with_errs: bool = True, with_diffs: bool = False,
                   with_alt: bool = False) -> Dict[str, torch.Tensor]:
    """Symmetry-set error (mp_pose_error_sym).  `symmetries` [n_mesh,S,4,4] + `n_sym` [n_mesh]: T_gt [b,4,4] is composed with them;
    `symmetries` None: T_gt holds the candidates [b,S,4,4].  -> err, idx, T_gt_sym (+ errs [b,S], diffs [b,N,3], err_alt)."""
    return _pose_error_sym_set(_lib.load().mp_pose_error_sym, T_pred, T_gt, symmetries, n_sym, points, mesh_ids, n_points, reduce, split,
                               with_errs, with_alt, with_diffs=bool(with_diffs))


def pose_error_nn(T_pred: torch.Tensor, T_gt: torch.Tensor, points: torch.Tensor, mesh_ids: Optional[torch.Tensor] = None,
                  n_points: Optional[torch.Tensor] = None, split: int = 0, with_diffs: bool = True,
                  with_assign: bool = True) -> Dict[str, torch.Tensor]:
    """Nearest-neighbour error (mp_pose_error_nn) -> mean, max [b] (+ diffs [b,N,3], assign [b,N] int32)."""
    T_pred, T_gt = _dev_f32(T_pred), _dev_f32(T_gt)
    b = T_pred.shape[0]
    points, mesh_ids, n_points = _pose_error_points(points, mesh_ids, n_points, b)
    n_pts = points.shape[1]
    dev = T_pred.device
    f = dict(dtype=torch.float32, device=dev)
    out = dict(mean=torch.empty(b, **f), max=torch.empty(b, **f))
    if with_diffs:
        out["diffs"] = torch.empty(b, n_pts, 3, **f)
    if with_assign:
        out["assign"] = torch.empty(b, n_pts, dtype=torch.int32, device=dev)
    ws = pose_error_workspace(b, n_pts, 1, dev)
    check(_lib.load().mp_pose_error_nn(T_pred.data_ptr(), T_gt.data_ptr(), points.data_ptr(), n_pts, mesh_ids.data_ptr(), _ptr(n_points),
                                       n_pts, b, int(split), _ptr(out.get("diffs")), _ptr(out.get("assign")), out["mean"].data_ptr(),
                                       out["max"].data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return out


def pose_error_rigid(T_a: torch.Tensor, T_b: torch.Tensor, K: Optional[torch.Tensor] = None, points: Optional[torch.Tensor] = None,
                     mesh_ids: Optional[torch.Tensor] = None, n_points: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """trans_err = |t_a - t_b|, rot_err_deg = angle of R_b R_a^T (+ proj_error with K and points): mp_pose_error_rigid."""
    T_a, T_b = _dev_f32(T_a), _dev_f32(T_b)
    b = T_a.shape[0]
    f = dict(dtype=torch.float32, device=T_a.device)
    out = dict(trans_err=torch.empty(b, **f), rot_err_deg=torch.empty(b, **f))
    n_pts = 0
    if K is not None:
        K = _dev_f32(K)
        points, mesh_ids, n_points = _pose_error_points(points, mesh_ids, n_points, b)
        n_pts = points.shape[1]
        out["proj_error"] = torch.empty(b, **f)
    check(_lib.load().mp_pose_error_rigid(T_a.data_ptr(), T_b.data_ptr(), b, _ptr(K), _ptr(points) if K is not None else None,
                                          n_pts, _ptr(mesh_ids) if K is not None else None, _ptr(n_points) if K is not None else None, n_pts,
                                          out["trans_err"].data_ptr(), out["rot_err_deg"].data_ptr(), _ptr(out.get("proj_error")), _stream()))
    return out


def pose_error_mspd(T_pred: torch.Tensor, T_gt: torch.Tensor, symmetries: Optional[torch.Tensor], n_sym: Optional[torch.Tensor],
                    points: torch.Tensor, K: torch.Tensor, mesh_ids: Optional[torch.Tensor] = None, n_points: Optional[torch.Tensor] = None,
                    reduce: int = POSE_ERROR_MAX, split: int = 0, with_errs: bool = True, with_alt: bool = False) -> Dict[str, torch.Tensor]:
    """Projected symmetry-set error (mp_pose_error_mspd; reduce = max is BOP's MSPD, in pixels).  Arguments as `pose_error_sym` plus
    K [b,3,3] -> err, idx, T_gt_sym (+ errs [b,S], err_alt)."""
    return _pose_error_sym_set(_lib.load().mp_pose_error_mspd, T_pred, T_gt, symmetries, n_sym, points, mesh_ids, n_points, reduce, split,
                               with_errs, with_alt, K=K)


def _row_ids(name: str, ids: Optional[torch.Tensor], maps: torch.Tensor, b: int) -> Optional[torch.Tensor]:
    """the optional map index of each of b rows: None needs one map per row, else int32 [b] on the device"""
    if ids is None:
        if maps.shape[0] < b:
            raise EngineError(f"without {name} the maps are per row: need {b}, got {maps.shape[0]}")
        return None
    ids = _dev_i32(ids)
    if ids.shape != (b,):
        raise EngineError(f"{name} must be [b], got {tuple(ids.shape)}")
    return ids


# --------------------------------------------------------------------------- #
# visible surface discrepancy (evaluation): csrc/vsd.hip
VSD_TAUS = tuple(0.05 * k for k in range(1, 11))


def vsd(depth_est: torch.Tensor, depth_gt: torch.Tensor, depth_test: torch.Tensor, K: torch.Tensor, diameter: torch.Tensor,
        delta: float = 0.015, taus=None, normalized_by_diameter: bool = True, est_ids: Optional[torch.Tensor] = None,
        gt_ids: Optional[torch.Tensor] = None, im_ids: Optional[torch.Tensor] = None, split: int = 0,
        with_counts: bool = True) -> Dict[str, torch.Tensor]:
    """BOP 2019 VSD (mp_vsd).  depth_* [n,h,w] metres; row i compares depth_est[est_ids[i]] with depth_gt[gt_ids[i]] under
    depth_test[im_ids[i]] (ids None: map i); K [b,3,3], diameter [b] -> errs [b,n_tau] (+ counts [b,2+n_tau] int32: n_union, n_inter,
    n_far_t).  The ids are not range-checked."""
    depth_est, depth_gt, depth_test = _dev_f32(depth_est), _dev_f32(depth_gt), _dev_f32(depth_test)
    K, diameter = _dev_f32(K), _dev_f32(diameter)
    if depth_est.dim() != 3 or depth_gt.dim() != 3 or depth_test.dim() != 3 or depth_gt.shape[1:] != depth_est.shape[1:] \
            or depth_test.shape[1:] != depth_est.shape[1:]:
        raise EngineError(f"depth maps must be [n,h,w] of one size, got {tuple(depth_est.shape)}, {tuple(depth_gt.shape)}, {tuple(depth_test.shape)}")
    b = K.shape[0]
    if K.shape != (b, 3, 3) or diameter.shape != (b,):
        raise EngineError(f"K must be [b,3,3] and diameter [b], got {tuple(K.shape)}, {tuple(diameter.shape)}")
    h, w = depth_est.shape[1:]
    ids = [_row_ids("est_ids", est_ids, depth_est, b), _row_ids("gt_ids", gt_ids, depth_gt, b), _row_ids("im_ids", im_ids, depth_test, b)]
    taus = [float(t) for t in (VSD_TAUS if taus is None else taus)]
    n_tau = len(taus)
    h_taus = (C.c_float * max(n_tau, 1))(*taus)
    dev = K.device
    out = dict(errs=torch.empty(b, n_tau, dtype=torch.float32, device=dev))
    if with_counts:
        out["counts"] = torch.empty(b, 2 + n_tau, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.mp_vsd_workspace_bytes(b, n_tau), dev)
    check(lib.mp_vsd(depth_est.data_ptr(), _ptr(ids[0]), depth_gt.data_ptr(), _ptr(ids[1]), depth_test.data_ptr(), _ptr(ids[2]),
                     depth_est.shape[0], depth_gt.shape[0], depth_test.shape[0], K.data_ptr(), diameter.data_ptr(), b, h, w, float(delta),
                     C.cast(h_taus, C.c_void_p), n_tau, int(bool(normalized_by_diameter)), int(split), out["errs"].data_ptr(),
                     _ptr(out.get("counts")), ws.data_ptr(), ws.numel(), _stream()))
    return out


# --------------------------------------------------------------------------- #
# BOP's ground-truth info (evaluation): csrc/gt_info.hip
def gt_info(depth_gt: torch.Tensor, depth_test: torch.Tensor, K: torch.Tensor, canvas: int = 3, delta: float = 0.015,
            gt_ids: Optional[torch.Tensor] = None, im_ids: Optional[torch.Tensor] = None, with_masks: bool = False,
            split: int = 0) -> Dict[str, torch.Tensor]:
    """BOP's gt info (mp_gt_info).  depth_gt [n_gt,canvas*canvas,h,w] metres: the object's renders on the canvas' tiles, row-major
    ([n_gt,h,w] is taken as canvas 1); depth_test [n_im,h,w]; row i takes depth_gt[gt_ids[i]] under depth_test[im_ids[i]] (ids None:
    map i) and K [b,3,3] -> counts [b,4] int32 (px_count_all, _image, _valid, _visib), boxes [b,8] int32 (bbox_obj then bbox_visib as
    inclusive xmin ymin xmax ymax, -1 over no pixel), visib_fract [b] (+ mask, mask_visib [b,h,w] uint8 0 / 255).  The ids are not
    range-checked."""
    depth_gt, depth_test, K = _dev_f32(depth_gt), _dev_f32(depth_test), _dev_f32(K)
    if depth_gt.dim() == 3 and canvas == 1:
        depth_gt = depth_gt.unsqueeze(1)
    if depth_gt.dim() != 4 or depth_test.dim() != 3 or depth_gt.shape[1] != canvas * canvas or depth_gt.shape[2:] != depth_test.shape[1:]:
        raise EngineError(f"depth_gt must be [n_gt,{canvas * canvas},h,w] and depth_test [n_im,h,w], got {tuple(depth_gt.shape)}, {tuple(depth_test.shape)}")
    b = K.shape[0]
    if K.shape != (b, 3, 3):
        raise EngineError(f"K must be [b,3,3], got {tuple(K.shape)}")
    h, w = depth_test.shape[1:]
    ids = [_row_ids("gt_ids", gt_ids, depth_gt, b), _row_ids("im_ids", im_ids, depth_test, b)]
    dev = K.device
    out = dict(counts=torch.empty(b, 4, dtype=torch.int32, device=dev), boxes=torch.empty(b, 8, dtype=torch.int32, device=dev),
               visib_fract=torch.empty(b, dtype=torch.float32, device=dev))
    if with_masks:
        out["mask"] = torch.empty(b, h, w, dtype=torch.uint8, device=dev)
        out["mask_visib"] = torch.empty(b, h, w, dtype=torch.uint8, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.mp_gt_info_workspace_bytes(b), dev)
    check(lib.mp_gt_info(depth_gt.data_ptr(), _ptr(ids[0]), depth_test.data_ptr(), _ptr(ids[1]), depth_gt.shape[0], depth_test.shape[0],
                         K.data_ptr(), b, h, w, int(canvas), float(delta), int(split), out["counts"].data_ptr(), out["boxes"].data_ptr(),
                         out["visib_fract"].data_ptr(), _ptr(out.get("mask")), _ptr(out.get("mask_visib")), ws.data_ptr(), ws.numel(),
                         _stream()))
    return out


# --------------------------------------------------------------------------- #
# BOP's greedy matching (evaluation): csrc/bop_match.hip
BOP_MATCH_MAX_ERRORS = 16            # E
BOP_MATCH_MAX_THETAS = 16            # n_theta
BOP_MATCH_MASK_BITS = 64             # fast path: ground truths of a group
BOP_MATCH_STAGE_FLOATS = 4096        # fast path: walked candidates of a group * E
BOP_MATCH_INDEX = ("cand_gt", "cand_lgt", "est_row", "est_off", "group_est_off", "group_n_gt", "group_taken_off")


def bop_match_limits() -> Dict[str, int]:
    """what the library was built for (mp_bop_match_limits); the constants above restate it"""
    v = [C.c_int(0) for _ in range(4)]
    check(_lib.load().mp_bop_match_limits(*[C.byref(x) for x in v]))
    return dict(zip(("max_errors", "max_thetas", "mask_bits", "stage_floats"), (int(x.value) for x in v)))


def _match_index(index: Dict[str, torch.Tensor], c: int, n_groups: Optional[int], checked: Sequence[str], misfit: str,
                 n_top: Optional[torch.Tensor]):
    """What bop_match and det_match share: the BOP_MATCH_INDEX tensors as int32 on the device, the shapes of those named in `checked`
    (any other shape: EngineError(misfit)), n_top [n_groups] and the host int `n_taken_words`; n_groups None = as many as group_n_gt has
    -> (index, its seven device addresses in call order, n_top, n_est, n_groups, n_words).  Keep `index` referenced until the launch is
    enqueued: the addresses point into it."""
    ix = {k: _dev_i32(index[k]) for k in BOP_MATCH_INDEX}
    n_est = ix["est_row"].shape[0]
    if n_groups is None:
        n_groups = ix["group_n_gt"].shape[0]
    shape = dict(cand_gt=(c,), cand_lgt=(c,), est_off=(n_est + 1,), group_est_off=(n_groups + 1,), group_n_gt=(n_groups,),
                 group_taken_off=(n_groups + 1,))
    if any(ix[k].shape != shape[k] for k in checked):
        raise EngineError(misfit)
    if n_top is not None:
        n_top = _dev_i32(n_top)
        if n_top.shape != (n_groups,):
            raise EngineError(f"n_top must be [n_groups], got {tuple(n_top.shape)}")
    n_words = int(index["n_taken_words"])            # a host int (= group_taken_off[-1]): nothing is read back here
    return ix, [ix[k].data_ptr() for k in BOP_MATCH_INDEX], n_top, n_est, n_groups, n_words


def bop_match(errs: torch.Tensor, index: Dict[str, torch.Tensor], thr: torch.Tensor, n_pred: int,
              n_top: Optional[torch.Tensor] = None) -> torch.Tensor:
    """BOP's greedy matching (mp_bop_match).  errs [C,E] float32 in the index's candidate order; index = the int32 tensors
    BOP_MATCH_INDEX as include/mp_engine.h lays them out plus the host int `n_taken_words` (`evaluation.bop_match_index` builds
    them); thr [n_groups,E,n_theta] float64;
    n_top [n_groups] int32 or None -> match [n_pred,E,n_theta] int32 (gt_row or -1).  The index is not range-checked."""
    errs = _dev_f32(errs)
    if errs.dim() != 2:
        raise EngineError(f"errs must be [C,E], got {tuple(errs.shape)}")
    dev = errs.device
    c, e = errs.shape
    thr = thr.to(device=dev, dtype=torch.float64).contiguous()
    if thr.dim() != 3 or thr.shape[1] != e:
        raise EngineError(f"thr must be [n_groups,{e},n_theta], got {tuple(thr.shape)}")
    n_groups, _, n_theta = thr.shape
    ix, ix_ptrs, n_top, n_est, n_groups, n_words = _match_index(
        index, c, n_groups, BOP_MATCH_INDEX[:2] + BOP_MATCH_INDEX[3:], "the index does not fit errs [C,E] and thr [n_groups,E,n_theta]", n_top)
    match = torch.empty(int(n_pred), e, n_theta, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.mp_bop_match_workspace_bytes(n_words, e, n_theta), dev)
    check(lib.mp_bop_match(errs.data_ptr(), *ix_ptrs, _ptr(n_top), thr.data_ptr(), int(n_pred), c, n_est, n_groups, n_words, e, n_theta,
                           match.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return match


# --------------------------------------------------------------------------- #
# BOP's detection / segmentation scores (evaluation): csrc/det_ap.hip
DET_MATCH_MAX_THETAS = 16            # n_theta
MASK_PAIR_MAX_PAIRS = 1 << 23        # candidates of one mp_mask_pair_counts call


def _dev_bytes(name: str, t: torch.Tensor) -> torch.Tensor:
    """a uint8 or bool device tensor as uint8, through a view: no copy unless it is not contiguous"""
    t = _dev(t, t.dtype)
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype != torch.uint8:
        raise EngineError(f"{name} must be uint8 or bool, got {t.dtype}")
    return t


def mask_pair_counts(pred_masks: torch.Tensor, gt_masks: torch.Tensor, cand_pred: torch.Tensor, cand_gt: torch.Tensor,
                     split: int = 0) -> torch.Tensor:
    """Pixel counts of mask pairs (mp_mask_pair_counts).  pred_masks [P,H,W], gt_masks [G,H,W] uint8 or bool (a pixel is set when its
    byte is non-zero; taken through a uint8 view, no copy); cand_pred, cand_gt [C] int32 -> counts [C,3] int32: intersection, area of
    pred_masks[cand_pred[c]], area of gt_masks[cand_gt[c]]; -1 -1 -1 for a candidate whose index is out of range.  More than
    MASK_PAIR_MAX_PAIRS candidates go in several launches."""
    pred_masks, gt_masks = _dev_bytes("pred_masks", pred_masks), _dev_bytes("gt_masks", gt_masks)
    if pred_masks.dim() != 3 or gt_masks.dim() != 3 or pred_masks.shape[1:] != gt_masks.shape[1:]:
        raise EngineError(f"masks must be [P,H,W] and [G,H,W], got {tuple(pred_masks.shape)}, {tuple(gt_masks.shape)}")
    cand_pred, cand_gt = _dev_i32(cand_pred), _dev_i32(cand_gt)
    if cand_pred.dim() != 1 or cand_pred.shape != cand_gt.shape:
        raise EngineError(f"cand_pred and cand_gt must be [C], got {tuple(cand_pred.shape)}, {tuple(cand_gt.shape)}")
    c = cand_pred.shape[0]
    h, w = pred_masks.shape[1:]
    counts = torch.empty(c, 3, dtype=torch.int32, device=pred_masks.device)
    lib = _lib.load()
    for c0 in range(0, max(c, 1), MASK_PAIR_MAX_PAIRS):
        n = min(c, c0 + MASK_PAIR_MAX_PAIRS) - c0
        check(lib.mp_mask_pair_counts(pred_masks.data_ptr(), gt_masks.data_ptr(), cand_pred[c0:].data_ptr(), cand_gt[c0:].data_ptr(),
                                      pred_masks.shape[0], gt_masks.shape[0], n, h, w, int(split), counts[c0:].data_ptr(), _stream()))
    return counts


def det_match(iou: torch.Tensor, index: Dict[str, torch.Tensor], gt_ignore: torch.Tensor, thr: torch.Tensor, n_pred: int,
              n_top: Optional[torch.Tensor] = None) -> torch.Tensor:
    """COCO's greedy matching (mp_det_match).  iou [C] float64 in the index's candidate order; index as `bop_match` takes it;
    gt_ignore [G] uint8 or bool, indexed by gt_row; thr [n_theta] float64; n_top [n_groups] int32 or None -> match [n_pred,n_theta]
    int32 (gt_row or -1).  Neither the index nor the gt_rows against gt_ignore are range-checked."""
    iou = _dev(iou, torch.float64)
    dev = iou.device
    thr = thr.to(device=dev, dtype=torch.float64).contiguous()
    if iou.dim() != 1 or thr.dim() != 1:
        raise EngineError(f"iou must be [C] and thr [n_theta], got {tuple(iou.shape)}, {tuple(thr.shape)}")
    c, n_theta = iou.shape[0], thr.shape[0]
    gt_ignore = _dev_bytes("gt_ignore", gt_ignore)
    misfit = "the index does not fit iou [C]"
    if gt_ignore.dim() != 1:
        raise EngineError(misfit)
    ix, ix_ptrs, n_top, n_est, n_groups, n_words = _match_index(
        index, c, None, ("cand_gt", "cand_lgt", "est_off", "group_est_off", "group_taken_off"), misfit, n_top)
    match = torch.empty(int(n_pred), n_theta, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.mp_det_match_workspace_bytes(n_words, n_theta), dev)
    check(lib.mp_det_match(iou.data_ptr(), *ix_ptrs, _ptr(n_top), gt_ignore.data_ptr(), thr.data_ptr(), int(n_pred), c, n_est, n_groups,
                           n_words, n_theta, match.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return match


# --------------------------------------------------------------------------- #
# BOP's result files (bop_files): COCO run-length encoding of masks, csrc/rle.hip
RLE_MAX_PIXELS = (1 << 31) - 2       # h * w
RLE_STATUS_EMPTY, RLE_STATUS_NEGATIVE, RLE_STATUS_SUM = 1, 2, 4   # bits of rle_decode's status


def _host_offsets(offsets, n_counts: int) -> np.ndarray:
    h_off = np.ascontiguousarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets).astype(np.int64)
    if h_off.ndim != 1 or len(h_off) < 1 or h_off[0] != 0 or (np.diff(h_off) < 0).any() or h_off[-1] > n_counts:
        raise EngineError(f"offsets must be [n + 1], start at 0, not descend and end within the {n_counts} counts")
    return h_off


def rle_encode(masks: torch.Tensor, rows_per_segment: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """COCO run-length encoding of masks (mp_rle_count, mp_rle_encode; the format is stated in csrc/rle_core.h).  masks [n,h,w] uint8 or
    bool on the device (a pixel is set when its byte is non-zero; taken through a uint8 view, no copy) -> counts [total] int32, the
    lists one after the other, offsets [n + 1] int64 (mask m's list is counts[offsets[m]:offsets[m + 1]]), areas [n] int32, boxes [n,4]
    int32 (x_min, y_min, x_max, y_max inclusive; 0 0 -1 -1 for an empty mask), all on the device.  A list walks the mask column by
    column and alternates run lengths of unset and set pixels, starting with unset.  rows_per_segment (0: the library's choice) only
    changes the decomposition, never a result.  ONE synchronisation: the n list lengths are read back between the two calls, as the
    ragged total is not known before."""
    masks = _dev_bytes("masks", masks)
    if masks.dim() != 3:
        raise EngineError(f"masks must be [n,h,w], got {tuple(masks.shape)}")
    n, h, w = (int(v) for v in masks.shape)
    dev = masks.device
    n_counts = torch.empty(n, dtype=torch.int32, device=dev)
    areas = torch.empty(n, dtype=torch.int32, device=dev)
    boxes = torch.empty(n, 4, dtype=torch.int32, device=dev)
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), areas, boxes
    lib = _lib.load()
    n_bytes = lib.mp_rle_workspace_bytes(n, h, w, int(rows_per_segment))
    if n_bytes == 0:
        raise EngineError(f"rle_encode: masks of {h} x {w} (at least 1 x 1, at most {RLE_MAX_PIXELS} pixels), rows_per_segment "
                          f"{rows_per_segment} (not negative), or too many jobs in one call")
    ws = _workspace(n_bytes, dev)
    check(lib.mp_rle_count(masks.data_ptr(), n, h, w, int(rows_per_segment), n_counts.data_ptr(), areas.data_ptr(), boxes.data_ptr(),
                           ws.data_ptr(), ws.numel(), _stream()))
    h_off = np.zeros(n + 1, np.int64)
    np.cumsum(n_counts.cpu().numpy(), dtype=np.int64, out=h_off[1:])       # the one synchronisation
    total = int(h_off[-1])
    counts = torch.empty(total, dtype=torch.int32, device=dev)
    check(lib.mp_rle_encode(masks.data_ptr(), n, h, w, int(rows_per_segment), h_off.ctypes.data, counts.data_ptr(), total, ws.data_ptr(),
                            ws.numel(), _stream()))
    return counts, torch.from_numpy(h_off).to(dev), areas, boxes


def rle_decode(counts: torch.Tensor, offsets, h: int, w: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Masks from run-length lists (mp_rle_decode).  counts [total] int32 on the device, offsets [n + 1] (host ints, an array or a
    tensor: the launch tests a host copy of them) -> masks [n,h,w] uint8 (0 / 1), status [n] int32: 0 for a well-formed list, else the
    OR of RLE_STATUS_EMPTY (no entries), RLE_STATUS_NEGATIVE (a negative entry) and RLE_STATUS_SUM (the entries do not sum to h * w), and
    the mask is all zeros.  Nothing synchronises (a tensor of offsets on the device is read back before the launch)."""
    counts = _dev_i32(counts)
    if counts.dim() != 1:
        raise EngineError(f"counts must be [total], got {tuple(counts.shape)}")
    dev = counts.device
    h_off = _host_offsets(offsets, counts.shape[0])
    n, h, w = len(h_off) - 1, int(h), int(w)
    if h < 1 or w < 1 or h * w > RLE_MAX_PIXELS:
        raise EngineError(f"rle_decode: masks of {h} x {w}: at least 1 x 1, at most {RLE_MAX_PIXELS} pixels")
    masks = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return masks, status
    lib = _lib.load()
    ws = _workspace(lib.mp_rle_decode_workspace_bytes(n, h, w, counts.shape[0]), dev)
    check(lib.mp_rle_decode(counts.data_ptr(), h_off.ctypes.data, counts.shape[0], n, h, w, masks.data_ptr(), status.data_ptr(), ws.data_ptr(),
                            ws.numel(), _stream()))
    return masks, status


# --------------------------------------------------------------------------- #
# Onboarding without a CAD model (onboarding): TSDF fusion and marching tetrahedra, csrc/tsdf.hip
TSDF_MIN_DIM, TSDF_MAX_DIM = 2, 512  # nodes a side
TSDF_MAX_NODES = 1 << 27             # nx * ny * nz
TSDF_MAX_SIDE = 8192                 # h, w of a frame


def _tsdf_dims(volume: torch.Tensor) -> Tuple[int, int, int, int]:
    if not volume.is_cuda or volume.dtype != torch.float32 or volume.dim() != 4 or volume.shape[0] not in (2, 6) or not volume.is_contiguous():
        raise EngineError("a TSDF volume is a contiguous float32 device tensor [2 or 6, nz, ny, nx] (tsdf_volume)")
    nz, ny, nx = (int(v) for v in volume.shape[1:])
    return nx, ny, nz, int(volume.shape[0] == 6)


def tsdf_volume(dims: Sequence[int], color: bool, device) -> torch.Tensor:
    """An empty volume of dims = (nx, ny, nz) nodes: float32 zeros [2 or 6, nz, ny, nx] -- the sum of truncated distances, the count of
    views (int32 bits: `volume[1].view(torch.int32)`), and with `color` the sums of red, green, blue and the colour count."""
    nx, ny, nz = (int(v) for v in dims)
    if _lib.load().mp_tsdf_volume_bytes(nx, ny, nz, int(bool(color))) == 0:
        raise EngineError(f"tsdf_volume: {nx} x {ny} x {nz} nodes: each side {TSDF_MIN_DIM} .. {TSDF_MAX_DIM}, at most {TSDF_MAX_NODES} nodes")
    return torch.zeros(6 if color else 2, nz, ny, nx, dtype=torch.float32, device=device)


def _posed_views(depth: torch.Tensor, K: torch.Tensor, TCO: torch.Tensor, masks: Optional[torch.Tensor], rgb: Optional[torch.Tensor],
                 poses_4x4: bool = False):
    """A set of n posed views as the onboarding entries take it, checked: depth [n,h,w], K [n,3,3] and TCO [n,4,4] or [n,3,4] (rows of
    any shape that holds those floats; `poses_4x4`: exactly [n,3,3] and [n,4,4], what tracking takes), masks [n,h,w] and rgb [n,h,w,3]
    uint8 / bool or None -> (depth, K, TCO, masks, rgb) as contiguous device tensors and (n, h, w, tco_floats).  Without views K and TCO
    are not looked at unless `poses_4x4`, and tco_floats is 16."""
    depth = _dev_f32(depth)
    if depth.dim() != 3:
        raise EngineError(f"depth must be [n,h,w], got {tuple(depth.shape)}")
    n, h, w = (int(v) for v in depth.shape)
    K, TCO = _dev_f32(K), _dev_f32(TCO)
    given = tuple(K.shape), tuple(TCO.shape)
    if poses_4x4:
        K_ok, TCO_ok = tuple(K.shape) == (n, 3, 3), tuple(TCO.shape) == (n, 4, 4)
    elif n:
        K, TCO = K.reshape(n, -1), TCO.reshape(n, -1)
        K_ok, TCO_ok = K.shape[1] == 9, TCO.shape[1] in (12, 16)
    else:
        K_ok = TCO_ok = True
    if not K_ok:
        raise EngineError(f"K must be [n,3,3], got {given[0]}")
    if not TCO_ok:
        raise EngineError(f"TCO must be [n,4,4]{'' if poses_4x4 else ' or [n,3,4]'}, got {given[1]}")
    if masks is not None:
        masks = _dev_bytes("masks", masks)
        if tuple(masks.shape) != (n, h, w):
            raise EngineError(f"masks must be {(n, h, w)}, got {tuple(masks.shape)}")
    if rgb is not None:
        rgb = _dev_bytes("rgb", rgb)
        if tuple(rgb.shape) != (n, h, w, 3):
            raise EngineError(f"rgb must be {(n, h, w, 3)}, got {tuple(rgb.shape)}")
    return (depth, K, TCO, masks, rgb), (n, h, w, int(TCO.numel() // n) if n else 16)


def _tsdf_mu(mu: Optional[float], voxel: float) -> float:   # the truncation distance in metres: 3 voxels when None
    return float(np.float32(3.0) * np.float32(voxel)) if mu is None else float(mu)


def tsdf_integrate(volume: torch.Tensor, origin: Sequence[float], voxel: float, depth: torch.Tensor, K: torch.Tensor, TCO: torch.Tensor,
                   masks: Optional[torch.Tensor] = None, rgb: Optional[torch.Tensor] = None, mu: Optional[float] = None, z_min: float = 1e-3,
                   carve: bool = True) -> None:
    """Fuses n posed depth views into `volume`, in place (mp_tsdf_integrate; the rules are stated in csrc/tsdf_core.h).  depth [n,h,w]
    metres (not finite or <= 0: no measurement), K [n,3,3], TCO [n,4,4] or [n,3,4] object to camera, masks [n,h,w] uint8 / bool (0: not
    the object; with `carve` such a pixel marks the nodes on its ray as free space, without it they are skipped), rgb [n,h,w,3] uint8.
    Node (i,j,k) lies at origin + voxel * (i,j,k); mu is the truncation distance in metres (3 voxels when None).  Calls continue each
    other bit for bit.  Nothing synchronises."""
    nx, ny, nz, color = _tsdf_dims(volume)
    (depth, K, TCO, masks, rgb), (n, h, w, tco_floats) = _posed_views(depth, K, TCO, masks, rgb)
    ox, oy, oz = (float(v) for v in origin)
    check(_lib.load().mp_tsdf_integrate(volume.data_ptr(), nx, ny, nz, color, ox, oy, oz, float(voxel), depth.data_ptr(), _ptr(masks), _ptr(rgb),
                                        K.data_ptr(), TCO.data_ptr(), tco_floats, n, h, w, _tsdf_mu(mu, voxel), float(z_min), int(bool(carve)),
                                        _stream()))


def tsdf_extract(volume: torch.Tensor, origin: Sequence[float], voxel: float, min_views: int = 1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The welded triangle mesh of the zero level of the volume's field over the nodes seen by at least min_views views, by marching
    tetrahedra (mp_tsdf_extract_count, mp_tsdf_extract) -> vertices [nv,3] float32 in the object's frame, colors [nv,3] float32 in
    0 .. 1 (white without colours), faces [nt,3] int32, wound so that normals point out of the object; all on the device.  ONE
    synchronisation: the two totals are read back between the two calls."""
    nx, ny, nz, color = _tsdf_dims(volume)
    dev = volume.device
    lib = _lib.load()
    ws = _workspace(lib.mp_tsdf_extract_workspace_bytes(nx, ny, nz), dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    check(lib.mp_tsdf_extract_count(volume.data_ptr(), nx, ny, nz, color, int(min_views), totals.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    nv, nt = (int(v) for v in totals.cpu().tolist())      # the one synchronisation
    vertices = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    colors = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(nt, 3, dtype=torch.int32, device=dev)
    ox, oy, oz = (float(v) for v in origin)
    check(lib.mp_tsdf_extract(volume.data_ptr(), nx, ny, nz, color, ox, oy, oz, float(voxel), nv, nt, vertices.data_ptr(), colors.data_ptr(),
                              faces.data_ptr(), nv, nt, ws.data_ptr(), ws.numel(), _stream()))
    return vertices, colors, faces


TSDF_TRACK_RECORD = 32              # doubles of a group's record


def tsdf_track_groups(h: int, w: int) -> int:
    """Records of 32 doubles a frame of h x w leaves in the partial sums (mp_tsdf_track_groups): one per 1024 pixels; 0 for a frame
    size the kernels refuse."""
    return int(_lib.load().mp_tsdf_track_groups(int(h), int(w)))


def tsdf_track(volume: torch.Tensor, origin: Sequence[float], voxel: float, depth: torch.Tensor, K: torch.Tensor, TCO: torch.Tensor,
               masks: Optional[torch.Tensor] = None, mu: Optional[float] = None, min_views: int = 1, min_pixels: int = 64, iters: int = 10,
               eps_rot: float = 1e-5, eps_trans: Optional[float] = None,
               partials: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The poses of n unposed depth frames against `volume`, each tracked from its own pose TCO [n,4,4] (object to camera) by
    Gauss-Newton on the signed distances the volume holds at the frame's back-projected pixels (mp_tsdf_track; the rules are stated in
    csrc/tsdf_track_core.h).  depth [n,h,w] metres, K [n,3,3], masks [n,h,w] uint8 / bool or None (every measured pixel).  mu is the
    truncation distance the volume was fused with (3 voxels when None); eps_rot (rad) and eps_trans (metres; 1e-3 voxel when None) end a
    frame's iterations early.  -> (TCO [n,4,4] float32, status [n] int32: 0 ran all iterations, 1 converged, -1 lost, -2 a non-finite K
    or pose; used [n] int32 pixels; rms [n] float32 metres), all on the device.  A frame of negative status returns its input pose bit
    for bit.  Frames are independent.  Nothing synchronises.  `partials`: a float64 device tensor of at least n * tsdf_track_groups(h,
    w) * 32 entries to be filled with the groups' records of the last iteration (for tests)."""
    nx, ny, nz, color = _tsdf_dims(volume)
    (depth, K, TCO, masks, _), (n, h, w, _) = _posed_views(depth, K, TCO, masks, None, poses_4x4=True)
    dev = volume.device
    out = torch.empty(n, 4, 4, dtype=torch.float32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    used = torch.empty(n, dtype=torch.int32, device=dev)
    rms = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out, status, used, rms
    groups = tsdf_track_groups(h, w)
    if groups == 0:
        raise EngineError(f"tsdf_track: frames of {h} x {w}: 1 .. {TSDF_MAX_SIDE} a side")
    if partials is None:
        partials = torch.empty(n, groups, TSDF_TRACK_RECORD, dtype=torch.float64, device=dev)
    elif not partials.is_cuda or partials.dtype != torch.float64 or not partials.is_contiguous():
        raise EngineError("tsdf_track: partials must be a contiguous float64 device tensor")
    eps_trans = float(np.float32(1e-3) * np.float32(voxel)) if eps_trans is None else float(eps_trans)
    ox, oy, oz = (float(v) for v in origin)
    check(_lib.load().mp_tsdf_track(volume.data_ptr(), nx, ny, nz, color, ox, oy, oz, float(voxel), depth.data_ptr(), _ptr(masks), K.data_ptr(),
                                    TCO.data_ptr(), n, h, w, _tsdf_mu(mu, voxel), int(min_views), int(min_pixels), int(iters), float(eps_rot),
                                    eps_trans, out.data_ptr(), status.data_ptr(), used.data_ptr(), rms.data_ptr(), partials.data_ptr(),
                                    partials.numel() // TSDF_TRACK_RECORD, _stream()))
    return out, status, used, rms


# --------------------------------------------------------------------------- #
# A texture atlas for a mesh from its posed views (onboarding.bake_texture), csrc/texture_bake.hip
TEXTURE_MIN_SIZE, TEXTURE_MAX_SIZE = 64, 8192   # texels a side, a power of two


def texture_atlas_block(n_triangles: int, size: int) -> int:
    """The side B of the square blocks of a size x size atlas for n_triangles (mp_texture_atlas_block): the largest of 64, 32, 16, 8, 4
    with ceil(n_triangles / 2) <= (size / B)^2, 0 when none fits or size is no power of two in 64 .. 8192.  Block k, in row-major
    order, holds triangles 2k and 2k + 1 with legs of B - 3 texels."""
    return int(_lib.load().mp_texture_atlas_block(int(n_triangles), int(size)))


def _texture_block(what: str, n_triangles: int, size: int) -> int:
    block = texture_atlas_block(n_triangles, size) if n_triangles >= 1 else 0
    if block == 0:
        raise EngineError(f"{what}: {n_triangles} triangles (at least 1) do not fit an atlas of {size} x {size} texels (a power of two, "
                          f"{TEXTURE_MIN_SIZE} .. {TEXTURE_MAX_SIZE}; two triangles per block of at least 4 x 4)")
    return block


def texture_atlas_uvs(n_triangles: int, size: int, device="cuda") -> torch.Tensor:
    """The per-corner texture coordinates [n_triangles,3,2] float32 of the atlas's charts (mp_texture_atlas_uvs): the centres of the
    charts' corner texels, row 0 of the texture being v = 0.  Nothing synchronises."""
    n_triangles, size = int(n_triangles), int(size)
    _texture_block("texture_atlas_uvs", n_triangles, size)
    uvs = torch.empty(n_triangles, 3, 2, dtype=torch.float32, device=device)
    check(_lib.load().mp_texture_atlas_uvs(n_triangles, size, uvs.data_ptr(), _stream()))
    return uvs


def texture_bake(vertices: torch.Tensor, faces: torch.Tensor, depth: torch.Tensor, K: torch.Tensor, TCO: torch.Tensor,
                 masks: Optional[torch.Tensor], rgb: torch.Tensor, size: int, colors: Optional[torch.Tensor] = None, depth_tol: float = 2e-3,
                 cos_min: float = 0.2, z_min: float = 1e-3, best_view: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Bakes the texture atlas of a mesh from n posed views (mp_texture_bake; the rules are stated in csrc/texture_bake_core.h).
    vertices [V,3] float32 in the object's frame, faces [T,3] int32, depth [n,h,w] metres (not finite or <= 0: no measurement), K
    [n,3,3], TCO [n,4,4] or [n,3,4] object to camera, masks [n,h,w] uint8 / bool or None (0: not the object), rgb [n,h,w,3] uint8,
    colors [V,3] floats in 0 .. 1 (what a texel no view sees takes; white without).  A view colours a texel when the texel's surface
    point projects into its frame, faces it with cos > cos_min and lies within depth_tol metres of the view's own depth there; the texel
    is the cos^2-weighted mean of the views' bilinear colours (best_view: the colour of the view that sees it most squarely).
    -> texels [size,size,4] uint8 (RGBA, row 0 is v = 0; alpha 255 on charts, 0 elsewhere), seen [size,size] uint8 (contributing views,
    capped at 255), on the device.  The charts' texture coordinates are texture_atlas_uvs(T, size).  Nothing synchronises."""
    vertices, colors = _mesh_vertices(vertices, colors)
    faces = _mesh_faces(faces)
    size = int(size)
    _texture_block("texture_bake", int(faces.shape[0]), size)
    if rgb is None:
        raise EngineError("texture_bake: rgb is what the texture is made of")
    (depth, K, TCO, masks, rgb), (n, h, w, tco_floats) = _posed_views(depth, K, TCO, masks, rgb)
    dev = vertices.device
    texels = torch.empty(size, size, 4, dtype=torch.uint8, device=dev)
    seen = torch.empty(size, size, dtype=torch.uint8, device=dev)
    ptr = (lambda t: t.data_ptr()) if n else (lambda t: None)   # noqa: E731
    check(_lib.load().mp_texture_bake(vertices.data_ptr() if vertices.shape[0] else None, int(vertices.shape[0]), faces.data_ptr(), int(faces.shape[0]),
                                      _ptr(colors), ptr(depth), _ptr(masks) if n else None, ptr(rgb), ptr(K), ptr(TCO), tco_floats,
                                      n, h, w, size, float(depth_tol), float(cos_min), float(z_min), int(bool(best_view)), texels.data_ptr(),
                                      seen.data_ptr(), _stream()))
    return texels, seen


# --------------------------------------------------------------------------- #
# Cleaning up a triangle mesh (mesh_cleanup): components, selection, vertex clustering, csrc/mesh_cleanup.hip
MESH_MAX_COUNT = 1 << 29             # vertices, faces
MESH_MAX_DIM = 512                   # cells a side
MESH_MAX_CELLS = 1 << 27             # gx * gy * gz


def _mesh_faces(faces: torch.Tensor) -> torch.Tensor:
    faces = _dev_i32(faces)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise EngineError(f"faces must be [F,3], got {tuple(faces.shape)}")
    return faces


def _mesh_vertices(vertices: torch.Tensor, colors: Optional[torch.Tensor]) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    vertices = _dev_f32(vertices)
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise EngineError(f"vertices must be [V,3], got {tuple(vertices.shape)}")
    if colors is not None:
        colors = _dev_f32(colors)
        if tuple(colors.shape) != tuple(vertices.shape):
            raise EngineError(f"colors must be {tuple(vertices.shape)}, got {tuple(colors.shape)}")
    return vertices, colors


def _mesh_grid(origin: Sequence[float], cell: float, dims: Sequence[int]):
    ox, oy, oz = (float(v) for v in origin)
    gx, gy, gz = (int(v) for v in dims)
    return (ox, oy, oz, float(cell)), (gx, gy, gz)


def mesh_components(vertices_or_V, faces: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The connected components of a mesh (mp_mesh_components; rules in csrc/mesh_cleanup_core.h).  vertices_or_V: the vertices [V,3]
    or their number; faces [F,3] int32 on the device -> labels [V] int32 (the smallest vertex index of the vertex's component),
    face_labels [F] int32 (-1 for a face with an index outside [0, V)), face_count [V] int32 (faces per label), totals [4] int32 on the
    device: components that own a face, the label of the one with the most faces (-1 without any), bad faces, status (non-zero: a loop
    of the union-find reached its cap and the labels are not to be used).  Nothing synchronises: the caller reads the totals when it
    needs them."""
    faces = _mesh_faces(faces)
    V = int(vertices_or_V.shape[0]) if torch.is_tensor(vertices_or_V) else int(vertices_or_V)
    F = int(faces.shape[0])
    dev = faces.device
    labels = torch.empty(max(V, 0), dtype=torch.int32, device=dev)
    face_count = torch.empty(max(V, 0), dtype=torch.int32, device=dev)
    face_labels = torch.empty(F, dtype=torch.int32, device=dev)
    totals = torch.empty(4, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.mp_mesh_components_workspace_bytes(V, F), dev)
    check(lib.mp_mesh_components(V, faces.data_ptr(), F, labels.data_ptr(), face_labels.data_ptr(), face_count.data_ptr(), totals.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _stream()))
    return labels, face_labels, face_count, totals


def mesh_select(vertices: torch.Tensor, faces: torch.Tensor, keep: torch.Tensor, colors: Optional[torch.Tensor] = None):
    """The faces with keep != 0 and the vertices they reference, renumbered, both in input order (mp_mesh_select_count,
    mp_mesh_select).  keep [F] uint8 or bool -> vertices [nv,3], faces [nf,3] int32, colors [nv,3] or None, n_bad (faces with an index
    outside [0, V): never kept).  ONE synchronisation: the totals are read back between the two calls."""
    vertices, colors = _mesh_vertices(vertices, colors)
    faces = _mesh_faces(faces)
    keep = _dev_bytes("keep", keep)
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    if tuple(keep.shape) != (F,):
        raise EngineError(f"keep must be [{F}], got {tuple(keep.shape)}")
    dev = vertices.device
    lib = _lib.load()
    ws = _workspace(lib.mp_mesh_select_workspace_bytes(V, F), dev)
    totals = torch.zeros(3, dtype=torch.int32, device=dev)
    check(lib.mp_mesh_select_count(V, faces.data_ptr(), F, keep.data_ptr(), totals.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    nv, nf, n_bad = (int(v) for v in totals.cpu().tolist())      # the one synchronisation
    out_v = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    out_c = None if colors is None else torch.empty(nv, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    check(lib.mp_mesh_select(vertices.data_ptr(), _ptr(colors), V, faces.data_ptr(), F, nv, nf, out_v.data_ptr(), _ptr(out_c), out_f.data_ptr(), nv, nf,
                             ws.data_ptr(), ws.numel(), _stream()))
    return out_v, out_f, out_c, n_bad


def _mesh_cluster_count(lib, vertices, faces, grid, dims, ws) -> Tuple[int, int, int]:
    totals = torch.zeros(3, dtype=torch.int32, device=vertices.device)
    check(lib.mp_mesh_cluster_count(vertices.data_ptr(), int(vertices.shape[0]), faces.data_ptr(), int(faces.shape[0]), *grid, *dims, totals.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _stream()))
    nv, nf, n_dropped = (int(v) for v in totals.cpu().tolist())  # the one synchronisation
    return nv, nf, n_dropped


def mesh_cluster_count(vertices: torch.Tensor, faces: torch.Tensor, origin: Sequence[float], cell: float, dims: Sequence[int]) -> Tuple[int, int, int]:
    """What mesh_cluster would give on this grid, without building it (mp_mesh_cluster_count) -> vertices out, faces out, faces
    dropped for a bad index or a vertex outside the grid.  One synchronisation."""
    vertices, _ = _mesh_vertices(vertices, None)
    faces = _mesh_faces(faces)
    grid, dims = _mesh_grid(origin, cell, dims)
    lib = _lib.load()
    ws = _workspace(lib.mp_mesh_cluster_workspace_bytes(int(vertices.shape[0]), int(faces.shape[0]), *dims), vertices.device)
    return _mesh_cluster_count(lib, vertices, faces, grid, dims, ws)


def mesh_cluster(vertices: torch.Tensor, faces: torch.Tensor, origin: Sequence[float], cell: float, dims: Sequence[int],
                 colors: Optional[torch.Tensor] = None):
    """Decimation by vertex clustering (mp_mesh_cluster_count, mp_mesh_cluster): the vertices of one cell of the grid (origin, cell size,
    dims = cells per axis) become their exact mean, triangles that lose a corner disappear -> vertices [nv,3] in cell order, faces
    [nf,3] int32 in input order, colors [nv,3] or None, n_dropped.  Bit-reproducible.  ONE synchronisation."""
    vertices, colors = _mesh_vertices(vertices, colors)
    faces = _mesh_faces(faces)
    grid, dims = _mesh_grid(origin, cell, dims)
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    dev = vertices.device
    lib = _lib.load()
    ws = _workspace(lib.mp_mesh_cluster_workspace_bytes(V, F, *dims), dev)
    nv, nf, n_dropped = _mesh_cluster_count(lib, vertices, faces, grid, dims, ws)
    out_v = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    out_c = None if colors is None else torch.empty(nv, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    check(lib.mp_mesh_cluster(vertices.data_ptr(), _ptr(colors), V, faces.data_ptr(), F, *grid, *dims, nv, nf, out_v.data_ptr(), _ptr(out_c),
                              out_f.data_ptr(), nv, nf, ws.data_ptr(), ws.numel(), _stream()))
    return out_v, out_f, out_c, n_dropped


# --------------------------------------------------------------------------- #
# BOP's model info (evaluation): csrc/model_info.hip
MODEL_INFO_TILE_STEP = 64            # a forced tile is a multiple of this ...
MODEL_INFO_MAX_TILE = 1024           # ... and at most this


def model_info(points: torch.Tensor, n_points, tile: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The exact diameter and the bounds of point sets (mp_model_info).  points [n_obj,stride,3] float32 on the device; n_points
    [n_obj] (host ints, an array or a tensor: the launch needs them on both sides), each in 1 .. stride: the rows beyond are padding and
    are never read; tile = the j points of one LDS stage (0: the library's choice; a multiple of 64 up to 1024 forces it, for tests)
    -> d2 [n_obj] float32 (the largest squared distance), pair [n_obj,2] int32 (the rows that reach it, i <= j, lowest i then lowest j
    on equal distances), bounds [n_obj,6] float32 (min x y z, size x y z).  An object with a non-finite coordinate gives NaN, -1 -1,
    NaN.  Nothing synchronises (a tensor of n_points is read back before the launch)."""
    points = _dev_f32(points)
    if points.dim() != 3 or points.shape[2] != 3:
        raise EngineError(f"points must be [n_obj,stride,3], got {tuple(points.shape)}")
    n_obj, stride = int(points.shape[0]), int(points.shape[1])
    h_n = np.ascontiguousarray(n_points.cpu().numpy() if isinstance(n_points, torch.Tensor) else n_points).astype(np.int32)
    if h_n.shape != (n_obj,) or n_obj < 1 or h_n.min() < 1 or h_n.max() > stride:
        raise EngineError(f"n_points must be [n_obj] with every count in 1 .. {stride}")
    dev = points.device
    d_n = torch.from_numpy(h_n).to(dev)
    lib = _lib.load()
    n_bytes = lib.mp_model_info_scratch_bytes(n_obj, h_n.ctypes.data, int(tile))
    if n_bytes == 0:
        raise EngineError(f"model_info: tile {tile} is not 0 or a multiple of {MODEL_INFO_TILE_STEP} up to {MODEL_INFO_MAX_TILE}, or too many jobs")
    ws = _workspace(n_bytes, dev)
    d2 = torch.empty(n_obj, dtype=torch.float32, device=dev)
    pair = torch.empty(n_obj, 2, dtype=torch.int32, device=dev)
    bounds = torch.empty(n_obj, 6, dtype=torch.float32, device=dev)
    check(lib.mp_model_info(points.data_ptr(), stride, d_n.data_ptr(), h_n.ctypes.data, n_obj, int(tile), ws.data_ptr(), d2.data_ptr(),
                            pair.data_ptr(), bounds.data_ptr(), _stream()))
    return d2, pair, bounds


# --------------------------------------------------------------------------- #
# object symmetries (evaluation): csrc/symmetry.hip
SYMMETRY_TILE_STEP = 64              # a forced tile is a multiple of this ...
SYMMETRY_MAX_TILE = 512              # ... and at most this
SYMMETRY_MAX_CANDIDATES = 1 << 20    # candidates of one call


def symmetry_check(vertices: torch.Tensor, faces, tests: torch.Tensor, cand_R: torch.Tensor, centers: torch.Tensor, vert_off, face_off,
                   test_off, cand_off, tol, mode: int = 0, tile: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Which candidate rotations map an object's surface into itself (mp_symmetry_check).  vertices [V,3] float32, tests [T,3] float32
    (the test points), cand_R [C,3,3] float32 (the candidates, row-major rotations about the object's centre) and centers [n_obj,3]
    float32 on the device; faces [F,3] int32 (indices local to the object; an array or a tensor: the launch checks a host copy of them and
    reads a device copy); vert_off, face_off, test_off, cand_off [n_obj + 1] host ints, the prefix arrays that cut the four into
    objects (rows beyond their last entry are padding and are never read); tol [n_obj] host floats, finite and not negative; mode 0 =
    screen with early outs, then measure the accepted candidates; mode 1 = measure every candidate; tile = the triangles of one LDS
    stage (0: the library's choice; a multiple of 64 up to 512 forces it, for tests) -> accept [C] uint8, dev2 [C] float32 (the largest
    squared distance of a transformed test point to the surface; NaN for a candidate that mode 0 rejected), worst [C] int32 (the test
    point that reaches it, -1 likewise).  No tile, grid or arrival order changes a bit.  Nothing synchronises (tensors of offsets or
    faces on the device are read back before the launch)."""
    vertices, tests, cand_R, centers = _dev_f32(vertices), _dev_f32(tests), _dev_f32(cand_R), _dev_f32(centers)
    dev = vertices.device
    h_faces = np.ascontiguousarray(faces.cpu().numpy() if isinstance(faces, torch.Tensor) else faces)
    if h_faces.ndim != 2 or h_faces.shape[1] != 3 or h_faces.dtype.kind not in "iu":
        raise EngineError(f"faces must be integers [F,3], got {h_faces.dtype} {tuple(h_faces.shape)}")
    h_faces = h_faces.astype(np.int32)
    d_faces = faces.to(dev).contiguous() if isinstance(faces, torch.Tensor) and faces.dtype == torch.int32 else torch.from_numpy(h_faces).to(dev)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or tests.dim() != 2 or tests.shape[1] != 3:
        raise EngineError(f"vertices must be [V,3] and tests [T,3], got {tuple(vertices.shape)} and {tuple(tests.shape)}")
    if cand_R.dim() != 3 or tuple(cand_R.shape[1:]) != (3, 3) or centers.dim() != 2 or centers.shape[1] != 3:
        raise EngineError(f"cand_R must be [C,3,3] and centers [n_obj,3], got {tuple(cand_R.shape)} and {tuple(centers.shape)}")
    n_obj = int(centers.shape[0])
    offs = [np.ascontiguousarray(o.cpu().numpy() if isinstance(o, torch.Tensor) else o).astype(np.int64) for o in (vert_off, face_off, test_off, cand_off)]
    rows = (vertices.shape[0], h_faces.shape[0], tests.shape[0], cand_R.shape[0])
    if n_obj < 1 or any(o.shape != (n_obj + 1,) or o[0] != 0 or (np.diff(o) < 0).any() or o[-1] > r for o, r in zip(offs, rows)):
        raise EngineError(f"vert_off, face_off, test_off and cand_off must be [n_obj + 1 = {n_obj + 1}], start at 0, not descend and end within "
                          f"{rows} rows")
    if offs[3][-1] > SYMMETRY_MAX_CANDIDATES:
        raise EngineError(f"symmetry_check: {offs[3][-1]} candidates, more than {SYMMETRY_MAX_CANDIDATES} in one call")
    offs = [o.astype(np.int32) for o in offs]
    h_tol = np.ascontiguousarray(tol, np.float32).reshape(-1)
    if h_tol.shape != (n_obj,):
        raise EngineError(f"tol must be [n_obj = {n_obj}], got {h_tol.shape}")
    lib = _lib.load()
    ws = _workspace(lib.mp_symmetry_check_scratch_bytes(n_obj), dev)
    n_cand = int(cand_R.shape[0])
    accept = torch.zeros(n_cand, dtype=torch.uint8, device=dev)
    dev2 = torch.full((n_cand,), float("nan"), dtype=torch.float32, device=dev)
    worst = torch.full((n_cand,), -1, dtype=torch.int32, device=dev)
    check(lib.mp_symmetry_check(vertices.data_ptr(), d_faces.data_ptr(), h_faces.ctypes.data, tests.data_ptr(), cand_R.data_ptr(), centers.data_ptr(),
                                offs[0].ctypes.data, offs[1].ctypes.data, offs[2].ctypes.data, offs[3].ctypes.data, h_tol.ctypes.data, n_obj,
                                int(tile), int(mode), ws.data_ptr(), accept.data_ptr(), dev2.data_ptr(), worst.data_ptr(), _stream()))
    return accept, dev2, worst


# --------------------------------------------------------------------------- #
# prediction overlays (visualisation): csrc/overlay.hip
OVERLAY_OUTPUTS = ("contour", "mesh", "canny", "mask")
OVERLAY_MAX_DILATE = 8               # dilate_iterations
OVERLAY_MAX_THICKNESS = 8            # thickness of draw_boxes
OVERLAY_MAX_SIDE = 8192              # h, w


def _overlay_images(name: str, t: torch.Tensor, like: Optional[torch.Tensor] = None) -> torch.Tensor:
    t = _dev_bytes(name, t)
    if t.dim() != 4 or t.shape[3] != 3 or (like is not None and t.shape != like.shape):
        raise EngineError(f"{name} must be uint8 [n,h,w,3]" + ("" if like is None else f" like images {tuple(like.shape)}") + f", got {tuple(t.shape)}")
    n, h, w = (int(v) for v in t.shape[:3])
    if not (1 <= h <= OVERLAY_MAX_SIDE and 1 <= w <= OVERLAY_MAX_SIDE) or n * h * w * 3 >= 2 ** 31:
        raise EngineError(f"{name}: h and w must be in 1 .. {OVERLAY_MAX_SIDE} and n * h * w * 3 below 2^31, got {tuple(t.shape)}")
    return t


def _overlay_colors(colors, device) -> torch.Tensor:
    colors = torch.as_tensor(colors, dtype=torch.uint8).to(device).contiguous()
    if colors.dim() != 2 or colors.shape[0] < 1 or colors.shape[1] != 3:
        raise EngineError(f"colors must be uint8 [n_colors,3] with n_colors >= 1, got {tuple(colors.shape)}")
    return colors


def overlay(images: torch.Tensor, render: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None, colors=((0, 255, 0),),
            dilate_iterations: int = 1, outputs: Sequence[str] = ("contour", "mesh", "canny", "mask")) -> Dict[str, torch.Tensor]:
    """Contour overlay, mesh blend, edge map and mask of a batch in one launch (mp_overlay).  images uint8 [n,h,w,3] on the device; render
    the same or None; labels int32 [n,h,w] or None (< 0 background, l >= 0 an instance; without labels: 0 where any channel of the render
    is > 0, else -1); colors uint8 [n_colors,3] (label l is drawn in colour l mod n_colors); dilate_iterations in 0 .. 8 -> a dict of
    the requested outputs: "contour" [n,h,w,3] (each instance's occlusion-aware Canny contour, dilated, in its colour over the image),
    "mesh" [n,h,w,3] (plot_overlay's blend; needs the render), "canny" [n,h,w] (255 on a contour), "mask" [n,h,w] (255 on an instance),
    all uint8.  Nothing synchronises."""
    images = _overlay_images("images", images)
    dev = images.device
    n, h, w = (int(v) for v in images.shape[:3])
    outputs = tuple(outputs)
    if any(o not in OVERLAY_OUTPUTS for o in outputs) or len(set(outputs)) != len(outputs):
        raise EngineError(f"outputs must be distinct names of {OVERLAY_OUTPUTS}, got {outputs}")
    if render is None and labels is None:
        raise EngineError("overlay needs a render or a label map")
    if render is None and "mesh" in outputs:
        raise EngineError("the mesh blend needs a render")
    if render is not None:
        render = _overlay_images("render", render, images)
    if labels is not None:
        labels = _dev_i32(labels)
        if labels.shape != images.shape[:3]:
            raise EngineError(f"labels must be int32 [n,h,w] like images {tuple(images.shape)}, got {tuple(labels.shape)}")
    colors = _overlay_colors(colors, dev)
    k = int(dilate_iterations)
    if not 0 <= k <= OVERLAY_MAX_DILATE:
        raise EngineError(f"dilate_iterations must be in 0 .. {OVERLAY_MAX_DILATE}, got {dilate_iterations}")
    out = {o: torch.empty((n, h, w, 3) if o in ("contour", "mesh") else (n, h, w), dtype=torch.uint8, device=dev) for o in outputs}
    check(_lib.load().mp_overlay(images.data_ptr(), _ptr(render), _ptr(labels), colors.data_ptr(), colors.shape[0], n, h, w, k,
                                 _ptr(out.get("contour")), _ptr(out.get("canny")), _ptr(out.get("mask")), _ptr(out.get("mesh")), _stream()))
    return out


def draw_boxes(images: torch.Tensor, boxes: torch.Tensor, image_ids: torch.Tensor, colors=((255, 0, 0),), thickness: int = 2) -> torch.Tensor:
    """Box frames on images (mp_draw_boxes).  images uint8 [n,h,w,3] on the device; boxes [n_boxes,4] float32 (x1, y1, x2, y2, truncated
    to integers); image_ids [n_boxes] int32 (an id outside 0 .. n - 1 draws nothing); colors uint8 [n_colors,3] (box j is drawn in colour
    j mod n_colors; of overlapping frames the highest j shows); thickness in 1 .. 8 -> uint8 [n,h,w,3].  No text is drawn.  Nothing
    synchronises."""
    images = _overlay_images("images", images)
    dev = images.device
    n, h, w = (int(v) for v in images.shape[:3])
    boxes, image_ids = _dev_f32(boxes), _dev_i32(image_ids)
    if boxes.dim() != 2 or boxes.shape[1] != 4 or image_ids.shape != boxes.shape[:1]:
        raise EngineError(f"boxes must be [n_boxes,4] and image_ids [n_boxes], got {tuple(boxes.shape)}, {tuple(image_ids.shape)}")
    colors = _overlay_colors(colors, dev)
    t = int(thickness)
    if not 1 <= t <= OVERLAY_MAX_THICKNESS:
        raise EngineError(f"thickness must be in 1 .. {OVERLAY_MAX_THICKNESS}, got {thickness}")
    out = torch.empty_like(images)
    check(_lib.load().mp_draw_boxes(images.data_ptr(), boxes.data_ptr(), image_ids.data_ptr(), boxes.shape[0], colors.data_ptr(), colors.shape[0],
                                    n, h, w, t, out.data_ptr(), _stream()))
    return out


# --------------------------------------------------------------------------- #
# training-free detector (LINE-2D template matching): csrc/template_match.hip
TM_MAX_SIDE = 8192                   # h, w
TM_MAX_T = 8                         # spreading / grid step
TM_MAX_WEAK = 1443                   # weak_threshold
TM_MAX_FEATURES = 63                 # features of one template
TM_MAX_BOX = 256                     # width, height of one template


def _tm_grid(h: int, w: int, T: int) -> Tuple[int, int]:
    if not 1 <= int(T) <= TM_MAX_T:
        raise EngineError(f"T must be in 1 .. {TM_MAX_T}, got {T}")
    return -(-h // T), -(-w // T)


def _tm_sizes(name: str, n: int, h: int, w: int) -> None:
    if not (1 <= h <= TM_MAX_SIDE and 1 <= w <= TM_MAX_SIDE) or n * h * w * 3 >= 2 ** 31:
        raise EngineError(f"{name}: h and w must be in 1 .. {TM_MAX_SIDE} and n * h * w * 3 below 2^31, got n {n}, h {h}, w {w}")


def tm_quantize(images: torch.Tensor, blur: bool = True, weak_threshold: int = 30, with_mag2: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Quantised gradient orientations (mp_tm_quantize).  images uint8 [n,h,w,3] on the device; blur: the binomial (1 4 6 4 1) / 16 first;
    a pixel is a candidate when its squared gradient magnitude is at least weak_threshold^2 -> ori uint8 [n,h,w] (0 or one of eight bits:
    the orientation at least 5 candidates of the 3x3 agree on) and mag2 int32 [n,h,w] (None without with_mag2).  Nothing synchronises."""
    images = _dev_bytes("images", images)
    if images.dim() != 4 or images.shape[3] != 3:
        raise EngineError(f"images must be uint8 [n,h,w,3], got {tuple(images.shape)}")
    n, h, w = (int(v) for v in images.shape[:3])
    _tm_sizes("images", n, h, w)
    weak = int(weak_threshold)
    if not 0 <= weak <= TM_MAX_WEAK:
        raise EngineError(f"weak_threshold must be in 0 .. {TM_MAX_WEAK}, got {weak_threshold}")
    ori = torch.empty((n, h, w), dtype=torch.uint8, device=images.device)
    mag2 = torch.empty((n, h, w), dtype=torch.int32, device=images.device) if with_mag2 else None
    check(_lib.load().mp_tm_quantize(images.data_ptr(), n, h, w, int(bool(blur)), weak, ori.data_ptr(), _ptr(mag2), _stream()))
    return ori, mag2


def tm_response(ori: torch.Tensor, T: int = 8) -> torch.Tensor:
    """Linearised response maps (mp_tm_response).  ori uint8 [n,h,w] of tm_quantize; T in 1 .. 8: the orientations are spread over T x T
    windows and the maps stored for stride-T access -> resp uint8 [n,8,T,T,gh,gw], gh = ceil(h / T), gw = ceil(w / T): the response (4, 1
    or 0) of orientation o at pixel (x, y) sits at [n, o, y mod T, x mod T, y div T, x div T].  Nothing synchronises."""
    ori = _dev_bytes("ori", ori)
    if ori.dim() != 3:
        raise EngineError(f"ori must be uint8 [n,h,w], got {tuple(ori.shape)}")
    n, h, w = (int(v) for v in ori.shape)
    _tm_sizes("ori", n, h, w)
    gh, gw = _tm_grid(h, w, T)
    if n * 8 * T * T * gh * gw >= 2 ** 31:
        raise EngineError(f"the response maps of n {n}, h {h}, w {w}, T {T} have 2^31 bytes or more")
    resp = torch.empty((n, 8, T, T, gh, gw), dtype=torch.uint8, device=ori.device)
    check(_lib.load().mp_tm_response(ori.data_ptr(), n, h, w, int(T), resp.data_ptr(), _stream()))
    return resp


def tm_match(resp: torch.Tensor, h: int, w: int, templates: torch.Tensor, features: torch.Tensor, n_objects: int, host_templates: np.ndarray,
             host_features: np.ndarray) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Every template at every grid location (mp_tm_match).  resp uint8 [n,8,T,T,gh,gw] of tm_response for images of h x w; templates int32
    [n_templates,5] = (object, first feature, n_features, width, height) and features uint8 [n_features,4] = (dx, dy, orientation index, 0)
    on the device, host_templates / host_features the same tables as numpy arrays (validated on the host before the launch) -> best_score,
    best_f uint8 and best_template int32, each [n,n_objects,gh,gw]: the valid template with the largest score / (4 f) at the location
    (the lower index on a tie), or 0, 0, -1.  Nothing synchronises."""
    resp = _dev_bytes("resp", resp)
    if resp.dim() != 6 or resp.shape[1] != 8 or resp.shape[2] != resp.shape[3]:
        raise EngineError(f"resp must be uint8 [n,8,T,T,gh,gw], got {tuple(resp.shape)}")
    n, T = int(resp.shape[0]), int(resp.shape[2])
    h, w, n_objects = int(h), int(w), int(n_objects)
    _tm_sizes("resp", n, h, w)
    gh, gw = _tm_grid(h, w, T)
    if tuple(resp.shape[4:]) != (gh, gw):
        raise EngineError(f"resp {tuple(resp.shape)} is not the maps of images of {h} x {w} at T {T}: gh, gw must be {gh}, {gw}")
    if not 1 <= n_objects <= 65535 or n > 65535 or n * n_objects * gh * gw >= 2 ** 31:
        raise EngineError(f"n_objects must be in 1 .. 65535, n at most 65535 and n * n_objects * gh * gw below 2^31, got n {n}, n_objects {n_objects}")
    templates = _dev_i32(templates)
    features = _dev_bytes("features", features)
    host_templates = np.ascontiguousarray(host_templates, np.int32)
    host_features = np.ascontiguousarray(host_features, np.uint8)
    if templates.dim() != 2 or templates.shape[1] != 5 or features.dim() != 2 or features.shape[1] != 4:
        raise EngineError(f"templates must be int32 [n_templates,5] and features uint8 [n_features,4], got {tuple(templates.shape)}, {tuple(features.shape)}")
    if host_templates.shape != tuple(templates.shape) or host_features.shape != tuple(features.shape):
        raise EngineError(f"the host copies {host_templates.shape}, {host_features.shape} must have the shapes of the tables {tuple(templates.shape)}, {tuple(features.shape)}")
    shape = (n, n_objects, gh, gw)
    best_score = torch.empty(shape, dtype=torch.uint8, device=resp.device)
    best_f = torch.empty(shape, dtype=torch.uint8, device=resp.device)
    best_template = torch.empty(shape, dtype=torch.int32, device=resp.device)
    check(_lib.load().mp_tm_match(resp.data_ptr(), n, h, w, T, templates.data_ptr(), host_templates.ctypes.data, features.data_ptr(),
                                  host_features.ctypes.data, templates.shape[0], features.shape[0], n_objects, best_score.data_ptr(), best_f.data_ptr(),
                                  best_template.data_ptr(), _stream()))
    return best_score, best_f, best_template


# --------------------------------------------------------------------------- #
# points drawn uniformly over mesh surfaces (mesh database): csrc/surface_sample.hip
SURFACE_BLOCK_STEP = 64              # a forced block is a multiple of this ...
SURFACE_MAX_BLOCK = 2048             # ... and at most this; an object has at most this many blocks
SURFACE_MAX_FACES = 1 << 22          # faces of one object


def surface_sample(vertices: torch.Tensor, faces: torch.Tensor, vert_off, face_off, u: torch.Tensor, block: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Points drawn uniformly over the surface of triangle meshes (mp_surface_sample).  vertices [V_total,3] float32 and faces
    [F_total,3] int32 (indices local to the object) on the device; vert_off, face_off [n_obj + 1] (host ints, an array or a tensor: the
    launch needs them on both sides) the prefix arrays that cut them into objects, each object with 1 .. 2^22 faces; u
    [n_obj,count,3] float32 uniforms in [0, 1) on the device (u0 picks the face in proportion to its area, u1 u2 the point in it:
    the engine draws nothing); block = the faces of one job (0: the library's choice; a multiple of 64 up to 2048 forces it, for tests)
    -> points [n_obj,count,3] float32, face [n_obj,count] int32.  No grid, block or arrival order changes a bit.  An object with a
    non-finite coordinate of a referenced vertex, an index outside its vertices, or no area gives NaN points and face -1.  Nothing
    synchronises (a tensor of offsets is read back before the launch)."""
    vertices, faces, u = _dev_f32(vertices), _dev_i32(faces), _dev_f32(u)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise EngineError(f"vertices must be [V_total,3] and faces [F_total,3], got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    if u.dim() != 3 or u.shape[2] != 3 or u.shape[0] < 1 or u.shape[1] < 1:
        raise EngineError(f"u must be [n_obj,count,3] with n_obj, count >= 1, got {tuple(u.shape)}")
    n_obj, count = int(u.shape[0]), int(u.shape[1])
    h_vo, h_fo = (np.ascontiguousarray(o.cpu().numpy() if isinstance(o, torch.Tensor) else o).astype(np.int64) for o in (vert_off, face_off))
    if h_vo.shape != (n_obj + 1,) or h_fo.shape != (n_obj + 1,) or h_vo[0] != 0 or h_fo[0] != 0 or h_vo[-1] != vertices.shape[0] or h_fo[-1] != faces.shape[0]:
        raise EngineError(f"vert_off and face_off must be [n_obj + 1 = {n_obj + 1}], start at 0 and end at {vertices.shape[0]} vertices and {faces.shape[0]} faces")
    if (np.diff(h_vo) < 0).any() or (np.diff(h_fo) < 1).any() or (np.diff(h_fo) > SURFACE_MAX_FACES).any():
        raise EngineError(f"vert_off must not descend, and every object must have 1 .. {SURFACE_MAX_FACES} faces")
    h_vo, h_fo = h_vo.astype(np.int32), h_fo.astype(np.int32)
    dev = vertices.device
    lib = _lib.load()
    n_bytes = lib.mp_surface_sample_scratch_bytes(n_obj, h_fo.ctypes.data, count, int(block))
    if n_bytes == 0:
        raise EngineError(f"surface_sample: block {block} is not 0 or a multiple of {SURFACE_BLOCK_STEP} up to {SURFACE_MAX_BLOCK}, or it cuts an object "
                          f"into more than {SURFACE_MAX_BLOCK} blocks, or too many objects")
    d_vo, d_fo = torch.from_numpy(h_vo).to(dev), torch.from_numpy(h_fo).to(dev)
    ws = _workspace(n_bytes, dev)
    points = torch.empty(n_obj, count, 3, dtype=torch.float32, device=dev)
    face = torch.empty(n_obj, count, dtype=torch.int32, device=dev)
    check(lib.mp_surface_sample(vertices.data_ptr(), faces.data_ptr(), d_vo.data_ptr(), d_fo.data_ptr(), h_vo.ctypes.data, h_fo.ctypes.data, n_obj,
                                u.data_ptr(), count, int(block), ws.data_ptr(), points.data_ptr(), face.data_ptr(), _stream()))
    return points, face


# --------------------------------------------------------------------------- #
def icp_refine(depth_meas: torch.Tensor, im_ids: torch.Tensor, depth_rend: torch.Tensor, K_images: torch.Tensor, K_rows: torch.Tensor,
               TCO: torch.Tensor, n_iterations: int = 100, n_levels: int = 4, tolerance: float = 0.05, n_min_points: int = 1000,
               user_masks: bool = False, association: str = "nn", return_iters: bool = False, masks: Optional[torch.Tensor] = None):
    """-> (TCO_refined [N,4,4], retval [N] int32 (0 ok / -1 input pose kept), residual [N]).  `user_masks`: the caller's masks
    are already applied to depth_meas; the 0.1 m measured-vs-rendered threshold mask is then not used (icp_refiner.py:249-250).
    association: "nn" = the reference's algorithm step for step (mp_icp_refine_nn: get_normal + OpenCV-style nearest-neighbour ICP);
    "projective" = the faster projective-association point-to-plane ICP (mp_icp_refine).  `masks` ("nn" only): the caller's per-frame
    masks [n_images,H,W], passed separately (depth_meas stays unmasked: the reference takes its normals from the whole frame)."""
    lib = _lib.load()
    depth_meas, depth_rend = _dev_f32(depth_meas), _dev_f32(depth_rend)
    K_images, K_rows, TCO = _dev_f32(K_images), _dev_f32(K_rows), _dev_f32(TCO)
    n_im, H, W = depth_meas.shape
    N = TCO.shape[0]
    assert depth_rend.shape == (N, H, W)
    dev = TCO.device
    out = torch.empty_like(TCO)
    retval = torch.empty(N, dtype=torch.int32, device=dev)
    residual = torch.empty(N, dtype=torch.float32, device=dev)
    if association == "nn":
        if user_masks:
            raise ValueError('association="nn" takes the caller\'s masks through `masks`, not pre-multiplied into the depth')
        if masks is not None:
            masks = (masks.to(dev) > 0).to(torch.uint8).contiguous()
            assert masks.shape == depth_meas.shape
        ws = torch.empty(lib.mp_icp_nn_workspace_bytes(n_im, N, H, W), dtype=torch.uint8, device=dev)
        iters = torch.zeros(N, 8, dtype=torch.int32, device=dev) if return_iters else None
        check(lib.mp_icp_refine_nn(depth_meas.data_ptr(), n_im, _dev_i32(im_ids).data_ptr(), depth_rend.data_ptr(), K_images.data_ptr(),
                                   K_rows.data_ptr(), TCO.data_ptr(), N, H, W, n_iterations, n_levels, tolerance, n_min_points, _ptr(masks),
                                   out.data_ptr(), retval.data_ptr(), residual.data_ptr(), _ptr(iters), ws.data_ptr(), ws.numel(), _stream()))
        return (out, retval, residual, iters) if return_iters else (out, retval, residual)
    if association != "projective":
        raise ValueError(f"association must be 'nn' or 'projective', got {association!r}")
    if masks is not None:
        raise ValueError('association="projective" takes masks pre-multiplied into depth_meas (user_masks=True)')
    ws = torch.empty(lib.mp_icp_workspace_bytes(n_im, N, H, W), dtype=torch.uint8, device=dev)
    check(lib.mp_icp_refine(depth_meas.data_ptr(), n_im, _dev_i32(im_ids).data_ptr(), depth_rend.data_ptr(), K_images.data_ptr(),
                            K_rows.data_ptr(), TCO.data_ptr(), N, H, W, n_iterations, n_levels, tolerance, n_min_points, int(user_masks), out.data_ptr(),
                            retval.data_ptr(), residual.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return out, retval, residual


# --------------------------------------------------------------------------- #
TEASER_MAX_POINTS = 1024           # correspondences of one row, at most (the consistency graph is a 1024 x 1024 bit matrix)
TEASER_MASK_TYPES = {"simple": 0, "threshold": 1}
TEASER_SELECTIONS = {"kcore": 0, "none": 1, "max_clique": 2}
TEASER_TIM_GRAPHS = {"chain": 0, "complete": 1}
TEASER_INFO = ("N", "M", "n_selected", "gnc_iterations", "num_inliers")
TEASER_CLIQUE_INFO = ("size", "upper_bound", "exact", "steps")


def _teaser_mode(name: str, table: Dict[str, int], value: str) -> int:
    if value not in table:
        raise EngineError(f"{name} must be one of {sorted(table)}, got {value!r}")
    return table[value]


def farthest_point_sample(points: torch.Tensor, counts: torch.Tensor, n_points: int, use_fps: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Farthest point sampling of point sets (mp_fps).  points [n,stride,3] float32 and counts [n] int32 on the device (the first
    counts[r] points of row r are valid) -> idx [n,n_points] int32 (-1 past M = min(n_points, count)), M [n] int32.  Pick 0 is point 0,
    every later pick the point with the largest running minimum of the squared fp32 distance to the picks so far, a tie to the lowest
    index; use_fps=False takes index floor(k * count / M)."""
    points, counts = _dev_f32(points), _dev_i32(counts)
    if points.dim() != 3 or points.shape[2] != 3 or points.shape[1] < 1 or counts.shape != (points.shape[0],) or int(n_points) < 1:
        raise EngineError(f"points must be [n,stride >= 1,3], counts [n] and n_points >= 1, got {tuple(points.shape)}, {tuple(counts.shape)}, {n_points}")
    n, stride = int(points.shape[0]), int(points.shape[1])
    lib = _lib.load()
    ws = _workspace(lib.mp_fps_workspace_bytes(n, stride), points.device)
    idx = torch.empty(n, int(n_points), dtype=torch.int32, device=points.device)
    m = torch.empty(n, dtype=torch.int32, device=points.device)
    check(lib.mp_fps(points.data_ptr(), counts.data_ptr(), n, stride, int(n_points), int(bool(use_fps)), idx.data_ptr(), m.data_ptr(), ws.data_ptr(),
                     ws.numel(), _stream()))
    return idx, m


def max_clique_step_limits() -> Tuple[int, int]:
    """(the default step budget of the maximum-clique search, the largest budget an argument may ask for)"""
    default = int(_lib.load().mp_max_clique_default_steps())
    return default, 16 * default


def _clique_steps(max_steps: Optional[int]) -> int:
    default, ceiling = max_clique_step_limits()
    if max_steps is None:
        return default
    if not 0 <= int(max_steps) <= ceiling:
        raise EngineError(f"the step budget of the maximum-clique search must be 0 .. {ceiling}, got {max_steps}")
    return int(max_steps)


def max_clique(adjacency: torch.Tensor, counts: Optional[torch.Tensor] = None, max_steps: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The exact maximum clique of graphs given as adjacency matrices (mp_max_clique; the rule is in csrc/teaser_clique_core.h).
    adjacency [n,stride <= 1024,stride] (any dtype; non-zero = set; an edge exists when i != j and a[i][j] or a[j][i]), counts [n] int32
    = the vertices of every row (None: stride) -> members [n,stride] int32 in ascending order (-1 past the size), info [n,4] int32 =
    TEASER_CLIQUE_INFO: exact = 0 when the search coloured more than max_steps vertices (None: the default budget) and returns the best
    clique found until then."""
    if adjacency.dim() != 3 or adjacency.shape[1] != adjacency.shape[2] or not 1 <= adjacency.shape[1] <= TEASER_MAX_POINTS:
        raise EngineError(f"adjacency must be [n,stride,stride] with stride 1 .. {TEASER_MAX_POINTS}, got {tuple(adjacency.shape)}")
    steps = _clique_steps(max_steps)
    adj = _dev(adjacency != 0, torch.uint8)
    n, stride, dev = int(adj.shape[0]), int(adj.shape[1]), adj.device
    if counts is not None:
        counts = _dev_i32(counts)
        if counts.shape != (n,):
            raise EngineError(f"counts must be [{n}], got {tuple(counts.shape)}")
    lib = _lib.load()
    ws = _workspace(lib.mp_max_clique_workspace_bytes(n, stride), dev)
    members = torch.empty(n, stride, dtype=torch.int32, device=dev)
    info = torch.empty(n, len(TEASER_CLIQUE_INFO), dtype=torch.int32, device=dev)
    check(lib.mp_max_clique(adj.data_ptr(), _ptr(counts), n, stride, steps, members.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return members, info


def _teaser_telemetry(n: int, stride: int, device, want: bool):
    if not want:
        return None, None, None, None
    return tuple(torch.full((n, stride), -1, dtype=torch.int32, device=device) for _ in range(3)) + (torch.zeros(n, len(TEASER_INFO), dtype=torch.int32, device=device),)


def _clique_info(n: int, device, want: bool):
    return torch.zeros(n, len(TEASER_CLIQUE_INFO), dtype=torch.int32, device=device) if want else None


def teaser_solve(src: torch.Tensor, dst: torch.Tensor, counts: torch.Tensor, noise_bound: float = 0.01, min_num_inliers: int = 0,
                 inlier_selection: str = "kcore", rotation_tim_graph: str = "chain", telemetry: bool = False, max_clique_steps: Optional[int] = None):
    """Robust registration of given correspondences (mp_teaser_solve_ex; the rules are in csrc/teaser_core.h).  src, dst [n,stride <= 1024,3]
    float32, counts [n] int32 on the device -> Rt [n,3,4] float64 with dst ~ R src + t, retval [n] int32 (0 when num_inliers >=
    min_num_inliers, else -1); with telemetry also a dict of degree, core, selected [n,stride] (-1 past a row's count) and info
    [n,5] = TEASER_INFO.  inlier_selection "max_clique" selects an exact maximum clique of the consistency graph under the step budget
    max_clique_steps (None: the default; see max_clique); the telemetry dict then also holds clique [n,4] = TEASER_CLIQUE_INFO."""
    src, dst, counts = _dev_f32(src), _dev_f32(dst), _dev_i32(counts)
    if src.dim() != 3 or src.shape[2] != 3 or dst.shape != src.shape or not 1 <= src.shape[1] <= TEASER_MAX_POINTS or counts.shape != (src.shape[0],):
        raise EngineError(f"src and dst must be [n,1 .. {TEASER_MAX_POINTS},3] and counts [n], got {tuple(src.shape)}, {tuple(dst.shape)}, {tuple(counts.shape)}")
    sel, graph = _teaser_mode("inlier_selection", TEASER_SELECTIONS, inlier_selection), _teaser_mode("rotation_tim_graph", TEASER_TIM_GRAPHS, rotation_tim_graph)
    n, stride, dev = int(src.shape[0]), int(src.shape[1]), src.device
    lib = _lib.load()
    steps = _clique_steps(max_clique_steps)
    ws = _workspace(lib.mp_teaser_workspace_bytes_ex(n, 0, 0, stride, sel), dev)
    Rt = torch.empty(n, 3, 4, dtype=torch.float64, device=dev)
    retval = torch.empty(n, dtype=torch.int32, device=dev)
    degree, core, selected, info = _teaser_telemetry(n, stride, dev, telemetry)
    clique = _clique_info(n, dev, telemetry and inlier_selection == "max_clique")
    check(lib.mp_teaser_solve_ex(src.data_ptr(), dst.data_ptr(), counts.data_ptr(), n, stride, float(noise_bound), sel, graph, int(min_num_inliers),
                                 Rt.data_ptr(), retval.data_ptr(), _ptr(degree), _ptr(core), _ptr(selected), _ptr(info), steps, _ptr(clique), ws.data_ptr(),
                                 ws.numel(), _stream()))
    if not telemetry:
        return Rt, retval
    tel = dict(degree=degree, core=core, selected=selected, info=info)
    if clique is not None:
        tel["clique"] = clique
    return Rt, retval, tel


def teaser_refine(depth_meas: torch.Tensor, im_ids: torch.Tensor, depth_rend: torch.Tensor, K_rows: torch.Tensor, TCO: torch.Tensor,
                  mask_type: str = "simple", depth_delta_thresh: float = 0.1, n_min_points: int = 100, n_points: int = 1000,
                  noise_bound: float = 0.01, min_num_inliers: int = 50, use_farthest_point_sampling: bool = True,
                  inlier_selection: str = "kcore", rotation_tim_graph: str = "chain", telemetry: bool = False, max_clique_steps: Optional[int] = None):
    """The TEASER++ depth refiner from depth frames (mp_teaser_refine_ex): depth_meas [B,H,W], im_ids [N], depth_rend [N,H,W] rendered at
    TCO [N,4,4], K_rows [N,3,3] -> (TCO_refined [N,4,4], retval [N] int32 (0 refined / -1 input pose kept), info [N,5] int32 =
    TEASER_INFO); with telemetry also a dict of Rt [N,3,4] float64, sample_idx [N,n_points] and degree, core, selected [N,n_points],
    and with inlier_selection "max_clique" (budget max_clique_steps, as teaser_solve) clique [N,4] = TEASER_CLIQUE_INFO."""
    depth_meas, depth_rend, K_rows, TCO, im_ids = _dev_f32(depth_meas), _dev_f32(depth_rend), _dev_f32(K_rows), _dev_f32(TCO), _dev_i32(im_ids)
    if depth_meas.dim() != 3 or TCO.dim() != 3 or TCO.shape[1:] != (4, 4):
        raise EngineError(f"depth_meas must be [B,H,W] and TCO [N,4,4], got {tuple(depth_meas.shape)} and {tuple(TCO.shape)}")
    n_im, H, W = (int(v) for v in depth_meas.shape)
    N, dev = int(TCO.shape[0]), TCO.device
    if depth_rend.shape != (N, H, W) or K_rows.shape != (N, 3, 3) or im_ids.shape != (N,):
        raise EngineError(f"depth_rend must be [{N},{H},{W}], K_rows [{N},3,3], im_ids [{N}]")
    if not 1 <= int(n_points) <= TEASER_MAX_POINTS:
        raise EngineError(f"n_points must be 1 .. {TEASER_MAX_POINTS}, got {n_points}")
    mask = _teaser_mode("mask_type", TEASER_MASK_TYPES, mask_type)
    sel, graph = _teaser_mode("inlier_selection", TEASER_SELECTIONS, inlier_selection), _teaser_mode("rotation_tim_graph", TEASER_TIM_GRAPHS, rotation_tim_graph)
    lib = _lib.load()
    steps = _clique_steps(max_clique_steps)
    ws = _workspace(lib.mp_teaser_workspace_bytes_ex(N, H, W, int(n_points), sel), dev)
    out = torch.empty_like(TCO)
    retval = torch.empty(N, dtype=torch.int32, device=dev)
    degree, core, selected, _ = _teaser_telemetry(N, int(n_points), dev, telemetry)
    info = torch.zeros(N, len(TEASER_INFO), dtype=torch.int32, device=dev)
    Rt = torch.empty(N, 3, 4, dtype=torch.float64, device=dev) if telemetry else None
    sample_idx = torch.empty(N, int(n_points), dtype=torch.int32, device=dev) if telemetry else None
    clique = _clique_info(N, dev, telemetry and inlier_selection == "max_clique")
    check(lib.mp_teaser_refine_ex(depth_meas.data_ptr(), n_im, im_ids.data_ptr(), depth_rend.data_ptr(), K_rows.data_ptr(), TCO.data_ptr(), N, H, W, mask,
                                  float(depth_delta_thresh), int(n_min_points), int(n_points), float(noise_bound), int(min_num_inliers),
                                  int(bool(use_farthest_point_sampling)), sel, graph, out.data_ptr(), retval.data_ptr(), _ptr(Rt), _ptr(sample_idx),
                                  _ptr(degree), _ptr(core), _ptr(selected), info.data_ptr(), steps, _ptr(clique), ws.data_ptr(), ws.numel(), _stream()))
    if not telemetry:
        return out, retval, info
    tel = dict(Rt=Rt, sample_idx=sample_idx, degree=degree, core=core, selected=selected)
    if clique is not None:
        tel["clique"] = clique
    return out, retval, info, tel


# --------------------------------------------------------------------------- #
class DetectorNet(_Handle):
    """mp_detector: the Mask R-CNN (ResNet-50 + FPN) detection graph resident on the device, one call per image batch
    (csrc/detector.hip).  `state_dict` uses torchvision's keys (= a checkpoint of the reference's DetectorMaskRCNN)."""
    _destroy = "mp_detector_destroy"

    def __init__(self, state_dict: Dict[str, torch.Tensor], n_classes: int, min_size: int, max_size: int, **overrides):
        lib = _lib.load()
        self.cfg = _lib.DetectorConfig()
        check(lib.mp_detector_default_config(C.byref(self.cfg), n_classes, min_size, max_size))
        for k, v in overrides.items():
            if not hasattr(self.cfg, k):
                raise EngineError(f"unknown detector option '{k}'")
            cur = getattr(self.cfg, k)
            if hasattr(cur, "__len__"):
                cur[:] = list(v)
            else:
                setattr(self.cfg, k, v)
        arr, items = _named_tensors(state_dict)   # (`items` owns what `arr` points into)
        h = C.c_void_p()
        check(lib.mp_detector_create(C.byref(self.cfg), arr, len(items), C.byref(h)))
        self.handle = h
        self.n_classes = n_classes
        self._ws: Optional[torch.Tensor] = None

    @staticmethod
    def state_spec(n_classes: int) -> List[Tuple[str, Tuple[int, ...]]]:
        """[(state_dict key, shape)] the detector expects (host only: mp_detector_state_spec)"""
        lib = _lib.load()
        out, i = [], 0
        while True:
            name = C.create_string_buffer(160)
            shp, nd = (C.c_int64 * 4)(), C.c_int32(0)
            rc = lib.mp_detector_state_spec(n_classes, i, name, 160, shp, C.byref(nd))
            if rc == 1:
                return out
            check(rc)
            out.append((name.value.decode(), tuple(int(s) for s in shp[: nd.value])))
            i += 1

    def forward(self, images: torch.Tensor, with_masks: bool = True):
        """images [n,3,H,W] fp32 in [0,1] on the GPU -> (boxes [n,D,4], scores [n,D], labels [n,D] int32, counts [n] int32,
        masks [n,D,H,W] or None); nothing synchronises, entries past counts[i] are zero."""
        lib = _lib.load()
        images = _dev_f32(images)
        n, c, H, W = images.shape
        if c != 3:
            raise EngineError("the detector takes RGB images [n,3,H,W]")
        dev = images.device
        D = int(self.cfg.box_detections_per_img)
        need = lib.mp_detector_workspace_bytes(self.handle, n, H, W)
        if need == 0:
            raise EngineError(f"mp_detector_workspace_bytes failed for {n} x {H} x {W}: {lib.mp_last_error().decode()}")
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        boxes = torch.empty(n, D, 4, dtype=torch.float32, device=dev)
        scores = torch.empty(n, D, dtype=torch.float32, device=dev)
        labels = torch.empty(n, D, dtype=torch.int32, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        masks = torch.empty(n, D, H, W, dtype=torch.float32, device=dev) if with_masks else None
        check(lib.mp_detector_forward(self.handle, images.data_ptr(), n, H, W, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                                      counts.data_ptr(), _ptr(masks), self._ws.data_ptr(), self._ws.numel(), _stream()))
        return boxes, scores, labels, counts, masks

    def debug_buffer(self, what: str):
        """the WHOLE buffer behind a tap of the last forward, borders and row padding included -> (flat tensor, shape4, border,
        row_stride).  The tensor is a VIEW of the workspace (the next forward overwrites it), int32 for the two count taps (the C entry
        has no slot for the element type), else float32."""
        lib = _lib.load()
        ptr, shp, border, rs, n_el = C.c_void_p(), (C.c_int64 * 4)(), C.c_int32(0), C.c_int64(0), C.c_int64(0)
        check(lib.mp_detector_debug_tensor(self.handle, what.encode(), C.byref(ptr), shp, C.byref(border), C.byref(rs), C.byref(n_el)))
        off = ptr.value - self._ws.data_ptr()
        if off < 0 or off + 4 * n_el.value > self._ws.numel():
            raise EngineError(f"debug tap '{what}' lies outside the workspace of the last forward")
        dt = torch.int32 if what in ("proposal_counts", "f_cnt") else torch.float32
        return self._ws[off : off + 4 * n_el.value].view(dt), [int(v) for v in shp], border.value, rs.value

    def debug_tensor(self, what: str) -> torch.Tensor:
        """a COPY of an intermediate of the last forward (parity tests): padded maps come back as their [n,h,w,c] interior.
        Taps: "x0", "pool", "C2".."C5", "L2".."L5", "P2".."P6", "keys", "proposals", "proposal_scores", "proposal_counts", "roi7", "class_logits",
        "f_cnt", "det_resized", "roi14", "mask_logits" (shapes: mp_detector_debug_tensor in include/mp_engine.h)"""
        flat, s, b, rs = self.debug_buffer(what)
        flat = flat.clone()
        if b:
            return flat.view(s[0], s[1] + 2 * b, s[2] + 2 * b, s[3])[:, b : b + s[1], b : b + s[2]].contiguous()
        if s[2] == 4:
            return flat.view(s[0], s[1], 4)
        if rs > 1:
            return flat.view(s[0], rs)[:, : s[1]].contiguous()
        return flat.view(s[0], s[1])
