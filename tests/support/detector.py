"""Shared pieces of the detector stage tests (tests/test_gpu_zz_detector_stages.py): reading the engine's debug taps (padded NHWC maps,
row matrices whose rows are padded past their logical width), the layout conversions the oracle (oracle/mask_rcnn.py) needs, and a
rank-for-rank matcher of selection results that tolerates only counted, near-tied exceptions."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional, Sequence

import numpy as np
import torch


def nhwc_to_nchw(t: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """[n, h, w, c] (a debug tap's interior) -> contiguous [n, c, h, w] on the CPU"""
    return t.detach().cpu().permute(0, 3, 1, 2).contiguous().to(dtype)


def raw_debug(net, what: str):
    """the WHOLE buffer behind a debug tap, borders and row padding included -> (flat CPU tensor, shape4, border, row_stride).
    DetectorNet.debug_tensor returns the logical view only; this one lets a test check what lies outside it (zero borders, zero pad
    columns of the padded row matrices)."""
    from megapose6d_amd import _lib
    from megapose6d_amd._lib import check

    lib = _lib.load()
    ptr, shp, border, rs, n_el = C.c_void_p(), (C.c_int64 * 4)(), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    check(lib.mp_detector_debug_tensor(net.handle, what.encode(), C.byref(ptr), shp, C.byref(border), C.byref(rs), C.byref(n_el)))
    off = ptr.value - net._ws.data_ptr()
    assert off >= 0 and off + 4 * n_el.value <= net._ws.numel()
    dt = torch.int32 if what in ("proposal_counts", "f_cnt") else torch.float32
    flat = net._ws[off : off + 4 * n_el.value].view(dt).cpu().clone()
    return flat, [int(v) for v in shp], border.value, rs.value


def debug_rows(net, what: str) -> torch.Tensor:
    """a row-matrix tap ("class_logits", "mask_logits") as [rows, row_stride]: every row in full, the pad columns past the logical
    width included"""
    flat, shp, border, rs = raw_debug(net, what)
    assert border == 0 and rs >= shp[1], (what, shp, rs)
    return flat.view(shp[0], rs)


def mask_logits_28(rows: torch.Tensor, n_det: int) -> torch.Tensor:
    """mask_logits rows [n_det * 14 * 14 * 4, Cs] -> [n_det, Cs, 28, 28].  Row ((det * 14 + y) * 14 + x) * 4 + a * 2 + b holds mask pixel
    (2 y + a, 2 x + b): the 2x2 stride-2 transposed convolution runs as a 1x1 convolution onto 4 sub-pixel channel groups."""
    cs = rows.shape[1]
    t = rows.reshape(n_det, 14, 14, 2, 2, cs).permute(0, 5, 1, 3, 2, 4)   # det, c, y, a, x, b
    return t.reshape(n_det, cs, 28, 28)


def iou_f32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """pairwise IoU [len(a), len(b)] in float32 with torchvision's nms_kernel operation order (the order det_nms_kernel uses)"""
    a, b = a.astype(np.float32), b.astype(np.float32)
    w = np.maximum(np.float32(0), np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]))
    h = np.maximum(np.float32(0), np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]))
    inter = w * h
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area_a[:, None] + area_b[None, :] - inter)


def match_ranked(same: Callable[[int, int], bool], n_got: int, ref_keys: Sequence[float], eps: float,
                 got_keys: Optional[Sequence[float]] = None):
    """Rank-for-rank comparison of a selection result (got) with the oracle's (ref).  `same(i, j)`: got entry i is ref entry j.
    Position i must hold ref entry i, with two exceptions, each counted:
      * a neighbour swap: got[i], got[i + 1] = ref[i + 1], ref[i] where the ref keys of the pair differ by less than eps;
      * the cut: the last position holds another entry whose key (got_keys) is within eps of the ref entry's key.
    eps = 0 admits no exception.  -> (n_exceptions, None) or (n_exceptions, message of the first mismatch)"""
    n_ref = len(ref_keys)
    if n_got != n_ref:
        return 0, f"{n_got} entries, the oracle has {n_ref}"
    exc, i = 0, 0
    while i < n_ref:
        if same(i, i):
            i += 1
        elif i + 1 < n_ref and same(i, i + 1) and same(i + 1, i) and abs(float(ref_keys[i]) - float(ref_keys[i + 1])) < eps:
            exc += 1
            i += 2
        elif i == n_ref - 1 and got_keys is not None and abs(float(got_keys[i]) - float(ref_keys[i])) < eps:
            exc += 1
            i += 1
        else:
            return exc, f"rank {i} of {n_ref}: not the oracle's entry (ref key {float(ref_keys[i])!r})"
    return exc, None
